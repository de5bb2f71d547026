// bvh_closest.cpp — crthip_bvh_closest: the host side of K-CLOSEST (include/corto_hip.h has the contract, bvh_closest.h the kernel's source).
// The call checks every set, writes the job table - a ClosestJob a set with points, then the block_start words - into a pinned block the
// context owns, sends it up in ONE copy and launches k_bvh_closest once, all on the context's main stream.
//
//   order    bvh_cast.cpp's: everything a decode enqueues that the query reads - the BVH's finishers, the quantised stores with their device
//            transform records, whatever made the index final - ends on ctx->stream, so the query goes there, behind it; no event, no host
//            wait.  crthip_ctx_sync waits for that stream.
//   blocks   the context's own (ctx->closest), apart from the cast's and the box query's, so that their files are as they were: two slots of
//            {pinned block, device block, event}, taken in turn.  A slot's event is recorded behind the launch that read it; the call that
//            takes the slot again waits for that event first, so neither a pending upload nor a running kernel ever has its table
//            overwritten.  Nothing is allocated once the blocks have grown.
#include "batch_internal.h"
#include "pool_internal.h"
#include "bvh_closest.h"

struct ClosestState {
	struct Slot { PinnedBuf pin; DeviceBuf dev; hipEvent_t ev = nullptr; bool pending = false; } slot[2];
	uint32_t next = 0;
};

void closest_state_release(crthip_ctx *ctx) {
	if(!ctx->closest) return;
	for(ClosestState::Slot &s : ctx->closest->slot) { s.pin.release(); s.dev.release(); if(s.ev) (void)hipEventDestroy(s.ev); }
	delete ctx->closest;
	ctx->closest = nullptr;
}

extern "C" int crthip_bvh_closest(crthip_ctx *ctx, uint32_t nsets, const crthip_bvh_closest_set *sets) {
	if(!ctx) return fail(CRTHIP_E_ARGUMENT, "crthip_bvh_closest: ctx is NULL");
	if(nsets && !sets) return fail(CRTHIP_E_ARGUMENT, "crthip_bvh_closest: sets is NULL");
	if(!nsets) return CRTHIP_OK;
	HIP_TRY(hipSetDevice(ctx->device));
	uint32_t njobs = 0;
	uint64_t nblocks = 0;
	for(uint32_t k = 0; k < nsets; k++) {
		const crthip_bvh_closest_set &s = sets[k];
		auto bad = [&](const char *why) { return fail(CRTHIP_E_ARGUMENT, "crthip_bvh_closest: set " + std::to_string(k) + ": " + why); };
		if(const char *why = bvh_closest_set_error(&s)) return bad(why);
		if(!s.npoint) continue;
		const uint32_t esize = s.index_format == CRTHIP_FMT_UINT16 ? 2u : 4u;
		const int dev = ctx->device;
		if(!resident_array_ok(s.nodes, (uint64_t)(2u*s.nface - 1u)*32, 16, dev)) return bad("nodes is not device memory of the context's device, or leaves its allocation");
		if(!resident_array_ok(s.position, bvh_closest_position_bytes(&s), 2, dev)) return bad("position is not device memory of the context's device, or leaves its allocation");
		if(!resident_array_ok(s.index, (uint64_t)s.nface*3*esize, esize, dev)) return bad("index is not device memory of the context's device, or leaves its allocation");
		if(s.transform && !resident_array_ok(s.transform, sizeof(crthip_quant_transform), 16, dev)) return bad("transform is not device memory of the context's device, or leaves its allocation");
		if(!resident_array_ok(s.points, (uint64_t)s.npoint*16, 16, dev)) return bad("points is not device memory of the context's device, or leaves its allocation");
		if(!resident_array_ok(s.hits, (uint64_t)s.npoint*48, 16, dev)) return bad("hits is not device memory of the context's device, or leaves its allocation");
		njobs++;
		nblocks += ((uint64_t)s.npoint + CAST_THREADS - 1)/CAST_THREADS;
	}
	if(nblocks > 0x7FFFFFFFull) return fail(CRTHIP_E_LIMIT, "crthip_bvh_closest: more than 2^31 - 1 workgroups of 64 points");
	if(!njobs) return CRTHIP_OK;

	if(!ctx->closest) ctx->closest = new (std::nothrow) ClosestState();
	if(!ctx->closest) return fail(CRTHIP_E_NOMEM);
	ClosestState::Slot &slot = ctx->closest->slot[ctx->closest->next];
	if(!slot.ev) HIP_TRY(hipEventCreateWithFlags(&slot.ev, hipEventDisableTiming));
	if(slot.pending) { HIP_TRY(hipEventSynchronize(slot.ev)); slot.pending = false; }   // (the call before the last one: its table is free again)
	const size_t start_off = (size_t)njobs*sizeof(ClosestJob), bytes = start_off + ((size_t)njobs + 1)*4;
	if(slot.pin.reserve(bytes) != CRTHIP_OK || slot.dev.reserve(bytes) != CRTHIP_OK) return fail(CRTHIP_E_NOMEM);
	ClosestJob *jobs = (ClosestJob *)slot.pin.p;
	uint32_t *block_start = (uint32_t *)((uint8_t *)slot.pin.p + start_off);
	uint32_t j = 0, b = 0;
	for(uint32_t k = 0; k < nsets; k++) {
		const crthip_bvh_closest_set &s = sets[k];
		if(!s.npoint) continue;
		ClosestJob &J = jobs[j];
		J.nodes = s.nodes; J.position = s.position; J.index = s.index; J.transform = s.transform; J.points = s.points; J.hits = s.hits;
		for(int c = 0; c < 3; c++) J.base[c] = s.base[c];
		J.pos_stride = bvh_closest_stride(&s);
		J.nvert = s.nvert; J.nface = s.nface; J.index_u16 = s.index_format == CRTHIP_FMT_UINT16; J.npoint = s.npoint;
		J.flags = s.flags; J.pad[0] = J.pad[1] = J.pad[2] = 0;
		block_start[j++] = b;
		b += (uint32_t)(((uint64_t)s.npoint + CAST_THREADS - 1)/CAST_THREADS);
	}
	block_start[j] = b;
	HIP_TRY(hipMemcpyAsync(slot.dev.p, slot.pin.p, bytes, hipMemcpyHostToDevice, ctx->stream));
	hipLaunchKernelGGL(k_bvh_closest, dim3(b), dim3(CAST_THREADS), 0, ctx->stream, (const ClosestJob *)slot.dev.p,
		(const uint32_t *)((const uint8_t *)slot.dev.p + start_off), njobs);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipEventRecord(slot.ev, ctx->stream));
	slot.pending = true;
	ctx->closest->next ^= 1u;
	return CRTHIP_OK;
}
