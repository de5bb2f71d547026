// bvh_query.cpp — crthip_bvh_query: the host side of K-QUERY (include/corto_hip.h has the contract, bvh_query.h the kernel's source).  The call
// checks every set, writes the job table - a QueryJob a set with boxes, then the block_start words - into a pinned block the context owns,
// sends it up in ONE copy and launches k_bvh_query once, all on the context's main stream.
//
//   order    bvh_cast.cpp's: everything a decode enqueues that the query reads - the BVH's finishers, the quantised stores with their device
//            transform records, whatever made the index final - ends on ctx->stream, so the query goes there, behind it; no event, no host
//            wait.  crthip_ctx_sync waits for that stream.
//   blocks   the context's own (ctx->query), apart from the cast's, so that bvh_cast.cpp is as it was: two slots of {pinned block, device
//            block, event}, taken in turn.  A slot's event is recorded behind the launch that read it; the call that takes the slot again
//            waits for that event first, so neither a pending upload nor a running kernel ever has its table overwritten.  Nothing is
//            allocated once the blocks have grown.
#include "batch_internal.h"
#include "pool_internal.h"
#include "bvh_query.h"

struct QueryState {
	struct Slot { PinnedBuf pin; DeviceBuf dev; hipEvent_t ev = nullptr; bool pending = false; } slot[2];
	uint32_t next = 0;
};

void query_state_release(crthip_ctx *ctx) {
	if(!ctx->query) return;
	for(QueryState::Slot &s : ctx->query->slot) { s.pin.release(); s.dev.release(); if(s.ev) (void)hipEventDestroy(s.ev); }
	delete ctx->query;
	ctx->query = nullptr;
}

extern "C" int crthip_bvh_query(crthip_ctx *ctx, uint32_t nsets, const crthip_bvh_query_set *sets) {
	if(!ctx) return fail(CRTHIP_E_ARGUMENT, "crthip_bvh_query: ctx is NULL");
	if(nsets && !sets) return fail(CRTHIP_E_ARGUMENT, "crthip_bvh_query: sets is NULL");
	if(!nsets) return CRTHIP_OK;
	HIP_TRY(hipSetDevice(ctx->device));
	uint32_t njobs = 0;
	uint64_t nblocks = 0;
	for(uint32_t k = 0; k < nsets; k++) {
		const crthip_bvh_query_set &s = sets[k];
		auto bad = [&](const char *why) { return fail(CRTHIP_E_ARGUMENT, "crthip_bvh_query: set " + std::to_string(k) + ": " + why); };
		if(const char *why = bvh_query_set_error(&s)) return bad(why);
		if(!s.nbox) continue;
		const uint32_t esize = s.index_format == CRTHIP_FMT_UINT16 ? 2u : 4u;
		const uint32_t cap = bvh_query_capacity(&s);
		const int dev = ctx->device;
		if(!resident_array_ok(s.nodes, (uint64_t)(2u*s.nface - 1u)*32, 16, dev)) return bad("nodes is not device memory of the context's device, or leaves its allocation");
		if(!resident_array_ok(s.position, bvh_query_position_bytes(&s), 2, dev)) return bad("position is not device memory of the context's device, or leaves its allocation");
		if(!resident_array_ok(s.index, (uint64_t)s.nface*3*esize, esize, dev)) return bad("index is not device memory of the context's device, or leaves its allocation");
		if(s.transform && !resident_array_ok(s.transform, sizeof(crthip_quant_transform), 16, dev)) return bad("transform is not device memory of the context's device, or leaves its allocation");
		if(!resident_array_ok(s.boxes, (uint64_t)s.nbox*32, 16, dev)) return bad("boxes is not device memory of the context's device, or leaves its allocation");
		if(!resident_array_ok(s.results, (uint64_t)s.nbox*16, 16, dev)) return bad("results is not device memory of the context's device, or leaves its allocation");
		// (nbox*face_capacity*4 stays below 2^64 only while the words stay below 2^62: both factors are below 2^32)
		if(cap && ((uint64_t)s.nbox*cap > (1ull << 61) || !resident_array_ok(s.faces, (uint64_t)s.nbox*cap*4, 4, dev)))
			return bad("faces is not device memory of the context's device, or leaves its allocation");
		njobs++;
		nblocks += ((uint64_t)s.nbox + CAST_THREADS - 1)/CAST_THREADS;
	}
	if(nblocks > 0x7FFFFFFFull) return fail(CRTHIP_E_LIMIT, "crthip_bvh_query: more than 2^31 - 1 workgroups of 64 boxes");
	if(!njobs) return CRTHIP_OK;

	if(!ctx->query) ctx->query = new (std::nothrow) QueryState();
	if(!ctx->query) return fail(CRTHIP_E_NOMEM);
	QueryState::Slot &slot = ctx->query->slot[ctx->query->next];
	if(!slot.ev) HIP_TRY(hipEventCreateWithFlags(&slot.ev, hipEventDisableTiming));
	if(slot.pending) { HIP_TRY(hipEventSynchronize(slot.ev)); slot.pending = false; }   // (the query before the last one: its table is free again)
	const size_t start_off = (size_t)njobs*sizeof(QueryJob), bytes = start_off + ((size_t)njobs + 1)*4;
	if(slot.pin.reserve(bytes) != CRTHIP_OK || slot.dev.reserve(bytes) != CRTHIP_OK) return fail(CRTHIP_E_NOMEM);
	QueryJob *jobs = (QueryJob *)slot.pin.p;
	uint32_t *block_start = (uint32_t *)((uint8_t *)slot.pin.p + start_off);
	uint32_t j = 0, b = 0;
	for(uint32_t k = 0; k < nsets; k++) {
		const crthip_bvh_query_set &s = sets[k];
		if(!s.nbox) continue;
		QueryJob &J = jobs[j];
		J.nodes = s.nodes; J.position = s.position; J.index = s.index; J.transform = s.transform; J.boxes = s.boxes; J.results = s.results;
		J.face_capacity = bvh_query_capacity(&s);
		J.faces = J.face_capacity ? s.faces : nullptr; J.pad0 = 0;
		for(int c = 0; c < 3; c++) J.base[c] = s.base[c];
		J.pos_stride = bvh_query_stride(&s);
		J.nvert = s.nvert; J.nface = s.nface; J.index_u16 = s.index_format == CRTHIP_FMT_UINT16; J.nbox = s.nbox;
		J.flags = s.flags; J.pad[0] = J.pad[1] = 0;
		block_start[j++] = b;
		b += (uint32_t)(((uint64_t)s.nbox + CAST_THREADS - 1)/CAST_THREADS);
	}
	block_start[j] = b;
	HIP_TRY(hipMemcpyAsync(slot.dev.p, slot.pin.p, bytes, hipMemcpyHostToDevice, ctx->stream));
	hipLaunchKernelGGL(k_bvh_query, dim3(b), dim3(CAST_THREADS), 0, ctx->stream, (const QueryJob *)slot.dev.p,
		(const uint32_t *)((const uint8_t *)slot.dev.p + start_off), njobs);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipEventRecord(slot.ev, ctx->stream));
	slot.pending = true;
	ctx->query->next ^= 1u;
	return CRTHIP_OK;
}
