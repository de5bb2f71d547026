// batch.cpp — host side of the MI355X decode path: context (stream, scratch pool), batch planner
// (walk -> job descriptors -> one H2D upload) and the kernel schedule.  Compiled by hipcc.
//
// The schedule restates the stage order of crt::Decoder::decodeMesh / decodePointCloud
// (src/decoder.cpp:133-196) for a whole batch of blobs at once:
//   decode-all (Tunstall + bit-unpack) -> topology -> delta-all -> postDelta (normals) -> dequantize-all.
#include "batch_internal.h"
#include "crt_walk.h"
#include "pool_internal.h"

// (the thread's last error, crthip_strerror and crthip_probe are host_probe.cpp's: no HIP there)
extern "C" uint32_t crthip_abi_version(void) { return CRTHIP_ABI_VERSION; }

// ------------------------------------------------------------------------------------------------
// host-only probes
// key\0value\0... into out when it fits; the bytes needed
static int64_t flat_pairs(const std::vector<std::pair<std::string, std::string>> &kvs, char *out, size_t cap) {
	std::string flat;
	for(auto &kv : kvs) { flat += kv.first; flat.push_back('\0'); flat += kv.second; flat.push_back('\0'); }
	if(out && cap >= flat.size()) memcpy(out, flat.data(), flat.size());
	return (int64_t)flat.size();
}

extern "C" int64_t crthip_probe_exif(const uint8_t *blob, size_t len, char *out, size_t cap) {
	BlobHeader h;
	int err = parse_header(blob, len, h);
	if(err) return fail(err);
	return flat_pairs(h.exif, out, cap);
}

extern "C" int64_t crthip_probe_groups(const uint8_t *blob, size_t len, uint32_t *group_end, size_t cap) {
	BlobLayout L;
	int err = walk_blob(blob, len, L);
	if(err) return fail(err);
	for(size_t i = 0; i < L.group_end.size() && i < cap; i++) group_end[i] = L.group_end[i];
	return (int64_t)L.group_end.size();
}

extern "C" int64_t crthip_probe_group_props(const uint8_t *blob, size_t len, uint32_t g, char *out, size_t cap) {
	BlobLayout L;
	int err = walk_blob(blob, len, L);
	if(err) return fail(err);
	if(g >= L.group_props.size()) return fail(CRTHIP_E_ARGUMENT);
	return flat_pairs(L.group_props[g], out, cap);
}

extern "C" uint64_t crthip_arena_layout(uint32_t nblobs, const uint32_t *lens, uint64_t *offsets) {
	uint64_t off = 0;
	for(uint32_t i = 0; i < nblobs; i++) {
		if(offsets) offsets[i] = off;
		off += ((uint64_t)lens[i] + 15) & ~15ull;
	}
	return off;
}

// Wait for the batch in flight on this context (if any) and move its per-blob status from the pinned landing zone into the
// batch object.  EVERY place that is about to reuse the context's stream, scratch or status buffer goes through here, so a
// decode(A); decode(B); sync(A) sequence still reports A's failures (status used to be read only by crthip_batch_sync(A) and
// was lost when another call had synchronised first).
int harvest(crthip_ctx *ctx) {
	crthip_batch *b = ctx->in_flight;
	if(!b) return CRTHIP_OK;
	crthip_ctx::Half &set = ctx_set(ctx, b);                               // the status block and the upload bookkeeping are its parity's
	if(hipEventSynchronize(ctx->ev_done) != hipSuccess) { ctx->in_flight = nullptr; return CRTHIP_E_DEVICE; }
	// (only an upload that sits in front of the event: one enqueued behind the decode is still on its way)
	if(set.done_covers_seq == set.upload_seq) set.arena_upload_pending = false;
	const int32_t *hs = (const int32_t *)set.status_host.p;
	const size_t n = b->blobs.size();
	const StatusWords W{n, b->quant_bound.size(), !b->meshlet_bound.empty()};
	for(size_t i = 0; i < n; i++) b->status[i] = b->blobs[i].host_status ? b->blobs[i].host_status : hs[W.status(i)];
	if(!b->quant_bound.empty()) {                                         // CRTHIP_BIND_QUANTIZED: the records the kernels wrote behind the status words
		const crthip_quant_transform *rec = (const crthip_quant_transform *)((const uint8_t *)hs + W.records());
		b->quant_recs.assign(rec, rec + b->quant_bound.size());
	}
	if(!b->meshlet_bound.empty()) {                                       // crthip_batch_bind_meshlets: a record a blob behind those
		const crthip_meshlet_counts *rec = (const crthip_meshlet_counts *)((const uint8_t *)hs + W.meshlet_record(0));
		b->meshlet_recs.assign(rec, rec + n);
	}
	b->stats.topology_fallbacks = 0; b->stats.delta_redone = 0; b->stats.delta_walked = 0;
	for(size_t i = 0; i < n; i++) {
		b->stats.topology_fallbacks += (uint64_t)(hs[W.topo_flags(i)] & 1);
		b->stats.delta_walked += (uint32_t)(hs[W.delta_flags(i) + 1] != 0);
		if(!b->planned_wide) b->stats.delta_redone += (uint64_t)(hs[W.delta_flags(i)] != 0);
	}
	// what the context learns from them (plan_feedback.h)
	ctx->delta.update(b->planned_wide, b->stats.delta_redone, ctx->dbg.delta_wide != 0);
	ctx->topo.update(n, [&](size_t i) { const auto &L = b->blobs[i].L;
		return TopoBlob{L.h.nface, L.clers.size, (uint32_t)hs[W.topo_flags(i)], b->status[i]}; });
	ctx->in_flight = nullptr;
	return CRTHIP_OK;
}

namespace corto_hip {
int ctx_device(crthip_ctx *ctx) { return ctx->device; }
int ctx_encode_topology(crthip_ctx *ctx) { return ctx->encode_topology; }
crthip_splice_stats &ctx_splice_stats(crthip_ctx *ctx) { return ctx->enc_splice; }
uint64_t ctx_encode_image_budget(crthip_ctx *ctx) { return ctx->dbg.encode_image_budget; }
hipStream_t ctx_stream(crthip_ctx *ctx) { return ctx->stream; }
bool ctx_pipelines(crthip_ctx *ctx) { return ctx->single_stream && !ctx->dbg.carry_off; }
bool batch_carriable(const crthip_batch *b) { return b && b->carriable; }
bool batch_entropy_done(const crthip_batch *b) { return b && b->staged && b->staged->e_done; }
// on the context's main stream, ordered before its next decode
int ctx_fill_async(crthip_ctx *ctx, void *dst, size_t bytes, int value) {
	if(!bytes) return CRTHIP_OK;
	if(hipSetDevice(ctx->device) != hipSuccess) return fail(CRTHIP_E_DEVICE);
	hipLaunchKernelGGL(k_fill_block, dim3(2048), dim3(256), 0, ctx->stream, (uint8_t *)dst, (uint64_t)bytes, (uint32_t)(value & 255));
	return hipGetLastError() == hipSuccess ? CRTHIP_OK : fail(CRTHIP_E_DEVICE);
}
// SURVEY 8d's secondary region: a decode's outputs copied to (pinned) host memory behind its kernels, on the context's main stream; what
// crthip_batch_sync / crthip_batch_done wait for moves behind the copy
int ctx_copy_to_host_async(crthip_ctx *ctx, void *host_dst, const void *dev_src, size_t bytes) {
	if(!bytes) return CRTHIP_OK;
	if(hipSetDevice(ctx->device) != hipSuccess) return fail(CRTHIP_E_DEVICE);
	if(hipMemcpyAsync(host_dst, dev_src, bytes, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) return fail(CRTHIP_E_DEVICE);
	if(hipEventRecord(ctx->ev_done, ctx->stream) != hipSuccess) return fail(CRTHIP_E_DEVICE);
	return CRTHIP_OK;
}
int ctx_quiesce(crthip_ctx *ctx) {
	if(harvest(ctx) != CRTHIP_OK) return fail(CRTHIP_E_DEVICE);
	ctx->last_decoded = nullptr;                         // the encoder stages reuse the scratch block
	return CRTHIP_OK;
}
}

int ctx_stream2(crthip_ctx *ctx, hipStream_t *out) {
	if(!ctx->stream2 && hipStreamCreateWithFlags(&ctx->stream2, hipStreamNonBlocking) != hipSuccess) {
		ctx->stream2 = nullptr; (void)hipGetLastError();
		return fail(CRTHIP_E_DEVICE, "hipStreamCreateWithFlags (second stream)");
	}
	*out = ctx->stream2;
	return CRTHIP_OK;
}

extern "C" int crthip_device_count(void) {
	int n = 0;
	if(hipGetDeviceCount(&n) != hipSuccess) return 0;
	return n;
}

extern "C" void crthip_ctx_destroy(crthip_ctx *c);
extern "C" void crthip_batch_destroy(crthip_batch *b);
extern "C" int crthip_ctx_create(int device, crthip_ctx **out) {
	if(!out) return fail(CRTHIP_E_ARGUMENT);
	int n = 0;
	if(hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return fail(CRTHIP_E_DEVICE);
	HIP_TRY(hipSetDevice(device));
	crthip_ctx *c = new crthip_ctx();
	c->device = device;
	// stream2 is made by the first launch that forks (ctx_stream2): a stream takes a share of a hardware queue whether it is used or not,
	// and the runtime gives each new stream the queue with the fewest streams - a pool's single-stream contexts, created one after the
	// other, then fall on the queues in turn instead of on every other one
	if(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
	   hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) != hipSuccess ||
	   hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) != hipSuccess ||
	   hipEventCreateWithFlags(&c->ev_done, hipEventDisableTiming) != hipSuccess) { delete c; return fail(CRTHIP_E_DEVICE); }
	c->dbg = debug_config_from_env();
	c->delta.wide = c->dbg.delta_wide != 0;
	// kernels that may ask for more than 64 KiB of dynamic LDS: raise their limit on this device, once per context
	// (function attributes are per device; doing it here keeps the launch paths free of shared state between host threads)
	if(hipFuncSetAttribute((const void *)k_topology_lds, hipFuncAttributeMaxDynamicSharedMemorySize, (int)TOPO_LDS_MAX) != hipSuccess ||
	   hipFuncSetAttribute((const void *)k_topology_lds_big, hipFuncAttributeMaxDynamicSharedMemorySize, (int)TOPO_LDS_MAX) != hipSuccess ||
	   hipFuncSetAttribute((const void *)k_delta_lds16, hipFuncAttributeMaxDynamicSharedMemorySize, (int)DELTA16_LDS_MAX) != hipSuccess ||
	   hipFuncSetAttribute((const void *)k_delta_lds16_carry, hipFuncAttributeMaxDynamicSharedMemorySize, (int)DELTA16_LDS_MAX) != hipSuccess ||
	   hipFuncSetAttribute((const void *)k_normal_blob<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)NORMAL_LDS_MAX) != hipSuccess ||
	   hipFuncSetAttribute((const void *)k_normal_blob<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)NORMAL_LDS_MAX) != hipSuccess ||
	   hipFuncSetAttribute((const void *)k_adjacency_blob, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ADJ_BLOB_LDS_MAX) != hipSuccess ||
	   hipFuncSetAttribute((const void *)k_weld_blob, hipFuncAttributeMaxDynamicSharedMemorySize, (int)WELD_BLOB_LDS_MAX) != hipSuccess ||
	   hipFuncSetAttribute((const void *)k_lod_blob, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LOD_BLOB_LDS_MAX) != hipSuccess ||
	   hipFuncSetAttribute((const void *)k_cloud_lod_blob, hipFuncAttributeMaxDynamicSharedMemorySize, (int)WELD_BLOB_LDS_MAX) != hipSuccess ||
	   hipFuncSetAttribute((const void *)k_bvh_blob, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bvh_blob_lds_bytes(BVH_BLOB_FACES)) != hipSuccess ||
	   hipFuncSetAttribute((const void *)k_enc_topo_walk<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ENC_TOPO_LDS_MAX) != hipSuccess ||
	   hipFuncSetAttribute((const void *)k_enc_tun_parse, hipFuncAttributeMaxDynamicSharedMemorySize,
	   	(int)enc_parse_lds(ENC_TRIE_LDS_MAX)) != hipSuccess) {
		crthip_ctx_destroy(c); return fail(CRTHIP_E_DEVICE, "hipFuncSetAttribute(MaxDynamicSharedMemorySize)");
	}
	*out = c;
	return CRTHIP_OK;
}

extern "C" void crthip_ctx_destroy(crthip_ctx *c) {
	if(!c) return;
	(void)hipSetDevice(c->device);
	(void)hipStreamSynchronize(c->stream);
	c->timer.release();
	if(c->host_batch) { crthip_batch *hb = c->host_batch; c->host_batch = nullptr; crthip_batch_destroy(hb); }
	for(crthip_ctx::Half &h : c->set) h.release();
	c->host_out.release(); c->host_pin.release();
	c->walk_dev.release(); c->walk_pin.release();
	cast_state_release(c);
	query_state_release(c);
	closest_state_release(c);
	if(c->ev_walk0) (void)hipEventDestroy(c->ev_walk0);
	if(c->ev_walk1) (void)hipEventDestroy(c->ev_walk1);
	if(c->stream2) (void)hipStreamSynchronize(c->stream2);
	(void)hipEventDestroy(c->ev_fork); (void)hipEventDestroy(c->ev_join); (void)hipEventDestroy(c->ev_done);
	if(c->stream2) (void)hipStreamDestroy(c->stream2);
	(void)hipStreamDestroy(c->stream);
	delete c;
}

extern "C" int crthip_ctx_set_profiling(crthip_ctx *c, int enable) {
	if(!c) return fail(CRTHIP_E_ARGUMENT);
	c->profiling = enable != 0;
	return CRTHIP_OK;
}

extern "C" int crthip_ctx_set_packed_host_blobs(crthip_ctx *c, int on) {
	if(!c) return fail(CRTHIP_E_ARGUMENT);
	c->packed_host = on != 0;
	return CRTHIP_OK;
}

extern "C" int crthip_ctx_encode_splice_stats(const crthip_ctx *c, crthip_splice_stats *s) {
	if(!c || !s) return fail(CRTHIP_E_ARGUMENT, "crthip_ctx_encode_splice_stats: null argument");
	*s = c->enc_splice;
	return CRTHIP_OK;
}

extern "C" int crthip_ctx_set_encode_topology(crthip_ctx *c, int where) {
	if(!c) return fail(CRTHIP_E_ARGUMENT);
	if(where != CRTHIP_TOPOLOGY_HOST && where != CRTHIP_TOPOLOGY_DEVICE && where != CRTHIP_TOPOLOGY_SPLIT)
		return fail(CRTHIP_E_ARGUMENT, "crthip_ctx_set_encode_topology: unknown mode");
	c->encode_topology = where;
	return CRTHIP_OK;
}

extern "C" int crthip_ctx_set_single_stream(crthip_ctx *c, int on) {
	if(!c) return fail(CRTHIP_E_ARGUMENT);
	c->single_stream = on != 0;
	// many batches in flight: kernels wait for LDS to come free, and a request of 29 KB finds room long before one of 78 KB does - the
	// normals kernel with its face normals in an L2-resident scratch array instead of LDS is slower alone (38 vs 34 us per C4 batch) and
	// the pipelined rate higher (round 2, 41 against 91 KB: +10 %)
	c->normal_fn_max = on ? 0u : NORMAL_FN_LDS_MAX;
	return CRTHIP_OK;
}

extern "C" int crthip_ctx_sync(crthip_ctx *c) {
	if(!c) return fail(CRTHIP_E_ARGUMENT);
	HIP_TRY(hipSetDevice(c->device));
	HIP_TRY(hipStreamSynchronize(c->stream));
	return CRTHIP_OK;
}

// ------------------------------------------------------------------------------------------------

// What batch_fill and batch_fill_resident share.  begin_fill: the object forgets its last life (a planned stage, stats, quantised records) and
// its set of per-call blocks is the one of its parity; adopt_blob: a blob whose layout is known takes its place in the arena, unbound, and is
// counted (its bytes in the arena layout are returned); end_fill: the arena and the status words of a fill that went through
static crthip_ctx::Half &begin_fill(crthip_ctx *ctx, crthip_batch *b) {
	b->ctx = ctx;
	drop_staged(b);
	b->stats = crthip_batch_stats{};
	b->walk = crthip_walk_stats{};
	b->dirty = true; b->decoded = false;
	b->d_arena = nullptr;
	b->quant_dev = nullptr; b->quant_bound.clear(); b->quant_recs.clear();
	b->meshlet_bound.clear(); b->meshlet_recs.clear();
	return ctx_set(ctx, b);
}
static uint64_t adopt_blob(BlobPlan &P, uint64_t arena_off, uint32_t len, crthip_batch_stats &stats) {
	P.arena_off = arena_off; P.len = len;
	P.bind.assign(P.L.h.attrs.size(), Binding{});
	P.index = nullptr; P.index_u16 = 0; P.host_status = 0; P.derived.clear();
	P.dbg_clers = P.dbg_pred = ~0ull; P.dbg_nclers = 0; P.clers_in_arena = false;
	stats.total_nvert += P.L.h.nvert; stats.total_nface += P.L.h.nface;
	if(P.L.h.nface) { stats.clers_symbols += P.L.clers.size; stats.split_bytes += (uint64_t)P.L.split.nwords*4; }
	return ((uint64_t)len + 15) & ~15ull;
}
static int end_fill(crthip_batch *b, const uint8_t *d_arena, uint64_t bytes, double t_create) {
	b->arena_bytes = bytes;
	b->stats.arena_bytes = bytes;
	b->d_arena = d_arena;
	b->status.assign(b->blobs.size(), 0);
	b->stats.host_create_us = (float)(now_us() - t_create);
	return CRTHIP_OK;
}
// the guards of every reset: the device, the object's decode in flight harvested, its intermediates no longer the context's last
static int begin_reset(crthip_batch *b) {
	crthip_ctx *ctx = b->ctx;
	HIP_TRY(hipSetDevice(ctx->device));
	if(ctx->in_flight == b) { if(harvest(ctx) != CRTHIP_OK) return fail(CRTHIP_E_DEVICE); }
	if(ctx->last_decoded == b) ctx->last_decoded = nullptr;
	return CRTHIP_OK;
}

// (re)fill a batch object from a list of blobs: header parse + bounds-checked walk of each, arena layout, upload unless resident
// (dev_off: null, or - device_arena set - where every blob lies relative to it; without it the blobs follow one another in arena layout)
static int batch_fill(crthip_ctx *ctx, crthip_batch *b, uint32_t nblobs, const uint8_t *const *blobs, const uint32_t *lens,
	const void *device_arena, const uint64_t *dev_off = nullptr) {
	const double t_create = now_us();
	crthip_ctx::Half &set = begin_fill(ctx, b);
	b->blobs.resize(nblobs);
	b->walk.host_walked = nblobs;
	uint64_t off = 0;
	for(uint32_t i = 0; i < nblobs; i++) {
		BlobPlan &P = b->blobs[i];
		reset_layout(P.L);
		int err = walk_blob(blobs[i], lens[i], P.L);
		if(err) return fail(err, std::string(crthip_strerror(err)) + " (blob " + std::to_string(i) + ")");
		off += adopt_blob(P, device_arena && dev_off ? dev_off[i] : off, lens[i], b->stats);
	}
	const uint8_t *d_arena = (const uint8_t *)device_arena;
	if(!device_arena && off) {
		if(b->own_arena.reserve(off) != CRTHIP_OK) return fail(CRTHIP_E_NOMEM);
		// the blobs are gathered in a pinned image of the arena and go up in ONE copy on the context's stream, in front of the kernels that
		// read them - and nobody waits for it (round 3: the hipStreamSynchronize that stood here was 100 us of every from-host step, on the
		// host thread): the image is this context's own buffer, reused only after harvest() has seen the batch it fed complete
		if(harvest(ctx) != CRTHIP_OK) return fail(CRTHIP_E_DEVICE);
		// packed host blobs (corto_hip.h): the caller's buffers ARE the arena's image, in pieces.  A run is a stretch of blobs that follow one another in
		// host memory as they do in the arena; every run goes up with a copy of its own, straight from the caller's memory.  One run is one copy of
		// one buffer; a pool lane's group of items is a run an item.  Beyond PACKED_RUNS_MAX (pool_internal.h) runs the copies' own cost (a few us of enqueue and a DMA
		// descriptor each) is no longer small beside the memcpy they save, and the blobs are gathered as if the switch were off
		using corto_hip::PACKED_RUNS_MAX;
		uint32_t run_first[PACKED_RUNS_MAX], nruns = 0;
		bool in_place = ctx->packed_host && nblobs > 0;
		for(uint32_t i = 0; in_place && i < nblobs; i++) {
			if(!corto_hip::packed_run_starts(blobs, lens, i)) continue;
			if(nruns == PACKED_RUNS_MAX) in_place = false; else run_first[nruns++] = i;
		}
		if(in_place) {
			// the copies below read the caller's buffers whenever the DMA engine gets to them: nothing here snapshots them or waits (corto_hip.h:
			// the caller keeps them alive and unchanged until the batch is synced).  A pageable buffer would still work (HIP stages it), a pinned
			// one is what the switch promises: on request, check
			for(uint32_t r = 0; r < nruns; r++) {
				const uint32_t i0 = run_first[r], i1 = r + 1 < nruns ? run_first[r + 1] : nblobs;
				const uint64_t at = b->blobs[i0].arena_off, bytes = b->blobs[i1 - 1].arena_off + lens[i1 - 1] - at;
				if(ctx->dbg.check_pinned) {
					hipPointerAttribute_t pa;
					if(hipPointerGetAttributes(&pa, blobs[i0]) != hipSuccess || pa.type != hipMemoryTypeHost) { (void)hipGetLastError();
						return fail(CRTHIP_E_ARGUMENT, "packed host blobs: the buffer is not pinned host memory ($CORTO_HIP_CHECK_PINNED)"); }
				}
				if(hipMemcpyAsync((uint8_t *)b->own_arena.p + at, blobs[i0], bytes, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) return fail(CRTHIP_E_DEVICE);
			}
			b->stats.upload_copies = nruns;
		} else {
		// (a batch that was created and not decoded yet: its upload has to be through before the image is reused)
		if(set.arena_upload_pending) {
			if(hipStreamSynchronize(ctx->stream) != hipSuccess) return fail(CRTHIP_E_DEVICE);
			set.arena_upload_pending = false; set.done_covers_seq = set.upload_seq;
		}
		if(set.arena_pin.reserve(off) != CRTHIP_OK) return fail(CRTHIP_E_NOMEM);
		uint8_t *h = (uint8_t *)set.arena_pin.p;
		for(uint32_t i = 0; i < nblobs; i++) memcpy(h + b->blobs[i].arena_off, blobs[i], lens[i]);
		if(hipMemcpyAsync(b->own_arena.p, h, off, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) return fail(CRTHIP_E_DEVICE);
		set.arena_upload_pending = true;
		set.upload_seq++;
		b->stats.upload_copies = 1; b->stats.upload_gathered_bytes = off;
		}
		d_arena = (const uint8_t *)b->own_arena.p;
	}
	return end_fill(b, d_arena, off, t_create);
}

extern "C" int crthip_batch_create(crthip_ctx *ctx, uint32_t nblobs, const uint8_t *const *blobs, const uint32_t *lens,
                                   const void *device_arena, crthip_batch **out) {
	if(!ctx || !out || (nblobs && (!blobs || !lens))) return fail(CRTHIP_E_ARGUMENT);
	HIP_TRY(hipSetDevice(ctx->device));
	crthip_batch *b = new crthip_batch();
	const int err = batch_fill(ctx, b, nblobs, blobs, lens, device_arena);
	if(err) { b->own_arena.release(); delete b; return err; }
	*out = b;
	return CRTHIP_OK;
}

extern "C" int crthip_batch_reset(crthip_batch *b, uint32_t nblobs, const uint8_t *const *blobs, const uint32_t *lens,
	const void *device_arena) {
	if(!b || !b->ctx || (nblobs && (!blobs || !lens))) return fail(CRTHIP_E_ARGUMENT);
	if(const int err = begin_reset(b)) return err;
	return batch_fill(b->ctx, b, nblobs, blobs, lens, device_arena);    // on failure the batch is left empty-handed: reset or destroy it
}

namespace corto_hip {
// crthip_batch_reset for blobs resident in SEVERAL device arenas (a pool lane's group of items): blob i lies at device_base + dev_off[i]
int batch_reset_at(crthip_batch *b, uint32_t nblobs, const uint8_t *const *blobs, const uint32_t *lens, const void *device_base, const uint64_t *dev_off) {
	if(!b || !b->ctx || !nblobs || !blobs || !lens || !device_base || !dev_off) return fail(CRTHIP_E_ARGUMENT);
	if(const int err = begin_reset(b)) return err;
	return batch_fill(b->ctx, b, nblobs, blobs, lens, device_base, dev_off);
}
}

// (re)fill a batch object from blobs that live in device memory: k_walk_blobs walks them on the context's main stream (one wave and one
// record a blob), the records come back in one copy, and the host turns each into the layout walk_blob would have returned.  A blob whose
// layout does not fit its record is copied back alone and walked here.  On failure the batch is left empty-handed.
static int batch_fill_resident(crthip_ctx *ctx, crthip_batch *b, uint32_t nblobs, const uint8_t *base, const uint64_t *offsets,
	const uint32_t *lens) {
	const double t_create = now_us();
	crthip_ctx::Half &set = begin_fill(ctx, b);
	b->blobs.clear(); b->status.clear(); b->arena_bytes = 0;
	for(uint32_t i = 0; i < nblobs; i++)
		if(offsets[i] & 15) return fail(CRTHIP_E_ARGUMENT, "resident blob offsets must be multiples of 16 (blob " + std::to_string(i) + ")");
	const uint32_t cap = WALK_RECORD_BYTES;
	const size_t jobs_bytes = ((size_t)nblobs*sizeof(WalkJob) + 255) & ~(size_t)255, rec_bytes = (size_t)nblobs*cap;
	uint8_t *recs = nullptr;
	if(nblobs) {
		if(ctx->walk_dev.reserve(jobs_bytes + rec_bytes) != CRTHIP_OK || ctx->walk_pin.reserve(jobs_bytes + rec_bytes) != CRTHIP_OK)
			return fail(CRTHIP_E_NOMEM);
		if(!ctx->ev_walk0 && hipEventCreate(&ctx->ev_walk0) != hipSuccess) { ctx->ev_walk0 = nullptr; return fail(CRTHIP_E_DEVICE); }
		if(!ctx->ev_walk1 && hipEventCreate(&ctx->ev_walk1) != hipSuccess) { ctx->ev_walk1 = nullptr; return fail(CRTHIP_E_DEVICE); }
		uint8_t *d = (uint8_t *)ctx->walk_dev.p, *h = (uint8_t *)ctx->walk_pin.p;
		WalkJob *jobs = (WalkJob *)h;
		for(uint32_t i = 0; i < nblobs; i++) jobs[i] = WalkJob{offsets[i], lens[i], 0};
		// behind whatever the stream holds (another batch's decode: this waits for it), then one synchronisation
		hipStream_t st = ctx->stream;
		bool ok = hipMemcpyAsync(d, h, (size_t)nblobs*sizeof(WalkJob), hipMemcpyHostToDevice, st) == hipSuccess &&
		          hipEventRecord(ctx->ev_walk0, st) == hipSuccess;
		if(ok) {
			hipLaunchKernelGGL(k_walk_blobs, dim3(nblobs), dim3(64), 0, st, base, (const WalkJob *)d, nblobs, d + jobs_bytes, cap);
			ok = hipGetLastError() == hipSuccess && hipEventRecord(ctx->ev_walk1, st) == hipSuccess &&
			     hipMemcpyAsync(h + jobs_bytes, d + jobs_bytes, rec_bytes, hipMemcpyDeviceToHost, st) == hipSuccess;
		}
		const bool synced = hipStreamSynchronize(st) == hipSuccess;
		if(!ok || !synced) { (void)hipGetLastError(); return fail(CRTHIP_E_DEVICE, "the device walk of resident blobs failed"); }
		set.arena_upload_pending = false; set.done_covers_seq = set.upload_seq;
		float ms = 0.f;
		if(hipEventElapsedTime(&ms, ctx->ev_walk0, ctx->ev_walk1) == hipSuccess) b->walk.walk_kernel_us = ms*1000.f;
		b->walk.bytes_to_host = rec_bytes;
		recs = h + jobs_bytes;
	}
	b->blobs.resize(nblobs);
	std::vector<uint32_t> copy;                                    // a fallback blob, 4-byte aligned
	uint64_t bytes = 0;
	for(uint32_t i = 0; i < nblobs; i++) {
		BlobPlan &P = b->blobs[i];
		reset_layout(P.L);
		int err = record_to_layout(recs + (size_t)i*cap, cap, P.L);
		if(err == WALK_FALLBACK) {
			reset_layout(P.L);
			copy.resize(((size_t)lens[i] + 3)/4 + 1);
			if(lens[i] && (hipMemcpyAsync(copy.data(), base + offsets[i], lens[i], hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
			   hipStreamSynchronize(ctx->stream) != hipSuccess)) {
				(void)hipGetLastError(); b->blobs.clear(); return fail(CRTHIP_E_DEVICE, "copying resident blob " + std::to_string(i) + " back");
			}
			b->walk.host_walked++; b->walk.bytes_to_host += lens[i];
			err = walk_blob((const uint8_t *)copy.data(), lens[i], P.L);
		} else b->walk.device_walked++;
		if(err) { b->blobs.clear(); return fail(err, std::string(crthip_strerror(err)) + " (blob " + std::to_string(i) + ")"); }
		bytes += adopt_blob(P, offsets[i], lens[i], b->stats);
	}
	return end_fill(b, base, bytes, t_create);
}

extern "C" int crthip_batch_create_resident(crthip_ctx *ctx, uint32_t nblobs, const void *device_base, const uint64_t *offsets,
                                            const uint32_t *lens, crthip_batch **out) {
	if(!ctx || !out || (nblobs && (!device_base || !offsets || !lens)) || ((uintptr_t)device_base & 15)) return fail(CRTHIP_E_ARGUMENT);
	HIP_TRY(hipSetDevice(ctx->device));
	crthip_batch *b = new crthip_batch();
	const int err = batch_fill_resident(ctx, b, nblobs, (const uint8_t *)device_base, offsets, lens);
	if(err) { delete b; return err; }
	*out = b;
	return CRTHIP_OK;
}

extern "C" int crthip_batch_reset_resident(crthip_batch *b, uint32_t nblobs, const void *device_base, const uint64_t *offsets,
                                           const uint32_t *lens) {
	if(!b || !b->ctx || (nblobs && (!device_base || !offsets || !lens)) || ((uintptr_t)device_base & 15)) return fail(CRTHIP_E_ARGUMENT);
	if(const int err = begin_reset(b)) return err;
	return batch_fill_resident(b->ctx, b, nblobs, (const uint8_t *)device_base, offsets, lens);
}

extern "C" void crthip_batch_destroy(crthip_batch *b) {
	if(!b) return;
	if(b->ctx) {
		(void)hipSetDevice(b->ctx->device);
		if(b->ctx->in_flight == b) { (void)hipStreamSynchronize(b->ctx->stream); b->ctx->in_flight = nullptr; }
		if(b->ctx->last_decoded == b) b->ctx->last_decoded = nullptr;
		if(b->ctx->host_batch == b) b->ctx->host_batch = nullptr;
		if(b->staged) (void)hipStreamSynchronize(b->ctx->stream);           // (its entropy stage may be on the stream, reading the arena)
	}
	drop_staged(b);
	b->own_arena.release();
	delete b;
}

extern "C" uint32_t crthip_batch_size(const crthip_batch *b) { return b ? (uint32_t)b->blobs.size() : 0; }

extern "C" int crthip_batch_info(const crthip_batch *b, uint32_t i, crthip_blob_info *info) {
	if(!b || !info || i >= b->blobs.size()) return fail(CRTHIP_E_ARGUMENT);
	fill_info(b->blobs[i].L.h, info);
	return CRTHIP_OK;
}

extern "C" int64_t crthip_batch_exif(const crthip_batch *b, uint32_t i, char *out, size_t cap) {
	if(!b || i >= b->blobs.size()) return fail(CRTHIP_E_ARGUMENT);
	return flat_pairs(b->blobs[i].L.h.exif, out, cap);
}

extern "C" int64_t crthip_batch_groups(const crthip_batch *b, uint32_t i, uint32_t *group_end, size_t cap) {
	if(!b || i >= b->blobs.size()) return fail(CRTHIP_E_ARGUMENT);
	const BlobLayout &L = b->blobs[i].L;
	for(size_t k = 0; k < L.group_end.size() && k < cap; k++) group_end[k] = L.group_end[k];
	return (int64_t)L.group_end.size();
}

extern "C" int64_t crthip_batch_group_props(const crthip_batch *b, uint32_t i, uint32_t g, char *out, size_t cap) {
	if(!b || i >= b->blobs.size() || g >= b->blobs[i].L.group_props.size()) return fail(CRTHIP_E_ARGUMENT);
	return flat_pairs(b->blobs[i].L.group_props[g], out, cap);
}

extern "C" int crthip_batch_walk_stats(const crthip_batch *b, crthip_walk_stats *s) {
	if(!b || !s) return fail(CRTHIP_E_ARGUMENT);
	*s = b->walk;
	return CRTHIP_OK;
}

static int build_and_launch_inner(crthip_batch *b);
static int decode_pair(crthip_batch *cur, crthip_batch *next);
void drop_staged(crthip_batch *b) { delete b->staged; b->staged = nullptr; }
// A decode call that fails half-way (a HIP error between two launches) may have kernels queued that write per-blob status into the
// context's pinned block and into its scratch; in_flight is not set on that path, so nothing downstream would wait for them before the
// next call clears or moves those blocks.  Drain the context's streams before the error is returned.
static int build_and_launch(crthip_batch *b) {
	const int err = build_and_launch_inner(b);
	if(err) {
		crthip_ctx *ctx = b->ctx;
		(void)hipStreamSynchronize(ctx->stream);
		if(ctx->stream2) (void)hipStreamSynchronize(ctx->stream2);
		(void)hipGetLastError();
		b->decoded = false;
	}
	return err;
}

static int build_and_launch_inner(crthip_batch *b) {
	// host-side cost of a decode call (crthip_batch_stats::host_*_us)
	const double t0 = now_us();
	b->ctx->timer.reset();
	ctx_set(b->ctx, b).plan.reset();
	Planner P(b);
	int err = P.carve();
	if(!err) err = P.jobs();
	if(err) return err;
	P.group();
	const double t1 = now_us();
	if((err = P.upload()) != CRTHIP_OK) return err;
	const double t2 = now_us();
	if((err = P.launch()) != CRTHIP_OK) return err;
	if((err = P.mark_done()) != CRTHIP_OK) return err;
	P.account();
	const double t3 = now_us();
	b->stats.host_plan_us = (float)(t1 - t0); b->stats.host_stage_us = (float)(t2 - t1); b->stats.host_launch_us = (float)(t3 - t2);
	return CRTHIP_OK;
}

extern "C" int crthip_batch_decode(crthip_batch *b) {
	if(!b || !b->ctx) return fail(CRTHIP_E_ARGUMENT);
	HIP_TRY(hipSetDevice(b->ctx->device));
	if(b->staged) return crthip_batch_decode_with_next(b, nullptr);        // planned by crthip_batch_decode_with_next: its mesh stage (and whatever else is due)
	return build_and_launch(b);
}

// The two-stage schedule of a pipelined lane (plan_launch.cpp: PH_*).  `next` is planned and uploaded like any decode; `cur` was `next` one call ago.
// Enqueued, in stream order: next's descriptor copy and zeroing | cur's stage M, with next's K-TAB inside k_front's grid and next's K-STREAM inside
// k_delta_lds16's when both batches allow it (Planner::hosts_carry / carry_args) | else next's K-TAB and K-STREAM as launches of their own | next's
// k_fill | the done-event.  A `next` whose schedule has no separate entropy stage (a context with two streams, long Tunstall streams) is only
// planned and uploaded here: the call that has it as `cur` runs its whole schedule.  Same bytes whichever way.
static int decode_pair(crthip_batch *cur, crthip_batch *next) {
	crthip_ctx *ctx = (cur ? cur : next)->ctx;
	const double t0 = now_us();
	ctx->timer.reset();
	int err;
	Planner *N = nullptr;
	Planner *const C = cur ? cur->staged : nullptr;
	Carry carry{}; bool carried = false, nsplit = false;
	double t1 = t0, t2 = t0;
	if(next) {
		drop_staged(next);
		ctx_set(ctx, next).plan.reset();
		next->staged = N = new Planner(next);
		err = N->carve();
		if(!err) err = N->jobs();
		if(err) return err;
		N->group();
		t1 = now_us();
		if((err = N->upload()) != CRTHIP_OK) return err;
		t2 = now_us();
		next->stats.host_plan_us = (float)(t1 - t0); next->stats.host_stage_us = (float)(t2 - t1);
		nsplit = N->splits();
		carried = cur && nsplit && N->carry_args(carry) && C->hosts_carry();  // (with or without its own entropy stage in front)
	}
	// the first batch of a lane runs its entropy stage alone; after that a stage that cannot be carried is not enqueued early at all - its launches
	// behind cur's kernels cost the queue what they cost in front of its own mesh stage, and measured slower (profiles/pool_carry.md)
	const bool early = nsplit && (carried || !cur);
	if(early && (err = N->launch(PH_UP)) != CRTHIP_OK) return err;
	if(cur && (err = C->launch(C->e_done ? (uint32_t)PH_MESH : (uint32_t)PH_ALL, carried ? &carry : nullptr)) != CRTHIP_OK) return err;
	if(early) {
		if((err = N->launch(carried ? (uint32_t)PH_FILL : (uint32_t)(PH_TUN | PH_FILL))) != CRTHIP_OK) return err;
		N->e_done = true;
	}
	if(cur) {
		if((err = C->mark_done()) != CRTHIP_OK) return err;
		C->account();
		cur->stats.host_launch_us = (float)(now_us() - t2);
		drop_staged(cur);
	} else HIP_TRY(hipEventRecord(ctx->ev_done, ctx->stream));
	return CRTHIP_OK;
}

extern "C" int crthip_batch_decode_with_next(crthip_batch *cur, crthip_batch *next) {
	if((!cur && !next) || cur == next) return fail(CRTHIP_E_ARGUMENT);
	crthip_ctx *ctx = (cur ? cur : next)->ctx;
	if(!ctx || (cur && next && (next->ctx != ctx || cur->parity == next->parity)))
		return fail(CRTHIP_E_ARGUMENT, "crthip_batch_decode_with_next: two batches of one context and of different parity");
	if(cur && !cur->staged) return fail(CRTHIP_E_ARGUMENT, "crthip_batch_decode_with_next: `cur` has not been `next` of an earlier call");
	HIP_TRY(hipSetDevice(ctx->device));
	// one call in flight per context: the one before is harvested first (its status block is about to be cleared when it shares `next`'s parity)
	if(harvest(ctx) != CRTHIP_OK) return fail(CRTHIP_E_DEVICE);
	const int err = decode_pair(cur, next);
	if(err) {                                                              // (as build_and_launch: nothing of a failed call stays queued)
		(void)hipStreamSynchronize(ctx->stream);
		if(ctx->stream2) (void)hipStreamSynchronize(ctx->stream2);
		(void)hipGetLastError();
		if(cur) { drop_staged(cur); cur->decoded = false; }
		if(next) { drop_staged(next); next->decoded = false; }
	}
	return err;
}

extern "C" int crthip_batch_set_parity(crthip_batch *b, uint32_t parity) {
	if(!b || !b->ctx || parity > 1) return fail(CRTHIP_E_ARGUMENT);
	if(b->parity == parity) return CRTHIP_OK;
	HIP_TRY(hipSetDevice(b->ctx->device));
	// what the object has on its old parity's blocks - an arena image on its way, a decode in flight, a planned stage - is finished or dropped first
	if(b->ctx->in_flight == b && harvest(b->ctx) != CRTHIP_OK) return fail(CRTHIP_E_DEVICE);
	if(b->staged || b->ctx->last_decoded == b) { HIP_TRY(hipStreamSynchronize(b->ctx->stream)); drop_staged(b); }
	if(b->ctx->last_decoded == b) b->ctx->last_decoded = nullptr;
	b->parity = (uint8_t)parity; b->dirty = true; b->decoded = false;
	return CRTHIP_OK;
}

extern "C" int crthip_batch_sync(crthip_batch *b, int32_t *status) {
	if(!b || !b->ctx) return fail(CRTHIP_E_ARGUMENT);
	crthip_ctx *ctx = b->ctx;
	HIP_TRY(hipSetDevice(ctx->device));
	// else: harvested when the context moved on (or never decoded)
	if(ctx->in_flight == b) { if(harvest(ctx) != CRTHIP_OK) return fail(CRTHIP_E_DEVICE); }
	int first = CRTHIP_OK;
	for(size_t i = 0; i < b->blobs.size(); i++) {
		if(status) status[i] = b->status[i];
		if(b->status[i] && !first) { first = b->status[i]; fail(first, std::string(crthip_strerror(first)) + " (blob " +
			std::to_string(i) + ")"); }
	}
	return first;
}

extern "C" int crthip_batch_done(crthip_batch *b) {
	if(!b || !b->ctx) return fail(CRTHIP_E_ARGUMENT);
	crthip_ctx *ctx = b->ctx;
	if(ctx->in_flight != b) return 1;                                  // harvested already, or never decoded
	if(hipSetDevice(ctx->device) != hipSuccess) return fail(CRTHIP_E_DEVICE);
	const hipError_t e = hipEventQuery(ctx->ev_done);
	if(e == hipSuccess) return 1;
	if(e == hipErrorNotReady) { (void)hipGetLastError(); return 0; }
	return fail(CRTHIP_E_DEVICE);
}

extern "C" int crthip_batch_get_stats(const crthip_batch *b, crthip_batch_stats *s) {
	if(!b || !s) return fail(CRTHIP_E_ARGUMENT);
	*s = b->stats;
	return CRTHIP_OK;
}

// the timer's records of the (synced) stream folded by kernel name
static void fold_kernel_times(const KernelTimer &timer, crthip_kernel_times *t) {
	memset(t, 0, sizeof(*t));
	for(auto &r : timer.recs) {
		float ms = 0;
		if(hipEventElapsedTime(&ms, timer.pool[r.e0], timer.pool[r.e1]) != hipSuccess) continue;
		uint32_t k = 0;
		for(; k < t->count; k++) if(strcmp(t->name[k], r.name) == 0) break;
		if(k == t->count) { if(t->count == CRTHIP_MAX_KERNELS) continue; t->name[k] = r.name; t->count++; }
		t->ms[k] += ms; t->launches[k]++;
	}
}

extern "C" int crthip_batch_kernel_times(crthip_batch *b, crthip_kernel_times *t) {
	if(!b || !t) return fail(CRTHIP_E_ARGUMENT);
	crthip_ctx *ctx = b->ctx;
	memset(t, 0, sizeof(*t));
	HIP_TRY(hipStreamSynchronize(ctx->stream));
	fold_kernel_times(ctx->timer, t);
	return CRTHIP_OK;
}

extern "C" int64_t crthip_batch_read_prediction(crthip_batch *b, uint32_t i, void *host_out, size_t cap) {
	return crthip_batch_debug_read(b, i, "prediction", host_out, cap);
}

extern "C" int64_t crthip_batch_debug_read(crthip_batch *b, uint32_t i, const char *what, void *host_out, size_t cap) {
	if(!b || i >= b->blobs.size() || !what || !host_out || !b->decoded) return fail(CRTHIP_E_ARGUMENT);
	crthip_ctx *ctx = b->ctx;
	if(ctx->last_decoded != b) return fail(CRTHIP_E_ARGUMENT, "the context's scratch block has been reused by a later call");
	HIP_TRY(hipStreamSynchronize(ctx->stream));
	const uint8_t *scratch = (const uint8_t *)ctx_set(ctx, b).scratch.p;
	BlobPlan &P = b->blobs[i];
	const uint8_t *src = nullptr; size_t n = 0;
	if(!strcmp(what, "clers")) {
		if(P.dbg_clers == ~0ull) return 0;
		src = P.clers_in_arena ? b->d_arena + P.dbg_clers : scratch + P.dbg_clers; n = P.dbg_nclers;
	} else if(!strcmp(what, "prediction")) {
		if(P.dbg_pred == ~0ull) return 0;
		src = scratch + P.dbg_pred; n = (size_t)P.L.h.nvert*12;
	} else return fail(CRTHIP_E_ARGUMENT);
	n = std::min(n, cap);
	HIP_TRY(hipMemcpy(host_out, src, n, hipMemcpyDeviceToHost));
	return (int64_t)n;
}

// ------------------------------------------------------------------------------------------------
// blobs with HOST output buffers: the crt::Decoder facade's decode() (one blob, crthip_decode_host) and its combiner (the blobs of
// every thread that called decode() at about the same time, decoder_facade.cpp).  The batch object, the device output block and its
// pinned landing zone live in the context: in the steady state a call is one upload of the blobs, one descriptor upload, the kernels,
// and ONE download of all outputs - no allocation, no per-attribute copies.  Serialised per context (host_mutex).
// A blob the walk rejects fails alone: the others are decoded without it.
namespace corto_hip {
int decode_host_many(crthip_ctx *ctx, uint32_t n, HostDecodeReq *reqs, bool copy_out) {
	if(!ctx || !reqs || n == 0) return fail(CRTHIP_E_ARGUMENT);
	std::lock_guard<std::mutex> lock(ctx->host_mutex);
	// whatever way this call ends, no request may be left saying "OK, nothing to copy": a request's status is CRTHIP_OK only once its
	// blob has been through the kernels (the facade's combiner publishes these words to other threads, decoder_facade.cpp)
	auto fail_all = [&](int code) {
		for(uint32_t i = 0; i < n; i++)
			if(reqs[i].status == CRTHIP_OK) { reqs[i].status = code; reqs[i].nout = 0; }
		return code;
	};
	for(uint32_t i = 0; i < n; i++) { reqs[i].status = CRTHIP_OK; reqs[i].nout = 0; }
	if(hipSetDevice(ctx->device) != hipSuccess) return fail_all(fail(CRTHIP_E_DEVICE, "hipSetDevice"));
	// the blobs the walk accepts (a malformed one must not take its neighbours down)
	std::vector<const uint8_t *> blobs; std::vector<uint32_t> lens; std::vector<uint32_t> who;
	for(uint32_t i = 0; i < n; i++) {
		HostDecodeReq &r = reqs[i];
		if(!r.blob || r.len > 0xFFFFFFFFull) { r.status = r.blob ? CRTHIP_E_LIMIT : CRTHIP_E_ARGUMENT; continue; }
		if(n > 1) { BlobLayout L; const int e = walk_blob(r.blob, r.len, L); if(e) { r.status = fail(e); continue; } }
		blobs.push_back(r.blob); lens.push_back((uint32_t)r.len); who.push_back(i);
	}
	const uint32_t m = (uint32_t)blobs.size();
	if(m == 0) return reqs[0].status;
	int err;
	if(!ctx->host_batch) err = crthip_batch_create(ctx, m, blobs.data(), lens.data(), nullptr, &ctx->host_batch);
	else err = crthip_batch_reset(ctx->host_batch, m, blobs.data(), lens.data(), nullptr);
	if(err) return fail_all(err);
	crthip_batch *b = ctx->host_batch;
	// outputs of every blob back to back in one device block (16-byte aligned pieces)
	std::vector<crthip_attr_binding> dev; std::vector<size_t> dev_first(m, 0); std::vector<void *> dindex(m, nullptr);
		std::vector<uint32_t> ifmt(m, CRTHIP_FMT_UINT32);
	struct Piece { uint32_t req, slot; size_t off, bytes; void *host; };
	std::vector<Piece> pieces;
	std::vector<std::pair<uint32_t, size_t>> pred_piece;            // (blob of the batch, offset in the output block)
	size_t total = 0;
	for(uint32_t k = 0; k < m; k++) {
		HostDecodeReq &r = reqs[who[k]];
		const BlobLayout &L = b->blobs[k].L;
		const uint32_t nvert = L.h.nvert, nface = L.h.nface;
		const size_t na = L.h.attrs.size();
		dev_first[k] = dev.size();
		for(size_t a = 0; a < na; a++) {
			// attrs == NULL: nothing bound (an index-only decode); host buffers have upstream's packed layouts - a stride is refused, not
			// ignored
			crthip_attr_binding d;
			if(r.attrs) d = r.attrs[a]; else { d.buffer = nullptr; d.format = CRTHIP_FMT_FLOAT; d.out_components = 0; d.stride = 0; d.reserved = 0; }
			if(d.buffer && d.stride) { r.status = fail(CRTHIP_E_ARGUMENT,
				"crthip_decode_host: host buffers are tightly packed (stride must be 0)"); d.buffer = nullptr; }
			d.stride = 0; d.reserved &= CRTHIP_BIND_STREAM_VALUES;
			if(d.buffer && r.status == CRTHIP_OK) {
				const AttrHeader &A = L.h.attrs[a];
				size_t bytes;
				if(A.codec == CRTHIP_CODEC_NORMAL) bytes = (size_t)nvert*3*(d.format == CRTHIP_FMT_INT16 ? 2 : 4);
				else if(A.codec == CRTHIP_CODEC_COLOR) bytes = (size_t)nvert*(d.out_components ? d.out_components : 4);
				// (the decode works in int32 / int64 records whatever the output format: DESIGN.md 1)
				else bytes = (size_t)nvert*A.N*generic_work_bytes(d.format);
				pieces.push_back(Piece{who[k], (uint32_t)a, total, bytes, d.buffer});
				d.buffer = (void *)(uintptr_t)(total + 1);                    // (offset + 1: rebased below, once the block is there)
				total += (bytes + 15) & ~(size_t)15;
			} else d.buffer = nullptr;
			dev.push_back(d);
		}
		if(r.index && nface && r.status == CRTHIP_OK) {
			const size_t bytes = (size_t)nface*3*(r.index_format == CRTHIP_FMT_UINT16 ? 2 : 4);
			pieces.push_back(Piece{who[k], CRTHIP_MAX_ATTRS, total, bytes, r.index});
			dindex[k] = (void *)(uintptr_t)(total + 1); ifmt[k] = r.index_format;
			total += (bytes + 15) & ~(size_t)15;
		}
		if(r.prediction && nface && r.status == CRTHIP_OK) {         // the prediction triples: copied out of the scratch block behind the kernels (below)
			pieces.push_back(Piece{who[k], CRTHIP_MAX_ATTRS + 1, total, (size_t)nvert*12, r.prediction});
			pred_piece.push_back({k, total});
			total += ((size_t)nvert*12 + 15) & ~(size_t)15;
		}
	}
	if(ctx->host_out.reserve(total + 16) != CRTHIP_OK || ctx->host_pin.reserve(total +
		16) != CRTHIP_OK) return fail_all(fail(CRTHIP_E_NOMEM));
	uint8_t *dbase = (uint8_t *)ctx->host_out.p, *hbase = (uint8_t *)ctx->host_pin.p;
	for(auto &d : dev) if(d.buffer) d.buffer = dbase + ((uintptr_t)d.buffer - 1);
	for(auto &p : dindex) if(p) p = dbase + ((uintptr_t)p - 1);
	// bound blob by blob: a binding the device path refuses (a format, an alignment) fails ITS blob - which is then decoded with nothing
	// bound - and nobody else's (upstream's Decoder objects share nothing, src/decoder.cpp:126-196)
	err = CRTHIP_OK;
	for(uint32_t k = 0; k < m && !err; k++) {
		HostDecodeReq &r = reqs[who[k]];
		const size_t na = b->blobs[k].L.h.attrs.size();
		int e = r.status != CRTHIP_OK ? r.status : crthip_batch_bind(b, k, na ? dev.data() + dev_first[k] : nullptr, dindex[k], ifmt[k]);
		if(e) {
			if(r.status == CRTHIP_OK) r.status = e;
			for(size_t a = 0; a < na; a++) dev[dev_first[k] + a].buffer = nullptr;
			e = crthip_batch_bind(b, k, na ? dev.data() + dev_first[k] : nullptr, nullptr, CRTHIP_FMT_UINT32);
			if(e) err = e;                                                 // (cannot happen: nothing is bound)
		}
	}
	if(!err) err = crthip_batch_decode(b);
	for(auto &pp : pred_piece) {
		const BlobPlan &P = b->blobs[pp.first];
		if(!err && P.dbg_pred != ~0ull && hipMemcpyAsync(dbase + pp.second, (const uint8_t *)ctx_set(ctx, b).scratch.p + P.dbg_pred, (size_t)P.L.h.nvert*12,
			hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess) err = fail(CRTHIP_E_DEVICE);
	}
	if(!err && total && hipMemcpyAsync(hbase, dbase, total, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) err = fail(CRTHIP_E_DEVICE);
	std::vector<int32_t> st(m, 0);
	// (waits for the kernels: the event behind them; keeps the context consistent on error)
	const int serr = crthip_batch_sync(b, st.data());
	if(hipStreamSynchronize(ctx->stream) != hipSuccess && !err) err = fail(CRTHIP_E_DEVICE);   // ... and this for the copy behind them
	if(!err && (serr == CRTHIP_E_DEVICE || serr == CRTHIP_E_NOMEM)) err = serr;
	for(uint32_t k = 0; k < m; k++) { HostDecodeReq &r = reqs[who[k]]; if(r.status != CRTHIP_OK) continue; r.status = err ? err : st[k]; }
	for(const Piece &p : pieces) {
		HostDecodeReq &r = reqs[p.req];
		if(r.status != CRTHIP_OK) continue;
		if(copy_out) memcpy(p.host, hbase + p.off, p.bytes);
		else if(r.nout < CRTHIP_MAX_ATTRS + 2) { r.out_src[r.nout] = hbase + p.off; r.out_dst[r.nout] = p.host; r.out_bytes[r.nout] =
			p.bytes; r.nout++; }
	}
	if(err) return err;
	// (the first failing blob's code - its message is the thread's last error; every status is in its request)
	for(uint32_t i = 0; i < n; i++) if(reqs[i].status) return reqs[i].status;
	return CRTHIP_OK;
}
}

extern "C" int crthip_decode_host(crthip_ctx *ctx, const uint8_t *blob, size_t len, const crthip_attr_binding *attrs,
                                  void *index, uint32_t index_format) {
	if(!ctx || !blob) return fail(CRTHIP_E_ARGUMENT);
	if(len > 0xFFFFFFFFull) return fail(CRTHIP_E_LIMIT, "blob larger than 4 GiB");
	HostDecodeReq r{};
	r.blob = blob; r.len = len; r.attrs = attrs; r.index = index; r.index_format = index_format;
	return decode_host_many(ctx, 1, &r, true);
}

// ------------------------------------------------------------------------------------------------
// stand-alone Tunstall run over device-resident blocks (roofline measurement of K-TAB/K-TUN)
extern "C" int crthip_tunstall_decode_blocks(crthip_ctx *ctx, uint32_t n, const uint8_t *host_blocks, const void *device_blocks,
                                             const uint64_t *block_offset, void *device_out, const uint64_t *out_offset,
                                             crthip_kernel_times *times) {
	if(!ctx || !host_blocks || !device_blocks || !block_offset || !device_out || !out_offset) return fail(CRTHIP_E_ARGUMENT);
	HIP_TRY(hipSetDevice(ctx->device));
	if(harvest(ctx) != CRTHIP_OK) return fail(CRTHIP_E_DEVICE);
	ctx->last_decoded = nullptr;
	std::vector<TunStream> tun; std::vector<uint32_t> chunk_stream; std::vector<FillJob> fills;
	uint32_t chunks = 0, max_nchunks = 0; bool multi = false;
	for(uint32_t i = 0; i < n; i++) {
		const uint8_t *p = host_blocks + block_offset[i];
		const uint32_t ns = p[0];
		auto rd = [&](const uint8_t *q) { return (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24);
			};
		const uint32_t size = rd(p + 1 + 2*ns), csize = rd(p + 5 + 2*ns);
		const uint8_t *dblk = (const uint8_t *)device_blocks + block_offset[i];
		uint8_t *dst = (uint8_t *)device_out + out_offset[i];
		if(size == 0) continue;
		if(ns == 1) { fills.push_back(FillJob{dst, size, p[1]}); continue; }
		if(ns == 0 || csize == 0) return fail(CRTHIP_E_TRUNCATED);
		TunStream t{};
		t.src = dblk + 9 + 2*ns; t.dst = dst; t.probs = dblk + 1; t.csize = csize; t.size = size; t.nsym = ns; t.table =
			(uint32_t)tun.size();
		t.chunk0 = chunks; tun_pick_geometry(t);
		if(t.nchunks > 1) multi = true;
		max_nchunks = std::max(max_nchunks, t.nchunks);
		for(uint32_t c = 0; c < t.nchunks; c++) chunk_stream.push_back((uint32_t)tun.size());
		chunks += t.nchunks;
		tun.push_back(t);
	}
	Carver cv;
	const uint64_t o_tab = cv.take(tun.size()*sizeof(TunTable)), o_part = cv.take(((uint64_t)chunks*4 + 4)*8);
	const uint64_t o_jobs = cv.take(0);
	const uint64_t o_tun = cv.take(tun.size()*sizeof(TunStream) + 16, 16), o_cs = cv.take(chunk_stream.size()*4 + 16, 16), o_fill =
		cv.take(fills.size()*sizeof(FillJob) + 16, 16);
	const uint64_t total = cv.take(0);
	crthip_ctx::Half &set = ctx->set[0];                                   // (no batch object: the blocks of a lone context's decodes)
	if(set.scratch.reserve(total + 256) != CRTHIP_OK || set.staging.reserve(total - o_jobs +
		256) != CRTHIP_OK) return fail(CRTHIP_E_NOMEM);
	uint8_t *base = (uint8_t *)set.scratch.p, *stage = (uint8_t *)set.staging.p;
	if(!tun.empty()) memcpy(stage + (o_tun - o_jobs), tun.data(), tun.size()*sizeof(TunStream));
	if(!chunk_stream.empty()) memcpy(stage + (o_cs - o_jobs), chunk_stream.data(), chunk_stream.size()*4);
	if(!fills.empty()) memcpy(stage + (o_fill - o_jobs), fills.data(), fills.size()*sizeof(FillJob));
	hipStream_t st = ctx->stream;
	HIP_TRY(hipMemcpyAsync(base + o_jobs, stage, total - o_jobs, hipMemcpyHostToDevice, st));
	ctx->timer.reset();
	Launch LT{ctx};
	{ int e_ = tun_chain(LT, st, tun, (TunStream *)(base + o_tun), (uint32_t *)(base + o_cs), chunks, (TunTable *)(base + o_tab), (uint64_t *)(base + o_part),
		max_nchunks, multi, (FillJob *)(base + o_fill), (uint32_t)fills.size()); if(e_) return e_; }
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipStreamSynchronize(st));
	if(times) fold_kernel_times(ctx->timer, times);
	return CRTHIP_OK;
}
