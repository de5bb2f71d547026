// plan_jobs.cpp — Planner::jobs: pass 2 - the job descriptors of every stage.  A pointer into scratch is written as SP(offset) and
// resolved by upload(); every other pointer goes in as the real address (the Planner's comment, batch_internal.h).
// jobs() keeps the status block, the CLERS streams and the loop over the blobs; what one blob contributes is made by the members below it.
#include "batch_internal.h"

// float -> int32 as x86's cvttss2si does it (out of range, NaN: INT_MIN): the unit of a normal attribute as upstream's host code computes it
static int32_t f2i_x86_host(float x) {
	if(!(x > -2147483904.0f && x < 2147483648.0f)) return (int32_t)0x80000000;
	return (int32_t)x;
}

// what the stages share about one blob
struct Planner::BlobView {
	uint32_t i; BlobPlan &P; const BlobLayout &L; BlobScratch &S;
	bool mesh; uint32_t nvert, nface;
	int pos_k, uv_k;                                     // the attributes named "position" and "uv", or -1
	bool tangents, bounds;                               // computes_tangents / bounds_meshlets
	bool pos_ints_needed, pos_by_normal;                 // who turns the integer positions into floats (view_of)
	size_t rec0;                                         // the blob's first quant record (crthip_batch_bind_all's order)
};
// the bit block of one attribute, shared by the K-BIT jobs of its streams
struct Planner::BitBlock { const uint32_t *words; uint32_t nwords, out_limit, chain0, first_job; bool by_wave; };

// the dictionary table is per launch group: the attribute streams' dictionaries are not shared with the CLERS streams' (different HIP streams)
void Planner::clear_dict_table() {
	if(ctx->dict_slots.size() != 8192) ctx->dict_slots.assign(8192, 0u);
	for(uint32_t u : ctx->dict_used) ctx->dict_slots[u] = 0;
	ctx->dict_used.clear(); ctx->dict_keys.clear(); ctx->dict_ids.clear();
	dict_group0 = (uint32_t)pl.tun_dict.v.size();
}

// the dictionary (TunTable slot) of a stream: a new one, or the one an earlier stream of this launch group with the same table got
uint32_t Planner::dict_of(const StreamRef &s, const TunStream &t) {
	std::vector<uint32_t> &dict_ids = ctx->dict_ids;
	const uint32_t fresh = (uint32_t)pl.tun_dict.v.size();
	auto make = [&]() { TunStream d = t; d.dst = nullptr; d.table = fresh; d.dict = fresh; d.nchunks = 1; pl.tun_dict.v.push_back(d); return fresh; };
	// (0 / 2: one dictionary per stream, whatever repeats)
	if(s.nsym > 16 || fresh - dict_group0 >= 4096 || ctx->dbg.tun_share == 0 || ctx->dbg.tun_share == 2) return make();
	uint64_t h = 0x9E3779B97F4A7C15ull ^ s.nsym;
	for(uint32_t k = 0; k < 2*s.nsym; k += 8) { uint64_t w; memcpy(&w, s.probs16 + k, 8); h = (h ^ w)*0xFF51AFD7ED558CCDull;
		h ^= h >> 32; }
	for(uint32_t pos = (uint32_t)h & 8191u;; pos = (pos + 1) & 8191u) {
		const uint32_t e = ctx->dict_slots[pos];
		if(!e) {
			ctx->dict_slots[pos] = (uint32_t)ctx->dict_keys.size() + 1; ctx->dict_used.push_back(pos);
			crthip_ctx::DictKey key; key.n = (uint8_t)s.nsym; memcpy(key.bytes, s.probs16, 32);
			ctx->dict_keys.push_back(key);
			const uint32_t d = make();
			dict_ids.push_back(d);
			return d;
		}
		const crthip_ctx::DictKey &key = ctx->dict_keys[e - 1];
		if(key.n == s.nsym && memcmp(key.bytes, s.probs16, 2*s.nsym) == 0) return dict_ids[e - 1];
	}
}

// where the decoded symbols of a stream will be: in the arena, or in scratch
const uint8_t *Planner::add_stream(const StreamRef &s, uint64_t sym_off, uint64_t blob_off) {
	if(s.mode == STREAM_RAW) return arena + blob_off + s.payload_off;
	if(s.mode == STREAM_EMPTY) return SP(0);
	if(s.mode == STREAM_FILL) { pl.fill.v.push_back(FillJob{SP(sym_off), s.size, s.fill}); return SP(sym_off); }
	TunStream t{};
	t.src = arena + blob_off + s.payload_off; t.dst = SP(sym_off); t.probs = arena + blob_off + s.probs_off;
	t.csize = s.csize; t.size = s.size; t.nsym = s.nsym; t.table = (uint32_t)pl.tun.v.size();
	t.chunk0 = tun_chunks; tun_pick_geometry(t);
	if(t.nchunks > 1) pl.tun_multi_chunk = true;
	pl.tun_max_nchunks = std::max(pl.tun_max_nchunks, t.nchunks);
	push_blocks(pl.tun_chunk_stream, (uint32_t)pl.tun.v.size(), t.nchunks);
	tun_chunks += t.nchunks;
	t.dict = dict_of(s, t);
	pl.tun.v.push_back(t);
	return SP(sym_off);
}

void Planner::push_unpack(const BitBlock &bb, const StreamRef &s, const uint8_t *logs, void *out, uint8_t mode, uint16_t fields, uint16_t stride,
	uint16_t comp, uint8_t out_kind) {
	if(s.size == 0) return;
	UnpackJob u{};
	u.logs = logs; u.words = bb.words; u.out = out; u.count = s.size; u.nwords = bb.nwords; u.out_limit = bb.out_limit;
	u.chunk0 = unpack_chunks; u.chain_chunk0 = bb.chain0; u.fields = fields; u.stride = stride; u.comp = comp; u.mode = mode;
	u.out_kind = out_kind;
	if(bb.by_wave) { u.chain_chunk0 = bb.first_job; pl.unpack_wave_ids.v.push_back((uint32_t)pl.unpack.v.size()); }
	else {
		const uint32_t nc = (s.size + CHUNK - 1)/CHUNK;
		push_blocks(pl.unpack_chunk_job, (uint32_t)pl.unpack.v.size(), nc);
		unpack_chunks += nc;
	}
	pl.unpack.v.push_back(u);
}

int Planner::jobs() {
	// the status block is about to move: the batch in flight writes to it
	// (a batch with a quantised binding keeps a crthip_quant_transform an attribute behind the status words)
	{
		uint32_t nattr = 0; bool any = false;
		for(const BlobPlan &P : b->blobs) { nattr += (uint32_t)P.bind.size(); for(const Binding &bd : P.bind) any = any || (bd.buffer && bd.quantized); }
		pl.quant_records = any ? nattr : 0u;
		for(const BlobPlan &P : b->blobs) pl.meshlet_records = pl.meshlet_records || builds_meshlets(P);
		hs = StatusWords{b->blobs.size(), pl.quant_records, pl.meshlet_records};
	}
	const size_t status_bytes = hs.bytes() + 16;
	if(status_bytes > set.status_host.cap && harvest(ctx) != CRTHIP_OK) return fail(CRTHIP_E_DEVICE);
	if(set.status_host.reserve(status_bytes) != CRTHIP_OK) return fail(CRTHIP_E_NOMEM);
	hs_base = (int32_t *)set.status_host.p;
	quant_rec_host = (QuantOutRecord *)((uint8_t *)hs_base + hs.records());

	// the CLERS streams come first in every stream/chunk/fill array: they are what the topology kernel waits for, the
	// attribute streams are decoded on the second HIP stream while topology runs
	clear_dict_table();
	std::vector<const uint8_t *> &clers_ptrs = ctx->plan_clers;
	clers_ptrs.assign(nblobs, nullptr);
	for(uint32_t i = 0; i < nblobs; i++) {
		const BlobLayout &L = b->blobs[i].L;
		if(L.h.nface > 0) clers_ptrs[i] = add_stream(L.clers, bs[i].clers, b->blobs[i].arena_off);
	}
	clers_tun = (uint32_t)pl.tun.v.size(); clers_chunks = tun_chunks; clers_fill = (uint32_t)pl.fill.v.size();
	clers_dict = (uint32_t)pl.tun_dict.v.size();
	clear_dict_table();                                                      // the attribute streams are a launch of their own

	est_vbase = est_fbase = 0;
	size_t rec0 = 0;
	for(uint32_t i = 0; i < nblobs; rec0 += b->blobs[i].bind.size(), i++) {
		const BlobView v = view_of(i, rec0);
		if(v.mesh) topo_job(v);
		for(size_t k = 0; k < v.L.attrs.size(); k++) attr_jobs(v, k);       // (a refused stored normal skips that attribute alone)
		// the derived outputs, each behind what it reads.  The bind calls checked them; one that is refused here all the same has set the blob's
		// host_status, and the blob gets no later derived job
		if(computes_normals(v.P) && !computed_normal_job(v)) continue;
		if(v.tangents && !tangent_job(v)) continue;
		if(builds_meshlets(v.P)) meshlet_jobs(v);
		if(binds_weld(v.P) && !v.P.host_status) weld_jobs(v);
		if(binds_adjacency(v.P) && !v.P.host_status) adjacency_jobs(v);
		if(binds_lod(v.P) && !v.P.host_status) lod_jobs(v);
		if(binds_cloud_lod(v.P) && !v.P.host_status) cloud_lod_jobs(v);
		if(binds_compact(v.P) && !v.P.host_status) compact_jobs(v);
		if(binds_bvh(v.P) && !v.P.host_status) bvh_jobs(v);
	}
	return CRTHIP_OK;
}

Planner::BlobView Planner::view_of(uint32_t i, size_t rec0) {
	BlobPlan &P = b->blobs[i]; const BlobLayout &L = P.L;
	const bool mesh = L.h.nface > 0; const uint32_t nvert = L.h.nvert, nface = L.h.nface;
	// position attribute (needed by ESTIMATED/BORDER normals)
	const int pos_k = attr_named(P, "position"), uv_k = attr_named(P, "uv");
	// computed tangents read the integer positions AND the integer uvs, behind every normal kernel: neither K-DELTA nor the fused normal
	// kernel may turn them into floats on the way - both fall to k_dequant, which runs behind the tangent kernels
	const bool tangents = computes_tangents(P);
	// ... and so do meshlet bounds, behind the meshlet kernels: the integer positions last until k_dequant
	const bool bounds = bounds_meshlets(P);
	// ... and so do the weld, in front of the adjacency kernels, and the levels of detail and the BVH behind them
	const bool weld = binds_weld(P) || binds_lod(P) || binds_bvh(P);
	// who turns the integer positions into floats: estimated normals read them as integers after K-DELTA, so the fused normal
	// kernel does it as their last reader (pos_by_normal), the separate normal kernels leave it to k_dequant behind them, and
	// without such normals K-DELTA does it on the way out of LDS like for every other attribute
	uint32_t readers = 0;
	for(size_t k = 0; k < L.attrs.size(); k++)
		if(mesh && L.h.attrs[k].codec == CRTHIP_CODEC_NORMAL && P.bind[k].buffer && (L.attrs[k].normal_prediction == 1 ||
			L.attrs[k].normal_prediction == 2)) readers++;
	if(computes_normals(P)) readers++;                        // computed normals read the integer positions as a stored estimate does
	const bool pos_ints_needed = readers > 0 || tangents || bounds || weld;
	const bool pos_by_normal = !tangents && !bounds && !weld && readers == 1 && normal_fused(nvert, nface) && pos_k >= 0 && P.bind[pos_k].format == CRTHIP_FMT_FLOAT;
	return BlobView{i, P, L, bs[i], mesh, nvert, nface, pos_k, uv_k, tangents, bounds, pos_ints_needed, pos_by_normal, rec0};
}

void Planner::topo_job(const BlobView &v) {
	BlobPlan &P = v.P; const BlobLayout &L = v.L; BlobScratch &S = v.S;
	const uint64_t bo = P.arena_off;
	P.clers_in_arena = L.clers.mode == STREAM_RAW;
	P.dbg_clers = L.clers.mode == STREAM_RAW ? bo + L.clers.payload_off : S.clers;
	P.dbg_nclers = L.clers.size; P.dbg_pred = S.pred;
	TopoJob t{};
	t.clers = ctx->plan_clers[v.i];
	t.split_words = (const uint32_t *)(arena + bo + L.split.words_off);
	t.group_end = (const uint32_t *)(uintptr_t)(pl.aux_u32.v.size()*4);   // bytes into aux_u32 (resolved by upload)
	for(uint32_t ge : L.group_end) pl.aux_u32.v.push_back(ge);
	const Faces f = faces_of(v.i); t.faces = f.p; t.faces_u16 = f.u16;
	t.pred = (uint32_t *)SP(S.pred);
	t.front_a = (uint4 *)SP(S.front_a); t.front_b = (uint2 *)SP(S.front_b);
	t.order = (uint32_t *)SP(S.order); t.delayed = (uint32_t *)SP(S.delayed);
	t.status = hs_base + hs.status(v.i);
	t.flags = hs_base + hs.topo_flags(v.i);
	t.nclers = L.clers.size; t.split_nwords = L.split.nwords; t.ngroups = (uint32_t)L.group_end.size();
	t.nvert = v.nvert; t.nface = v.nface; t.front_cap = S.front_cap;
	t.opts = S.progress != ~0ull ? TOPO_OPT_PROGRESS : 0u;
	// every mesh takes the LDS path; a lone big mesh may use most of a CU's LDS, a batch keeps its blobs small
	uint32_t ring, pool, symwin;
	uint32_t scale = ctx->topo.scale, pool_q8 = ctx->topo.pool_q8, need;
	// as much of what the context has learnt as fits a CU
	for(;;) {
		topo_lds_geometry(v.nface, L.clers.size, TOPO_SLOTS_MAX, scale, pool_q8, topo_slots(nblobs), ring, pool, symwin, ctx->topo.pool_cap);
		// every delayed edge is a pool record: same capacity
		need = topo_lds_bytes(ring, pool, pool, symwin);
#ifdef CORTO_TOPO_STAMPS
		if(need <= 32768 && L.clers.size < 8190) need = 65536;              // (the dispatch trace: k_mesh.hip TOPO_ASM_STAMP)
#endif
		if(need <= TOPO_LDS_MAX || (scale == 1 && pool_q8 == 8)) break;
		if(pool_q8 > 8 && (pool > ring || scale == 1)) pool_q8 = std::max(8u, pool_q8/2); else scale >>= 1;
	}
	if(need <= TOPO_LDS_MAX) {
		t.lds_ring = ring; t.lds_pool = pool; t.lds_delayed_cap = pool; t.lds_symwin = symwin;
		// (split into two launches below)
		pl.topo_lds_ids.v.push_back((uint32_t)pl.topo.v.size()); pl.topo_need.push_back(need);
	}
	else pl.topo_glob_ids.v.push_back((uint32_t)pl.topo.v.size());
	pl.topo.v.push_back(t);
}

// one bound attribute: its log streams, the K-BIT jobs of its bit block, the inverse of its prediction, its finisher
void Planner::attr_jobs(const BlobView &v, size_t k) {
	const AttrHeader &a = v.L.h.attrs[k]; const AttrStreams &as = v.L.attrs[k]; const Binding &bd = v.P.bind[k];
	if(!bd.buffer) return;
	AttrScratch &A = v.S.attr[k];
	const uint64_t bo = v.P.arena_off; const uint32_t nvert = v.nvert;
	uint64_t attr_logs = 0;
	for(const StreamRef &lg : as.logs) attr_logs += lg.size;
	// one wave per stream, no look-back; its bit cursors are 32-bit (k_stream.hip)
	const bool by_wave = attr_logs <= UNPACK_WAVE_MAX_LOGS && as.bits.nwords < (1u << 26) && !ctx->dbg.unpack_chunked;
	const BitBlock bb{(const uint32_t *)(arena + bo + as.bits.words_off), as.bits.nwords, nvert, unpack_chunks, (uint32_t)pl.unpack.v.size(), by_wave};
	// K-BIT hands its values on as int16 where that is PROVEN to hold them: the attribute's log streams are Tunstall-coded and no width in their tables
	// exceeds 16 bits (decodeArray: v in [-2^(d-1), 2^(d-1)); decodeValues folds the sign the other way: |v| < 2^d, 15 bits), the consumer reads
	// halfwords (k_delta_lds16 on 16-bit records, k_normal_blob), and the stream goes a wave a stream.  Half the bytes of that round trip through HBM
	auto widths_fit = [&](const StreamRef &s, uint32_t bits) { return s.mode != STREAM_RAW && s.max_sym <= bits; };
	bool hand_i16 = false;
	if(v.mesh && by_wave && !wide && !ctx->dbg.values_i32 && nvert > 1) {
		if(a.codec == CRTHIP_CODEC_NORMAL) hand_i16 = as.normal_prediction != 0 && normal_fused(nvert, v.nface) && widths_fit(as.logs[0], 16);
		else if(a.codec != CRTHIP_CODEC_COLOR && !bd.stream_values) {
			DeltaJob probe{};
			probe.nvert = nvert; probe.N = a.N;
			hand_i16 = delta_in_lds(probe, wide);
			if(a.strategy & CRTHIP_CORRELATED) hand_i16 = hand_i16 && widths_fit(as.logs[0], 16);
			else for(uint32_t c = 0; c < a.N && hand_i16; c++) hand_i16 = widths_fit(as.logs[c], 15);
		}
	}
	const uint8_t val_fmt = hand_i16 ? UNPACK_OUT_I16 : UNPACK_OUT_I32;
	std::vector<const uint8_t *> &logs = ctx->plan_logs;
	logs.assign(as.logs.size(), nullptr);
	for(size_t j = 0; j < as.logs.size(); j++) logs[j] = add_stream(as.logs[j], A.sym[j], bo);

	if(a.codec == CRTHIP_CODEC_NORMAL) {
		push_unpack(bb, as.logs[0], logs[0], SP(A.diffs), 0, 2, 2, 0, val_fmt);
		// a (malformed) stream with fewer diffs than vertices: upstream's vector is zero-filled behind them (normal_attribute.cpp:180-184)
		// (only DIFF reads all nvert entries; the other predictions stop at ndiffs)
		if(as.normal_prediction == 0 && as.logs[0].size < nvert) pl.fill.v.push_back(FillJob{SP(A.diffs +
			(uint64_t)as.logs[0].size*8), (nvert - as.logs[0].size)*8u, 0u});
		// DIFF only (normal_attribute.cpp:190-191)
		if(as.normal_prediction == 0) inverse_job(v, k, SP(A.diffs), 2, false, 0, hand_i16);
		stored_normal_job(v, k, hand_i16);
		return;
	}
	bool dequantised;                                        // by K-DELTA (or, the position, by the fused normal kernel): no k_dequant job
	if(a.codec == CRTHIP_CODEC_COLOR) {
		for(uint32_t c = 0; c < a.N; c++) push_unpack(bb, as.logs[c], logs[c], SP(A.color), 1, 1, (uint16_t)a.N, (uint16_t)c, UNPACK_OUT_U8);
		dequantised = inverse_job(v, k, SP(A.color), a.N, (a.strategy & CRTHIP_PARALLEL) != 0, 1, hand_i16);
	} else {
		// packed output: the caller's buffer is the int32 workspace (like upstream, vertex_attribute.h:190-193); with a stride, as
		// DOUBLE (eight bytes a value: upstream widens in place, front to back) or as uint16 grid values (CRTHIP_BIND_QUANTIZED): scratch
		void *work = ints_of(v.i, k);
		if(a.strategy & CRTHIP_CORRELATED) push_unpack(bb, as.logs[0], logs[0], work, 0, (uint16_t)a.N, (uint16_t)a.N, 0, val_fmt);
		else for(uint32_t c = 0; c < a.N; c++) push_unpack(bb, as.logs[c], logs[c], work, 1, 1, (uint16_t)a.N, (uint16_t)c, val_fmt);
		// the device half of a caller-supplied codec object (CRTHIP_BIND_STREAM_VALUES): the stream's int32 values stay as they are -
		// GenericAttr<int>::decode's result (vertex_attribute.h:151-156); deltaDecode / dequantize are the caller's, on the host
		if(bd.stream_values) return;
		dequantised = inverse_job(v, k, work, a.N, (a.strategy & CRTHIP_PARALLEL) != 0, 0, hand_i16);
	}
	if(bd.quantized) quant_job(v, k);
	else if(!dequantised && !((int)k == v.pos_k && v.pos_by_normal)) dequant_job(v, k);
}

// the inverse of an attribute's prediction: K-DELTA along the automaton's graph for a mesh, a scan for a cloud.  True: K-DELTA finishes the attribute
// on its way out of LDS (no k_dequant job)
bool Planner::inverse_job(const BlobView &v, size_t k, void *values, uint32_t N, bool para, uint8_t is_u8, bool hand_i16) {
	const AttrHeader &a = v.L.h.attrs[k]; const AttrStreams &as = v.L.attrs[k]; const Binding &bd = v.P.bind[k];
	const uint32_t nvert = v.nvert;
	if(nvert <= 1) return false;
	if(!v.mesh) {
		CloudJob c{};
		c.values = values; c.nvert = nvert; c.N = N; c.chunk0 = cloud_chunks; c.is_u8 = is_u8;
		const uint32_t nc = N*((nvert + CHUNK - 1)/CHUNK);
		for(uint32_t q = 0; q < nc; q++) pl.cloud_chunk_job.v.push_back((uint32_t)pl.cloud.v.size());
		cloud_chunks += nc;
		pl.cloud.v.push_back(c);
		return false;
	}
	bool dequantised = false;
	DeltaJob d{};
	d.values = values; d.pred = (const uint32_t *)SP(v.S.pred); d.nvert = nvert; d.N = N;
	d.parallelogram = para; d.is_u8 = is_u8; d.in_i16 = hand_i16; d.wide = wide; d.rounds = ctx->dbg.delta_rounds ? 1u : 0u;
	d.progress = v.S.progress != ~0ull ? SP(v.S.progress) : nullptr;   // (k_delta_tiles)
	d.flags = hs_base + hs.delta_flags(v.i);
	// (k_delta_tiles reports a progress word that never came in the blob's status word)
	d.status_back = (uint32_t)(hs.delta_flags(v.i) - hs.status(v.i));
	if(a.codec != CRTHIP_CODEC_NORMAL && delta_in_lds(d, wide)) {
		if(a.codec == CRTHIP_CODEC_COLOR) {
			d.deq = 2; d.out = bd.buffer; d.out_components = bd.out_components; d.out_stride = bd.stride;
			for(int c = 0; c < 4; c++) d.qc[c] = as.qc[c];
			dequantised = true;
		} else if(!bd.stride && bd.format == CRTHIP_FMT_FLOAT && !((int)k == v.pos_k && v.pos_ints_needed) && !((int)k == v.uv_k && v.tangents)) {
			d.deq = 1; d.q = a.q; dequantised = true;
		}
	}
	for(uint32_t f = 0; f < N; f += 4) { d.first = f; pl.delta.v.push_back(d); }   // more than four components: k_delta_tiles jobs of four
	return dequantised;
}

// what ESTIMATED / BORDER normals - stored or computed - share behind their own fields: the integer positions and the index, then either the fused
// kernel (its id list and LDS request are the caller's: stored and computed normals are two launches; its face normals in `facen` when not in LDS; its
// duty as the positions' last reader) or a slice of the batch-wide arrays of the separate kernels.  False: no usable position, host_status is set
bool Planner::estimated_normal_tail(const BlobView &v, NormalJob &n, HostArr<uint32_t> &fused_ids, uint32_t &fused_lds, uint64_t facen) {
	if(!generic_source_ok(v.P, v.pos_k, 3)) { v.P.host_status = CRTHIP_E_NORMAL_NEEDS_POSITION; return false; }
	const Binding &pos = v.P.bind[v.pos_k];
	n.position = ints_of(v.i, v.pos_k);
	const Faces f = faces_of(v.i); n.faces = f.p; n.faces_u16 = f.u16;
	if(normal_fused(v.nvert, v.nface)) {
		n.fused = 1;
		n.fn_scratch = facen != ~0ull ? (float *)SP(facen) : nullptr;
		if(v.pos_by_normal) { n.pos_out = pos.buffer; n.pos_stride = pos.stride ? pos.stride : 12u; n.pos_q = v.L.h.attrs[v.pos_k].q; }
		fused_ids.v.push_back((uint32_t)pl.normal.v.size());
		fused_lds = std::max(fused_lds, normal_blob_lds_fn(v.nvert, v.nface) <= ctx->normal_fn_max ? normal_blob_lds_fn(v.nvert, v.nface) :
			normal_blob_lds(v.nvert, v.nface));
	} else {
		n.vbase = est_vbase; n.fbase = est_fbase; est_vbase += v.nvert; est_fbase += v.nface;
		pl.any_est_normal = true;
	}
	return true;
}

void Planner::stored_normal_job(const BlobView &v, size_t k, bool hand_i16) {
	const AttrStreams &as = v.L.attrs[k]; const Binding &bd = v.P.bind[k]; AttrScratch &A = v.S.attr[k];
	const uint32_t pr = as.normal_prediction;
	if(!(pr == 0 || (v.mesh && (pr == 1 || pr == 2)))) return;       // clouds: postDelta never runs (decoder.cpp:142-143)
	NormalJob n{};
	n.diffs = (int32_t *)SP(A.diffs); n.out = bd.buffer; n.nvert = v.nvert; n.nface = v.nface;
	n.out_stride = bd.stride ? bd.stride : (bd.format == CRTHIP_FMT_INT16 ? 6u : 12u);
	n.ndiffs = std::min(as.logs[0].size, v.nvert); n.unit = f2i_x86_host(v.L.h.attrs[k].q);
	n.prediction = (uint8_t)pr; n.out_i16 = bd.format == CRTHIP_FMT_INT16;
	n.status = hs_base + hs.status(v.i);
	n.diffs_i16 = hand_i16;                                          // (only ever set for a fused estimate: attr_jobs)
	if(pr == 0) pl.any_diff_normal = true;
	else if(!estimated_normal_tail(v, n, pl.normal_fused_ids, pl.normal_fused_lds, A.facen)) return;
	pl.normal.v.push_back(n);
}

// the second finisher of the scratch path: uint16 relative to the minimum + the record (k_quant_out.hip).  No vertex: no job (upload fills the record)
void Planner::quant_job(const BlobView &v, size_t k) {
	const Binding &bd = v.P.bind[k]; AttrScratch &A = v.S.attr[k];
	const uint32_t nvert = v.nvert;
	if(nvert == 0) return;
	QuantOutJob q{};
	q.values = (const int32_t *)SP(A.vals); q.buffer = bd.buffer; q.stride = bd.stride; q.nvert = nvert; q.N = v.L.h.attrs[k].N; q.q = v.L.h.attrs[k].q;
	q.rec_host = (QuantOutRecord *)((crthip_quant_transform *)quant_rec_host + v.rec0 + k);
	q.rec_dev = b->quant_dev ? (QuantOutRecord *)((crthip_quant_transform *)b->quant_dev + v.rec0 + k) : nullptr;
	q.status = hs_base + hs.status(v.i);
	if(nvert <= qout_blob_max()) pl.quant_blob_ids.v.push_back((uint32_t)pl.quant.v.size());
	else {
		q.range = (uint32_t *)SP(A.qrange);
		q.block0 = (uint32_t)pl.quant_block_job.v.size();
		push_blocks(pl.quant_block_job, (uint32_t)pl.quant.v.size(), (nvert + QOUT_BLOCK - 1)/QOUT_BLOCK);
		// the seed of k_quant_range's integer atomics rides with the entropy stage's fills: 0xFF.. the minima, 0 the maxima (quant_out.h: qout_bias)
		pl.fill.v.push_back(FillJob{SP(A.qrange), 16u, 0xFFu}); pl.fill.v.push_back(FillJob{SP(A.qrange + 16), 16u, 0u});
	}
	pl.quant.v.push_back(q);
}

void Planner::dequant_job(const BlobView &v, size_t k) {
	const AttrHeader &a = v.L.h.attrs[k]; const Binding &bd = v.P.bind[k]; AttrScratch &A = v.S.attr[k];
	DequantJob q{};
	q.buffer = bd.buffer; q.q = a.q; q.nvert = v.nvert; q.N = a.N; q.out_components = bd.out_components;
	for(int c = 0; c < 4; c++) q.qc[c] = v.L.attrs[k].qc[c];
	q.block0 = (uint32_t)pl.dequant_block_job.v.size();
	q.is_color = a.codec == CRTHIP_CODEC_COLOR;
	q.format = q.is_color ? (uint8_t)CRTHIP_FMT_FLOAT : (uint8_t)bd.format;
	q.stride = bd.stride;
	if(q.is_color) q.src = SP(A.color);
	else if(bd.stride || bd.format == CRTHIP_FMT_DOUBLE) q.src = SP(A.vals);
	const uint64_t elems = q.is_color ? v.nvert : (uint64_t)v.nvert*a.N;
	const uint32_t nb = (uint32_t)((elems + CHUNK - 1)/CHUNK);
	push_blocks(pl.dequant_block_job, (uint32_t)pl.dequant.v.size(), nb);
	pl.dequant.v.push_back(q);
}

// normals for a blob that stores (or binds) none: crthip_batch_bind_computed_normals.  An ESTIMATED job without corrections - no stream, no
// K-BIT job, nothing of the entropy stage; position, faces, the fused kernel's last-reader duty and the batch-wide slices as for a stored estimate
bool Planner::computed_normal_job(const BlobView &v) {
	const Binding &bd = v.P.derived.normals;
	NormalJob n{};
	n.out = bd.buffer; n.nvert = v.nvert; n.nface = v.nface;
	n.out_stride = bd.stride ? bd.stride : (bd.format == CRTHIP_FMT_INT16 ? 6u : 12u);
	n.prediction = 3; n.out_i16 = bd.format == CRTHIP_FMT_INT16;
	n.status = hs_base + hs.status(v.i);
	if(!estimated_normal_tail(v, n, pl.normal_computed_ids, pl.normal_computed_lds, v.S.cn_facen)) return false;
	pl.normal.v.push_back(n);
	return true;
}

// tangents: crthip_batch_bind_computed_tangents.  The integers where K-DELTA left them (the caller's packed buffer, or scratch), the index, the
// normals where their binding puts them
bool Planner::tangent_job(const BlobView &v) {
	const Binding &bd = v.P.derived.tangents;
	const Binding *nb = tangent_normal_source(v.P);
	if(!generic_source_ok(v.P, v.pos_k, 3)) { v.P.host_status = CRTHIP_E_NORMAL_NEEDS_POSITION; return false; }
	if(!generic_source_ok(v.P, v.uv_k, 2) || !nb) { v.P.host_status = CRTHIP_E_ARGUMENT; return false; }
	const uint32_t nvert = v.nvert, nface = v.nface;
	TangentJob t{};
	t.position = ints_of(v.i, v.pos_k); t.uv = ints_of(v.i, v.uv_k);
	const Faces f = faces_of(v.i); t.faces = f.p; t.faces_u16 = f.u16;
	t.normal = nb->buffer; t.normal_i16 = nb->format == CRTHIP_FMT_INT16;
	t.normal_stride = nb->stride ? nb->stride : (t.normal_i16 ? 6u : 12u);
	t.out = bd.buffer; t.out_i16 = bd.format == CRTHIP_FMT_INT16; t.out_stride = bd.stride ? bd.stride : (t.out_i16 ? 8u : 16u);
	t.nvert = nvert; t.nface = nface;
	if(tangent_in_blob(nvert)) {
		pl.tangent_blob_ids.v.push_back((uint32_t)pl.tangent.v.size());
		pl.tangent_lds = std::max(pl.tangent_lds, tangent_blob_lds(nvert));
	} else {
		t.acc = (uint64_t *)SP(v.S.tan_acc);
		t.fblock0 = (uint32_t)pl.tan_fblock_job.v.size(); t.vblock0 = (uint32_t)pl.tan_vblock_job.v.size();
		push_blocks(pl.tan_fblock_job, (uint32_t)pl.tangent.v.size(), (nface + TAN_BLOCK - 1)/TAN_BLOCK);
		push_blocks(pl.tan_vblock_job, (uint32_t)pl.tangent.v.size(), (nvert + TAN_BLOCK - 1)/TAN_BLOCK);
	}
	pl.tangent.v.push_back(t);
	return true;
}

// meshlets: crthip_batch_bind_meshlets.  The index where the automaton leaves it, the cuts made here from the group table (in aux_u32 behind
// the group lists), the caller's arrays; scratch for a blob of more than one segment.  A refused blob gets neither job
void Planner::meshlet_jobs(const BlobView &v) {
	const crthip_meshlet_binding &mb = v.P.derived.meshlets;
	BlobScratch &S = v.S;
	std::vector<MltSeg> segs; crthip_meshlet_counts bound;
	if(!mlt_plan_of(v.P, mb, &segs, bound) || meshlet_binding_error(&mb, true, bound) || (bound.segments > 1 && S.mlt == ~0ull)) { v.P.host_status = CRTHIP_E_ARGUMENT; return; }
	MeshletJob m{};
	const Faces f = faces_of(v.i); m.faces = f.p; m.faces_u16 = f.u16;
	while(pl.aux_u32.v.size() % 4) pl.aux_u32.v.push_back(0);             // (an MltSeg is read as one 16-byte word)
	m.segs = (const void *)(uintptr_t)(pl.aux_u32.v.size()*4);            // bytes into aux_u32 (resolved by upload)
	for(const MltSeg &sg : segs) { pl.aux_u32.v.push_back(sg.f0); pl.aux_u32.v.push_back(sg.f1); pl.aux_u32.v.push_back(sg.mbase); pl.aux_u32.v.push_back(sg.tbase); }
	m.meshlets = mb.meshlets; m.vertices = mb.vertices; m.triangles = mb.triangles;
	m.rec_host = (uint8_t *)hs_base + hs.meshlet_record(v.i); m.rec_dev = mb.counts;
	m.nface = v.nface; m.nseg = bound.segments; m.max_vertices = mb.max_vertices; m.max_triangles = mb.max_triangles;
	if(bound.segments > 1) {
		const MltScratchLayout lay = mlt_scratch_layout(v.nface, bound);
		m.scratch = SP(S.mlt); m.sc_vertices = (uint32_t)lay.vertices; m.sc_triangles = (uint32_t)lay.triangles; m.sc_counts = (uint32_t)lay.counts;
	}
	if(bound.segments <= MESHLET_BLOB_SEGS) {
		pl.meshlet_blob_ids.v.push_back((uint32_t)pl.meshlet.v.size());
		pl.meshlet_waves = std::max(pl.meshlet_waves, bound.segments);
	} else {
		m.block0 = (uint32_t)pl.mlt_block_job.v.size();
		push_blocks(pl.mlt_block_job, (uint32_t)pl.meshlet.v.size(), bound.segments);
	}
	// meshlet bounds: crthip_batch_bind_meshlet_bounds.  The integer positions as the tangents take them, the arrays above, and the blob's counts
	// in DEVICE memory: the binding's own copy, or one in scratch that the meshlet kernels write in its place.  Skipped when the blob's host_status
	// is set, by this check or by anything before it; the meshlet job is pushed all the same
	if(v.bounds) {
		const bool pos_ok = generic_source_ok(v.P, v.pos_k, 3);
		if(!pos_ok || (!mb.counts && S.mlt_counts == ~0ull)) v.P.host_status = pos_ok ? CRTHIP_E_ARGUMENT : CRTHIP_E_NORMAL_NEEDS_POSITION;
	}
	if(v.bounds && !v.P.host_status) {
		if(!mb.counts) m.rec_dev = SP(S.mlt_counts);
		MeshletBoundsJob q{};
		q.position = ints_of(v.i, v.pos_k);
		q.meshlets = mb.meshlets; q.vertices = mb.vertices; q.triangles = mb.triangles; q.counts = m.rec_dev; q.out = v.P.derived.bounds;
		q.nvert = v.nvert; q.capacity = bound.meshlets;
		q.block0 = (uint32_t)pl.mlb_block_job.v.size();
		push_blocks(pl.mlb_block_job, (uint32_t)pl.meshlet_bounds.v.size(), (bound.meshlets + MB_WAVES - 1)/MB_WAVES);
		pl.meshlet_bounds.v.push_back(q);
	}
	pl.meshlet.v.push_back(m);
}

// the weld: crthip_batch_bind_weld.  The integer positions as the tangents take them, the index where the automaton leaves it, the caller's
// arrays; a blob whose table fits LDS needs no more.  The others keep their table - zeroed by a FillJob in stage E, so that a second decode starts
// clean - in scratch, and a record there if the binding has none.  (The bind call checked all of it)
void Planner::weld_jobs(const BlobView &v) {
	const crthip_weld_binding &wb = v.P.derived.weld;
	const bool blob = weld_in_blob(v.nvert);
	if(!generic_source_ok(v.P, v.pos_k, 3)) { v.P.host_status = CRTHIP_E_NORMAL_NEEDS_POSITION; return; }
	if(weld_binding_error(&wb, v.nvert, v.nface) || (!blob && v.S.weld == ~0ull)) { v.P.host_status = CRTHIP_E_ARGUMENT; return; }
	WeldJob w{};
	w.position = ints_of(v.i, v.pos_k);
	const Faces f = faces_of(v.i); w.index = f.p; w.index_u16 = f.u16;
	w.remap = wb.remap; w.windex = wb.index; w.counts = wb.counts; w.nface = v.nface; w.nvert = v.nvert;
	const uint32_t id = (uint32_t)pl.weld.v.size();
	if(blob) {
		pl.weld_blob_ids.v.push_back(id);
		pl.weld_lds = std::max(pl.weld_lds, (uint32_t)(weld_slots(v.nvert)*4));
	} else {
		const WeldScratchLayout lay = weld_scratch_layout(v.nvert);
		w.table = (uint32_t *)SP(v.S.weld);
		if(!wb.counts) w.counts = SP(v.S.weld + lay.record);
		zero_fill(v.S.weld, lay.record);
		w.vblock0 = (uint32_t)pl.weld_vblock_job.v.size();
		push_blocks(pl.weld_vblock_job, id, weld_vblocks(v.nvert));
		if(wb.index) {
			w.cblock0 = (uint32_t)pl.weld_cblock_job.v.size();
			push_blocks(pl.weld_cblock_job, id, weld_cblocks(v.nface));
		}
	}
	pl.weld.v.push_back(w);
}

// levels of detail: crthip_batch_bind_lod.  A job a LEVEL: the integer positions as the weld takes them, the index where the automaton leaves it, the
// level's arrays, its clustered triples in scratch; a job whose tables fit LDS needs no more.  The others keep both tables - zeroed by ONE FillJob in
// stage E, so that a second decode starts clean -, a word a block of faces and, if the level has none, a record in scratch.  (The bind call
// checked all of it)
void Planner::lod_jobs(const BlobView &v) {
	const crthip_lod_binding &lb = v.P.derived.lod;
	const bool blob = lod_in_blob(v.nvert, v.nface);
	if(!generic_source_ok(v.P, v.pos_k, 3)) { v.P.host_status = CRTHIP_E_NORMAL_NEEDS_POSITION; return; }
	if(lod_binding_error(&lb, v.nvert, v.nface)) { v.P.host_status = CRTHIP_E_ARGUMENT; return; }
	for(uint32_t k = 0; k < lb.levels; k++) if(v.S.lod[k] == ~0ull) { v.P.host_status = CRTHIP_E_ARGUMENT; return; }
	const LodScratchLayout lay = lod_scratch_layout(v.nvert, v.nface);
	const Faces f = faces_of(v.i);
	for(uint32_t k = 0; k < lb.levels; k++) {
		const crthip_lod_level &lv = lb.level[k];
		const uint64_t S = v.S.lod[k];
		LodJob l{};
		l.position = ints_of(v.i, v.pos_k); l.index = f.p; l.index_u16 = f.u16;
		l.remap = lv.remap; l.lod_index = lv.index; l.counts = lv.counts; l.nface = v.nface; l.nvert = v.nvert; l.shift = lv.shift;
		l.triples = (uint32_t *)SP(S + lay.triples);
		const uint32_t id = (uint32_t)pl.lod.v.size();
		// (a level that a compaction reads needs its record: the set keeps one for a level without)
		if(const int cs = v.P.derived.compact_set_of(CRTHIP_COMPACT_LOD, k); blob && !lv.counts && cs >= 0 && v.S.compact[cs] != ~0ull)
			l.counts = SP(v.S.compact[cs] + compact_layout_of(v.P, v.P.derived.compact.set[cs]).src_record);
		if(blob) {
			pl.lod_blob_ids.v.push_back(id);
			pl.lod_lds = std::max(pl.lod_lds, (uint32_t)(lod_table_slots(v.nvert, v.nface)*4));
		} else {
			l.vtable = (uint32_t *)SP(S + lay.vtable); l.ftable = (uint32_t *)SP(S + lay.ftable); l.blocks = (uint32_t *)SP(S + lay.blocks);
			if(!lv.counts) l.counts = SP(S + lay.record);
			zero_fill(S + lay.vtable, lay.tables_bytes);
			pl.lod_big_ids.v.push_back(id);
			l.vblock0 = (uint32_t)pl.lod_vblock_job.v.size();
			for(uint32_t c = 0; c < weld_vblocks(v.nvert); c++) pl.lod_vblock_job.v.push_back(id);
			l.fblock0 = (uint32_t)pl.lod_fblock_job.v.size();
			for(uint32_t c = 0; c < lod_fblocks(v.nface); c++) pl.lod_fblock_job.v.push_back(id);
		}
		pl.lod.v.push_back(l);
	}
}

// a cloud's levels of detail: crthip_batch_bind_cloud_lod.  A job a LEVEL: the integer positions as the weld takes them and the level's arrays; a job
// whose table fits LDS needs no more.  The others keep the table and the weight words - one range, zeroed by ONE FillJob in stage E, so that a
// second decode starts clean -, a word a block of vertices and, if the level has none, a record in scratch.  A cloud's inverse_job never turns
// integers into floats on its way (that is dequant_job's or quant_job's, in finish()), so view_of has no reader to count: a packed buffer holds
// the integers until k_dequant, a strided, DOUBLE or quantised one keeps them in scratch.  (The bind call checked all of it)
void Planner::cloud_lod_jobs(const BlobView &v) {
	const crthip_cloud_lod_binding &lb = v.P.derived.cloud_lod;
	const bool blob = weld_in_blob(v.nvert);
	if(!generic_source_ok(v.P, v.pos_k, 3)) { v.P.host_status = CRTHIP_E_NORMAL_NEEDS_POSITION; return; }
	if(v.mesh || !v.nvert || cloud_lod_binding_error(&lb, v.nvert)) { v.P.host_status = CRTHIP_E_ARGUMENT; return; }
	for(uint32_t k = 0; k < lb.levels; k++) if(!blob && v.S.cloud_lod[k] == ~0ull) { v.P.host_status = CRTHIP_E_ARGUMENT; return; }
	const CloudLodScratchLayout lay = cloud_lod_scratch_layout(v.nvert);
	for(uint32_t k = 0; k < lb.levels; k++) {
		const crthip_cloud_lod_level &lv = lb.level[k];
		CloudLodJob c{};
		c.position = ints_of(v.i, v.pos_k);
		c.remap = lv.remap; c.points = lv.points; c.weight = lv.weight; c.chunks = lv.chunks; c.counts = lv.counts;
		c.nvert = v.nvert; c.shift = lv.shift; c.chunk_points = lb.chunk_points;
		const uint32_t id = (uint32_t)pl.cloud_lod.v.size();
		if(const int cs = v.P.derived.compact_set_of(CRTHIP_COMPACT_CLOUD_LOD, k); blob && !lv.counts && cs >= 0 && v.S.compact[cs] != ~0ull)
			c.counts = SP(v.S.compact[cs] + compact_layout_of(v.P, v.P.derived.compact.set[cs]).src_record);   // (as lod_jobs)
		if(blob) {
			pl.cloud_lod_blob_ids.v.push_back(id);
			pl.cloud_lod_lds = std::max(pl.cloud_lod_lds, (uint32_t)(weld_slots(v.nvert)*4));
		} else {
			const uint64_t S = v.S.cloud_lod[k];
			c.table = (uint32_t *)SP(S + lay.table); c.wacc = (uint32_t *)SP(S + lay.weights); c.blocks = (uint32_t *)SP(S + lay.blocks);
			if(!lv.counts) c.counts = SP(S + lay.record);
			zero_fill(S + lay.table, lv.weight ? lay.zero_bytes : lay.weights);   // (no weights: the table alone)
			pl.cloud_lod_big_ids.v.push_back(id);
			c.vblock0 = (uint32_t)pl.cloud_lod_vblock_job.v.size();
			push_blocks(pl.cloud_lod_vblock_job, id, weld_vblocks(v.nvert));
			if(lv.chunks) {
				c.cblock0 = (uint32_t)pl.cloud_lod_cblock_job.v.size();
				push_blocks(pl.cloud_lod_cblock_job, id, cloud_lod_chunks_of(v.nvert, lb.chunk_points));
			}
		}
		pl.cloud_lod.v.push_back(c);
	}
}

// compaction: crthip_batch_bind_compact.  A job a MESH set: its id list where its source leaves it - the index where the automaton does, the welded
// index, a level's index with the level's record, which lod_jobs has just given a job -, the set's arrays, and in scratch what it lacks: a record,
// an order for its gathers, beyond compact_blob a newid for its index, the mask - zeroed by ONE FillJob in stage E, so that a second decode starts
// clean - and a word a block of vertices.  And a job a GATHER of every set: the source's own buffer as bound, the set's order (a cloud's: its level's
// points) and the record `used` is read from (a cloud's: its level's `cells`).  (The bind call checked all of it)
void Planner::compact_jobs(const BlobView &v) {
	const crthip_compact_binding &cb = v.P.derived.compact;
	std::string why;
	if(const int err = compact_binding_error(v.P, &cb, why)) { v.P.host_status = err; return; }
	for(uint32_t s = 0; s < cb.sets; s++) if(v.S.compact[s] == ~0ull) { v.P.host_status = CRTHIP_E_ARGUMENT; return; }
	// the record of a named level that has none and whose job keeps none: in the scratch of the FIRST set that names the level (lod_jobs, cloud_lod_jobs)
	auto level_record = [&](uint32_t source, uint32_t level) {
		const int cs = v.P.derived.compact_set_of(source, level);
		return (const uint32_t *)SP(v.S.compact[cs] + compact_layout_of(v.P, cb.set[cs]).src_record);
	};
	for(uint32_t s = 0; s < cb.sets; s++) {
		const crthip_compact_set &t = cb.set[s];
		const uint64_t S = v.S.compact[s];
		const CompactScratchLayout lay = compact_layout_of(v.P, t);
		const bool cloud = t.source == CRTHIP_COMPACT_CLOUD_LOD, clip_v = t.order || t.ngather;
		const uint32_t *order = t.order, *count_rec = nullptr;
		void *rec = t.counts ? (void *)t.counts : (void *)SP(S + lay.record);
		if(cloud) {
			const crthip_cloud_lod_level &lv = v.P.derived.cloud_lod.level[t.level];
			order = lv.points;
			// (the level's record: the caller's, cloud_lod_jobs' in scratch beyond weld_in_blob, or this set's)
			count_rec = lv.counts ? (const uint32_t *)lv.counts : weld_in_blob(v.nvert) ? level_record(t.source, t.level)
				: (const uint32_t *)SP(v.S.cloud_lod[t.level] + cloud_lod_scratch_layout(v.nvert).record);
		} else {
			CompactJob c{};
			const Faces f = faces_of(v.i);
			if(t.source == CRTHIP_COMPACT_INDEX) { c.src = f.p; c.src_u16 = f.u16; }
			else if(t.source == CRTHIP_COMPACT_WELD) c.src = v.P.derived.weld.index;
			else {
				const crthip_lod_level &lv = v.P.derived.lod.level[t.level];
				c.src = lv.index;
				c.src_rec = lv.counts ? (const uint32_t *)lv.counts : lod_in_blob(v.nvert, v.nface) ? level_record(t.source, t.level)
					: (const uint32_t *)SP(v.S.lod[t.level] + lod_scratch_layout(v.nvert, v.nface).record);
			}
			const bool blob = compact_in_blob(v.nvert, v.nface);
			if(!order && t.ngather) order = (const uint32_t *)SP(S + lay.order);
			c.newid = t.newid; c.order = (uint32_t *)order; c.index = t.index; c.counts = rec;
			c.nface = v.nface; c.nvert = v.nvert; c.vcap = t.vertex_capacity; c.icap = t.index_capacity; c.clip_v = clip_v;
			const uint32_t id = (uint32_t)pl.compact.v.size();
			if(blob) pl.compact_blob_ids.v.push_back(id);
			else {
				if(!c.newid && t.index) c.newid = (uint32_t *)SP(S + lay.newid);
				c.mask = (uint32_t *)SP(S + lay.mask); c.blocks = (uint32_t *)SP(S + lay.blocks);
				zero_fill(S + lay.mask, lay.mask_bytes);
				pl.compact_big_ids.v.push_back(id);
				c.vblock0 = (uint32_t)pl.compact_vblock_job.v.size();
				push_blocks(pl.compact_vblock_job, id, compact_vblocks(v.nvert));
				c.cblock0 = (uint32_t)pl.compact_cblock_job.v.size();
				push_blocks(pl.compact_cblock_job, id, compact_cblocks(v.nface));
			}
			pl.compact.v.push_back(c);
			count_rec = (const uint32_t *)rec;
		}
		// (a cloud set's record is stored by its first gather's first workgroup: a set without gathers gets a job of no bytes for it)
		for(uint32_t q = 0; q < t.ngather || (cloud && q == 0 && t.counts); q++) {
			CompactGatherJob g{};
			g.order = order; g.count_rec = count_rec; g.cloud_rec = cloud && q == 0 && t.counts ? rec : nullptr;
			g.vcap = t.vertex_capacity; g.nvert = v.nvert; g.clip_v = clip_v;
			if(q < t.ngather) {
				const CompactSource src = compact_source_of(v.P, t.gather[q].source);
				g.src = (const uint8_t *)src.buffer; g.dst = (uint8_t *)t.gather[q].dst;
				g.E = src.E; g.sstride = src.stride; g.dstride = t.gather[q].dst_stride ? t.gather[q].dst_stride : src.E;
				g.unit = compact_unit((uintptr_t)g.src, (uintptr_t)g.dst, g.E, g.sstride, g.dstride);
			}
			const uint32_t id = (uint32_t)pl.compact_gather.v.size();
			g.block0 = (uint32_t)pl.compact_gblock_job.v.size();
			push_blocks(pl.compact_gblock_job, id, compact_gather_blocks(v.nvert, g.vcap, g.E, g.unit));
			pl.compact_gather.v.push_back(g);
		}
	}
}

// the BVH: crthip_batch_bind_bvh.  The integer positions as the weld takes them, the index where the automaton leaves it, the caller's arrays; a
// blob of up to 4 096 faces needs no more.  The others keep their extent and their arrival counters - zeroed by ONE FillJob in stage E, so that a
// second decode starts clean -, their pairs and the sort's table in scratch, and a parent array there if the binding has none.  (The bind call
// checked all of it)
void Planner::bvh_jobs(const BlobView &v) {
	const crthip_bvh_binding &vb = v.P.derived.bvh;
	const bool blob = bvh_in_blob(v.nface);
	if(!generic_source_ok(v.P, v.pos_k, 3)) { v.P.host_status = CRTHIP_E_NORMAL_NEEDS_POSITION; return; }
	if(bvh_binding_error(&vb, v.nface) || (!blob && v.S.bvh == ~0ull)) { v.P.host_status = CRTHIP_E_ARGUMENT; return; }
	BvhJob j{};
	j.position = ints_of(v.i, v.pos_k);
	const Faces f = faces_of(v.i); j.index = f.p; j.index_u16 = f.u16;
	j.nodes = vb.nodes; j.parent = vb.parent; j.order = vb.order; j.counts = vb.counts; j.nface = v.nface; j.nvert = v.nvert;
	const uint32_t id = (uint32_t)pl.bvh.v.size();
	if(blob) {
		pl.bvh_blob_ids.v.push_back(id);
		pl.bvh_lds = std::max(pl.bvh_lds, bvh_blob_lds_bytes(v.nface));
	} else {
		const BvhScratchLayout lay = bvh_scratch_layout(v.nface, !vb.parent);
		j.scratch = (uint8_t *)SP(v.S.bvh);
		if(!vb.parent) j.parent = (uint32_t *)SP(v.S.bvh + lay.parent);
		zero_fill(v.S.bvh, lay.zero_bytes);
		pl.bvh_big_ids.v.push_back(id);
		j.fblock0 = (uint32_t)pl.bvh_fblock_job.v.size();
		push_blocks(pl.bvh_fblock_job, id, bvh_fblocks(v.nface));
		j.tblock0 = (uint32_t)pl.bvh_tblock_job.v.size();
		push_blocks(pl.bvh_tblock_job, id, bvh_tiles(v.nface));
	}
	pl.bvh.v.push_back(j);
}

// adjacency: crthip_batch_bind_adjacency.  The index where the automaton leaves it - or, under CRTHIP_WELD_ADJACENCY, the welded index of the blob's
// weld binding, which weld_jobs has just given a job - and the caller's twin array; a blob whose lists fit LDS needs no
// more.  The others keep their ends - zeroed by a FillJob in stage E - and their entries in scratch, and a record there if the binding has none.
// (The bind call checked all of it)
void Planner::adjacency_jobs(const BlobView &v) {
	const crthip_adjacency_binding &ab = v.P.derived.adjacency;
	const bool blob = adj_in_blob(v.nvert, v.nface);
	if(adjacency_binding_error(&ab, v.nface) || (!blob && v.S.adj == ~0ull)) { v.P.host_status = CRTHIP_E_ARGUMENT; return; }
	AdjacencyJob a{};
	const Faces f = faces_of(v.i); a.index = f.p; a.index_u16 = f.u16;
	if(welds_adjacency(v.P)) { a.index = v.P.derived.weld.index; a.index_u16 = 0; }
	a.twin = ab.twin; a.counts = ab.counts; a.nface = v.nface; a.nvert = v.nvert;
	const uint32_t id = (uint32_t)pl.adjacency.v.size();
	if(blob) {
		pl.adjacency_blob_ids.v.push_back(id);
		pl.adjacency_lds = std::max(pl.adjacency_lds, (uint32_t)adj_blob_lds(v.nvert, v.nface));
	} else {
		const AdjScratchLayout lay = adj_scratch_layout(v.nvert, v.nface);
		a.ends = (uint32_t *)SP(v.S.adj); a.list = (uint32_t *)SP(v.S.adj + lay.list);
		if(!ab.counts) a.counts = SP(v.S.adj + lay.record);
		zero_fill(v.S.adj, ((uint64_t)v.nvert + 1)*4);
		pl.adj_big_ids.v.push_back(id);
		a.block0 = (uint32_t)pl.adj_block_job.v.size();
		push_blocks(pl.adj_block_job, id, adj_blocks(v.nface));
	}
	pl.adjacency.v.push_back(a);
}
