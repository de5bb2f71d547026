// cloud_lod.h — crthip_batch_bind_cloud_lod: levels of detail of a point cloud (include/corto_hip.h has the contract).  One LEVEL of one blob is
// one job: the points are clustered by the grid cell of their integer position as lod.h clusters a mesh's vertices, the least vertex of every cell
// is kept, in vertex order, with the number of points it stands for, and every run of K kept points gets the box of their positions.  The method,
// the phases and both partitions as __host__ __device__ code over lod.h's workgroup abstraction, so that the host runs the very same source in
// the kernels' partitions (crthip_cloud_lod_model, cloud_lod_host.cpp).
//
//   method   lod.h's, taken from there without a copy: lod_insert and lod_lookup over LodCellOf, on weld.h's two tables; block_sum and
//            block_scan of its workgroup.  New here: the compaction of the kept VERTICES, the weights, the boxes, the record.
//   compact  order-preserving, as lod.h's over faces: a block scan of the kept flags (remap[v] == v) a round of 256 vertices;
//            cloud_lod_blob carries a running base, partition 1 takes the block's base from cloud_lod_offsets' exclusive scan of the
//            block counts that cloud_lod_lookup left.  No look-back, no spinning.
//   weights  sums, one atomic add a point on a word a VERTEX (its representative's): a sum does not depend on the order of the atomics.
//              partition 0  in LDS, in the TABLE'S OWN WORDS: behind the lookup the table is free, and its T >= 2*nvert words hold nvert
//                           weight words.  No LDS beside the table, so the request stays the weld's and two workgroups still share a CU
//              partition 1  nvert words of blob scratch behind the table, zeroed by the same FillJob, agent-scope atomics in cloud_lod_lookup
//            NOBODY HAS MEASURED either against the other, or against adding a wave's equal representatives up before the atomic: chosen, not
//            varied (profiles/cloud_lod.md says what was measured).
//   boxes    six words a chunk in LDS - the table's words once more in partition 0, six words of its own a workgroup of cloud_lod_chunks -
//            started at the empty box and lowered / raised by one atomic minimum / maximum a component.  A thread keeps a box of its own
//            while its points stay in one chunk and sends it when the chunk changes: 6 atomics a thread and chunk, not 6 a point.  Minimum and
//            maximum: no byte depends on the order.
//   memory   a position is read from memory wherever a walk compares one (weld.h) and once more for its box.
//   group    lod.h's G.  A value every thread needs outside thread 0 (the kept count) is carried in every lane's `run`, which block_scan's t
//            keeps equal in all of them.
#pragma once
#include "lod.h"

namespace corto_hip {

constexpr uint32_t CLOUD_LOD_CHUNK_MIN = 32, CLOUD_LOD_CHUNK_MAX = 65536;
static_assert(CRTHIP_CLOUD_LOD_MAX_LEVELS == 4 && sizeof(crthip_cloud_lod_level) == 56 && sizeof(crthip_cloud_lod_binding) == 240 &&
              sizeof(crthip_cloud_chunk) == 32 && sizeof(crthip_cloud_lod_counts) == 16, "crthip_batch_bind_cloud_lod's layout");

WELD_HD uint32_t cloud_lod_chunks_of(uint32_t n, uint32_t K) { return K ? (uint32_t)(((uint64_t)n + K - 1)/K) : 0u; }
// a job beyond weld_in_blob keeps in scratch: the table and the weight words (one range, zeroed by one FillJob), a word a block of vertices, and
// a record for a level without one (cloud_lod_chunks reads `cells` from it)
struct CloudLodScratchLayout { uint64_t table, weights, zero_bytes, blocks, record, total; };
WELD_HD CloudLodScratchLayout cloud_lod_scratch_layout(uint32_t nvert) {
	CloudLodScratchLayout l;
	uint64_t o = 0;
	l.table = o; o += weld_slots(nvert)*4;
	l.weights = o; o += ((uint64_t)nvert*4 + 15) & ~15ull;
	l.zero_bytes = o;
	l.blocks = o; o += ((uint64_t)weld_vblocks(nvert)*4 + 15) & ~15ull;
	l.record = o; o += 16;
	l.total = weld_in_blob(nvert) ? 0 : o;
	return l;
}
// partition 0 keeps its boxes in the table's words: 6*ceil(nvert/32) <= weld_slots(nvert) = max(64, 2*nvert rounded up) - 6 <= 64 up to 32
// points, 12 <= 66 up to 64, and 0.1875*nvert + 6 <= 2*nvert beyond
static_assert(6*((8192 + CLOUD_LOD_CHUNK_MIN - 1)/CLOUD_LOD_CHUNK_MIN) <= WELD_BLOB_LDS_MAX/4/2, "the boxes fit the table");

// ---- the words the atomics land on ---------------------------------------------------------------------------------------------------------------

WELD_HD void cloud_lds_add(WELD_LDS uint32_t *w, uint32_t c) {
#if WELD_DEVICE_PASS
	(void)__hip_atomic_fetch_add(w, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#else
	*w += c;
#endif
}
WELD_HD void cloud_mem_add(WELD_MEM uint32_t *w, uint32_t c) {
#if WELD_DEVICE_PASS
	(void)__hip_atomic_fetch_add(w, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
	*w += c;
#endif
}
WELD_HD void cloud_lds_lower(WELD_LDS int32_t *w, int32_t x) {
#if WELD_DEVICE_PASS
	(void)__hip_atomic_fetch_min(w, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#else
	if(x < *w) *w = x;
#endif
}
WELD_HD void cloud_lds_raise(WELD_LDS int32_t *w, int32_t x) {
#if WELD_DEVICE_PASS
	(void)__hip_atomic_fetch_max(w, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#else
	if(x > *w) *w = x;
#endif
}

// ---- the boxes -----------------------------------------------------------------------------------------------------------------------------------

struct CloudBox { int32_t x0, y0, z0, x1, y1, z1; };
WELD_HD CloudBox cloud_box_empty() { return CloudBox{INT32_MAX, INT32_MAX, INT32_MAX, INT32_MIN, INT32_MIN, INT32_MIN}; }
WELD_HD void cloud_box_start(WELD_LDS int32_t *a) { a[0] = a[1] = a[2] = INT32_MAX; a[3] = a[4] = a[5] = INT32_MIN; }
WELD_HD void cloud_box_send(WELD_LDS int32_t *a, const CloudBox &b) {
	cloud_lds_lower(a, b.x0); cloud_lds_lower(a + 1, b.y0); cloud_lds_lower(a + 2, b.z0);
	cloud_lds_raise(a + 3, b.x1); cloud_lds_raise(a + 4, b.y1); cloud_lds_raise(a + 5, b.z1);
}
// thread tid's share of the kept points [j0, j1): j0 + tid, + LOD_THREADS, ...; point j belongs to chunk j / K, whose six words are at
// acc + 6*(j/K - c0).  Every points[j] is a vertex: the compaction wrote it
WELD_HD void cloud_boxes_thread(const LodIn &J, WELD_MEM const uint32_t *points, WELD_LDS int32_t *acc, uint32_t tid, uint64_t j0, uint64_t j1, uint32_t K, uint32_t c0) {
	CloudBox b = cloud_box_empty();
	uint32_t cur = 0; bool any = false;
	for(uint64_t j = j0 + tid; j < j1; j += LOD_THREADS) {
		const uint32_t c = (uint32_t)j/K;                                      // (j < cells <= nvert: 32 bits)
		if(any && c != cur) { cloud_box_send(acc + (uint64_t)(cur - c0)*6, b); b = cloud_box_empty(); }
		cur = c; any = true;
		const WeldPos p = weld_pos(J.w, points[j]);
		const int32_t x = (int32_t)p.x, y = (int32_t)p.y, z = (int32_t)p.z;
		b.x0 = x < b.x0 ? x : b.x0; b.y0 = y < b.y0 ? y : b.y0; b.z0 = z < b.z0 ? z : b.z0;
		b.x1 = x > b.x1 ? x : b.x1; b.y1 = y > b.y1 ? y : b.y1; b.z1 = z > b.z1 ? z : b.z1;
	}
	if(any) cloud_box_send(acc + (uint64_t)(cur - c0)*6, b);
}
// chunk c of a level with `cells` kept points, from its six final words: two 16-byte stores
WELD_HD void cloud_chunk_store(WELD_MEM crthip_cloud_chunk *chunks, WELD_LDS const int32_t *a, uint32_t c, uint32_t K, uint32_t cells) {
	const uint64_t first = (uint64_t)c*K;
	const uint32_t count = cells - first < K ? (uint32_t)(cells - first) : K;
#if WELD_DEVICE_PASS
	WELD_MEM weld_u32x4 *o = (WELD_MEM weld_u32x4 *)(chunks + c);
	o[0] = weld_u32x4{(uint32_t)a[0], (uint32_t)a[1], (uint32_t)a[2], (uint32_t)first};
	o[1] = weld_u32x4{(uint32_t)a[3], (uint32_t)a[4], (uint32_t)a[5], count};
#else
	chunks[c] = crthip_cloud_chunk{{a[0], a[1], a[2]}, (uint32_t)first, {a[3], a[4], a[5]}, count};
#endif
}

// the record, written whole by the one workgroup that knows `cells`: cloud_lod_blob's, or cloud_lod_offsets'
WELD_HD void cloud_record_store(WELD_MEM crthip_cloud_lod_counts *rec, uint32_t nvert, uint32_t cells, uint32_t chunks) {
#if WELD_DEVICE_PASS
	*(WELD_MEM weld_u32x4 *)rec = weld_u32x4{nvert, cells, chunks, 0u};
#else
	*rec = crthip_cloud_lod_counts{nvert, cells, chunks, 0u};
#endif
}

// ---- the phases ----------------------------------------------------------------------------------------------------------------------------------

// a point to its representative's weight word, in LDS (remap is final: behind a barrier)
template <class G> WELD_HD void cloud_weigh_lds(G &g, uint32_t nvert, WELD_MEM const uint32_t *remap, WELD_LDS uint32_t *w) {
	g.each([&](uint32_t tid, LodLane &) { for(uint64_t v = tid; v < nvert; v += LOD_THREADS) cloud_lds_add(w + remap[v], 1u); });
}
// ... in scratch: a thread reads the remap words it stored itself
template <class G> WELD_HD void cloud_weigh_mem(G &g, WELD_MEM const uint32_t *remap, WELD_MEM uint32_t *w, uint32_t v0, uint32_t v1) {
	g.each([&](uint32_t tid, LodLane &) { for(uint64_t v = (uint64_t)v0 + tid; v < v1; v += LOD_THREADS) cloud_mem_add(w + remap[v], 1u); });
}
// the round of 256 vertices from v0: the kept ones to points (and their weight words to weight) from `base + L.run` on; L.run grows by the
// round's kept count in every lane.  W: where the weight words are (LDS or memory); weight null: no weights
template <class G, class W> WELD_HD void cloud_compact_round(G &g, uint32_t nvert, WELD_MEM const uint32_t *remap, W w, WELD_MEM uint32_t *points, WELD_MEM uint32_t *weight,
	uint64_t v0, uint32_t base) {
	g.each([&](uint32_t tid, LodLane &L) { const uint64_t v = v0 + tid; L.c = v < nvert && remap[v] == (uint32_t)v; });
	g.block_scan();
	g.each([&](uint32_t tid, LodLane &L) {
		if(L.c) {
			const uint32_t at = base + L.run + L.x;
			points[at] = (uint32_t)(v0 + tid);
			if(weight) weight[at] = w[v0 + tid];
		}
		L.run += L.t;
	});
}

// ---- partition 0: a job by ONE workgroup, the table in LDS, its words used three times (the table; the weight words; the boxes).  weight, chunks
// and rec may be null; K is read only with chunks ----------------------------------------------------------------------------------------------------

template <class G> WELD_HD void cloud_lod_blob(G &g, const LodIn &J, const WeldLdsTable &tb, uint32_t K, WELD_MEM uint32_t *remap, WELD_MEM uint32_t *points,
	WELD_MEM uint32_t *weight, WELD_MEM crthip_cloud_chunk *chunks, WELD_MEM crthip_cloud_lod_counts *rec, LodStats *stats) {
	const uint32_t nvert = J.w.nvert;
	const uint64_t T = weld_slots(nvert);
	g.each([&](uint32_t tid, LodLane &) { for(uint64_t s = tid; s < T; s += LOD_THREADS) tb.put(s, 0u); });
	g.sync();
	lod_insert(g, J, tb, T, 0, nvert, stats);
	g.sync();
	lod_lookup(g, J, tb, T, remap, 0, nvert);
	g.sync();                                                                  // (remap is read below by other threads than wrote it; the table is free)
	if(weight) {
		g.each([&](uint32_t tid, LodLane &) { for(uint64_t s = tid; s < nvert; s += LOD_THREADS) tb.put(s, 0u); });
		g.sync();
		cloud_weigh_lds(g, nvert, remap, tb.t);
		g.sync();
	}
	g.each([&](uint32_t, LodLane &L) { L.run = 0; });
	for(uint64_t v0 = 0; v0 < nvert; v0 += LOD_THREADS) cloud_compact_round(g, nvert, remap, (WELD_LDS const uint32_t *)tb.t, points, weight, v0, 0u);
	// (every lane's run is `cells` now)
	if(chunks) {
		WELD_LDS int32_t *acc = (WELD_LDS int32_t *)tb.t;
		g.sync();                                                              // (the weight words have been read; points is read below by other threads than wrote it)
		g.each([&](uint32_t tid, LodLane &L) { for(uint32_t c = tid; c < cloud_lod_chunks_of(L.run, K); c += LOD_THREADS) cloud_box_start(acc + (uint64_t)c*6); });
		g.sync();
		g.each([&](uint32_t tid, LodLane &L) { cloud_boxes_thread(J, points, acc, tid, 0, L.run, K, 0u); });
		g.sync();
		g.each([&](uint32_t tid, LodLane &L) { for(uint32_t c = tid; c < cloud_lod_chunks_of(L.run, K); c += LOD_THREADS) cloud_chunk_store(chunks, acc + (uint64_t)c*6, c, K, L.run); });
	}
	g.thread0([&](LodLane &L) { if(rec) cloud_record_store(rec, nvert, L.run, chunks ? cloud_lod_chunks_of(L.run, K) : 0u); });
}

// ---- partition 1: workgroup k of a job's ceil(nvert/LOD_BLOCK) in cloud_lod_insert / _lookup / _scatter, one workgroup a job in cloud_lod_offsets,
// workgroup c of its ceil(nvert/K) in cloud_lod_chunks.  rec is never null here (the planner gives a level without a record one in scratch) -----------

template <class G> WELD_HD void cloud_lod_insert_block(G &g, const LodIn &J, const WeldMemTable &tb, uint32_t k, LodStats *stats) {
	lod_insert(g, J, tb, weld_slots(J.w.nvert), k*LOD_BLOCK, (uint32_t)weld_block_end(J.w.nvert, k), stats);
}
// remap, the block's kept count to its word, and (wacc not null) a point to its representative's weight word
template <class G> WELD_HD void cloud_lod_lookup_block(G &g, const LodIn &J, const WeldMemTable &tb, WELD_MEM uint32_t *remap, WELD_MEM uint32_t *blocks, WELD_MEM uint32_t *wacc, uint32_t k) {
	const uint32_t v0 = k*LOD_BLOCK, v1 = (uint32_t)weld_block_end(J.w.nvert, k);
	lod_lookup(g, J, tb, weld_slots(J.w.nvert), remap, v0, v1);
	g.thread0([&](LodLane &L) { blocks[k] = L.c; });
	if(wacc) cloud_weigh_mem(g, remap, wacc, v0, v1);
}
// the exclusive scan of a job's block counts, in place, and the record: the total is `cells`
template <class G> WELD_HD void cloud_lod_offsets_job(G &g, uint32_t nvert, uint32_t K, bool chunks, WELD_MEM uint32_t *blocks, WELD_MEM crthip_cloud_lod_counts *rec) {
	const uint32_t nb = weld_vblocks(nvert);
	g.each([&](uint32_t, LodLane &L) { L.run = 0; });
	for(uint64_t b0 = 0; b0 < nb; b0 += LOD_THREADS) {
		g.each([&](uint32_t tid, LodLane &L) { L.c = b0 + tid < nb ? blocks[b0 + tid] : 0u; });
		g.block_scan();
		g.each([&](uint32_t tid, LodLane &L) {
			if(b0 + tid < nb) blocks[b0 + tid] = L.run + L.x;
			L.run += L.t;
		});
	}
	g.thread0([&](LodLane &L) { cloud_record_store(rec, nvert, L.run, chunks ? cloud_lod_chunks_of(L.run, K) : 0u); });
}
template <class G> WELD_HD void cloud_lod_scatter_block(G &g, uint32_t nvert, WELD_MEM const uint32_t *remap, WELD_MEM const uint32_t *blocks, WELD_MEM const uint32_t *wacc,
	WELD_MEM uint32_t *points, WELD_MEM uint32_t *weight, uint32_t k) {
	g.each([&](uint32_t, LodLane &L) { L.run = 0; });
	cloud_compact_round(g, nvert, remap, wacc, points, weight, (uint64_t)k*LOD_BLOCK, blocks[k]);
}
// chunk c: `cells` is read from the record cloud_lod_offsets stored; a workgroup past the level's chunks has nothing to do.  acc: six words of LDS
template <class G> WELD_HD void cloud_lod_chunk_block(G &g, const LodIn &J, uint32_t K, WELD_MEM const uint32_t *points, WELD_MEM const crthip_cloud_lod_counts *rec,
	WELD_MEM crthip_cloud_chunk *chunks, WELD_LDS int32_t *acc, uint32_t c) {
	const uint32_t cells = rec->cells;
	const uint64_t first = (uint64_t)c*K;
	if(first >= cells) return;
	const uint64_t end = first + K < cells ? first + K : cells;
	g.thread0([&](LodLane &) { cloud_box_start(acc); });
	g.sync();
	g.each([&](uint32_t tid, LodLane &) { cloud_boxes_thread(J, points, acc, tid, first, end, K, c); });
	g.sync();
	g.thread0([&](LodLane &) { cloud_chunk_store(chunks, acc, c, K, cells); });
}

// what crthip_batch_bind_cloud_lod (and the hook) ask of a binding on a cloud of nvert points, behind "no such blob", "not a point cloud" and "no
// points", in the header's order; null: fine
inline const char *cloud_lod_binding_error(const crthip_cloud_lod_binding *l, uint32_t nvert) {
	if(l->levels < 1 || l->levels > CRTHIP_CLOUD_LOD_MAX_LEVELS) return "cloud lod: levels is not in 1..CRTHIP_CLOUD_LOD_MAX_LEVELS";
	const uint32_t K = l->chunk_points;
	if(K && (K < CLOUD_LOD_CHUNK_MIN || K > CLOUD_LOD_CHUNK_MAX)) return "cloud lod: chunk_points is neither 0 nor in 32..65536";
	for(uint32_t k = 0; k < l->levels; k++) if(!K && l->level[k].chunks) return "cloud lod: chunk_points is 0 and a level has chunks";
	for(uint32_t k = 0; k < l->levels; k++) {
		const crthip_cloud_lod_level &v = l->level[k];
		if(!v.remap || (uintptr_t)v.remap % 4 || !v.points || (uintptr_t)v.points % 4) return "cloud lod: a level's remap or points is NULL or not 4-byte aligned";
		if((uintptr_t)v.weight % 4) return "cloud lod: a level's weight is not 4-byte aligned";
		if((uintptr_t)v.chunks % 16 || (uintptr_t)v.counts % 16) return "cloud lod: a level's chunks or counts is not 16-byte aligned";
		if(v.capacity < nvert) return "cloud lod: a level's capacity is below nvert";
		if(v.chunks && v.chunks_capacity < cloud_lod_chunks_of(nvert, K)) return "cloud lod: a level's chunks_capacity is below ceil(nvert / chunk_points)";
		if(v.shift > 31) return "cloud lod: a level's shift is above 31";
		if(k && v.shift <= l->level[k - 1].shift) return "cloud lod: a level's shift is not above the level's before";
		if(v.reserved) return "cloud lod: a level's reserved is not 0";
	}
	if(l->flags) return "cloud lod: unknown flag bits";
	if(l->reserved) return "cloud lod: reserved is not 0";
	return nullptr;
}

} // namespace corto_hip
