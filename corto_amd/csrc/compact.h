// compact.h — crthip_batch_bind_compact: a level's own vertex buffers (include/corto_hip.h has the contract).  One SET of one blob is one job: the
// vertices an id list uses are marked, counted and renumbered 0..used-1 in vertex order, the id list is rewritten through the new numbers, and
// the blob's final vertex outputs of the used vertices are copied into compact arrays.  The method, the phases and both partitions as
// __host__ __device__ code over lod.h's workgroup abstraction, so that the host runs the very same source in the kernels' partitions
// (crthip_compact_model, compact_host.cpp).
//
//   method   a BITMASK of the used vertices, a bit a vertex, built with one atomic OR a corner: an OR does not depend on the order of the
//            atomics.  A vertex's new id is the number of set bits below its own: the exclusive scan of the popcounts up to its word or block
//            plus the popcount of the bits below it inside.  Ascending order keeps the decoder's own vertex order and makes every byte
//            independent of any execution order.
//              partition 0  the mask and the exclusive scan of its WORDS' popcounts in LDS (a thread a word: 8 192 vertices are 256 words, one
//                           round of block_scan); a new id is pre[v >> 5] + popcount(mask[v >> 5] below bit v & 31), for the newid / order stores and for
//                           the index alike - no newid array is read back
//              partition 1  the mask in scratch (zeroed by ONE FillJob in stage E), a word a block of 256 vertices for the block's popcount, then
//                           its base (compact_offsets' exclusive scan, in rounds of 256 blocks); compact_place makes a block's new ids with one
//                           block_scan of its 256 bits; compact_index reads newid (the caller's array, or scratch where the set has none)
//            No look-back, no spinning: the kernels' order on the stream is the only dependency.
//   F        the faces a set reads are the source's OWN count: a LOD level's `faces` is read on the device from the level's record (word 1),
//            clamped to the bound nface the grids and the arrays were sized from; threads beyond 3*F leave.
//   ids      an id >= nvert is compared and never used as an address: it marks nothing and becomes CRTHIP_NO_VERTEX in the index.
//   clip     order[j] is stored for j < vertex_capacity, index[k] for k < index_capacity; the record says whether anything was left out.
//   gather   compact_gather, behind every kernel that writes a final vertex byte (Planner::finish): a thread copies ONE UNIT of one record;
//            adjacent lanes take adjacent units of a record and then the next record, so the stores coalesce, and since order ascends the
//            reads walk forward through the source.  The unit is chosen a gather when the job is planned (compact_unit): 16 bytes where E, both
//            strides and both pointers are multiples of 16, else 4, 2 or 1 by the same test.  CHOSEN, NOT TUNED (profiles/compact.md).
//   group    lod.h's G.  A value every thread needs (the used count) is carried in every lane's `run`, which block_scan's t keeps equal in all
//            of them.
#pragma once
#include "lod.h"

namespace corto_hip {

static_assert(CRTHIP_COMPACT_MAX_SETS == 4 && CRTHIP_COMPACT_MAX_GATHERS == 8 && sizeof(crthip_compact_counts) == 16 && sizeof(crthip_compact_gather) == 16 &&
              sizeof(crthip_compact_set) == 192 && sizeof(crthip_compact_binding) == 784 && sizeof(crthip_compact_model_gather) == 32, "crthip_batch_bind_compact's layout");

constexpr uint32_t COMPACT_THREADS = LOD_THREADS, COMPACT_BLOCK = LOD_BLOCK;
// compact_blob's limit: a set of up to this many vertices AND bound faces.  It is the levels' threshold (lod_in_blob), so that a level and its
// compaction change partitions together, and AS UNMEASURED AS THEIRS: chosen, not varied (profiles/compact.md says what was measured)
constexpr uint32_t COMPACT_BLOB_MAX = 8192;
constexpr uint32_t COMPACT_BLOB_WORDS = COMPACT_BLOB_MAX/32;                // 256: a thread a mask word
static_assert(COMPACT_BLOB_WORDS == COMPACT_THREADS, "one round of block_scan covers compact_blob's mask");

WELD_HD bool compact_in_blob(uint32_t nvert, uint32_t nface) { return nvert <= COMPACT_BLOB_MAX && nface <= COMPACT_BLOB_MAX; }
WELD_HD uint32_t compact_words(uint32_t nvert) { return (uint32_t)(((uint64_t)nvert + 31)/32); }
WELD_HD uint32_t compact_vblocks(uint32_t nvert) { return (uint32_t)(((uint64_t)nvert + COMPACT_BLOCK - 1)/COMPACT_BLOCK); }
WELD_HD uint32_t compact_cblocks(uint32_t nface) { return weld_cblocks(nface); }
// what a set keeps in scratch: a record where the caller gives none, a record for a named level that has none, newid and order where a later
// kernel reads them and the caller gives none, and beyond compact_blob the mask (zeroed by a FillJob) and a word a block of vertices
struct CompactScratchLayout { uint64_t record, src_record, mask, mask_bytes, blocks, newid, order, total; };
WELD_HD CompactScratchLayout compact_scratch_layout(uint32_t nvert, uint32_t nface, bool cloud, bool own_newid, uint32_t own_order_words) {
	CompactScratchLayout l;
	uint64_t o = 0;
	l.record = o; o += 16;
	l.src_record = o; o += 16;
	l.mask = l.blocks = l.newid = o; l.mask_bytes = 0;
	if(!cloud && !compact_in_blob(nvert, nface)) {
		l.mask_bytes = ((uint64_t)compact_words(nvert)*4 + 15) & ~15ull;
		l.mask = o; o += l.mask_bytes;
		l.blocks = o; o += ((uint64_t)compact_vblocks(nvert)*4 + 15) & ~15ull;
		l.newid = o; if(own_newid) o += ((uint64_t)nvert*4 + 15) & ~15ull;
	}
	l.order = o; o += ((uint64_t)own_order_words*4 + 15) & ~15ull;
	l.total = o;
	return l;
}

// the copy unit of a gather: the largest of 16, 4, 2, 1 that divides E, both strides and both addresses
WELD_HD uint32_t compact_unit(uint64_t src, uint64_t dst, uint32_t E, uint32_t sstride, uint32_t dstride) {
	const uint64_t all = src | dst | E | sstride | dstride;
	return !(all & 15) ? 16u : !(all & 3) ? 4u : !(all & 1) ? 2u : 1u;
}

// ---- the words the atomics land on ---------------------------------------------------------------------------------------------------------------

WELD_HD void compact_lds_or(WELD_LDS uint32_t *w, uint32_t bits) {
#if WELD_DEVICE_PASS
	(void)__hip_atomic_fetch_or(w, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#else
	*w |= bits;
#endif
}
WELD_HD void compact_mem_or(WELD_MEM uint32_t *w, uint32_t bits) {
#if WELD_DEVICE_PASS
	(void)__hip_atomic_fetch_or(w, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
	*w |= bits;
#endif
}
WELD_HD uint32_t compact_popc(uint32_t x) { return (uint32_t)__builtin_popcount(x); }
WELD_HD uint32_t compact_below(uint32_t word, uint32_t v) { return compact_popc(word & ((1u << (v & 31u)) - 1u)); }   // set bits below v's own

// ---- the inputs ----------------------------------------------------------------------------------------------------------------------------------

// a mesh set.  J: weld.h's reader of the id list (index, index_u16, nvert; nface is the BOUND).  src_rec: the record whose word 1 is F, or null:
// F = nface.  newid, order, index may be null; rec is never null in partition 1 and may be null in partition 0 only where nothing reads it later
struct CompactIn {
	WeldIn w;
	WELD_MEM const uint32_t *src_rec;
	uint32_t vcap, icap;           // vertex_capacity, index_capacity
	uint32_t clip_v;               // the set has an order or a gather: used > vcap leaves something out
};
// F, as every kernel of a set reads it: never beyond the bound
WELD_HD uint32_t compact_faces(const CompactIn &J) {
	if(!J.src_rec) return J.w.nface;
	const uint32_t f = J.src_rec[1];
	return f < J.w.nface ? f : J.w.nface;
}
WELD_HD void compact_record_store(WELD_MEM crthip_compact_counts *rec, uint32_t nvert, uint32_t used, uint32_t faces, uint32_t clipped) {
#if WELD_DEVICE_PASS
	*(WELD_MEM weld_u32x4 *)rec = weld_u32x4{nvert, used, faces, clipped};
#else
	*rec = crthip_compact_counts{nvert, used, faces, clipped};
#endif
}
WELD_HD uint32_t compact_clipped(const CompactIn &J, bool has_index, uint32_t used, uint32_t F) {
	return ((J.clip_v && used > J.vcap) || (has_index && (uint64_t)F*3 > J.icap)) ? 1u : 0u;
}

// ---- partition 0: a set by ONE workgroup; mask and pre are COMPACT_BLOB_WORDS words of LDS each ---------------------------------------------------

template <class G> WELD_HD void compact_blob(G &g, const CompactIn &J, WELD_LDS uint32_t *mask, WELD_LDS uint32_t *pre, WELD_MEM uint32_t *newid, WELD_MEM uint32_t *order,
	WELD_MEM uint32_t *index, WELD_MEM crthip_compact_counts *rec) {
	const uint32_t nvert = J.w.nvert, W = compact_words(nvert), F = compact_faces(J);
	const uint64_t K = (uint64_t)F*3;
	g.each([&](uint32_t tid, LodLane &) { if(tid < W) mask[tid] = 0u; });
	g.sync();
	g.each([&](uint32_t tid, LodLane &) {
		for(uint64_t k = tid; k < K; k += COMPACT_THREADS) {
			const uint32_t id = weld_corner(J.w, k);
			if(id < nvert) compact_lds_or(mask + (id >> 5), 1u << (id & 31u));
		}
	});
	g.sync();
	g.each([&](uint32_t tid, LodLane &L) { L.c = tid < W ? compact_popc(mask[tid]) : 0u; });
	g.block_scan();
	g.each([&](uint32_t tid, LodLane &L) { if(tid < W) pre[tid] = L.x; L.run = L.t; });   // (every lane's run is `used` now)
	g.sync();
	if(newid || order) g.each([&](uint32_t tid, LodLane &) {
		for(uint64_t v = tid; v < nvert; v += COMPACT_THREADS) {
			const uint32_t m = mask[v >> 5];
			const bool used = (m >> (v & 31u)) & 1u;
			const uint32_t id = pre[v >> 5] + compact_below(m, (uint32_t)v);
			if(newid) newid[v] = used ? id : CRTHIP_NO_VERTEX;
			if(order && used && id < J.vcap) order[id] = (uint32_t)v;
		}
	});
	if(index) g.each([&](uint32_t tid, LodLane &) {
		const uint64_t end = K < J.icap ? K : J.icap;
		for(uint64_t k = tid; k < end; k += COMPACT_THREADS) {
			const uint32_t id = weld_corner(J.w, k);
			index[k] = id < nvert ? pre[id >> 5] + compact_below(mask[id >> 5], id) : CRTHIP_NO_VERTEX;
		}
	});
	g.thread0([&](LodLane &L) { if(rec) compact_record_store(rec, nvert, L.run, F, compact_clipped(J, index != nullptr, L.run, F)); });
}

// ---- partition 1: workgroup k of a set's ceil(3*nface/256) in compact_mark / _index, of its ceil(nvert/256) in compact_count / _place; one
// workgroup a set in compact_offsets.  mask: ceil(nvert/32) words, zeroed in front; blocks: a word a block of vertices ------------------------------

template <class G> WELD_HD void compact_mark_block(G &g, const CompactIn &J, WELD_MEM uint32_t *mask, uint32_t k) {
	const uint64_t K = (uint64_t)compact_faces(J)*3;
	g.each([&](uint32_t tid, LodLane &) {
		const uint64_t c = (uint64_t)k*COMPACT_BLOCK + tid;
		if(c >= K) return;
		const uint32_t id = weld_corner(J.w, c);
		if(id < J.w.nvert) compact_mem_or(mask + (id >> 5), 1u << (id & 31u));
	});
}
// a vertex's bit, by its own thread (the mask is final: the kernel before)
WELD_HD uint32_t compact_bit(WELD_MEM const uint32_t *mask, uint32_t nvert, uint64_t v) { return v < nvert ? (mask[v >> 5] >> (v & 31u)) & 1u : 0u; }
template <class G> WELD_HD void compact_count_block(G &g, uint32_t nvert, WELD_MEM const uint32_t *mask, WELD_MEM uint32_t *blocks, uint32_t k) {
	// (a thread a mask word of the block's eight: their popcounts are the block's)
	g.each([&](uint32_t tid, LodLane &L) {
		const uint64_t w = (uint64_t)k*(COMPACT_BLOCK/32) + tid;
		L.c = tid < COMPACT_BLOCK/32 && w < compact_words(nvert) ? compact_popc(mask[w]) : 0u;
	});
	g.block_sum();
	g.thread0([&](LodLane &L) { blocks[k] = L.c; });
}
// the exclusive scan of a set's block counts, in place, and the record: the total is `used`
template <class G> WELD_HD void compact_offsets_job(G &g, const CompactIn &J, bool has_index, WELD_MEM uint32_t *blocks, WELD_MEM crthip_compact_counts *rec) {
	const uint32_t nb = compact_vblocks(J.w.nvert);
	g.each([&](uint32_t, LodLane &L) { L.run = 0; });
	for(uint64_t b0 = 0; b0 < nb; b0 += COMPACT_THREADS) {
		g.each([&](uint32_t tid, LodLane &L) { L.c = b0 + tid < nb ? blocks[b0 + tid] : 0u; });
		g.block_scan();
		g.each([&](uint32_t tid, LodLane &L) {
			if(b0 + tid < nb) blocks[b0 + tid] = L.run + L.x;
			L.run += L.t;
		});
	}
	g.thread0([&](LodLane &L) { const uint32_t F = compact_faces(J); compact_record_store(rec, J.w.nvert, L.run, F, compact_clipped(J, has_index, L.run, F)); });
}
template <class G> WELD_HD void compact_place_block(G &g, const CompactIn &J, WELD_MEM const uint32_t *mask, WELD_MEM const uint32_t *blocks, WELD_MEM uint32_t *newid,
	WELD_MEM uint32_t *order, uint32_t k) {
	g.each([&](uint32_t tid, LodLane &L) { L.c = compact_bit(mask, J.w.nvert, (uint64_t)k*COMPACT_BLOCK + tid); });
	g.block_scan();
	g.each([&](uint32_t tid, LodLane &L) {
		const uint64_t v = (uint64_t)k*COMPACT_BLOCK + tid;
		if(v >= J.w.nvert) return;
		const uint32_t id = blocks[k] + L.x;
		if(newid) newid[v] = L.c ? id : CRTHIP_NO_VERTEX;
		if(order && L.c && id < J.vcap) order[id] = (uint32_t)v;
	});
}
// (newid is final: the kernel before; never null for a set with an index)
template <class G> WELD_HD void compact_index_block(G &g, const CompactIn &J, WELD_MEM const uint32_t *newid, WELD_MEM uint32_t *index, uint32_t k) {
	const uint64_t K = (uint64_t)compact_faces(J)*3, end = K < J.icap ? K : J.icap;
	g.each([&](uint32_t tid, LodLane &) {
		const uint64_t c = (uint64_t)k*COMPACT_BLOCK + tid;
		if(c >= end) return;
		const uint32_t id = weld_corner(J.w, c);
		index[c] = id < J.w.nvert ? newid[id] : CRTHIP_NO_VERTEX;
	});
}

// ---- the gather: workgroup k of a gather's ceil(min(vertex_capacity, nvert)*units/256), at least one -----------------------------------------------

// count_rec: the record whose word 1 is `used` (the set's own; a cloud's: its level's, `cells`).  order: the set's (a cloud's: its level's points);
// every order[j], j < used, is a vertex.  cloud_rec (a cloud set's first gather only, else null): the set's record, which no other kernel writes
struct CompactGatherIn {
	WELD_MEM const uint8_t *src; WELD_MEM uint8_t *dst;
	WELD_MEM const uint32_t *order, *count_rec;
	WELD_MEM crthip_compact_counts *cloud_rec;
	uint32_t E, sstride, dstride, unit, vcap, nvert, clip_v;
};
WELD_HD void compact_copy_unit(WELD_MEM const uint8_t *s, WELD_MEM uint8_t *d, uint32_t unit) {
	if(unit == 16) *(WELD_MEM weld_u32x4 *)d = *(WELD_MEM const weld_u32x4 *)s;
	else if(unit == 4) *(WELD_MEM uint32_t *)d = *(WELD_MEM const uint32_t *)s;
	else if(unit == 2) *(WELD_MEM uint16_t *)d = *(WELD_MEM const uint16_t *)s;
	else *d = *s;
}
template <class G> WELD_HD void compact_gather_block(G &g, const CompactGatherIn &J, uint32_t k) {
	uint32_t used = J.count_rec[1];
	used = used < J.nvert ? used : J.nvert;                                  // (never beyond what the arrays were sized from)
	if(J.cloud_rec && k == 0) g.thread0([&](LodLane &) { compact_record_store(J.cloud_rec, J.nvert, used, 0u, J.clip_v && used > J.vcap ? 1u : 0u); });
	if(!J.E) return;                                                          // (a cloud set without gathers: the record alone)
	const uint32_t n = used < J.vcap ? used : J.vcap, upr = J.E/J.unit;
	g.each([&](uint32_t tid, LodLane &) {
		const uint64_t t = (uint64_t)k*COMPACT_BLOCK + tid;
		const uint64_t j = (t >> 32) ? t/upr : (uint64_t)((uint32_t)t/upr);   // (a 64-bit division only where a grid passes 2^32 units)
		if(j >= n) return;
		const uint32_t u = (uint32_t)(t - j*upr)*J.unit;
		compact_copy_unit(J.src + (uint64_t)J.order[j]*J.sstride + u, J.dst + j*J.dstride + u, J.unit);
	});
}
WELD_HD uint32_t compact_gather_blocks(uint32_t nvert, uint32_t vcap, uint32_t E, uint32_t unit) {
	const uint64_t n = vcap < nvert ? vcap : nvert, units = E ? n*(E/unit) : 0;
	const uint64_t nb = (units + COMPACT_BLOCK - 1)/COMPACT_BLOCK;
	return nb ? (uint32_t)nb : 1u;                                            // (at least one: a cloud set's first gather stores the record)
}

} // namespace corto_hip
