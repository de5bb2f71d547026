// lod.h — crthip_batch_bind_lod: clustered levels of detail of a blob's index (include/corto_hip.h has the contract).  One LEVEL of one blob is one
// job: the vertices are clustered by the grid cell of their integer position (cell = position >> shift, arithmetic), every corner goes to its
// cell's least vertex, and the faces that stay - not degenerate, not a duplicate of a lower face - are written in their order.  The method, the
// phases and both partitions as __host__ __device__ code over a workgroup abstraction, so that the host runs the very same source in the kernels'
// partitions (crthip_lod_model, lod_host.cpp).
//
//   method   weld.h's OPEN-ADDRESSED TABLE OF REPRESENTATIVES, taken from there without a copy: the two tables (WeldLdsTable, WeldMemTable),
//            weld_fmix / weld_hash, weld_slots, weld_pos, weld_corner, weld_map.  What is stated here, once, is the insert and the lookup walk
//            as a template over a KEY FUNCTOR: key(i) gives item i's three-word key (LodKey, with its equality).
//              LodCellOf            a vertex's cell: the three coordinates shifted right, arithmetically
//              LodFaceKeyOf         a face's key, read from the stored clustered triple and rotated so that its least id comes first
//              LodFaceKeyFromIndex  the same key made from the index through remap: what lod_faces' insert walk compares, because the triple
//                                   of another workgroup's face may not have reached memory yet in the kernel that stores it (remap and the
//                                   index are a kernel old).  lod_blob has a barrier between the store and the walk and reads the triples
//            The walk's decisions are weld.h's: one compare-and-swap an empty slot, one atomic minimum a slot of the same key, no retry, the
//            loop bounded by the table.  A lookup finds a MINIMUM, the counts are sums: no output bit depends on the order of the atomics.
//   triples  the clustered triples live in blob scratch, 12 bytes a face: the face walks read a representative's key from there, and the
//            compaction its kept faces.  NOBODY HAS MEASURED recomputing them from the index and remap instead (profiles/lod.md).
//   dropped  (partition 1) lod_keep MARKS a dropped face in the first word of its own triple (LOD_DROPPED, no vertex id) and lod_scatter reads
//            the mark.  No race: another face's walk only ever reads a key's LEAST face, and that one is kept.
//   compact  order-preserving: a block scan of the kept flags a round of 256 faces; lod_blob carries a running base, partition 1 takes the
//            block's base from lod_offsets' exclusive scan of the block counts.  No look-back, no spinning.
//   group    G is the workgroup of LOD_THREADS: each(f) runs f(tid, LodLane &) for every thread, sync() is its barrier, block_sum() leaves the
//            sum of every lane's c in thread 0's c, block_scan() leaves in every lane x = the sum of the lower threads' c and t = the sum of all,
//            thread0(f) runs f(LodLane &) for thread 0.
#pragma once
#include "weld.h"

namespace corto_hip {

constexpr uint32_t LOD_THREADS = WELD_THREADS;
constexpr uint32_t LOD_BLOCK = 256;                        // vertices a workgroup of lod_insert / _lookup, faces a workgroup of lod_faces / _keep / _scatter
// lod_blob's limit: a job whose bigger table fits this much LDS (nvert <= 8 192 and nface <= 8 192; a C4 unit asks for 32 KiB).  It is the weld's
// threshold and AS UNMEASURED AS THE WELD'S: chosen and not varied (profiles/lod.md says what was measured)
constexpr uint32_t LOD_BLOB_LDS_MAX = 64u << 10;
constexpr uint32_t LOD_DROPPED = 0xFFFFFFFFu;              // the first word of a dropped face's triple (partition 1): no vertex id, nvert is 32 bits
static_assert(LOD_BLOCK == LOD_THREADS, "a thread a vertex, a thread a face");

WELD_HD uint64_t lod_table_slots(uint32_t nvert, uint32_t nface) {
	const uint64_t a = weld_slots(nvert), b = weld_slots(nface);
	return a > b ? a : b;
}
WELD_HD bool lod_in_blob(uint32_t nvert, uint32_t nface) { return lod_table_slots(nvert, nface)*4 <= LOD_BLOB_LDS_MAX; }
WELD_HD uint32_t lod_fblocks(uint32_t nface) { return (uint32_t)(((uint64_t)nface + LOD_BLOCK - 1)/LOD_BLOCK); }
// a level's scratch: the clustered triples; and beyond lod_blob the two tables (one range, zeroed by one FillJob), a word a block of faces, and a
// record for a level without one
struct LodScratchLayout { uint64_t triples, vtable, ftable, blocks, record, tables_bytes, total; };
WELD_HD LodScratchLayout lod_scratch_layout(uint32_t nvert, uint32_t nface) {
	LodScratchLayout l;
	l.triples = 0;
	uint64_t o = ((uint64_t)nface*12 + 15) & ~15ull;
	l.vtable = l.ftable = l.blocks = l.record = o; l.tables_bytes = 0;
	if(!lod_in_blob(nvert, nface)) {
		l.vtable = o; o += weld_slots(nvert)*4;
		l.ftable = o; o += weld_slots(nface)*4;
		l.tables_bytes = o - l.vtable;
		l.blocks = o; o += ((uint64_t)lod_fblocks(nface)*4 + 15) & ~15ull;
		l.record = o; o += 16;
	}
	l.total = o;
	return l;
}

// ---- the inputs and the keys -------------------------------------------------------------------------------------------------------------------

struct LodIn { WeldIn w; uint32_t shift; };
struct LodKey {
	uint32_t x, y, z;
	WELD_HD bool operator==(const LodKey &o) const { return x == o.x && y == o.y && z == o.z; }
};
WELD_HD uint32_t lod_hash(const LodKey &k) { return weld_hash(WeldPos{k.x, k.y, k.z}); }
// a triple rotated so that its least id comes first, the orientation kept (three different ids)
WELD_HD LodKey lod_rotated(uint32_t a, uint32_t b, uint32_t c) {
	if(a < b && a < c) return LodKey{a, b, c};
	return b < c ? LodKey{b, c, a} : LodKey{c, a, b};
}
WELD_HD bool lod_degenerate(uint32_t a, uint32_t b, uint32_t c, uint32_t nvert) { return !(a != b && b != c && a != c && a < nvert && b < nvert && c < nvert); }

struct LodCellOf {
	WeldIn J; uint32_t shift;
	WELD_HD LodKey operator()(uint32_t v) const {
		const WeldPos p = weld_pos(J, v);
		return LodKey{(uint32_t)((int32_t)p.x >> shift), (uint32_t)((int32_t)p.y >> shift), (uint32_t)((int32_t)p.z >> shift)};
	}
};
struct LodFaceKeyOf {
	WELD_MEM const uint32_t *tri;
	WELD_HD LodKey operator()(uint32_t f) const {
		WELD_MEM const uint32_t *t = tri + (uint64_t)f*3;
		return lod_rotated(t[0], t[1], t[2]);
	}
};
struct LodFaceKeyFromIndex {
	WeldIn J; WELD_MEM const uint32_t *remap;
	WELD_HD LodKey operator()(uint32_t f) const {
		const uint64_t k = (uint64_t)f*3;
		return lod_rotated(weld_map(J, remap, weld_corner(J, k)), weld_map(J, remap, weld_corner(J, k + 1)), weld_map(J, remap, weld_corner(J, k + 2)));
	}
};

// a thread's state: c goes into block_sum / block_scan, x and t come out of block_scan; run is the running base of a compaction, n a count a
// thread keeps over rounds, cells thread 0's first sum while the others are made
struct LodLane { uint32_t c, x, t, run, n, cells; };
// the hook's figures: the slots all insert walks visited and the longest walk, for the vertices and for the faces (the host pass only)
struct LodStats { uint64_t vtotal, vlongest, ftotal, flongest; };

// ---- the walks, once, over a key functor: as values (weld.h says why) ----------------------------------------------------------------------------

// item i goes into the table; the slots its walk visited
template <class S, class K> WELD_HD uint64_t lod_insert_one(const S &tb, uint64_t T, const K &key, uint32_t i) {
	const LodKey k = key(i);
	uint64_t s = lod_hash(k) & (T - 1);
	for(uint64_t n = 0; n < T; n++, s = (s + 1) & (T - 1)) {
		uint32_t w = tb.get(s);
		if(!w) { w = tb.cas(s, i + 1); if(!w) return n + 1; }
		if(key(w - 1) == k) { tb.lower(s, i + 1); return n + 1; }
	}
	return T;                                                                  // (impossible: n items in at least 2*n slots)
}
// the least item with i's key: the representative of the slot the same walk ends at; i itself on the impossible miss
template <class S, class K> WELD_HD uint32_t lod_lookup_one(const S &tb, uint64_t T, const K &key, uint32_t i) {
	const LodKey k = key(i);
	uint64_t s = lod_hash(k) & (T - 1);
	for(uint64_t n = 0; n < T; n++, s = (s + 1) & (T - 1)) {
		const uint32_t w = tb.get(s);
		if(!w) break;
		if(key(w - 1) == k) return w - 1;
	}
	return i;
}

// ---- the phases: vertices [v0, v1) or faces [f0, f1) by one workgroup, thread tid takes the first + tid, + LOD_THREADS, ... -------------------------

template <class G, class S> WELD_HD void lod_insert(G &g, const LodIn &J, const S &tb, uint64_t T, uint32_t v0, uint32_t v1, LodStats *stats) {
	const LodCellOf key{J.w, J.shift};
	g.each([&](uint32_t tid, LodLane &) {
		for(uint64_t v = (uint64_t)v0 + tid; v < v1; v += LOD_THREADS) {
			const uint64_t walk = lod_insert_one(tb, T, key, (uint32_t)v);
#if !WELD_DEVICE_PASS
			if(stats) { stats->vtotal += walk; if(walk > stats->vlongest) stats->vlongest = walk; }
#else
			(void)walk; (void)stats;
#endif
		}
	});
}
// remap, and the workgroup's vertices that are their own cell's least in thread 0's c
template <class G, class S> WELD_HD void lod_lookup(G &g, const LodIn &J, const S &tb, uint64_t T, WELD_MEM uint32_t *remap, uint32_t v0, uint32_t v1) {
	const LodCellOf key{J.w, J.shift};
	g.each([&](uint32_t tid, LodLane &L) {
		uint32_t nu = 0;
		for(uint64_t v = (uint64_t)v0 + tid; v < v1; v += LOD_THREADS) {
			const uint32_t u = lod_lookup_one(tb, T, key, (uint32_t)v);
			remap[v] = u; nu += u == (uint32_t)v;
		}
		L.c = nu;
	});
	g.block_sum();
}
// the clustered triples (remap is final: behind a barrier, or the kernel before)
template <class G> WELD_HD void lod_triples(G &g, const LodIn &J, WELD_MEM const uint32_t *remap, WELD_MEM uint32_t *tri, uint32_t f0, uint32_t f1) {
	g.each([&](uint32_t tid, LodLane &) {
		for(uint64_t f = (uint64_t)f0 + tid; f < f1; f += LOD_THREADS) {
			const uint64_t k = f*3;
			tri[k] = weld_map(J.w, remap, weld_corner(J.w, k));
			tri[k + 1] = weld_map(J.w, remap, weld_corner(J.w, k + 1));
			tri[k + 2] = weld_map(J.w, remap, weld_corner(J.w, k + 2));
		}
	});
}
// the faces that are not degenerate go into the face table by `key`; a thread reads its own faces' triples (it stored them, or a barrier lies between)
template <class G, class S, class K> WELD_HD void lod_face_insert(G &g, const LodIn &J, const S &tb, uint64_t T, const K &key, WELD_MEM const uint32_t *tri,
	uint32_t f0, uint32_t f1, LodStats *stats) {
	g.each([&](uint32_t tid, LodLane &) {
		for(uint64_t f = (uint64_t)f0 + tid; f < f1; f += LOD_THREADS) {
			WELD_MEM const uint32_t *t = tri + f*3;
			if(lod_degenerate(t[0], t[1], t[2], J.w.nvert)) continue;
			const uint64_t walk = lod_insert_one(tb, T, key, (uint32_t)f);
#if !WELD_DEVICE_PASS
			if(stats) { stats->ftotal += walk; if(walk > stats->flongest) stats->flongest = walk; }
#else
			(void)walk; (void)stats;
#endif
		}
	});
}
// face f's verdict from its stored triple and the final face table: 0 kept, 1 degenerate, 2 a duplicate of a lower face
template <class S> WELD_HD uint32_t lod_verdict(const S &tb, uint64_t T, WELD_MEM const uint32_t *tri, uint32_t nvert, uint32_t f) {
	WELD_MEM const uint32_t *t = tri + (uint64_t)f*3;
	if(lod_degenerate(t[0], t[1], t[2], nvert)) return 1u;
	return lod_lookup_one(tb, T, LodFaceKeyOf{tri}, f) == f ? 0u : 2u;
}
// a kept face's triple goes to slot `at` of the level's index
WELD_HD void lod_emit(WELD_MEM uint32_t *index, WELD_MEM const uint32_t *tri, uint32_t f, uint32_t at) {
	WELD_MEM const uint32_t *t = tri + (uint64_t)f*3;
	WELD_MEM uint32_t *o = index + (uint64_t)at*3;
	o[0] = t[0]; o[1] = t[1]; o[2] = t[2];
}

// the record: written whole by the one workgroup of a job, or started by lod_insert's first workgroup, added to by every workgroup of lod_lookup
// (cells) and lod_keep (degenerate, duplicate) and finished by lod_offsets (faces)
WELD_HD void lod_record_store(WELD_MEM crthip_lod_counts *rec, uint32_t cells, uint32_t faces, uint32_t degenerate, uint32_t duplicate) {
#if WELD_DEVICE_PASS
	*(WELD_MEM weld_u32x4 *)rec = weld_u32x4{cells, faces, degenerate, duplicate};
#else
	*rec = crthip_lod_counts{cells, faces, degenerate, duplicate};
#endif
}
WELD_HD void lod_record_add(WELD_MEM crthip_lod_counts *rec, uint32_t word, uint32_t c) {
#if WELD_DEVICE_PASS
	(void)__hip_atomic_fetch_add((WELD_MEM uint32_t *)rec + word, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
	((uint32_t *)rec)[word] += c;
#endif
}

// ---- partition 0: a job by ONE workgroup, ONE table in LDS used twice (vertices by cell, then faces by key); rec may be null ---------------------

template <class G> WELD_HD void lod_blob(G &g, const LodIn &J, const WeldLdsTable &tb, WELD_MEM uint32_t *remap, WELD_MEM uint32_t *tri, WELD_MEM uint32_t *index,
	WELD_MEM crthip_lod_counts *rec, LodStats *stats) {
	const uint32_t nvert = J.w.nvert, nface = J.w.nface;
	const uint64_t Tv = weld_slots(nvert), Tf = weld_slots(nface);
	g.each([&](uint32_t tid, LodLane &) { for(uint64_t s = tid; s < Tv; s += LOD_THREADS) tb.put(s, 0u); });
	g.sync();
	lod_insert(g, J, tb, Tv, 0, nvert, stats);
	g.sync();
	lod_lookup(g, J, tb, Tv, remap, 0, nvert);
	g.thread0([&](LodLane &L) { L.cells = L.c; });
	g.sync();                                                                  // (remap is read below by other threads than wrote it; the table is free)
	lod_triples(g, J, remap, tri, 0, nface);
	g.each([&](uint32_t tid, LodLane &) { for(uint64_t s = tid; s < Tf; s += LOD_THREADS) tb.put(s, 0u); });
	g.sync();                                                                  // (a face's walk reads other threads' triples)
	lod_face_insert(g, J, tb, Tf, LodFaceKeyOf{tri}, tri, 0, nface, stats);
	g.sync();
	g.each([&](uint32_t, LodLane &L) { L.run = 0; L.n = 0; });
	for(uint64_t f0 = 0; f0 < nface; f0 += LOD_THREADS) {                      // a round of 256 faces: verdicts, the block scan, the kept triples
		g.each([&](uint32_t tid, LodLane &L) {
			const uint64_t f = f0 + tid;
			const uint32_t vd = f < nface ? lod_verdict(tb, Tf, tri, nvert, (uint32_t)f) : 1u;
			L.c = vd == 0u; L.n += f < nface && vd == 2u;
		});
		g.block_scan();
		g.each([&](uint32_t tid, LodLane &L) {
			if(L.c) lod_emit(index, tri, (uint32_t)(f0 + tid), L.run + L.x);
			L.run += L.t;
		});
	}
	g.each([&](uint32_t, LodLane &L) { L.c = L.n; });
	g.block_sum();
	g.thread0([&](LodLane &L) { if(rec) lod_record_store(rec, L.cells, L.run, nface - L.run - L.c, L.c); });
}

// ---- partition 1: workgroup k of a job's ceil(nvert/LOD_BLOCK) in lod_insert / _lookup, of its ceil(nface/LOD_BLOCK) in lod_faces / _keep / _scatter;
// one workgroup a job in lod_offsets.  rec is never null here (the planner gives a level without a record one in scratch) -------------------------

template <class G> WELD_HD void lod_insert_block(G &g, const LodIn &J, const WeldMemTable &vtb, WELD_MEM crthip_lod_counts *rec, uint32_t k, LodStats *stats) {
	lod_insert(g, J, vtb, weld_slots(J.w.nvert), k*LOD_BLOCK, (uint32_t)weld_block_end(J.w.nvert, k), stats);
	if(k == 0) g.thread0([&](LodLane &) { lod_record_store(rec, 0u, 0u, 0u, 0u); });
}
template <class G> WELD_HD void lod_lookup_block(G &g, const LodIn &J, const WeldMemTable &vtb, WELD_MEM uint32_t *remap, WELD_MEM crthip_lod_counts *rec, uint32_t k) {
	lod_lookup(g, J, vtb, weld_slots(J.w.nvert), remap, k*LOD_BLOCK, (uint32_t)weld_block_end(J.w.nvert, k));
	g.thread0([&](LodLane &L) { lod_record_add(rec, 0, L.c); });
}
template <class G> WELD_HD void lod_faces_block(G &g, const LodIn &J, const WeldMemTable &ftb, WELD_MEM const uint32_t *remap, WELD_MEM uint32_t *tri, uint32_t k, LodStats *stats) {
	const uint32_t f0 = k*LOD_BLOCK, f1 = (uint32_t)weld_block_end(J.w.nface, k);
	lod_triples(g, J, remap, tri, f0, f1);
	lod_face_insert(g, J, ftb, weld_slots(J.w.nface), LodFaceKeyFromIndex{J.w, remap}, tri, f0, f1, stats);
}
// the verdicts: a dropped face is marked, the workgroup's kept faces go to its word, its other two counts to the record (three
// fields of 10 bits in one sum, at bits 0, 10 and 20: a field reaches 256 where every face of a full block has one verdict, which needs 9 bits)
template <class G> WELD_HD void lod_keep_block(G &g, const LodIn &J, const WeldMemTable &ftb, WELD_MEM uint32_t *tri, WELD_MEM uint32_t *blocks, WELD_MEM crthip_lod_counts *rec, uint32_t k) {
	const uint64_t T = weld_slots(J.w.nface);
	g.each([&](uint32_t tid, LodLane &L) {
		const uint64_t f = (uint64_t)k*LOD_BLOCK + tid;
		L.c = 0;
		if(f < J.w.nface) {
			const uint32_t vd = lod_verdict(ftb, T, tri, J.w.nvert, (uint32_t)f);
			if(vd) tri[f*3] = LOD_DROPPED;
			L.c = 1u << 10*vd;
		}
	});
	g.block_sum();
	g.thread0([&](LodLane &L) {
		blocks[k] = L.c & 1023u;
		lod_record_add(rec, 2, L.c >> 10 & 1023u);
		lod_record_add(rec, 3, L.c >> 20);
	});
}
// the exclusive scan of a job's block counts, in place, and the record's `faces`
template <class G> WELD_HD void lod_offsets_job(G &g, uint32_t nface, WELD_MEM uint32_t *blocks, WELD_MEM crthip_lod_counts *rec) {
	const uint32_t nb = lod_fblocks(nface);
	g.each([&](uint32_t, LodLane &L) { L.run = 0; });
	for(uint64_t b0 = 0; b0 < nb; b0 += LOD_THREADS) {
		g.each([&](uint32_t tid, LodLane &L) { L.c = b0 + tid < nb ? blocks[b0 + tid] : 0u; });
		g.block_scan();
		g.each([&](uint32_t tid, LodLane &L) {
			if(b0 + tid < nb) blocks[b0 + tid] = L.run + L.x;
			L.run += L.t;
		});
	}
	g.thread0([&](LodLane &L) { lod_record_add(rec, 1, L.run); });
}
template <class G> WELD_HD void lod_scatter_block(G &g, const LodIn &J, WELD_MEM const uint32_t *tri, WELD_MEM const uint32_t *blocks, WELD_MEM uint32_t *index, uint32_t k) {
	g.each([&](uint32_t tid, LodLane &L) {
		const uint64_t f = (uint64_t)k*LOD_BLOCK + tid;
		L.c = f < J.w.nface && tri[f*3] != LOD_DROPPED;
	});
	g.block_scan();
	g.each([&](uint32_t tid, LodLane &L) { if(L.c) lod_emit(index, tri, k*LOD_BLOCK + tid, blocks[k] + L.x); });
}

// what crthip_batch_bind_lod (and the hook) ask of a binding on a blob of nvert vertices and nface faces, behind "no such blob" and "a point
// cloud", in the header's order; null: fine
inline const char *lod_binding_error(const crthip_lod_binding *l, uint32_t nvert, uint32_t nface) {
	if(l->levels < 1 || l->levels > CRTHIP_LOD_MAX_LEVELS) return "lod: levels is not in 1..CRTHIP_LOD_MAX_LEVELS";
	for(uint32_t k = 0; k < l->levels; k++) {
		const crthip_lod_level &v = l->level[k];
		if(!v.remap || (uintptr_t)v.remap % 4 || !v.index || (uintptr_t)v.index % 4) return "lod: a level's remap or index is NULL or not 4-byte aligned";
		if((uintptr_t)v.counts % 16) return "lod: a level's counts is not 16-byte aligned";
		if(v.remap_capacity < nvert || (uint64_t)v.index_capacity < (uint64_t)nface*3) return "lod: a level's remap_capacity is below nvert or its index_capacity below 3*nface";
		if(v.shift > 31) return "lod: a level's shift is above 31";
		if(k && v.shift <= l->level[k - 1].shift) return "lod: a level's shift is not above the level's before";
		if(v.reserved) return "lod: a level's reserved is not 0";
	}
	if(l->flags) return "lod: unknown flag bits";
	if(l->reserved[0] || l->reserved[1]) return "lod: reserved is not 0";
	return nullptr;
}

} // namespace corto_hip
