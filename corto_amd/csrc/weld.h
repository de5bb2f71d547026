// weld.h — crthip_batch_bind_weld: the weld map of a blob's integer positions and its welded index (include/corto_hip.h has the contract).  The
// method, the phases and both partitions as __host__ __device__ code over a workgroup abstraction, so that the host runs the very same source in
// the kernels' partitions (crthip_weld_model, weld_host.cpp).
//
//   method   an OPEN-ADDRESSED TABLE OF REPRESENTATIVES with linear probing, not a list a bucket.  T = weld_slots(nvert) words, the least power
//            of two >= 2*nvert (at least 64): a load of at most 1/2.  A word is 0 (empty) or u + 1 for a vertex u that has the slot's position.
//              insert   v walks from weld_hash(p[v]) & (T - 1): an empty slot gets ONE compare-and-swap 0 -> v + 1 (won: done; lost: the value it
//                       returned is the word); a word whose vertex has p[v]'s position gets one atomic minimum with v + 1 (done); else the next slot.
//                       A slot never becomes empty again and its representative only changes to another vertex of the same position, so a
//                       position lives in exactly one slot and every later walk takes the same decisions.  No retry: the loop is bounded by T
//              lookup   (behind a barrier, or in the next kernel) the same walk to the slot whose representative has p[v]: remap[v] = word - 1
//              index    windex[k] = remap[id] for id < nvert, else id; a face whose welded corners are not three different ids below nvert is
//                       DEGENERATE (adjacency's "invalid" on the welded index)
//   order    which vertex wins a slot's compare-and-swap depends on the order of the atomics; the word a lookup finds is a MINIMUM and the two
//            counts are sums: no output bit depends on that order.  k coincident vertices cost k atomics on one word, not k*k reads.
//   cost     many DISTINCT positions on one probe chain cost the chain's length each (DESIGN.md §3.5g "Left out").
//   memory   a position is read from memory wherever a walk compares one, as adjacency reads heads from the index.  NOBODY HAS MEASURED
//            staging the blob's positions in LDS for weld_blob instead (12 bytes a vertex beside the table): profiles/weld.md.
//   stores   WeldLdsTable: the table in LDS, one workgroup a blob (weld_blob: k_weld_blob).  WeldMemTable: the table in device memory, zeroed by
//            a FillJob, WELD_BLOCK vertices or corners a workgroup (weld_insert, weld_lookup, weld_index as a kernel each).
//   group    G is the workgroup of WELD_THREADS: each(f) runs f(tid, WeldLane &) for every thread (the kernel: its own; the host: all of them in
//            a shuffled order), sync() is its barrier, block_sum() leaves the sum of every lane's c in thread 0's c, thread0(f) runs
//            f(WeldLane &) for thread 0.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/corto_hip.h"

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define WELD_HD __host__ __device__ __forceinline__         // (a call left standing takes the address of a lane's state: scratch)
#else
#define WELD_HD inline
#endif
// k_weld.hip defines WELD_KERNELS: pointers into device memory and into LDS carry their address space there (global_* / ds_* and never flat_*:
// kernels_common.h); everywhere else, and in the host pass, the qualifiers are empty
#if defined(WELD_KERNELS) && defined(__HIP_DEVICE_COMPILE__)
#define WELD_MEM __attribute__((address_space(1)))
#define WELD_LDS __attribute__((address_space(3)))
#define WELD_DEVICE_PASS 1
#else
#define WELD_MEM
#define WELD_LDS
#define WELD_DEVICE_PASS 0
#endif

namespace corto_hip {

constexpr uint32_t WELD_THREADS = 256;
constexpr uint32_t WELD_BLOCK = 256;                       // vertices a workgroup of weld_insert / _lookup, corners a workgroup of weld_index
// weld_blob's limit: a blob whose table fits this much LDS (nvert <= 8 192), so that two workgroups share a CU's 160 KiB (a C4 unit's table
// takes 32 KiB).  NOBODY HAS MEASURED THIS THRESHOLD: it is the largest power of two that leaves room for two workgroups, chosen and not varied
// (profiles/weld.md says what was measured)
constexpr uint32_t WELD_BLOB_LDS_MAX = 64u << 10;
static_assert(WELD_BLOCK == WELD_THREADS, "a thread a vertex, a thread a corner");

// sixteen bytes as one access (a plain vector: HIP's uint4 is a class whose assignment takes a generic `this`, which makes the store FLAT)
typedef uint32_t weld_u32x4 __attribute__((ext_vector_type(4)));

// the table's slots: the least power of two >= 2*nvert, at least 64 (2^33 for nvert beyond 2^32 - 2^31: the walk's slot numbers are 64 bits)
WELD_HD uint64_t weld_slots(uint32_t nvert) {
	uint64_t T = 64;
	while(T < 2*(uint64_t)nvert) T <<= 1;
	return T;
}
WELD_HD bool weld_in_blob(uint32_t nvert) { return weld_slots(nvert)*4 <= WELD_BLOB_LDS_MAX; }
// scratch of a bigger blob: the table, and a record for a binding without one
struct WeldScratchLayout { uint64_t record, total; };
WELD_HD WeldScratchLayout weld_scratch_layout(uint32_t nvert) {
	WeldScratchLayout l;
	l.record = weld_slots(nvert)*4;
	l.total = l.record + 16;
	return l;
}

// ---- the inputs ------------------------------------------------------------------------------------------------------------------------------

struct WeldIn { WELD_MEM const int32_t *position; WELD_MEM const void *index; uint32_t index_u16, nface, nvert; };
struct WeldPos { uint32_t x, y, z; };
WELD_HD WeldPos weld_pos(const WeldIn &J, uint32_t v) {
	WELD_MEM const uint32_t *p = (WELD_MEM const uint32_t *)J.position + (uint64_t)v*3;
	return WeldPos{p[0], p[1], p[2]};
}
WELD_HD bool weld_same(const WeldPos &a, const WeldPos &b) { return a.x == b.x && a.y == b.y && a.z == b.z; }
// where a position's walk starts: murmur3's finaliser over each coordinate in turn - a full avalanche of all 96 bits, the sign bits included, so
// that the coordinates of a lattice do not cluster (tests/test_weld_cpu.py holds the mean walk of the lattices to 5 slots)
WELD_HD uint32_t weld_fmix(uint32_t h) {
	h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
	return h;
}
WELD_HD uint32_t weld_hash(const WeldPos &p) { return weld_fmix(weld_fmix(weld_fmix(p.x + 0x9E3779B9u) + p.y) + p.z); }
WELD_HD uint32_t weld_corner(const WeldIn &J, uint64_t k) {
	return J.index_u16 ? (uint32_t)((WELD_MEM const uint16_t *)J.index)[k] : ((WELD_MEM const uint32_t *)J.index)[k];
}

// ---- the two tables --------------------------------------------------------------------------------------------------------------------------

// get(s): the word; cas(s, x): one compare-and-swap 0 -> x, the word before (0: won); lower(s, x): word = min(word, x), atomically.
// A get beside the atomics may see an older word: 0 sends it to the compare-and-swap, which returns the word; an older representative has the
// slot's position like the present one
struct WeldLdsTable {
	WELD_LDS uint32_t *t;
	WELD_HD uint32_t get(uint64_t s) const {
#if WELD_DEVICE_PASS
		return __hip_atomic_load(t + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#else
		return t[s];
#endif
	}
	WELD_HD uint32_t cas(uint64_t s, uint32_t x) const {
#if WELD_DEVICE_PASS
		uint32_t old = 0;
		(void)__hip_atomic_compare_exchange_strong(t + s, &old, x, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
		return old;
#else
		const uint32_t old = t[s]; if(!old) t[s] = x; return old;
#endif
	}
	WELD_HD void lower(uint64_t s, uint32_t x) const {
#if WELD_DEVICE_PASS
		(void)__hip_atomic_fetch_min(t + s, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#else
		if(x < t[s]) t[s] = x;
#endif
	}
	WELD_HD void put(uint64_t s, uint32_t x) const { t[s] = x; }
};
struct WeldMemTable {
	WELD_MEM uint32_t *t;
	WELD_HD uint32_t get(uint64_t s) const {
#if WELD_DEVICE_PASS
		return __hip_atomic_load(t + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
		return t[s];
#endif
	}
	WELD_HD uint32_t cas(uint64_t s, uint32_t x) const {
#if WELD_DEVICE_PASS
		uint32_t old = 0;
		(void)__hip_atomic_compare_exchange_strong(t + s, &old, x, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		return old;
#else
		const uint32_t old = t[s]; if(!old) t[s] = x; return old;
#endif
	}
	WELD_HD void lower(uint64_t s, uint32_t x) const {
#if WELD_DEVICE_PASS
		(void)__hip_atomic_fetch_min(t + s, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
		if(x < t[s]) t[s] = x;
#endif
	}
};

// a thread's state: its share of a count, and (thread 0 of weld_blob) the first count while the second is summed
struct WeldLane { uint32_t c, unique; };
// the hook's figures: the slots all insert walks visited, and the longest walk (the host pass only)
struct WeldStats { uint64_t total, longest; };

// ---- the walks: as values (a result reached through a pointer chosen at run time would put the lane's state into scratch) ----------------------

// vertex v goes into the table; the slots its walk visited
template <class S> WELD_HD uint64_t weld_insert_one(const WeldIn &J, const S &tb, uint64_t T, uint32_t v) {
	const WeldPos p = weld_pos(J, v);
	uint64_t s = weld_hash(p) & (T - 1);
	for(uint64_t n = 0; n < T; n++, s = (s + 1) & (T - 1)) {
		uint32_t w = tb.get(s);
		if(!w) { w = tb.cas(s, v + 1); if(!w) return n + 1; }
		if(weld_same(weld_pos(J, w - 1), p)) { tb.lower(s, v + 1); return n + 1; }
	}
	return T;                                                                  // (impossible: nvert positions in 2*nvert slots)
}
// the least vertex with v's position: the representative of the slot the same walk ends at; v itself on the impossible miss
template <class S> WELD_HD uint32_t weld_lookup_one(const WeldIn &J, const S &tb, uint64_t T, uint32_t v) {
	const WeldPos p = weld_pos(J, v);
	uint64_t s = weld_hash(p) & (T - 1);
	for(uint64_t n = 0; n < T; n++, s = (s + 1) & (T - 1)) {
		const uint32_t w = tb.get(s);
		if(!w) break;
		if(weld_same(weld_pos(J, w - 1), p)) return w - 1;
	}
	return v;
}
WELD_HD uint32_t weld_map(const WeldIn &J, WELD_MEM const uint32_t *remap, uint32_t id) { return id < J.nvert ? remap[id] : id; }

// ---- the phases: vertices [v0, v1) or corners [k0, k1) by one workgroup, thread tid takes v0 + tid, + WELD_THREADS, ... -------------------------

template <class G, class S> WELD_HD void weld_insert(G &g, const WeldIn &J, const S &tb, uint64_t T, uint32_t v0, uint32_t v1, WeldStats *stats) {
	g.each([&](uint32_t tid, WeldLane &) {
		for(uint64_t v = (uint64_t)v0 + tid; v < v1; v += WELD_THREADS) {
			const uint64_t walk = weld_insert_one(J, tb, T, (uint32_t)v);
#if !WELD_DEVICE_PASS
			if(stats) { stats->total += walk; if(walk > stats->longest) stats->longest = walk; }
#else
			(void)walk; (void)stats;
#endif
		}
	});
}
// remap, and the workgroup's vertices that are their own representative in thread 0's c
template <class G, class S> WELD_HD void weld_lookup(G &g, const WeldIn &J, const S &tb, uint64_t T, WELD_MEM uint32_t *remap, uint32_t v0, uint32_t v1) {
	g.each([&](uint32_t tid, WeldLane &L) {
		uint32_t nu = 0;
		for(uint64_t v = (uint64_t)v0 + tid; v < v1; v += WELD_THREADS) {
			const uint32_t u = weld_lookup_one(J, tb, T, (uint32_t)v);
			remap[v] = u; nu += u == (uint32_t)v;
		}
		L.c = nu;
	});
	g.block_sum();
}
// the welded index (remap is final: behind a barrier, or the kernel before), and the workgroup's degenerate faces in thread 0's c: the thread
// of a face's first corner looks at all three
template <class G> WELD_HD void weld_index(G &g, const WeldIn &J, WELD_MEM const uint32_t *remap, WELD_MEM uint32_t *windex, uint64_t k0, uint64_t k1) {
	g.each([&](uint32_t tid, WeldLane &L) {
		uint32_t nd = 0;
		for(uint64_t k = k0 + tid; k < k1; k += WELD_THREADS) {
			const uint32_t a = weld_map(J, remap, weld_corner(J, k));
			windex[k] = a;
			if(k%3 == 0) {
				const uint32_t b = weld_map(J, remap, weld_corner(J, k + 1)), c = weld_map(J, remap, weld_corner(J, k + 2));
				nd += !(a != b && b != c && a != c && a < J.nvert && b < J.nvert && c < J.nvert);
			}
		}
		L.c = nd;
	});
	g.block_sum();
}

// the record: written whole by the one workgroup of a blob, or started by weld_insert's first workgroup and added to by every workgroup of
// weld_lookup (unique) and weld_index (degenerate)
WELD_HD void weld_record_store(WELD_MEM crthip_weld_counts *rec, uint32_t nvert, uint32_t unique, uint32_t degenerate) {
#if WELD_DEVICE_PASS
	*(WELD_MEM weld_u32x4 *)rec = weld_u32x4{nvert, unique, degenerate, 0u};
#else
	*rec = crthip_weld_counts{nvert, unique, degenerate, 0u};
#endif
}
WELD_HD void weld_record_add(WELD_MEM crthip_weld_counts *rec, uint32_t word, uint32_t c) {
#if WELD_DEVICE_PASS
	(void)__hip_atomic_fetch_add((WELD_MEM uint32_t *)rec + word, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
	((uint32_t *)rec)[word] += c;
#endif
}

// ---- partition 0: a blob by ONE workgroup, the table in LDS; windex and rec may be null ----------------------------------------------------------

template <class G> WELD_HD void weld_blob(G &g, const WeldIn &J, const WeldLdsTable &tb, WELD_MEM uint32_t *remap, WELD_MEM uint32_t *windex,
	WELD_MEM crthip_weld_counts *rec, WeldStats *stats) {
	const uint64_t T = weld_slots(J.nvert);
	g.each([&](uint32_t tid, WeldLane &) { for(uint64_t s = tid; s < T; s += WELD_THREADS) tb.put(s, 0u); });
	g.sync();
	weld_insert(g, J, tb, T, 0, J.nvert, stats);
	g.sync();
	weld_lookup(g, J, tb, T, remap, 0, J.nvert);
	g.thread0([&](WeldLane &L) { L.unique = L.c; L.c = 0; });
	g.sync();                                                                  // (remap is read below by other threads than wrote it)
	if(windex) weld_index(g, J, remap, windex, 0, (uint64_t)J.nface*3);
	g.thread0([&](WeldLane &L) { if(rec) weld_record_store(rec, J.nvert, L.unique, L.c); });
}

// ---- partition 1: workgroup k of a blob's ceil(nvert/WELD_BLOCK) in weld_insert / _lookup, of its ceil(3*nface/WELD_BLOCK) in weld_index -------

// (at least one workgroup: a blob's first one stores the record, whatever the blob has)
WELD_HD uint32_t weld_vblocks(uint32_t nvert) { return nvert ? (uint32_t)(((uint64_t)nvert + WELD_BLOCK - 1)/WELD_BLOCK) : 1u; }
WELD_HD uint32_t weld_cblocks(uint32_t nface) { return (uint32_t)(((uint64_t)nface*3 + WELD_BLOCK - 1)/WELD_BLOCK); }
WELD_HD uint64_t weld_block_end(uint64_t n, uint32_t k) { const uint64_t e = ((uint64_t)k + 1)*WELD_BLOCK; return e < n ? e : n; }
template <class G> WELD_HD void weld_insert_block(G &g, const WeldIn &J, const WeldMemTable &tb, WELD_MEM crthip_weld_counts *rec, uint32_t k, WeldStats *stats) {
	weld_insert(g, J, tb, weld_slots(J.nvert), k*WELD_BLOCK, (uint32_t)weld_block_end(J.nvert, k), stats);
	if(k == 0) g.thread0([&](WeldLane &) { weld_record_store(rec, J.nvert, 0u, 0u); });
}
template <class G> WELD_HD void weld_lookup_block(G &g, const WeldIn &J, const WeldMemTable &tb, WELD_MEM uint32_t *remap, WELD_MEM crthip_weld_counts *rec, uint32_t k) {
	weld_lookup(g, J, tb, weld_slots(J.nvert), remap, k*WELD_BLOCK, (uint32_t)weld_block_end(J.nvert, k));
	g.thread0([&](WeldLane &L) { weld_record_add(rec, 1, L.c); });
}
template <class G> WELD_HD void weld_index_block(G &g, const WeldIn &J, WELD_MEM const uint32_t *remap, WELD_MEM uint32_t *windex, WELD_MEM crthip_weld_counts *rec, uint32_t k) {
	weld_index(g, J, remap, windex, (uint64_t)k*WELD_BLOCK, weld_block_end((uint64_t)J.nface*3, k));
	g.thread0([&](WeldLane &L) { weld_record_add(rec, 2, L.c); });
}

// what crthip_batch_bind_weld (and the hook) ask of a binding on a blob of nvert vertices and nface faces, behind "no such blob" and "a point
// cloud", in the header's order; null: fine
inline const char *weld_binding_error(const crthip_weld_binding *w, uint32_t nvert, uint32_t nface) {
	if(!w->remap || (uintptr_t)w->remap % 4) return "weld: remap is NULL or not 4-byte aligned";
	if((uintptr_t)w->index % 4 || (uintptr_t)w->counts % 16) return "weld: index is not 4-byte aligned, or counts is not 16-byte aligned";
	if(w->remap_capacity < nvert) return "weld: remap_capacity is below nvert";
	if(w->index && (uint64_t)w->index_capacity < (uint64_t)nface*3) return "weld: index_capacity is below 3*nface";
	if(w->flags & ~(uint32_t)CRTHIP_WELD_ADJACENCY) return "weld: unknown flag bits";
	if(w->reserved) return "weld: reserved is not 0";
	if((w->flags & CRTHIP_WELD_ADJACENCY) && !w->index) return "weld: CRTHIP_WELD_ADJACENCY needs index";
	return nullptr;
}

} // namespace corto_hip
