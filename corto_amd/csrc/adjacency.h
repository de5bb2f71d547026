// adjacency.h — crthip_batch_bind_adjacency: the half-edge twins of a blob's decoded index (include/corto_hip.h has the contract).  The rule,
// the phases and both partitions as __host__ __device__ code over a workgroup abstraction, so that the host runs the very same source in the
// kernels' partitions (crthip_adjacency_model, adjacency_host.cpp).
//
//   method   an INCIDENCE LIST BY ORIGIN VERTEX (CSR), not a hash of edges.  `end` has nvert + 1 words, `list` one entry a half-edge.
//              count    end[a] += 1 for every valid half-edge a -> b                                   (end starts out zero)
//              scan     end becomes its inclusive prefix sum: end[v] is where v's list ENDS
//              fill     a valid half-edge h = a -> b takes the slot --end[a] (an atomic decrement) and puts h there; afterwards end[v] is
//                       where v's list STARTS and end[v + 1] where it ends (end[nvert] never moves: nobody's origin)
//              twin     for h = a -> b: walk b's list for the least entry whose head is a (the twin), and a's list for an entry below h whose
//                       head is b (the duplicate test).  The head of an entry is read from the index.  twin[h] is written for every h
//   order    the slot a half-edge gets within its vertex's list depends on the order of the atomics.  Every result is a MINIMUM over a list or
//            an EXISTENCE test in it, and the three counts are sums: no output bit depends on that order.
//   cost     a vertex of valence d costs d*d list reads (every one of its d half-edges walks a list of d).  See DESIGN.md §3.5f "Left out".
//   stores   AdjLdsStore: end and 16-bit entries in LDS, one workgroup a blob (adj_blob: k_adjacency_blob).  AdjMemStore: end and 32-bit
//            entries in device memory, ADJ_BLOCK half-edges a workgroup (adj_count, adj_scan, adj_fill, adj_twin as a kernel each).
//   group    G is the workgroup of ADJ_THREADS: each(f) runs f(tid, AdjLane &) for every thread (the kernel: its own; the host: all of them in
//            a shuffled order), sync() is its barrier, wave_scan() turns every lane's v into incl (inclusive over its wave) and tot (the
//            wave's sum), wave_carry() turns every lane's v into carry (the sum of v over the waves in front of its own), block_sums() leaves
//            the sums of c's three counts over the workgroup in thread 0's c, thread0(f) runs f(AdjLane &) for thread 0.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/corto_hip.h"

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define ADJ_HD __host__ __device__ __forceinline__          // (a call left standing takes the address of a lane's state: scratch)
#else
#define ADJ_HD inline
#endif
// k_adjacency.hip defines ADJ_KERNELS: pointers into device memory and into LDS carry their address space there (global_* / ds_* and never
// flat_*: kernels_common.h); everywhere else, and in the host pass, the qualifiers are empty
#if defined(ADJ_KERNELS) && defined(__HIP_DEVICE_COMPILE__)
#define ADJ_MEM __attribute__((address_space(1)))
#define ADJ_LDS __attribute__((address_space(3)))
#define ADJ_DEVICE_PASS 1
#else
#define ADJ_MEM
#define ADJ_LDS
#define ADJ_DEVICE_PASS 0
#endif

namespace corto_hip {

constexpr uint32_t ADJ_WAVE = 64, ADJ_WAVES = 4, ADJ_THREADS = ADJ_WAVE*ADJ_WAVES;
constexpr uint32_t ADJ_BLOCK = 256;                        // half-edges a workgroup of adjacency_count / _fill / _twin
// adjacency_blob's limit: a blob whose lists fit this much LDS, so that two workgroups share a CU's 160 KiB (a C4 unit needs about 33 KiB).
// NOBODY HAS MEASURED THIS THRESHOLD: it is the largest power of two that leaves room for two workgroups, chosen and not varied
// (profiles/adjacency.md says what was measured).  Its 16-bit entries hold a half-edge: 3*nface <= 65 536 as well
constexpr uint32_t ADJ_BLOB_LDS_MAX = 64u << 10;
constexpr uint32_t ADJ_BLOB_HALFEDGES_MAX = 65536;
static_assert(ADJ_BLOCK == ADJ_THREADS, "a thread a half-edge");

// sixteen bytes as one access (a plain vector: HIP's uint4 is a class whose assignment takes a generic `this`, which makes the store FLAT)
typedef uint32_t adj_u32x4 __attribute__((ext_vector_type(4)));

// LDS of a blob in adjacency_blob: the ends (rounded up to 16 bytes), then the entries
ADJ_HD uint64_t adj_ends_bytes(uint32_t nvert) { return (((uint64_t)nvert + 1)*4 + 15) & ~15ull; }
ADJ_HD uint64_t adj_blob_lds(uint32_t nvert, uint32_t nface) { return adj_ends_bytes(nvert) + (((uint64_t)nface*6 + 15) & ~15ull); }
ADJ_HD bool adj_in_blob(uint32_t nvert, uint32_t nface) { return (uint64_t)nface*3 <= ADJ_BLOB_HALFEDGES_MAX && adj_blob_lds(nvert, nface) <= ADJ_BLOB_LDS_MAX; }
// scratch of a bigger blob: the ends, the entries (32 bits each), and a record for a binding without one
struct AdjScratchLayout { uint64_t list, record, total; };
ADJ_HD AdjScratchLayout adj_scratch_layout(uint32_t nvert, uint32_t nface) {
	AdjScratchLayout l;
	l.list = adj_ends_bytes(nvert);
	l.record = l.list + (((uint64_t)nface*12 + 15) & ~15ull);
	l.total = l.record + 16;
	return l;
}

// ---- the index -----------------------------------------------------------------------------------------------------------------------------

struct AdjIn { ADJ_MEM const void *index; uint32_t index_u16, nface, nvert; };
ADJ_HD uint32_t adj_corner(const AdjIn &J, uint32_t k) {
	return J.index_u16 ? (uint32_t)((ADJ_MEM const uint16_t *)J.index)[k] : ((ADJ_MEM const uint32_t *)J.index)[k];
}
// half-edge h: from a to b, and whether its face is valid (three different corners, all below nvert)
struct AdjEdge { uint32_t a, b; bool valid; };
ADJ_HD AdjEdge adj_edge(const AdjIn &J, uint32_t h) {
	const uint32_t f3 = h/3*3, s = h - f3;
	const uint32_t c0 = adj_corner(J, f3), c1 = adj_corner(J, f3 + 1), c2 = adj_corner(J, f3 + 2);
	AdjEdge e;
	e.valid = c0 != c1 && c1 != c2 && c0 != c2 && c0 < J.nvert && c1 < J.nvert && c2 < J.nvert;
	e.a = s == 0 ? c0 : s == 1 ? c1 : c2;
	e.b = s == 0 ? c1 : s == 1 ? c2 : c0;
	return e;
}
// where half-edge h points (h is a list entry: its face is valid)
ADJ_HD uint32_t adj_head(const AdjIn &J, uint32_t h) {
	const uint32_t f3 = h/3*3, s = h - f3;
	return adj_corner(J, f3 + (s == 2 ? 0u : s + 1));
}

// ---- the two stores ------------------------------------------------------------------------------------------------------------------------

// add(v, d): end[v] += d, atomically; the value before
struct AdjLdsStore {
	ADJ_LDS uint32_t *end; ADJ_LDS uint16_t *list;
	ADJ_HD uint32_t add(uint32_t v, uint32_t d) const {
#if ADJ_DEVICE_PASS
		return __hip_atomic_fetch_add(end + v, d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#else
		const uint32_t old = end[v]; end[v] = old + d; return old;
#endif
	}
	ADJ_HD uint32_t get(uint32_t v) const { return end[v]; }
	ADJ_HD void put(uint32_t v, uint32_t x) const { end[v] = x; }
	ADJ_HD uint32_t entry(uint32_t p) const { return list[p]; }
	ADJ_HD void set_entry(uint32_t p, uint32_t h) const { list[p] = (uint16_t)h; }
};
struct AdjMemStore {
	ADJ_MEM uint32_t *end; ADJ_MEM uint32_t *list;
	ADJ_HD uint32_t add(uint32_t v, uint32_t d) const {
#if ADJ_DEVICE_PASS
		return __hip_atomic_fetch_add(end + v, d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
		const uint32_t old = end[v]; end[v] = old + d; return old;
#endif
	}
	ADJ_HD uint32_t get(uint32_t v) const { return end[v]; }
	ADJ_HD void put(uint32_t v, uint32_t x) const { end[v] = x; }
	ADJ_HD uint32_t entry(uint32_t p) const { return list[p]; }
	ADJ_HD void set_entry(uint32_t p, uint32_t h) const { list[p] = h; }
};

// a thread's state: the scan's value, its wave's inclusive sum and total, the carry in front of its wave; its share of the three counts
// (named fields, no array: a lane's state stays in registers)
struct AdjCounts { uint32_t boundary, duplicate, invalid; };
struct AdjLane { uint32_t v, incl, tot, carry, in; AdjCounts c; };

// ---- the phases: half-edges [h0, h1) by one workgroup, thread tid takes h0 + tid, + ADJ_THREADS, ... ----------------------------------------

template <class G, class S> ADJ_HD void adj_count(G &g, const AdjIn &J, const S &st, uint32_t h0, uint32_t h1) {
	g.each([&](uint32_t tid, AdjLane &) {
		for(uint64_t h = (uint64_t)h0 + tid; h < h1; h += ADJ_THREADS) {
			const AdjEdge e = adj_edge(J, (uint32_t)h);
			if(e.valid) (void)st.add(e.a, 1u);
		}
	});
}

// `end` (n = nvert + 1 words) becomes its inclusive prefix sum.  A wave takes a stretch of whole rounds of 64 words: it adds its stretch up,
// gets the sum of the stretches in front of it (wave_carry), and goes through it again round by round with a wave scan and a running carry
template <class G, class S> ADJ_HD void adj_scan(G &g, const S &st, uint32_t n) {
	const uint32_t rounds = (uint32_t)(((uint64_t)n + ADJ_THREADS - 1)/ADJ_THREADS);
	auto at = [&](uint32_t tid, uint32_t r) { return ((uint64_t)(tid/ADJ_WAVE)*rounds + r)*ADJ_WAVE + tid%ADJ_WAVE; };
	g.each([&](uint32_t tid, AdjLane &L) {
		uint32_t s = 0;
		for(uint32_t r = 0; r < rounds; r++) { const uint64_t i = at(tid, r); if(i < n) s += st.get((uint32_t)i); }
		L.v = s;
	});
	g.wave_carry();
	for(uint32_t r = 0; r < rounds; r++) {
		g.each([&](uint32_t tid, AdjLane &L) { const uint64_t i = at(tid, r); L.in = i < n; L.v = L.in ? st.get((uint32_t)i) : 0u; });
		g.wave_scan();
		g.each([&](uint32_t tid, AdjLane &L) { if(L.in) st.put((uint32_t)at(tid, r), L.carry + L.incl); L.carry += L.tot; });
	}
}

template <class G, class S> ADJ_HD void adj_fill(G &g, const AdjIn &J, const S &st, uint32_t h0, uint32_t h1) {
	g.each([&](uint32_t tid, AdjLane &) {
		for(uint64_t h = (uint64_t)h0 + tid; h < h1; h += ADJ_THREADS) {
			const AdjEdge e = adj_edge(J, (uint32_t)h);
			if(e.valid) st.set_entry(st.add(e.a, 0xFFFFFFFFu) - 1u, (uint32_t)h);
		}
	});
}

// the rule for one half-edge: its twin, and its share of the counts (as values: a count reached through a pointer chosen at run time would
// put the lane's state into scratch)
struct AdjTwin { uint32_t twin; AdjCounts c; };
template <class S> ADJ_HD AdjTwin adj_twin_of(const AdjIn &J, const S &st, uint32_t h) {
	const AdjEdge e = adj_edge(J, h);
	uint32_t t = CRTHIP_NO_TWIN;
	bool dup = false;
	if(e.valid) {
		for(uint32_t p = st.get(e.b), pe = st.get(e.b + 1); p < pe; p++) {          // b's list: the least b -> a
			const uint32_t o = st.entry(p);
			if(o < t && adj_head(J, o) == e.a) t = o;
		}
		for(uint32_t p = st.get(e.a), pe = st.get(e.a + 1); p < pe && !dup; p++) {  // a's list (h is in it): an a -> b below h
			const uint32_t o = st.entry(p);
			dup = o < h && adj_head(J, o) == e.b;
		}
	}
	return AdjTwin{t, AdjCounts{e.valid && t == CRTHIP_NO_TWIN ? 1u : 0u, dup ? 1u : 0u, e.valid ? 0u : 1u}};
}
template <class G, class S> ADJ_HD void adj_twin(G &g, const AdjIn &J, const S &st, ADJ_MEM uint32_t *twin, uint32_t h0, uint32_t h1) {
	g.each([&](uint32_t tid, AdjLane &L) {
		uint32_t nb = 0, nd = 0, ni = 0;
		for(uint64_t h = (uint64_t)h0 + tid; h < h1; h += ADJ_THREADS) {
			const AdjTwin r = adj_twin_of(J, st, (uint32_t)h);
			twin[h] = r.twin; nb += r.c.boundary; nd += r.c.duplicate; ni += r.c.invalid;
		}
		L.c = AdjCounts{nb, nd, ni};
	});
	g.block_sums();
}

// the record: written whole by the one workgroup of a blob, or zeroed (adjacency_offsets) and added to by every workgroup (adjacency_twin)
ADJ_HD void adj_record_store(ADJ_MEM crthip_adjacency_counts *rec, uint32_t halfedges, const AdjCounts &c) {
#if ADJ_DEVICE_PASS
	*(ADJ_MEM adj_u32x4 *)rec = adj_u32x4{halfedges, c.boundary, c.duplicate, c.invalid};
#else
	*rec = crthip_adjacency_counts{halfedges, c.boundary, c.duplicate, c.invalid};
#endif
}
ADJ_HD void adj_record_add(ADJ_MEM crthip_adjacency_counts *rec, const AdjCounts &c) {
#if ADJ_DEVICE_PASS
	ADJ_MEM uint32_t *w = (ADJ_MEM uint32_t *)rec;
	(void)__hip_atomic_fetch_add(w + 1, c.boundary, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	(void)__hip_atomic_fetch_add(w + 2, c.duplicate, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	(void)__hip_atomic_fetch_add(w + 3, c.invalid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
	rec->boundary += c.boundary; rec->duplicate += c.duplicate; rec->invalid += c.invalid;
#endif
}

// ---- partition 0: a blob by ONE workgroup, everything in LDS; rec may be null ----------------------------------------------------------------

template <class G> ADJ_HD void adj_blob(G &g, const AdjIn &J, const AdjLdsStore &st, ADJ_MEM uint32_t *twin, ADJ_MEM crthip_adjacency_counts *rec) {
	const uint32_t n = J.nvert + 1, H = 3*J.nface;
	g.each([&](uint32_t tid, AdjLane &) { for(uint32_t i = tid; i < n; i += ADJ_THREADS) st.put(i, 0u); });
	g.sync();
	adj_count(g, J, st, 0, H);
	g.sync();
	adj_scan(g, st, n);
	g.sync();
	adj_fill(g, J, st, 0, H);
	g.sync();
	adj_twin(g, J, st, twin, 0, H);
	g.thread0([&](AdjLane &L) { if(rec) adj_record_store(rec, H, L.c); });
}

// ---- partition 1: workgroup k of a blob's ceil(3*nface/ADJ_BLOCK) in adjacency_count / _fill / _twin, one workgroup in adjacency_offsets ------

ADJ_HD uint32_t adj_blocks(uint32_t nface) { return (uint32_t)(((uint64_t)nface*3 + ADJ_BLOCK - 1)/ADJ_BLOCK); }
ADJ_HD uint32_t adj_block_end(uint32_t nface, uint32_t k) { const uint64_t H = (uint64_t)nface*3, e = ((uint64_t)k + 1)*ADJ_BLOCK; return (uint32_t)(e < H ? e : H); }
template <class G> ADJ_HD void adj_count_block(G &g, const AdjIn &J, const AdjMemStore &st, uint32_t k) { adj_count(g, J, st, k*ADJ_BLOCK, adj_block_end(J.nface, k)); }
template <class G> ADJ_HD void adj_offsets(G &g, const AdjIn &J, const AdjMemStore &st, ADJ_MEM crthip_adjacency_counts *rec) {
	adj_scan(g, st, J.nvert + 1);
	g.thread0([&](AdjLane &) { adj_record_store(rec, 3*J.nface, AdjCounts{0, 0, 0}); });
}
template <class G> ADJ_HD void adj_fill_block(G &g, const AdjIn &J, const AdjMemStore &st, uint32_t k) { adj_fill(g, J, st, k*ADJ_BLOCK, adj_block_end(J.nface, k)); }
template <class G> ADJ_HD void adj_twin_block(G &g, const AdjIn &J, const AdjMemStore &st, ADJ_MEM uint32_t *twin, ADJ_MEM crthip_adjacency_counts *rec, uint32_t k) {
	adj_twin(g, J, st, twin, k*ADJ_BLOCK, adj_block_end(J.nface, k));
	g.thread0([&](AdjLane &L) { adj_record_add(rec, L.c); });
}

// what crthip_batch_bind_adjacency (and the hook) ask of a binding on a blob of nface faces, behind "no such blob" and "a point cloud", in the
// header's order; null: fine
inline const char *adjacency_binding_error(const crthip_adjacency_binding *a, uint32_t nface) {
	if(!a->twin || (uintptr_t)a->twin % 4 || (uintptr_t)a->counts % 16) return "adjacency: twin is NULL or not 4-byte aligned, or counts is not 16-byte aligned";
	if(a->reserved) return "adjacency: reserved is not 0";
	if((uint64_t)a->capacity < (uint64_t)nface*3) return "adjacency: capacity is below 3*nface";
	return nullptr;
}

} // namespace corto_hip
