// bvh.h — crthip_batch_bind_bvh: a binary triangle BVH of a blob's integer positions and its index (include/corto_hip.h has the contract).  The
// face box, the key, the sort steps, the split search, the refit step and both partitions as __host__ __device__ code over the workgroup
// abstraction of lod.h, so that the host runs the very same source in the kernels' partitions (crthip_bvh_model, bvh_host.cpp).
//
//   boxes    a face's box is the signed minimum and maximum of its three corners' integers; an ABSENT face (a corner >= nvert: compared, never
//            an address) has the empty box.  The extent L, H of the box mids is six atomic MAXIMA over order-preserving unsigned words - the
//            minimum as the maximum of the complement - so that a zeroed record is the empty extent, and a seventh word counts the absent faces
//   keys     a 30-bit Morton code of the mid's cell in the 1024^3 grid over [L, H]; absent faces get 0x80000000, behind every present one
//   sort     a stable LSD radix sort of (key, face).  Its ONE step is bvh_split: a stable split of n pairs in LDS by one key bit, a thread its
//            consecutive pairs, one block scan.  bvh_blob runs it over bits 0..29 (and 31 where a face is absent) on the whole blob, ids in 16
//            bits.  Bigger blobs sort 8 bits a pass in four passes over tiles of BVH_TILE pairs: a digit histogram a tile (bvh_sort_count), one
//            exclusive scan a blob over its digit-major table (bvh_sort_offsets), and a tile sorted by the digit with eight splits, then
//            scattered to its digits' places (bvh_sort_scatter).  Every step is stable, so the order is that of (key, face)
//   tree     Karras 2012, a thread an internal node: its direction from its two neighbours' prefixes, its far end by doubling, its split by
//            bisection, all on the codes (key << 32 | rank).  Node ids are the contract's: the left child of a split m is m, the right m + 1
//   refit    a thread a leaf climbs: it stores its node, then ARRIVES at the parent with ONE atomic add of its height + 1.  The first arrival
//            (the word was 0) leaves; the second finds the sibling's height in the word, reads the sibling's box, stores the parent and climbs.
//            The arrival is acquire-release: it releases the first arrival's node stores and acquires them for the second, at workgroup scope
//            on a counter in LDS (bvh_blob: both threads are in the one workgroup) and at agent scope on a counter in memory (bvh_refit: a
//            release fence, a wait for its write-back, the add, and an acquire fence for the second arrival alone).  Nobody polls.  The thread that finds no parent is at the root and stores the record
//   order    which thread arrives first changes with the schedule; a box is a union, a height a maximum, an extent six maxima: no byte does.
//   group    G is the workgroup of BVH_THREADS (lod.h): each(f) runs f(tid, LodLane &) for every thread, sync() is its barrier, block_scan()
//            leaves in x the sum of c over the threads in front and in t the sum over all.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/corto_hip.h"
#include "lod.h"

namespace corto_hip {

constexpr uint32_t BVH_THREADS = LOD_THREADS;
// bvh_blob's limit: one workgroup a blob of up to 4 096 faces (a C4 unit), 16 pairs a thread and ids in 16 bits.  CHOSEN, NOT TUNED: nobody has
// varied it (profiles/bvh.md says what was measured)
constexpr uint32_t BVH_BLOB_FACES = 4096;
constexpr uint32_t BVH_BLOB_CHUNK = BVH_BLOB_FACES/BVH_THREADS;
// the bigger blobs' sort tile: 8 pairs a thread.  Chosen, not tuned, likewise
constexpr uint32_t BVH_TILE_CHUNK = 8;
constexpr uint32_t BVH_TILE = BVH_TILE_CHUNK*BVH_THREADS;
constexpr uint32_t BVH_DIGIT_BITS = 8, BVH_DIGITS = 1u << BVH_DIGIT_BITS, BVH_PASSES = 32/BVH_DIGIT_BITS;
constexpr uint32_t BVH_BLOCK = 256;                        // faces (and nodes, and leaves) a workgroup of bvh_boxes, _keys, _tree, _refit
constexpr uint32_t BVH_ABSENT_KEY = 0x80000000u;
static_assert(BVH_DIGITS == BVH_THREADS && BVH_BLOCK == BVH_THREADS, "a thread a digit, a thread a face");
static_assert(BVH_PASSES % 2 == 0, "the sorted pairs end in the buffer they started in");

WELD_HD bool bvh_in_blob(uint32_t nface) { return nface <= BVH_BLOB_FACES; }
WELD_HD uint32_t bvh_fblocks(uint32_t nface) { return (uint32_t)(((uint64_t)nface + BVH_BLOCK - 1)/BVH_BLOCK); }
WELD_HD uint32_t bvh_tiles(uint32_t nface) { return (uint32_t)(((uint64_t)nface + BVH_TILE - 1)/BVH_TILE); }
WELD_HD uint32_t bvh_clz32(uint32_t x) { return (uint32_t)__builtin_clz(x); }   // (x != 0)

// ---- words that threads meet at: the extent's seven, the arrival counters ---------------------------------------------------------------------

enum { BVH_W_LO = 0, BVH_W_HI = 3, BVH_W_ABSENT = 6, BVH_EXT_WORDS = 8 };

constexpr int BVH_WAIT_VMCNT0 = 0x0F70;                    // s_waitcnt vmcnt(0) alone, gfx9 encoding: expcnt and lgkmcnt at their maxima

// raise(i, x): word = max(word, x); add(i, x); arrive(i, x): word += x with acquire-release order, the word before.  get: a plain load, behind a
// barrier or in a later kernel
struct BvhLdsWords {
	WELD_LDS uint32_t *w;
	WELD_HD uint32_t get(uint32_t i) const { return w[i]; }
	WELD_HD void put(uint32_t i, uint32_t x) const { w[i] = x; }
	WELD_HD void raise(uint32_t i, uint32_t x) const {
#if WELD_DEVICE_PASS
		(void)__hip_atomic_fetch_max(w + i, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#else
		if(x > w[i]) w[i] = x;
#endif
	}
	WELD_HD void add(uint32_t i, uint32_t x) const {
#if WELD_DEVICE_PASS
		(void)__hip_atomic_fetch_add(w + i, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#else
		w[i] += x;
#endif
	}
	WELD_HD uint32_t arrive(uint32_t i, uint32_t x) const {
#if WELD_DEVICE_PASS
		// (the thread's node stores have left before the add: the compiler's workgroup-scope release waits for LDS only)
		__builtin_amdgcn_s_waitcnt(BVH_WAIT_VMCNT0);
		return __hip_atomic_fetch_add(w + i, x, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
#else
		const uint32_t old = w[i]; w[i] = old + x; return old;
#endif
	}
};
struct BvhMemWords {
	WELD_MEM uint32_t *w;
	WELD_HD uint32_t get(uint32_t i) const { return w[i]; }
	WELD_HD void raise(uint32_t i, uint32_t x) const {
#if WELD_DEVICE_PASS
		(void)__hip_atomic_fetch_max(w + i, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
		if(x > w[i]) w[i] = x;
#endif
	}
	WELD_HD void add(uint32_t i, uint32_t x) const {
#if WELD_DEVICE_PASS
		(void)__hip_atomic_fetch_add(w + i, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
		w[i] += x;
#endif
	}
	WELD_HD uint32_t arrive(uint32_t i, uint32_t x) const {
#if WELD_DEVICE_PASS
		// release: the write-back of this thread's node stores, and a wait for it IN FRONT OF the add - an acquire-release add alone compiles
		// to the write-back, the add and no wait between them.  acquire: the second arrival alone reads behind it
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
		__builtin_amdgcn_s_waitcnt(BVH_WAIT_VMCNT0);
		const uint32_t old = __hip_atomic_fetch_add(w + i, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		if(old) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
		return old;
#else
		const uint32_t old = w[i]; w[i] = old + x; return old;
#endif
	}
};

// ---- the face box and the key -------------------------------------------------------------------------------------------------------------------

struct BvhBox { int32_t lo[3], hi[3]; };
struct BvhFace { BvhBox b; uint32_t present; };
WELD_HD BvhFace bvh_face(const WeldIn &J, uint32_t f) {
	const uint32_t a = weld_corner(J, (uint64_t)f*3), b = weld_corner(J, (uint64_t)f*3 + 1), c = weld_corner(J, (uint64_t)f*3 + 2);
	BvhFace r;
	r.present = a < J.nvert && b < J.nvert && c < J.nvert;
	if(r.present) {
		WELD_MEM const int32_t *pa = J.position + (uint64_t)a*3, *pb = J.position + (uint64_t)b*3, *pc = J.position + (uint64_t)c*3;
#pragma unroll
		for(uint32_t q = 0; q < 3; q++) {
			const int32_t x = pa[q], y = pb[q], z = pc[q];
			const int32_t lo = x < y ? x : y, hi = x < y ? y : x;
			r.b.lo[q] = lo < z ? lo : z; r.b.hi[q] = hi < z ? z : hi;
		}
	} else {
#pragma unroll
		for(uint32_t q = 0; q < 3; q++) { r.b.lo[q] = INT32_MAX; r.b.hi[q] = INT32_MIN; }
	}
	return r;
}
WELD_HD void bvh_unite(BvhBox &b, const BvhBox &s) {
#pragma unroll
	for(uint32_t q = 0; q < 3; q++) { if(s.lo[q] < b.lo[q]) b.lo[q] = s.lo[q]; if(s.hi[q] > b.hi[q]) b.hi[q] = s.hi[q]; }
}
// the box's mid as a word whose unsigned order is the signed one
WELD_HD uint32_t bvh_mid(const BvhBox &b, uint32_t q) { return (uint32_t)(int32_t)(((int64_t)b.lo[q] + b.hi[q]) >> 1) ^ 0x80000000u; }
// a present face goes into the extent
template <class W> WELD_HD void bvh_extend(const W &w, const BvhBox &b) {
#pragma unroll
	for(uint32_t q = 0; q < 3; q++) { const uint32_t m = bvh_mid(b, q); w.raise(BVH_W_LO + q, ~m); w.raise(BVH_W_HI + q, m); }
}
// L as (uint32)L[c], and the shift k
struct BvhGrid { uint32_t L[3], k; };
template <class W> WELD_HD BvhGrid bvh_grid(const W &w, uint32_t nface) {
	BvhGrid g; uint32_t E = 0;
#pragma unroll
	for(uint32_t q = 0; q < 3; q++) {
		const uint32_t lo = ~w.get(BVH_W_LO + q) ^ 0x80000000u, hi = w.get(BVH_W_HI + q) ^ 0x80000000u;
		g.L[q] = lo;
		if(hi - lo > E) E = hi - lo;
	}
	if(w.get(BVH_W_ABSENT) >= nface) E = 0;                                // (no face present: L and H play no part)
	const uint32_t bits = E ? 32u - bvh_clz32(E) : 0u;
	g.k = bits > 10u ? bits - 10u : 0u;
	return g;
}
WELD_HD uint32_t bvh_spread(uint32_t x) {                                   // bit i of a 10-bit x to bit 3i
	x = (x | (x << 16)) & 0x030000FFu; x = (x | (x << 8)) & 0x0300F00Fu; x = (x | (x << 4)) & 0x030C30C3u; x = (x | (x << 2)) & 0x09249249u;
	return x;
}
WELD_HD uint32_t bvh_key(const BvhGrid &g, const BvhFace &f) {
	if(!f.present) return BVH_ABSENT_KEY;
	uint32_t cell[3];
#pragma unroll
	for(uint32_t q = 0; q < 3; q++) cell[q] = (((bvh_mid(f.b, q) ^ 0x80000000u) - g.L[q]) >> g.k) & 1023u;
	return (bvh_spread(cell[0]) << 2) | (bvh_spread(cell[1]) << 1) | bvh_spread(cell[2]);
}

// ---- the sort's one step: a stable split of n pairs in LDS by key bit `bit`, thread tid owns the C consecutive pairs from tid*C -------------------
// (the pairs of ka / ia are final: the caller's barrier; kb / ib are final behind this one's)

template <uint32_t C, class G, class I> WELD_HD void bvh_split(G &g, WELD_LDS const uint32_t *ka, WELD_LDS const I *ia, WELD_LDS uint32_t *kb, WELD_LDS I *ib,
	uint32_t n, uint32_t bit) {
	g.each([&](uint32_t tid, LodLane &L) {
		uint32_t z = 0;
		for(uint32_t e = 0; e < C; e++) { const uint32_t i = tid*C + e; if(i < n) z += !((ka[i] >> bit) & 1u); }
		L.c = z;
	});
	g.block_scan();
	g.each([&](uint32_t tid, LodLane &L) {
		uint32_t z = L.x;                                                   // the zeros in front of pair i; i - z: the ones
		for(uint32_t e = 0; e < C; e++) {
			const uint32_t i = tid*C + e;
			if(i >= n) break;
			const uint32_t k = ka[i], one = (k >> bit) & 1u;
			const uint32_t at = one ? L.t + (i - z) : z;
			kb[at] = k; ib[at] = ia[i];
			z += !one;
		}
	});
	g.sync();
}

// ---- the split search ----------------------------------------------------------------------------------------------------------------------------

struct BvhLdsKeys { WELD_LDS const uint32_t *k; WELD_HD uint32_t operator()(uint32_t j) const { return k[j]; } };
struct BvhMemKeys { WELD_MEM const uint32_t *k; WELD_HD uint32_t operator()(uint32_t j) const { return k[j]; } };
// the common prefix of codes i and j (key << 32 | rank), -1 beyond the ends; j != i
template <class K> WELD_HD int32_t bvh_delta(const K &key, uint32_t F, uint32_t i, uint32_t ki, int64_t j) {
	if(j < 0 || j >= (int64_t)F) return -1;
	const uint32_t kj = key((uint32_t)j);
	return (int32_t)(ki != kj ? bvh_clz32(ki ^ kj) : 32u + bvh_clz32(i ^ (uint32_t)j));
}
struct BvhSplit { uint32_t left, right; };
// internal node i of F >= 2 sorted codes: its two children's node ids
template <class K> WELD_HD BvhSplit bvh_split_of(const K &key, uint32_t F, uint32_t i) {
	const uint32_t ki = key(i);
	const int64_t d = bvh_delta(key, F, i, ki, (int64_t)i + 1) > bvh_delta(key, F, i, ki, (int64_t)i - 1) ? 1 : -1;
	const int32_t dmin = bvh_delta(key, F, i, ki, (int64_t)i - d);
	int64_t lmax = 2;
	while(bvh_delta(key, F, i, ki, (int64_t)i + lmax*d) > dmin) lmax <<= 1;
	int64_t l = 0;
	for(int64_t t = lmax >> 1; t >= 1; t >>= 1) if(bvh_delta(key, F, i, ki, (int64_t)i + (l + t)*d) > dmin) l += t;
	const int64_t j = (int64_t)i + l*d;
	const int32_t dn = bvh_delta(key, F, i, ki, j);
	int64_t s = 0, t = l;
	do {
		t = (t + 1) >> 1;
		if(bvh_delta(key, F, i, ki, (int64_t)i + (s + t)*d) > dn) s += t;
	} while(t > 1);
	const int64_t m = (int64_t)i + s*d + (d < 0 ? -1 : 0);
	const int64_t a = j < (int64_t)i ? j : (int64_t)i, b = j < (int64_t)i ? (int64_t)i : j;
	BvhSplit r;
	r.left = a == m ? F - 1 + (uint32_t)m : (uint32_t)m;
	r.right = b == m + 1 ? F - 1 + (uint32_t)m + 1 : (uint32_t)m + 1;
	return r;
}

// ---- the nodes and the refit step --------------------------------------------------------------------------------------------------------------

WELD_HD void bvh_node_store(WELD_MEM crthip_bvh_node *nodes, uint32_t n, const BvhBox &b, uint32_t left, uint32_t right) {
#if WELD_DEVICE_PASS
	WELD_MEM weld_u32x4 *p = (WELD_MEM weld_u32x4 *)(nodes + n);
	p[0] = weld_u32x4{(uint32_t)b.lo[0], (uint32_t)b.lo[1], (uint32_t)b.lo[2], left};
	p[1] = weld_u32x4{(uint32_t)b.hi[0], (uint32_t)b.hi[1], (uint32_t)b.hi[2], right};
#else
	nodes[n] = crthip_bvh_node{{b.lo[0], b.lo[1], b.lo[2]}, left, {b.hi[0], b.hi[1], b.hi[2]}, right};
#endif
}
WELD_HD BvhBox bvh_node_box(WELD_MEM const crthip_bvh_node *nodes, uint32_t n) {
	BvhBox b;
#if WELD_DEVICE_PASS
	WELD_MEM const weld_u32x4 *p = (WELD_MEM const weld_u32x4 *)(nodes + n);
	const weld_u32x4 lo = p[0], hi = p[1];
	b.lo[0] = (int32_t)lo.x; b.lo[1] = (int32_t)lo.y; b.lo[2] = (int32_t)lo.z; b.hi[0] = (int32_t)hi.x; b.hi[1] = (int32_t)hi.y; b.hi[2] = (int32_t)hi.z;
#else
	for(uint32_t q = 0; q < 3; q++) { b.lo[q] = nodes[n].min[q]; b.hi[q] = nodes[n].max[q]; }
#endif
	return b;
}
WELD_HD void bvh_record_store(WELD_MEM crthip_bvh_counts *rec, uint32_t nface, uint32_t absent, uint32_t height) {
#if WELD_DEVICE_PASS
	*(WELD_MEM weld_u32x4 *)rec = weld_u32x4{2u*nface - 1u, nface, absent, height};
#else
	*rec = crthip_bvh_counts{2u*nface - 1u, nface, absent, height};
#endif
}

// where the climb finds the tree.  bvh_blob: parents and child pairs in LDS, 16 bits an id (0xFFFF: no parent), the counters in LDS
struct BvhLdsTree {
	WELD_LDS const uint32_t *lr; WELD_LDS const uint16_t *par; BvhLdsWords count;
	WELD_HD uint32_t parent(uint32_t n) const { const uint32_t p = par[n]; return p == 0xFFFFu ? CRTHIP_NO_NODE : p; }
	WELD_HD uint32_t left(uint32_t p) const { return lr[p] & 0xFFFFu; }
	WELD_HD uint32_t right(uint32_t p) const { return lr[p] >> 16; }
	WELD_HD uint32_t arrive(uint32_t p, uint32_t x) const { return count.arrive(p, x); }
};
// bigger blobs: the parent array and the nodes' child words, both final since bvh_tree; the counters in scratch, zeroed by the FillJob
struct BvhMemTree {
	WELD_MEM const uint32_t *par; WELD_MEM const crthip_bvh_node *nodes; BvhMemWords count;
	WELD_HD uint32_t parent(uint32_t n) const { return par[n]; }
	WELD_HD uint32_t left(uint32_t p) const { return nodes[p].left; }
	WELD_HD uint32_t right(uint32_t p) const { return nodes[p].right; }
	WELD_HD uint32_t arrive(uint32_t p, uint32_t x) const { return count.arrive(p, x); }
};
// leaf j (face f, box b) is stored, then climbs.  A path has at most 64 edges: the loop is bounded by that
template <class T> WELD_HD void bvh_climb(const T &tree, WELD_MEM crthip_bvh_node *nodes, WELD_MEM crthip_bvh_counts *rec, uint32_t nface, uint32_t absent,
	uint32_t j, uint32_t f, BvhBox b) {
	uint32_t n = nface - 1 + j, h = 0;
	bvh_node_store(nodes, n, b, f, CRTHIP_BVH_LEAF);
	for(uint32_t edge = 0; edge <= 64; edge++) {
		const uint32_t p = tree.parent(n);
		if(p == CRTHIP_NO_NODE) { if(rec) bvh_record_store(rec, nface, absent, h); return; }
		const uint32_t old = tree.arrive(p, h + 1);
		if(!old) return;                                                    // the first arrival leaves; its node's stores are released
		const uint32_t l = tree.left(p), r = tree.right(p);
		bvh_unite(b, bvh_node_box(nodes, l == n ? r : l));                   // (behind the acquire)
		h = (h > old - 1 ? h : old - 1) + 1;
		bvh_node_store(nodes, p, b, l, r);
		n = p;
	}
}

// ---- partition 0: a blob of up to BVH_BLOB_FACES faces by ONE workgroup ------------------------------------------------------------------------------

// the workgroup's LDS: eight scalar words, two key arrays, the counters, two id arrays and the parents, each for the face count rounded up to 8
WELD_HD uint32_t bvh_blob_round(uint32_t nface) { return (nface + 7u) & ~7u; }
WELD_HD uint32_t bvh_blob_lds_bytes(uint32_t nface) { return BVH_EXT_WORDS*4u + 20u*bvh_blob_round(nface); }
struct BvhBlobLds { WELD_LDS uint32_t *ext, *key[2], *count; WELD_LDS uint16_t *id[2], *parent; };
WELD_HD BvhBlobLds bvh_blob_carve(WELD_LDS uint8_t *p, uint32_t nface) {
	const uint32_t R = bvh_blob_round(nface);
	BvhBlobLds l;
	l.ext = (WELD_LDS uint32_t *)p; p += BVH_EXT_WORDS*4u;
	l.key[0] = (WELD_LDS uint32_t *)p; p += 4u*R;
	l.key[1] = (WELD_LDS uint32_t *)p; p += 4u*R;
	l.count = (WELD_LDS uint32_t *)p; p += 4u*R;
	l.id[0] = (WELD_LDS uint16_t *)p; p += 2u*R;
	l.id[1] = (WELD_LDS uint16_t *)p; p += 2u*R;
	l.parent = (WELD_LDS uint16_t *)p;                                      // 2*nface - 1 entries in 4*R bytes
	return l;
}

// parent, order and rec may be null
template <class G> WELD_HD void bvh_blob(G &g, const WeldIn &J, WELD_LDS uint8_t *lds, WELD_MEM crthip_bvh_node *nodes, WELD_MEM uint32_t *parent,
	WELD_MEM uint32_t *order, WELD_MEM crthip_bvh_counts *rec) {
	const uint32_t F = J.nface;
	const BvhBlobLds S = bvh_blob_carve(lds, F);
	const BvhLdsWords ext{S.ext};
	g.each([&](uint32_t tid, LodLane &) { if(tid < BVH_EXT_WORDS) ext.put(tid, 0u); });
	g.sync();
	// the extent of the mids and the absent faces
	g.each([&](uint32_t tid, LodLane &) {
		for(uint32_t e = 0; e < BVH_BLOB_CHUNK; e++) {
			const uint32_t f = tid*BVH_BLOB_CHUNK + e;
			if(f >= F) break;
			const BvhFace t = bvh_face(J, f);
			if(t.present) bvh_extend(ext, t.b); else ext.add(BVH_W_ABSENT, 1u);
		}
	});
	g.sync();
	// the keys, a thread its consecutive faces
	g.each([&](uint32_t tid, LodLane &) {
		const BvhGrid grid = bvh_grid(ext, F);
		for(uint32_t e = 0; e < BVH_BLOB_CHUNK; e++) {
			const uint32_t f = tid*BVH_BLOB_CHUNK + e;
			if(f >= F) break;
			S.key[0][f] = bvh_key(grid, bvh_face(J, f)); S.id[0][f] = (uint16_t)f;
		}
	});
	g.sync();
	// the sort: 30 key bits, and bit 31 where a face is absent
	const uint32_t absent = ext.get(BVH_W_ABSENT);
	// (the two buffers as named pointers that swap: a pointer array indexed at run time would live in scratch)
	WELD_LDS uint32_t *keys = S.key[0], *lr = S.key[1];
	WELD_LDS uint16_t *ids = S.id[0], *ids_b = S.id[1];
	for(uint32_t bit = 0; bit < 32; bit++) {
		if(bit == 30 || (bit == 31 && !absent)) continue;
		bvh_split<BVH_BLOB_CHUNK>(g, keys, ids, lr, ids_b, F, bit);
		WELD_LDS uint32_t *k = keys; keys = lr; lr = k;
		WELD_LDS uint16_t *i = ids; ids = ids_b; ids_b = i;
	}
	// (lr, the other key array, is free now: the child pairs)
	// the tree: a thread an internal node; the counters start at 0
	g.each([&](uint32_t tid, LodLane &) {
		for(uint32_t i = tid; i + 1 < F; i += BVH_THREADS) {
			const BvhSplit s = bvh_split_of(BvhLdsKeys{keys}, F, i);
			lr[i] = s.left | (s.right << 16);
			S.parent[s.left] = (uint16_t)i; S.parent[s.right] = (uint16_t)i;
			S.count[i] = 0u;
			if(parent) { parent[s.left] = i; parent[s.right] = i; }
		}
		if(tid == 0) { S.parent[0] = 0xFFFFu; if(parent) parent[0] = CRTHIP_NO_NODE; }
		if(order) for(uint32_t j = tid; j < F; j += BVH_THREADS) order[j] = ids[j];
	});
	g.sync();
	// the refit: a thread a leaf
	g.each([&](uint32_t tid, LodLane &) {
		const BvhLdsTree tree{lr, S.parent, BvhLdsWords{S.count}};
		for(uint32_t j = tid; j < F; j += BVH_THREADS) {
			const uint32_t f = ids[j];
			bvh_climb(tree, nodes, rec, F, absent, j, f, bvh_face(J, f).b);
		}
	});
}

// ---- partition 1: bigger blobs, everything in scratch ------------------------------------------------------------------------------------------------

// a blob's block of scratch: the extent's words and the arrival counters - ONE range, zeroed by one FillJob -, the pairs twice, the digit-major
// histogram of the tiles, and a parent array for a binding without one
struct BvhScratchLayout { uint64_t ext, count, zero_bytes, key[2], id[2], hist, parent, total; };
WELD_HD BvhScratchLayout bvh_scratch_layout(uint32_t nface, bool own_parent) {
	const uint64_t R = ((uint64_t)nface + 3u) & ~(uint64_t)3u;
	BvhScratchLayout l;
	l.ext = 0; l.count = BVH_EXT_WORDS*4u; l.zero_bytes = l.count + 4*R;
	l.key[0] = l.zero_bytes; l.key[1] = l.key[0] + 4*R; l.id[0] = l.key[1] + 4*R; l.id[1] = l.id[0] + 4*R;
	l.hist = l.id[1] + 4*R;
	l.parent = l.hist + (uint64_t)BVH_DIGITS*bvh_tiles(nface)*4u;
	l.total = l.parent + (own_parent ? 8*R : 0u);
	return l;
}
struct BvhBig { WELD_MEM uint32_t *ext, *count, *key[2], *id[2], *hist; };
WELD_HD BvhBig bvh_big_carve(WELD_MEM uint8_t *p, uint32_t nface) {
	const BvhScratchLayout l = bvh_scratch_layout(nface, false);
	BvhBig s;
	s.ext = (WELD_MEM uint32_t *)(p + l.ext); s.count = (WELD_MEM uint32_t *)(p + l.count);
	s.key[0] = (WELD_MEM uint32_t *)(p + l.key[0]); s.key[1] = (WELD_MEM uint32_t *)(p + l.key[1]);
	s.id[0] = (WELD_MEM uint32_t *)(p + l.id[0]); s.id[1] = (WELD_MEM uint32_t *)(p + l.id[1]);
	s.hist = (WELD_MEM uint32_t *)(p + l.hist);
	return s;
}
WELD_HD uint32_t bvh_block_end(uint32_t n, uint32_t k, uint32_t block) { const uint64_t e = ((uint64_t)k + 1)*block; return e < n ? (uint32_t)e : n; }

// bvh_boxes, workgroup k of ceil(F/BVH_BLOCK): a thread a face into the workgroup's extent in LDS (lext: BVH_EXT_WORDS words), then seven atomics
// a workgroup into the blob's
template <class G> WELD_HD void bvh_boxes_block(G &g, const WeldIn &J, const BvhBig &S, WELD_LDS uint32_t *lext, uint32_t k) {
	const BvhLdsWords le{lext};
	const BvhMemWords ext{S.ext};
	g.each([&](uint32_t tid, LodLane &) { if(tid < BVH_EXT_WORDS) le.put(tid, 0u); });
	g.sync();
	g.each([&](uint32_t tid, LodLane &) {
		const uint64_t f = (uint64_t)k*BVH_BLOCK + tid;
		if(f >= J.nface) return;
		const BvhFace t = bvh_face(J, (uint32_t)f);
		if(t.present) bvh_extend(le, t.b); else le.add(BVH_W_ABSENT, 1u);
	});
	g.sync();
	g.each([&](uint32_t tid, LodLane &) {
		if(tid < BVH_W_ABSENT) ext.raise(tid, le.get(tid));
		else if(tid == BVH_W_ABSENT && le.get(tid)) ext.add(tid, le.get(tid));
	});
}
// bvh_keys: a thread a face; the extent is final since bvh_boxes
template <class G> WELD_HD void bvh_keys_block(G &g, const WeldIn &J, const BvhBig &S, uint32_t k) {
	g.each([&](uint32_t tid, LodLane &) {
		const uint64_t f = (uint64_t)k*BVH_BLOCK + tid;
		if(f >= J.nface) return;
		S.key[0][f] = bvh_key(bvh_grid(BvhMemWords{S.ext}, J.nface), bvh_face(J, (uint32_t)f)); S.id[0][f] = (uint32_t)f;
	});
}
WELD_HD uint32_t bvh_digit(uint32_t key, uint32_t pass) { return (key >> (pass*BVH_DIGIT_BITS)) & (BVH_DIGITS - 1u); }
// bvh_sort_count, tile k of pass `pass`: the tile's digit histogram (lh: BVH_DIGITS words of LDS) to column k of the digit-major table
template <class G> WELD_HD void bvh_sort_count_tile(G &g, uint32_t nface, const BvhBig &S, WELD_LDS uint32_t *lh, uint32_t pass, uint32_t k) {
	WELD_MEM const uint32_t *keys = pass & 1u ? S.key[1] : S.key[0];
	const BvhLdsWords h{lh};
	const uint32_t nt = bvh_tiles(nface), f0 = k*BVH_TILE, f1 = bvh_block_end(nface, k, BVH_TILE);
	g.each([&](uint32_t tid, LodLane &) { h.put(tid, 0u); });
	g.sync();
	g.each([&](uint32_t tid, LodLane &) { for(uint64_t f = (uint64_t)f0 + tid; f < f1; f += BVH_THREADS) h.add(bvh_digit(keys[f], pass), 1u); });
	g.sync();
	g.each([&](uint32_t tid, LodLane &) { S.hist[(uint64_t)tid*nt + k] = h.get(tid); });
}
// bvh_sort_offsets, one workgroup a blob: the exclusive scan of the table in rounds of BVH_THREADS words
template <class G> WELD_HD void bvh_sort_offsets_job(G &g, uint32_t nface, const BvhBig &S) {
	const uint64_t n = (uint64_t)BVH_DIGITS*bvh_tiles(nface);
	g.each([&](uint32_t, LodLane &L) { L.run = 0; });
	for(uint64_t r = 0; r < n; r += BVH_THREADS) {
		g.each([&](uint32_t tid, LodLane &L) { L.c = r + tid < n ? S.hist[r + tid] : 0u; });
		g.block_scan();
		g.each([&](uint32_t tid, LodLane &L) { if(r + tid < n) S.hist[r + tid] = L.run + L.x; L.run += L.t; });
	}
}
// bvh_sort_scatter, tile k: the tile's pairs into LDS, eight stable splits by the digit's bits, the first place of every digit (first:
// BVH_DIGITS words), and every pair to its digit's place: the table's word plus its rank among the tile's pairs of that digit
struct BvhTileLds { WELD_LDS uint32_t *key[2], *id[2], *first; };
constexpr uint32_t BVH_TILE_LDS = 16u*BVH_TILE + 4u*BVH_DIGITS;
WELD_HD BvhTileLds bvh_tile_carve(WELD_LDS uint8_t *p) {
	BvhTileLds l;
	l.key[0] = (WELD_LDS uint32_t *)p; l.key[1] = l.key[0] + BVH_TILE; l.id[0] = l.key[1] + BVH_TILE; l.id[1] = l.id[0] + BVH_TILE; l.first = l.id[1] + BVH_TILE;
	return l;
}
template <class G> WELD_HD void bvh_sort_scatter_tile(G &g, uint32_t nface, const BvhBig &S, WELD_LDS uint8_t *lds, uint32_t pass, uint32_t k) {
	const BvhTileLds T = bvh_tile_carve(lds);
	WELD_MEM const uint32_t *ka = pass & 1u ? S.key[1] : S.key[0], *ia = pass & 1u ? S.id[1] : S.id[0];
	WELD_MEM uint32_t *kb = pass & 1u ? S.key[0] : S.key[1], *ib = pass & 1u ? S.id[0] : S.id[1];
	const uint32_t nt = bvh_tiles(nface), f0 = k*BVH_TILE, n = bvh_block_end(nface, k, BVH_TILE) - f0;
	g.each([&](uint32_t tid, LodLane &) { for(uint32_t i = tid; i < n; i += BVH_THREADS) { T.key[0][i] = ka[(uint64_t)f0 + i]; T.id[0][i] = ia[(uint64_t)f0 + i]; } });
	g.sync();
	// (an even number of splits: the pairs end where they were loaded)
	for(uint32_t bit = 0; bit < BVH_DIGIT_BITS; bit += 2) {
		bvh_split<BVH_TILE_CHUNK>(g, T.key[0], T.id[0], T.key[1], T.id[1], n, pass*BVH_DIGIT_BITS + bit);
		bvh_split<BVH_TILE_CHUNK>(g, T.key[1], T.id[1], T.key[0], T.id[0], n, pass*BVH_DIGIT_BITS + bit + 1);
	}
	WELD_LDS const uint32_t *keys = T.key[0], *ids = T.id[0];
	g.each([&](uint32_t tid, LodLane &) {
		for(uint32_t i = tid; i < n; i += BVH_THREADS) {
			const uint32_t d = bvh_digit(keys[i], pass);
			if(i == 0 || bvh_digit(keys[i - 1], pass) != d) T.first[d] = i;
		}
	});
	g.sync();
	g.each([&](uint32_t tid, LodLane &) {
		for(uint32_t i = tid; i < n; i += BVH_THREADS) {
			const uint32_t d = bvh_digit(keys[i], pass);
			const uint64_t at = (uint64_t)S.hist[(uint64_t)d*nt + k] + (i - T.first[d]);
			if(at < nface) { kb[at] = keys[i]; ib[at] = ids[i]; }             // (always: the table sums to nface)
		}
	});
}
// bvh_tree, workgroup k: a thread an internal node - its child words in the caller's nodes, its children's parent words -, and a word of order
template <class G> WELD_HD void bvh_tree_block(G &g, uint32_t nface, const BvhBig &S, WELD_MEM crthip_bvh_node *nodes, WELD_MEM uint32_t *parent,
	WELD_MEM uint32_t *order, uint32_t k) {
	g.each([&](uint32_t tid, LodLane &) {
		const uint64_t i = (uint64_t)k*BVH_BLOCK + tid;
		if(i >= nface) return;
		if(i + 1 < nface) {
			const BvhSplit s = bvh_split_of(BvhMemKeys{S.key[0]}, nface, (uint32_t)i);
			nodes[i].left = s.left; nodes[i].right = s.right;
			parent[s.left] = (uint32_t)i; parent[s.right] = (uint32_t)i;
		}
		if(i == 0) parent[0] = CRTHIP_NO_NODE;
		if(order) order[i] = S.id[0][i];
	});
}
// bvh_refit, workgroup k: a thread a leaf
template <class G> WELD_HD void bvh_refit_block(G &g, const WeldIn &J, const BvhBig &S, WELD_MEM crthip_bvh_node *nodes, WELD_MEM const uint32_t *parent,
	WELD_MEM crthip_bvh_counts *rec, uint32_t k) {
	g.each([&](uint32_t tid, LodLane &) {
		const uint64_t j = (uint64_t)k*BVH_BLOCK + tid;
		if(j >= J.nface) return;
		const uint32_t f = S.id[0][j];
		bvh_climb(BvhMemTree{parent, nodes, BvhMemWords{S.count}}, nodes, rec, J.nface, BvhMemWords{S.ext}.get(BVH_W_ABSENT), (uint32_t)j, f, bvh_face(J, f).b);
	});
}

// what crthip_batch_bind_bvh asks of a binding on a mesh of nface faces, behind "no such blob" and "a point cloud", in the header's order; null: fine
inline const char *bvh_binding_error(const crthip_bvh_binding *v, uint32_t nface) {
	if(!v->nodes || (uintptr_t)v->nodes % 16) return "bvh: nodes is NULL or not 16-byte aligned";
	if((uintptr_t)v->parent % 4 || (uintptr_t)v->order % 4 || (uintptr_t)v->counts % 16) return "bvh: parent or order is not 4-byte aligned, or counts is not 16-byte aligned";
	if((uint64_t)v->node_capacity < 2*(uint64_t)nface - 1) return "bvh: node_capacity is below 2*nface - 1";
	if(v->order && v->order_capacity < nface) return "bvh: order_capacity is below nface";
	if(v->flags || v->reserved) return "bvh: flags or reserved is not 0";
	return nullptr;
}

} // namespace corto_hip
