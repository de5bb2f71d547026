// bvh_cast.h — crthip_bvh_cast: exact segment casts against a blob's BVH (include/corto_hip.h has the contract).  The face test, the 128-bit
// comparison, the box test and the traversal loop with its bounds as __host__ __device__ code over the conventions of weld.h, so that the
// host runs the very same source as the kernel (crthip_bvh_cast_model, bvh_cast_host.cpp).
//
//   frame    everything is RELATIVE to the position's base: a vertex is its uint16 triple, an endpoint E - base (in range: 20 bits with the
//            sign), a node's box min - base and max - base in 64 bits (ANY bytes of a node stay below 2^33 there)
//   face     the contract's integers as they stand: n, D, K in 64 bits (below 2^55), U, V, W in 64 bits (below 2^63), D as d . n and never
//            as the sum of the three
//   order    t1 < t2 iff |K1|*|D2| < |K2|*|D1| on 128-bit products: cast_mul is __umul64hi on the device and unsigned __int128 on the host,
//            the one helper behind which the two differ; no __int128 in device code
//   box      exact and closed, separating axes on DOUBLED coordinates: c2 = min + max, h = max - min, m = P + Q - c2, and the segment's
//            doubled half-vector is d.  Reject if |m[i]| > |d[i]| + h[i] on an axis, or |m[j]d[k] - m[k]d[j]| > h[j]|d[k]| + h[k]|d[j]| on
//            a cross axis.  The empty box of a subtree of absent faces has h < 0 and fails the first test.  Below 2^56 whatever the bytes
//   prune    against the best hit so far, num/den: a box whose slab on some axis is entered at te = e/|d[i]| > num/den (e*den > num*|d[i]|
//            on 128-bit products, e > 0 the distance from P to the slab's near side) holds only points behind the best hit.  STRICTLY
//            greater, so a face of equal t and a lower id is still met; exact and conservative, so the answer - a minimum over a total
//            order - does not depend on it.  Not under CRTHIP_CAST_ANY.  Never a float.
//   walk     a stack of node ids, the root first; a node taken from it is loaded (two 16-byte loads), its box tested, a leaf's face tested,
//            an internal node's children pushed right first, so that the left one is taken next.  The bounds: a child id >= 2F - 1, a leaf's
//            face >= F, a push beyond CAST_STACK entries, more than 2F - 1 nodes taken - each ends the thread with CRTHIP_CAST_TREE before
//            the id is used as an address.  The children go on the stack in the nodes' own order: visiting the nearer child first is the
//            refinement that was not built (it needs both children's boxes in hand before either is taken)
//   stack    S.get(k) / S.put(k, x): entry k of this thread's stack.  The kernel keeps [65][64] words in LDS, depth-major: lane l's entry k
//            is word 64k + l, so the 64 lanes of any access fall on 64 consecutive words - no two on one bank - and the stack is never in
//            scratch memory.  The BVH contract bounds the height at 64: 65 entries suffice for every tree crthip_batch_bind_bvh writes.
//            CHOSEN, NOT TUNED: one thread a segment, one wave a workgroup (16 640 bytes of LDS: nine workgroups a CU by LDS); nobody has
//            varied either (profiles/bvh_cast.md says what was measured).  A stackless walk over the optional `parent` array is the named
//            alternative and is not built
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/corto_hip.h"
#include "weld.h"

namespace corto_hip {

constexpr uint32_t CAST_THREADS = 64;                       // one wave a workgroup, a thread a segment
constexpr uint32_t CAST_STACK = 65;                         // entries a thread: the BVH contract's height bound + 1
constexpr uint32_t CAST_LDS_WORDS = CAST_STACK*CAST_THREADS;
constexpr int64_t CAST_RANGE = 1 << 19;                     // an endpoint's components relative to the base: [-2^19, 2^19)
constexpr uint32_t CAST_FLAGS = CRTHIP_CAST_ANY | CRTHIP_CAST_FRONT;

// a set as the kernel reads it: the job table's record (bvh_cast.cpp fills it, 16-byte multiples)
struct CastJob {
	const crthip_bvh_node *nodes; const void *position; const void *index; const crthip_quant_transform *transform;
	const crthip_segment *segments; crthip_cast_hit *hits;
	int32_t base[3]; uint32_t pos_stride;                   // (pos_stride: resolved, never 0)
	uint32_t nvert, nface, index_u16, nseg;
	uint32_t flags, pad[3];
};
static_assert(sizeof(CastJob) == 96, "the job table's record");

// what a thread walks: the arrays with their address space, the base in 64 bits
struct CastIn {
	WELD_MEM const uint8_t *nodes, *position; WELD_MEM const void *index;
	int64_t base[3];
	uint32_t stride, nvert, nface, index_u16, flags;
};

// 16 bytes at once: a node's half, a segment's half, a hit record's half (the pointers are 16-byte aligned by the call's checks)
struct alignas(16) __attribute__((may_alias)) CastQuad { uint32_t x, y, z, w; };
WELD_HD CastQuad cast_load(WELD_MEM const void *p) { return *(WELD_MEM const CastQuad *)p; }
WELD_HD void cast_store(WELD_MEM void *p, const CastQuad &q) { *(WELD_MEM CastQuad *)p = q; }

struct CastVec { int64_t x, y, z; };
WELD_HD int64_t cast_dot(const CastVec &a, const CastVec &b) { return a.x*b.x + a.y*b.y + a.z*b.z; }
WELD_HD CastVec cast_cross(const CastVec &a, const CastVec &b) { return CastVec{a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z, a.x*b.y - a.y*b.x}; }
WELD_HD CastVec cast_sub(const CastVec &a, const CastVec &b) { return CastVec{a.x - b.x, a.y - b.y, a.z - b.z}; }
WELD_HD uint64_t cast_abs(int64_t x) { return x < 0 ? 0ull - (uint64_t)x : (uint64_t)x; }

// ---- the 128-bit comparison ------------------------------------------------------------------------------------------------------------------

struct CastWide { uint64_t hi, lo; };
WELD_HD CastWide cast_mul(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
	return CastWide{__umul64hi(a, b), a*b};
#else
	const unsigned __int128 p = (unsigned __int128)a*b;
	return CastWide{(uint64_t)(p >> 64), (uint64_t)p};
#endif
}
WELD_HD bool cast_less(const CastWide &a, const CastWide &b) { return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo); }
// a/b < c/d for positive b, d
WELD_HD bool cast_ratio_less(uint64_t a, uint64_t b, uint64_t c, uint64_t d) { return cast_less(cast_mul(a, d), cast_mul(c, b)); }

// ---- the face test ---------------------------------------------------------------------------------------------------------------------------

WELD_HD uint32_t cast_corner(const CastIn &J, uint64_t k) {
	return J.index_u16 ? (uint32_t)((WELD_MEM const uint16_t *)J.index)[k] : ((WELD_MEM const uint32_t *)J.index)[k];
}
// vertex v (< nvert) relative to the base: its three halfwords
WELD_HD CastVec cast_vertex(const CastIn &J, uint32_t v) {
	WELD_MEM const uint16_t *p = (WELD_MEM const uint16_t *)(J.position + (uint64_t)v*J.stride);
	return CastVec{(int64_t)p[0], (int64_t)p[1], (int64_t)p[2]};
}
struct CastFace { uint32_t hit, side; uint64_t num, den; };
// P: the segment's start relative to the base, d = Q - P
WELD_HD CastFace cast_face(const CastIn &J, uint32_t f, const CastVec &P, const CastVec &d) {
	CastFace r{0u, 0u, 0ull, 0ull};
	const uint32_t ia = cast_corner(J, (uint64_t)f*3), ib = cast_corner(J, (uint64_t)f*3 + 1), ic = cast_corner(J, (uint64_t)f*3 + 2);
	if(ia >= J.nvert || ib >= J.nvert || ic >= J.nvert) return r;         // absent: compared, never an address
	const CastVec A = cast_sub(cast_vertex(J, ia), P), B = cast_sub(cast_vertex(J, ib), P), C = cast_sub(cast_vertex(J, ic), P);
	const CastVec n = cast_cross(cast_sub(B, A), cast_sub(C, A));
	const int64_t D = cast_dot(d, n);
	if(D == 0) return r;                                                  // degenerate (n = 0) or in the face's plane
	if((J.flags & CRTHIP_CAST_FRONT) && D > 0) return r;
	const int64_t K = cast_dot(A, n);
	if(K != 0 && ((K < 0) != (D < 0))) return r;                          // t < 0
	if(cast_abs(K) > cast_abs(D)) return r;                               // t > 1
	const int64_t U = cast_dot(d, cast_cross(B, C)), V = cast_dot(d, cast_cross(C, A)), W = cast_dot(d, cast_cross(A, B));
	if(!((U >= 0 && V >= 0 && W >= 0) || (U <= 0 && V <= 0 && W <= 0))) return r;
	r.hit = 1u; r.side = D < 0 ? 1u : 0u; r.num = cast_abs(K); r.den = cast_abs(D);
	return r;
}

// ---- the box test ----------------------------------------------------------------------------------------------------------------------------

// q0, q1: a node's halves; S = P + Q; best: the hit to prune against (den == 0: none)
WELD_HD bool cast_box(const CastIn &J, const CastQuad &q0, const CastQuad &q1, const CastVec &P, const CastVec &S, const CastVec &d, uint64_t num, uint64_t den) {
	const int64_t lx = (int64_t)(int32_t)q0.x - J.base[0], ly = (int64_t)(int32_t)q0.y - J.base[1], lz = (int64_t)(int32_t)q0.z - J.base[2];
	const int64_t hx = (int64_t)(int32_t)q1.x - J.base[0], hy = (int64_t)(int32_t)q1.y - J.base[1], hz = (int64_t)(int32_t)q1.z - J.base[2];
	const CastVec h{hx - lx, hy - ly, hz - lz}, m{S.x - (lx + hx), S.y - (ly + hy), S.z - (lz + hz)};
	const int64_t ax = (int64_t)cast_abs(d.x), ay = (int64_t)cast_abs(d.y), az = (int64_t)cast_abs(d.z);
	if((int64_t)cast_abs(m.x) > ax + h.x || (int64_t)cast_abs(m.y) > ay + h.y || (int64_t)cast_abs(m.z) > az + h.z) return false;
	if((int64_t)cast_abs(m.y*d.z - m.z*d.y) > h.y*az + h.z*ay) return false;
	if((int64_t)cast_abs(m.z*d.x - m.x*d.z) > h.z*ax + h.x*az) return false;
	if((int64_t)cast_abs(m.x*d.y - m.y*d.x) > h.x*ay + h.y*ax) return false;
	if(den) {
		// e: from P to the slab's near side along the segment's direction on that axis; positive where the slab lies ahead
		const int64_t ex = d.x > 0 ? lx - P.x : P.x - hx, ey = d.y > 0 ? ly - P.y : P.y - hy, ez = d.z > 0 ? lz - P.z : P.z - hz;
		if(d.x != 0 && ex > 0 && cast_ratio_less(num, den, (uint64_t)ex, (uint64_t)ax)) return false;
		if(d.y != 0 && ey > 0 && cast_ratio_less(num, den, (uint64_t)ey, (uint64_t)ay)) return false;
		if(d.z != 0 && ez > 0 && cast_ratio_less(num, den, (uint64_t)ez, (uint64_t)az)) return false;
	}
	return true;
}

// ---- the walk --------------------------------------------------------------------------------------------------------------------------------

struct CastStack {                                          // a thread's stack inside the workgroup's block: depth-major
	WELD_LDS uint32_t *s; uint32_t lane;
	WELD_HD uint32_t get(uint32_t k) const { return s[k*CAST_THREADS + lane]; }
	WELD_HD void put(uint32_t k, uint32_t x) const { s[k*CAST_THREADS + lane] = x; }
};
struct CastNoCount { WELD_HD void node() const {} WELD_HD void face() const {} };

struct CastResult { uint32_t status, face, side; uint64_t num, den; };
WELD_HD CastResult cast_none(uint32_t status) { return CastResult{status, CRTHIP_NO_FACE, 0u, 0ull, 0ull}; }

// the segment P -> P + d, in range, against the set's faces through its tree
template <class C> WELD_HD CastResult cast_walk(const CastIn &J, const CastStack &S, const CastVec &P, const CastVec &d, C &count) {
	const uint32_t nn = 2u*J.nface - 1u;                                  // (nface <= 2^31 - 1: the call's check)
	const bool any = (J.flags & CRTHIP_CAST_ANY) != 0;
	const CastVec PQ{P.x + P.x + d.x, P.y + P.y + d.y, P.z + P.z + d.z};
	CastResult best = cast_none(CRTHIP_CAST_MISS);
	uint32_t depth = 1, taken = 0;
	S.put(0, 0u);
	while(depth) {                                                        // at most nn + 1 rounds: every round takes a node
		const uint32_t id = S.get(--depth);
		if(++taken > nn) return cast_none(CRTHIP_CAST_TREE);
		count.node();
		WELD_MEM const uint8_t *node = J.nodes + (uint64_t)id*32;         // id < nn: the root, or checked when it was pushed
		const CastQuad q0 = cast_load(node), q1 = cast_load(node + 16);
		if(!cast_box(J, q0, q1, P, PQ, d, best.num, any ? 0ull : best.den)) continue;
		if(q1.w == CRTHIP_BVH_LEAF) {
			const uint32_t f = q0.w;
			if(f >= J.nface) return cast_none(CRTHIP_CAST_TREE);
			count.face();
			const CastFace h = cast_face(J, f, P, d);
			if(!h.hit) continue;
			if(any) return cast_none(CRTHIP_CAST_HIT);
			bool better = best.status != CRTHIP_CAST_HIT;
			if(!better) {
				const CastWide a = cast_mul(h.num, best.den), b = cast_mul(best.num, h.den);
				better = cast_less(a, b) || (!cast_less(b, a) && f < best.face);
			}
			if(better) best = CastResult{CRTHIP_CAST_HIT, f, h.side, h.num, h.den};
			continue;
		}
		if(q0.w >= nn || q1.w >= nn) return cast_none(CRTHIP_CAST_TREE);
		if(depth + 2 > CAST_STACK) return cast_none(CRTHIP_CAST_TREE);
		S.put(depth++, q1.w); S.put(depth++, q0.w);
	}
	return best;
}

// segment i of a set: the frame, the range, the walk, the record.  tr: the set's transform record (or null: J.base is the caller's)
template <class C> WELD_HD void cast_segment(CastIn J, WELD_MEM const uint8_t *tr, WELD_MEM const uint8_t *segments, WELD_MEM uint8_t *hits, const CastStack &S,
	uint32_t i, C &count) {
	bool written = true;
	if(tr) {
		const CastQuad b = cast_load(tr), w = cast_load(tr + 32);         // base[4]; q, components, written, reserved
		J.base[0] = (int64_t)(int32_t)b.x; J.base[1] = (int64_t)(int32_t)b.y; J.base[2] = (int64_t)(int32_t)b.z;
		written = w.z != 0u;
	}
	const CastQuad s0 = cast_load(segments + (uint64_t)i*32), s1 = cast_load(segments + (uint64_t)i*32 + 16);
	const CastVec P{(int64_t)(int32_t)s0.x - J.base[0], (int64_t)(int32_t)s0.y - J.base[1], (int64_t)(int32_t)s0.z - J.base[2]};
	const CastVec Q{(int64_t)(int32_t)s1.x - J.base[0], (int64_t)(int32_t)s1.y - J.base[1], (int64_t)(int32_t)s1.z - J.base[2]};
	auto in = [](int64_t x) { return x >= -CAST_RANGE && x < CAST_RANGE; };
	CastResult r;
	if(!written || !(in(P.x) && in(P.y) && in(P.z) && in(Q.x) && in(Q.y) && in(Q.z))) r = cast_none(CRTHIP_CAST_RANGE);
	else r = cast_walk(J, S, P, cast_sub(Q, P), count);
	WELD_MEM uint8_t *out = hits + (uint64_t)i*32;
	cast_store(out, CastQuad{r.status, r.face, r.side, 0u});
	cast_store(out + 16, CastQuad{(uint32_t)r.num, (uint32_t)(r.num >> 32), (uint32_t)r.den, (uint32_t)(r.den >> 32)});
}

// a set's own checks, in the contract's order (bvh_cast_host.cpp).  The message names the field; null: fine
const char *bvh_cast_set_error(const crthip_bvh_cast_set *s);
inline uint32_t bvh_cast_stride(const crthip_bvh_cast_set *s) { return s->pos_stride ? s->pos_stride : 6u; }
inline uint64_t bvh_cast_position_bytes(const crthip_bvh_cast_set *s) { return s->nvert ? (uint64_t)(s->nvert - 1)*bvh_cast_stride(s) + 6 : 0; }

} // namespace corto_hip
