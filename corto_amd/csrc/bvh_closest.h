// bvh_closest.h — crthip_bvh_closest: exact closest-face queries against a blob's BVH (include/corto_hip.h has the contract).  The wide
// arithmetic, the face rule, the node prune and the traversal loop with its bounds as __host__ __device__ code over bvh_cast.h's parts - the
// 16-byte loads and stores, the vectors, the LDS stack, the vertex and corner loads, cast_mul -, so that the host runs the very same source
// as the kernel (crthip_bvh_closest_model, bvh_closest_host.cpp).
//
//   frame    bvh_cast.h's: everything is RELATIVE to the position's base.  A vertex is its uint16 triple, the point P - base (in range: 20 bits
//            with the sign), a corner relative to the point A = a - P (|A[c]| < 2^20), an edge the difference of two corners (|e[c]| < 2^16),
//            a node's box min - base and max - base in 64 bits (ANY bytes of a node stay below 2^33 there)
//   widths   a corner's |A|^2 below 2^42.  An edge: |e|^2 below 2^34 (the edge's den), s = -A . e below 2^38, A x e below 2^38 a component,
//            |A x e|^2 below 2^76 (the edge's num).  The interior: n = e0 x e1 below 2^33 a component, |n|^2 below 2^68 (den), n . A below
//            2^55, (n . A)^2 below 2^110 (num); a side test (A_i x e_i) . n has terms below 2^71 and a sum below 2^72: a signed 128-bit sum
//            of three 64x64 products, of which only the sign is used.  num1*den2 against num2*den1 is below 2^178: 256-bit products
//   wide     Closest128 {lo, hi} is the unsigned 128-bit value, closest_mul a 64x64 product in it, closest_mul256 the 128x128 product from
//            four cast_mul, closest_less256 its comparison, closest_dot_nonneg the sign of the signed sum.  No __int128 in device code: the
//            device and the host differ only behind cast_mul.  Plain C++, CHOSEN, NOT TUNED: every comparison of two distances goes through
//            the 256-bit product, also where both sides would fit 128 bits
//   face     closest_face: the contract's seven candidates in the order 0 to 6, each taken only if STRICTLY less than the best of this face
//            so far - the corners {|A_k|^2, 1}; the edges {|A_i x e_i|^2, |e_i|^2} where |e_i|^2 > 0 and 0 <= -A_i . e_i <= |e_i|^2; the
//            interior {(n . A)^2, |n|^2} where |n|^2 > 0 and all three (A_i x e_i) . n >= 0.  A face with a corner >= nvert is absent
//   prune    closest_gap2: per axis g = max(lo - P, P - hi, 0) clamped at 2^21, D2 = sum g^2 below 2^44, the squared distance from P to the
//            node's box or less.  A node is skipped iff D2*den > num of the best so far (closest_beyond: a 64x128-bit product) - STRICTLY,
//            so that a face of equal distance and a lower id is still met.  Exact and conservative: the answer, a minimum over the total
//            order (num/den, face), does not depend on it.  Under CRTHIP_CLOSEST_WITHIN the best starts as r^2/1 with face CRTHIP_NO_FACE:
//            the same strict prune, and a face AT r^2 still wins by its lower id, which is what keeps the radius inclusive.  The clamp
//            cannot turn a skip into a miss: every best is below 2^42.  The empty box of a subtree of absent faces has a gap of 2^21 on
//            every axis and is skipped as soon as there is a best; before that its leaves are met and are absent
//   walk     cast_walk's loop and its four bounds.  NEARER CHILD FIRST (order 0, the kernel's): an internal node taken from the stack has
//            both children's boxes loaded - their ids are compared first -, a child beyond the best is not pushed at all, and of two that
//            are the farther goes on the stack first; at equal gaps the left one is taken first.  Order 1 pushes the children in the
//            nodes' own order, right first, as the cast does; the host hook keeps it to count against (profiles/bvh_closest.md has both
//            counts: on the benchmark's blobs nearer-first takes a fraction of the nodes).  No byte of a record depends on the order
//   stack    bvh_cast.h's CastStack: [65][64] words of LDS, depth-major.  CHOSEN, NOT TUNED, like one thread a point and one wave a workgroup
#pragma once
#include "bvh_cast.h"

namespace corto_hip {

constexpr uint32_t CLOSEST_FLAGS = CRTHIP_CLOSEST_WITHIN | CRTHIP_CLOSEST_ANY;
constexpr int64_t CLOSEST_CLAMP = 1 << 21;                  // a gap an axis, and the radius: every present face is closer to an in-range point

// a set as the kernel reads it: the job table's record (bvh_closest.cpp fills it, 16-byte multiples)
struct ClosestJob {
	const crthip_bvh_node *nodes; const void *position; const void *index; const crthip_quant_transform *transform;
	const crthip_point *points; crthip_closest_hit *hits;
	int32_t base[3]; uint32_t pos_stride;                   // (pos_stride: resolved, never 0)
	uint32_t nvert, nface, index_u16, npoint;
	uint32_t flags, pad[3];
};
static_assert(sizeof(ClosestJob) == 96, "the job table's record");
static_assert(sizeof(crthip_point) == 16 && sizeof(crthip_closest_hit) == 48, "the records are read and written in 16-byte units");

// ---- the wide arithmetic ---------------------------------------------------------------------------------------------------------------------

struct Closest128 { uint64_t lo, hi; };                     // unsigned, or two's complement where it says so
struct Closest256 { uint64_t w[4]; };                       // least word first

WELD_HD Closest128 closest_wide(uint64_t x) { return Closest128{x, 0ull}; }
WELD_HD Closest128 closest_mul(uint64_t a, uint64_t b) { const CastWide p = cast_mul(a, b); return Closest128{p.lo, p.hi}; }
WELD_HD Closest128 closest_add(const Closest128 &a, const Closest128 &b) {
	const uint64_t lo = a.lo + b.lo;
	return Closest128{lo, a.hi + b.hi + (lo < a.lo ? 1ull : 0ull)};
}
WELD_HD Closest128 closest_neg(const Closest128 &a) { const uint64_t lo = 0ull - a.lo; return Closest128{lo, ~a.hi + (lo == 0ull ? 1ull : 0ull)}; }
WELD_HD Closest128 closest_square(int64_t x) { const uint64_t a = cast_abs(x); return closest_mul(a, a); }
// |v|^2 of a vector whose components are below 2^63 in magnitude and whose sum of squares fits 128 bits
WELD_HD Closest128 closest_norm2(const CastVec &v) { return closest_add(closest_add(closest_square(v.x), closest_square(v.y)), closest_square(v.z)); }

// a*b in 256 bits: four cast_mul, the carries by comparison
WELD_HD Closest256 closest_mul256(const Closest128 &a, const Closest128 &b) {
	const CastWide ll = cast_mul(a.lo, b.lo), lh = cast_mul(a.lo, b.hi), hl = cast_mul(a.hi, b.lo), hh = cast_mul(a.hi, b.hi);
	Closest256 r;
	r.w[0] = ll.lo;
	uint64_t carry = 0, s = ll.hi + lh.lo;
	carry += s < lh.lo ? 1u : 0u;
	s += hl.lo; carry += s < hl.lo ? 1u : 0u;
	r.w[1] = s;
	uint64_t carry2 = 0, t = lh.hi + carry;
	carry2 += t < carry ? 1u : 0u;
	t += hl.hi; carry2 += t < hl.hi ? 1u : 0u;
	t += hh.lo; carry2 += t < hh.lo ? 1u : 0u;
	r.w[2] = t;
	r.w[3] = hh.hi + carry2;                                              // (the product of two 128-bit values fits: no carry out)
	return r;
}
WELD_HD bool closest_less256(const Closest256 &a, const Closest256 &b) {
	if(a.w[3] != b.w[3]) return a.w[3] < b.w[3];
	if(a.w[2] != b.w[2]) return a.w[2] < b.w[2];
	if(a.w[1] != b.w[1]) return a.w[1] < b.w[1];
	return a.w[0] < b.w[0];
}
// n1/d1 < n2/d2 for positive d1, d2
WELD_HD bool closest_ratio_less(const Closest128 &n1, const Closest128 &d1, const Closest128 &n2, const Closest128 &d2) {
	return closest_less256(closest_mul256(n1, d2), closest_mul256(n2, d1));
}
// a . b >= 0, the sum in signed 128 bits (every term below 2^126 in magnitude)
WELD_HD bool closest_dot_nonneg(const CastVec &a, const CastVec &b) {
	auto term = [](int64_t x, int64_t y) {
		const Closest128 p = closest_mul(cast_abs(x), cast_abs(y));
		return ((x < 0) != (y < 0)) ? closest_neg(p) : p;
	};
	const Closest128 s = closest_add(closest_add(term(a.x, b.x), term(a.y, b.y)), term(a.z, b.z));
	return (s.hi >> 63) == 0ull;
}
// D2*den > num: a 64x128-bit product in three words
WELD_HD bool closest_beyond(uint64_t D2, const Closest128 &num, const Closest128 &den) {
	const CastWide p0 = cast_mul(D2, den.lo), p1 = cast_mul(D2, den.hi);
	const uint64_t w1 = p0.hi + p1.lo, w2 = p1.hi + (w1 < p0.hi ? 1ull : 0ull);
	if(w2) return true;
	return w1 > num.hi || (w1 == num.hi && p0.lo > num.lo);
}

// ---- the face rule ---------------------------------------------------------------------------------------------------------------------------

struct ClosestFace { uint32_t present, feature; Closest128 num, den; };

// edge i of a face: A its start relative to the point, e the edge, c = A x e
WELD_HD void closest_edge(ClosestFace &r, const CastVec &A, const CastVec &e, const CastVec &c, uint32_t code) {
	const int64_t ee = cast_dot(e, e), s = -cast_dot(A, e);
	if(ee <= 0 || s < 0 || s > ee) return;
	const Closest128 num = closest_norm2(c), den = closest_wide((uint64_t)ee);
	if(closest_ratio_less(num, den, r.num, r.den)) { r.feature = code; r.num = num; r.den = den; }
}

// face f (< nface) of the set against the point P (relative to the base)
WELD_HD ClosestFace closest_face(const CastIn &J, uint32_t f, const CastVec &P) {
	ClosestFace r{0u, 0u, Closest128{0ull, 0ull}, Closest128{0ull, 0ull}};
	const uint32_t ia = cast_corner(J, (uint64_t)f*3), ib = cast_corner(J, (uint64_t)f*3 + 1), ic = cast_corner(J, (uint64_t)f*3 + 2);
	if(ia >= J.nvert || ib >= J.nvert || ic >= J.nvert) return r;         // absent: compared, never an address
	const CastVec A = cast_sub(cast_vertex(J, ia), P), B = cast_sub(cast_vertex(J, ib), P), C = cast_sub(cast_vertex(J, ic), P);
	const uint64_t da = (uint64_t)cast_dot(A, A), db = (uint64_t)cast_dot(B, B), dc = (uint64_t)cast_dot(C, C);
	uint64_t d = da;
	r.present = 1u;
	if(db < d) { d = db; r.feature = 1u; }
	if(dc < d) { d = dc; r.feature = 2u; }
	r.num = closest_wide(d); r.den = closest_wide(1ull);
	const CastVec e0 = cast_sub(B, A), e1 = cast_sub(C, B), e2 = cast_sub(A, C);
	const CastVec c0 = cast_cross(A, e0), c1 = cast_cross(B, e1), c2 = cast_cross(C, e2);
	closest_edge(r, A, e0, c0, 3u);
	closest_edge(r, B, e1, c1, 4u);
	closest_edge(r, C, e2, c2, 5u);
	const CastVec n = cast_cross(e0, e1);
	if(n.x == 0 && n.y == 0 && n.z == 0) return r;                        // degenerate: the segment or the point that it is
	if(!closest_dot_nonneg(c0, n) || !closest_dot_nonneg(c1, n) || !closest_dot_nonneg(c2, n)) return r;
	const Closest128 num = closest_square(cast_dot(n, A)), den = closest_norm2(n);
	if(closest_ratio_less(num, den, r.num, r.den)) { r.feature = 6u; r.num = num; r.den = den; }
	return r;
}

// ---- the node prune --------------------------------------------------------------------------------------------------------------------------

// q0, q1: a node's halves.  The squared distance from P to the node's box, every axis clamped at 2^21: below 2^44 whatever the bytes
WELD_HD uint64_t closest_gap2(const CastIn &J, const CastQuad &q0, const CastQuad &q1, const CastVec &P) {
	auto gap = [](int64_t lo, int64_t hi, int64_t p) {
		int64_t g = lo - p > p - hi ? lo - p : p - hi;
		g = g < 0 ? 0 : g;
		return g > CLOSEST_CLAMP ? CLOSEST_CLAMP : g;
	};
	const int64_t gx = gap((int64_t)(int32_t)q0.x - J.base[0], (int64_t)(int32_t)q1.x - J.base[0], P.x);
	const int64_t gy = gap((int64_t)(int32_t)q0.y - J.base[1], (int64_t)(int32_t)q1.y - J.base[1], P.y);
	const int64_t gz = gap((int64_t)(int32_t)q0.z - J.base[2], (int64_t)(int32_t)q1.z - J.base[2], P.z);
	return (uint64_t)(gx*gx + gy*gy + gz*gz);
}

// ---- the walk --------------------------------------------------------------------------------------------------------------------------------

struct ClosestNoCount { WELD_HD void node() const {} WELD_HD void face() const {} };

struct ClosestResult { uint32_t status, face, feature; Closest128 num, den; };
WELD_HD ClosestResult closest_none(uint32_t status) { return ClosestResult{status, CRTHIP_NO_FACE, 0u, Closest128{0ull, 0ull}, Closest128{0ull, 0ull}}; }

// the point P, in range, against the set's faces through its tree.  NEAR: the nearer child first (the kernel's), else the nodes' own order
template <bool NEAR, class C> WELD_HD ClosestResult closest_walk(const CastIn &J, const CastStack &S, const CastVec &P, uint32_t radius, C &count) {
	const uint32_t nn = 2u*J.nface - 1u;                                  // (nface <= 2^31 - 1: the call's check)
	const bool any = (J.flags & CRTHIP_CLOSEST_ANY) != 0;
	ClosestResult best = closest_none(CRTHIP_CLOSEST_MISS);
	bool bounded = (J.flags & CRTHIP_CLOSEST_WITHIN) != 0;                // there is a best to compare and to prune against
	if(bounded) {
		const uint64_t r = radius < (uint64_t)CLOSEST_CLAMP ? radius : (uint64_t)CLOSEST_CLAMP;
		best.num = closest_wide(r*r); best.den = closest_wide(1ull);      // (face CRTHIP_NO_FACE: a face at r^2 has the lower id)
	}
	uint32_t depth = 1, taken = 0;
	S.put(0, 0u);
	while(depth) {                                                        // at most nn + 1 rounds: every round takes a node
		const uint32_t id = S.get(--depth);
		if(++taken > nn) return closest_none(CRTHIP_CLOSEST_TREE);
		count.node();
		WELD_MEM const uint8_t *node = J.nodes + (uint64_t)id*32;         // id < nn: the root, or checked when it was pushed
		const CastQuad q0 = cast_load(node), q1 = cast_load(node + 16);
		if(bounded && closest_beyond(closest_gap2(J, q0, q1, P), best.num, best.den)) continue;
		if(q1.w == CRTHIP_BVH_LEAF) {
			const uint32_t f = q0.w;
			if(f >= J.nface) return closest_none(CRTHIP_CLOSEST_TREE);
			count.face();
			const ClosestFace h = closest_face(J, f, P);
			if(!h.present) continue;
			if(bounded && !closest_ratio_less(h.num, h.den, best.num, best.den) && (closest_ratio_less(best.num, best.den, h.num, h.den) || f >= best.face)) continue;
			if(any) return closest_none(CRTHIP_CLOSEST_HIT);
			best = ClosestResult{CRTHIP_CLOSEST_HIT, f, h.feature, h.num, h.den};
			bounded = true;
			continue;
		}
		if(q0.w >= nn || q1.w >= nn) return closest_none(CRTHIP_CLOSEST_TREE);
		if(depth + 2 > CAST_STACK) return closest_none(CRTHIP_CLOSEST_TREE);
		if(NEAR) {
			WELD_MEM const uint8_t *l = J.nodes + (uint64_t)q0.w*32, *r = J.nodes + (uint64_t)q1.w*32;
			const uint64_t gl = closest_gap2(J, cast_load(l), cast_load(l + 16), P), gr = closest_gap2(J, cast_load(r), cast_load(r + 16), P);
			const bool tl = !(bounded && closest_beyond(gl, best.num, best.den)), tr = !(bounded && closest_beyond(gr, best.num, best.den));
			if(gr < gl) { if(tl) S.put(depth++, q0.w); if(tr) S.put(depth++, q1.w); }
			else { if(tr) S.put(depth++, q1.w); if(tl) S.put(depth++, q0.w); }
		} else {
			S.put(depth++, q1.w); S.put(depth++, q0.w);
		}
	}
	return best.status == CRTHIP_CLOSEST_HIT ? best : closest_none(CRTHIP_CLOSEST_MISS);
}

// point i of a set: the frame, the range, the walk, the record.  tr: the set's transform record (or null: J.base is the caller's)
template <bool NEAR, class C> WELD_HD void closest_point(CastIn J, WELD_MEM const uint8_t *tr, WELD_MEM const uint8_t *points, WELD_MEM uint8_t *hits, const CastStack &S,
	uint32_t i, C &count) {
	bool written = true;
	if(tr) {
		const CastQuad b = cast_load(tr), w = cast_load(tr + 32);         // base[4]; q, components, written, reserved
		J.base[0] = (int64_t)(int32_t)b.x; J.base[1] = (int64_t)(int32_t)b.y; J.base[2] = (int64_t)(int32_t)b.z;
		written = w.z != 0u;
	}
	const CastQuad s = cast_load(points + (uint64_t)i*16);
	const CastVec P{(int64_t)(int32_t)s.x - J.base[0], (int64_t)(int32_t)s.y - J.base[1], (int64_t)(int32_t)s.z - J.base[2]};
	auto in = [](int64_t x) { return x >= -CAST_RANGE && x < CAST_RANGE; };
	ClosestResult r;
	if(!written || !(in(P.x) && in(P.y) && in(P.z))) r = closest_none(CRTHIP_CLOSEST_RANGE);
	else r = closest_walk<NEAR>(J, S, P, s.w, count);
	WELD_MEM uint8_t *out = hits + (uint64_t)i*48;
	cast_store(out, CastQuad{r.status, r.face, r.feature, 0u});
	cast_store(out + 16, CastQuad{(uint32_t)r.num.lo, (uint32_t)(r.num.lo >> 32), (uint32_t)r.num.hi, (uint32_t)(r.num.hi >> 32)});
	cast_store(out + 32, CastQuad{(uint32_t)r.den.lo, (uint32_t)(r.den.lo >> 32), (uint32_t)r.den.hi, (uint32_t)(r.den.hi >> 32)});
}

// a set's own checks, in the contract's order (bvh_closest_host.cpp).  The message names the field; null: fine
const char *bvh_closest_set_error(const crthip_bvh_closest_set *s);
inline uint32_t bvh_closest_stride(const crthip_bvh_closest_set *s) { return s->pos_stride ? s->pos_stride : 6u; }
inline uint64_t bvh_closest_position_bytes(const crthip_bvh_closest_set *s) { return s->nvert ? (uint64_t)(s->nvert - 1)*bvh_closest_stride(s) + 6 : 0; }

} // namespace corto_hip
