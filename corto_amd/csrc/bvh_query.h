// bvh_query.h — crthip_bvh_query: exact box queries against a blob's BVH (include/corto_hip.h has the contract).  The three face rules, the node
// test and the traversal loop with its bounds as __host__ __device__ code over bvh_cast.h's parts - the 16-byte loads and stores, the vectors,
// the LDS stack, the vertex and corner loads -, so that the host runs the very same source as the kernel (crthip_bvh_query_model,
// bvh_query_host.cpp).
//
//   frame    bvh_cast.h's: everything is RELATIVE to the position's base.  A vertex is its uint16 triple, a box corner E - base (in range: 20
//            bits with the sign), a node's box min - base and max - base in 64 bits
//   doubled  c2 = lo + hi and h = hi - lo of the query box (|c2| < 2^20, 0 <= h < 2^20), a corner V = 2p - c2 (|V| < 2^21), an edge the
//            difference of two corners (|e| < 2^18): the box is |x| <= h around the origin, and no half appears
//   face     query_face: the box axes first (min V[c] > h[c] or max V[c] < -h[c]: no match) - under CRTHIP_QUERY_BOXES that is the whole rule,
//            under CRTHIP_QUERY_INSIDE all six of min V[c] >= -h[c], max V[c] <= h[c] are -; then the face's plane, n = e0 x e1 (|n| < 2^36),
//            |n . V0| > sum h|n| (below 2^59); then the nine axes u_k x e_i (below 2^41).  For the axis u_k x e_i the two ends of edge i
//            project to the SAME value (their difference is (u_k x e_i) . e_i = 0, exactly), so two projections an axis stand for the three:
//            the edge's start and the corner opposite.  A zero axis (equal corners, an edge along u_k) separates nothing: 0 > 0 is false.
//            Signed 64 bits throughout, no 128-bit product
//   node     query_node: the closed overlap of the node's box with the query box, three comparisons a side.  The empty box of a subtree of
//            absent faces (min = INT32_MAX, max = INT32_MIN) overlaps nothing in range
//   walk     cast_walk's loop and its four bounds, without an early end: every matching face is counted, and the first `cap` of them go to
//            out[0..] in the order they are met - left first, which is ascending rank on crthip_batch_bind_bvh's nodes.  A bound that trips
//            ends the thread with CRTHIP_QUERY_TREE before the id is used as an address
//   stack    bvh_cast.h's CastStack: [65][64] words of LDS, depth-major.  CHOSEN, NOT TUNED, like one thread a box and one wave a workgroup
#pragma once
#include "bvh_cast.h"

namespace corto_hip {

constexpr uint32_t QUERY_FLAGS = CRTHIP_QUERY_COUNT | CRTHIP_QUERY_BOXES | CRTHIP_QUERY_INSIDE;

// a set as the kernel reads it: the job table's record (bvh_query.cpp fills it, 16-byte multiples)
struct QueryJob {
	const crthip_bvh_node *nodes; const void *position; const void *index; const crthip_quant_transform *transform;
	const crthip_box *boxes; crthip_query_result *results; uint32_t *faces; uint64_t pad0;
	int32_t base[3]; uint32_t pos_stride;                   // (pos_stride: resolved, never 0)
	uint32_t nvert, nface, index_u16, nbox;
	uint32_t face_capacity, flags, pad[2];                  // (face_capacity: resolved, 0 under CRTHIP_QUERY_COUNT)
};
static_assert(sizeof(QueryJob) == 112, "the job table's record");

// the query box relative to the base, doubled: |x[c]| <= h[c] around c2/2; lo, hi for the node test
struct QueryBox { int64_t lo[3], hi[3]; CastVec c2, h; };

// ---- the face rules --------------------------------------------------------------------------------------------------------------------------

WELD_HD int64_t query_min3(int64_t a, int64_t b, int64_t c) { const int64_t m = a < b ? a : b; return m < c ? m : c; }
WELD_HD int64_t query_max3(int64_t a, int64_t b, int64_t c) { const int64_t m = a > b ? a : b; return m > c ? m : c; }
WELD_HD int64_t query_iabs(int64_t x) { return x < 0 ? -x : x; }

// the three axes u_k x e for edge e, A the edge's start and O the corner opposite: true if one of them separates
WELD_HD bool query_edge_separates(const CastVec &e, const CastVec &A, const CastVec &O, const CastVec &h) {
	const int64_t ax = query_iabs(e.x), ay = query_iabs(e.y), az = query_iabs(e.z);
	int64_t a, o, r;
	a = e.y*A.z - e.z*A.y; o = e.y*O.z - e.z*O.y; r = h.y*az + h.z*ay;      // u_x x e = (0, -e.z, e.y)
	if((a < o ? a : o) > r || (a > o ? a : o) < -r) return true;
	a = e.z*A.x - e.x*A.z; o = e.z*O.x - e.x*O.z; r = h.x*az + h.z*ax;      // u_y x e = (e.z, 0, -e.x)
	if((a < o ? a : o) > r || (a > o ? a : o) < -r) return true;
	a = e.x*A.y - e.y*A.x; o = e.x*O.y - e.y*O.x; r = h.x*ay + h.y*ax;      // u_z x e = (-e.y, e.x, 0)
	if((a < o ? a : o) > r || (a > o ? a : o) < -r) return true;
	return false;
}

// the doubled corners V0, V1, V2 of a present face against the box |x| <= h, under the set's flags
WELD_HD bool query_rule(const CastVec &V0, const CastVec &V1, const CastVec &V2, const CastVec &h, uint32_t flags) {
	const int64_t nx = query_min3(V0.x, V1.x, V2.x), ny = query_min3(V0.y, V1.y, V2.y), nz = query_min3(V0.z, V1.z, V2.z);
	const int64_t xx = query_max3(V0.x, V1.x, V2.x), xy = query_max3(V0.y, V1.y, V2.y), xz = query_max3(V0.z, V1.z, V2.z);
	if(nx > h.x || xx < -h.x || ny > h.y || xy < -h.y || nz > h.z || xz < -h.z) return false;
	if(flags & CRTHIP_QUERY_BOXES) return true;
	if(flags & CRTHIP_QUERY_INSIDE) return nx >= -h.x && xx <= h.x && ny >= -h.y && xy <= h.y && nz >= -h.z && xz <= h.z;
	const CastVec e0 = cast_sub(V1, V0), e1 = cast_sub(V2, V1), e2 = cast_sub(V0, V2);
	const CastVec n = cast_cross(e0, e1);
	if(query_iabs(cast_dot(n, V0)) > h.x*query_iabs(n.x) + h.y*query_iabs(n.y) + h.z*query_iabs(n.z)) return false;
	if(query_edge_separates(e0, V0, V2, h)) return false;
	if(query_edge_separates(e1, V1, V0, h)) return false;
	if(query_edge_separates(e2, V2, V1, h)) return false;
	return true;
}

// face f (< nface) of the set against the box
WELD_HD bool query_face(const CastIn &J, uint32_t f, const QueryBox &B) {
	const uint32_t ia = cast_corner(J, (uint64_t)f*3), ib = cast_corner(J, (uint64_t)f*3 + 1), ic = cast_corner(J, (uint64_t)f*3 + 2);
	if(ia >= J.nvert || ib >= J.nvert || ic >= J.nvert) return false;        // absent: compared, never an address
	const CastVec a = cast_vertex(J, ia), b = cast_vertex(J, ib), c = cast_vertex(J, ic);
	const CastVec V0{a.x + a.x - B.c2.x, a.y + a.y - B.c2.y, a.z + a.z - B.c2.z};
	const CastVec V1{b.x + b.x - B.c2.x, b.y + b.y - B.c2.y, b.z + b.z - B.c2.z};
	const CastVec V2{c.x + c.x - B.c2.x, c.y + c.y - B.c2.y, c.z + c.z - B.c2.z};
	return query_rule(V0, V1, V2, B.h, J.flags);
}

// ---- the node test ---------------------------------------------------------------------------------------------------------------------------

// q0, q1: a node's halves
WELD_HD bool query_node(const CastIn &J, const CastQuad &q0, const CastQuad &q1, const QueryBox &B) {
	const int64_t lx = (int64_t)(int32_t)q0.x - J.base[0], ly = (int64_t)(int32_t)q0.y - J.base[1], lz = (int64_t)(int32_t)q0.z - J.base[2];
	const int64_t hx = (int64_t)(int32_t)q1.x - J.base[0], hy = (int64_t)(int32_t)q1.y - J.base[1], hz = (int64_t)(int32_t)q1.z - J.base[2];
	return lx <= B.hi[0] && hx >= B.lo[0] && ly <= B.hi[1] && hy >= B.lo[1] && lz <= B.hi[2] && hz >= B.lo[2];
}

// ---- the walk --------------------------------------------------------------------------------------------------------------------------------

struct QueryNoCount { WELD_HD void node() const {} WELD_HD void face() const {} };

struct QueryResult { uint32_t status, count, written; };
WELD_HD QueryResult query_none(uint32_t status) { return QueryResult{status, 0u, 0u}; }

// the box B, in range and not empty, against the set's faces through its tree; out: the box's slice of cap words (cap 0: never touched)
template <class C> WELD_HD QueryResult query_walk(const CastIn &J, const CastStack &S, const QueryBox &B, WELD_MEM uint32_t *out, uint32_t cap, C &count) {
	const uint32_t nn = 2u*J.nface - 1u;                                  // (nface <= 2^31 - 1: the call's check)
	uint32_t depth = 1, taken = 0, found = 0;                             // (found <= nface: a leaf a node taken, nn of them at most)
	S.put(0, 0u);
	while(depth) {                                                        // at most nn + 1 rounds: every round takes a node
		const uint32_t id = S.get(--depth);
		if(++taken > nn) return query_none(CRTHIP_QUERY_TREE);
		count.node();
		WELD_MEM const uint8_t *node = J.nodes + (uint64_t)id*32;         // id < nn: the root, or checked when it was pushed
		const CastQuad q0 = cast_load(node), q1 = cast_load(node + 16);
		if(!query_node(J, q0, q1, B)) continue;
		if(q1.w == CRTHIP_BVH_LEAF) {
			const uint32_t f = q0.w;
			if(f >= J.nface) return query_none(CRTHIP_QUERY_TREE);
			count.face();
			if(!query_face(J, f, B)) continue;
			if(found < cap) out[found] = f;
			found++;
			continue;
		}
		if(q0.w >= nn || q1.w >= nn) return query_none(CRTHIP_QUERY_TREE);
		if(depth + 2 > CAST_STACK) return query_none(CRTHIP_QUERY_TREE);
		S.put(depth++, q1.w); S.put(depth++, q0.w);
	}
	return QueryResult{0u, found, found < cap ? found : cap};
}

// box i of a set: the frame, the range, the walk, the record.  tr: the set's transform record (or null: J.base is the caller's); cap: the
// set's face_capacity, 0 under CRTHIP_QUERY_COUNT
template <class C> WELD_HD void query_box(CastIn J, WELD_MEM const uint8_t *tr, WELD_MEM const uint8_t *boxes, WELD_MEM uint8_t *results, WELD_MEM uint32_t *faces,
	uint32_t cap, const CastStack &S, uint32_t i, C &count) {
	bool written = true;
	if(tr) {
		const CastQuad b = cast_load(tr), w = cast_load(tr + 32);         // base[4]; q, components, written, reserved
		J.base[0] = (int64_t)(int32_t)b.x; J.base[1] = (int64_t)(int32_t)b.y; J.base[2] = (int64_t)(int32_t)b.z;
		written = w.z != 0u;
	}
	const CastQuad s0 = cast_load(boxes + (uint64_t)i*32), s1 = cast_load(boxes + (uint64_t)i*32 + 16);
	QueryBox B;
	B.lo[0] = (int64_t)(int32_t)s0.x - J.base[0]; B.lo[1] = (int64_t)(int32_t)s0.y - J.base[1]; B.lo[2] = (int64_t)(int32_t)s0.z - J.base[2];
	B.hi[0] = (int64_t)(int32_t)s1.x - J.base[0]; B.hi[1] = (int64_t)(int32_t)s1.y - J.base[1]; B.hi[2] = (int64_t)(int32_t)s1.z - J.base[2];
	auto in = [](int64_t x) { return x >= -CAST_RANGE && x < CAST_RANGE; };
	QueryResult r;
	if(!written || !(in(B.lo[0]) && in(B.lo[1]) && in(B.lo[2]) && in(B.hi[0]) && in(B.hi[1]) && in(B.hi[2]))) r = query_none(CRTHIP_QUERY_RANGE);
	else if(B.lo[0] > B.hi[0] || B.lo[1] > B.hi[1] || B.lo[2] > B.hi[2]) r = query_none(CRTHIP_QUERY_OK);
	else {
		B.c2 = CastVec{B.lo[0] + B.hi[0], B.lo[1] + B.hi[1], B.lo[2] + B.hi[2]};
		B.h = CastVec{B.hi[0] - B.lo[0], B.hi[1] - B.lo[1], B.hi[2] - B.lo[2]};
		r = query_walk(J, S, B, cap ? faces + (uint64_t)i*cap : faces, cap, count);   // (cap 0: faces may be null, and is never an address)
		if(r.status == CRTHIP_QUERY_OK && !(J.flags & CRTHIP_QUERY_COUNT) && r.written < r.count) r.status = CRTHIP_QUERY_CLIPPED;
	}
	cast_store(results + (uint64_t)i*16, CastQuad{r.status, r.count, r.written, 0u});
}

// a set's own checks, in the contract's order (bvh_query_host.cpp).  The message names the field; null: fine
const char *bvh_query_set_error(const crthip_bvh_query_set *s);
inline uint32_t bvh_query_stride(const crthip_bvh_query_set *s) { return s->pos_stride ? s->pos_stride : 6u; }
inline uint64_t bvh_query_position_bytes(const crthip_bvh_query_set *s) { return s->nvert ? (uint64_t)(s->nvert - 1)*bvh_query_stride(s) + 6 : 0; }
inline uint32_t bvh_query_capacity(const crthip_bvh_query_set *s) { return (s->flags & CRTHIP_QUERY_COUNT) ? 0u : s->face_capacity; }

} // namespace corto_hip
