// enc_input_check.h — what the encoder reads from a mesh's arrays before it quantises (encoder.cpp: encode_check's index scan, setup's
// position step) restated as __host__ __device__ code, so that k_encode_check.hip runs it on arrays that live in device memory
// (crthip_encode_batch_resident) and the host can run the very same source in the kernels' partition (crthip_encode_input_model,
// which = 1; tests/test_encode_resident_cpu.py holds it against the host's own loops).
//
// Three things, each upstream's arithmetic in upstream's order:
//   index range    every entry against nvert; a violation is a bit in the mesh's record (integer OR: order cannot matter)
//   bounding box   the six floats the host's loop leaves, `if(v < mn) mn = v; if(v > mx) mx = v;` over the vertices in order from a seed
//                  (vertex 0: Encoder::addPositionsBits, src/encoder.cpp:49-63; +-FLT_MAX: a cloud's volume recipe, :83-91).  That loop keeps
//                  a NaN seed for ever, ignores every other NaN, and among values that compare equal (the two zeros) keeps the first.
//                  "Leftmost smallest" is associative, so the vertices are cut into runs and tiles: a partial starts from (+inf, -inf),
//                  which no value replaces and which replaces nothing, takes its vertices in order, and partials are merged earlier-into-
//                  later-never: merge(a, b) with a the earlier one keeps a's value unless b's is strictly smaller (larger).  The seed is
//                  the earliest of all.
//   edge sum       the mesh recipe (:105-110): float norms of every face's first edge added into a double IN FACE ORDER - the terms are
//                  made in parallel, the sum is one lane's.  sqrtf(s) is the host's (float)sqrt((double)s) (tests/cpp/sqrt_equiv.hip).
//                  A face whose first edge names a vertex >= nvert is never gathered through: its term is 0 and the record's bit is set.
// A crthip_mesh_layout changes where a value is read - a stride between vertices, uint16 index entries - and, for a cloud's box, subtracts the
// origin from each component first; partition, merge order and the in-order sum are untouched, so the argument above holds as it stands.
// The library is built with -ffp-contract=off: no product here is fused into a sum.
#pragma once
#include <float.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define EIN_HD __host__ __device__ inline
#else
#define EIN_HD inline
#endif

namespace corto_hip {

constexpr uint32_t EIN_THREADS = 256;
constexpr uint32_t EIN_RUN = 4;                           // vertices a lane takes in order: 12 floats, 48 bytes - as aligned as the array
constexpr uint32_t EIN_TILE = EIN_THREADS*EIN_RUN;        // vertices a workgroup folds into one partial box
constexpr uint32_t EIN_INDEX_TILE = 4096;                 // index entries a workgroup compares
constexpr uint32_t EIN_EDGE_TILE = 1024;                  // edge terms made at a time (in LDS) before lane 0 adds them
constexpr uint32_t EIN_FOLD_LANES = 64;                   // lanes that fold a mesh's partials: each a contiguous stretch, then lane order

// how setup derives the position step (encoder.cpp); nface: 0 for a point cloud
enum { EIN_STEP_GIVEN = 0, EIN_STEP_BOX_FIRST = 1, EIN_STEP_EDGE = 2, EIN_STEP_BOX_MAX = 3 };
EIN_HD uint32_t enc_in_recipe(int32_t position_bits, float position_q, uint32_t nvert, uint32_t nface) {
	if(position_bits > 0) return EIN_STEP_BOX_FIRST;
	if(position_q == 0.0f && nface) return EIN_STEP_EDGE;
	if(position_q == 0.0f && nvert) return EIN_STEP_BOX_MAX;
	return EIN_STEP_GIVEN;
}

struct EncInputBox { float mn[3], mx[3]; };
struct EncInputRecord {                                   // what comes back per item; zeroed before the pass
	uint32_t bad_index, pad0;                             // != 0: an index entry >= nvert
	double sum;                                           // EIN_STEP_EDGE: the first edges' lengths, added in face order
	EncInputBox box;                                      // EIN_STEP_BOX_*: the host loop's mn / mx
	uint32_t pad1[6];
};
static_assert(sizeof(EncInputRecord) == 64, "one record is 64 bytes");

enum { EIN_JOB_RANGE = 0, EIN_JOB_BOX = 1, EIN_JOB_EDGE = 2 };
struct EncInputJob {                                      // one kind of work on one item; its workgroups are counted from block_start
	const float *position;                                // vertex v's three floats at (bytes) position + v*pos_stride, 4-byte aligned
	const void *index;                                    // nface*3 uint32 (4-byte aligned), or uint16 (index16; 2-byte aligned) (RANGE, EDGE)
	EncInputBox *partials;                                // BOX: one per tile of EIN_TILE vertices
	EncInputRecord *rec;
	uint32_t nvert, nface, kind, recipe;
	// crthip_mesh_layout
	uint32_t pos_stride;                                  // bytes from one vertex to the next; 12: packed
	uint32_t index16;                                     // != 0: the index entries are uint16, widened as they are read
	uint32_t has_origin, pad;                             // != 0: the cloud's box runs on position - origin (src/encoder.cpp:80-88)
	float origin[4];
};
// how a job reads its arrays, for the kernels and for the host's walk of their partition alike
EIN_HD uint32_t enc_in_index(const EncInputJob &J, uint64_t i) {
	return J.index16 ? (uint32_t)((const uint16_t *)J.index)[i] : ((const uint32_t *)J.index)[i];
}
EIN_HD const float *enc_in_vertex(const EncInputJob &J, uint64_t v) { return (const float *)((const uint8_t *)J.position + v*J.pos_stride); }
// what the box loop sees of a vertex: the position, minus the origin where there is one (one float subtraction a component)
EIN_HD void enc_in_box_value(const EncInputJob &J, const float *p, float out[3]) {
	for(int k = 0; k < 3; k++) out[k] = J.has_origin ? p[k] - J.origin[k] : p[k];
}
// the range pass's cut of n entries: `head` entries up to the first 16-byte boundary, then groups of `per` (16 bytes), then the tail
EIN_HD void enc_in_range_cut(const EncInputJob &J, uint64_t n, uint32_t &per, uint64_t &head, uint64_t &groups, uint64_t &tail) {
	const uint32_t esize = J.index16 ? 2u : 4u;
	per = 16u/esize;
	const uint64_t to_boundary = ((16u - (uint32_t)((uintptr_t)J.index & 15u)) & 15u)/esize;
	head = to_boundary < n ? to_boundary : n;
	groups = (n - head)/per; tail = n - head - groups*per;
}

EIN_HD void enc_in_box_empty(EncInputBox &b) { for(int k = 0; k < 3; k++) { b.mn[k] = INFINITY; b.mx[k] = -INFINITY; } }
EIN_HD void enc_in_box_add(EncInputBox &b, const float *v) {                     // the host loop's body
	for(int k = 0; k < 3; k++) { if(v[k] < b.mn[k]) b.mn[k] = v[k]; if(v[k] > b.mx[k]) b.mx[k] = v[k]; }
}
EIN_HD void enc_in_box_merge(EncInputBox &a, const EncInputBox &later) {         // a: everything before `later`
	for(int k = 0; k < 3; k++) { if(later.mn[k] < a.mn[k]) a.mn[k] = later.mn[k]; if(later.mx[k] > a.mx[k]) a.mx[k] = later.mx[k]; }
}
// the host's seed: vertex 0 (nvert > 0) or +-FLT_MAX
EIN_HD void enc_in_box_seed(EncInputBox &b, uint32_t recipe, const float *position) {
	for(int k = 0; k < 3; k++) {
		b.mn[k] = recipe == EIN_STEP_BOX_FIRST ? position[k] : FLT_MAX;
		b.mx[k] = recipe == EIN_STEP_BOX_FIRST ? position[k] : -FLT_MAX;
	}
}
// a lane's run: `count` (<= EIN_RUN) vertices of v in order
EIN_HD void enc_in_box_run(EncInputBox &b, const float *v, uint32_t count) {
	enc_in_box_empty(b);
	for(uint32_t i = 0; i < EIN_RUN; i++) if(i < count) enc_in_box_add(b, v + 3*i);
}
// the stretch of `nparts` partials that fold lane `lane` takes, in order
EIN_HD void enc_in_fold_stretch(EncInputBox &b, const EncInputBox *parts, uint32_t nparts, uint32_t lane) {
	const uint32_t per = (nparts + EIN_FOLD_LANES - 1)/EIN_FOLD_LANES;
	enc_in_box_empty(b);
	for(uint32_t i = 0; i < per; i++) {
		const uint64_t p = (uint64_t)lane*per + i;
		if(p < nparts) enc_in_box_merge(b, parts[p]);
	}
}

// the length of face f's first edge, as Point3f::norm makes it (include/corto/point.h:111); never reads a vertex >= nvert
// (the raw positions: a mesh's recipe knows no origin, src/encoder.cpp:101-111)
EIN_HD float enc_in_edge_term(const EncInputJob &J, uint32_t f, uint32_t &bad) {
	const uint32_t ia = enc_in_index(J, (uint64_t)f*3), ib = enc_in_index(J, (uint64_t)f*3 + 1);
	if(ia >= J.nvert || ib >= J.nvert) { bad = 1; return 0.0f; }
	const float *a = enc_in_vertex(J, ia), *b = enc_in_vertex(J, ib);
	const float d[3] = {a[0] - b[0], a[1] - b[1], a[2] - b[2]};
	return sqrtf(d[0]*d[0] + d[1]*d[1] + d[2]*d[2]);
}

} // namespace corto_hip
