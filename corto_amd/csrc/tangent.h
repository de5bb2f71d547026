// tangent.h — crthip_batch_bind_computed_tangents: a vertex's tangent frame from the blob's delta-decoded INTEGER positions and uvs, the decoded
// index and the vertex's final normal (include/corto_hip.h has the contract).  The arithmetic and the partition of k_tangent.hip as
// __host__ __device__ code, so that the host runs the very same source in the kernels' partition (crthip_tangent_model, tangent_host.cpp).
//
//   face    e1 = p[b]-p[a], e2 = p[c]-p[a], (s1,r1) = t[b]-t[a], (s2,r2) = t[c]-t[a] widened to 64 bits; det = s1*r2 - s2*r1;
//           Tf = sg*(e1*r2 - e2*r1), Bf = sg*(e2*s1 - e1*s2) with sg = sign(det), added to the accumulators of a, b and c.  Everything is
//           two's-complement arithmetic modulo 2^64 (done on uint64_t: no signed overflow), so the sums are associative and commutative:
//           no order of faces, lanes, waves or blocks can change a bit of them, and an atomic add needs no ordered gather behind it.
//   vertex  k = max(0, bitlength(max |x| over T[v], B[v]) - 24); x -> sign(x)*(|x| >> k), exact as a float; Gram-Schmidt against the normal
//           in a form that is invariant to the normal's scale; w from dot(cross(n, u), B); (1, 0, 0, +1) where the length is not a finite
//           value above zero.  Every float operation is rounded on its own (-ffp-contract=off on both sides).
// The one-workgroup kernel holds ONE accumulator of 3 x int64 a vertex: it sums T, keeps sign(x)*(|x| >> kT) with kT from T alone in
// registers (tan_blob_keep_T), sums B in the same words, and shifts T the rest of the way (tan_rescale): (|x| >> kT) >> (k - kT) = |x| >> k.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define TAN_HD __host__ __device__ inline
#else
#define TAN_HD inline
#endif
// k_tangent.hip defines TAN_KERNELS: its pointers into device memory carry their address space, so that loads and stores are global_* and not
// flat_* (a FLAT access counts against the LDS counter too: kernels_common.h); everywhere else, and in the host pass, the qualifier is empty
#if defined(TAN_KERNELS) && defined(__HIP_DEVICE_COMPILE__)
#define TAN_MEM __attribute__((address_space(1)))
#else
#define TAN_MEM
#endif

namespace corto_hip {

constexpr uint32_t TAN_THREADS = 256;
constexpr uint32_t TAN_BLOCK = 1024;                       // faces (tangent_faces) or vertices (tangent_vertex) a workgroup of the batch-wide kernels takes
constexpr uint32_t TAN_BLOB_SLOTS = 9;                     // vertices a lane of the one-workgroup kernel finishes: TANGENT_BLOB_MAX/TAN_THREADS (batch_internal.h)
constexpr uint32_t TAN_ACC_WORDS = 6;                      // the batch-wide kernels' scratch a vertex: T | B, 3 x int64 each

// what every pass knows of a blob
struct TanIn {
	TAN_MEM const int32_t *position, *uv;                  // nvert x 3, nvert x 2: delta-decoded integers, packed
	TAN_MEM const void *faces; uint32_t faces_u16, nvert, nface;
	TAN_MEM const void *normal; uint32_t normal_i16, normal_stride; // the vertex's final normal where its binding put it: 3 f32 or 3 i16, stride in bytes
	TAN_MEM void *out; uint32_t out_i16, out_stride;       // 4 f32 or 4 i16 a vertex, stride in bytes
};
// faces a lane takes a round: their indices, then their coordinates, are loaded together.  A lane of a TAN_BLOCK block has four faces; the
// one-workgroup kernel's lanes have some 17 of a 2 112-vertex blob, and eight a round measured no faster than four (profiles/computed_tangents.md)
constexpr uint32_t TAN_ROUND = 4;

TAN_HD void tan_load_face(const TanIn &J, uint32_t f, uint32_t &a, uint32_t &b, uint32_t &c) {
	if(J.faces_u16) { TAN_MEM const uint16_t *p = (TAN_MEM const uint16_t *)J.faces + (size_t)f*3; a = p[0]; b = p[1]; c = p[2]; }
	else { TAN_MEM const uint32_t *p = (TAN_MEM const uint32_t *)J.faces + (size_t)f*3; a = p[0]; b = p[1]; c = p[2]; }
}
TAN_HD uint64_t tan_wide(int32_t x, int32_t y) { return (uint64_t)((int64_t)x - (int64_t)y); }   // the widened difference, as a residue modulo 2^64

// the face's term for T (which 0) or B (which 1); false: det == 0, the face adds nothing.  a, b, c < nvert
TAN_HD bool tan_face_term(const TanIn &J, uint32_t a, uint32_t b, uint32_t c, uint32_t which, uint64_t out[3]) {
	TAN_MEM const int32_t *ta = J.uv + (size_t)a*2, *tb = J.uv + (size_t)b*2, *tc = J.uv + (size_t)c*2;
	const uint64_t s1 = tan_wide(tb[0], ta[0]), r1 = tan_wide(tb[1], ta[1]), s2 = tan_wide(tc[0], ta[0]), r2 = tan_wide(tc[1], ta[1]);
	const uint64_t det = s1*r2 - s2*r1;
	const bool neg = (int64_t)det < 0;
	TAN_MEM const int32_t *pa = J.position + (size_t)a*3, *pb = J.position + (size_t)b*3, *pc = J.position + (size_t)c*3;
	// T: e1*r2 - e2*r1;  B: e2*s1 - e1*s2 = e1*(-s2) - e2*(-s1)
	const uint64_t m1 = which ? 0 - s2 : r2, m2 = which ? 0 - s1 : r1;
	for(int i = 0; i < 3; i++) {
		const uint64_t x = tan_wide(pb[i], pa[i])*m1 - tan_wide(pc[i], pa[i])*m2;
		out[i] = neg ? 0 - x : x;
	}
	return det != 0;
}

// One lane's faces f0 + lane, f0 + lane + TAN_THREADS, ... below f1: the term `which` into add(vertex, component, value) of the three
// corners.  A face that names a vertex twice adds twice; one with an index beyond nvert adds nothing.  TAN_ROUND faces a round:
// every index of a round is loaded before the first coordinate, every coordinate before the first add (a face at a time, a round was two
// dependent trips to memory); a slot past f1 or with a bad index reads vertex 0 and adds nothing.  f0 < f1 <= nface, nvert >= 1
template <class Add> TAN_HD void tan_faces_lane(const TanIn &J, uint32_t which, uint32_t f0, uint32_t f1, uint32_t lane, Add add) {
	for(uint32_t f = f0 + lane; f < f1; f += TAN_ROUND*TAN_THREADS) {
		uint32_t A[TAN_ROUND], B[TAN_ROUND], C[TAN_ROUND];
		bool ok[TAN_ROUND];
		uint64_t x[TAN_ROUND][3];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
		for(uint32_t u = 0; u < TAN_ROUND; u++) {
			const uint32_t fu = f + u*TAN_THREADS;
			const bool in = fu < f1 && fu >= f;                              // (>= f: the sum did not wrap)
			tan_load_face(J, in ? fu : f, A[u], B[u], C[u]);
			ok[u] = in;
		}
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
		for(uint32_t u = 0; u < TAN_ROUND; u++) {
			ok[u] = ok[u] && A[u] < J.nvert && B[u] < J.nvert && C[u] < J.nvert;
			const bool term = tan_face_term(J, ok[u] ? A[u] : 0u, ok[u] ? B[u] : 0u, ok[u] ? C[u] : 0u, which, x[u]);
			ok[u] = ok[u] && term;
		}
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
		for(uint32_t u = 0; u < TAN_ROUND; u++)
			if(ok[u]) for(uint32_t i = 0; i < 3; i++) { add(A[u], i, x[u][i]); add(B[u], i, x[u][i]); add(C[u], i, x[u][i]); }
	}
}

TAN_HD uint64_t tan_abs(uint64_t x) { return (int64_t)x < 0 ? 0 - x : x; }                       // |INT64_MIN| = 2^63 fits
TAN_HD uint32_t tan_bitlen(uint64_t m) { uint32_t n = 0; while(m) { n++; m >>= 1; } return n; }
TAN_HD uint32_t tan_shift_of(uint64_t max_abs) { const uint32_t n = tan_bitlen(max_abs); return n > 24 ? n - 24 : 0u; }
TAN_HD uint64_t tan_max_abs3(const uint64_t x[3]) {
	const uint64_t a = tan_abs(x[0]), b = tan_abs(x[1]), c = tan_abs(x[2]);
	const uint64_t m = a > b ? a : b;
	return m > c ? m : c;
}
// sign(x)*(|x| >> k), truncated toward zero; below 2^24 in magnitude where k covers x
TAN_HD int32_t tan_scaled(uint64_t x, uint32_t k) { const int32_t m = (int32_t)(tan_abs(x) >> k); return (int64_t)x < 0 ? -m : m; }
// ... of a value that was scaled by some k' <= k already: d = k - k' more bits
TAN_HD int32_t tan_rescale(int32_t s, uint32_t d) {
	if(d >= 31) return 0;
	const int32_t m = (s < 0 ? -s : s) >> d;
	return s < 0 ? -m : m;
}

TAN_HD void tan_load_normal(const TanIn &J, uint32_t v, float n[3]) {
	TAN_MEM const uint8_t *p = (TAN_MEM const uint8_t *)J.normal + (size_t)v*J.normal_stride;
	if(J.normal_i16) { TAN_MEM const int16_t *q = (TAN_MEM const int16_t *)p; n[0] = (float)q[0]; n[1] = (float)q[1]; n[2] = (float)q[2]; }
	else { TAN_MEM const float *q = (TAN_MEM const float *)p; n[0] = q[0]; n[1] = q[1]; n[2] = q[2]; }
}

// float -> int16 by the rule of the INT16 normals: truncation; out of int32's range or NaN gives INT32_MIN, whose low half is 0
TAN_HD int16_t tan_f2s(float x) {
	const int32_t i = !(x > -2147483904.0f && x < 2147483648.0f) ? (int32_t)0x80000000 : (int32_t)x;
	return (int16_t)(uint16_t)(uint32_t)i;
}

// the vertex's value from its scaled sums and its normal, stored: exactly the vertex's own 16 or 8 bytes
TAN_HD void tan_finish(const TanIn &J, uint32_t v, const int32_t Ti[3], const int32_t Bi[3]) {
	float n[3];
	tan_load_normal(J, v, n);
	const float Tx = (float)Ti[0], Ty = (float)Ti[1], Tz = (float)Ti[2], Bx = (float)Bi[0], By = (float)Bi[1], Bz = (float)Bi[2];
	const float nx = n[0], ny = n[1], nz = n[2];
	float nn = nx*nx + ny*ny; nn = nn + nz*nz;
	float nt = nx*Tx + ny*Ty; nt = nt + nz*Tz;
	const float ux = Tx*nn - nx*nt, uy = Ty*nn - ny*nt, uz = Tz*nn - nz*nt;
	float l2 = ux*ux + uy*uy; l2 = l2 + uz*uz;
	const float len = sqrtf(l2);
	const float cx = ny*uz - nz*uy, cy = nz*ux - nx*uz, cz = nx*uy - ny*ux;
	float h = cx*Bx + cy*By; h = h + cz*Bz;
	const bool minus = h < 0;
	const bool ok = len > 0 && len < INFINITY;              // (a NaN fails both)
	TAN_MEM uint8_t *o = (TAN_MEM uint8_t *)J.out + (size_t)v*J.out_stride;
	if(J.out_i16) {
		TAN_MEM int16_t *q = (TAN_MEM int16_t *)o;
		if(ok) { const float l = 32767.0f/len; q[0] = tan_f2s(ux*l); q[1] = tan_f2s(uy*l); q[2] = tan_f2s(uz*l); q[3] = minus ? -32767 : 32767; }
		else { q[0] = 32767; q[1] = 0; q[2] = 0; q[3] = 32767; }
	} else {
		TAN_MEM float *q = (TAN_MEM float *)o;
		if(ok) { q[0] = ux/len; q[1] = uy/len; q[2] = uz/len; q[3] = minus ? -1.0f : 1.0f; }
		else { q[0] = 1.0f; q[1] = 0.0f; q[2] = 0.0f; q[3] = 1.0f; }
	}
}

// a vertex of the batch-wide pass: its six sums in scratch
TAN_HD void tan_vertex(const TanIn &J, uint32_t v, TAN_MEM const uint64_t *acc) {
	const uint64_t T[3] = {acc[(size_t)v*TAN_ACC_WORDS], acc[(size_t)v*TAN_ACC_WORDS + 1], acc[(size_t)v*TAN_ACC_WORDS + 2]};
	const uint64_t B[3] = {acc[(size_t)v*TAN_ACC_WORDS + 3], acc[(size_t)v*TAN_ACC_WORDS + 4], acc[(size_t)v*TAN_ACC_WORDS + 5]};
	const uint64_t mt = tan_max_abs3(T), mb = tan_max_abs3(B);
	const uint32_t k = tan_shift_of(mt > mb ? mt : mb);
	const int32_t Ti[3] = {tan_scaled(T[0], k), tan_scaled(T[1], k), tan_scaled(T[2], k)};
	const int32_t Bi[3] = {tan_scaled(B[0], k), tan_scaled(B[1], k), tan_scaled(B[2], k)};
	tan_finish(J, v, Ti, Bi);
}

// ---- the one-workgroup partition: lane `lane` owns the vertices lane, lane + TAN_THREADS, ... (up to TAN_BLOB_SLOTS of them) ----
struct TanLaneState { int32_t T[TAN_BLOB_SLOTS][3]; uint32_t kT[TAN_BLOB_SLOTS]; };

// after the T pass: T leaves the accumulator scaled by what T alone asks for, and the words are zero again for B
template <class Acc> TAN_HD void tan_blob_keep_T(const TanIn &J, Acc *acc, uint32_t lane, TanLaneState &S) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
	for(uint32_t s = 0; s < TAN_BLOB_SLOTS; s++) {
		const uint32_t v = lane + s*TAN_THREADS;
		if(v >= J.nvert) continue;
		const uint64_t T[3] = {acc[3*v], acc[3*v + 1], acc[3*v + 2]};
		const uint32_t k = tan_shift_of(tan_max_abs3(T));
		S.kT[s] = k; S.T[s][0] = tan_scaled(T[0], k); S.T[s][1] = tan_scaled(T[1], k); S.T[s][2] = tan_scaled(T[2], k);
		acc[3*v] = 0; acc[3*v + 1] = 0; acc[3*v + 2] = 0;
	}
}
// after the B pass: the shift of all six, T the rest of its way, the value
template <class Acc> TAN_HD void tan_blob_finish(const TanIn &J, const Acc *acc, uint32_t lane, const TanLaneState &S) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
	for(uint32_t s = 0; s < TAN_BLOB_SLOTS; s++) {
		const uint32_t v = lane + s*TAN_THREADS;
		if(v >= J.nvert) continue;
		const uint64_t B[3] = {acc[3*v], acc[3*v + 1], acc[3*v + 2]};
		const uint32_t kB = tan_shift_of(tan_max_abs3(B)), k = kB > S.kT[s] ? kB : S.kT[s];
		const int32_t Ti[3] = {tan_rescale(S.T[s][0], k - S.kT[s]), tan_rescale(S.T[s][1], k - S.kT[s]), tan_rescale(S.T[s][2], k - S.kT[s])};
		const int32_t Bi[3] = {tan_scaled(B[0], k), tan_scaled(B[1], k), tan_scaled(B[2], k)};
		tan_finish(J, v, Ti, Bi);
	}
}

} // namespace corto_hip
