// k_normal.hip — normal reconstruction for gfx950.
//   DIFF      : octahedral ints -> unit vectors                    src/normal_attribute.cpp:257-279, include/corto/normal_attribute.h:104-122
//   ESTIMATED / BORDER (NormalAttr::postDelta, src/normal_attribute.cpp:210-255):
//     estimateNormals :40-59   per-face float cross products of the INTEGER positions, accumulated per vertex
//                              in face order (float addition order is part of the result)
//     markBoundary    :24-37   XOR of neighbour ids (order-free -> atomicXor)
//     computeNormals  :281-325 toOcta(est) + diff[slot] -> toSphere, or est/|est|
//   COMPUTED (prediction 3, crthip_batch_bind_computed_normals): no stored attribute at all - every vertex takes computeNormals'
//     no-correction branch (:294-302, :320-323), and a vertex whose estimate is zero gets (0,0,1)
//
// Ordered accumulation without a serial pass over faces: build a CSR of incident faces per vertex with
// atomics (arbitrary order), then each vertex walks its own short list in ascending face id.  All float
// code is compiled with -ffp-contract=off: an FMA changes the reference's bits.
#include "kernels_common.h"
#include "kernels.h"

namespace corto_hip {

// include/corto/point.h:111 — (float)sqrt((double)((x*x + y*y) + z*z)).  The f32 square root gives the same bits for every float: a double's 53-bit
// root rounded to 24 bits IS the correctly rounded single root (53 >= 2*24 + 2: the double rounding is innocuous), and the device's sqrtf is correctly
// rounded - tests/cpp/sqrt_equiv.hip compares the two over all 2^31 non-negative patterns (test_device_sqrtf_is_the_reference_norm_for_every_float).
// 17 f32 issue slots instead of 34 with f64 arithmetic at half rate, once per vertex.
__device__ __forceinline__ float norm3(float x, float y, float z) {
	float s = x*x + y*y;
	s = s + z*z;
	return sqrtf(s);
}

// include/corto/normal_attribute.h:75-85
__device__ __forceinline__ void to_octa(float vx, float vy, float vz, int32_t unit, int32_t &ox, int32_t &oy) {
	float s = fabsf(vx) + fabsf(vy);
	s = s + fabsf(vz);
	float px = vx/s, py = vy/s;
	if(vz < 0) {
		const float qx = 1.0f - fabsf(py), qy = 1.0f - fabsf(px);
		px = qx; py = qy;
		if(vx < 0) px = -px;
		if(vy < 0) py = -py;
	}
	ox = f2i_x86(px*(float)unit);
	oy = f2i_x86(py*(float)unit);
}

// include/corto/normal_attribute.h:104-112 (x, y already narrowed to the caller's integer type)
__device__ __forceinline__ void to_sphere(int32_t x, int32_t y, int32_t unit, float &nx, float &ny, float &nz) {
	const uint32_t ax = x < 0 ? 0u - (uint32_t)x : (uint32_t)x, ay = y < 0 ? 0u - (uint32_t)y : (uint32_t)y;
	const int32_t z = (int32_t)((uint32_t)unit - ax - ay);
	nx = (float)x; ny = (float)y; nz = (float)z;
	if(nz < 0) {
		nx = (float)(int32_t)((x > 0 ? 1u : 0xFFFFFFFFu)*((uint32_t)unit - ay));
		ny = (float)(int32_t)((y > 0 ? 1u : 0xFFFFFFFFu)*((uint32_t)unit - ax));
	}
	const float l = norm3(nx, ny, nz);
	nx /= l; ny /= l; nz /= l;
}

__device__ __forceinline__ void store_normal(const NormalJob &J, uint32_t i, float nx, float ny, float nz) {
	if(J.out_i16) {                                     // Point3s(n*32767) (normal_attribute.h:121)
		CRT_GLOBAL int16_t *o = (CRT_GLOBAL int16_t *)(as_global((uint8_t *)J.out) + (size_t)i*J.out_stride);     // explicit address space: a FLAT store would make the next LDS read wait for its acknowledgement
		o[0] = f2s_x86(nx*32767); o[1] = f2s_x86(ny*32767); o[2] = f2s_x86(nz*32767);
	} else {
		CRT_GLOBAL float *o = (CRT_GLOBAL float *)(as_global((uint8_t *)J.out) + (size_t)i*J.out_stride);
		o[0] = nx; o[1] = ny; o[2] = nz;
	}
}

__device__ __forceinline__ void load_face(const NormalJob &J, uint32_t f, uint32_t &a, uint32_t &b, uint32_t &c) {
	if(J.faces_u16) { const uint16_t *p = (const uint16_t *)J.faces + (size_t)f*3; a = p[0]; b = p[1]; c = p[2]; }
	else { const uint32_t *p = (const uint32_t *)J.faces + (size_t)f*3; a = p[0]; b = p[1]; c = p[2]; }
}

// ---- DIFF: dequantize (normal_attribute.cpp:257-279). block -> job; thread = vertex ----
__global__ __launch_bounds__(256) void k_normal_diff(const NormalJob *__restrict__ jobs, const uint32_t *__restrict__ block_job,
                                                     const uint32_t *__restrict__ block_first, uint32_t nblocks) {
	if(blockIdx.x >= nblocks) return;
	const NormalJob J = jobs[block_job[blockIdx.x]];
	if(J.prediction != 0) return;
	const uint32_t i = (blockIdx.x - block_first[block_job[blockIdx.x]])*256 + threadIdx.x;
	if(i >= J.nvert) return;
	int32_t x = J.diffs[2*(size_t)i], y = J.diffs[2*(size_t)i + 1];
	if(J.out_i16) { x = (int16_t)(uint16_t)(uint32_t)x; y = (int16_t)(uint16_t)(uint32_t)y; }   // Point2s(diffs...) :269
	float nx, ny, nz;
	to_sphere(x, y, J.unit, nx, ny, nz);
	store_normal(J, i, nx, ny, nz);
}

// ---- ESTIMATED/BORDER step 1: per face: cross product, incidence counts, boundary XOR ----
__global__ __launch_bounds__(256) void k_normal_faces(const NormalJob *__restrict__ jobs, const uint32_t *__restrict__ block_job,
                                                      const uint32_t *__restrict__ block_first, uint32_t nblocks,
                                                      float *__restrict__ facen, uint32_t *__restrict__ cnt, uint32_t *__restrict__ bnd) {
	if(blockIdx.x >= nblocks) return;
	const NormalJob J = jobs[block_job[blockIdx.x]];
	const uint32_t f = (blockIdx.x - block_first[block_job[blockIdx.x]])*256 + threadIdx.x;
	if(f >= J.nface) return;
	uint32_t a, b, c;
	load_face(J, f, a, b, c);
	float *n = facen + ((size_t)J.fbase + f)*3;
	if(a >= J.nvert || b >= J.nvert || c >= J.nvert) { n[0] = n[1] = n[2] = 0.f; *J.status = -5; return; }
	const int32_t *p0 = J.position + (size_t)a*3, *p1 = J.position + (size_t)b*3, *p2 = J.position + (size_t)c*3;
	const float x0 = (float)p0[0], y0 = (float)p0[1], z0 = (float)p0[2];
	const float ax = (float)p1[0] - x0, ay = (float)p1[1] - y0, az = (float)p1[2] - z0;
	const float bx = (float)p2[0] - x0, by = (float)p2[1] - y0, bz = (float)p2[2] - z0;
	n[0] = ay*bz - az*by;                               // point.h:113-115
	n[1] = az*bx - ax*bz;
	n[2] = ax*by - ay*bx;
	atomicAdd(&cnt[J.vbase + a], 1u); atomicAdd(&cnt[J.vbase + b], 1u); atomicAdd(&cnt[J.vbase + c], 1u);
	if(J.prediction == 2) {                             // markBoundary
		atomicXor(&bnd[J.vbase + a], b ^ c); atomicXor(&bnd[J.vbase + b], c ^ a); atomicXor(&bnd[J.vbase + c], a ^ b);
	}
}

// ---- step 2 (after scanning cnt -> start): scatter face ids into each vertex' slot range ----
__global__ __launch_bounds__(256) void k_normal_fill(const NormalJob *__restrict__ jobs, const uint32_t *__restrict__ block_job,
                                                     const uint32_t *__restrict__ block_first, uint32_t nblocks,
                                                     const uint32_t *__restrict__ start, uint32_t *__restrict__ cursor, uint32_t *__restrict__ adj) {
	if(blockIdx.x >= nblocks) return;
	const NormalJob J = jobs[block_job[blockIdx.x]];
	const uint32_t f = (blockIdx.x - block_first[block_job[blockIdx.x]])*256 + threadIdx.x;
	if(f >= J.nface) return;
	uint32_t v[3];
	load_face(J, f, v[0], v[1], v[2]);
	if(v[0] >= J.nvert || v[1] >= J.nvert || v[2] >= J.nvert) return;
#pragma unroll
	for(int k = 0; k < 3; k++) {
		const uint32_t g = J.vbase + v[k];
		adj[start[g] + atomicAdd(&cursor[g], 1u)] = f;
	}
}

// ---- step 3: flag vertices that take a correction (ESTIMATED: all, BORDER: boundary != 0) ----
__global__ __launch_bounds__(256) void k_normal_flags(const NormalJob *__restrict__ jobs, const uint32_t *__restrict__ block_job,
                                                      const uint32_t *__restrict__ block_first, uint32_t nblocks,
                                                      const uint32_t *__restrict__ bnd, uint32_t *__restrict__ flag) {
	if(blockIdx.x >= nblocks) return;
	const NormalJob J = jobs[block_job[blockIdx.x]];
	if(J.prediction == 0 || J.fused) return;            // DIFF / fused jobs own no slice of the per-vertex scratch
	const uint32_t i = (blockIdx.x - block_first[block_job[blockIdx.x]])*256 + threadIdx.x;
	if(i >= J.nvert) return;
	flag[J.vbase + i] = (J.prediction == 1 || (J.prediction == 2 && bnd[J.vbase + i] != 0)) ? 1u : 0u;   // (COMPUTED: no vertex takes a correction)
}

// ---- step 4: per vertex ordered accumulation + computeNormals ----
__global__ __launch_bounds__(256) void k_normal_vertex(const NormalJob *__restrict__ jobs, const uint32_t *__restrict__ block_job,
                                                       const uint32_t *__restrict__ block_first, uint32_t nblocks,
                                                       const float *__restrict__ facen, const uint32_t *__restrict__ start,
                                                       const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ adj,
                                                       const uint32_t *__restrict__ flag, const uint32_t *__restrict__ slot) {
	if(blockIdx.x >= nblocks) return;
	const NormalJob J = jobs[block_job[blockIdx.x]];
	if(J.prediction == 0 || J.fused) return;
	const uint32_t i = (blockIdx.x - block_first[block_job[blockIdx.x]])*256 + threadIdx.x;
	if(i >= J.nvert) return;
	const uint32_t g = J.vbase + i;
	const uint32_t deg = cnt[g];
	const uint32_t *__restrict__ list = adj + start[g];
	float ex = 0.f, ey = 0.f, ez = 0.f;
	// incident faces in ascending id (= the order estimateNormals visits them); a face listing this vertex
	// twice adds twice, consecutively, as the reference's three += in a row do.
	int64_t last = -1;
	for(uint32_t done = 0; done < deg;) {
		uint32_t best = 0xFFFFFFFFu, mult = 0;
		for(uint32_t k = 0; k < deg; k++) {
			const uint32_t f = list[k];
			if((int64_t)f > last) { if(f < best) { best = f; mult = 1; } else if(f == best) mult++; }
		}
		const float *n = facen + ((size_t)J.fbase + best)*3;
		const float nx = n[0], ny = n[1], nz = n[2];
		for(uint32_t m = 0; m < mult; m++) { ex += nx; ey += ny; ez += nz; }
		last = best; done += mult;
	}
	if(flag[g]) {                                       // normal_attribute.cpp:289-293 / 313-316
		const uint32_t s = slot[g] - slot[J.vbase];
		int32_t qx, qy;
		to_octa(ex, ey, ez, J.unit, qx, qy);
		int32_t dx = 0, dy = 0;
		if(s < J.ndiffs) { dx = J.diffs[2*(size_t)s]; dy = J.diffs[2*(size_t)s + 1]; }
		int32_t x = (int32_t)((uint32_t)qx + (uint32_t)dx), y = (int32_t)((uint32_t)qy + (uint32_t)dy);
		if(J.out_i16) { x = (int16_t)(uint16_t)(uint32_t)x; y = (int16_t)(uint16_t)(uint32_t)y; }
		float nx, ny, nz;
		to_sphere(x, y, J.unit, nx, ny, nz);
		store_normal(J, i, nx, ny, nz);
	} else if(J.out_i16) {                              // normal_attribute.cpp:294-302
		float len = norm3(ex, ey, ez);
		int16_t *o = (int16_t *)((uint8_t *)J.out + (size_t)i*J.out_stride);
		if(!(len < 0.00001f)) {
			len = 32767.0f/len;
			o[0] = f2s_x86(ex*len); o[1] = f2s_x86(ey*len); o[2] = f2s_x86(ez*len);
		} else if(J.prediction == 3) { o[0] = 0; o[1] = 0; o[2] = 32767; }   // COMPUTED: upstream sets (0,0,1) here and never stores it
	} else {                                            // normal_attribute.cpp:317-322
		const float len = norm3(ex, ey, ez);
		float *o = (float *)((uint8_t *)J.out + (size_t)i*J.out_stride);
		if(J.prediction == 3 && len < 0.00001f) { o[0] = 0.f; o[1] = 0.f; o[2] = 1.f; }   // COMPUTED: no 0/0 for a renderer
		else { o[0] = ex/len; o[1] = ey/len; o[2] = ez/len; }
	}
}

// ------------------------------------------------------------------------------------------------
// Small-blob path: the whole ESTIMATED/BORDER pipeline of one blob in ONE workgroup with its intermediates in LDS
// (incidence counts -> CSR offsets, boundary XORs, adjacency, correction slots), replacing nine batch-wide launches.
// Same arithmetic and the same ascending-face-id accumulation order as the kernels above.  The integer positions are
// read from HBM/L2 (25 KB for a 2K-vertex blob: it stays in the CU's L1) rather than staged, and offsets are 16-bit
// (3*nface <= 65535), so that the workgroup's LDS (50 KB for the 4K-triangle blob) fits beside the CLERS automata of
// the batches behind it in a pipelined decode (k_mesh.hip: three 49 KB fronts per CU leave little).
// Dynamic LDS layout (round 3: 41.5 -> 28.6 KB for the 4K-triangle blob; LDS.time is what bounds a pipelined decode):
//   cur[nvert+2] u16 | fbits[2*ceil(nvert/64)] u32 | fpre[same] u16 | bnd[nvert] u32, later adj[3*nface] u16
// cur is, in turn, the incidence counts (two vertices share a dword: ds_add_u32 of 1 or 1<<16; no half can overflow, 3*nface <= 65535),
// their exclusive scan IN PLACE, the fill cursors - and, after the fill, cur[i] is where vertex i's list ENDS, i.e. where vertex i+1's
// starts: no separate offset array.  The vertices that take a correction (ESTIMATED: all; BORDER: the boundary) are a bitmap with a
// prefix count per dword; a vertex' slot in the diff stream is a popcount away.  The adjacency takes the boundary XORs' place.
// COMPUTED (k_normal_blob<true>: prediction 3, normals for a blob that stores none): the same counts, scan, fill, ordered accumulation and
// positions-to-float pass in the same LDS layout, without what a correction needs - no boundary XORs, no bitmap / prefix counts, no diff reads, no
// octahedral round trip - and every vertex normalised, (0,0,1) where the estimate is zero.  A template parameter of the kernel (k_delta_tiles' idiom)
// and a launch of its own over its own id list: <false> is the kernel as it was, instruction for instruction (through a shared __device__ body
// the same source came out with 4 more VGPRs and three times the SGPR spills).
template <bool COMPUTED> __global__ __launch_bounds__(256) void k_normal_blob(const NormalJob *__restrict__ jobs, const uint32_t *__restrict__ job_ids, uint32_t njobs, uint32_t lds_bytes) {
	if(blockIdx.x >= njobs) return;
	const NormalJob J = jobs[job_ids[blockIdx.x]];
	extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
	const uint32_t nv = J.nvert, nf = J.nface, tid = threadIdx.x;
	const uint32_t ncur = (nv + 2) & ~1u, ndw = 2*((nv + 63)/64);
	CRT_LDS uint16_t *cur = (CRT_LDS uint16_t *)as_lds(lds_raw);
	CRT_LDS uint32_t *cur32 = (CRT_LDS uint32_t *)cur;
	CRT_LDS uint32_t *fbits = (CRT_LDS uint32_t *)(cur + ncur);
	CRT_LDS uint16_t *fpre = (CRT_LDS uint16_t *)(fbits + ndw);
	CRT_LDS uint32_t *bnd = (CRT_LDS uint32_t *)(as_lds(lds_raw) + normal_blob_lds_head(nv));
	CRT_LDS uint16_t *adj = (CRT_LDS uint16_t *)bnd;
	auto bump = [&](uint32_t v) -> uint32_t {                              // cur[v]++ ; returns the old value
		const uint32_t sh = (v & 1u)*16u;
		return (atomicAdd((uint32_t *)&cur32[v >> 1], 1u << sh) >> sh) & 0xFFFFu;
	};
	// small blobs: every face's normal is computed once, while the incidence is counted, and kept in LDS; the ordered accumulation
	// then never leaves LDS.  Bigger blobs recompute it per incident vertex from HBM/L2 (two dependent loads per face and vertex)
	// to stay within a CU's LDS.
	const bool fn_lds = normal_blob_lds_fn(nv, nf) <= lds_bytes;
	CRT_LDS float *fn = (CRT_LDS float *)(as_lds(lds_raw) + ((normal_blob_lds(nv, nf) + 15u) & ~15u));
	// ... or once into a scratch array in HBM (it never leaves L2: 48 KB for a 4K-triangle blob) - what a context gets when many batches are
	// in flight: the LDS-lean layout without recomputing every face's normal for each of its three vertices (round 2's lean path: 72
	// dependent loads and three cross products per vertex where 18 loads do; 50 -> 3x us per C4 batch, and LDS.time is what bounds the pipeline)
	CRT_GLOBAL float *fng = !fn_lds && J.fn_scratch ? as_global(J.fn_scratch) : nullptr;
	const bool fn_any = fn_lds || fng != nullptr;
	__shared__ uint32_t scan_s[4];
	CRT_GLOBAL const int32_t *pos = as_global(J.position);
	CRT_GLOBAL const uint32_t *f32 = J.faces_u16 ? nullptr : as_global((const uint32_t *)J.faces);
	CRT_GLOBAL const uint16_t *f16 = J.faces_u16 ? as_global((const uint16_t *)J.faces) : nullptr;
	auto face = [&](uint32_t f, uint32_t &a, uint32_t &b, uint32_t &c) {
		if(f16) { a = f16[3*(size_t)f]; b = f16[3*(size_t)f + 1]; c = f16[3*(size_t)f + 2]; }
		else { a = f32[3*(size_t)f]; b = f32[3*(size_t)f + 1]; c = f32[3*(size_t)f + 2]; }
	};
	// the correction of diff-stream slot `rank`: two int32, or (K-BIT wrote halfwords: every width of the stream <= 16 bits) two int16 in one dword
	const bool diffs_i16 = J.diffs_i16 != 0;
	auto diff_at = [&](uint32_t rank, int32_t &dx, int32_t &dy) {
		if(diffs_i16) { const uint32_t w = ((CRT_GLOBAL const uint32_t *)as_global(J.diffs))[rank]; dx = (int32_t)(int16_t)(w & 0xFFFFu); dy = (int32_t)(int16_t)(w >> 16); }
		else { CRT_GLOBAL const int32_t *dp = as_global(J.diffs) + 2*(size_t)rank; dx = dp[0]; dy = dp[1]; }
	};
	if constexpr(!COMPUTED) for(uint32_t i = tid; i < nv; i += 256) bnd[i] = 0;
	for(uint32_t i = tid; i < ncur/2; i += 256) cur32[i] = 0;
	__syncthreads();
	// incidence counts + boundary XOR (markBoundary, normal_attribute.cpp:24-37)
	bool bad = false;
	for(uint32_t f0 = tid; f0 < nf; f0 += 1024) {                           // four faces per thread and pass: their indices in flight together, then their
		uint32_t A[4], B[4], C[4];                                           // 36 coordinates (one face at a time every pass was two dependent round trips)
		bool ok[4];
#pragma unroll
		for(uint32_t u = 0; u < 4; u++) face(f0 + 256*u < nf ? f0 + 256*u : nf - 1u, A[u], B[u], C[u]);
#pragma unroll
		for(uint32_t u = 0; u < 4; u++) asm volatile("" : "+v"(A[u]), "+v"(B[u]), "+v"(C[u]));
#pragma unroll
		for(uint32_t u = 0; u < 4; u++) {
			const bool in = f0 + 256*u < nf;
			ok[u] = in && A[u] < nv && B[u] < nv && C[u] < nv;
			bad |= in && !ok[u];
		}
		int32_t P[4][9];
		if(fn_any) {
#pragma unroll
			for(uint32_t u = 0; u < 4; u++) {
				CRT_GLOBAL const int32_t *p0 = pos + 3*(ok[u] ? A[u] : 0u), *p1 = pos + 3*(ok[u] ? B[u] : 0u), *p2 = pos + 3*(ok[u] ? C[u] : 0u);
				P[u][0] = p0[0]; P[u][1] = p0[1]; P[u][2] = p0[2]; P[u][3] = p1[0]; P[u][4] = p1[1]; P[u][5] = p1[2]; P[u][6] = p2[0]; P[u][7] = p2[1]; P[u][8] = p2[2];
			}
#pragma unroll
			for(uint32_t u = 0; u < 4; u++) asm volatile("" : "+v"(P[u][0]), "+v"(P[u][1]), "+v"(P[u][2]), "+v"(P[u][3]), "+v"(P[u][4]), "+v"(P[u][5]), "+v"(P[u][6]), "+v"(P[u][7]), "+v"(P[u][8]));
		}
#pragma unroll
		for(uint32_t u = 0; u < 4; u++) if(ok[u]) {
			const uint32_t f = f0 + 256*u, a = A[u], b = B[u], c = C[u];
			(void)bump(a); (void)bump(b); (void)bump(c);
			if(fn_any) {
				const float x0 = (float)P[u][0], y0 = (float)P[u][1], z0 = (float)P[u][2];
				const float ax = (float)P[u][3] - x0, ay = (float)P[u][4] - y0, az = (float)P[u][5] - z0;
				const float bx = (float)P[u][6] - x0, by = (float)P[u][7] - y0, bz = (float)P[u][8] - z0;
				const float nx = ay*bz - az*by, ny = az*bx - ax*bz, nz = ax*by - ay*bx;   // point.h:113-115
				if(fn_lds) { fn[3*f] = nx; fn[3*f + 1] = ny; fn[3*f + 2] = nz; }
				else { fng[3*(size_t)f] = nx; fng[3*(size_t)f + 1] = ny; fng[3*(size_t)f + 2] = nz; }
			}
			if constexpr(!COMPUTED) if(J.prediction == 2) { atomicXor((uint32_t *)&bnd[a], b ^ c); atomicXor((uint32_t *)&bnd[b], c ^ a); atomicXor((uint32_t *)&bnd[c], a ^ b); }
		}
	}
	if(bad) *as_global(J.status) = -5;
	if(fng) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");           // the face normals in HBM: written here, read by other waves of this workgroup below
	__syncthreads();
	if(fng) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
	// the integer positions have been read for the last time when the face normals sit in LDS: they become floats now (in place, or
	// into an interleaved vertex buffer), while the rest of the kernel works from LDS; otherwise at the very end (below)
	auto positions_out = [&]() {                                           // (loads in groups, every one of a group in flight: one at a time this loop was a third of the kernel)
		if(!J.pos_out) return;
		CRT_GLOBAL uint8_t *po = as_global((uint8_t *)J.pos_out);
		const uint32_t n3 = 3*nv;
		if(n3 == 0) return;
		typedef uint32_t nu4 __attribute__((ext_vector_type(4)));
		typedef float nf4 __attribute__((ext_vector_type(4)));
		uint32_t done = 0;
		if(J.pos_stride == 12 && ((((uintptr_t)po) | ((uintptr_t)pos)) & 15) == 0 && n3 >= 4) {   // packed: 16-byte vectors, four per thread and pass
			const uint32_t nvec = n3 >> 2;
			CRT_GLOBAL const nu4 *src4 = (CRT_GLOBAL const nu4 *)pos;
			CRT_GLOBAL nf4 *dst4 = (CRT_GLOBAL nf4 *)po;
			for(uint32_t i = tid; i < nvec; i += 1024) {
				nu4 t[4];
#pragma unroll
				for(uint32_t u = 0; u < 4; u++) t[u] = src4[i + 256*u < nvec ? i + 256*u : nvec - 1u];
#pragma unroll
				for(uint32_t u = 0; u < 4; u++) asm volatile("" : "+v"(t[u]));
#pragma unroll
				for(uint32_t u = 0; u < 4; u++) if(i + 256*u < nvec) {
					nf4 f;
					f.x = (float)(int32_t)t[u].x*J.pos_q; f.y = (float)(int32_t)t[u].y*J.pos_q; f.z = (float)(int32_t)t[u].z*J.pos_q; f.w = (float)(int32_t)t[u].w*J.pos_q;
					dst4[i + 256*u] = f;
				}
			}
			done = nvec << 2;
		}
		for(uint32_t e0 = done + tid; e0 < n3; e0 += 2048) {                // interleaved vertex buffers, tails: eight scalars per thread and pass
			int32_t t[8];
#pragma unroll
			for(uint32_t u = 0; u < 8; u++) t[u] = pos[e0 + 256*u < n3 ? e0 + 256*u : n3 - 1u];
			asm volatile("" : "+v"(t[0]), "+v"(t[1]), "+v"(t[2]), "+v"(t[3]), "+v"(t[4]), "+v"(t[5]), "+v"(t[6]), "+v"(t[7]));
#pragma unroll
			for(uint32_t u = 0; u < 8; u++) {
				const uint32_t e = e0 + 256*u;
				if(e < n3) { const uint32_t i = e/3, c = e - 3*i; const float f = (float)t[u]; *(CRT_GLOBAL float *)(po + (size_t)i*J.pos_stride + 4u*c) = f*J.pos_q; }
			}
		}
	};
	if(fn_any) positions_out();
	// the counts become CSR offsets (block-wide exclusive scan, in place); the vertices that take a correction become a bitmap + prefix counts
	const uint32_t per = (nv + 255)/256;
	{
		const uint32_t i0 = tid*per;
		uint32_t s = 0, total;
		if(per <= 16) {                                                    // (uniform) the thread's elements read once, all reads in flight, kept in registers
			uint32_t x[16];
#pragma unroll
			for(uint32_t k = 0; k < 16; k++) x[k] = cur[i0 + k < nv ? i0 + k : 0u];
			asm volatile("" : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]), "+v"(x[4]), "+v"(x[5]), "+v"(x[6]), "+v"(x[7]));
			asm volatile("" : "+v"(x[8]), "+v"(x[9]), "+v"(x[10]), "+v"(x[11]), "+v"(x[12]), "+v"(x[13]), "+v"(x[14]), "+v"(x[15]));
#pragma unroll
			for(uint32_t k = 0; k < 16; k++) { x[k] = k < per && i0 + k < nv ? x[k] : 0u; s += x[k]; }
			uint32_t o = block256_exclusive_scan<uint32_t>(s, scan_s, &total);
#pragma unroll
			for(uint32_t k = 0; k < 16; k++) if(k < per && i0 + k < nv) { cur[i0 + k] = (uint16_t)o; o += x[k]; }
		} else {
			for(uint32_t k = 0; k < per; k++) { const uint32_t i = i0 + k; if(i < nv) s += cur[i]; }
			uint32_t o = block256_exclusive_scan<uint32_t>(s, scan_s, &total);
			for(uint32_t k = 0; k < per; k++) { const uint32_t i = i0 + k; if(i < nv) { const uint32_t x = cur[i]; cur[i] = (uint16_t)o; o += x; } }
		}
	}
	if constexpr(!COMPUTED) {                                              // (the two blocks below keep their indentation: no vertex of a COMPUTED job takes a correction)
	for(uint32_t b0 = 0; b0 < nv; b0 += 256) {                               // (uniform trip count) 64 vertices' flags are one ballot
		const uint32_t i = b0 + tid;
		const uint64_t m = __ballot(i < nv && (J.prediction == 1 || bnd[i] != 0));
		if((tid & 63u) == 0 && i < nv) { fbits[(b0 + tid) >> 5] = (uint32_t)m; fbits[((b0 + tid) >> 5) + 1] = (uint32_t)(m >> 32); }
	}
	__syncthreads();
	{
		const uint32_t pd = (ndw + 255)/256, d0 = tid*pd;                      // <= 4 dwords a thread (nvert <= 32767)
		uint32_t s = 0, total;
		for(uint32_t k = 0; k < pd; k++) if(d0 + k < ndw && 32u*(d0 + k) < nv) s += (uint32_t)__popc(fbits[d0 + k]);
		uint32_t o = block256_exclusive_scan<uint32_t>(s, scan_s, &total);
		for(uint32_t k = 0; k < pd; k++) if(d0 + k < ndw) { fpre[d0 + k] = (uint16_t)o; if(32u*(d0 + k) < nv) o += (uint32_t)__popc(fbits[d0 + k]); }
	}
	}                                                                      // !COMPUTED
	__syncthreads();                                                       // (bnd has been read for the last time: the adjacency takes its place; COMPUTED: the offsets are in place)
	for(uint32_t f0 = tid; f0 < nf; f0 += 1024) {                           // four faces per thread and pass, as above; the twelve cursor bumps in flight together
		uint32_t V[4][3], at[4][3];                                          // (a face that is out or malformed bumps the spare counter cur[nv] and stores nothing)
#pragma unroll
		for(uint32_t u = 0; u < 4; u++) face(f0 + 256*u < nf ? f0 + 256*u : nf - 1u, V[u][0], V[u][1], V[u][2]);
#pragma unroll
		for(uint32_t u = 0; u < 4; u++) asm volatile("" : "+v"(V[u][0]), "+v"(V[u][1]), "+v"(V[u][2]));
		bool ok[4];
#pragma unroll
		for(uint32_t u = 0; u < 4; u++) {
			ok[u] = f0 + 256*u < nf && V[u][0] < nv && V[u][1] < nv && V[u][2] < nv;
#pragma unroll
			for(int k = 0; k < 3; k++) at[u][k] = bump(ok[u] ? V[u][k] : nv);
		}
#pragma unroll
		for(uint32_t u = 0; u < 4; u++) asm volatile("" : "+v"(at[u][0]), "+v"(at[u][1]), "+v"(at[u][2]));
#pragma unroll
		for(uint32_t u = 0; u < 4; u++) if(ok[u]) {
#pragma unroll
			for(int k = 0; k < 3; k++) adj[at[u][k]] = (uint16_t)(f0 + 256*u);
		}
	}
	__syncthreads();
	// per vertex: ordered accumulation (estimateNormals :40-59) + computeNormals (:281-325)
	// what a vertex' sum of face normals becomes (its correction: fetched by the caller ahead of the sum)
	auto finish = [&](uint32_t i, float ex, float ey, float ez, bool flagged, bool has_diff, int32_t pdx, int32_t pdy) {
		if constexpr(COMPUTED) {                                         // normal_attribute.cpp:294-302 / 320-323 at every vertex; a zero estimate: (0,0,1)
			const float len = norm3(ex, ey, ez);
			const bool zero = len < 0.00001f;                            // (integer positions: len is 0 or >= 1)
			if(J.out_i16) {
				const float l = 32767.0f/len;
				CRT_GLOBAL int16_t *o = (CRT_GLOBAL int16_t *)(as_global((uint8_t *)J.out) + (size_t)i*J.out_stride);
				o[0] = zero ? (int16_t)0 : f2s_x86(ex*l); o[1] = zero ? (int16_t)0 : f2s_x86(ey*l); o[2] = zero ? (int16_t)32767 : f2s_x86(ez*l);
			} else {
				CRT_GLOBAL float *o = (CRT_GLOBAL float *)(as_global((uint8_t *)J.out) + (size_t)i*J.out_stride);
				o[0] = zero ? 0.f : ex/len; o[1] = zero ? 0.f : ey/len; o[2] = zero ? 1.f : ez/len;
			}
			return;
		}
		if(flagged) {                                                    // ESTIMATED: every vertex; BORDER: boundary vertices
			int32_t qx, qy;
			to_octa(ex, ey, ez, J.unit, qx, qy);
			asm volatile("" : "+v"(pdx), "+v"(pdy));
			const int32_t dx = has_diff ? pdx : 0, dy = has_diff ? pdy : 0;
			int32_t x = (int32_t)((uint32_t)qx + (uint32_t)dx), y = (int32_t)((uint32_t)qy + (uint32_t)dy);
			if(J.out_i16) { x = (int16_t)(uint16_t)(uint32_t)x; y = (int16_t)(uint16_t)(uint32_t)y; }
			float nx, ny, nz;
			to_sphere(x, y, J.unit, nx, ny, nz);
			store_normal(J, i, nx, ny, nz);
		} else if(J.out_i16) {
			float len = norm3(ex, ey, ez);
			if(!(len < 0.00001f)) {
				len = 32767.0f/len;
				CRT_GLOBAL int16_t *o = (CRT_GLOBAL int16_t *)(as_global((uint8_t *)J.out) + (size_t)i*J.out_stride);
				o[0] = f2s_x86(ex*len); o[1] = f2s_x86(ey*len); o[2] = f2s_x86(ez*len);
			}
		} else {
			const float len = norm3(ex, ey, ez);
			CRT_GLOBAL float *o = (CRT_GLOBAL float *)(as_global((uint8_t *)J.out) + (size_t)i*J.out_stride);
			o[0] = ex/len; o[1] = ey/len; o[2] = ez/len;
		}
	};
	// Round 5: valences beyond 8 (a Delaunay mesh goes to 11, a decimated one to 20, a cone's apex to hundreds) took a selection loop of deg^2 LDS reads and
	// data-dependent branches with the whole wave waiting for its one such vertex (Delaunay discs: 0.100 ms a batch against the grid's 0.035; a valence-128
	// apex: 1.47 ms).  Now: up to 16 incident faces sort in a 63-exchange network in registers (every lane of a wave that holds such a vertex takes it: no
	// divergence), and a vertex beyond 16 is left to its WAVE afterwards - ranks by counting, the sorted ids back in place, the normals of 64 faces a
	// round in registers, and the sum taken in id order through v_readlane.
	const uint32_t HEAVY = 16;
	for(uint32_t i = tid; i < nv; i += 256) {
		uint32_t s0 = cur[i ? i - 1u : 0u], fw = 0, fp = 0;
		if constexpr(!COMPUTED) { fw = fbits[i >> 5]; fp = fpre[i >> 5]; }
		const uint32_t e0 = cur[i];
		asm volatile("" : "+v"(s0), "+v"(fw), "+v"(fp));
		s0 = i ? s0 : 0u;
		const uint32_t deg = e0 - s0;
		// the vertex' correction is fetched NOW (its slot is known), so that the load is back by the time the sum of face normals is
		const bool flagged = (fw >> (i & 31u)) & 1u;
		const uint32_t rank = fp + (uint32_t)__popc(fw & ((1u << (i & 31u)) - 1u));
		const bool has_diff = flagged && rank < J.ndiffs;
		int32_t pdx = 0, pdy = 0;
		if constexpr(!COMPUTED) if(J.ndiffs) diff_at(has_diff ? rank : 0u, pdx, pdy);
		float ex = 0.f, ey = 0.f, ez = 0.f;
		const bool wide = fn_any && __any(deg > 8 && deg <= HEAVY);          // (uniform) somebody in this wave needs the 16-wide network
		if(fn_any && deg > HEAVY) continue;                                  // the wave's job, below
		if(deg <= 8 && deg > 0 && !wide) {
			// the usual vertex: its (at most eight) incident faces sorted by id with a branch-free network and their normals added in that
			// order.  Equal ids (a face naming the vertex twice) end up adjacent and are added twice, as the reference does.  (The selection
			// loop below takes deg^2 data-dependent branches; a lone wave pays ~20 clocks for each.)
			// Every load here is UNCONDITIONAL, on a clamped index, and pinned by an empty asm statement: written as `k < deg ? adj[..] : ..`
			// the compiler sinks each one into an exec-masked branch of its own with its own wait - eight LDS round trips for the ids and
			// one per face for what follows, where one and two do.
			uint32_t id[8];
#pragma unroll
			for(uint32_t k = 0; k < 8; k++) id[k] = (uint32_t)adj[s0 + (k < deg ? k : 0u)];
			asm volatile("" : "+v"(id[0]), "+v"(id[1]), "+v"(id[2]), "+v"(id[3]), "+v"(id[4]), "+v"(id[5]), "+v"(id[6]), "+v"(id[7]));
#pragma unroll
			for(uint32_t k = 0; k < 8; k++) id[k] = k < deg ? id[k] : 0xFFFFFFFFu;
#define CRT_CX(p, q) { const uint32_t lo_ = min(id[p], id[q]), hi_ = max(id[p], id[q]); id[p] = lo_; id[q] = hi_; }
			CRT_CX(0, 1) CRT_CX(2, 3) CRT_CX(4, 5) CRT_CX(6, 7)
			CRT_CX(0, 2) CRT_CX(1, 3) CRT_CX(4, 6) CRT_CX(5, 7)
			CRT_CX(1, 2) CRT_CX(5, 6) CRT_CX(0, 4) CRT_CX(3, 7)
			CRT_CX(1, 5) CRT_CX(2, 6)
			CRT_CX(1, 4) CRT_CX(3, 6)
			CRT_CX(2, 4) CRT_CX(3, 5)
			CRT_CX(3, 4)
#undef CRT_CX
			const uint32_t id0 = id[0];                                      // a valid face: stands in for the unused slots' loads
			if(fn_any) {
				float n[8][3];
				if(fn_lds) {
#pragma unroll
					for(uint32_t k = 0; k < 8; k++) { const uint32_t f = k < deg ? id[k] : id0; n[k][0] = fn[3*f]; n[k][1] = fn[3*f + 1]; n[k][2] = fn[3*f + 2]; }
				} else {
#pragma unroll
					for(uint32_t k = 0; k < 8; k++) { const uint32_t f = k < deg ? id[k] : id0; CRT_GLOBAL const float *q = fng + 3*(size_t)f; n[k][0] = q[0]; n[k][1] = q[1]; n[k][2] = q[2]; }
				}
#pragma unroll
				for(uint32_t k = 0; k < 8; k++) asm volatile("" : "+v"(n[k][0]), "+v"(n[k][1]), "+v"(n[k][2]));
#pragma unroll
				for(uint32_t k = 0; k < 8; k++) { const bool on = k < deg; ex = on ? ex + n[k][0] : ex; ey = on ? ey + n[k][1] : ey; ez = on ? ez + n[k][2] : ez; }   // (select AFTER the add: x + 0.0f is not x for x = -0.0f)
			} else {
				// the LDS-lean layout (no face-normal array: what a context gets when many batches are in flight): the faces' indices and their
				// nine coordinates are fetched four faces at a time - every load of a group in flight together, two dependent round trips per
				// group instead of two per face - and the normals recomputed and added in id order
#pragma unroll
				for(uint32_t h = 0; h < 8; h += 4) {
					if(h >= deg) break;
					uint32_t fa[4][3];
					int32_t P[4][9];
#pragma unroll
					for(uint32_t k = 0; k < 4; k++) face(h + k < deg ? id[h + k] : id0, fa[k][0], fa[k][1], fa[k][2]);
#pragma unroll
					for(uint32_t k = 0; k < 4; k++) asm volatile("" : "+v"(fa[k][0]), "+v"(fa[k][1]), "+v"(fa[k][2]));
#pragma unroll
					for(uint32_t k = 0; k < 4; k++) {
#pragma unroll
						for(uint32_t v = 0; v < 3; v++) { CRT_GLOBAL const int32_t *q = pos + 3*fa[k][v]; P[k][3*v] = q[0]; P[k][3*v + 1] = q[1]; P[k][3*v + 2] = q[2]; }
					}
#pragma unroll
					for(uint32_t k = 0; k < 4; k++) asm volatile("" : "+v"(P[k][0]), "+v"(P[k][1]), "+v"(P[k][2]), "+v"(P[k][3]), "+v"(P[k][4]), "+v"(P[k][5]), "+v"(P[k][6]), "+v"(P[k][7]), "+v"(P[k][8]));
#pragma unroll
					for(uint32_t k = 0; k < 4; k++) {
						const float x0 = (float)P[k][0], y0 = (float)P[k][1], z0 = (float)P[k][2];
						const float ax = (float)P[k][3] - x0, ay = (float)P[k][4] - y0, az = (float)P[k][5] - z0;
						const float bx = (float)P[k][6] - x0, by = (float)P[k][7] - y0, bz = (float)P[k][8] - z0;
						const bool on = h + k < deg;
						const float nx = ay*bz - az*by, ny = az*bx - ax*bz, nz = ax*by - ay*bx;   // point.h:113-115
						ex = on ? ex + nx : ex; ey = on ? ey + ny : ey; ez = on ? ez + nz : ez;
					}
				}
			}
		} else if(fn_any && deg > 0) {                                       // up to 16 incident faces: the same recipe, twice as wide
			uint32_t id[16];
#pragma unroll
			for(uint32_t k = 0; k < 16; k++) id[k] = (uint32_t)adj[s0 + (k < deg ? k : 0u)];
			asm volatile("" : "+v"(id[0]), "+v"(id[1]), "+v"(id[2]), "+v"(id[3]), "+v"(id[4]), "+v"(id[5]), "+v"(id[6]), "+v"(id[7]));
			asm volatile("" : "+v"(id[8]), "+v"(id[9]), "+v"(id[10]), "+v"(id[11]), "+v"(id[12]), "+v"(id[13]), "+v"(id[14]), "+v"(id[15]));
#pragma unroll
			for(uint32_t k = 0; k < 16; k++) id[k] = k < deg ? id[k] : 0xFFFFFFFFu;
#define CRT_CX(p, q) { const uint32_t lo_ = min(id[p], id[q]), hi_ = max(id[p], id[q]); id[p] = lo_; id[q] = hi_; }
			CRT_CX(0, 1) CRT_CX(2, 3) CRT_CX(0, 2) CRT_CX(1, 3) CRT_CX(1, 2) CRT_CX(4, 5) CRT_CX(6, 7) CRT_CX(4, 6) CRT_CX(5, 7) CRT_CX(5, 6) CRT_CX(0, 4) CRT_CX(2, 6) CRT_CX(2, 4) CRT_CX(1, 5) CRT_CX(3, 7) CRT_CX(3, 5) CRT_CX(1, 2) CRT_CX(3, 4) CRT_CX(5, 6) CRT_CX(8, 9) CRT_CX(10, 11) CRT_CX(8, 10) CRT_CX(9, 11) CRT_CX(9, 10) CRT_CX(12, 13) CRT_CX(14, 15) CRT_CX(12, 14) CRT_CX(13, 15) CRT_CX(13, 14) CRT_CX(8, 12) CRT_CX(10, 14) CRT_CX(10, 12) CRT_CX(9, 13) CRT_CX(11, 15) CRT_CX(11, 13) CRT_CX(9, 10) CRT_CX(11, 12) CRT_CX(13, 14) CRT_CX(0, 8) CRT_CX(4, 12) CRT_CX(4, 8) CRT_CX(2, 10) CRT_CX(6, 14) CRT_CX(6, 10) CRT_CX(2, 4) CRT_CX(6, 8) CRT_CX(10, 12) CRT_CX(1, 9) CRT_CX(5, 13) CRT_CX(5, 9) CRT_CX(3, 11) CRT_CX(7, 15) CRT_CX(7, 11) CRT_CX(3, 5) CRT_CX(7, 9) CRT_CX(11, 13) CRT_CX(1, 2) CRT_CX(3, 4) CRT_CX(5, 6) CRT_CX(7, 8) CRT_CX(9, 10) CRT_CX(11, 12) CRT_CX(13, 14)      // Batcher's odd-even merge sort, 63 exchanges (checked on all 2^16 0/1 inputs)
#undef CRT_CX
			const uint32_t id0 = id[0];
#pragma unroll
			for(uint32_t h = 0; h < 16; h += 8) {                                // eight faces' normals in flight at a time
				if(h >= deg) break;
				float n[8][3];
				if(fn_lds) {
#pragma unroll
					for(uint32_t k = 0; k < 8; k++) { const uint32_t f = h + k < deg ? id[h + k] : id0; n[k][0] = fn[3*f]; n[k][1] = fn[3*f + 1]; n[k][2] = fn[3*f + 2]; }
				} else {
#pragma unroll
					for(uint32_t k = 0; k < 8; k++) { const uint32_t f = h + k < deg ? id[h + k] : id0; CRT_GLOBAL const float *q = fng + 3*(size_t)f; n[k][0] = q[0]; n[k][1] = q[1]; n[k][2] = q[2]; }
				}
#pragma unroll
				for(uint32_t k = 0; k < 8; k++) asm volatile("" : "+v"(n[k][0]), "+v"(n[k][1]), "+v"(n[k][2]));
#pragma unroll
				for(uint32_t k = 0; k < 8; k++) { const bool on = h + k < deg; ex = on ? ex + n[k][0] : ex; ey = on ? ey + n[k][1] : ey; ez = on ? ez + n[k][2] : ez; }
			}
		} else if(deg > 0) {                                                 // the LDS-lean layout without a face-normal array (a context that was given no scratch for one): the selection loop
		int32_t last = -1;
		for(uint32_t done = 0; done < deg;) {
			uint32_t best = 0xFFFFFFFFu, mult = 0;
			for(uint32_t k = 0; k < deg; k++) {
				const uint32_t f = adj[s0 + k];
				if((int32_t)f > last) { if(f < best) { best = f; mult = 1; } else if(f == best) mult++; }
			}
			float nx, ny, nz;
			if(fn_lds) { nx = fn[3*best]; ny = fn[3*best + 1]; nz = fn[3*best + 2]; }
			else if(fng) { nx = fng[3*(size_t)best]; ny = fng[3*(size_t)best + 1]; nz = fng[3*(size_t)best + 2]; }
			else {
				uint32_t a, b, c; face(best, a, b, c);
				CRT_GLOBAL const int32_t *p0 = pos + 3*a, *p1 = pos + 3*b, *p2 = pos + 3*c;
				const float x0 = (float)p0[0], y0 = (float)p0[1], z0 = (float)p0[2];
				const float ax = (float)p1[0] - x0, ay = (float)p1[1] - y0, az = (float)p1[2] - z0;
				const float bx = (float)p2[0] - x0, by = (float)p2[1] - y0, bz = (float)p2[2] - z0;
				nx = ay*bz - az*by; ny = az*bx - ax*bz; nz = ax*by - ay*bx;   // point.h:113-115
			}
			for(uint32_t m = 0; m < mult; m++) { ex += nx; ey += ny; ez += nz; }
			last = (int32_t)best; done += mult;
		}
		}
		finish(i, ex, ey, ez, flagged, has_diff, pdx, pdy);
	}
	if(fn_any) {
		// vertices of more than 16 faces, one at a time by the wave that skipped them above (wave w's lanes hold vertices 256*r + 64*w + lane)
		const uint32_t lane = tid & 63u;
		for(uint32_t base = tid & ~63u; base < nv; base += 256) {
			const uint32_t i = base + lane;
			uint32_t s0l = i < nv ? (uint32_t)cur[i ? i - 1u : 0u] : 0u;
			const uint32_t e0l = i < nv ? (uint32_t)cur[i] : 0u;
			s0l = i ? s0l : 0u;
			uint64_t hm = __ballot(i < nv && e0l - s0l > HEAVY);
			while(hm) {                                                          // (uniform)
				const uint32_t j = (uint32_t)__builtin_ctzll(hm);
				hm &= hm - 1;
				const uint32_t v = base + j;
				const uint32_t s0 = (uint32_t)__builtin_amdgcn_readlane((int)s0l, (int)j), deg = (uint32_t)__builtin_amdgcn_readlane((int)e0l, (int)j) - s0;
				float ex = 0.f, ey = 0.f, ez = 0.f;
				if(deg <= 512) {
					uint32_t id[8], rk[8];
#pragma unroll
					for(uint32_t k = 0; k < 8; k++) { const uint32_t e = lane + 64u*k; id[k] = e < deg ? (uint32_t)adj[s0 + e] : 0xFFFFFFFFu; rk[k] = 0; }
					for(uint32_t q = 0; q < deg; q++) {                               // ranks by counting: a broadcast read an element
						const uint32_t fq = (uint32_t)adj[s0 + q];
#pragma unroll
						for(uint32_t k = 0; k < 8; k++) rk[k] += (fq < id[k] || (fq == id[k] && q < lane + 64u*k)) ? 1u : 0u;
					}
					// (every lane has read what it needs: the wave runs in lockstep) the sorted ids take the list's place
#pragma unroll
					for(uint32_t k = 0; k < 8; k++) if(lane + 64u*k < deg) adj[s0 + rk[k]] = (uint16_t)id[k];
					for(uint32_t h = 0; h < deg; h += 64) {                           // 64 faces a round: their normals in registers, summed in id order
						const uint32_t e = h + lane;
						const uint32_t f = (uint32_t)adj[s0 + (e < deg ? e : 0u)];
						float nx, ny, nz;
						if(fn_lds) { nx = fn[3*f]; ny = fn[3*f + 1]; nz = fn[3*f + 2]; }
						else { CRT_GLOBAL const float *qn = fng + 3*(size_t)f; nx = qn[0]; ny = qn[1]; nz = qn[2]; }
						const uint32_t cnt = deg - h < 64u ? deg - h : 64u;
						for(uint32_t q = 0; q < cnt; q++) {
							ex += __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, nx), (int)q));
							ey += __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, ny), (int)q));
							ez += __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, nz), (int)q));
						}
					}
				} else {
					// more than 512 faces around one vertex (a polygon triangulated as a fan): no sort at all - the faces are walked in id order, 64 at a
					// time, and the ones that name the vertex add their normal (once per mention, as estimateNormals' three += do): nface / 64 rounds
					// whatever the valence (rounds 2-4 took a deg^2 selection loop here: seconds for a valence of 20 000)
					for(uint32_t f0 = 0; f0 < nf; f0 += 64) {
						const uint32_t f = f0 + lane;
						uint32_t fa, fb, fc;
						face(f < nf ? f : nf - 1u, fa, fb, fc);
						const bool okf = f < nf && fa < nv && fb < nv && fc < nv;       // (what the incidence count took)
						const uint32_t m = okf ? (fa == v ? 1u : 0u) + (fb == v ? 1u : 0u) + (fc == v ? 1u : 0u) : 0u;
						uint64_t hit = __ballot(m != 0);
						if(!hit) continue;
						const uint32_t fr = m ? f : 0u;
						float nx, ny, nz;
						if(fn_lds) { nx = fn[3*fr]; ny = fn[3*fr + 1]; nz = fn[3*fr + 2]; }
						else { CRT_GLOBAL const float *qn = fng + 3*(size_t)fr; nx = qn[0]; ny = qn[1]; nz = qn[2]; }
						while(hit) {
							const int q = (int)__builtin_ctzll(hit);
							hit &= hit - 1;
							const uint32_t mq = (uint32_t)__builtin_amdgcn_readlane((int)m, q);
							const float ax = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, nx), q));
							const float ay = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, ny), q));
							const float az = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, nz), q));
							for(uint32_t t = 0; t < mq; t++) { ex += ax; ey += ay; ez += az; }
						}
					}
				}
				if(lane == 0) {
					uint32_t fw = 0, fp = 0;
					if constexpr(!COMPUTED) { fw = fbits[v >> 5]; fp = fpre[v >> 5]; }
					const bool flagged = (fw >> (v & 31u)) & 1u;
					const uint32_t rank = fp + (uint32_t)__popc(fw & ((1u << (v & 31u)) - 1u));
					const bool has_diff = flagged && rank < J.ndiffs;
					int32_t pdx = 0, pdy = 0;
					if constexpr(!COMPUTED) if(has_diff) diff_at(rank, pdx, pdy);
					finish(v, ex, ey, ez, flagged, has_diff, pdx, pdy);
				}
			}
		}
	}
	if(!fn_any) { __syncthreads(); positions_out(); }
}
template __global__ void k_normal_blob<false>(const NormalJob *, const uint32_t *, uint32_t, uint32_t);
template __global__ void k_normal_blob<true>(const NormalJob *, const uint32_t *, uint32_t, uint32_t);

} // namespace corto_hip
