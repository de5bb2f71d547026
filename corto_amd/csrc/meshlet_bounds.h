// meshlet_bounds.h — crthip_batch_bind_meshlet_bounds: a box, a sphere and a normal cone a meshlet, from the blob's delta-decoded INTEGER
// positions and its final meshlet arrays (include/corto_hip.h has the contract).  The arithmetic and the partition of k_meshlet_bounds.hip as
// __host__ __device__ code, so that the host runs the very same source in the kernel's partition (crthip_meshlet_bounds_model,
// meshlet_bounds_host.cpp).
//
//   wave     one WAVE a meshlet (mb_meshlet).  Its lanes stride over the meshlet's vertices - the id, a presence test, the position into the
//            wave's LDS slots, a running minimum and maximum - and the wave reduces the six box sides; then over the slots again for the
//            largest squared distance from the centre; then twice over the faces: the sum S of the exact normals (integers modulo 2^64: no
//            order of lanes can change it), and, with the stored axis known, the least cosine (a float minimum is exact in any order).
//            Recomputing a face's normal in the second pass is cheaper than keeping 8 faces x 3 x 64 bits a lane.
//   wave ops every reduction is a 32-bit unsigned maximum or a 32-bit sum over the lanes: a signed value goes in biased, a minimum inverted,
//            a 64-bit maximum as its high half and then the low halves of the lanes that have it, a 64-bit sum in three pieces of 22 bits, a
//            float through the order-preserving key mb_fkey.  The kernel has DPP for both (kernels_common.h).
//   absent   a vertex id >= nvert is never an address: its slot is marked, it takes no part in box and sphere, and a face that names it is
//            no cone face.  A local id >= the meshlet's vertex count (no builder writes one) is treated the same way.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/corto_hip.h"
#include "tangent.h"

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define MB_HD __host__ __device__ inline
#else
#define MB_HD inline
#endif
// k_meshlet_bounds.hip defines MB_KERNELS: pointers into device memory and into LDS carry their address space there (global_* / ds_* and
// never flat_*: kernels_common.h); everywhere else, and in the host pass, the qualifiers are empty
#if defined(MB_KERNELS) && defined(__HIP_DEVICE_COMPILE__)
#define MB_MEM __attribute__((address_space(1)))
#define MB_LDS __attribute__((address_space(3)))
#define MB_DEVICE_PASS 1
#else
#define MB_MEM
#define MB_LDS
#define MB_DEVICE_PASS 0
#endif

namespace corto_hip {

constexpr uint32_t MB_WAVE = 64;
constexpr uint32_t MB_WAVES = 4;                           // meshlets a workgroup
constexpr uint32_t MB_MAX_VERTICES = 255, MB_MAX_TRIANGLES = 512;   // crthip_batch_bind_meshlets' limits
constexpr uint32_t MB_SLOTS = 256;                         // a wave's LDS: x, y, z, present a vertex
typedef int32_t mb_i32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t mb_u32x4 __attribute__((ext_vector_type(4)));
struct MbWaveMem { mb_i32x4 slot[MB_SLOTS]; };
static_assert(sizeof(MbWaveMem) == 4096, "a wave's LDS");

// what a wave knows of its blob
struct MbIn {
	MB_MEM const int32_t *position; uint32_t nvert;        // nvert x 3 delta-decoded integers, packed
	MB_MEM const mb_u32x4 *meshlets;                       // the final arrays of the meshlet binding
	MB_MEM const uint32_t *vertices;
	MB_MEM const uint8_t *triangles;
	uint32_t nmeshlets, nvertices, ntriangle_bytes;        // the blob's counts
	MB_MEM mb_u32x4 *out;                                  // crthip_meshlet_bounds records, three words of 16 bytes each
};
// a lane's share of every step
struct MbLane { uint32_t mn[3], mx[3], any; uint64_t r2; uint64_t S[3]; uint32_t faces; float m; };

MB_HD uint32_t mb_bias(int32_t x) { return (uint32_t)x ^ 0x80000000u; }      // order-preserving int32 -> uint32
MB_HD int32_t mb_unbias(uint32_t x) { return (int32_t)(x ^ 0x80000000u); }
// order-preserving finite float -> uint32 (-0 sorts below +0; both mean the same to everything behind)
MB_HD uint32_t mb_fkey(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return (u & 0x80000000u) ? ~u : u | 0x80000000u; }
MB_HD float mb_funkey(uint32_t k) { const uint32_t u = (k & 0x80000000u) ? k & 0x7FFFFFFFu : ~k; float f; __builtin_memcpy(&f, &u, 4); return f; }

// the smallest r in [0, 2^32 - 1] with r*r >= x, or 2^32 - 1 if there is none
MB_HD uint32_t mb_ceil_sqrt(uint64_t x) {
	uint32_t r = 0;                                                          // the largest r with r*r <= x, bit by bit
	for(uint32_t b = 0x80000000u; b; b >>= 1) { const uint32_t t = r | b; if((uint64_t)t*t <= x) r = t; }
	return (uint64_t)r*r == x || r == 0xFFFFFFFFu ? r : r + 1;
}

// a face's exact normal from three slots, modulo 2^64; false: a corner is absent or the normal is zero
MB_HD bool mb_face_normal(MB_LDS const MbWaveMem &W, uint32_t nv, uint32_t la, uint32_t lb, uint32_t lc, uint64_t N[3]) {
	if(la >= nv || lb >= nv || lc >= nv) return false;
	const mb_i32x4 a = W.slot[la], b = W.slot[lb], c = W.slot[lc];
	if(!(a.w && b.w && c.w)) return false;
	const uint64_t e1[3] = {tan_wide(b.x, a.x), tan_wide(b.y, a.y), tan_wide(b.z, a.z)}, e2[3] = {tan_wide(c.x, a.x), tan_wide(c.y, a.y), tan_wide(c.z, a.z)};
	N[0] = e1[1]*e2[2] - e1[2]*e2[1]; N[1] = e1[2]*e2[0] - e1[0]*e2[2]; N[2] = e1[0]*e2[1] - e1[1]*e2[0];
	return (N[0] | N[1] | N[2]) != 0;
}
// a sum's three components by their own shift, as floats (exact: below 2^24 in magnitude)
MB_HD void mb_scaled3(const uint64_t S[3], float s[3]) {
	const uint32_t k = tan_shift_of(tan_max_abs3(S));
	for(int c = 0; c < 3; c++) s[c] = (float)tan_scaled(S[c], k);
}
MB_HD float mb_len3(const float s[3]) { float l = s[0]*s[0] + s[1]*s[1]; l = l + s[2]*s[2]; return sqrtf(l); }

// The wave ops of the header's first lines, from the two the wave X has: x.max_u32(get) and x.sum_u32(get) over get(const MbLane &) of every lane
template <class X, class G> MB_HD uint32_t mb_min_u32(X &x, G get) { return ~x.max_u32([&](const MbLane &L) { return ~get(L); }); }
template <class X, class G> MB_HD uint64_t mb_max_u64(X &x, G get) {
	const uint32_t hi = x.max_u32([&](const MbLane &L) { return (uint32_t)(get(L) >> 32); });
	const uint32_t lo = x.max_u32([&](const MbLane &L) { const uint64_t v = get(L); return (uint32_t)(v >> 32) == hi ? (uint32_t)v : 0u; });
	return (uint64_t)hi << 32 | lo;
}
template <class X, class G> MB_HD uint64_t mb_sum_u64(X &x, G get) {         // 64 lanes x 22 bits stay below 2^28
	const uint64_t a = x.sum_u32([&](const MbLane &L) { return (uint32_t)get(L) & 0x3FFFFFu; });
	const uint64_t b = x.sum_u32([&](const MbLane &L) { return (uint32_t)(get(L) >> 22) & 0x3FFFFFu; });
	const uint64_t c = x.sum_u32([&](const MbLane &L) { return (uint32_t)(get(L) >> 44); });
	return a + (b << 22) + (c << 44);
}

// Meshlet k by one wave.  X is the wave: each(f) runs f(lane, MbLane &) for every lane (the kernel: its own; the host: all 64 in a shuffled
// order), sync() orders the lanes' LDS traffic, max_u32 / sum_u32 as above, uniform over the wave.  k < J.nmeshlets
template <class X> MB_HD void mb_meshlet(X &x, MB_LDS MbWaveMem &W, const MbIn &J, uint32_t k) {
	const mb_u32x4 rec = J.meshlets[k];
	// (what the builder wrote keeps all of these; a record that did not is cut to what is there, so that no address leaves the arrays)
	const uint32_t vo = rec.x < J.nvertices ? rec.x : J.nvertices, to = rec.y < J.ntriangle_bytes ? rec.y : J.ntriangle_bytes;
	uint32_t nv = rec.z < MB_MAX_VERTICES ? rec.z : MB_MAX_VERTICES, nt = rec.w < MB_MAX_TRIANGLES ? rec.w : MB_MAX_TRIANGLES;
	if(nv > J.nvertices - vo) nv = J.nvertices - vo;
	if(nt > (J.ntriangle_bytes - to)/3) nt = (J.ntriangle_bytes - to)/3;
	MB_MEM const uint32_t *V = J.vertices + vo;
	MB_MEM const uint8_t *T = J.triangles + to;

	// the vertices: into the slots, the lane's share of the box
	x.each([&](uint32_t lane, MbLane &L) {
		L.any = 0;
		for(int c = 0; c < 3; c++) { L.mn[c] = 0xFFFFFFFFu; L.mx[c] = 0; }
		for(uint32_t i = lane; i < nv; i += MB_WAVE) {
			const uint32_t id = V[i];
			mb_i32x4 p = {0, 0, 0, 0};
			if(id < J.nvert) {
				MB_MEM const int32_t *q = J.position + (size_t)id*3;
				p.x = q[0]; p.y = q[1]; p.z = q[2]; p.w = 1;
				const uint32_t u[3] = {mb_bias(p.x), mb_bias(p.y), mb_bias(p.z)};
				for(int c = 0; c < 3; c++) { if(u[c] < L.mn[c]) L.mn[c] = u[c]; if(u[c] > L.mx[c]) L.mx[c] = u[c]; }
				L.any = 1;
			}
			W.slot[i] = p;
		}
	});
	x.sync();
	mb_u32x4 r0 = {0, 0, 0, 0}, r1 = {0, 0, 0, 0}, r2 = {0, 0, 0x7Fu << 24, 0};     // (the all-zero record with cone_cutoff 127)
	if(x.max_u32([](const MbLane &L) { return L.any; })) {
		int32_t bmin[3], bmax[3], center[3];
		for(int c = 0; c < 3; c++) {
			bmin[c] = mb_unbias(mb_min_u32(x, [c](const MbLane &L) { return L.mn[c]; }));
			bmax[c] = mb_unbias(x.max_u32([c](const MbLane &L) { return L.mx[c]; }));
			const uint32_t span = (uint32_t)bmax[c] - (uint32_t)bmin[c];
			center[c] = (int32_t)((uint32_t)bmin[c] + (span >> 1));
		}
		// the sphere: the largest squared distance of a present vertex from the centre
		x.each([&](uint32_t lane, MbLane &L) {
			L.r2 = 0;
			for(uint32_t i = lane; i < nv; i += MB_WAVE) {
				const mb_i32x4 p = W.slot[i];
				if(!p.w) continue;
				const uint64_t dx = tan_wide(p.x, center[0]), dy = tan_wide(p.y, center[1]), dz = tan_wide(p.z, center[2]);
				const uint64_t d = dx*dx + dy*dy + dz*dz;
				if(d > L.r2) L.r2 = d;
			}
		});
		const uint32_t radius = mb_ceil_sqrt(mb_max_u64(x, [](const MbLane &L) { return L.r2; }));
		// the cone, first pass: the sum of the cone faces' normals
		x.each([&](uint32_t lane, MbLane &L) {
			L.S[0] = L.S[1] = L.S[2] = 0; L.faces = 0;
			for(uint32_t f = lane; f < nt; f += MB_WAVE) {
				uint64_t N[3];
				if(!mb_face_normal(W, nv, T[3*f], T[3*f + 1], T[3*f + 2], N)) continue;
				L.S[0] += N[0]; L.S[1] += N[1]; L.S[2] += N[2]; L.faces = 1;
			}
		});
		int32_t axis[3] = {0, 0, 0}, cutoff = 127;
		if(x.max_u32([](const MbLane &L) { return L.faces; })) {
			uint64_t S[3];
			for(int c = 0; c < 3; c++) S[c] = mb_sum_u64(x, [c](const MbLane &L) { return L.S[c]; });
			float s[3];
			mb_scaled3(S, s);
			const float len = mb_len3(s);
			if(len > 0) {
				float A[3];
				for(int c = 0; c < 3; c++) {
					float t = s[c]/len; t = t*127.0f;
					axis[c] = (int32_t)(int8_t)(int32_t)(t + (t < 0 ? -0.5f : 0.5f));
					A[c] = (float)axis[c];
				}
				const float la = mb_len3(A);
				// second pass: the least cosine between the stored axis and a cone face's normal
				x.each([&](uint32_t lane, MbLane &L) {
					L.m = INFINITY;
					for(uint32_t f = lane; f < nt; f += MB_WAVE) {
						uint64_t N[3];
						if(!mb_face_normal(W, nv, T[3*f], T[3*f + 1], T[3*f + 2], N)) continue;
						float n[3];
						mb_scaled3(N, n);
						float dot = A[0]*n[0] + A[1]*n[1]; dot = dot + A[2]*n[2];
						const float d = dot/(la*mb_len3(n));
						if(mb_fkey(d) < mb_fkey(L.m)) L.m = d;
					}
				});
				const float m = mb_funkey(mb_min_u32(x, [](const MbLane &L) { return mb_fkey(L.m); }));
				if(m > 0.1f) {
					float w = 1.0f - m*m;
					if(!(w > 0)) w = 0;                                          // (m may round to a step above 1)
					const int32_t cut = (int32_t)(sqrtf(w)*127.0f) + 2;
					cutoff = cut < 127 ? cut : 127;
				} else cutoff = 127;
			}
		}
		r0 = mb_u32x4{(uint32_t)bmin[0], (uint32_t)bmin[1], (uint32_t)bmin[2], (uint32_t)bmax[0]};
		r1 = mb_u32x4{(uint32_t)bmax[1], (uint32_t)bmax[2], (uint32_t)center[0], (uint32_t)center[1]};
		r2 = mb_u32x4{(uint32_t)center[2], radius, ((uint32_t)axis[0] & 255u) | ((uint32_t)axis[1] & 255u) << 8 | ((uint32_t)axis[2] & 255u) << 16 | (uint32_t)cutoff << 24, 0u};
	}
	x.each([&](uint32_t lane, MbLane &) {
		if(lane) return;
		MB_MEM mb_u32x4 *o = J.out + (size_t)3*k;                            // three 16-byte stores
		o[0] = r0; o[1] = r1; o[2] = r2;
	});
	x.sync();                                                                // (the slots are free for the wave's next meshlet)
}

} // namespace corto_hip
