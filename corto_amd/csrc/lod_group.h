// lod_group.h — the workgroup as lod.h sees it, on the device: what k_lod.hip and k_cloud_lod.hip share.  One thread's state, and four words of LDS
// for what the waves tell one another (DPP scan, readlane, the barrier, the carry over the four waves).  Included behind kernels_common.h and lod.h
// by a file that defines WELD_KERNELS.
#pragma once

namespace corto_hip {

namespace {

struct LodGroupDev {
	LodLane L;
	WELD_LDS uint32_t *part;                                                 // a wave's sum (block_sum, block_scan)
	template <class F> __device__ __forceinline__ void each(F f) { f(threadIdx.x, L); }
	__device__ __forceinline__ void sync() { __syncthreads(); }
	__device__ __forceinline__ void block_sum() {
		const uint32_t s = (uint32_t)__builtin_amdgcn_readlane((int)wave_inclusive_scan_u32(L.c), 63);
		__syncthreads();                                                     // (the sums before these have been read)
		if(lane_id() == 0) part[wave_id()] = s;
		__syncthreads();
		if(threadIdx.x == 0) L.c = part[0] + part[1] + part[2] + part[3];
	}
	__device__ __forceinline__ void block_scan() {
		const uint32_t incl = wave_inclusive_scan_u32(L.c);
		const uint32_t tot = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
		__syncthreads();                                                     // (the sums before these have been read)
		if(lane_id() == 0) part[wave_id()] = tot;
		__syncthreads();
		const uint32_t p0 = part[0], p1 = part[1], p2 = part[2], p3 = part[3], w = wave_id();
		L.x = incl - L.c + (w > 0 ? p0 : 0u) + (w > 1 ? p1 : 0u) + (w > 2 ? p2 : 0u);
		L.t = p0 + p1 + p2 + p3;
	}
	template <class F> __device__ __forceinline__ void thread0(F f) { if(threadIdx.x == 0) f(L); }
};

} // namespace

} // namespace corto_hip
