// k_weld.hip — K-WELD: the weld map of the integer positions and the welded index for gfx950 (crthip_batch_bind_weld).  weld.h has the method, the
// phases and both partitions; here are the workgroup (DPP scan, readlane, the barrier) and the four grids.  Launched in stage M directly in front
// of the adjacency kernels, which may read the welded index (CRTHIP_WELD_ADJACENCY): the integer positions have been final since K-DELTA, the
// index since the automata, and k_dequant, which turns the positions into floats, runs behind.
//
//   k_weld_blob     one workgroup a blob whose table fits WELD_BLOB_LDS_MAX (nvert <= 8 192), from an id list: weld_slots(nvert) words of
//                   dynamic LDS; zero, insert, barrier, lookup with the remap store and the `unique` sum, barrier, the welded index with the
//                   `degenerate` sum; thread 0 stores the record as one 16-byte word.  LDS atomics only: no global atomic, no scratch.
//   k_weld_insert   bigger blobs, WELD_BLOCK vertices a workgroup through a block -> job map: the table in scratch (zeroed by a FillJob in
//                   front); a blob's first workgroup stores the record {nvert, 0, 0, 0}
//   k_weld_lookup   ... remap; one atomic add a workgroup to the record's `unique`
//   k_weld_index    ... WELD_BLOCK corners a workgroup through a second map, blobs with an index output only: the welded index; one atomic add a
//                   workgroup to the record's `degenerate`
//                   No look-back, no spinning: the kernels' order on the stream is the only dependency.
// Plain C++: no inline assembly.
#define WELD_KERNELS                                                         // (weld.h: WELD_MEM / WELD_LDS are address spaces here)
#include "kernels_common.h"
#include "kernels.h"
#include "weld.h"

namespace corto_hip {

namespace {

// the workgroup as weld.h sees it: one thread's state, and four words of LDS for what the waves tell one another
struct WeldGroupDev {
	WeldLane L;
	WELD_LDS uint32_t *part;                                                 // a wave's sum (block_sum)
	template <class F> __device__ __forceinline__ void each(F f) { f(threadIdx.x, L); }
	__device__ __forceinline__ void sync() { __syncthreads(); }
	__device__ __forceinline__ void block_sum() {
		const uint32_t s = (uint32_t)__builtin_amdgcn_readlane((int)wave_inclusive_scan_u32(L.c), 63);
		__syncthreads();                                                     // (the sum before this one has been read)
		if(lane_id() == 0) part[wave_id()] = s;
		__syncthreads();
		if(threadIdx.x == 0) L.c = part[0] + part[1] + part[2] + part[3];
	}
	template <class F> __device__ __forceinline__ void thread0(F f) { if(threadIdx.x == 0) f(L); }
};

__device__ __forceinline__ WeldIn in_of(const WeldJob &j) {
	WeldIn J; J.position = (WELD_MEM const int32_t *)j.position; J.index = (WELD_MEM const void *)j.index; J.index_u16 = j.index_u16; J.nface = j.nface; J.nvert = j.nvert;
	return J;
}

} // namespace

__global__ __launch_bounds__(WELD_THREADS) void k_weld_blob(const WeldJob *__restrict__ jobs, const uint32_t *__restrict__ job_ids, uint32_t njobs) {
	extern __shared__ __attribute__((aligned(16))) uint8_t weld_lds[];
	__shared__ uint32_t part[4];
	if(blockIdx.x >= njobs) return;
	const WeldJob j = jobs[job_ids[blockIdx.x]];
	WeldGroupDev g; g.part = (WELD_LDS uint32_t *)part; g.L.c = 0; g.L.unique = 0;
	weld_blob(g, in_of(j), WeldLdsTable{(WELD_LDS uint32_t *)weld_lds}, (WELD_MEM uint32_t *)j.remap, (WELD_MEM uint32_t *)j.windex, (WELD_MEM crthip_weld_counts *)j.counts, nullptr);
}

__global__ __launch_bounds__(WELD_THREADS) void k_weld_insert(const WeldJob *__restrict__ jobs, const uint32_t *__restrict__ block_job, uint32_t nblocks) {
	if(blockIdx.x >= nblocks) return;
	const WeldJob j = jobs[block_job[blockIdx.x]];
	const uint32_t k = blockIdx.x - j.vblock0;
	if(k >= weld_vblocks(j.nvert)) return;
	WeldGroupDev g; g.part = nullptr;
	weld_insert_block(g, in_of(j), WeldMemTable{(WELD_MEM uint32_t *)j.table}, (WELD_MEM crthip_weld_counts *)j.counts, k, nullptr);
}

__global__ __launch_bounds__(WELD_THREADS) void k_weld_lookup(const WeldJob *__restrict__ jobs, const uint32_t *__restrict__ block_job, uint32_t nblocks) {
	__shared__ uint32_t part[4];
	if(blockIdx.x >= nblocks) return;
	const WeldJob j = jobs[block_job[blockIdx.x]];
	const uint32_t k = blockIdx.x - j.vblock0;
	if(k >= weld_vblocks(j.nvert)) return;
	WeldGroupDev g; g.part = (WELD_LDS uint32_t *)part;
	weld_lookup_block(g, in_of(j), WeldMemTable{(WELD_MEM uint32_t *)j.table}, (WELD_MEM uint32_t *)j.remap, (WELD_MEM crthip_weld_counts *)j.counts, k);
}

__global__ __launch_bounds__(WELD_THREADS) void k_weld_index(const WeldJob *__restrict__ jobs, const uint32_t *__restrict__ block_job, uint32_t nblocks) {
	__shared__ uint32_t part[4];
	if(blockIdx.x >= nblocks) return;
	const WeldJob j = jobs[block_job[blockIdx.x]];
	const uint32_t k = blockIdx.x - j.cblock0;
	if(k >= weld_cblocks(j.nface)) return;
	WeldGroupDev g; g.part = (WELD_LDS uint32_t *)part;
	weld_index_block(g, in_of(j), (WELD_MEM const uint32_t *)j.remap, (WELD_MEM uint32_t *)j.windex, (WELD_MEM crthip_weld_counts *)j.counts, k);
}

} // namespace corto_hip
