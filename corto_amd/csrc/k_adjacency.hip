// k_adjacency.hip — K-ADJ: the half-edge twins of the decoded index for gfx950 (crthip_batch_bind_adjacency).  adjacency.h has the rule, the
// phases and both partitions; here are the workgroup (DPP scan, readlane, the barrier) and the five grids.  Launched in stage M beside the
// meshlet kernels: the index has been final since the automata.
//
//   k_adjacency_blob     one workgroup a blob whose lists fit ADJ_BLOB_LDS_MAX, from an id list: uint32 ends (nvert + 1) and uint16 entries
//                        (3*nface) in dynamic LDS; count, scan, fill, twin and the block sums of the three counts in one kernel.  LDS atomics
//                        only: no global atomic, no scratch.
//   k_adjacency_count    bigger blobs, ADJ_BLOCK half-edges a workgroup through a block -> job map: the ends (zeroed by a FillJob in front)
//   k_adjacency_offsets  ... a workgroup a blob scans the nvert + 1 ends and zeroes the record
//   k_adjacency_fill     ... the entries, by atomic decrement of the ends
//   k_adjacency_twin     ... the twins; three atomic adds a workgroup to the record
//                        No look-back, no spinning: the kernels' order on the stream is the only dependency.
// Plain C++: no inline assembly.
#define ADJ_KERNELS                                                          // (adjacency.h: ADJ_MEM / ADJ_LDS are address spaces here)
#include "kernels_common.h"
#include "kernels.h"
#include "adjacency.h"

namespace corto_hip {

namespace {

// the workgroup as adjacency.h sees it: one thread's state, and sixteen words of LDS for what the waves tell one another
struct AdjGroupDev {
	AdjLane L;
	ADJ_LDS uint32_t *part;                                                  // [0, 4): a wave's sum (wave_carry); [4, 16): three counts a wave (block_sums)
	template <class F> __device__ __forceinline__ void each(F f) { f(threadIdx.x, L); }
	__device__ __forceinline__ void sync() { __syncthreads(); }
	__device__ __forceinline__ void wave_scan() {
		L.incl = wave_inclusive_scan_u32(L.v);
		L.tot = (uint32_t)__builtin_amdgcn_readlane((int)L.incl, 63);
	}
	__device__ __forceinline__ void wave_carry() {
		const uint32_t tot = (uint32_t)__builtin_amdgcn_readlane((int)wave_inclusive_scan_u32(L.v), 63);
		if(lane_id() == 0) part[wave_id()] = tot;
		__syncthreads();
		uint32_t c = 0;
		for(uint32_t k = 0; k < wave_id(); k++) c += part[k];
		L.carry = c;
	}
	__device__ __forceinline__ uint32_t wave_sum(uint32_t x) { return (uint32_t)__builtin_amdgcn_readlane((int)wave_inclusive_scan_u32(x), 63); }
	__device__ __forceinline__ void block_sums() {
		const uint32_t b = wave_sum(L.c.boundary), d = wave_sum(L.c.duplicate), i = wave_sum(L.c.invalid);
		if(lane_id() == 0) { part[4 + wave_id()] = b; part[8 + wave_id()] = d; part[12 + wave_id()] = i; }
		__syncthreads();
		if(threadIdx.x == 0) L.c = AdjCounts{part[4] + part[5] + part[6] + part[7], part[8] + part[9] + part[10] + part[11], part[12] + part[13] + part[14] + part[15]};
	}
	template <class F> __device__ __forceinline__ void thread0(F f) { if(threadIdx.x == 0) f(L); }
};

__device__ __forceinline__ AdjIn in_of(const AdjacencyJob &j) {
	AdjIn J; J.index = (ADJ_MEM const void *)j.index; J.index_u16 = j.index_u16; J.nface = j.nface; J.nvert = j.nvert;
	return J;
}
__device__ __forceinline__ AdjMemStore mem_of(const AdjacencyJob &j) { return AdjMemStore{(ADJ_MEM uint32_t *)j.ends, (ADJ_MEM uint32_t *)j.list}; }

} // namespace

__global__ __launch_bounds__(ADJ_THREADS) void k_adjacency_blob(const AdjacencyJob *__restrict__ jobs, const uint32_t *__restrict__ job_ids, uint32_t njobs) {
	extern __shared__ __attribute__((aligned(16))) uint8_t adj_lds[];
	__shared__ uint32_t part[16];
	if(blockIdx.x >= njobs) return;
	const AdjacencyJob j = jobs[job_ids[blockIdx.x]];
	const AdjLdsStore st{(ADJ_LDS uint32_t *)adj_lds, (ADJ_LDS uint16_t *)(adj_lds + (uint32_t)adj_ends_bytes(j.nvert))};
	AdjGroupDev g; g.part = (ADJ_LDS uint32_t *)part;
	adj_blob(g, in_of(j), st, (ADJ_MEM uint32_t *)j.twin, (ADJ_MEM crthip_adjacency_counts *)j.counts);
}

__global__ __launch_bounds__(ADJ_THREADS) void k_adjacency_count(const AdjacencyJob *__restrict__ jobs, const uint32_t *__restrict__ block_job, uint32_t nblocks) {
	if(blockIdx.x >= nblocks) return;
	const AdjacencyJob j = jobs[block_job[blockIdx.x]];
	const uint32_t k = blockIdx.x - j.block0;
	if(k >= adj_blocks(j.nface)) return;
	AdjGroupDev g; g.part = nullptr;
	adj_count_block(g, in_of(j), mem_of(j), k);
}

__global__ __launch_bounds__(ADJ_THREADS) void k_adjacency_offsets(const AdjacencyJob *__restrict__ jobs, const uint32_t *__restrict__ job_ids, uint32_t njobs) {
	__shared__ uint32_t part[16];
	if(blockIdx.x >= njobs) return;
	const AdjacencyJob j = jobs[job_ids[blockIdx.x]];
	AdjGroupDev g; g.part = (ADJ_LDS uint32_t *)part;
	adj_offsets(g, in_of(j), mem_of(j), (ADJ_MEM crthip_adjacency_counts *)j.counts);
}

__global__ __launch_bounds__(ADJ_THREADS) void k_adjacency_fill(const AdjacencyJob *__restrict__ jobs, const uint32_t *__restrict__ block_job, uint32_t nblocks) {
	if(blockIdx.x >= nblocks) return;
	const AdjacencyJob j = jobs[block_job[blockIdx.x]];
	const uint32_t k = blockIdx.x - j.block0;
	if(k >= adj_blocks(j.nface)) return;
	AdjGroupDev g; g.part = nullptr;
	adj_fill_block(g, in_of(j), mem_of(j), k);
}

__global__ __launch_bounds__(ADJ_THREADS) void k_adjacency_twin(const AdjacencyJob *__restrict__ jobs, const uint32_t *__restrict__ block_job, uint32_t nblocks) {
	__shared__ uint32_t part[16];
	if(blockIdx.x >= nblocks) return;
	const AdjacencyJob j = jobs[block_job[blockIdx.x]];
	const uint32_t k = blockIdx.x - j.block0;
	if(k >= adj_blocks(j.nface)) return;
	AdjGroupDev g; g.part = (ADJ_LDS uint32_t *)part;
	adj_twin_block(g, in_of(j), mem_of(j), (ADJ_MEM uint32_t *)j.twin, (ADJ_MEM crthip_adjacency_counts *)j.counts, k);
}

} // namespace corto_hip
