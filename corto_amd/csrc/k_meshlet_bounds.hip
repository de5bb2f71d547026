// k_meshlet_bounds.hip — K-MLB: a box, a sphere and a normal cone a meshlet for gfx950 (crthip_batch_bind_meshlet_bounds).  meshlet_bounds.h has
// the arithmetic and the wave's steps; here are the wave (DPP maximum and sum, readlane) and the grid.  Launched behind the meshlet kernels - the
// arrays and the blob's counts are final - and in front of k_dequant and the quant kernels: a packed FLOAT position still holds its integers.
//
//   k_meshlet_bounds    a wave a meshlet, MB_WAVES (4) waves a workgroup, sizeof(MbWaveMem) (4 096 bytes) of LDS a wave: the meshlet's
//                       positions, 16 bytes a vertex.  The number of meshlets is known on the device only: the grid comes from a
//                       block -> job map sized by the capacity BOUND, every wave reads the blob's counts from device memory (the meshlet
//                       kernels' record) and a wave at or past them returns.  Lane 0 stores the record as three 16-byte words.
// Plain C++: no inline assembly, no atomics.
#define MB_KERNELS                                                           // (meshlet_bounds.h: MB_MEM / MB_LDS are address spaces here)
#include "kernels_common.h"
#include "kernels.h"
#include "meshlet_bounds.h"

namespace corto_hip {

namespace {

// the wave as mb_meshlet sees it: one lane a thread
struct MbWaveDev {
	MbLane L;
	uint32_t lane;
	template <class F> __device__ __forceinline__ void each(F f) { f(lane, L); }
	__device__ __forceinline__ void sync() {                                // the lanes of ONE wave: the LDS pipe keeps their order, the compiler must too
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
		__builtin_amdgcn_wave_barrier();
		__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
	}
	template <class G> __device__ __forceinline__ uint32_t max_u32(G get) { return wave_max_u32(get(L)); }
	template <class G> __device__ __forceinline__ uint32_t sum_u32(G get) { return (uint32_t)__builtin_amdgcn_readlane((int)wave_inclusive_scan_u32(get(L)), 63); }
};

} // namespace

__global__ __launch_bounds__(256) void k_meshlet_bounds(const MeshletBoundsJob *__restrict__ jobs, const uint32_t *__restrict__ block_job, uint32_t nblocks) {
	__shared__ __attribute__((aligned(16))) MbWaveMem mem[MB_WAVES];
	if(blockIdx.x >= nblocks) return;
	const MeshletBoundsJob j = jobs[block_job[blockIdx.x]];
	const uint32_t w = wave_id(), k = (blockIdx.x - j.block0)*MB_WAVES + w;
	const mb_u32x4 c = *(MB_MEM const mb_u32x4 *)j.counts;                   // crthip_meshlet_counts, as the meshlet kernels left it
	if(k >= c.x || k >= j.capacity) return;                                  // (whole waves: the grid is sized by the bound)
	MbIn J;
	J.position = (MB_MEM const int32_t *)j.position; J.nvert = j.nvert;
	J.meshlets = (MB_MEM const mb_u32x4 *)j.meshlets; J.vertices = (MB_MEM const uint32_t *)j.vertices; J.triangles = (MB_MEM const uint8_t *)j.triangles;
	J.nmeshlets = c.x; J.nvertices = c.y; J.ntriangle_bytes = c.z;
	J.out = (MB_MEM mb_u32x4 *)j.out;
	MbWaveDev x; x.lane = lane_id();
	mb_meshlet(x, *((MB_LDS MbWaveMem *)mem + w), J, k);
}

} // namespace corto_hip
