// k_encode_topo.hip — crthip_encode_batch's CLERS topology pass on the device for gfx950 (crthip_ctx_set_encode_topology): every mesh of a
// batch in one set of launches, one workgroup per mesh, running the stages of enc_topology.h.
//
//   K-ENC-TOPO-C   k_enc_topo_compact   degenerate faces dropped group by group (block scans keep the order), new group ends, used vertices
//   K-ENC-TOPO-P   k_enc_topo_pair      twin[] group by group: counts and scatter with atomics, then one lane per bucket puts its sides back
//                                       in fill order, sorts them as std::sort would (StdSortModel) and pairs them
//   K-ENC-TOPO-W   k_enc_topo_walk<LDS> the walk: lane 0 follows the chain, the workgroup clears and fills the state between groups.
//                                       LDS = true: the state image (16-bit links) in dynamic LDS, one workgroup a CU for a C4-sized mesh;
//                                       LDS = false: 32-bit links in the job's global image.  The planner picks per mesh (enc_topo_fits_lds).
// A dependent ds_read is about 50 cycles, a dependent L2 hit about 200 (MI355X_MICROARCH cycle table): that ratio is why the LDS image exists.
#include "kernels_common.h"
#include "kernels.h"
#include "enc_topology.h"

namespace corto_hip {

namespace {
struct EncTopoDevTeam {
	uint32_t tid, n;
	uint32_t *smem;                                   // 4 words for the block scan
	// (the device-scope fence: the stages count and scatter with atomics, which are carried out in L2, and then read those words with
	// plain loads - those must not be served from a line the CU's L1 took in before)
	__device__ __forceinline__ void sync() { __threadfence(); __syncthreads(); }
	__device__ __forceinline__ uint32_t scan(uint32_t v, uint32_t &total) { return block256_exclusive_scan<uint32_t>(v, smem, &total); }
	__device__ __forceinline__ uint32_t add(uint32_t *p, uint32_t v) { return atomicAdd(p, v); }
	__device__ __forceinline__ uint32_t order(uint32_t i, uint32_t) { return i; }
};
}

static_assert(ETOPO_THREADS == 256, "the team's scan is block256_exclusive_scan");
static_assert(ENC_TOPO_LDS_MAX == ETOPO_LDS_MAX, "the context raises the walk kernel's dynamic LDS limit to this");

__global__ __launch_bounds__(256) void k_enc_topo_compact(const EncTopoJob *__restrict__ jobs, uint32_t njobs) {
	__shared__ uint32_t smem[4];
	if(blockIdx.x >= njobs) return;
	EncTopoDevTeam T{threadIdx.x, ETOPO_THREADS, smem};
	enc_topo_compact(T, jobs[blockIdx.x]);
}

__global__ __launch_bounds__(256) void k_enc_topo_pair(const EncTopoJob *__restrict__ jobs, uint32_t njobs) {
	__shared__ uint32_t smem[4];
	if(blockIdx.x >= njobs) return;
	EncTopoDevTeam T{threadIdx.x, ETOPO_THREADS, smem};
	enc_topo_pair(T, jobs[blockIdx.x]);
}

template <bool LDS>
__global__ __launch_bounds__(256) void k_enc_topo_walk(const EncTopoJob *__restrict__ jobs, const uint32_t *__restrict__ ids, uint32_t nids) {
	extern __shared__ __attribute__((aligned(16))) uint8_t topo_image[];
	__shared__ uint32_t smem[4];
	if(blockIdx.x >= nids) return;
	const EncTopoJob &J = jobs[ids[blockIdx.x]];
	EncTopoDevTeam T{threadIdx.x, ETOPO_THREADS, smem};
	if(LDS) enc_topo_walk<uint16_t>(T, J, topo_image);
	else enc_topo_walk<uint32_t>(T, J, J.state);
}
template __global__ void k_enc_topo_walk<true>(const EncTopoJob *, const uint32_t *, uint32_t);
template __global__ void k_enc_topo_walk<false>(const EncTopoJob *, const uint32_t *, uint32_t);

} // namespace corto_hip
