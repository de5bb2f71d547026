// k_tangent.hip — K-TAN: vertex tangents for gfx950 (crthip_batch_bind_computed_tangents).  tangent.h has the arithmetic, the partition and
// the reason no order can change a bit: the per-face terms are summed as integers modulo 2^64, so the adds below are plain atomics with no
// ordered gather behind them (K-NRM's float sums need one).  Launched behind every normal kernel and in front of k_dequant: the normals
// are final, packed FLOAT position and uv buffers still hold their integers.
//
//   k_tangent_blob     one workgroup of 256 lanes a blob of up to TANGENT_BLOB_MAX vertices.  ONE accumulator of 3 x int64 a vertex in LDS
//                      (24 bytes a vertex: 50 KB for a 2 112-vertex blob, 54 KB at the limit), used twice: zeroed, the faces' T terms by
//                      ds_add_u64, a barrier, every lane keeps its vertices' T scaled in registers and zeroes their words, the faces' B terms,
//                      a barrier, the value.  The index, positions and uvs are read twice, through L1 / L2.
//   k_tangent_faces    blobs beyond that: blocks of TAN_BLOCK faces add both terms to the job's 6 x int64 a vertex of zeroed scratch with
//   k_tangent_vertex   64-bit global atomics (the vector memory path); then blocks of TAN_BLOCK vertices finish the values.
// A vertex's store is exactly its own 16 (FLOAT) or 8 (INT16) bytes.  Plain C++: no inline assembly, no float atomics.
#define TAN_KERNELS                                                          // (tangent.h: TAN_MEM is the global address space here)
#include "kernels_common.h"
#include "kernels.h"
#include "tangent.h"

namespace corto_hip {

namespace {

__device__ __forceinline__ TanIn in_of(const TangentJob &j) {
	TanIn J;
	// (TAN_MEM: the global address space in the device pass - tangent.h)
	J.position = (TAN_MEM const int32_t *)j.position; J.uv = (TAN_MEM const int32_t *)j.uv; J.faces = (TAN_MEM const void *)j.faces;
	J.faces_u16 = j.faces_u16; J.nvert = j.nvert; J.nface = j.nface;
	J.normal = (TAN_MEM const void *)j.normal; J.normal_i16 = j.normal_i16; J.normal_stride = j.normal_stride;
	J.out = (TAN_MEM void *)j.out; J.out_i16 = j.out_i16; J.out_stride = j.out_stride;
	return J;
}

} // namespace

__global__ __launch_bounds__(256) void k_tangent_blob(const TangentJob *__restrict__ jobs, const uint32_t *__restrict__ job_ids, uint32_t njobs) {
	extern __shared__ __attribute__((aligned(16))) uint8_t tan_lds[];
	if(blockIdx.x >= njobs) return;
	const TangentJob j = jobs[job_ids[blockIdx.x]];
	if(j.nvert > TAN_BLOB_SLOTS*TAN_THREADS) return;                         // (the planner sends no such job: the lanes' slots end there)
	const TanIn J = in_of(j);
	CRT_LDS uint64_t *acc = (CRT_LDS uint64_t *)as_lds(tan_lds);
	const uint32_t tid = threadIdx.x, nw = 3*J.nvert;
	for(uint32_t i = tid; i < nw; i += TAN_THREADS) acc[i] = 0;
	__syncthreads();
	auto add = [&](uint32_t v, uint32_t i, uint64_t x) { atomicAdd((unsigned long long *)&acc[3*v + i], (unsigned long long)x); };
	tan_faces_lane(J, 0, 0, J.nface, tid, add);
	__syncthreads();
	TanLaneState S;
	tan_blob_keep_T(J, acc, tid, S);                                         // (a lane reads and zeroes its own vertices' words only)
	__syncthreads();
	tan_faces_lane(J, 1, 0, J.nface, tid, add);
	__syncthreads();
	tan_blob_finish(J, acc, tid, S);
}

__global__ __launch_bounds__(256) void k_tangent_faces(const TangentJob *__restrict__ jobs, const uint32_t *__restrict__ block_job, uint32_t nblocks) {
	if(blockIdx.x >= nblocks) return;
	const TangentJob j = jobs[block_job[blockIdx.x]];
	const TanIn J = in_of(j);
	const uint32_t f0 = (blockIdx.x - j.fblock0)*TAN_BLOCK, f1 = J.nface - f0 > TAN_BLOCK ? f0 + TAN_BLOCK : J.nface;
	TAN_MEM uint64_t *acc = (TAN_MEM uint64_t *)j.acc;
#pragma unroll
	for(uint32_t which = 0; which < 2; which++)
		tan_faces_lane(J, which, f0, f1, threadIdx.x, [&](uint32_t v, uint32_t i, uint64_t x) {
			atomicAdd((unsigned long long *)&acc[(size_t)v*TAN_ACC_WORDS + 3*which + i], (unsigned long long)x); });
}

__global__ __launch_bounds__(256) void k_tangent_vertex(const TangentJob *__restrict__ jobs, const uint32_t *__restrict__ block_job, uint32_t nblocks) {
	if(blockIdx.x >= nblocks) return;
	const TangentJob j = jobs[block_job[blockIdx.x]];
	const TanIn J = in_of(j);
	const uint32_t v0 = (blockIdx.x - j.vblock0)*TAN_BLOCK, v1 = J.nvert - v0 > TAN_BLOCK ? v0 + TAN_BLOCK : J.nvert;
	for(uint32_t v = v0 + threadIdx.x; v < v1; v += TAN_THREADS) tan_vertex(J, v, (TAN_MEM const uint64_t *)j.acc);
}

} // namespace corto_hip
