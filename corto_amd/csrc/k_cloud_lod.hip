// k_cloud_lod.hip — K-CLOUD-LOD: levels of detail of a point cloud for gfx950 (crthip_batch_bind_cloud_lod).  cloud_lod.h has the method, the
// phases and both partitions; here are the workgroup (lod_group.h: k_lod.hip's) and the six grids.  A job is one LEVEL of one blob, so no
// kernel loops over levels.  Launched in stage M behind the levels of detail of the meshes and in front of k_dequant: a cloud's integer positions
// have been final since k_cloud_apply.
//
//   k_cloud_lod_blob     one workgroup a job whose table fits WELD_BLOB_LDS_MAX (nvert <= 8 192), from an id list: weld_slots(nvert) words of
//                        dynamic LDS, used three times; zero, insert the points by cell, barrier, lookup with the remap store, barrier; the
//                        weight words in the table's place, an LDS atomic add a point; a round of 256 vertices at a time the block scan of the
//                        kept flags, points and weights at the running base; the boxes in the table's place, LDS atomic minima and maxima;
//                        thread 0 stores the record as one 16-byte word.  LDS atomics only: no global atomic.
//   k_cloud_lod_insert   bigger jobs, LOD_BLOCK vertices a workgroup through a block -> job map: the table in scratch (zeroed, with the weight
//                        words behind it, by a FillJob in front)
//   k_cloud_lod_lookup   ... remap, the workgroup's kept count to its word, one atomic add a point to its representative's weight word
//   k_cloud_lod_offsets  one workgroup a job: the exclusive scan of the block counts, and the record
//   k_cloud_lod_scatter  ... LOD_BLOCK vertices a workgroup: the block scan of the kept flags, points and weights at the block's base
//   k_cloud_lod_chunks   a workgroup a chunk of the CAPACITY, ceil(nvert / K), through a second map: `cells` is read from the record, a
//                        workgroup past the level's chunks exits; six words of LDS, one record as two 16-byte stores
//                        No look-back, no spinning: the kernels' order on the stream is the only dependency.
// Plain C++: no inline assembly.
#define WELD_KERNELS                                                         // (weld.h: WELD_MEM / WELD_LDS are address spaces here)
#include "kernels_common.h"
#include "kernels.h"
#include "cloud_lod.h"
#include "lod_group.h"                                                       // (LodGroupDev: the workgroup as lod.h sees it)

namespace corto_hip {

namespace {

__device__ __forceinline__ LodIn in_of(const CloudLodJob &j) {
	LodIn J; J.w.position = (WELD_MEM const int32_t *)j.position; J.w.index = nullptr; J.w.index_u16 = 0;
	J.w.nface = 0; J.w.nvert = j.nvert; J.shift = j.shift;
	return J;
}

} // namespace

__global__ __launch_bounds__(LOD_THREADS) void k_cloud_lod_blob(const CloudLodJob *__restrict__ jobs, const uint32_t *__restrict__ job_ids, uint32_t njobs) {
	extern __shared__ __attribute__((aligned(16))) uint8_t cloud_lod_lds[];
	__shared__ uint32_t part[4];
	if(blockIdx.x >= njobs) return;
	const CloudLodJob j = jobs[job_ids[blockIdx.x]];
	LodGroupDev g; g.part = (WELD_LDS uint32_t *)part; g.L = LodLane{0u, 0u, 0u, 0u, 0u, 0u};
	cloud_lod_blob(g, in_of(j), WeldLdsTable{(WELD_LDS uint32_t *)cloud_lod_lds}, j.chunk_points, (WELD_MEM uint32_t *)j.remap, (WELD_MEM uint32_t *)j.points,
		(WELD_MEM uint32_t *)j.weight, (WELD_MEM crthip_cloud_chunk *)j.chunks, (WELD_MEM crthip_cloud_lod_counts *)j.counts, nullptr);
}

__global__ __launch_bounds__(LOD_THREADS) void k_cloud_lod_insert(const CloudLodJob *__restrict__ jobs, const uint32_t *__restrict__ block_job, uint32_t nblocks) {
	if(blockIdx.x >= nblocks) return;
	const CloudLodJob j = jobs[block_job[blockIdx.x]];
	const uint32_t k = blockIdx.x - j.vblock0;
	if(k >= weld_vblocks(j.nvert)) return;
	LodGroupDev g; g.part = nullptr;
	cloud_lod_insert_block(g, in_of(j), WeldMemTable{(WELD_MEM uint32_t *)j.table}, k, nullptr);
}

__global__ __launch_bounds__(LOD_THREADS) void k_cloud_lod_lookup(const CloudLodJob *__restrict__ jobs, const uint32_t *__restrict__ block_job, uint32_t nblocks) {
	__shared__ uint32_t part[4];
	if(blockIdx.x >= nblocks) return;
	const CloudLodJob j = jobs[block_job[blockIdx.x]];
	const uint32_t k = blockIdx.x - j.vblock0;
	if(k >= weld_vblocks(j.nvert)) return;
	LodGroupDev g; g.part = (WELD_LDS uint32_t *)part;
	cloud_lod_lookup_block(g, in_of(j), WeldMemTable{(WELD_MEM uint32_t *)j.table}, (WELD_MEM uint32_t *)j.remap, (WELD_MEM uint32_t *)j.blocks,
		(WELD_MEM uint32_t *)(j.weight ? j.wacc : nullptr), k);
}

__global__ __launch_bounds__(LOD_THREADS) void k_cloud_lod_offsets(const CloudLodJob *__restrict__ jobs, const uint32_t *__restrict__ job_ids, uint32_t njobs) {
	__shared__ uint32_t part[4];
	if(blockIdx.x >= njobs) return;
	const CloudLodJob j = jobs[job_ids[blockIdx.x]];
	LodGroupDev g; g.part = (WELD_LDS uint32_t *)part;
	cloud_lod_offsets_job(g, j.nvert, j.chunk_points, j.chunks != nullptr, (WELD_MEM uint32_t *)j.blocks, (WELD_MEM crthip_cloud_lod_counts *)j.counts);
}

__global__ __launch_bounds__(LOD_THREADS) void k_cloud_lod_scatter(const CloudLodJob *__restrict__ jobs, const uint32_t *__restrict__ block_job, uint32_t nblocks) {
	__shared__ uint32_t part[4];
	if(blockIdx.x >= nblocks) return;
	const CloudLodJob j = jobs[block_job[blockIdx.x]];
	const uint32_t k = blockIdx.x - j.vblock0;
	if(k >= weld_vblocks(j.nvert)) return;
	LodGroupDev g; g.part = (WELD_LDS uint32_t *)part;
	cloud_lod_scatter_block(g, j.nvert, (WELD_MEM const uint32_t *)j.remap, (WELD_MEM const uint32_t *)j.blocks, (WELD_MEM const uint32_t *)j.wacc,
		(WELD_MEM uint32_t *)j.points, (WELD_MEM uint32_t *)j.weight, k);
}

__global__ __launch_bounds__(LOD_THREADS) void k_cloud_lod_chunks(const CloudLodJob *__restrict__ jobs, const uint32_t *__restrict__ block_job, uint32_t nblocks) {
	__shared__ int32_t acc[6];
	if(blockIdx.x >= nblocks) return;
	const CloudLodJob j = jobs[block_job[blockIdx.x]];
	const uint32_t c = blockIdx.x - j.cblock0;
	if(!j.chunks || c >= cloud_lod_chunks_of(j.nvert, j.chunk_points)) return;
	LodGroupDev g; g.part = nullptr;
	cloud_lod_chunk_block(g, in_of(j), j.chunk_points, (WELD_MEM const uint32_t *)j.points, (WELD_MEM const crthip_cloud_lod_counts *)j.counts,
		(WELD_MEM crthip_cloud_chunk *)j.chunks, (WELD_LDS int32_t *)acc, c);
}

} // namespace corto_hip
