// k_lod.hip — K-LOD: clustered levels of detail of the index for gfx950 (crthip_batch_bind_lod).  lod.h has the method, the phases and both
// partitions; here are the seven grids, over the workgroup of lod_group.h (DPP scan, readlane, the barrier, the carry over the four waves:
// k_cloud_lod.hip's too).  A job is one LEVEL of one blob, so no kernel loops over levels.  Launched in stage M behind the adjacency kernels and
// in front of k_dequant: the integer positions have been final since K-DELTA, the index since the automata.
//
//   k_lod_blob      one workgroup a job whose tables fit LOD_BLOB_LDS_MAX (nvert <= 8 192 and nface <= 8 192), from an id list:
//                   max(weld_slots(nvert), weld_slots(nface)) words of dynamic LDS, used twice; zero, insert the vertices by cell, barrier, lookup
//                   with the remap store and the `cells` sum, barrier, the clustered triples, zero again, insert the faces by key, barrier, then
//                   a round of 256 faces at a time: verdict, block scan of the kept flags, the kept triples at the running base; thread 0 stores
//                   the record as one 16-byte word.  LDS atomics only: no global atomic.
//   k_lod_insert    bigger jobs, LOD_BLOCK vertices a workgroup through a block -> job map: the vertex table in scratch (zeroed by a FillJob in
//                   front); a job's first workgroup stores the record {0, 0, 0, 0}
//   k_lod_lookup    ... remap; one atomic add a workgroup to the record's `cells`
//   k_lod_faces     LOD_BLOCK faces a workgroup through a second map: the clustered triples, and the faces that are not degenerate into the
//                   face table
//   k_lod_keep      ... the verdicts: a dropped face marked in its triple, the workgroup's kept count to its word, one atomic add each to the
//                   record's `degenerate` and `duplicate`
//   k_lod_offsets   one workgroup a job: the exclusive scan of the block counts, and the record's `faces`
//   k_lod_scatter   ... LOD_BLOCK faces a workgroup: the block scan of the kept flags, the kept triples at the block's base
//                   No look-back, no spinning: the kernels' order on the stream is the only dependency.
// Plain C++: no inline assembly.
#define WELD_KERNELS                                                         // (weld.h: WELD_MEM / WELD_LDS are address spaces here)
#include "kernels_common.h"
#include "kernels.h"
#include "lod.h"
#include "lod_group.h"                                                       // (LodGroupDev: the workgroup as lod.h sees it)

namespace corto_hip {

namespace {

__device__ __forceinline__ LodIn in_of(const LodJob &j) {
	LodIn J; J.w.position = (WELD_MEM const int32_t *)j.position; J.w.index = (WELD_MEM const void *)j.index; J.w.index_u16 = j.index_u16;
	J.w.nface = j.nface; J.w.nvert = j.nvert; J.shift = j.shift;
	return J;
}

} // namespace

__global__ __launch_bounds__(LOD_THREADS) void k_lod_blob(const LodJob *__restrict__ jobs, const uint32_t *__restrict__ job_ids, uint32_t njobs) {
	extern __shared__ __attribute__((aligned(16))) uint8_t lod_lds[];
	__shared__ uint32_t part[4];
	if(blockIdx.x >= njobs) return;
	const LodJob j = jobs[job_ids[blockIdx.x]];
	LodGroupDev g; g.part = (WELD_LDS uint32_t *)part; g.L = LodLane{0u, 0u, 0u, 0u, 0u, 0u};
	lod_blob(g, in_of(j), WeldLdsTable{(WELD_LDS uint32_t *)lod_lds}, (WELD_MEM uint32_t *)j.remap, (WELD_MEM uint32_t *)j.triples, (WELD_MEM uint32_t *)j.lod_index,
		(WELD_MEM crthip_lod_counts *)j.counts, nullptr);
}

__global__ __launch_bounds__(LOD_THREADS) void k_lod_insert(const LodJob *__restrict__ jobs, const uint32_t *__restrict__ block_job, uint32_t nblocks) {
	if(blockIdx.x >= nblocks) return;
	const LodJob j = jobs[block_job[blockIdx.x]];
	const uint32_t k = blockIdx.x - j.vblock0;
	if(k >= weld_vblocks(j.nvert)) return;
	LodGroupDev g; g.part = nullptr;
	lod_insert_block(g, in_of(j), WeldMemTable{(WELD_MEM uint32_t *)j.vtable}, (WELD_MEM crthip_lod_counts *)j.counts, k, nullptr);
}

__global__ __launch_bounds__(LOD_THREADS) void k_lod_lookup(const LodJob *__restrict__ jobs, const uint32_t *__restrict__ block_job, uint32_t nblocks) {
	__shared__ uint32_t part[4];
	if(blockIdx.x >= nblocks) return;
	const LodJob j = jobs[block_job[blockIdx.x]];
	const uint32_t k = blockIdx.x - j.vblock0;
	if(k >= weld_vblocks(j.nvert)) return;
	LodGroupDev g; g.part = (WELD_LDS uint32_t *)part;
	lod_lookup_block(g, in_of(j), WeldMemTable{(WELD_MEM uint32_t *)j.vtable}, (WELD_MEM uint32_t *)j.remap, (WELD_MEM crthip_lod_counts *)j.counts, k);
}

__global__ __launch_bounds__(LOD_THREADS) void k_lod_faces(const LodJob *__restrict__ jobs, const uint32_t *__restrict__ block_job, uint32_t nblocks) {
	if(blockIdx.x >= nblocks) return;
	const LodJob j = jobs[block_job[blockIdx.x]];
	const uint32_t k = blockIdx.x - j.fblock0;
	if(k >= lod_fblocks(j.nface)) return;
	LodGroupDev g; g.part = nullptr;
	lod_faces_block(g, in_of(j), WeldMemTable{(WELD_MEM uint32_t *)j.ftable}, (WELD_MEM const uint32_t *)j.remap, (WELD_MEM uint32_t *)j.triples, k, nullptr);
}

__global__ __launch_bounds__(LOD_THREADS) void k_lod_keep(const LodJob *__restrict__ jobs, const uint32_t *__restrict__ block_job, uint32_t nblocks) {
	__shared__ uint32_t part[4];
	if(blockIdx.x >= nblocks) return;
	const LodJob j = jobs[block_job[blockIdx.x]];
	const uint32_t k = blockIdx.x - j.fblock0;
	if(k >= lod_fblocks(j.nface)) return;
	LodGroupDev g; g.part = (WELD_LDS uint32_t *)part;
	lod_keep_block(g, in_of(j), WeldMemTable{(WELD_MEM uint32_t *)j.ftable}, (WELD_MEM uint32_t *)j.triples, (WELD_MEM uint32_t *)j.blocks, (WELD_MEM crthip_lod_counts *)j.counts, k);
}

__global__ __launch_bounds__(LOD_THREADS) void k_lod_offsets(const LodJob *__restrict__ jobs, const uint32_t *__restrict__ job_ids, uint32_t njobs) {
	__shared__ uint32_t part[4];
	if(blockIdx.x >= njobs) return;
	const LodJob j = jobs[job_ids[blockIdx.x]];
	LodGroupDev g; g.part = (WELD_LDS uint32_t *)part;
	lod_offsets_job(g, j.nface, (WELD_MEM uint32_t *)j.blocks, (WELD_MEM crthip_lod_counts *)j.counts);
}

__global__ __launch_bounds__(LOD_THREADS) void k_lod_scatter(const LodJob *__restrict__ jobs, const uint32_t *__restrict__ block_job, uint32_t nblocks) {
	__shared__ uint32_t part[4];
	if(blockIdx.x >= nblocks) return;
	const LodJob j = jobs[block_job[blockIdx.x]];
	const uint32_t k = blockIdx.x - j.fblock0;
	if(k >= lod_fblocks(j.nface)) return;
	LodGroupDev g; g.part = (WELD_LDS uint32_t *)part;
	lod_scatter_block(g, in_of(j), (WELD_MEM const uint32_t *)j.triples, (WELD_MEM const uint32_t *)j.blocks, (WELD_MEM uint32_t *)j.lod_index, k);
}

} // namespace corto_hip
