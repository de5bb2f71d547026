// k_compact.hip — K-COMPACT: a level's own vertex buffers for gfx950 (crthip_batch_bind_compact).  compact.h has the method, the phases and both
// partitions; here are the workgroup (lod_group.h: k_lod.hip's) and the seven grids.  A job is one SET of one blob, so no kernel loops over sets.
// The mark, scan and renumber kernels are launched in stage M behind the clouds' levels of detail: every id list they read (the index, the welded
// index, a level's index) is final there.  k_compact_gather is launched behind k_quant_store, the last kernel that writes a final vertex byte.
//
//   k_compact_blob     one workgroup a set of up to 8 192 vertices and 8 192 bound faces, from an id list: the used set a bitmask in 1 KiB of LDS
//                      built with LDS atomic ORs, its words' popcounts through one block scan into a second KiB; then the newid / order stores,
//                      then the index through the two LDS arrays; thread 0 stores the record as one 16-byte word.  No global atomic.
//   k_compact_mark     bigger sets, 256 corners a workgroup through a block -> job map: an atomic OR a corner into the mask in scratch (zeroed by a
//                      FillJob in front)
//   k_compact_count    ... 256 vertices a workgroup through a second map: the popcount of the block's eight mask words to the block's word
//   k_compact_offsets  one workgroup a set: the exclusive scan of the block counts in rounds of 256 blocks, and the record
//   k_compact_place    ... 256 vertices a workgroup: the block scan of the block's bits, newid and order at the block's base
//   k_compact_index    ... 256 corners a workgroup: the renumbered index through newid
//   k_compact_gather   every set, both partitions and clouds: a thread a copy unit of a record through a third map; the count is read from
//                      the set's record (a cloud's: its level's), threads beyond min(used, vertex_capacity) leave
//                      No look-back, no spinning: the kernels' order on the stream is the only dependency.
// Plain C++: no inline assembly.
#define WELD_KERNELS                                                         // (weld.h: WELD_MEM / WELD_LDS are address spaces here)
#include "kernels_common.h"
#include "kernels.h"
#include "compact.h"
#include "lod_group.h"                                                       // (LodGroupDev: the workgroup as lod.h sees it)

namespace corto_hip {

namespace {

__device__ __forceinline__ CompactIn in_of(const CompactJob &j) {
	CompactIn J; J.w.position = nullptr; J.w.index = (WELD_MEM const void *)j.src; J.w.index_u16 = j.src_u16;
	J.w.nface = j.nface; J.w.nvert = j.nvert; J.src_rec = (WELD_MEM const uint32_t *)j.src_rec; J.vcap = j.vcap; J.icap = j.icap; J.clip_v = j.clip_v;
	return J;
}

} // namespace

__global__ __launch_bounds__(COMPACT_THREADS) void k_compact_blob(const CompactJob *__restrict__ jobs, const uint32_t *__restrict__ job_ids, uint32_t njobs) {
	__shared__ uint32_t mask[COMPACT_BLOB_WORDS], pre[COMPACT_BLOB_WORDS];
	__shared__ uint32_t part[4];
	if(blockIdx.x >= njobs) return;
	const CompactJob j = jobs[job_ids[blockIdx.x]];
	if(!compact_in_blob(j.nvert, j.nface)) return;                          // (the planner never lists such a set here: the LDS arrays end at 8 192 vertices)
	LodGroupDev g; g.part = (WELD_LDS uint32_t *)part; g.L = LodLane{0u, 0u, 0u, 0u, 0u, 0u};
	compact_blob(g, in_of(j), (WELD_LDS uint32_t *)mask, (WELD_LDS uint32_t *)pre, (WELD_MEM uint32_t *)j.newid, (WELD_MEM uint32_t *)j.order,
		(WELD_MEM uint32_t *)j.index, (WELD_MEM crthip_compact_counts *)j.counts);
}

__global__ __launch_bounds__(COMPACT_THREADS) void k_compact_mark(const CompactJob *__restrict__ jobs, const uint32_t *__restrict__ block_job, uint32_t nblocks) {
	if(blockIdx.x >= nblocks) return;
	const CompactJob j = jobs[block_job[blockIdx.x]];
	const uint32_t k = blockIdx.x - j.cblock0;
	if(k >= compact_cblocks(j.nface)) return;
	LodGroupDev g; g.part = nullptr;
	compact_mark_block(g, in_of(j), (WELD_MEM uint32_t *)j.mask, k);
}

__global__ __launch_bounds__(COMPACT_THREADS) void k_compact_count(const CompactJob *__restrict__ jobs, const uint32_t *__restrict__ block_job, uint32_t nblocks) {
	__shared__ uint32_t part[4];
	if(blockIdx.x >= nblocks) return;
	const CompactJob j = jobs[block_job[blockIdx.x]];
	const uint32_t k = blockIdx.x - j.vblock0;
	if(k >= compact_vblocks(j.nvert)) return;
	LodGroupDev g; g.part = (WELD_LDS uint32_t *)part;
	compact_count_block(g, j.nvert, (WELD_MEM const uint32_t *)j.mask, (WELD_MEM uint32_t *)j.blocks, k);
}

__global__ __launch_bounds__(COMPACT_THREADS) void k_compact_offsets(const CompactJob *__restrict__ jobs, const uint32_t *__restrict__ job_ids, uint32_t njobs) {
	__shared__ uint32_t part[4];
	if(blockIdx.x >= njobs) return;
	const CompactJob j = jobs[job_ids[blockIdx.x]];
	LodGroupDev g; g.part = (WELD_LDS uint32_t *)part;
	compact_offsets_job(g, in_of(j), j.index != nullptr, (WELD_MEM uint32_t *)j.blocks, (WELD_MEM crthip_compact_counts *)j.counts);
}

__global__ __launch_bounds__(COMPACT_THREADS) void k_compact_place(const CompactJob *__restrict__ jobs, const uint32_t *__restrict__ block_job, uint32_t nblocks) {
	__shared__ uint32_t part[4];
	if(blockIdx.x >= nblocks) return;
	const CompactJob j = jobs[block_job[blockIdx.x]];
	const uint32_t k = blockIdx.x - j.vblock0;
	if(k >= compact_vblocks(j.nvert)) return;
	LodGroupDev g; g.part = (WELD_LDS uint32_t *)part;
	compact_place_block(g, in_of(j), (WELD_MEM const uint32_t *)j.mask, (WELD_MEM const uint32_t *)j.blocks, (WELD_MEM uint32_t *)j.newid, (WELD_MEM uint32_t *)j.order, k);
}

__global__ __launch_bounds__(COMPACT_THREADS) void k_compact_index(const CompactJob *__restrict__ jobs, const uint32_t *__restrict__ block_job, uint32_t nblocks) {
	if(blockIdx.x >= nblocks) return;
	const CompactJob j = jobs[block_job[blockIdx.x]];
	const uint32_t k = blockIdx.x - j.cblock0;
	if(!j.index || !j.newid || k >= compact_cblocks(j.nface)) return;
	LodGroupDev g; g.part = nullptr;
	compact_index_block(g, in_of(j), (WELD_MEM const uint32_t *)j.newid, (WELD_MEM uint32_t *)j.index, k);
}

__global__ __launch_bounds__(COMPACT_THREADS) void k_compact_gather(const CompactGatherJob *__restrict__ jobs, const uint32_t *__restrict__ block_job, uint32_t nblocks) {
	if(blockIdx.x >= nblocks) return;
	const CompactGatherJob j = jobs[block_job[blockIdx.x]];
	const uint32_t k = blockIdx.x - j.block0;
	if(k >= compact_gather_blocks(j.nvert, j.vcap, j.E, j.unit)) return;
	CompactGatherIn J; J.src = (WELD_MEM const uint8_t *)j.src; J.dst = (WELD_MEM uint8_t *)j.dst; J.order = (WELD_MEM const uint32_t *)j.order;
	J.count_rec = (WELD_MEM const uint32_t *)j.count_rec; J.cloud_rec = (WELD_MEM crthip_compact_counts *)j.cloud_rec;
	J.E = j.E; J.sstride = j.sstride; J.dstride = j.dstride; J.unit = j.unit; J.vcap = j.vcap; J.nvert = j.nvert; J.clip_v = j.clip_v;
	LodGroupDev g; g.part = nullptr;
	compact_gather_block(g, J, k);
}

} // namespace corto_hip
