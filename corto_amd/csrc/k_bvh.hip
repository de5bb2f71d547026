// k_bvh.hip — K-BVH: a binary triangle BVH of the integer positions and the index for gfx950 (crthip_batch_bind_bvh).  bvh.h has the boxes, the
// keys, the sort steps, the split search, the refit step and both partitions; here are the workgroup (lod_group.h: k_lod.hip's) and the eight
// grids.  Launched in stage M behind the kernels that make the index final and in front of k_dequant, which turns the positions into floats.
//
//   k_bvh_blob          one workgroup a blob of up to 4 096 faces, from an id list: 32 + 20 bytes a face of dynamic LDS (the launch asks for
//                       the largest among them).  The extent with LDS atomics, the keys, 30 (with absent faces 31) stable splits of the whole
//                       blob, ids in 16 bits, a thread an internal node, a thread a leaf; the arrival counters in LDS, acquire-release at
//                       workgroup scope; nodes and the record as 16-byte stores.  No global atomic.
//   k_bvh_boxes         bigger blobs, 256 faces a workgroup through a block -> job map: the extent in LDS, then seven atomics a workgroup into
//                       the blob's words in scratch (zeroed, with the arrival counters, by ONE FillJob in front)
//   k_bvh_keys          ... a thread a face: the key and the face id
//   k_bvh_sort_count    ... a tile of 2 048 pairs a workgroup through a second map, four passes of 8 bits: the tile's digit histogram
//   k_bvh_sort_offsets  one workgroup a blob from an id list: the exclusive scan of the digit-major table
//   k_bvh_sort_scatter  ... a tile a workgroup: eight stable splits in 33 KiB of LDS, then every pair to its digit's place
//   k_bvh_tree          ... a thread an internal node: the child words of the caller's nodes, the parent words, the order
//   k_bvh_refit         ... a thread a leaf: the climb of bvh.h, ONE acquire-release atomic add at agent scope an arrival: the order of that atomic
//                       releases the first arrival's node and acquires it for the second, which reads the sibling's box behind it (L1 is per
//                       CU and L2 per XCD: a plain flag behind a fence would not do).  The first arrival returns: nobody polls.
//                       No look-back, no spinning: beyond the arrival, the kernels' order on the stream is the only dependency.
// Plain C++: no inline assembly.
#define WELD_KERNELS                                                         // (weld.h: WELD_MEM / WELD_LDS are address spaces here)
#include "kernels_common.h"
#include "kernels.h"
#include "bvh.h"
#include "lod_group.h"                                                       // (LodGroupDev: the workgroup as lod.h sees it)

namespace corto_hip {

namespace {

__device__ __forceinline__ WeldIn in_of(const BvhJob &j) {
	WeldIn J; J.position = (WELD_MEM const int32_t *)j.position; J.index = (WELD_MEM const void *)j.index; J.index_u16 = j.index_u16; J.nface = j.nface; J.nvert = j.nvert;
	return J;
}
__device__ __forceinline__ BvhBig big_of(const BvhJob &j) { return bvh_big_carve((WELD_MEM uint8_t *)j.scratch, j.nface); }

} // namespace

__global__ __launch_bounds__(BVH_THREADS) void k_bvh_blob(const BvhJob *__restrict__ jobs, const uint32_t *__restrict__ job_ids, uint32_t njobs) {
	extern __shared__ __attribute__((aligned(16))) uint8_t bvh_lds[];
	__shared__ uint32_t part[4];
	if(blockIdx.x >= njobs) return;
	const BvhJob j = jobs[job_ids[blockIdx.x]];
	if(!j.nface || !bvh_in_blob(j.nface)) return;                          // (the planner never lists such a blob here: the LDS arrays and the 16-bit ids end at 4 096 faces)
	LodGroupDev g; g.part = (WELD_LDS uint32_t *)part; g.L = LodLane{0u, 0u, 0u, 0u, 0u, 0u};
	bvh_blob(g, in_of(j), (WELD_LDS uint8_t *)bvh_lds, (WELD_MEM crthip_bvh_node *)j.nodes, (WELD_MEM uint32_t *)j.parent, (WELD_MEM uint32_t *)j.order,
		(WELD_MEM crthip_bvh_counts *)j.counts);
}

__global__ __launch_bounds__(BVH_THREADS) void k_bvh_boxes(const BvhJob *__restrict__ jobs, const uint32_t *__restrict__ block_job, uint32_t nblocks) {
	__shared__ uint32_t lext[BVH_EXT_WORDS];
	if(blockIdx.x >= nblocks) return;
	const BvhJob j = jobs[block_job[blockIdx.x]];
	const uint32_t k = blockIdx.x - j.fblock0;
	if(k >= bvh_fblocks(j.nface)) return;
	LodGroupDev g; g.part = nullptr;
	bvh_boxes_block(g, in_of(j), big_of(j), (WELD_LDS uint32_t *)lext, k);
}

__global__ __launch_bounds__(BVH_THREADS) void k_bvh_keys(const BvhJob *__restrict__ jobs, const uint32_t *__restrict__ block_job, uint32_t nblocks) {
	if(blockIdx.x >= nblocks) return;
	const BvhJob j = jobs[block_job[blockIdx.x]];
	const uint32_t k = blockIdx.x - j.fblock0;
	if(k >= bvh_fblocks(j.nface)) return;
	LodGroupDev g; g.part = nullptr;
	bvh_keys_block(g, in_of(j), big_of(j), k);
}

__global__ __launch_bounds__(BVH_THREADS) void k_bvh_sort_count(const BvhJob *__restrict__ jobs, const uint32_t *__restrict__ block_job, uint32_t nblocks, uint32_t pass) {
	__shared__ uint32_t lh[BVH_DIGITS];
	if(blockIdx.x >= nblocks) return;
	const BvhJob j = jobs[block_job[blockIdx.x]];
	const uint32_t k = blockIdx.x - j.tblock0;
	if(k >= bvh_tiles(j.nface) || pass >= BVH_PASSES) return;
	LodGroupDev g; g.part = nullptr;
	bvh_sort_count_tile(g, j.nface, big_of(j), (WELD_LDS uint32_t *)lh, pass, k);
}

__global__ __launch_bounds__(BVH_THREADS) void k_bvh_sort_offsets(const BvhJob *__restrict__ jobs, const uint32_t *__restrict__ job_ids, uint32_t njobs) {
	__shared__ uint32_t part[4];
	if(blockIdx.x >= njobs) return;
	const BvhJob j = jobs[job_ids[blockIdx.x]];
	LodGroupDev g; g.part = (WELD_LDS uint32_t *)part;
	bvh_sort_offsets_job(g, j.nface, big_of(j));
}

__global__ __launch_bounds__(BVH_THREADS) void k_bvh_sort_scatter(const BvhJob *__restrict__ jobs, const uint32_t *__restrict__ block_job, uint32_t nblocks, uint32_t pass) {
	__shared__ __attribute__((aligned(16))) uint8_t lds[BVH_TILE_LDS];
	__shared__ uint32_t part[4];
	if(blockIdx.x >= nblocks) return;
	const BvhJob j = jobs[block_job[blockIdx.x]];
	const uint32_t k = blockIdx.x - j.tblock0;
	if(k >= bvh_tiles(j.nface) || pass >= BVH_PASSES) return;
	LodGroupDev g; g.part = (WELD_LDS uint32_t *)part;
	bvh_sort_scatter_tile(g, j.nface, big_of(j), (WELD_LDS uint8_t *)lds, pass, k);
}

__global__ __launch_bounds__(BVH_THREADS) void k_bvh_tree(const BvhJob *__restrict__ jobs, const uint32_t *__restrict__ block_job, uint32_t nblocks) {
	if(blockIdx.x >= nblocks) return;
	const BvhJob j = jobs[block_job[blockIdx.x]];
	const uint32_t k = blockIdx.x - j.fblock0;
	if(k >= bvh_fblocks(j.nface)) return;
	LodGroupDev g; g.part = nullptr;
	bvh_tree_block(g, j.nface, big_of(j), (WELD_MEM crthip_bvh_node *)j.nodes, (WELD_MEM uint32_t *)j.parent, (WELD_MEM uint32_t *)j.order, k);
}

__global__ __launch_bounds__(BVH_THREADS) void k_bvh_refit(const BvhJob *__restrict__ jobs, const uint32_t *__restrict__ block_job, uint32_t nblocks) {
	if(blockIdx.x >= nblocks) return;
	const BvhJob j = jobs[block_job[blockIdx.x]];
	const uint32_t k = blockIdx.x - j.fblock0;
	if(k >= bvh_fblocks(j.nface)) return;
	LodGroupDev g; g.part = nullptr;
	bvh_refit_block(g, in_of(j), big_of(j), (WELD_MEM crthip_bvh_node *)j.nodes, (WELD_MEM const uint32_t *)j.parent, (WELD_MEM crthip_bvh_counts *)j.counts, k);
}

} // namespace corto_hip
