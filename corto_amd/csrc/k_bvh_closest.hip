// k_bvh_closest.hip — K-CLOSEST: exact closest-face queries against a blob's BVH for gfx950 (crthip_bvh_closest).  bvh_closest.h has the wide
// arithmetic, the face rule, the node prune and the walk with its bounds; here are the workgroup and the grid.  Launched by the call itself on
// the context's main stream (bvh_closest.cpp), never by a decode.
//
//   k_bvh_closest  one thread a point, one wave of 64 a workgroup, through a block_start table over the call's sets (k_bvh_cast's shape: the
//                  set of workgroup b is the last j with block_start[j] <= b).  The traversal stack is the cast's [65][64] words of static
//                  LDS, depth-major: 16 640 bytes, free of bank conflicts, never scratch memory.  A point is ONE 16-byte load, a node two
//                  (and two more for each child of an internal node, whose gaps order the pushes), a hit record three 16-byte stores; the
//                  set's transform record, where one is given, is read by every thread.  Every loop is bounded by the set's node count and
//                  every id is compared before it is an address: any bytes in the nodes end the thread with CRTHIP_CLOSEST_TREE.  The block
//                  shape and the stack's place are CHOSEN, NOT TUNED (bvh_closest.h), and so is the wide arithmetic.
// Plain C++: no inline assembly.
#define WELD_KERNELS                                                         // (weld.h: WELD_MEM / WELD_LDS are address spaces here)
#include "kernels_common.h"
#include "kernels.h"
#include "bvh_closest.h"

namespace corto_hip {

__global__ __launch_bounds__(CAST_THREADS) void k_bvh_closest(const ClosestJob *__restrict__ jobs, const uint32_t *__restrict__ block_start, uint32_t njobs) {
	__shared__ uint32_t stack[CAST_LDS_WORDS];
	if(!njobs) return;
	const uint32_t j = enc_job_of(block_start, njobs, blockIdx.x);
	const ClosestJob job = jobs[j];
	const uint64_t i = (uint64_t)(blockIdx.x - block_start[j])*CAST_THREADS + threadIdx.x;
	if(i >= job.npoint) return;
	CastIn J;
	J.nodes = (WELD_MEM const uint8_t *)job.nodes; J.position = (WELD_MEM const uint8_t *)job.position; J.index = (WELD_MEM const void *)job.index;
	J.base[0] = job.base[0]; J.base[1] = job.base[1]; J.base[2] = job.base[2];
	J.stride = job.pos_stride; J.nvert = job.nvert; J.nface = job.nface; J.index_u16 = job.index_u16; J.flags = job.flags;
	ClosestNoCount count;
	closest_point<true>(J, (WELD_MEM const uint8_t *)job.transform, (WELD_MEM const uint8_t *)job.points, (WELD_MEM uint8_t *)job.hits,
		CastStack{(WELD_LDS uint32_t *)stack, threadIdx.x}, (uint32_t)i, count);
}

} // namespace corto_hip
