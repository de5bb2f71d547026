// k_bvh_query.hip — K-QUERY: exact box queries against a blob's BVH for gfx950 (crthip_bvh_query).  bvh_query.h has the face rules, the node
// test and the walk with its bounds; here are the workgroup and the grid.  Launched by the call itself on the context's main stream
// (bvh_query.cpp), never by a decode.
//
//   k_bvh_query  one thread a box, one wave of 64 a workgroup, through a block_start table over the call's sets (k_bvh_cast's shape: the set
//                of workgroup b is the last j with block_start[j] <= b).  The traversal stack is the cast's [65][64] words of static LDS,
//                depth-major: 16 640 bytes, free of bank conflicts, never scratch memory.  A box is two 16-byte loads, a node two, a result
//                record ONE 16-byte store; a matching face is one plain 4-byte store into the thread's own slice of `faces`, at most
//                face_capacity of them; the set's transform record, where one is given, is read by every thread.  Every loop is bounded by
//                the set's node count and every id is compared before it is an address: any bytes in the nodes end the thread with
//                CRTHIP_QUERY_TREE.  The block shape and the stack's place are CHOSEN, NOT TUNED (bvh_query.h).
// Plain C++: no inline assembly.
#define WELD_KERNELS                                                         // (weld.h: WELD_MEM / WELD_LDS are address spaces here)
#include "kernels_common.h"
#include "kernels.h"
#include "bvh_query.h"

namespace corto_hip {

__global__ __launch_bounds__(CAST_THREADS) void k_bvh_query(const QueryJob *__restrict__ jobs, const uint32_t *__restrict__ block_start, uint32_t njobs) {
	__shared__ uint32_t stack[CAST_LDS_WORDS];
	if(!njobs) return;
	const uint32_t j = enc_job_of(block_start, njobs, blockIdx.x);
	const QueryJob job = jobs[j];
	const uint64_t i = (uint64_t)(blockIdx.x - block_start[j])*CAST_THREADS + threadIdx.x;
	if(i >= job.nbox) return;
	CastIn J;
	J.nodes = (WELD_MEM const uint8_t *)job.nodes; J.position = (WELD_MEM const uint8_t *)job.position; J.index = (WELD_MEM const void *)job.index;
	J.base[0] = job.base[0]; J.base[1] = job.base[1]; J.base[2] = job.base[2];
	J.stride = job.pos_stride; J.nvert = job.nvert; J.nface = job.nface; J.index_u16 = job.index_u16; J.flags = job.flags;
	QueryNoCount count;
	query_box(J, (WELD_MEM const uint8_t *)job.transform, (WELD_MEM const uint8_t *)job.boxes, (WELD_MEM uint8_t *)job.results, (WELD_MEM uint32_t *)job.faces,
		job.face_capacity, CastStack{(WELD_LDS uint32_t *)stack, threadIdx.x}, (uint32_t)i, count);
}

} // namespace corto_hip
