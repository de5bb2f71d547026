// k_meshlet.hip — K-MLT: meshlets from the decoded index for gfx950 (crthip_batch_bind_meshlets).  meshlet.h has the cut rule, the builder's
// step, the table and the placement rule; here are the wave (DPP scan, ballot, readlane) and the three grids.  Launched in stage M behind the
// normal and tangent kernels: the index is final.
//
//   k_meshlet_blob      one workgroup a blob of up to MESHLET_BLOB_SEGS segments, a wave a segment, sizeof(MltWaveMem) (5 760 bytes) of LDS a wave.
//                       A blob of ONE segment - a C4 unit at the default - has nothing in front of its meshlets: the wave writes the caller's
//                       arrays directly.  Otherwise the waves write the job's scratch, the workgroup meets at a barrier, every thread adds up
//                       the counts in front of each segment and the workgroup moves the pieces.  Thread 0 writes the record(s).
//   k_meshlet_segments  bigger blobs: a wave (a workgroup of 64) a segment through a block -> job map, into scratch, with a count a segment;
//   k_meshlet_place     then a workgroup a segment sums the counts of the segments in front of it, moves its pieces and adds the offsets; the
//                       last segment's workgroup writes the record(s).  No look-back, no spinning: the kernels' order on the stream is the
//                       only dependency.
// Stores are whole words (vertex ids, four local-id bytes) or a whole 16-byte record.  Plain C++: no inline assembly.
#define MLT_KERNELS                                                          // (meshlet.h: MLT_MEM / MLT_LDS are address spaces here)
#include "kernels_common.h"
#include "kernels.h"
#include "meshlet.h"

namespace corto_hip {

namespace {

// the wave as mlt_segment sees it: one lane a thread
struct MltWaveDev {
	MltLane L;
	uint32_t lane;
	__device__ __forceinline__ void window(const MltIn &J, uint32_t pos, uint32_t, uint32_t nwin) { L.in = lane < nwin; if(L.in) mlt_load_face(J, pos + lane, L.v); }
	template <class F> __device__ __forceinline__ void each(F f) { f(lane, L); }
	__device__ __forceinline__ void sync() {                                // the lanes of ONE wave: the LDS pipe keeps their order, the compiler must too
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
		__builtin_amdgcn_wave_barrier();
		__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
	}
	__device__ __forceinline__ void scan() { L.incl = wave_inclusive_scan_u32(L.cnt); }
	template <class P> __device__ __forceinline__ uint32_t first(P pred) {
		const uint64_t m = __ballot(pred(lane, L));
		return m ? (uint32_t)__builtin_ctzll(m) : 64u;
	}
	__device__ __forceinline__ uint32_t incl_of(uint32_t l) { return (uint32_t)__builtin_amdgcn_readlane((int)L.incl, (int)l); }
};

__device__ __forceinline__ MltIn in_of(const MeshletJob &j) {
	MltIn J; J.faces = (MLT_MEM const void *)j.faces; J.faces_u16 = j.faces_u16; J.max_vertices = j.max_vertices; J.max_triangles = j.max_triangles;
	return J;
}
__device__ __forceinline__ MltOut final_of(const MeshletJob &j) {
	return MltOut{(MLT_MEM crthip_meshlet *)j.meshlets, (MLT_MEM uint32_t *)j.vertices, (MLT_MEM uint32_t *)j.triangles};
}
__device__ __forceinline__ MltScratch scratch_of(const MeshletJob &j) {
	MLT_MEM uint8_t *s = (MLT_MEM uint8_t *)j.scratch;
	return MltScratch{(MLT_MEM crthip_meshlet *)s, (MLT_MEM uint32_t *)(s + j.sc_vertices), (MLT_MEM uint32_t *)(s + j.sc_triangles), (MLT_MEM MltCount *)(s + j.sc_counts)};
}
__device__ __forceinline__ MltSeg seg_of(const MeshletJob &j, uint32_t k) {
	const mlt_u32x4 r = ((MLT_MEM const mlt_u32x4 *)j.segs)[k];
	return MltSeg{r.x, r.y, r.z, r.w};
}
__device__ __forceinline__ MltCount count_at(MLT_MEM const MltCount *p) { const mlt_u32x4 r = *(MLT_MEM const mlt_u32x4 *)p; return MltCount{r.x, r.y, r.z, 0}; }
__device__ __forceinline__ void record(const MeshletJob &j, const MltCount &c) {
	const mlt_u32x4 r = {c.meshlets, c.vertices, c.triangle_bytes, j.nseg};
	*(MLT_MEM mlt_u32x4 *)j.rec_host = r;
	if(j.rec_dev) *(MLT_MEM mlt_u32x4 *)j.rec_dev = r;
}
// the wave's table starts out empty (serial 0 is nobody's)
__device__ __forceinline__ void clear_table(MLT_LDS MltWaveMem &W, uint32_t lane) {
	for(uint32_t i = lane; i < MLT_TAB; i += 64) W.tab[i] = 0;
}

} // namespace

__global__ __launch_bounds__(256) void k_meshlet_blob(const MeshletJob *__restrict__ jobs, const uint32_t *__restrict__ job_ids, uint32_t njobs) {
	extern __shared__ __attribute__((aligned(16))) uint8_t mlt_lds[];
	if(blockIdx.x >= njobs) return;
	const MeshletJob j = jobs[job_ids[blockIdx.x]];
	const uint32_t w = wave_id(), lane = lane_id();
	const MltIn J = in_of(j);
	const MltOut F = final_of(j);
	if(j.nseg <= 1) {                                                        // nothing in front of this segment: in place
		if(w != 0) return;
		MltCount c{0, 0, 0, 0};
		if(j.nseg) {
			MLT_LDS MltWaveMem &W = *(MLT_LDS MltWaveMem *)mlt_lds;
			clear_table(W, lane);
			MltWaveDev x; x.lane = lane;
			x.sync();
			c = mlt_segment(x, W, J, seg_of(j, 0), F);
		}
		if(lane == 0) record(j, c);
		return;
	}
	const MltScratch P = scratch_of(j);
	if(w < j.nseg) {                                                         // (the launch has a wave for every segment of every listed blob)
		MLT_LDS MltWaveMem &W = *((MLT_LDS MltWaveMem *)mlt_lds + w);
		clear_table(W, lane);
		MltWaveDev x; x.lane = lane;
		x.sync();
		const MltSeg sg = seg_of(j, w);
		const MltCount c = mlt_segment(x, W, J, sg, mlt_provisional(P, sg));
		if(lane == 0) *(MLT_MEM mlt_u32x4 *)&P.counts[w] = mlt_u32x4{c.meshlets, c.vertices, c.triangle_bytes, 0};
	}
	__syncthreads();                                                         // the waves' global stores, seen by the whole workgroup (one CU, one L1)
	MltCount before{0, 0, 0, 0};
	for(uint32_t k = 0; k < j.nseg; k++) {
		const MltCount own = count_at(&P.counts[k]);
		mlt_place(P, F, seg_of(j, k), before, own, threadIdx.x, blockDim.x);
		before = mlt_add(before, own);
	}
	if(threadIdx.x == 0) record(j, before);
}

__global__ __launch_bounds__(64) void k_meshlet_segments(const MeshletJob *__restrict__ jobs, const uint32_t *__restrict__ block_job, uint32_t nblocks) {
	__shared__ __attribute__((aligned(16))) MltWaveMem mem;
	if(blockIdx.x >= nblocks) return;
	const MeshletJob j = jobs[block_job[blockIdx.x]];
	const uint32_t k = blockIdx.x - j.block0, lane = lane_id();
	if(k >= j.nseg) return;
	const MltScratch P = scratch_of(j);
	MLT_LDS MltWaveMem &W = *(MLT_LDS MltWaveMem *)&mem;
	clear_table(W, lane);
	MltWaveDev x; x.lane = lane;
	x.sync();
	const MltSeg sg = seg_of(j, k);
	const MltCount c = mlt_segment(x, W, in_of(j), sg, mlt_provisional(P, sg));
	if(lane == 0) *(MLT_MEM mlt_u32x4 *)&P.counts[k] = mlt_u32x4{c.meshlets, c.vertices, c.triangle_bytes, 0};
}

__global__ __launch_bounds__(256) void k_meshlet_place(const MeshletJob *__restrict__ jobs, const uint32_t *__restrict__ block_job, uint32_t nblocks) {
	__shared__ uint32_t part[3][4];
	if(blockIdx.x >= nblocks) return;
	const MeshletJob j = jobs[block_job[blockIdx.x]];
	const uint32_t k = blockIdx.x - j.block0, tid = threadIdx.x;
	if(k >= j.nseg) return;
	const MltScratch P = scratch_of(j);
	uint32_t s[3] = {0, 0, 0};                                               // the counts in front of segment k, a share a thread
	for(uint32_t i = tid; i < k; i += MLT_PLACE_THREADS) { const MltCount c = count_at(&P.counts[i]); s[0] += c.meshlets; s[1] += c.vertices; s[2] += c.triangle_bytes; }
#pragma unroll
	for(uint32_t q = 0; q < 3; q++) {
		const uint32_t tot = (uint32_t)__builtin_amdgcn_readlane((int)wave_inclusive_scan_u32(s[q]), 63);
		if(lane_id() == 0) part[q][wave_id()] = tot;
	}
	__syncthreads();
	const MltCount before{part[0][0] + part[0][1] + part[0][2] + part[0][3], part[1][0] + part[1][1] + part[1][2] + part[1][3],
		part[2][0] + part[2][1] + part[2][2] + part[2][3], 0};
	const MltCount own = count_at(&P.counts[k]);
	mlt_place(P, final_of(j), seg_of(j, k), before, own, tid, MLT_PLACE_THREADS);
	if(k + 1 == j.nseg && tid == 0) record(j, mlt_add(before, own));
}

} // namespace corto_hip
