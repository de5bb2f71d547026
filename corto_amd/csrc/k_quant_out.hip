// k_quant_out.hip — K-QOUT: the finisher of a generic attribute bound with CRTHIP_BIND_QUANTIZED, for gfx950.  The attribute was decoded as int32
// into the batch's scratch (the path of a strided FLOAT binding); here its values leave as uint16 relative to the blob's per-component minimum
// and the blob's crthip_quant_transform is written (quant_out.h has the arithmetic and the partition, and says why no order can change a bit).
//
//   k_quant_out_blob   one workgroup of 256 lanes a job of up to QOUT_BLOB_MAX vertices: a lane folds its vertices into min / max in registers,
//                      the wave reduces them with DPP row operations, the four waves meet in 32 bytes of LDS (ds_min / ds_max); then the
//                      workgroup re-reads the values it has just pulled through L2 and stores.  Lane 0 writes the record(s), and on a span
//                      beyond 65535 the status in place of the values.
//   k_quant_range      jobs beyond that: a block of 1 024 vertices folded as above, merged into the job's eight scratch words with integer
//   k_quant_store      atomicMin / atomicMax; then every block reads the words and stores (or does not); a job's first block publishes.
// Packed outputs go out as aligned 16-byte vectors between a scalar head and tail, strided ones as the halfwords of one vertex a lane: no
// byte outside [buffer + i*stride, + 2*N) of a vertex is written.  No float atomics, no look-back, plain C++.
#include "kernels_common.h"
#include "kernels.h"
#include "quant_out.h"

namespace corto_hip {

namespace {

// the workgroup's range: every lane ends with it.  red: 8 words of LDS.  On qout_bias images, the minimum as the maximum of the complement,
// so that 0 - what a DPP row operation leaves in a lane it does not write - is the identity of both (wave_max_u32)
__device__ __forceinline__ void block_range(QuantRange &r, uint32_t N, uint32_t *red) {
	if(threadIdx.x < 8) red[threadIdx.x] = threadIdx.x < 4 ? 0xFFFFFFFFu : 0u;
	__syncthreads();
#pragma unroll
	for(uint32_t c = 0; c < 4; c++) {
		if(c < N) {                                                              // (uniform)
			const uint32_t mn = ~wave_max_u32(~qout_bias(r.mn[c])), mx = wave_max_u32(qout_bias(r.mx[c]));
			if(lane_id() == 0) { atomicMin(&red[c], mn); atomicMax(&red[4 + c], mx); }
		}
	}
	__syncthreads();
#pragma unroll
	for(uint32_t c = 0; c < 4; c++) { r.mn[c] = qout_unbias(red[c]); r.mx[c] = qout_unbias(red[4 + c]); }
}

// the record(s), and the status of a blob whose span does not fit (an earlier code stays): one lane
__device__ __forceinline__ void publish(const QuantOutJob &j, const crthip_quant_transform &t) {
	*(crthip_quant_transform *)j.rec_host = t;
	if(j.rec_dev) *(crthip_quant_transform *)j.rec_dev = t;
	if(!t.written && *j.status == CRTHIP_OK) *j.status = CRTHIP_E_FORMAT;
}

__device__ __forceinline__ QuantStore store_of(const QuantOutJob &j, const crthip_quant_transform &t) {
	QuantStore S;
	S.values = j.values; S.buffer = j.buffer; S.stride = j.stride; S.nvert = j.nvert; S.N = j.N;
#pragma unroll
	for(int c = 0; c < 4; c++) S.base[c] = t.base[c];
	return S;
}

} // namespace

__global__ __launch_bounds__(256) void k_quant_out_blob(const QuantOutJob *__restrict__ jobs, const uint32_t *__restrict__ job_ids, uint32_t njobs) {
	__shared__ uint32_t red[8];
	if(blockIdx.x >= njobs) return;
	const QuantOutJob j = jobs[job_ids[blockIdx.x]];
	QuantRange r;
	qout_fold_lane(r, j.values, j.N, 0, j.nvert, threadIdx.x);
	block_range(r, j.N, red);
	crthip_quant_transform t;
	const uint32_t written = qout_transform(r, j.N, j.q, t);
	if(threadIdx.x == 0) publish(j, t);
	if(!written) return;
	qout_store_lane(store_of(j, t), 0, ~0ull, 0, j.nvert, true, threadIdx.x);
}

__global__ __launch_bounds__(256) void k_quant_range(const QuantOutJob *__restrict__ jobs, const uint32_t *__restrict__ block_job, uint32_t nblocks) {
	__shared__ uint32_t red[8];
	if(blockIdx.x >= nblocks) return;
	const QuantOutJob j = jobs[block_job[blockIdx.x]];
	const uint64_t v0 = (uint64_t)(blockIdx.x - j.block0)*QOUT_BLOCK, v1 = v0 + QOUT_BLOCK < j.nvert ? v0 + QOUT_BLOCK : j.nvert;
	QuantRange r;
	qout_fold_lane(r, j.values, j.N, v0, v1, threadIdx.x);
	block_range(r, j.N, red);
#pragma unroll
	for(uint32_t c = 0; c < 4; c++)                                             // (lane c: component c; constant indices keep r in registers)
		if(threadIdx.x == c && c < j.N) { atomicMin(&j.range[c], qout_bias(r.mn[c])); atomicMax(&j.range[4 + c], qout_bias(r.mx[c])); }
}

__global__ __launch_bounds__(256) void k_quant_store(const QuantOutJob *__restrict__ jobs, const uint32_t *__restrict__ block_job, uint32_t nblocks) {
	if(blockIdx.x >= nblocks) return;
	const QuantOutJob j = jobs[block_job[blockIdx.x]];
	const uint32_t b = blockIdx.x - j.block0;
	QuantRangeWords w;
#pragma unroll
	for(int c = 0; c < 4; c++) { w.mn[c] = j.range[c]; w.mx[c] = j.range[4 + c]; }
	QuantRange r;
	qout_range_from_words(r, w);
	crthip_quant_transform t;
	const uint32_t written = qout_transform(r, j.N, j.q, t);
	if(b == 0 && threadIdx.x == 0) publish(j, t);
	if(!written) return;
	const uint64_t per = qout_groups_per_block(j.N), v0 = (uint64_t)b*QOUT_BLOCK;
	qout_store_lane(store_of(j, t), b*per, (b + 1)*per, v0, v0 + QOUT_BLOCK < j.nvert ? v0 + QOUT_BLOCK : j.nvert, b == 0, threadIdx.x);
}

} // namespace corto_hip
