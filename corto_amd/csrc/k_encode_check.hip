// k_encode_check.hip — K-ENC-CHECK: what crthip_encode_batch_resident must know about the caller's DEVICE arrays before anything indexes
// with them or quantises them, for gfx950.  Every item of a batch in two launches, from a job table (enc_input_check.h has the
// arithmetic and says why the partition cannot change a bit of the result).
//
//   k_enc_input_check    workgroups by job kind (block_start / enc_job_of, as the batch's other kernels):
//                          RANGE  4 096 index entries a workgroup against nvert; atomicOr into the item's record
//                          BOX    1 024 vertices a workgroup -> one partial box: a lane takes 4 vertices in order, lanes merge in lane
//                                 order (shuffles: the lower lane is the earlier run), the four waves in wave order
//                          EDGE   one workgroup an item: 1 024 first-edge lengths at a time into LDS, lane 0 adds them to a double in face
//                                 order while the workgroup fills the other buffer
//   k_enc_input_reduce   one wave per BOX item: its partials folded in block order onto the host's seed -> the record
// Loads are 16 bytes wide where the caller's pointer allows: only element alignment is promised, so a lane's 48 bytes (an index
// group's 16: four uint32 entries or eight uint16) are reached through a scalar head and tail when the array starts off a 16-byte
// boundary; a strided position (crthip_mesh_layout) is one 16-byte load a vertex where base and stride are multiples of 16.  Nothing is read beyond
// nvert*3 floats / nface*3 entries, nothing is gathered through an entry >= nvert, and the caller's arrays are never written.
// No float atomics (k_encode_batch.hip's rule).
#include "kernels_common.h"
#include "kernels.h"
#include "enc_input_check.h"

namespace corto_hip {

namespace {

// 12 floats from p, whose first 16-byte boundary is HEAD floats on (p itself when HEAD == 0)
template <int HEAD> __device__ __forceinline__ void load12(const float *p, float v[12]) {
#pragma unroll
	for(int k = 0; k < HEAD; k++) v[k] = p[k];
	constexpr int NV = HEAD ? 2 : 3;
#pragma unroll
	for(int q = 0; q < NV; q++) {
		const float4 x = *(const float4 *)(p + HEAD + 4*q);
		v[HEAD + 4*q] = x.x; v[HEAD + 4*q + 1] = x.y; v[HEAD + 4*q + 2] = x.z; v[HEAD + 4*q + 3] = x.w;
	}
#pragma unroll
	for(int k = HEAD + 4*NV; k < 12; k++) v[k] = p[k];
}

__device__ __forceinline__ void wave_merge_in_lane_order(EncInputBox &b) {      // lane 0 ends with the wave's box
#pragma unroll
	for(int off = 1; off < 64; off <<= 1) {
		EncInputBox o;
#pragma unroll
		for(int k = 0; k < 3; k++) { o.mn[k] = __shfl_down(b.mn[k], off, 64); o.mx[k] = __shfl_down(b.mx[k], off, 64); }
		enc_in_box_merge(b, o);                                                  // (a lane without a partner gets its own box back: no change)
	}
}

// PER entries of T in one 16-byte load: 4 uint32 or 8 uint16
template <class T> __device__ __forceinline__ uint32_t group_bad(const T *p, uint32_t nvert);
template <> __device__ __forceinline__ uint32_t group_bad<uint32_t>(const uint32_t *p, uint32_t nvert) {
	const uint4 x = *(const uint4 *)p;
	return (x.x >= nvert) | (x.y >= nvert) | (x.z >= nvert) | (x.w >= nvert);
}
template <> __device__ __forceinline__ uint32_t group_bad<uint16_t>(const uint16_t *p, uint32_t nvert) {
	const uint4 x = *(const uint4 *)p;
	const uint32_t w[4] = {x.x, x.y, x.z, x.w};
	uint32_t bad = 0;
#pragma unroll
	for(int k = 0; k < 4; k++) bad |= ((w[k] & 0xFFFFu) >= nvert) | ((w[k] >> 16) >= nvert);
	return bad;
}

template <class T> __device__ __forceinline__ void range_blocks(const EncInputJob &J, uint32_t b) {
	const uint64_t n = (uint64_t)J.nface*3;
	const T *ix = (const T *)J.index;
	uint32_t per; uint64_t head, groups, tail;
	enc_in_range_cut(J, n, per, head, groups, tail);                             // (per == 16/sizeof(T): head and tail are below it)
	uint32_t bad = 0;
	for(uint32_t p = 0; p < EIN_INDEX_TILE/4/EIN_THREADS; p++) {                  // (uint16: the same trip count covers a tile's entries twice over)
		const uint64_t g = (uint64_t)b*(EIN_INDEX_TILE/4) + p*EIN_THREADS + threadIdx.x;
		if(g < groups) bad |= group_bad<T>(ix + head + g*per, J.nvert);
	}
	if(b == 0) {                                                                 // the entries before and behind the 16-byte groups
		if(threadIdx.x < head) bad |= ix[threadIdx.x] >= J.nvert;
		if(threadIdx.x >= 64 && threadIdx.x - 64 < tail) bad |= ix[head + groups*per + (threadIdx.x - 64)] >= J.nvert;
	}
	if(bad) atomicOr(&J.rec->bad_index, 1u);
}

__device__ __forceinline__ void box_block(const EncInputJob &J, uint32_t b, EncInputBox *waves) {
	const uint64_t v0 = (uint64_t)b*EIN_TILE + (uint64_t)threadIdx.x*EIN_RUN;
	const float *p = J.position + v0*3;
	float v[12];
	uint32_t count = 0;
	if(J.pos_stride != 12) {
		// a strided array: a vertex's record, one 16-byte load where base and stride keep every record on a boundary - but never the
		// array's last vertex, whose record may end with its position (the checked extent does) - else three words
		const bool wide = (((uintptr_t)J.position | J.pos_stride) & 15u) == 0;
		count = v0 + EIN_RUN <= J.nvert ? EIN_RUN : v0 < J.nvert ? (uint32_t)(J.nvert - v0) : 0u;
#pragma unroll
		for(uint32_t r = 0; r < EIN_RUN; r++) {
			if(r < count) {
				const float *q = enc_in_vertex(J, v0 + r);
				if(wide && v0 + r + 1 < J.nvert) { const float4 x = *(const float4 *)q; v[3*r] = x.x; v[3*r + 1] = x.y; v[3*r + 2] = x.z; }
				else { v[3*r] = q[0]; v[3*r + 1] = q[1]; v[3*r + 2] = q[2]; }
			} else v[3*r] = v[3*r + 1] = v[3*r + 2] = 0.0f;
		}
	} else if(v0 + EIN_RUN <= J.nvert) {
		count = EIN_RUN;
		switch((uint32_t)(((uintptr_t)J.position >> 2) & 3u)) {                  // (a lane's 48 bytes keep the array's offset from a boundary)
		case 0: load12<0>(p, v); break;
		case 1: load12<3>(p, v); break;
		case 2: load12<2>(p, v); break;
		default: load12<1>(p, v); break;
		}
	} else {
		count = v0 < J.nvert ? (uint32_t)(J.nvert - v0) : 0u;
#pragma unroll
		for(int k = 0; k < 12; k++) v[k] = (uint32_t)k < count*3 ? p[k] : 0.0f;
	}
	if(J.has_origin) {
#pragma unroll
		for(int r = 0; r < (int)EIN_RUN; r++) enc_in_box_value(J, v + 3*r, v + 3*r);
	}
	EncInputBox box;
	enc_in_box_run(box, v, count);
	wave_merge_in_lane_order(box);
	if(lane_id() == 0) waves[wave_id()] = box;
	__syncthreads();
	if(threadIdx.x == 0) {
		for(uint32_t w = 1; w < EIN_THREADS/64; w++) enc_in_box_merge(box, waves[w]);
		J.partials[b] = box;
	}
}

__device__ __forceinline__ void edge_block(const EncInputJob &J, float (*terms)[EIN_EDGE_TILE]) {
	const uint32_t ntiles = (J.nface + EIN_EDGE_TILE - 1)/EIN_EDGE_TILE;
	uint32_t bad = 0;
	double sum = 0;
	auto fill = [&](uint32_t t) {
		const uint32_t first = t*EIN_EDGE_TILE, cnt = min(EIN_EDGE_TILE, J.nface - first);
		for(uint32_t i = threadIdx.x; i < cnt; i += EIN_THREADS) terms[t & 1][i] = enc_in_edge_term(J, first + i, bad);
	};
	if(ntiles) fill(0);
	__syncthreads();
	for(uint32_t t = 0; t < ntiles; t++) {
		if(t + 1 < ntiles) fill(t + 1);
		if(threadIdx.x == 0) {
			const uint32_t cnt = min(EIN_EDGE_TILE, J.nface - t*EIN_EDGE_TILE);
			const float *x = terms[t & 1];
			uint32_t i = 0;
#pragma unroll 4
			for(; i + 4 <= cnt; i += 4) {                                          // (four LDS words a read, reads ahead of the adds; the adds stay in order)
				const float4 q = *(const float4 *)(x + i);
				sum += (double)q.x; sum += (double)q.y; sum += (double)q.z; sum += (double)q.w;
			}
			for(; i < cnt; i++) sum += (double)x[i];
		}
		__syncthreads();
	}
	if(bad) atomicOr(&J.rec->bad_index, 1u);
	if(threadIdx.x == 0) J.rec->sum = sum;
}

} // namespace

__global__ __launch_bounds__(256) void k_enc_input_check(const EncInputJob *__restrict__ jobs, const uint32_t *__restrict__ block_start, uint32_t njobs) {
	__shared__ __attribute__((aligned(16))) float terms[2][EIN_EDGE_TILE];
	__shared__ EncInputBox waves[EIN_THREADS/64];
	const uint32_t j = enc_job_of(block_start, njobs, blockIdx.x);
	const EncInputJob J = jobs[j];
	const uint32_t b = blockIdx.x - block_start[j];
	if(J.kind == EIN_JOB_RANGE) { if(J.index16) range_blocks<uint16_t>(J, b); else range_blocks<uint32_t>(J, b); }
	else if(J.kind == EIN_JOB_BOX) box_block(J, b, waves);
	else edge_block(J, terms);
}

// jobs: the BOX jobs alone, one wave each
__global__ __launch_bounds__(64) void k_enc_input_reduce(const EncInputJob *__restrict__ jobs, const uint32_t *__restrict__ ids, uint32_t nids) {
	if(blockIdx.x >= nids) return;
	const EncInputJob J = jobs[ids[blockIdx.x]];
	const uint32_t nparts = (J.nvert + EIN_TILE - 1)/EIN_TILE;
	EncInputBox box;
	enc_in_fold_stretch(box, J.partials, nparts, threadIdx.x);
	wave_merge_in_lane_order(box);
	if(threadIdx.x == 0) {
		EncInputBox seed;
		enc_in_box_seed(seed, J.recipe, J.position);                             // (a BOX job has nvert > 0)
		enc_in_box_merge(seed, box);
		J.rec->box = seed;
	}
}

} // namespace corto_hip
