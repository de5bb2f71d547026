// k_encode_batch.hip — the per-vertex stages of crthip_encode_batch for gfx950: every mesh of a batch in one set of launches (each point cloud's sort in launches of its own).
//
//   K-ENC-Q      k_enc_quantize_batch   quantisation of every attribute of every mesh, from a job table (k_enc_quantize's recipes; a job with
//                                       a stride, an origin or int16 normals reads the caller's array where it lies: enc_quant.h)
//   K-ENC-EST    k_enc_corners          corners keyed by vertex for the incidence sort; BORDER's neighbour XORs (integer atomics)
//                k_enc_est_normal       NormalAttr::preDelta (src/normal_attribute.cpp:113-143): the face normals of a vertex summed in
//                                       INCREASING FACE ORDER - the corners were sorted stably by vertex, so a vertex's run of the sorted
//                                       corners lists its faces in the order the host adds them - then the octahedral estimate subtracted
//   K-ENC-DELTA  k_enc_delta            the residuals over the prediction quads; BORDER's compaction is a scan in encode order
//   K-ENC-Z      k_enc_zmin / zkeys     63-bit Morton keys of a point cloud (include/corto/zpoint.h:34-38)
//                k_enc_rs_*             LSD radix sort, 8-bit digits, stable (a wave's equal digits ranked by ballots)
//                k_enc_zflag            adjacent equal keys: std::sort leaves those in an order no stable sort reproduces, so the host sorts
//                                       that cloud again; otherwise the quads of the sorted order
// Float arithmetic is the host's operation for operation (the library is built with -ffp-contract=off).  No float atomics anywhere.
#include "kernels_common.h"
#include "kernels.h"
#include "enc_quant.h"

namespace corto_hip {

__global__ __launch_bounds__(256) void k_enc_gather(const CopyJob *__restrict__ jobs, uint32_t njobs) {
	if(blockIdx.x >= njobs) return;
	const CopyJob J = jobs[blockIdx.x];
	if((((uintptr_t)J.src | (uintptr_t)J.dst | J.bytes) & 3u) == 0) {
		const uint32_t *s = (const uint32_t *)J.src; uint32_t *d = (uint32_t *)J.dst;
		for(uint64_t i = threadIdx.x; i < J.bytes/4; i += 256) d[i] = s[i];
	} else for(uint64_t i = threadIdx.x; i < J.bytes; i += 256) J.dst[i] = J.src[i];
}

__global__ __launch_bounds__(256) void k_enc_quantize_batch(const QuantJob *__restrict__ jobs, const uint32_t *__restrict__ block_start, uint32_t njobs) {
	const uint32_t j = enc_job_of(block_start, njobs, blockIdx.x);
	const QuantJob &J = jobs[j];
	const uint32_t i = (blockIdx.x - block_start[j])*256 + threadIdx.x;
	if(i >= J.count) return;
	enc_quantize_one(J, i);
}

// one thread per face: its three corners (key: the vertex in the batch's numbering, payload: the face) and, for BORDER, the XORs
__global__ __launch_bounds__(256) void k_enc_corners(const EstJob *__restrict__ jobs, const uint32_t *__restrict__ block_start, uint32_t njobs,
                                                      uint32_t *__restrict__ keys, uint32_t *__restrict__ vals) {
	const uint32_t j = enc_job_of(block_start, njobs, blockIdx.x);
	const EstJob &J = jobs[j];
	const uint32_t f = (blockIdx.x - block_start[j])*256 + threadIdx.x;
	if(f >= J.nface) return;
	const uint32_t v[3] = {J.faces[(size_t)f*3], J.faces[(size_t)f*3 + 1], J.faces[(size_t)f*3 + 2]};
	for(int k = 0; k < 3; k++) {
		const size_t c = (size_t)J.cbase + (size_t)f*3 + k;
		keys[c] = J.vbase + v[k];
		vals[c] = J.fbase + f;
	}
	if(J.boundary) for(int k = 0; k < 3; k++) {
		atomicXor(&J.boundary[v[k]], (int32_t)v[(k + 1)%3]);
		atomicXor(&J.boundary[v[k]], (int32_t)v[(k + 2)%3]);
	}
}

// one thread per vertex: its faces' cross products summed in face order, then values -= toOcta(estimate)
__global__ __launch_bounds__(256) void k_enc_est_normal(const EstJob *__restrict__ jobs, const uint32_t *__restrict__ block_start, uint32_t njobs,
                                                         const uint32_t *__restrict__ keys, const uint32_t *__restrict__ vals, uint32_t ncorners,
                                                         const uint32_t *__restrict__ faces) {
	const uint32_t j = enc_job_of(block_start, njobs, blockIdx.x);
	const EstJob &J = jobs[j];
	const uint32_t v = (blockIdx.x - block_start[j])*256 + threadIdx.x;
	if(v >= J.nvert) return;
	const uint32_t key = J.vbase + v;
	uint32_t lo = J.cbase, hi = J.cbase + 3*J.nface;         // the mesh's corners: lower_bound of the key among them
	while(lo < hi) { const uint32_t mid = (lo + hi) >> 1; if(keys[mid] < key) lo = mid + 1; else hi = mid; }
	float est[3] = {0.f, 0.f, 0.f};
	for(uint32_t c = lo; c < ncorners && keys[c] == key; c++) {
		const uint32_t *F = faces + (size_t)vals[c]*3;
		const int32_t *p0 = J.coords + (size_t)F[0]*3, *p1 = J.coords + (size_t)F[1]*3, *p2 = J.coords + (size_t)F[2]*3;
		const float ax = (float)p1[0] - (float)p0[0], ay = (float)p1[1] - (float)p0[1], az = (float)p1[2] - (float)p0[2];
		const float bx = (float)p2[0] - (float)p0[0], by = (float)p2[1] - (float)p0[1], bz = (float)p2[2] - (float)p0[2];
		const float n0 = ay*bz - az*by, n1 = az*bx - ax*bz, n2 = ax*by - ay*bx;
		est[0] += n0; est[1] += n1; est[2] += n2;
	}
	int32_t o[2];
	enc_to_octa(est[0], est[1], est[2], J.unit, o);
	int32_t *nv = J.normals + (size_t)v*2;
	nv[0] = (int32_t)((uint32_t)nv[0] - (uint32_t)o[0]);
	nv[1] = (int32_t)((uint32_t)nv[1] - (uint32_t)o[1]);
}

__global__ __launch_bounds__(256) void k_enc_delta(const DeltaEncJob *__restrict__ jobs, const uint32_t *__restrict__ block_start, uint32_t njobs) {
	const uint32_t j = enc_job_of(block_start, njobs, blockIdx.x);
	const DeltaEncJob &J = jobs[j];
	const uint32_t N = J.N;
	if(J.kind == DENC_NRM_BORDER) {                          // one workgroup: the boundary vertices in encode order, compacted
		__shared__ uint32_t scan[4];
		const int32_t *val = (const int32_t *)J.values;
		int32_t *out = (int32_t *)J.out;
		uint32_t w = 0;
		for(uint32_t base = 0; base < J.count; base += 256) {
			const uint32_t i = base + threadIdx.x;
			uint32_t t = 0, keep = 0;
			if(i < J.count) { t = J.quads[(size_t)i*4]; keep = J.boundary[t] != 0; }
			uint32_t total;
			const uint32_t at = w + block256_exclusive_scan<uint32_t>(keep, scan, &total);
			if(keep) { out[(size_t)at*2] = val[(size_t)t*2]; out[(size_t)at*2 + 1] = val[(size_t)t*2 + 1]; }
			w += total;
		}
		if(threadIdx.x == 0) *J.out_count = w;
		return;
	}
	const uint32_t first = (blockIdx.x - block_start[j])*DENC_BLOCK;
	for(uint32_t i = first + threadIdx.x; i < J.count && i < first + DENC_BLOCK; i += 256) {
		const uint32_t *q = J.quads + (size_t)i*4;
		const uint32_t t = q[0], a = q[1], b = q[2], c = q[3];
		if(J.kind == DENC_U8) {
			const uint8_t *val = (const uint8_t *)J.values; uint8_t *out = (uint8_t *)J.out;
			for(uint32_t k = 0; k < N; k++) {
				uint8_t d;
				if(i == 0) d = val[(size_t)t*N + k];
				else if(a != b && J.parallel) d = (uint8_t)(val[(size_t)t*N + k] - (val[(size_t)a*N + k] + val[(size_t)b*N + k] - val[(size_t)c*N + k]));
				else d = (uint8_t)(val[(size_t)t*N + k] - val[(size_t)a*N + k]);
				out[(size_t)i*N + k] = d;
			}
		} else if(J.kind == DENC_I32) {
			const uint32_t *val = (const uint32_t *)J.values; uint32_t *out = (uint32_t *)J.out;
			for(uint32_t k = 0; k < N; k++) {
				uint32_t d;
				if(i == 0) d = val[(size_t)t*N + k];
				else if(a != b && J.parallel) d = val[(size_t)t*N + k] - (val[(size_t)a*N + k] + val[(size_t)b*N + k] - val[(size_t)c*N + k]);
				else d = val[(size_t)t*N + k] - val[(size_t)a*N + k];
				out[(size_t)i*N + k] = d;
			}
		} else {                                              // normals: DIFF against q.a, ESTIMATED the values themselves
			const uint32_t *val = (const uint32_t *)J.values; uint32_t *out = (uint32_t *)J.out;
			for(uint32_t k = 0; k < 2; k++)
				out[(size_t)i*2 + k] = J.kind == DENC_NRM_DIFF && i > 0 ? val[(size_t)t*2 + k] - val[(size_t)a*2 + k] : val[(size_t)t*2 + k];
		}
	}
}

// ---- K-ENC-Z ----
__global__ __launch_bounds__(256) void k_enc_zmin(ZJob J) {
	const uint32_t i = blockIdx.x*256 + threadIdx.x;
	int32_t m[3] = {0, 0, 0};
	if(i < J.n) for(int k = 0; k < 3; k++) m[k] = min(0, J.coords[(size_t)i*3 + k]);
	for(int k = 0; k < 3; k++) {
		int32_t x = m[k];
		for(int d = 32; d >= 1; d >>= 1) x = min(x, __shfl_xor(x, d));
		if(lane_id() == 0 && x < 0) atomicMin(&J.mn[k], x);
	}
}

__global__ __launch_bounds__(256) void k_enc_zkeys(ZJob J) {
	const uint32_t i = blockIdx.x*256 + threadIdx.x;
	if(i >= J.n) return;
	const uint64_t x = (uint64_t)(int64_t)(J.coords[(size_t)i*3] - J.mn[0]), y = (uint64_t)(int64_t)(J.coords[(size_t)i*3 + 1] - J.mn[1]),
	               w = (uint64_t)(int64_t)(J.coords[(size_t)i*3 + 2] - J.mn[2]);
	uint64_t bits = 0; const uint64_t l = 1;
	for(int k = 0; k < 21; k++) bits |= (x & l << k) << (2*k) | (y & l << k) << (2*k + 1) | (w & l << k) << (2*k + 2);
	J.keys[i] = bits; J.vals[i] = i;
}

// the sorted records (ascending keys: the host's z after std::sort over the reversed range) -> prediction quads, and the equal-key flag
__global__ __launch_bounds__(256) void k_enc_zflag(ZJob J) {
	const uint32_t i = blockIdx.x*256 + threadIdx.x;
	if(i >= J.n) return;
	const uint32_t prev = i ? J.vals[i - 1] : 0xffffffffu;
	uint32_t *q = J.quads + (size_t)i*4;
	q[0] = J.vals[i]; q[1] = prev; q[2] = prev; q[3] = prev;
	if(i && J.keys[i] == J.keys[i - 1]) atomicOr(J.flag, 1u);
}

// ---- LSD radix sort ----
template <typename K>
__global__ __launch_bounds__(RS_THREADS) void k_enc_rs_hist(const K *__restrict__ keys, uint32_t n, uint32_t shift, uint32_t *__restrict__ hist) {
	__shared__ uint32_t h[256];
	h[threadIdx.x] = 0;
	__syncthreads();
	const uint32_t base = blockIdx.x*RS_TILE;
	for(uint32_t k = 0; k < RS_ITEMS; k++) {
		const uint32_t i = base + k*RS_THREADS + threadIdx.x;
		if(i < n) atomicAdd(&h[(uint32_t)(keys[i] >> shift) & 255u], 1u);
	}
	__syncthreads();
	hist[(size_t)threadIdx.x*gridDim.x + blockIdx.x] = h[threadIdx.x];
}

// exclusive scan of len counts by one workgroup of 1024: each thread a contiguous run
__global__ __launch_bounds__(1024) void k_enc_rs_scan(uint32_t *__restrict__ hist, uint32_t len) {
	__shared__ uint32_t wsum[16];
	const uint32_t t = threadIdx.x, per = (len + 1023)/1024, b = t*per, e = min(len, b + per);
	uint32_t s = 0;
	for(uint32_t i = b; i < e; i++) s += hist[i];
	const uint32_t inc = wave_inclusive_scan_u32(s);
	if(lane_id() == 63) wsum[wave_id()] = inc;
	__syncthreads();
	uint32_t off = 0;
	for(uint32_t w = 0; w < wave_id(); w++) off += wsum[w];
	uint32_t run = off + inc - s;
	for(uint32_t i = b; i < e; i++) { const uint32_t c = hist[i]; hist[i] = run; run += c; }
}

template <typename K>
__global__ __launch_bounds__(RS_THREADS) void k_enc_rs_scatter(const K *__restrict__ keys, const uint32_t *__restrict__ vals, K *__restrict__ keys_out,
                                                                uint32_t *__restrict__ vals_out, uint32_t n, uint32_t shift, const uint32_t *__restrict__ hist) {
	__shared__ uint32_t run[256];
	__shared__ uint32_t wc[RS_THREADS/64][256];
	const uint32_t t = threadIdx.x, lane = lane_id(), w = wave_id();
	run[t] = hist[(size_t)t*gridDim.x + blockIdx.x];
	const uint64_t lt = (1ull << lane) - 1ull;
	const uint32_t base = blockIdx.x*RS_TILE;
	for(uint32_t k = 0; k < RS_ITEMS; k++) {
		const uint32_t i = base + k*RS_THREADS + t;
		const bool valid = i < n;
		K key = 0; uint32_t val = 0, d = 0;
		if(valid) { key = keys[i]; val = vals[i]; d = (uint32_t)(key >> shift) & 255u; }
		for(uint32_t x = t; x < (RS_THREADS/64)*256; x += RS_THREADS) (&wc[0][0])[x] = 0;
		__syncthreads();
		uint64_t same = __ballot(valid);
		for(uint32_t bit = 0; bit < 8; bit++) { const uint64_t bb = __ballot((d >> bit) & 1u); same &= ((d >> bit) & 1u) ? bb : ~bb; }
		const uint32_t rank = (uint32_t)__popcll(same & lt);
		if(valid && rank == 0) wc[w][d] = (uint32_t)__popcll(same);
		__syncthreads();
		if(valid) {
			uint32_t at = run[d] + rank;
			for(uint32_t v = 0; v < w; v++) at += wc[v][d];
			keys_out[at] = key; vals_out[at] = val;
		}
		__syncthreads();
		uint32_t add = 0;
		for(uint32_t v = 0; v < RS_THREADS/64; v++) add += wc[v][t];
		run[t] += add;
		__syncthreads();
	}
}

template __global__ void k_enc_rs_hist<uint32_t>(const uint32_t *, uint32_t, uint32_t, uint32_t *);
template __global__ void k_enc_rs_hist<uint64_t>(const uint64_t *, uint32_t, uint32_t, uint32_t *);
template __global__ void k_enc_rs_scatter<uint32_t>(const uint32_t *, const uint32_t *, uint32_t *, uint32_t *, uint32_t, uint32_t, const uint32_t *);
template __global__ void k_enc_rs_scatter<uint64_t>(const uint64_t *, const uint32_t *, uint64_t *, uint32_t *, uint32_t, uint32_t, const uint32_t *);

} // namespace corto_hip
