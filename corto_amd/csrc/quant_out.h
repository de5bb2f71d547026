// quant_out.h — CRTHIP_BIND_QUANTIZED: a generic attribute's delta-decoded integers leave the decoder as uint16 grid values relative to the
// blob's per-component minimum, with the transform that takes them back (crthip_quant_transform, include/corto_hip.h).  The arithmetic and
// the partition of k_quant_out.hip as __host__ __device__ code, so that the host can run the very same source in the kernels' partition
// (crthip_quant_out_model, quant_out_host.cpp; tests/cpp/quant_out_check.cpp runs it under the sanitizers).
//
// Two passes over nvert x N int32 values (packed, in the batch's scratch):
//   range   signed min / max a component.  A lane folds the vertices lane, lane + QOUT_THREADS, ... of its stretch; lanes, waves and blocks
//           are merged with integer min / max, which are associative and commutative: no order can change a bit of the result.
//           Between blocks the merge is an atomicMin / atomicMax on the values' order-preserving image in uint32 (qout_bias: INT32_MIN -> 0,
//           INT32_MAX -> 0xFFFFFFFF), so that the record's seed is a fill of 0xFF bytes (the minima) and of 0x00 bytes (the maxima).
//   store   out[i][c] = (uint16_t)(v[i][c] - base[c]) where every span fits 16 bits; else nothing is stored (written = 0).
//           Packed (stride 0): the nvert*N halfwords are one array - up to seven halfwords to the first 16-byte boundary, 16-byte vectors of
//           eight, up to seven behind them (enc_in_range_cut's cut).  With a stride: a lane a vertex, N halfword stores.
//           Either way the bytes written are exactly [buffer + i*stride, + 2*N) of every vertex.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/corto_hip.h"

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define QOUT_HD __host__ __device__ inline
#else
#define QOUT_HD inline
#endif

namespace corto_hip {

constexpr uint32_t QOUT_THREADS = 256;
constexpr uint32_t QOUT_BLOCK = 1024;                      // vertices a workgroup of the two-kernel path (k_quant_range / k_quant_store)
constexpr uint32_t QOUT_SPAN_MAX = 65535;

struct QuantRange { int32_t mn[4], mx[4]; };
// the two-kernel path's accumulator in scratch: qout_bias images, seeded mn = 0xFFFFFFFF, mx = 0
struct QuantRangeWords { uint32_t mn[4], mx[4]; };
struct alignas(16) QuantVec { uint32_t w[4]; };            // eight halfwords: one 16-byte store

QOUT_HD uint32_t qout_bias(int32_t v) { return (uint32_t)v ^ 0x80000000u; }
QOUT_HD int32_t qout_unbias(uint32_t u) { return (int32_t)(u ^ 0x80000000u); }

QOUT_HD void qout_range_empty(QuantRange &r) { for(int c = 0; c < 4; c++) { r.mn[c] = INT32_MAX; r.mx[c] = INT32_MIN; } }
QOUT_HD void qout_range_merge(QuantRange &a, const QuantRange &b) {
	for(int c = 0; c < 4; c++) { if(b.mn[c] < a.mn[c]) a.mn[c] = b.mn[c]; if(b.mx[c] > a.mx[c]) a.mx[c] = b.mx[c]; }
}
// a lane's share of the vertices [v0, v1): v0 + lane, v0 + lane + QOUT_THREADS, ...
QOUT_HD void qout_fold_lane(QuantRange &r, const int32_t *values, uint32_t N, uint64_t v0, uint64_t v1, uint32_t lane) {
	qout_range_empty(r);
	for(uint64_t v = v0 + lane; v < v1; v += QOUT_THREADS) {
		const int32_t *p = values + v*N;
		for(uint32_t c = 0; c < 4; c++) if(c < N) { const int32_t x = p[c]; if(x < r.mn[c]) r.mn[c] = x; if(x > r.mx[c]) r.mx[c] = x; }
	}
}
QOUT_HD void qout_range_from_words(QuantRange &r, const QuantRangeWords &w) {
	for(int c = 0; c < 4; c++) { r.mn[c] = qout_unbias(w.mn[c]); r.mx[c] = qout_unbias(w.mx[c]); }
}

// the record of an attribute whose values span `r` (nvert >= 1); components beyond N are zero.  Returns written
QOUT_HD uint32_t qout_transform(const QuantRange &r, uint32_t N, float q, crthip_quant_transform &t) {
	uint32_t fits = 1;
	for(uint32_t c = 0; c < 4; c++) {
		const bool has = c < N;
		t.base[c] = has ? r.mn[c] : 0;
		t.span[c] = has ? (uint32_t)((int64_t)r.mx[c] - (int64_t)r.mn[c]) : 0u;   // in 64 bits: INT32_MAX - INT32_MIN is 2^32 - 1
		if(t.span[c] > QOUT_SPAN_MAX) fits = 0;
	}
	t.q = q; t.components = N; t.written = fits; t.reserved = 0;
	return fits;
}

// the packed array's cut: n halfwords from `buffer` (2-byte aligned)
QOUT_HD void qout_cut(const void *buffer, uint64_t n, uint64_t &head, uint64_t &groups, uint64_t &tail) {
	const uint64_t to_boundary = ((16u - (uint32_t)((uintptr_t)buffer & 15u)) & 15u)/2u;
	head = to_boundary < n ? to_boundary : n;
	groups = (n - head)/8u; tail = n - head - groups*8u;
}
QOUT_HD uint16_t qout_value(int32_t v, int32_t base) { return (uint16_t)((uint32_t)v - (uint32_t)base); }

struct QuantStore {                                         // what the store pass knows of a job
	const int32_t *values; void *buffer; uint32_t stride, nvert, N; int32_t base[4];
};
// base[c] for a c that is not a compile-time constant, by selects: a register array indexed by a variable would be moved to LDS or scratch
QOUT_HD int32_t qout_base(const QuantStore &S, uint32_t c) { return c == 0 ? S.base[0] : c == 1 ? S.base[1] : c == 2 ? S.base[2] : S.base[3]; }
// groups of the packed array a workgroup of the two-kernel path takes: what QOUT_BLOCK vertices of N components hold
QOUT_HD uint64_t qout_groups_per_block(uint32_t N) { return (uint64_t)QOUT_BLOCK*N/8u; }

// One lane's stores.  Packed: the groups g0 + lane, g0 + lane + QOUT_THREADS, ... below g1, and - `edges`: one workgroup a job does them - the
// head (lanes 0..6) and the tail (lanes 64..70).  Strided: the vertices v0 + lane, ... below v1.
QOUT_HD void qout_store_lane(const QuantStore &S, uint64_t g0, uint64_t g1, uint64_t v0, uint64_t v1, bool edges, uint32_t lane) {
	if(S.stride) {
		for(uint64_t v = v0 + lane; v < v1; v += QOUT_THREADS) {
			const int32_t *p = S.values + v*S.N;
			uint16_t *o = (uint16_t *)((uint8_t *)S.buffer + v*S.stride);
			for(uint32_t c = 0; c < 4; c++) if(c < S.N) o[c] = qout_value(p[c], S.base[c]);
		}
		return;
	}
	const uint64_t n = (uint64_t)S.nvert*S.N;
	uint64_t head, groups, tail;
	qout_cut(S.buffer, n, head, groups, tail);
	uint16_t *o = (uint16_t *)S.buffer;
	if(g1 > groups) g1 = groups;
	for(uint64_t g = g0 + lane; g < g1; g += QOUT_THREADS) {
		const uint64_t e = head + g*8u;
		const int32_t *p = S.values + e;
		uint32_t c = (uint32_t)(e % S.N);
		QuantVec x;
		for(int k = 0; k < 4; k++) {
			const uint32_t lo = qout_value(p[2*k], qout_base(S, c)); c = c + 1 == S.N ? 0u : c + 1;
			const uint32_t hi = qout_value(p[2*k + 1], qout_base(S, c)); c = c + 1 == S.N ? 0u : c + 1;
			x.w[k] = lo | (hi << 16);
		}
		*(QuantVec *)(o + e) = x;
	}
	if(!edges) return;
	if(lane < head) o[lane] = qout_value(S.values[lane], qout_base(S, lane % S.N));
	if(lane >= 64 && lane - 64 < tail) { const uint64_t e = head + groups*8u + (lane - 64); o[e] = qout_value(S.values[e], qout_base(S, (uint32_t)(e % S.N))); }
}

} // namespace corto_hip
