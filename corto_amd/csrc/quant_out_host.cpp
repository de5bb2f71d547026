// quant_out_host.cpp — the test hook of CRTHIP_BIND_QUANTIZED (crthip_quant_out_model): the two passes of quant_out.h on the host, in
// k_quant_out.hip's partition - a workgroup's 256 lanes walked in a loop from the last to the first, the blocks of the two-kernel path in
// a shuffled order (min / max and the stores are independent of it: any order gives the same bytes).
#include <algorithm>
#include <new>
#include <vector>

#include "../../include/corto_hip.h"
#include "encoder_internal.h"
#include "quant_out.h"

using namespace corto_hip;

namespace corto_hip {

static std::vector<uint32_t> shuffled(uint32_t n, uint64_t seed) {
	std::vector<uint32_t> order(n);
	for(uint32_t i = 0; i < n; i++) order[i] = i;
	uint64_t x = 0x9E3779B97F4A7C15ull ^ seed;
	for(uint32_t i = n; i > 1; i--) {                                     // Fisher-Yates on a 64-bit LCG
		x = x*6364136223846793005ull + 1442695040888963407ull;
		std::swap(order[i - 1], order[(uint32_t)((x >> 33) % i)]);
	}
	return order;
}

// a workgroup's range of the vertices [v0, v1): lanes into waves, waves into the block (block_range)
static QuantRange block_fold(const int32_t *values, uint32_t N, uint64_t v0, uint64_t v1) {
	QuantRange waves[QOUT_THREADS/64];
	for(uint32_t w = 0; w < QOUT_THREADS/64; w++) qout_range_empty(waves[w]);
	for(uint32_t lane = QOUT_THREADS; lane-- > 0;) { QuantRange r; qout_fold_lane(r, values, N, v0, v1, lane); qout_range_merge(waves[lane/64], r); }
	QuantRange all;
	qout_range_empty(all);
	for(uint32_t w = QOUT_THREADS/64; w-- > 0;) qout_range_merge(all, waves[w]);
	return all;
}

void quant_out_model(const int32_t *values, uint32_t nvert, uint32_t N, uint32_t stride, void *out, crthip_quant_transform &t, int which, uint32_t seed) {
	const float q = t.q;
	QuantStore S;
	S.values = values; S.buffer = out; S.stride = stride == 2*N ? 0u : stride; S.nvert = nvert; S.N = N;
	if(nvert == 0) { t = crthip_quant_transform{}; t.written = 1; return; }
	if(which == 0) {                                                      // k_quant_out_blob
		const QuantRange r = block_fold(values, N, 0, nvert);
		if(!qout_transform(r, N, q, t)) return;
		for(int c = 0; c < 4; c++) S.base[c] = t.base[c];
		for(uint32_t lane = QOUT_THREADS; lane-- > 0;) qout_store_lane(S, 0, ~0ull, 0, nvert, true, lane);
		return;
	}
	const uint32_t nblocks = (nvert + QOUT_BLOCK - 1)/QOUT_BLOCK;
	QuantRangeWords w;                                                    // the FillJobs' seed
	for(int c = 0; c < 4; c++) { w.mn[c] = 0xFFFFFFFFu; w.mx[c] = 0u; }
	for(uint32_t b : shuffled(nblocks, seed)) {                           // k_quant_range
		const uint64_t v0 = (uint64_t)b*QOUT_BLOCK;
		const QuantRange r = block_fold(values, N, v0, std::min<uint64_t>(v0 + QOUT_BLOCK, nvert));
		for(uint32_t c = 0; c < N; c++) { w.mn[c] = std::min(w.mn[c], qout_bias(r.mn[c])); w.mx[c] = std::max(w.mx[c], qout_bias(r.mx[c])); }
	}
	QuantRange r;
	qout_range_from_words(r, w);
	if(!qout_transform(r, N, q, t)) return;
	for(int c = 0; c < 4; c++) S.base[c] = t.base[c];
	const uint64_t per = qout_groups_per_block(N);
	for(uint32_t b : shuffled(nblocks, seed + 0x51ED27ull)) {             // k_quant_store
		const uint64_t v0 = (uint64_t)b*QOUT_BLOCK;
		for(uint32_t lane = QOUT_THREADS; lane-- > 0;) qout_store_lane(S, b*per, (b + 1)*per, v0, std::min<uint64_t>(v0 + QOUT_BLOCK, nvert), b == 0, lane);
	}
}

} // namespace corto_hip

extern "C" int crthip_quant_out_model(const int32_t *values, uint32_t nvert, uint32_t N, uint32_t stride, void *out, crthip_quant_transform *transform,
                                      int which, uint32_t seed) {
	if(!transform || N < 1 || N > 4 || (which != 0 && which != 1) || (nvert && (!values || !out)))
		return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_quant_out_model: null argument, N outside 1..4 or an unknown partition");
	if(((uintptr_t)out & 1u) || (stride && (stride < 2*N || (stride & 1u))))
		return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_quant_out_model: a destination or stride a binding would refuse");
	try {
		quant_out_model(values, nvert, N, stride, out, *transform, which, seed);
		return CRTHIP_OK;
	} catch(const std::bad_alloc &) {
		return ctx_fail(CRTHIP_E_NOMEM, nullptr);
	}
}
