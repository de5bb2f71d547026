// tangent_host.cpp — the test hook of crthip_batch_bind_computed_tangents (crthip_tangent_model): tangent.h on the host, in k_tangent.hip's
// partitions - a workgroup's 256 lanes walked in a loop and the blocks of the batch-wide kernels, both in an order shuffled by the seed
// (the sums are integers modulo 2^64 and every vertex is finished by one lane: any order gives the same bytes).
#include <algorithm>
#include <new>
#include <vector>

#include "../../include/corto_hip.h"
#include "encoder_internal.h"
#include "tangent.h"

using namespace corto_hip;

namespace corto_hip {

static std::vector<uint32_t> tan_shuffled(uint32_t n, uint64_t seed) {
	std::vector<uint32_t> order(n);
	for(uint32_t i = 0; i < n; i++) order[i] = i;
	uint64_t x = 0x9E3779B97F4A7C15ull ^ seed;
	for(uint32_t i = n; i > 1; i--) {                                     // Fisher-Yates on a 64-bit LCG
		x = x*6364136223846793005ull + 1442695040888963407ull;
		std::swap(order[i - 1], order[(uint32_t)((x >> 33) % i)]);
	}
	return order;
}

void tangent_model(const TanIn &J, int which, uint32_t seed) {
	uint64_t s = seed;
	auto lanes = [&]() { return tan_shuffled(TAN_THREADS, s += 0x51ED27ull); };
	if(which == 0) {                                                      // k_tangent_blob: one accumulator, used for T and then for B
		std::vector<uint64_t> acc((size_t)3*J.nvert, 0);
		std::vector<TanLaneState> S(TAN_THREADS);
		auto add = [&](uint32_t v, uint32_t i, uint64_t x) { acc[(size_t)3*v + i] += x; };
		for(uint32_t lane : lanes()) tan_faces_lane(J, 0, 0, J.nface, lane, add);
		for(uint32_t lane : lanes()) tan_blob_keep_T(J, acc.data(), lane, S[lane]);
		for(uint32_t lane : lanes()) tan_faces_lane(J, 1, 0, J.nface, lane, add);
		for(uint32_t lane : lanes()) tan_blob_finish(J, acc.data(), lane, S[lane]);
		return;
	}
	std::vector<uint64_t> acc((size_t)TAN_ACC_WORDS*J.nvert, 0);           // the zeroed scratch
	const uint32_t nfb = (J.nface + TAN_BLOCK - 1)/TAN_BLOCK, nvb = (J.nvert + TAN_BLOCK - 1)/TAN_BLOCK;
	for(uint32_t b : tan_shuffled(nfb, s += 0x9E37ull)) {                 // k_tangent_faces
		const uint32_t f0 = b*TAN_BLOCK, f1 = J.nface - f0 > TAN_BLOCK ? f0 + TAN_BLOCK : J.nface;
		for(uint32_t lane : lanes())
			for(uint32_t w = 0; w < 2; w++)
				tan_faces_lane(J, w, f0, f1, lane, [&](uint32_t v, uint32_t i, uint64_t x) { acc[(size_t)v*TAN_ACC_WORDS + 3*w + i] += x; });
	}
	for(uint32_t b : tan_shuffled(nvb, s += 0x9E37ull)) {                 // k_tangent_vertex
		const uint32_t v0 = b*TAN_BLOCK, v1 = J.nvert - v0 > TAN_BLOCK ? v0 + TAN_BLOCK : J.nvert;
		for(uint32_t lane : lanes()) for(uint32_t v = v0 + lane; v < v1; v += TAN_THREADS) tan_vertex(J, v, acc.data());
	}
}

} // namespace corto_hip

extern "C" int crthip_tangent_model(const int32_t *position, const int32_t *uv, const void *index, uint32_t index_u16, uint32_t nvert, uint32_t nface,
                                    const void *normal, uint32_t normal_format, uint32_t normal_stride, void *out, uint32_t format, uint32_t stride,
                                    int which, uint32_t seed) {
	if((which != 0 && which != 1) || (nvert && (!position || !uv || !normal || !out)) || (nface && !index))
		return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_tangent_model: null argument or an unknown partition");
	if((format != CRTHIP_FMT_FLOAT && format != CRTHIP_FMT_INT16) || (normal_format != CRTHIP_FMT_FLOAT && normal_format != CRTHIP_FMT_INT16))
		return ctx_fail(CRTHIP_E_FORMAT, "crthip_tangent_model: tangents and normals are FLOAT or INT16");
	const uint32_t el = format == CRTHIP_FMT_INT16 ? 2u : 4u, nel = normal_format == CRTHIP_FMT_INT16 ? 2u : 4u;
	if(((uintptr_t)out % el) || (stride && (stride < 4*el || stride % el)) || ((uintptr_t)normal % nel) || (normal_stride && (normal_stride < 3*nel || normal_stride % nel)))
		return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_tangent_model: a destination, a normal array or a stride a binding would refuse");
	if(which == 0 && nvert > TAN_BLOB_SLOTS*TAN_THREADS)
		return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_tangent_model: the one-workgroup partition takes up to 2304 vertices");
	TanIn J;
	J.position = position; J.uv = uv; J.faces = index; J.faces_u16 = index_u16 ? 1u : 0u; J.nvert = nvert; J.nface = nface;
	J.normal = normal; J.normal_i16 = normal_format == CRTHIP_FMT_INT16; J.normal_stride = normal_stride ? normal_stride : 3*nel;
	J.out = out; J.out_i16 = format == CRTHIP_FMT_INT16; J.out_stride = stride ? stride : 4*el;
	try {
		tangent_model(J, which, seed);
		return CRTHIP_OK;
	} catch(const std::bad_alloc &) {
		return ctx_fail(CRTHIP_E_NOMEM, nullptr);
	}
}
