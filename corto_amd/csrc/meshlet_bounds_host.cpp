// meshlet_bounds_host.cpp — the test hook of crthip_batch_bind_meshlet_bounds (crthip_meshlet_bounds_model): meshlet_bounds.h on the host in
// k_meshlet_bounds.hip's partition - a grid of workgroups sized by the capacity, four waves each, a wave's 64 lanes walked in a loop at every
// step, all in orders shuffled by the seed (meshlets are independent, a step's lanes meet only through the wave's maximum and sum, and the
// record has one writer: any order gives the same bytes).
#include <algorithm>
#include <new>
#include <vector>

#include "../../include/corto_hip.h"
#include "encoder_internal.h"
#include "meshlet_bounds.h"

using namespace corto_hip;

namespace corto_hip {

namespace {

std::vector<uint32_t> mb_shuffled(uint32_t n, uint64_t &x) {
	std::vector<uint32_t> order(n);
	for(uint32_t i = 0; i < n; i++) order[i] = i;
	for(uint32_t i = n; i > 1; i--) {                                     // Fisher-Yates on a 64-bit LCG
		x = x*6364136223846793005ull + 1442695040888963407ull;
		std::swap(order[i - 1], order[(uint32_t)((x >> 33) % i)]);
	}
	return order;
}

// the wave as mb_meshlet sees it, on the host: 64 lane states, every step's lanes in a fresh order
struct MbWaveHost {
	MbLane L[MB_WAVE];
	uint64_t *rng;
	template <class F> void each(F f) { for(uint32_t lane : mb_shuffled(MB_WAVE, *rng)) f(lane, L[lane]); }
	void sync() {}
	template <class G> uint32_t max_u32(G get) { uint32_t m = 0; for(uint32_t lane : mb_shuffled(MB_WAVE, *rng)) m = std::max(m, (uint32_t)get(L[lane])); return m; }
	template <class G> uint32_t sum_u32(G get) { uint32_t s = 0; for(uint32_t lane : mb_shuffled(MB_WAVE, *rng)) s += (uint32_t)get(L[lane]); return s; }
};

} // namespace

void meshlet_bounds_model(const MbIn &J, uint32_t capacity, uint32_t seed) {
	uint64_t rng = 0x9E3779B97F4A7C15ull ^ seed;
	std::vector<MbWaveMem> mem(MB_WAVES);
	for(auto &m : mem) for(auto &s : m.slot) s = mb_i32x4{(int32_t)0xA5A5A5A5, (int32_t)0xA5A5A5A5, (int32_t)0xA5A5A5A5, (int32_t)0xA5A5A5A5};   // (LDS is not zeroed either)
	for(uint32_t block : mb_shuffled((capacity + MB_WAVES - 1)/MB_WAVES, rng))
		for(uint32_t w : mb_shuffled(MB_WAVES, rng)) {
			const uint32_t k = block*MB_WAVES + w;
			if(k >= J.nmeshlets || k >= capacity) continue;
			MbWaveHost x{}; x.rng = &rng;
			mb_meshlet(x, mem[w], J, k);
		}
}

} // namespace corto_hip

extern "C" int crthip_meshlet_bounds_model(const int32_t *position, uint32_t nvert, const crthip_meshlet *meshlets, const uint32_t *vertices,
                                           const uint8_t *triangles, const crthip_meshlet_counts *counts, crthip_meshlet_bounds *bounds, uint32_t capacity,
                                           uint32_t seed) {
	if(!counts || (nvert && !position) || (counts->meshlets && (!meshlets || !bounds)) || (counts->vertices && !vertices) || (counts->triangle_bytes && !triangles))
		return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_meshlet_bounds_model: null argument");
	if((uintptr_t)bounds % 16 || (uintptr_t)meshlets % 16) return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_meshlet_bounds_model: the records are 16-byte aligned");
	if(capacity < counts->meshlets) return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_meshlet_bounds_model: capacity is below the counts");
	for(uint32_t k = 0; k < counts->meshlets; k++) {                          // a finished build: every meshlet inside the arrays, every local id inside the meshlet
		const crthip_meshlet &m = meshlets[k];
		bool ok = m.vertex_count <= MB_MAX_VERTICES && m.triangle_count <= MB_MAX_TRIANGLES && m.vertex_offset <= counts->vertices &&
			m.vertex_count <= counts->vertices - m.vertex_offset && m.triangle_offset <= counts->triangle_bytes &&
			3ull*m.triangle_count <= counts->triangle_bytes - m.triangle_offset;
		for(uint32_t e = 0; ok && e < 3*m.triangle_count; e++) ok = triangles[m.triangle_offset + e] < m.vertex_count;
		if(!ok) return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_meshlet_bounds_model: a meshlet reaches outside the arrays or its own vertex list");
	}
	static_assert(sizeof(crthip_meshlet_bounds) == 48 && sizeof(crthip_meshlet) == 16, "record layout");
	MbIn J;
	J.position = position; J.nvert = nvert;
	J.meshlets = (const mb_u32x4 *)meshlets; J.vertices = vertices; J.triangles = triangles;
	J.nmeshlets = counts->meshlets; J.nvertices = counts->vertices; J.ntriangle_bytes = counts->triangle_bytes;
	J.out = (mb_u32x4 *)bounds;
	try {
		meshlet_bounds_model(J, capacity, seed);
		return CRTHIP_OK;
	} catch(const std::bad_alloc &) {
		return ctx_fail(CRTHIP_E_NOMEM, nullptr);
	}
}
