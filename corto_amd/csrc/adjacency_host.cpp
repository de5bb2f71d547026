// adjacency_host.cpp — the test hook of crthip_batch_bind_adjacency (crthip_adjacency_model): adjacency.h on the host in k_adjacency.hip's
// partitions - a workgroup's 256 threads walked in a loop at every step, the workgroups of a grid too, all in orders shuffled by the seed.  The order of the atomics, and so the slot a half-edge gets in its vertex's
// list, changes with the seed; every result is a minimum, an existence test or a sum, so the bytes do not.
#include <algorithm>
#include <new>
#include <vector>

#include "../../include/corto_hip.h"
#include "encoder_internal.h"
#include "adjacency.h"

using namespace corto_hip;

namespace corto_hip {

namespace {

std::vector<uint32_t> adj_shuffled(uint32_t n, uint64_t &x) {
	std::vector<uint32_t> order(n);
	for(uint32_t i = 0; i < n; i++) order[i] = i;
	for(uint32_t i = n; i > 1; i--) {                                     // Fisher-Yates on a 64-bit LCG
		x = x*6364136223846793005ull + 1442695040888963407ull;
		std::swap(order[i - 1], order[(uint32_t)((x >> 33) % i)]);
	}
	return order;
}

// the workgroup as adjacency.h sees it, on the host: 256 thread states, every step's threads in a fresh order
struct AdjGroupHost {
	AdjLane L[ADJ_THREADS];
	uint64_t *rng;
	template <class F> void each(F f) { for(uint32_t tid : adj_shuffled(ADJ_THREADS, *rng)) f(tid, L[tid]); }
	void sync() {}
	void wave_scan() {
		for(uint32_t w = 0; w < ADJ_WAVES; w++) {
			uint32_t s = 0;
			for(uint32_t l = 0; l < ADJ_WAVE; l++) { s += L[w*ADJ_WAVE + l].v; L[w*ADJ_WAVE + l].incl = s; }
			for(uint32_t l = 0; l < ADJ_WAVE; l++) L[w*ADJ_WAVE + l].tot = s;
		}
	}
	void wave_carry() {
		uint32_t c = 0;
		for(uint32_t w = 0; w < ADJ_WAVES; w++) {
			uint32_t s = 0;
			for(uint32_t l = 0; l < ADJ_WAVE; l++) { s += L[w*ADJ_WAVE + l].v; L[w*ADJ_WAVE + l].carry = c; }
			c += s;
		}
	}
	void block_sums() {
		AdjCounts s{0, 0, 0};
		for(uint32_t tid : adj_shuffled(ADJ_THREADS, *rng)) { s.boundary += L[tid].c.boundary; s.duplicate += L[tid].c.duplicate; s.invalid += L[tid].c.invalid; }
		L[0].c = s;
	}
	template <class F> void thread0(F f) { f(L[0]); }
};

// a fresh workgroup: its thread states hold garbage, as registers do
AdjGroupHost fresh_group(uint64_t &rng) {
	AdjGroupHost g;
	for(AdjLane &l : g.L) { l.v = l.incl = l.tot = l.carry = l.in = 0xA5A5A5A5u; l.c = AdjCounts{0xA5A5A5A5u, 0xA5A5A5A5u, 0xA5A5A5A5u}; }
	g.rng = &rng;
	return g;
}

} // namespace

// which 0: k_adjacency_blob (the caller made sure of adj_in_blob); which 1: k_adjacency_count, _offsets, _fill, _twin.  rec is never null here
void adjacency_model(const AdjIn &J, uint32_t *twin, crthip_adjacency_counts *rec, int which, uint32_t seed) {
	uint64_t rng = 0x9E3779B97F4A7C15ull ^ seed;
	if(which == 0) {
		// (LDS is not zeroed on the device either; exactly the kernel's bytes, so that a sanitizer sees a step past them)
		std::vector<uint32_t> end((size_t)J.nvert + 1, 0xA5A5A5A5u);
		std::vector<uint16_t> list((size_t)J.nface*3, (uint16_t)0xA5A5u);
		AdjGroupHost g = fresh_group(rng);
		adj_blob(g, J, AdjLdsStore{end.data(), list.data()}, twin, rec);
		return;
	}
	std::vector<uint32_t> end((size_t)J.nvert + 1, 0u);                  // (the FillJob in front of adjacency_count)
	std::vector<uint32_t> list((size_t)J.nface*3, 0xA5A5A5A5u);
	*rec = crthip_adjacency_counts{0xA5A5A5A5u, 0xA5A5A5A5u, 0xA5A5A5A5u, 0xA5A5A5A5u};   // (adjacency_offsets zeroes it)
	const AdjMemStore st{end.data(), list.data()};
	const uint32_t nb = adj_blocks(J.nface);
	for(uint32_t k : adj_shuffled(nb, rng)) { AdjGroupHost g = fresh_group(rng); adj_count_block(g, J, st, k); }
	{ AdjGroupHost g = fresh_group(rng); adj_offsets(g, J, st, rec); }
	for(uint32_t k : adj_shuffled(nb, rng)) { AdjGroupHost g = fresh_group(rng); adj_fill_block(g, J, st, k); }
	for(uint32_t k : adj_shuffled(nb, rng)) { AdjGroupHost g = fresh_group(rng); adj_twin_block(g, J, st, twin, rec, k); }
}

} // namespace corto_hip

extern "C" int crthip_adjacency_model(const void *index, uint32_t index_u16, uint32_t nface, uint32_t nvert, uint32_t *twin, crthip_adjacency_counts *counts,
                                      int which, uint32_t seed) {
	if((which != 0 && which != 1) || (nface && !index)) return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_adjacency_model: null index or an unknown partition");
	crthip_adjacency_counts rec{0, 0, 0, 0};
	if(nface) {
		// (the binding's checks: a host array of exactly 3*nface words, no device record)
		crthip_adjacency_binding a{twin, nullptr, (uint64_t)nface*3 <= 0xFFFFFFFFull ? nface*3 : 0u, 0u};
		if(const char *why = adjacency_binding_error(&a, nface)) return ctx_fail(CRTHIP_E_ARGUMENT, why);
		if(nvert == 0xFFFFFFFFu) return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_adjacency_model: nvert + 1 does not fit 32 bits");
		if(which == 0 && !adj_in_blob(nvert, nface)) return ctx_fail(CRTHIP_E_LIMIT, "crthip_adjacency_model: the blob's lists do not fit adjacency_blob's LDS (partition 1 takes it)");
		AdjIn J; J.index = index; J.index_u16 = index_u16 ? 1u : 0u; J.nface = nface; J.nvert = nvert;
		try {
			adjacency_model(J, twin, &rec, which, seed);
		} catch(const std::bad_alloc &) {
			return ctx_fail(CRTHIP_E_NOMEM, nullptr);
		}
	}
	if(counts) *counts = rec;
	return CRTHIP_OK;
}
