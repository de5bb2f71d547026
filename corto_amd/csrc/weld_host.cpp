// weld_host.cpp — the test hook of crthip_batch_bind_weld (crthip_weld_model): weld.h on the host in k_weld.hip's partitions - a workgroup's 256
// threads walked in a loop at every step, the workgroups of a grid too, all in orders shuffled by the seed.  Which vertex wins a slot's
// compare-and-swap changes with the seed; every result is a minimum or a sum, so the bytes do not.
#include <algorithm>
#include <new>
#include <vector>

#include "../../include/corto_hip.h"
#include "encoder_internal.h"
#include "weld.h"

using namespace corto_hip;

namespace corto_hip {

namespace {

std::vector<uint32_t> weld_shuffled(uint32_t n, uint64_t &x) {
	std::vector<uint32_t> order(n);
	for(uint32_t i = 0; i < n; i++) order[i] = i;
	for(uint32_t i = n; i > 1; i--) {                                     // Fisher-Yates on a 64-bit LCG
		x = x*6364136223846793005ull + 1442695040888963407ull;
		std::swap(order[i - 1], order[(uint32_t)((x >> 33) % i)]);
	}
	return order;
}

// the workgroup as weld.h sees it, on the host: 256 thread states, every step's threads in a fresh order
struct WeldGroupHost {
	WeldLane L[WELD_THREADS];
	uint64_t *rng;
	template <class F> void each(F f) { for(uint32_t tid : weld_shuffled(WELD_THREADS, *rng)) f(tid, L[tid]); }
	void sync() {}
	void block_sum() {
		uint32_t s = 0;
		for(uint32_t tid : weld_shuffled(WELD_THREADS, *rng)) s += L[tid].c;
		L[0].c = s;
	}
	template <class F> void thread0(F f) { f(L[0]); }
};

// a fresh workgroup: its thread states hold garbage, as registers do (k_weld_blob clears its own two words: a blob without faces or without a
// welded index sums nothing into them)
WeldGroupHost fresh_group(uint64_t &rng, bool cleared) {
	WeldGroupHost g;
	for(WeldLane &l : g.L) l.c = l.unique = cleared ? 0u : 0xA5A5A5A5u;
	g.rng = &rng;
	return g;
}

} // namespace

// which 0: k_weld_blob (the caller made sure of weld_in_blob); which 1: k_weld_insert, _lookup, _index.  rec is never null here
void weld_model(const WeldIn &J, uint32_t *remap, uint32_t *windex, crthip_weld_counts *rec, WeldStats *stats, int which, uint32_t seed) {
	uint64_t rng = 0x9E3779B97F4A7C15ull ^ seed;
	const uint64_t T = weld_slots(J.nvert);
	if(which == 0) {
		// (LDS is not zeroed on the device either; exactly the kernel's words, so that a sanitizer sees a step past them)
		std::vector<uint32_t> table((size_t)T, 0xA5A5A5A5u);
		WeldGroupHost g = fresh_group(rng, true);
		weld_blob(g, J, WeldLdsTable{table.data()}, remap, windex, rec, stats);
		return;
	}
	std::vector<uint32_t> table((size_t)T, 0u);                           // (the FillJob in front of weld_insert)
	*rec = crthip_weld_counts{0xA5A5A5A5u, 0xA5A5A5A5u, 0xA5A5A5A5u, 0xA5A5A5A5u};   // (weld_insert's first workgroup stores it)
	const WeldMemTable tb{table.data()};
	const uint32_t nv = weld_vblocks(J.nvert), nc = weld_cblocks(J.nface);
	for(uint32_t k : weld_shuffled(nv, rng)) { WeldGroupHost g = fresh_group(rng, false); weld_insert_block(g, J, tb, rec, k, stats); }
	for(uint32_t k : weld_shuffled(nv, rng)) { WeldGroupHost g = fresh_group(rng, false); weld_lookup_block(g, J, tb, remap, rec, k); }
	if(windex) for(uint32_t k : weld_shuffled(nc, rng)) { WeldGroupHost g = fresh_group(rng, false); weld_index_block(g, J, remap, windex, rec, k); }
}

} // namespace corto_hip

extern "C" int crthip_weld_model(const int32_t *position, const void *index, uint32_t index_u16, uint32_t nface, uint32_t nvert, uint32_t *remap, uint32_t *windex,
                                 crthip_weld_counts *counts, uint64_t *stats, int which, uint32_t seed) {
	if((which != 0 && which != 1) || (nvert && !position) || (nface && !index)) return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_weld_model: null position or index, or an unknown partition");
	if((uint64_t)nface*3 > 0xFFFFFFFFull) return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_weld_model: 3*nface does not fit 32 bits");
	crthip_weld_counts rec{0, 0, 0, 0};
	WeldStats st{0, 0};
	uint32_t none = 0;                                                    // (a blob without vertices has no remap word to point at)
	if(nvert || nface) {
		// (the binding's checks: host arrays of exactly nvert and 3*nface words, no device record)
		crthip_weld_binding w{nvert ? remap : &none, nface ? windex : nullptr, nullptr, nvert, nface*3, 0u, 0u};
		if(const char *why = weld_binding_error(&w, nvert, nface)) return ctx_fail(CRTHIP_E_ARGUMENT, why);
		if(which == 0 && !weld_in_blob(nvert)) return ctx_fail(CRTHIP_E_LIMIT, "crthip_weld_model: the blob's table does not fit weld_blob's LDS (partition 1 takes it)");
		WeldIn J; J.position = position; J.index = index; J.index_u16 = index_u16 ? 1u : 0u; J.nface = nface; J.nvert = nvert;
		try {
			weld_model(J, w.remap, w.index, &rec, &st, which, seed);
		} catch(const std::bad_alloc &) {
			return ctx_fail(CRTHIP_E_NOMEM, nullptr);
		}
	}
	if(counts) *counts = rec;
	if(stats) { stats[0] = st.total; stats[1] = st.longest; }
	return CRTHIP_OK;
}
