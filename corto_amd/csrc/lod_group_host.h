// lod_group_host.h — the workgroup as lod.h sees it, on the host: what the test hooks lod_host.cpp and cloud_lod_host.cpp share.  256 thread
// states, every step's threads walked in a fresh order shuffled by the seed, the workgroups of a grid too.
#pragma once
#include <algorithm>
#include <vector>

#include "lod.h"

namespace corto_hip {

namespace {

std::vector<uint32_t> lod_shuffled(uint32_t n, uint64_t &x) {
	std::vector<uint32_t> order(n);
	for(uint32_t i = 0; i < n; i++) order[i] = i;
	for(uint32_t i = n; i > 1; i--) {                                     // Fisher-Yates on a 64-bit LCG
		x = x*6364136223846793005ull + 1442695040888963407ull;
		std::swap(order[i - 1], order[(uint32_t)((x >> 33) % i)]);
	}
	return order;
}

// the workgroup as lod.h sees it, on the host: 256 thread states, every step's threads in a fresh order
struct LodGroupHost {
	LodLane L[LOD_THREADS];
	uint64_t *rng;
	template <class F> void each(F f) { for(uint32_t tid : lod_shuffled(LOD_THREADS, *rng)) f(tid, L[tid]); }
	void sync() {}
	void block_sum() {
		uint32_t s = 0;
		for(uint32_t tid : lod_shuffled(LOD_THREADS, *rng)) s += L[tid].c;
		L[0].c = s;
	}
	void block_scan() {
		uint32_t s = 0;
		for(uint32_t tid = 0; tid < LOD_THREADS; tid++) { L[tid].x = s; s += L[tid].c; }
		for(uint32_t tid = 0; tid < LOD_THREADS; tid++) L[tid].t = s;
	}
	template <class F> void thread0(F f) { f(L[0]); }
};

// a fresh workgroup: its thread states hold garbage, as registers do (the blob kernels clear their own)
LodGroupHost fresh_group(uint64_t &rng, bool cleared) {
	LodGroupHost g;
	for(LodLane &l : g.L) l.c = l.x = l.t = l.run = l.n = l.cells = cleared ? 0u : 0xA5A5A5A5u;
	g.rng = &rng;
	return g;
}

} // namespace

} // namespace corto_hip
