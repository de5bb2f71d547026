// cloud_lod_host.cpp — the test hook of crthip_batch_bind_cloud_lod (crthip_cloud_lod_model): cloud_lod.h on the host in k_cloud_lod.hip's
// partitions, one level - a workgroup's 256 threads walked in a loop at every step, the workgroups of a grid too, all in orders shuffled by the
// seed (lod_group_host.h).  Which point wins a slot's compare-and-swap changes with the seed; every result is a minimum, a maximum, a sum or a scan
// in thread order, so the bytes do not.
#include <new>
#include <vector>

#include "../../include/corto_hip.h"
#include "encoder_internal.h"
#include "cloud_lod.h"
#include "lod_group_host.h"

using namespace corto_hip;

namespace corto_hip {

// which 0: k_cloud_lod_blob (the caller made sure of weld_in_blob); which 1: the five kernels.  rec is never null here.  The scratch is made here
// at exactly the kernels' sizes (LDS is not zeroed on the device either), so that a sanitizer sees a step past it
void cloud_lod_model(const LodIn &J, uint32_t K, uint32_t *remap, uint32_t *points, uint32_t *weight, crthip_cloud_chunk *chunks, crthip_cloud_lod_counts *rec,
	LodStats *stats, int which, uint32_t seed) {
	uint64_t rng = 0x9E3779B97F4A7C15ull ^ seed;
	const uint32_t nvert = J.w.nvert;
	if(which == 0) {
		std::vector<uint32_t> table((size_t)weld_slots(nvert), 0xA5A5A5A5u);
		LodGroupHost g = fresh_group(rng, true);
		cloud_lod_blob(g, J, WeldLdsTable{table.data()}, K, remap, points, weight, chunks, rec, stats);
		return;
	}
	std::vector<uint32_t> table((size_t)weld_slots(nvert), 0u), wacc(nvert, weight ? 0u : 0xA5A5A5A5u);   // (the FillJob in front of cloud_lod_insert)
	const uint32_t nv = weld_vblocks(nvert), nc = chunks ? cloud_lod_chunks_of(nvert, K) : 0u;
	std::vector<uint32_t> blocks(nv, 0xA5A5A5A5u);
	*rec = crthip_cloud_lod_counts{0xA5A5A5A5u, 0xA5A5A5A5u, 0xA5A5A5A5u, 0xA5A5A5A5u};   // (cloud_lod_offsets stores it)
	const WeldMemTable tb{table.data()};
	for(uint32_t k : lod_shuffled(nv, rng)) { LodGroupHost g = fresh_group(rng, false); cloud_lod_insert_block(g, J, tb, k, stats); }
	for(uint32_t k : lod_shuffled(nv, rng)) { LodGroupHost g = fresh_group(rng, false); cloud_lod_lookup_block(g, J, tb, remap, blocks.data(), weight ? wacc.data() : nullptr, k); }
	{ LodGroupHost g = fresh_group(rng, false); cloud_lod_offsets_job(g, nvert, K, chunks != nullptr, blocks.data(), rec); }
	for(uint32_t k : lod_shuffled(nv, rng)) { LodGroupHost g = fresh_group(rng, false); cloud_lod_scatter_block(g, nvert, remap, blocks.data(), wacc.data(), points, weight, k); }
	for(uint32_t c : lod_shuffled(nc, rng)) {
		int32_t acc[6] = {(int32_t)0xA5A5A5A5u, (int32_t)0xA5A5A5A5u, (int32_t)0xA5A5A5A5u, (int32_t)0xA5A5A5A5u, (int32_t)0xA5A5A5A5u, (int32_t)0xA5A5A5A5u};
		LodGroupHost g = fresh_group(rng, false);
		cloud_lod_chunk_block(g, J, K, points, rec, chunks, acc, c);
	}
}

} // namespace corto_hip

extern "C" int crthip_cloud_lod_model(const int32_t *position, uint32_t nvert, uint32_t shift, uint32_t chunk_points, uint32_t *remap, uint32_t *points,
                                      uint32_t *weight, crthip_cloud_chunk *chunks, crthip_cloud_lod_counts *counts, uint64_t *stats, int which, uint32_t seed) {
	if((which != 0 && which != 1) || !position) return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_cloud_lod_model: a null position, or an unknown partition");
	if(!nvert) return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_cloud_lod_model: the cloud has no points");
	// (the binding's checks: one level, host arrays of exactly nvert words and ceil(nvert / K) records, no device record)
	crthip_cloud_lod_binding b{};
	b.levels = 1; b.chunk_points = chunk_points;
	b.level[0] = crthip_cloud_lod_level{remap, points, weight, chunks, nullptr, nvert, cloud_lod_chunks_of(nvert, chunk_points), shift, 0u};
	if(const char *why = cloud_lod_binding_error(&b, nvert)) return ctx_fail(CRTHIP_E_ARGUMENT, why);
	if(which == 0 && !weld_in_blob(nvert)) return ctx_fail(CRTHIP_E_LIMIT, "crthip_cloud_lod_model: the job's table does not fit cloud_lod_blob's LDS (partition 1 takes it)");
	crthip_cloud_lod_counts rec{0, 0, 0, 0};
	LodStats st{0, 0, 0, 0};
	LodIn J; J.w.position = position; J.w.index = nullptr; J.w.index_u16 = 0u; J.w.nface = 0; J.w.nvert = nvert; J.shift = shift;
	try {
		cloud_lod_model(J, chunk_points, remap, points, weight, chunks, &rec, &st, which, seed);
	} catch(const std::bad_alloc &) {
		return ctx_fail(CRTHIP_E_NOMEM, nullptr);
	}
	if(counts) *counts = rec;
	if(stats) { stats[0] = st.vtotal; stats[1] = st.vlongest; }
	return CRTHIP_OK;
}
