// lod_host.cpp — the test hook of crthip_batch_bind_lod (crthip_lod_model): lod.h on the host in k_lod.hip's partitions, one level - a workgroup's
// 256 threads walked in a loop at every step, the workgroups of a grid too, all in orders shuffled by the seed.  Which item wins a slot's
// compare-and-swap changes with the seed; every result is a minimum, a sum or a scan in thread order, so the bytes do not.
#include <algorithm>
#include <new>
#include <vector>

#include "../../include/corto_hip.h"
#include "encoder_internal.h"
#include "lod.h"
#include "lod_group_host.h"                                                  // (LodGroupHost, fresh_group, lod_shuffled)

using namespace corto_hip;

namespace corto_hip {

// which 0: k_lod_blob (the caller made sure of lod_in_blob); which 1: the six kernels.  rec is never null here.  The scratch is made here at
// exactly the kernels' sizes (LDS is not zeroed on the device either), so that a sanitizer sees a step past it
void lod_model(const LodIn &J, uint32_t *remap, uint32_t *index, crthip_lod_counts *rec, LodStats *stats, int which, uint32_t seed) {
	uint64_t rng = 0x9E3779B97F4A7C15ull ^ seed;
	const uint32_t nvert = J.w.nvert, nface = J.w.nface;
	std::vector<uint32_t> tri((size_t)nface*3, 0xA5A5A5A5u);
	if(which == 0) {
		std::vector<uint32_t> table((size_t)lod_table_slots(nvert, nface), 0xA5A5A5A5u);
		LodGroupHost g = fresh_group(rng, true);
		lod_blob(g, J, WeldLdsTable{table.data()}, remap, tri.data(), index, rec, stats);
		return;
	}
	std::vector<uint32_t> vtable((size_t)weld_slots(nvert), 0u), ftable((size_t)weld_slots(nface), 0u);   // (the FillJob in front of lod_insert)
	const uint32_t nv = weld_vblocks(nvert), nf = lod_fblocks(nface);
	std::vector<uint32_t> blocks(nf, 0xA5A5A5A5u);
	*rec = crthip_lod_counts{0xA5A5A5A5u, 0xA5A5A5A5u, 0xA5A5A5A5u, 0xA5A5A5A5u};   // (lod_insert's first workgroup stores it)
	const WeldMemTable vtb{vtable.data()}, ftb{ftable.data()};
	for(uint32_t k : lod_shuffled(nv, rng)) { LodGroupHost g = fresh_group(rng, false); lod_insert_block(g, J, vtb, rec, k, stats); }
	for(uint32_t k : lod_shuffled(nv, rng)) { LodGroupHost g = fresh_group(rng, false); lod_lookup_block(g, J, vtb, remap, rec, k); }
	for(uint32_t k : lod_shuffled(nf, rng)) { LodGroupHost g = fresh_group(rng, false); lod_faces_block(g, J, ftb, remap, tri.data(), k, stats); }
	for(uint32_t k : lod_shuffled(nf, rng)) { LodGroupHost g = fresh_group(rng, false); lod_keep_block(g, J, ftb, tri.data(), blocks.data(), rec, k); }
	{ LodGroupHost g = fresh_group(rng, false); lod_offsets_job(g, nface, blocks.data(), rec); }
	for(uint32_t k : lod_shuffled(nf, rng)) { LodGroupHost g = fresh_group(rng, false); lod_scatter_block(g, J, tri.data(), blocks.data(), index, k); }
}

} // namespace corto_hip

extern "C" int crthip_lod_model(const int32_t *position, const void *index, uint32_t index_u16, uint32_t nface, uint32_t nvert, uint32_t shift, uint32_t *remap,
                                uint32_t *lod_index, crthip_lod_counts *counts, uint64_t *stats, int which, uint32_t seed) {
	if((which != 0 && which != 1) || (nvert && !position) || (nface && !index)) return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_lod_model: null position or index, or an unknown partition");
	if((uint64_t)nface*3 > 0xFFFFFFFFull) return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_lod_model: 3*nface does not fit 32 bits");
	crthip_lod_counts rec{0, 0, 0, 0};
	LodStats st{0, 0, 0, 0};
	uint32_t none[2] = {0, 0};                                            // (a blob without vertices or faces has no word to point at)
	if(nvert || nface) {
		// (the binding's checks: one level, host arrays of exactly nvert and 3*nface words, no device record)
		crthip_lod_binding b{};
		b.levels = 1;
		b.level[0] = crthip_lod_level{nvert ? remap : &none[0], nface ? lod_index : &none[1], nullptr, nvert, nface*3, shift, 0u};
		if(const char *why = lod_binding_error(&b, nvert, nface)) return ctx_fail(CRTHIP_E_ARGUMENT, why);
		if(which == 0 && !lod_in_blob(nvert, nface)) return ctx_fail(CRTHIP_E_LIMIT, "crthip_lod_model: the job's tables do not fit lod_blob's LDS (partition 1 takes it)");
		LodIn J; J.w.position = position; J.w.index = index; J.w.index_u16 = index_u16 ? 1u : 0u; J.w.nface = nface; J.w.nvert = nvert; J.shift = shift;
		try {
			lod_model(J, b.level[0].remap, b.level[0].index, &rec, &st, which, seed);
		} catch(const std::bad_alloc &) {
			return ctx_fail(CRTHIP_E_NOMEM, nullptr);
		}
	}
	if(counts) *counts = rec;
	if(stats) { stats[0] = st.vtotal; stats[1] = st.vlongest; stats[2] = st.ftotal; stats[3] = st.flongest; }
	return CRTHIP_OK;
}
