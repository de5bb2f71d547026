// bvh_host.cpp — the test hook of crthip_batch_bind_bvh (crthip_bvh_model): bvh.h on the host in k_bvh.hip's partitions - a workgroup's 256
// threads walked in a loop at every step, the workgroups of a grid too, all in orders shuffled by the seed (lod_group_host.h).  Which thread
// arrives first at a node, and which face raises an extent word first, changes with the seed; every result is a union, a maximum or a sum, and
// the sort is stable, so the bytes do not.
#include <new>
#include <vector>

#include "../../include/corto_hip.h"
#include "encoder_internal.h"
#include "bvh.h"
#include "lod_group_host.h"

using namespace corto_hip;

namespace corto_hip {

// which 0: k_bvh_blob (the caller made sure of bvh_in_blob); which 1: the kernels over scratch.  What stands for LDS and for scratch is made here
// at exactly the kernels' sizes (LDS is not zeroed on the device either), so that a sanitizer sees a step past it
void bvh_model(const WeldIn &J, crthip_bvh_node *nodes, uint32_t *parent, uint32_t *order, crthip_bvh_counts *rec, int which, uint32_t seed) {
	uint64_t rng = 0x9E3779B97F4A7C15ull ^ seed;
	const uint32_t F = J.nface;
	if(which == 0) {
		std::vector<uint32_t> lds(bvh_blob_lds_bytes(F)/4, 0xA5A5A5A5u);
		LodGroupHost g = fresh_group(rng, true);
		bvh_blob(g, J, (uint8_t *)lds.data(), nodes, parent, order, rec);
		return;
	}
	const BvhScratchLayout lay = bvh_scratch_layout(F, !parent);
	std::vector<uint32_t> scratch((size_t)(lay.total/4), 0xA5A5A5A5u);
	for(uint64_t k = 0; k < lay.zero_bytes/4; k++) scratch[(size_t)k] = 0u;   // (the FillJob in stage E)
	const BvhBig S = bvh_big_carve((uint8_t *)scratch.data(), F);
	if(!parent) parent = scratch.data() + lay.parent/4;
	const uint32_t nb = bvh_fblocks(F), nt = bvh_tiles(F);
	for(uint32_t k : lod_shuffled(nb, rng)) { std::vector<uint32_t> le(BVH_EXT_WORDS, 0xA5A5A5A5u); LodGroupHost g = fresh_group(rng, false); bvh_boxes_block(g, J, S, le.data(), k); }
	for(uint32_t k : lod_shuffled(nb, rng)) { LodGroupHost g = fresh_group(rng, false); bvh_keys_block(g, J, S, k); }
	for(uint32_t pass = 0; pass < BVH_PASSES; pass++) {
		for(uint32_t k : lod_shuffled(nt, rng)) { std::vector<uint32_t> lh(BVH_DIGITS, 0xA5A5A5A5u); LodGroupHost g = fresh_group(rng, false); bvh_sort_count_tile(g, F, S, lh.data(), pass, k); }
		{ LodGroupHost g = fresh_group(rng, false); bvh_sort_offsets_job(g, F, S); }
		for(uint32_t k : lod_shuffled(nt, rng)) {
			std::vector<uint32_t> lds(BVH_TILE_LDS/4, 0xA5A5A5A5u);
			LodGroupHost g = fresh_group(rng, false);
			bvh_sort_scatter_tile(g, F, S, (uint8_t *)lds.data(), pass, k);
		}
	}
	for(uint32_t k : lod_shuffled(nb, rng)) { LodGroupHost g = fresh_group(rng, false); bvh_tree_block(g, F, S, nodes, parent, order, k); }
	for(uint32_t k : lod_shuffled(nb, rng)) { LodGroupHost g = fresh_group(rng, false); bvh_refit_block(g, J, S, nodes, parent, rec, k); }
}

} // namespace corto_hip

extern "C" int crthip_bvh_model(const int32_t *position, uint32_t nvert, const void *index, uint32_t index_u16, uint32_t nface, crthip_bvh_node *nodes,
                                uint32_t *parent, uint32_t *order, crthip_bvh_counts *counts, int which, uint32_t seed) {
	if((which != 0 && which != 1) || !nface || (nvert && !position) || !index)
		return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_bvh_model: an unknown partition, no faces, or a null position or index");
	if(nface > 0x7FFFFFFFu) return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_bvh_model: 2*nface - 1 does not fit 32 bits");
	// (the binding's checks: host arrays of exactly 2*nface - 1 records and nface words, no device record)
	crthip_bvh_binding v{nodes, parent, order, nullptr, 2*nface - 1, nface, 0u, 0u};
	if(const char *why = bvh_binding_error(&v, nface)) return ctx_fail(CRTHIP_E_ARGUMENT, why);
	if(which == 0 && !bvh_in_blob(nface)) return ctx_fail(CRTHIP_E_LIMIT, "crthip_bvh_model: the blob is beyond bvh_blob's 4 096 faces (partition 1 takes it)");
	crthip_bvh_counts rec{0, 0, 0, 0};
	WeldIn J; J.position = position; J.index = index; J.index_u16 = index_u16 ? 1u : 0u; J.nface = nface; J.nvert = nvert;
	try {
		bvh_model(J, nodes, parent, order, &rec, which, seed);
	} catch(const std::bad_alloc &) {
		return ctx_fail(CRTHIP_E_NOMEM, nullptr);
	}
	if(counts) *counts = rec;
	return CRTHIP_OK;
}
