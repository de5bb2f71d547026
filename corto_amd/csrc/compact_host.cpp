// compact_host.cpp — the test hook of crthip_batch_bind_compact (crthip_compact_model): compact.h on the host in k_compact.hip's partitions, one
// set - a workgroup's 256 threads walked in a loop at every step, the workgroups of a grid too, all in orders shuffled by the seed
// (lod_group_host.h).  Which corner sets a bit first changes with the seed; every result is an OR, a popcount or a scan in thread order, so the
// bytes do not.
#include <new>
#include <vector>

#include "../../include/corto_hip.h"
#include "encoder_internal.h"
#include "compact.h"
#include "lod_group_host.h"

using namespace corto_hip;

namespace corto_hip {

// which 0: k_compact_blob (the caller made sure of compact_in_blob); which 1: the five kernels; which 2: a cloud set - nothing but the gathers.
// Then k_compact_gather, a grid a gather.  The scratch is made here at exactly the kernels' sizes (LDS is not zeroed on the device either),
// so that a sanitizer sees a step past it.  src_rec: the record the kernels read F (a cloud: `used`) from
void compact_model(const CompactIn &J, const uint32_t *src_rec, uint32_t *newid, uint32_t *order, uint32_t *index, crthip_compact_counts *rec,
	const crthip_compact_model_gather *gathers, uint32_t ngather, int which, uint32_t seed) {
	uint64_t rng = 0x9E3779B97F4A7C15ull ^ seed;
	const uint32_t nvert = J.w.nvert, nface = J.w.nface;
	// (what the planner gives a set without them: an order for its gathers, a newid for its index beyond compact_blob)
	std::vector<uint32_t> own_order, own_newid;
	const uint32_t ocap = J.vcap < nvert ? J.vcap : nvert;
	if(which != 2 && !order && ngather) { own_order.assign(ocap, 0xA5A5A5A5u); order = own_order.data(); }
	if(which == 1 && !newid && index) { own_newid.assign(nvert, 0xA5A5A5A5u); newid = own_newid.data(); }
	if(which == 0) {
		std::vector<uint32_t> mask(compact_words(nvert), 0xA5A5A5A5u), pre(compact_words(nvert), 0xA5A5A5A5u);
		LodGroupHost g = fresh_group(rng, true);
		compact_blob(g, J, mask.data(), pre.data(), newid, order, index, rec);
	} else if(which == 1) {
		std::vector<uint32_t> mask(compact_words(nvert), 0u);                  // (the FillJob in front of compact_mark)
		const uint32_t nv = compact_vblocks(nvert), nc = compact_cblocks(nface);
		std::vector<uint32_t> blocks(nv, 0xA5A5A5A5u);
		*rec = crthip_compact_counts{0xA5A5A5A5u, 0xA5A5A5A5u, 0xA5A5A5A5u, 0xA5A5A5A5u};   // (compact_offsets stores it)
		for(uint32_t k : lod_shuffled(nc, rng)) { LodGroupHost g = fresh_group(rng, false); compact_mark_block(g, J, mask.data(), k); }
		for(uint32_t k : lod_shuffled(nv, rng)) { LodGroupHost g = fresh_group(rng, false); compact_count_block(g, nvert, mask.data(), blocks.data(), k); }
		{ LodGroupHost g = fresh_group(rng, false); compact_offsets_job(g, J, index != nullptr, blocks.data(), rec); }
		for(uint32_t k : lod_shuffled(nv, rng)) { LodGroupHost g = fresh_group(rng, false); compact_place_block(g, J, mask.data(), blocks.data(), newid, order, k); }
		if(index) for(uint32_t k : lod_shuffled(nc, rng)) { LodGroupHost g = fresh_group(rng, false); compact_index_block(g, J, newid, index, k); }
	}
	for(uint32_t q = 0; q < ngather || (which == 2 && q == 0); q++) {
		CompactGatherIn G{};
		G.order = which == 2 ? (const uint32_t *)J.w.index : order;
		G.count_rec = which == 2 ? src_rec : (const uint32_t *)rec;
		G.cloud_rec = which == 2 && q == 0 ? rec : nullptr;
		G.vcap = J.vcap; G.nvert = nvert; G.clip_v = J.clip_v;
		if(q < ngather) {
			const crthip_compact_model_gather &m = gathers[q];
			G.src = (const uint8_t *)m.src; G.dst = (uint8_t *)m.dst; G.E = m.E;
			G.sstride = m.src_stride ? m.src_stride : m.E; G.dstride = m.dst_stride ? m.dst_stride : m.E;
			G.unit = compact_unit((uintptr_t)m.src, (uintptr_t)m.dst, G.E, G.sstride, G.dstride);
		}
		for(uint32_t k : lod_shuffled(compact_gather_blocks(nvert, G.vcap, G.E, G.unit), rng)) { LodGroupHost g = fresh_group(rng, false); compact_gather_block(g, G, k); }
	}
}

} // namespace corto_hip

extern "C" int crthip_compact_model(const void *src, uint32_t src_u16, uint32_t nface, uint32_t faces, uint32_t nvert, uint32_t *newid, uint32_t *order,
                                    uint32_t *index, uint32_t vertex_capacity, uint32_t index_capacity, crthip_compact_counts *counts,
                                    const crthip_compact_model_gather *gathers, uint32_t ngather, int which, uint32_t seed) {
	if(which < 0 || which > 2 || (!src && nface) || faces > nface) return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_compact_model: an unknown partition, a null source, or faces above nface");
	if(ngather > CRTHIP_COMPACT_MAX_GATHERS || (ngather && !gathers)) return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_compact_model: ngather is above CRTHIP_COMPACT_MAX_GATHERS");
	for(uint32_t q = 0; q < ngather; q++) {
		const crthip_compact_model_gather &m = gathers[q];
		if(!m.src || !m.dst || !m.E || (m.src_stride && m.src_stride < m.E) || (m.dst_stride && m.dst_stride < m.E))
			return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_compact_model: a gather with a null pointer, no bytes or a stride below them");
	}
	if(which == 2 && (newid || order || index || src_u16)) return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_compact_model: a cloud set has no newid, order or index");
	if(which == 0 && !compact_in_blob(nvert, nface)) return ctx_fail(CRTHIP_E_LIMIT, "crthip_compact_model: the set is beyond compact_blob's 8 192 vertices and faces (partition 1 takes it)");
	crthip_compact_counts rec{0, 0, 0, 0};
	const uint32_t src_rec[4] = {0xA5A5A5A5u, faces, 0xA5A5A5A5u, 0xA5A5A5A5u};   // (a level's record: word 1 is all the kernels read)
	CompactIn J; J.w.position = nullptr; J.w.index = src; J.w.index_u16 = src_u16; J.w.nface = nface; J.w.nvert = nvert;
	J.src_rec = src_rec; J.vcap = vertex_capacity; J.icap = index_capacity; J.clip_v = (order || ngather) ? 1u : 0u;
	try {
		compact_model(J, src_rec, newid, order, index, &rec, gathers, ngather, which, seed);
	} catch(const std::bad_alloc &) {
		return ctx_fail(CRTHIP_E_NOMEM, nullptr);
	}
	if(counts) *counts = rec;
	return CRTHIP_OK;
}
