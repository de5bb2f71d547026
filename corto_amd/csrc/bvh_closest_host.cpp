// bvh_closest_host.cpp — the test hook of crthip_bvh_closest (crthip_bvh_closest_model): bvh_closest.h on the host in k_bvh_closest.hip's
// partition - one workgroup of 64 points after another, each with a stack block of exactly the kernel's size (LDS is not zeroed on the device
// either), so that a sanitizer sees a step past it.  The stats hook also runs the walk the kernel does not: the children in the nodes' own
// order, to count against.  And the checks of a set that the call and the hook share.
#include <new>
#include <string>
#include <vector>

#include "../../include/corto_hip.h"
#include "encoder_internal.h"
#include "bvh_closest.h"

using namespace corto_hip;

namespace corto_hip {

// a set's own checks, in the contract's order; where the memory is, is the call's to ask (bvh_closest.cpp)
const char *bvh_closest_set_error(const crthip_bvh_closest_set *s) {
	auto bad = [](const void *p, uintptr_t align) { return !p || ((uintptr_t)p & (align - 1)); };
	const uintptr_t ialign = s->index_format == CRTHIP_FMT_UINT16 ? 2 : 4;   // (an unknown format is refused below; its index is held to 4 bytes)
	if(s->npoint) {
		if(bad(s->nodes, 16)) return "nodes is NULL or not 16-byte aligned";
		if(bad(s->position, 2)) return "position is NULL or not 2-byte aligned";
		if(bad(s->index, ialign)) return "index is NULL or not aligned to an entry";
		if(s->transform && ((uintptr_t)s->transform & 15)) return "transform is not 16-byte aligned";
		if(bad(s->points, 16)) return "points is NULL or not 16-byte aligned";
		if(bad(s->hits, 16)) return "hits is NULL or not 16-byte aligned";
	}
	if(!s->nface || s->nface > 0x7FFFFFFFu) return "nface is 0, or 2*nface - 1 does not fit 32 bits";
	if(s->index_format != CRTHIP_FMT_UINT32 && s->index_format != CRTHIP_FMT_UINT16) return "index_format is neither CRTHIP_FMT_UINT32 nor CRTHIP_FMT_UINT16";
	if(s->pos_stride && (s->pos_stride < 6 || (s->pos_stride & 1))) return "pos_stride is neither 0 nor even and at least 6";
	if(s->flags & ~CLOSEST_FLAGS) return "unknown flags";
	if((s->flags & CRTHIP_CLOSEST_ANY) && !(s->flags & CRTHIP_CLOSEST_WITHIN)) return "flags has CRTHIP_CLOSEST_ANY without CRTHIP_CLOSEST_WITHIN";
	if(s->reserved) return "reserved is not 0";
	return nullptr;
}

struct ClosestCount { uint64_t nodes = 0, faces = 0; WELD_HD void node() { nodes++; } WELD_HD void face() { faces++; } };

static void closest_model(const crthip_bvh_closest_set &s, crthip_closest_hit *hits, uint64_t *stats, bool near) {
	CastIn J;
	J.nodes = (const uint8_t *)s.nodes; J.position = (const uint8_t *)s.position; J.index = s.index;
	for(int c = 0; c < 3; c++) J.base[c] = s.base[c];
	J.stride = bvh_closest_stride(&s); J.nvert = s.nvert; J.nface = s.nface; J.index_u16 = s.index_format == CRTHIP_FMT_UINT16; J.flags = s.flags;
	ClosestCount count;
	const uint32_t nblocks = (uint32_t)(((uint64_t)s.npoint + CAST_THREADS - 1)/CAST_THREADS);
	for(uint32_t b = 0; b < nblocks; b++) {
		std::vector<uint32_t> lds(CAST_LDS_WORDS, 0xA5A5A5A5u);
		for(uint32_t t = 0; t < CAST_THREADS; t++) {
			const uint64_t i = (uint64_t)b*CAST_THREADS + t;
			if(i >= s.npoint) break;
			const CastStack S{lds.data(), t};
			if(near) closest_point<true>(J, (const uint8_t *)s.transform, (const uint8_t *)s.points, (uint8_t *)hits, S, (uint32_t)i, count);
			else closest_point<false>(J, (const uint8_t *)s.transform, (const uint8_t *)s.points, (uint8_t *)hits, S, (uint32_t)i, count);
		}
	}
	if(stats) { stats[0] = count.nodes; stats[1] = count.faces; }
}

} // namespace corto_hip

extern "C" int crthip_bvh_closest_model_stats(const crthip_bvh_closest_set *set, crthip_closest_hit *hits, uint64_t *stats, uint32_t order) {
	if(!set) return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_bvh_closest_model: set is NULL");
	if(order > 1u) return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_bvh_closest_model: order is neither 0 nor 1");
	crthip_bvh_closest_set s = *set;
	s.hits = hits;
	if(const char *why = bvh_closest_set_error(&s)) return ctx_fail(CRTHIP_E_ARGUMENT, (std::string("crthip_bvh_closest_model: ") + why).c_str());
	try {
		closest_model(s, hits, stats, order == 0u);
	} catch(const std::bad_alloc &) {
		return ctx_fail(CRTHIP_E_NOMEM, nullptr);
	}
	return CRTHIP_OK;
}

extern "C" int crthip_bvh_closest_model(const crthip_bvh_closest_set *set, crthip_closest_hit *hits) {
	return crthip_bvh_closest_model_stats(set, hits, nullptr, 0u);
}
