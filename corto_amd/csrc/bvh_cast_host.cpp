// bvh_cast_host.cpp — the test hook of crthip_bvh_cast (crthip_bvh_cast_model): bvh_cast.h on the host in k_bvh_cast.hip's partition - one
// workgroup of 64 segments after another, each with a stack block of exactly the kernel's size (LDS is not zeroed on the device either), so
// that a sanitizer sees a step past it.  And the checks of a set that the call and the hook share.
#include <new>
#include <string>
#include <vector>

#include "../../include/corto_hip.h"
#include "encoder_internal.h"
#include "bvh_cast.h"

using namespace corto_hip;

namespace corto_hip {

// a set's own checks, in the contract's order; where the memory is, is the call's to ask (bvh_cast.cpp)
const char *bvh_cast_set_error(const crthip_bvh_cast_set *s) {
	auto bad = [](const void *p, uintptr_t align) { return !p || ((uintptr_t)p & (align - 1)); };
	const uintptr_t ialign = s->index_format == CRTHIP_FMT_UINT16 ? 2 : 4;   // (an unknown format is refused below; its index is held to 4 bytes)
	if(s->nseg) {
		if(bad(s->nodes, 16)) return "nodes is NULL or not 16-byte aligned";
		if(bad(s->position, 2)) return "position is NULL or not 2-byte aligned";
		if(bad(s->index, ialign)) return "index is NULL or not aligned to an entry";
		if(s->transform && ((uintptr_t)s->transform & 15)) return "transform is not 16-byte aligned";
		if(bad(s->segments, 16)) return "segments is NULL or not 16-byte aligned";
		if(bad(s->hits, 16)) return "hits is NULL or not 16-byte aligned";
	}
	if(!s->nface || s->nface > 0x7FFFFFFFu) return "nface is 0, or 2*nface - 1 does not fit 32 bits";
	if(s->index_format != CRTHIP_FMT_UINT32 && s->index_format != CRTHIP_FMT_UINT16) return "index_format is neither CRTHIP_FMT_UINT32 nor CRTHIP_FMT_UINT16";
	if(s->pos_stride && (s->pos_stride < 6 || (s->pos_stride & 1))) return "pos_stride is neither 0 nor even and at least 6";
	if(s->flags & ~CAST_FLAGS) return "unknown flags";
	if(s->reserved) return "reserved is not 0";
	return nullptr;
}

struct CastCount { uint64_t nodes = 0, faces = 0; WELD_HD void node() { nodes++; } WELD_HD void face() { faces++; } };

static void cast_model(const crthip_bvh_cast_set &s, crthip_cast_hit *hits, uint64_t *stats) {
	CastIn J;
	J.nodes = (const uint8_t *)s.nodes; J.position = (const uint8_t *)s.position; J.index = s.index;
	for(int c = 0; c < 3; c++) J.base[c] = s.base[c];
	J.stride = bvh_cast_stride(&s); J.nvert = s.nvert; J.nface = s.nface; J.index_u16 = s.index_format == CRTHIP_FMT_UINT16; J.flags = s.flags;
	CastCount count;
	const uint32_t nblocks = (uint32_t)(((uint64_t)s.nseg + CAST_THREADS - 1)/CAST_THREADS);
	for(uint32_t b = 0; b < nblocks; b++) {
		std::vector<uint32_t> lds(CAST_LDS_WORDS, 0xA5A5A5A5u);
		for(uint32_t t = 0; t < CAST_THREADS; t++) {
			const uint64_t i = (uint64_t)b*CAST_THREADS + t;
			if(i >= s.nseg) break;
			cast_segment(J, (const uint8_t *)s.transform, (const uint8_t *)s.segments, (uint8_t *)hits, CastStack{lds.data(), t}, (uint32_t)i, count);
		}
	}
	if(stats) { stats[0] = count.nodes; stats[1] = count.faces; }
}

} // namespace corto_hip

extern "C" int crthip_bvh_cast_model_stats(const crthip_bvh_cast_set *set, crthip_cast_hit *hits, uint64_t *stats) {
	if(!set) return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_bvh_cast_model: set is NULL");
	crthip_bvh_cast_set s = *set;
	s.hits = hits;
	if(const char *why = bvh_cast_set_error(&s)) return ctx_fail(CRTHIP_E_ARGUMENT, (std::string("crthip_bvh_cast_model: ") + why).c_str());
	try {
		cast_model(s, hits, stats);
	} catch(const std::bad_alloc &) {
		return ctx_fail(CRTHIP_E_NOMEM, nullptr);
	}
	return CRTHIP_OK;
}

extern "C" int crthip_bvh_cast_model(const crthip_bvh_cast_set *set, crthip_cast_hit *hits) { return crthip_bvh_cast_model_stats(set, hits, nullptr); }
