// meshlet_host.cpp — the host's part of crthip_batch_bind_meshlets: the segment table and the capacity bound (mlt_plan, crthip_meshlet_bound), and
// the test hook crthip_meshlet_model: meshlet.h on the host in k_meshlet.hip's partitions - a wave's 64 lanes walked in a loop at every step, the
// segments and the placement's workgroups and threads too, all in orders shuffled by the seed (segments are independent, a step's lanes meet
// only through the table's compare-and-swap and min, and every moved word has one writer: any order gives the same bytes).
#include <algorithm>
#include <new>
#include <vector>

#include "../../include/corto_hip.h"
#include "encoder_internal.h"
#include "meshlet.h"

using namespace corto_hip;

namespace corto_hip {

bool mlt_plan(uint32_t nface, uint32_t ngroups, const uint32_t *group_end, uint32_t max_vertices, uint32_t max_triangles, uint32_t segment_faces,
              std::vector<MltSeg> *segs, crthip_meshlet_counts &bound) {
	bound = crthip_meshlet_counts{0, 0, 0, 0};
	if(!mlt_params_ok(max_vertices, max_triangles, segment_faces) || (ngroups && !group_end)) return false;
	const uint32_t tmin = mlt_tmin(max_vertices, max_triangles);
	std::vector<uint32_t> sorted((size_t)ngroups + 1);
	uint64_t mb = 0, nseg = 0;
	if(segs) segs->clear();
	mlt_segments(nface, ngroups, group_end, segment_faces, sorted.data(), [&](uint32_t f0, uint32_t f1) {
		if(segs && mb <= 0x3FFFFFFFu) segs->push_back(MltSeg{f0, f1, (uint32_t)mb, (uint32_t)((3ull*f0 + 3ull*mb + 3) & ~3ull)});
		mb += (f1 - f0 + tmin - 1)/tmin; nseg++;
	});
	const uint64_t tb = 3ull*nface + 3ull*mb;
	if(tb + 8 > 0xFFFFFFFFull || 3ull*nface > 0xFFFFFFFFull) return false;
	bound.meshlets = (uint32_t)mb; bound.vertices = 3*nface; bound.triangle_bytes = (uint32_t)tb; bound.segments = (uint32_t)nseg;
	return true;
}

namespace {

std::vector<uint32_t> mlt_shuffled(uint32_t n, uint64_t &x) {
	std::vector<uint32_t> order(n);
	for(uint32_t i = 0; i < n; i++) order[i] = i;
	for(uint32_t i = n; i > 1; i--) {                                     // Fisher-Yates on a 64-bit LCG
		x = x*6364136223846793005ull + 1442695040888963407ull;
		std::swap(order[i - 1], order[(uint32_t)((x >> 33) % i)]);
	}
	return order;
}

// the wave as mlt_segment sees it, on the host: 64 lane states, every step's lanes in a fresh order
struct MltWaveHost {
	MltLane L[MLT_WAVE];
	uint64_t *rng;
	template <class F> void each(F f) { for(uint32_t lane : mlt_shuffled(MLT_WAVE, *rng)) f(lane, L[lane]); }
	void window(const MltIn &J, uint32_t pos, uint32_t, uint32_t nwin) { each([&](uint32_t lane, MltLane &l) { l.in = lane < nwin; if(l.in) mlt_load_face(J, pos + lane, l.v); }); }
	void sync() {}
	void scan() { uint32_t s = 0; for(uint32_t l = 0; l < MLT_WAVE; l++) { s += L[l].cnt; L[l].incl = s; } }
	template <class P> uint32_t first(P pred) { for(uint32_t l = 0; l < MLT_WAVE; l++) if(pred(l, L[l])) return l; return MLT_WAVE; }
	uint32_t incl_of(uint32_t l) { return L[l].incl; }
};

MltCount run_segment(const MltIn &J, const MltSeg &sg, const MltOut &O, uint64_t &rng) {
	std::vector<MltWaveMem> W(1);                                         // (value-initialised: the table starts out empty)
	MltWaveHost x{}; x.rng = &rng;
	return mlt_segment(x, W[0], J, sg, O);
}

} // namespace

// which 0: k_meshlet_blob - in place for one segment, else scratch, then every thread of the workgroup moves its share of every segment;
// which 1: k_meshlet_segments, then k_meshlet_place's workgroups
void meshlet_model(const MltIn &J, uint32_t nface, const std::vector<MltSeg> &segs, const crthip_meshlet_counts &bound, const MltOut &F,
                   crthip_meshlet_counts &rec, int which, uint32_t seed) {
	uint64_t rng = 0x9E3779B97F4A7C15ull ^ seed;
	const uint32_t nseg = (uint32_t)segs.size();
	rec = crthip_meshlet_counts{0, 0, 0, nseg};
	if(which == 0 && nseg <= 1) {
		if(nseg) { const MltCount c = run_segment(J, segs[0], F, rng); rec.meshlets = c.meshlets; rec.vertices = c.vertices; rec.triangle_bytes = c.triangle_bytes; }
		return;
	}
	const MltScratchLayout lay = mlt_scratch_layout(nface, bound);
	std::vector<uint64_t> block((size_t)(lay.total + 7)/8, 0xA5A5A5A5A5A5A5A5ull);   // (scratch is not zeroed on the device either)
	uint8_t *s = (uint8_t *)block.data();
	const MltScratch P{(crthip_meshlet *)s, (uint32_t *)(s + lay.vertices), (uint32_t *)(s + lay.triangles), (MltCount *)(s + lay.counts)};
	for(uint32_t k : mlt_shuffled(nseg, rng)) P.counts[k] = run_segment(J, segs[k], mlt_provisional(P, segs[k]), rng);
	MltCount total{0, 0, 0, 0};
	if(which == 0) {
		const uint32_t nthr = 64*std::min(nseg, 4u);
		for(uint32_t k = 0; k < nseg; k++) {
			for(uint32_t tid : mlt_shuffled(nthr, rng)) mlt_place(P, F, segs[k], total, P.counts[k], tid, nthr);
			total = mlt_add(total, P.counts[k]);
		}
	} else {
		for(uint32_t k : mlt_shuffled(nseg, rng)) {
			MltCount before{0, 0, 0, 0};
			for(uint32_t i = 0; i < k; i++) before = mlt_add(before, P.counts[i]);
			for(uint32_t tid : mlt_shuffled(MLT_PLACE_THREADS, rng)) mlt_place(P, F, segs[k], before, P.counts[k], tid, MLT_PLACE_THREADS);
			if(k + 1 == nseg) total = mlt_add(before, P.counts[k]);
		}
	}
	rec.meshlets = total.meshlets; rec.vertices = total.vertices; rec.triangle_bytes = total.triangle_bytes;
}

// what crthip_batch_bind_meshlets and the hook ask of a binding's parameters, buffers and capacities; null: fine
const char *meshlet_binding_error(const crthip_meshlet_binding *m, bool have_bound, const crthip_meshlet_counts &bound) {
	if(!mlt_params_ok(m->max_vertices, m->max_triangles, m->segment_faces))
		return "meshlets: max_vertices is 3..255, max_triangles 1..512, segment_faces 0 or 1..65536";
	if(!have_bound) return "meshlets: the capacity bound of this index does not fit 32 bits";
	if(!m->meshlets || !m->vertices || !m->triangles) return "meshlets: a buffer is NULL";
	if((uintptr_t)m->meshlets % 16 || (uintptr_t)m->vertices % 4 || (uintptr_t)m->triangles % 4 || (uintptr_t)m->counts % 16)
		return "meshlets: the records (and the counts) are 16-byte aligned, vertices and triangles 4-byte aligned";
	if(m->meshlet_capacity < bound.meshlets) return "meshlets: meshlet_capacity is below crthip_meshlet_bound";
	if(m->vertex_capacity < bound.vertices) return "meshlets: vertex_capacity is below crthip_meshlet_bound";
	if(m->triangle_capacity < bound.triangle_bytes) return "meshlets: triangle_capacity is below crthip_meshlet_bound";
	return nullptr;
}

} // namespace corto_hip

extern "C" int crthip_meshlet_bound(uint32_t nface, uint32_t ngroups, const uint32_t *group_end, uint32_t max_vertices, uint32_t max_triangles,
                                    uint32_t segment_faces, crthip_meshlet_counts *out) {
	if(!out) return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_meshlet_bound: out is NULL");
	try {
		if(!mlt_plan(nface, ngroups, group_end, max_vertices, max_triangles, segment_faces, nullptr, *out))
			return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_meshlet_bound: max_vertices is 3..255, max_triangles 1..512, segment_faces 0 or 1..65536, group_end not NULL, the bound within 32 bits");
		return CRTHIP_OK;
	} catch(const std::bad_alloc &) {
		return ctx_fail(CRTHIP_E_NOMEM, nullptr);
	}
}

extern "C" int crthip_meshlet_model(const void *index, uint32_t index_u16, uint32_t nface, uint32_t ngroups, const uint32_t *group_end,
                                    const crthip_meshlet_binding *m, crthip_meshlet_counts *counts, int which, uint32_t seed) {
	if((which != 0 && which != 1) || !m || !counts || (nface && !index) || (ngroups && !group_end))
		return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_meshlet_model: null argument or an unknown partition");
	try {
		std::vector<MltSeg> segs;
		crthip_meshlet_counts bound;
		const bool ok = mlt_params_ok(m->max_vertices, m->max_triangles, m->segment_faces) &&
			mlt_plan(nface, ngroups, group_end, m->max_vertices, m->max_triangles, m->segment_faces, &segs, bound);
		if(const char *why = meshlet_binding_error(m, ok, bound)) return ctx_fail(CRTHIP_E_ARGUMENT, why);
		MltIn J; J.faces = index; J.faces_u16 = index_u16 ? 1u : 0u; J.max_vertices = m->max_vertices; J.max_triangles = m->max_triangles;
		crthip_meshlet_counts rec;
		meshlet_model(J, nface, segs, bound, MltOut{m->meshlets, m->vertices, (uint32_t *)m->triangles}, rec, which, seed);
		*counts = rec;
		if(m->counts) *m->counts = rec;
		return CRTHIP_OK;
	} catch(const std::bad_alloc &) {
		return ctx_fail(CRTHIP_E_NOMEM, nullptr);
	}
}
