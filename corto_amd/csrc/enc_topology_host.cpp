// enc_topology_host.cpp — the test hooks of the encoder's device topology pass: the rule that picks LDS or global walk state, and the
// stages of enc_topology.h run on the host by a team of one thread (the same source k_encode_topo.hip compiles for the device), next
// to the host encoder's own pass (encoder.cpp) for comparison.
#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/corto_hip.h"
#include "enc_topology.h"
#include "encoder_internal.h"

using namespace corto_hip;

static_assert(CRTHIP_TOPOLOGY_CLERS_CAP(1000u) == 7064ull && CRTHIP_TOPOLOGY_SPLIT_CAP(1000u) == 4004ull, "the header's bounds are enc_topology.h's");

namespace {

int model_device_source(const crthip_mesh *m, bool index16, crthip_topology_result *r) {
	const uint32_t nvert = m->nvert, nface = m->nface;
	if(enc_topo_clers_cap(nface) != CRTHIP_TOPOLOGY_CLERS_CAP(nface) || enc_topo_split_cap(nface) != CRTHIP_TOPOLOGY_SPLIT_CAP(nface)) return CRTHIP_E_ARGUMENT;
	const uint32_t one_group[1] = {nface};
	const bool lds = enc_topo_fits_lds(nvert, nface);
	std::vector<uint32_t> first((size_t)nvert + 1), cursor(nvert), twin((size_t)nface*3), split(enc_topo_split_cap(nface));
	std::vector<EncTopoSide> sides((size_t)nface*3);
	std::vector<uint8_t> image(lds ? enc_topo_state_bytes<uint16_t>(nface, nvert) : enc_topo_state_bytes<uint32_t>(nface, nvert));
	EncTopoRecord rec;
	memset(&rec, 0, sizeof(rec));
	EncTopoJob J;
	memset(&J, 0, sizeof(J));
	J.index = m->index; J.gend_in = m->ngroups ? m->group_end : one_group; J.ngroups = m->ngroups ? m->ngroups : 1u;
	J.faces = r->faces; J.gend_out = r->group_end;
	J.first = first.data(); J.cursor = cursor.data(); J.sides = sides.data(); J.twin = twin.data();
	J.state = image.data(); J.quads = r->quads; J.clers = r->clers; J.split = split.data();
	J.split_packed = r->split_words; J.split_cursor = nullptr;
	J.rec = &rec; J.nvert = nvert; J.nface = nface; J.index16 = index16;
	EncTopoHostTeam T;
	enc_topo_compact(T, J);
	enc_topo_pair(T, J);
	if(lds) enc_topo_walk<uint16_t>(T, J, image.data()); else enc_topo_walk<uint32_t>(T, J, image.data());
	if(rec.status) return rec.status;
	if(rec.split_words) memcpy(r->split_words, split.data(), (size_t)rec.split_words*4);
	r->nvert = rec.nvert; r->nface = rec.nface; r->ngroups = J.ngroups; r->max_front = rec.max_front; r->nclers = rec.nclers;
	r->split_bits = rec.split_bits; r->nsplit_words = rec.split_words; r->lds = lds;
	return CRTHIP_OK;
}

int model_host_pass(const crthip_mesh *m, crthip_topology_result *r) {
	TopologyModel t;
	topology_host_model(m, t);
	if(t.clers.size() > CRTHIP_TOPOLOGY_CLERS_CAP(m->nface) || t.split_words.size() > CRTHIP_TOPOLOGY_SPLIT_CAP(m->nface) ||
	   t.faces.size() > (size_t)m->nface*3 || t.quads.size() > (size_t)m->nvert*4 || t.group_end.size() > std::max(m->ngroups, 1u))
		return ctx_fail(CRTHIP_E_LIMIT, "crthip_encode_topology_model: the pass left its bounds");
	if(!t.faces.empty()) memcpy(r->faces, t.faces.data(), t.faces.size()*4);
	if(!t.group_end.empty()) memcpy(r->group_end, t.group_end.data(), t.group_end.size()*4);
	if(!t.quads.empty()) memcpy(r->quads, t.quads.data(), t.quads.size()*4);
	if(!t.clers.empty()) memcpy(r->clers, t.clers.data(), t.clers.size());
	if(!t.split_words.empty()) memcpy(r->split_words, t.split_words.data(), t.split_words.size()*4);
	r->nvert = t.nvert; r->nface = t.nface; r->ngroups = (uint32_t)t.group_end.size(); r->max_front = t.max_front;
	r->nclers = (uint32_t)t.clers.size(); r->split_bits = (uint32_t)t.split_bits; r->nsplit_words = (uint32_t)t.split_words.size(); r->lds = 0;
	return CRTHIP_OK;
}

} // namespace

extern "C" int crthip_encode_topology_fits_lds(const crthip_mesh *m) {
	return m && m->index && enc_topo_fits_lds(m->nvert, m->nface) ? 1 : 0;
}

extern "C" int crthip_encode_topology_model(const crthip_mesh *m, int which, crthip_topology_result *r) {
	return crthip_encode_topology_model_layout(m, nullptr, which, r);
}

// the index alone matters to the pass: a uint16 one is widened for the host pass and read as it is by the device source
extern "C" int crthip_encode_topology_model_layout(const crthip_mesh *m, const crthip_mesh_layout *layout, int which, crthip_topology_result *r) {
	if(which != 0 && which != 1) return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_encode_topology_model: which must be 0 (host pass) or 1 (device source)");
	if(!r || !r->faces || !r->group_end || !r->quads || !r->clers || !r->split_words) return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_encode_topology_model: null buffer");
	{ const int e = encode_check(m, false); if(e) return e; }
	MeshRead rd;
	{ const int e = layout_resolve(m, nullptr, layout, rd); if(e) return e; }
	{ const int e = index_range_host(m, rd); if(e) return e; }
	if(!m->index || !m->nface) return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_encode_topology_model: a point cloud has no topology pass");
	try {
		if(which == 1) return model_device_source(m, rd.index16, r);
		if(!rd.index16) return model_host_pass(m, r);
		std::vector<uint32_t> wide((size_t)m->nface*3);
		for(size_t i = 0; i < wide.size(); i++) wide[i] = ((const uint16_t *)m->index)[i];
		crthip_mesh w = *m;
		w.index = wide.data();
		return model_host_pass(&w, r);
	} catch(const std::bad_alloc &) {
		return ctx_fail(CRTHIP_E_NOMEM, nullptr);
	} catch(...) {
		return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_encode_topology_model: internal error");
	}
}
