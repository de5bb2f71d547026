// enc_input_host.cpp — the test hook of crthip_encode_batch_resident's input pass (crthip_encode_input_model): the host encoder's own
// loops over a mesh's arrays (encoder.cpp: input_stats_host, what crthip_encode runs) next to the source the device kernels run
// (enc_input_check.h), walked on the host in k_encode_check.hip's partition: runs of EIN_RUN vertices, lanes merged by the shuffle tree,
// waves in order, one partial a tile, the partials folded in EIN_FOLD_LANES stretches and the same tree, the seed first of all; the edge
// terms a tile at a time, added in face order.
#include <cstring>
#include <new>
#include <vector>

#include "../../include/corto_hip.h"
#include "enc_input_check.h"
#include "encoder_internal.h"

using namespace corto_hip;

namespace {

// wave_merge_in_lane_order of k_encode_check.hip: lane i takes lane i + off's box, a lane without a partner its own
void tree64(EncInputBox *lanes) {
	for(uint32_t off = 1; off < 64; off <<= 1) {
		EncInputBox next[64];
		for(uint32_t i = 0; i < 64; i++) { next[i] = lanes[i]; enc_in_box_merge(next[i], lanes[i + off < 64 ? i + off : i]); }
		memcpy(lanes, next, sizeof(next));
	}
}

void box_in_kernel_partition(const EncInputJob &J, EncInputBox &out) {
	const uint32_t nvert = J.nvert, recipe = J.recipe;
	const uint32_t ntiles = (uint32_t)(((uint64_t)nvert + EIN_TILE - 1)/EIN_TILE);
	std::vector<EncInputBox> parts(ntiles);
	for(uint32_t b = 0; b < ntiles; b++) {
		EncInputBox lanes[EIN_THREADS];
		for(uint32_t t = 0; t < EIN_THREADS; t++) {
			const uint64_t v0 = (uint64_t)b*EIN_TILE + (uint64_t)t*EIN_RUN;
			const uint32_t count = v0 + EIN_RUN <= nvert ? EIN_RUN : v0 < nvert ? (uint32_t)(nvert - v0) : 0u;
			float v[3*EIN_RUN] = {};
			for(uint32_t r = 0; r < count; r++) enc_in_box_value(J, enc_in_vertex(J, v0 + r), v + 3*r);
			enc_in_box_run(lanes[t], v, count);
		}
		for(uint32_t w = 0; w < EIN_THREADS/64; w++) tree64(lanes + 64*w);
		for(uint32_t w = 1; w < EIN_THREADS/64; w++) enc_in_box_merge(lanes[0], lanes[64*w]);
		parts[b] = lanes[0];
	}
	EncInputBox fold[EIN_FOLD_LANES];
	for(uint32_t l = 0; l < EIN_FOLD_LANES; l++) enc_in_fold_stretch(fold[l], parts.data(), ntiles, l);
	tree64(fold);
	enc_in_box_seed(out, recipe, J.position);
	enc_in_box_merge(out, fold[0]);
}

// which = 0: the host's scan; which = 1: range_blocks' cut - head, 16-byte groups, tail - each part flagged on its own, as the kernel's lanes do
uint32_t range_flag(const EncInputJob &J, int which) {
	const uint64_t n = (uint64_t)J.nface*3;
	uint32_t bad = 0;
	if(which == 0) { for(uint64_t i = 0; i < n; i++) bad |= enc_in_index(J, i) >= J.nvert; return bad; }
	uint32_t per; uint64_t head, groups, tail;
	enc_in_range_cut(J, n, per, head, groups, tail);
	for(uint64_t i = 0; i < head; i++) bad |= enc_in_index(J, i) >= J.nvert;
	for(uint64_t g = groups; g-- > 0;) for(uint32_t k = 0; k < per; k++) bad |= enc_in_index(J, head + g*per + k) >= J.nvert;
	for(uint64_t i = 0; i < tail; i++) bad |= enc_in_index(J, head + groups*per + i) >= J.nvert;
	return bad;
}

void model(const crthip_mesh *m, const MeshRead *rd, int which, crthip_encode_input_result *r) {
	memset(r, 0, sizeof(*r));
	const EncInputJob J = enc_input_job(m, rd);
	const uint32_t nface = J.nface, recipe = J.recipe;
	r->recipe = recipe;
	r->index_out_of_range = range_flag(J, which);
	EncInputRecord rec;
	memset(&rec, 0, sizeof(rec));
	if(which == 0) {
		// the host's loops trust the index (encode_check has scanned it before setup runs) and read position[0] of an empty mesh: neither here
		const bool box = recipe == EIN_STEP_BOX_FIRST || recipe == EIN_STEP_BOX_MAX;
		if((box && m->nvert) || (recipe == EIN_STEP_EDGE && !r->index_out_of_range)) input_stats_host(m, recipe, rec, rd);
	} else {
		if((recipe == EIN_STEP_BOX_FIRST || recipe == EIN_STEP_BOX_MAX) && m->nvert) box_in_kernel_partition(J, rec.box);
		if(recipe == EIN_STEP_EDGE) {
			uint32_t bad = 0;
			double sum = 0;
			std::vector<float> terms(EIN_EDGE_TILE);
			for(uint32_t first = 0; first < nface; first += EIN_EDGE_TILE) {
				const uint32_t cnt = nface - first < EIN_EDGE_TILE ? nface - first : EIN_EDGE_TILE;
				for(uint32_t i = cnt; i-- > 0;) terms[i] = enc_in_edge_term(J, first + i, bad);   // (any order: they are independent)
				for(uint32_t i = 0; i < cnt; i++) sum += (double)terms[i];
				if(first + EIN_EDGE_TILE < first) break;
			}
			r->index_out_of_range |= bad;
			rec.sum = sum;
		}
	}
	// a mesh with an entry out of range is refused: its sum (a term per face that could be gathered) and step mean nothing and are reported as 0
	if(r->index_out_of_range) rec.sum = 0;
	for(int k = 0; k < 3; k++) { r->mn[k] = rec.box.mn[k]; r->mx[k] = rec.box.mx[k]; }
	r->sum = rec.sum;
	r->step = r->index_out_of_range ? 0.0f : position_step(m, recipe, rec);
}

} // namespace

extern "C" int crthip_encode_input_model(const crthip_mesh *m, int which, crthip_encode_input_result *r) {
	return crthip_encode_input_model_layout(m, nullptr, which, r);
}

extern "C" int crthip_encode_input_model_layout(const crthip_mesh *m, const crthip_mesh_layout *layout, int which, crthip_encode_input_result *r) {
	if(which != 0 && which != 1) return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_encode_input_model: which must be 0 (host loops) or 1 (device source)");
	if(!r) return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_encode_input_model: null result");
	{ const int e = encode_check(m, false); if(e) return e; }
	MeshRead rd;
	{ const int e = layout_resolve(m, nullptr, layout, rd); if(e) return e; }
	try {
		model(m, layout ? &rd : nullptr, which, r);
		return CRTHIP_OK;
	} catch(const std::bad_alloc &) {
		return ctx_fail(CRTHIP_E_NOMEM, nullptr);
	} catch(...) {
		return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_encode_input_model: internal error");
	}
}
