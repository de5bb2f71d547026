// enc_topology.h — the encoder's CLERS topology pass (encoder.cpp: Encoder::topology, pair_half_edges, Encoder::encode_faces) restated as
// __host__ __device__ code over flat arrays, so that k_encode_topo.hip runs it on the device for crthip_encode_batch and the host can run
// the very same source (crthip_encode_topology_model, which = 1; tests/test_encode_topology_cpu.py holds it against the host pass).
// Same results byte for byte, non-manifold input included: which two of several sides on an edge get paired depends on the order
// std::sort leaves a bucket in, so every bucket goes through StdSortModel (std_sort_model.h) from the same starting order.
//
// Three stages, each written for a TEAM of cooperating lanes (one workgroup on the device, one thread on the host):
//   enc_topo_compact     faces with two equal corners dropped group by group, order kept; new group ends, nface, the used vertices counted
//   enc_topo_pair_group  twin[] of one group: sides bucketed by their smaller vertex, one lane per bucket restores fill order (ascending
//                        half-edge id), sorts by the larger vertex unless the host would have skipped the bucket, and scans for pairs
//   enc_topo_walk        the region-growing walk, groups in sequence; one dependent chain on lane 0, the other lanes clear and fill arrays.
//                        Its state is addressed through EncTopoState<L>: L = uint16_t for an image that fits LDS, uint32_t for one in
//                        global memory - the same code either way, chosen per mesh from its sizes alone (enc_topo_fits_lds).
// A Team gives: tid, n, sync(), scan(v, total) (exclusive scan of one value per lane), add(p, v) (atomic fetch-add),
// order(i, n) (the item a lane takes in turn i of a scatter loop: the host team walks backwards, so the order-restoring step is exercised).
// Every loop is bounded by the sizes; a walk that would exceed its bound, or an output that would leave its buffer, stops with
// CRTHIP_E_DEVICE in the mesh's record.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/corto_hip.h"
#include "std_sort_model.h"

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define ETOPO_HD __host__ __device__ inline
#else
#define ETOPO_HD inline
#endif

namespace corto_hip {

constexpr uint32_t ETOPO_NONE = 0xffffffffu;          // no twin / no pending gate
constexpr uint32_t ETOPO_LDS_MAX = 156*1024;          // of the CU's 160 KiB
constexpr uint32_t ETOPO_LDS_FIXED = 64;              // the team's scan words, rounded up
constexpr uint32_t ETOPO_THREADS = 256;

// output bounds from the sizes alone.  CLERS: one symbol per face written, at most one BOUNDARY and one DELAY per half-edge that joins
// the front (3 per face).  Split bits: a seed writes at most 3 + 3*32, a SPLIT 32: under 128 bits a face.
ETOPO_HD uint64_t enc_topo_clers_cap(uint32_t nface) { return 7ull*nface + 64; }
ETOPO_HD uint64_t enc_topo_split_cap(uint32_t nface) { return 4ull*nface + 4; }          // u32 words

struct EncTopoSide { uint32_t hi, half, flipped; };    // a side in its bucket: the larger vertex, 3*face + side, runs hi -> lo

struct EncTopoRecord {                                 // what comes back per mesh
	int32_t status;
	uint32_t nvert, nface, max_front, nclers, split_bits, split_words, split_off, nused;
	uint32_t pad[7];
};
static_assert(sizeof(EncTopoRecord) == 64, "one record is 64 bytes");

struct EncTopoJob {
	const void *index;           // nface*3 as given: uint32, or uint16 (index16) - stage 1 widens as it reads, everything behind it sees faces
	const uint32_t *gend_in;     // ngroups >= 1 ascending ends, each <= nface
	uint32_t *faces;             // out: compacted faces
	uint32_t *gend_out;          // out: ngroups new ends
	uint32_t *first, *cursor;    // nvert + 1 and nvert words: vertex marks, then a group's bucket starts and write cursors
	EncTopoSide *sides;          // 3*nface
	uint32_t *twin;              // 3*nface: per group, half-edge ids counted from the group's first face
	uint8_t *state;              // the walk's global image (enc_topo_state_bytes<uint32_t>), unused by a mesh that walks in LDS
	uint32_t *quads;             // out: nvert x (t, a, b, c)
	uint8_t *clers;              // out: enc_topo_clers_cap(nface) bytes
	uint32_t *split;             // out: enc_topo_split_cap(nface) words
	uint32_t *split_packed;      // the batch's split words back to back ...
	uint32_t *split_cursor;      // ... and how many are there (atomic); null: leave them in split
	EncTopoRecord *rec;          // zeroed before the first stage
	uint32_t nvert, nface, ngroups, index16;
};
ETOPO_HD uint32_t enc_topo_index(const EncTopoJob &J, size_t i) { return J.index16 ? (uint32_t)((const uint16_t *)J.index)[i] : ((const uint32_t *)J.index)[i]; }

template <class L> struct EncTopoState {
	L *before, *after, *twin, *gates, *postponed, *encoded;
	uint8_t *where, *coded;
};
template <class L> ETOPO_HD uint64_t enc_topo_state_bytes(uint32_t nface, uint32_t nvert) {
	return sizeof(L)*(15ull*nface + nvert) + 4ull*nface;
}
template <class L> ETOPO_HD EncTopoState<L> enc_topo_carve(uint8_t *base, uint32_t nface, uint32_t nvert) {
	const size_t nh = 3*(size_t)nface;
	EncTopoState<L> s;
	L *p = (L *)base;
	s.before = p; s.after = p + nh; s.twin = p + 2*nh; s.gates = p + 3*nh; s.postponed = p + 4*nh; s.encoded = p + 5*nh;
	s.where = (uint8_t *)(s.encoded + nvert); s.coded = s.where + nh;
	return s;
}
// the rule that picks the walk's state: 16-bit links in LDS while every half-edge id and vertex number stays below 0xFFFF and the image
// fits; sizes as given (before the degenerate faces are dropped), never timing
ETOPO_HD bool enc_topo_fits_lds(uint32_t nvert, uint32_t nface) {
	if(nface == 0 || 3ull*nface > 65535ull || nvert > 65534u) return false;
	return enc_topo_state_bytes<uint16_t>(nface, nvert) + ETOPO_LDS_FIXED <= ETOPO_LDS_MAX;
}

ETOPO_HD int enc_topo_ilog2(uint32_t p) { int k = 0; while(p >>= 1) ++k; return k; }

// ---- stage 1 ----
template <class Team> ETOPO_HD void enc_topo_compact(Team &T, const EncTopoJob &J) {
	for(uint32_t v = T.tid; v <= J.nvert; v += T.n) J.first[v] = 0;
	T.sync();
	uint32_t start = 0, count = 0;
	for(uint32_t g = 0; g < J.ngroups; g++) {
		uint32_t end = J.gend_in[g];
		if(end > J.nface) end = J.nface;
		if(end < start) end = start;
		for(uint32_t base = start; base < end; base += T.n) {          // the same trip count for every lane: scan() is a team operation
			const uint32_t i = base + T.tid;
			uint32_t f0 = 0, f1 = 0, f2 = 0, keep = 0;
			if(i < end && i >= base) {
				f0 = enc_topo_index(J, (size_t)i*3); f1 = enc_topo_index(J, (size_t)i*3 + 1); f2 = enc_topo_index(J, (size_t)i*3 + 2);
				keep = !(f0 == f1 || f0 == f2 || f1 == f2);
			}
			uint32_t total = 0;
			const uint32_t at = count + T.scan(keep, total);
			if(keep) {
				J.faces[(size_t)at*3] = f0; J.faces[(size_t)at*3 + 1] = f1; J.faces[(size_t)at*3 + 2] = f2;
				if(f0 < J.nvert) J.first[f0] = 1;
				if(f1 < J.nvert) J.first[f1] = 1;
				if(f2 < J.nvert) J.first[f2] = 1;
			}
			count += total;
			if(base + T.n < base) break;
		}
		start = end;
		if(T.tid == 0) J.gend_out[g] = count;
	}
	T.sync();
	uint32_t used = 0;
	for(uint32_t v = T.tid; v < J.nvert; v += T.n) used += J.first[v];
	if(used) T.add(&J.rec->nused, used);
	if(T.tid == 0) J.rec->nface = count;
}

// ---- stage 2 ----
struct EncTopoLessHalf { ETOPO_HD bool operator()(const EncTopoSide &a, const EncTopoSide &b) const { return a.half < b.half; } };
struct EncTopoLessHi { ETOPO_HD bool operator()(const EncTopoSide &a, const EncTopoSide &b) const { return a.hi < b.hi; } };

// side s of face t runs from corner (s+1)%3 to corner (s+2)%3
ETOPO_HD void enc_topo_ends(const uint32_t *corner, uint32_t h, uint32_t &from, uint32_t &to) {
	const uint32_t t = h/3, s = h%3;
	from = corner[(size_t)3*t + (s + 1)%3]; to = corner[(size_t)3*t + (s + 2)%3];
}

template <class Team> ETOPO_HD void enc_topo_pair_group(Team &T, const uint32_t *corner, uint32_t ntri, uint32_t nvert, uint32_t *first, uint32_t *cursor,
                                                        EncTopoSide *sides, uint32_t *twin) {
	const uint32_t nh = 3*ntri;
	for(uint32_t v = T.tid; v <= nvert; v += T.n) first[v] = 0;
	for(uint32_t h = T.tid; h < nh; h += T.n) twin[h] = ETOPO_NONE;
	T.sync();
	for(uint32_t h = T.tid; h < nh; h += T.n) {
		uint32_t a, b; enc_topo_ends(corner, h, a, b);
		const uint32_t lo = a < b ? a : b;
		if(lo < nvert) T.add(&first[lo], 1u);
	}
	T.sync();
	// bucket starts: first[v] = sides whose smaller vertex is below v, first[nvert] = all of them
	uint32_t carry = 0;
	for(uint32_t base = 0; base <= nvert; base += T.n) {
		const uint32_t v = base + T.tid;
		const bool in = v <= nvert && v >= base;
		const uint32_t c = in ? first[v] : 0u;
		uint32_t total = 0;
		const uint32_t e = carry + T.scan(c, total);
		if(in) { first[v] = e; if(v < nvert) cursor[v] = e; }
		carry += total;
		if(base + T.n < base) break;
	}
	T.sync();
	for(uint32_t i = T.tid; i < nh; i += T.n) {
		const uint32_t h = T.order(i, nh);
		uint32_t a, b; enc_topo_ends(corner, h, a, b);
		const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
		if(lo >= nvert) continue;
		const uint32_t at = T.add(&cursor[lo], 1u);
		if(at < nh) { EncTopoSide s; s.hi = hi; s.half = h; s.flipped = a > b; sides[at] = s; }
	}
	T.sync();
	// buckets are independent: a candidate never pairs across a change of the smaller vertex
	for(uint32_t v = T.tid; v < nvert; v += T.n) {
		const uint32_t b0 = first[v], b1 = first[v + 1];
		if(b1 <= b0 || b1 > nh) continue;
		EncTopoSide *s = sides + b0;
		const int len = (int)(b1 - b0);
		std_sort_model(s, len, EncTopoLessHalf());                 // fill order: face by face, side 0, 1, 2
		// (the host skips every bucket that starts at offset 0 except vertex 0's: the first non-empty bucket stays in fill order
		// when vertex 0 is not the smaller end of any side - encoder.cpp: pair_half_edges)
		if(!(v > 0 && b0 == 0)) std_sort_model(s, len, EncTopoLessHi());
		int cand = -1;
		for(int k = 0; k < len; k++) {
			if(cand >= 0 && s[cand].hi == s[k].hi && s[cand].flipped != s[k].flipped) {
				if(twin[s[k].half] == ETOPO_NONE && twin[s[cand].half] == ETOPO_NONE) { twin[s[k].half] = s[cand].half; twin[s[cand].half] = s[k].half; }
			} else cand = k;
		}
	}
	T.sync();
}

template <class Team> ETOPO_HD void enc_topo_pair(Team &T, const EncTopoJob &J) {
	uint32_t start = 0;
	for(uint32_t g = 0; g < J.ngroups; g++) {
		uint32_t end = J.gend_out[g];
		if(end > J.nface) end = J.nface;
		if(end < start) end = start;
		enc_topo_pair_group(T, J.faces + (size_t)start*3, end - start, J.nvert, J.first, J.cursor, J.sides, J.twin + (size_t)start*3);
		start = end;
	}
}

// ---- stage 3 ----
enum { ETOPO_VERTEX = 0, ETOPO_LEFT = 1, ETOPO_RIGHT = 2, ETOPO_END = 3, ETOPO_BOUNDARY = 4, ETOPO_DELAY = 5, ETOPO_SPLIT = 6 };
enum { ETOPO_OFF_FRONT = 0, ETOPO_ON_FRONT = 1, ETOPO_CLOSED = 2 };

// what the walk writes, carried from group to group (lane 0's)
struct EncTopoOut {
	uint8_t *clers; uint64_t clers_cap; uint32_t nclers;
	uint32_t *split; uint64_t split_cap; uint32_t nwords, buff; int bits;      // MSB-first bit writer (encoder.cpp: BitWriter)
	uint64_t nbits;
	uint32_t *quads; uint32_t nvert;
	uint32_t current_vertex, last_index, max_front;
	int idbits;
	int32_t status;

	ETOPO_HD void symbol(uint32_t s) { if(nclers < clers_cap) clers[nclers] = (uint8_t)s; else status = CRTHIP_E_DEVICE; nclers++; }
	ETOPO_HD void word(uint32_t w) { if(nwords < split_cap) split[nwords] = w; else status = CRTHIP_E_DEVICE; nwords++; }
	ETOPO_HD void write(uint32_t value, int n) {
		nbits += (uint64_t)n;
		if(n >= bits) {
			buff = (bits == 32 ? 0u : (buff << bits)) | (value >> (n - bits));
			word(buff);
			const int rest = n - bits;
			value &= rest >= 32 ? 0xFFFFFFFFu : ((1u << rest) - 1u);
			n = rest; bits = 32; buff = 0;
		}
		if(n > 0) { buff = (buff << n) | value; bits -= n; }
	}
	ETOPO_HD void flush() { if(bits != 32) { word(buff << bits); buff = 0; bits = 32; } }
};

// the chain of one group (one lane): Encoder::encode_faces statement for statement
template <class L> ETOPO_HD void enc_topo_chain(const EncTopoState<L> &S, EncTopoOut &O, const uint32_t *corner, uint32_t ntri) {
	const L NONE_L = (L)~(L)0;
	const uint32_t nh = 3*ntri;
	uint32_t gate_cursor = 0, ngates = 0, npost = 0, seed_cursor = 0, remaining = ntri, joined = 0, pending = ETOPO_NONE;
	// every turn of the loop is a seed (at most one per face) or a visit to a half-edge that joined the front (each at most twice: once
	// from the FIFO or as the pending edge, once more from the postponed stack)
	uint64_t turns = 0;
	const uint64_t max_turns = 10ull*ntri + 16;

	auto onto_front = [&](uint32_t h, uint32_t p, uint32_t n) { S.where[h] = ETOPO_ON_FRONT; S.before[h] = (L)p; S.after[h] = (L)n; joined++; };
	auto introduce = [&](uint32_t v, uint32_t a, uint32_t b, uint32_t c) {
		if(O.current_vertex < O.nvert) { uint32_t *q = O.quads + (size_t)O.current_vertex*4; q[0] = v; q[1] = a; q[2] = b; q[3] = c; }
		else O.status = CRTHIP_E_DEVICE;
		S.encoded[v] = (L)O.current_vertex++;
		O.last_index = v;
	};
	auto mention = [&](uint32_t v) { O.write((uint32_t)S.encoded[v], O.idbits); };
	auto push_gate = [&](uint32_t h) { if(ngates < nh) S.gates[ngates++] = (L)h; else O.status = CRTHIP_E_DEVICE; };

	while(remaining) {
		if(O.status) break;
		if(++turns > max_turns) { O.status = CRTHIP_E_DEVICE; break; }
		uint32_t gate;
		if(pending != ETOPO_NONE) { gate = pending; pending = ETOPO_NONE; }
		else if(gate_cursor < ngates) gate = S.gates[gate_cursor++];
		else if(npost) gate = S.postponed[--npost];
		else {
			while(seed_cursor < ntri && S.coded[seed_cursor]) seed_cursor++;
			if(seed_cursor == ntri) break;
			const uint32_t t = seed_cursor;
			const uint32_t *c3 = corner + 3*(size_t)t;
			uint32_t known = 0;
			for(int k = 0; k < 3; k++) if(S.encoded[c3[k]] != NONE_L) known |= 1u << k;
			if(known) { O.symbol(ETOPO_SPLIT); O.write(known, 3); } else O.symbol(ETOPO_VERTEX);
			for(int k = 0; k < 3; k++) {
				if(S.encoded[c3[k]] != NONE_L) mention(c3[k]);
				else introduce(c3[k], O.last_index, O.last_index, O.last_index);
			}
			const uint32_t h = 3*t;
			onto_front(h, h + 2, h + 1); onto_front(h + 1, h, h + 2); onto_front(h + 2, h + 1, h);
			push_gate(h); push_gate(h + 1); push_gate(h + 2);
			S.coded[t] = 1; remaining--;
			continue;
		}
		if(S.where[gate] == ETOPO_CLOSED) continue;
		const L tw_l = S.twin[gate];
		if(tw_l == NONE_L || S.coded[(uint32_t)tw_l/3]) { O.symbol(ETOPO_BOUNDARY); continue; }
		const uint32_t tw = tw_l;
		const uint32_t across = tw/3;
		const uint32_t s_far = tw%3, s_a = (s_far + 1)%3, s_b = (s_a + 1)%3;
		// the corners this step may need come from global memory: asked for here, in one go, so that their latency runs beside the
		// front's reads below instead of once for the far corner and once more for the quad
		const uint32_t *ca = corner + 3*(size_t)across;
		const uint32_t far = ca[s_far], c_a = ca[s_a], c_b = ca[s_b], c_gate = corner[gate];
		const uint32_t left = S.before[gate], right = S.after[gate];
		const L tl = S.twin[left], tr = S.twin[right];
		const bool zip_left = tl != NONE_L && (uint32_t)tl/3 == across;
		const bool zip_right = tr != NONE_L && (uint32_t)tr/3 == across;
		const uint32_t h_a = 3*across + s_a, h_b = 3*across + s_b;
		if(zip_left && zip_right) {
			O.symbol(ETOPO_END);
			const uint32_t ll = S.before[left], rr = S.after[right];
			S.where[left] = ETOPO_CLOSED; S.where[right] = ETOPO_CLOSED;
			S.after[ll] = (L)rr; S.before[rr] = (L)ll;
		} else if(zip_left) {
			O.symbol(ETOPO_LEFT);
			const uint32_t ll = S.before[left];
			S.where[left] = ETOPO_CLOSED;
			onto_front(h_b, ll, right);
			S.after[ll] = (L)h_b; S.before[right] = (L)h_b;
			pending = h_b;
		} else if(zip_right) {
			O.symbol(ETOPO_RIGHT);
			const uint32_t rr = S.after[right];
			S.where[right] = ETOPO_CLOSED;
			onto_front(h_a, left, rr);
			S.before[rr] = (L)h_a; S.after[left] = (L)h_a;
			pending = h_a;
		} else {
			if(S.encoded[far] != NONE_L && gate_cursor < ngates) {
				if(npost < nh) S.postponed[npost++] = (L)gate; else O.status = CRTHIP_E_DEVICE;
				O.symbol(ETOPO_DELAY);
				continue;
			}
			if(S.encoded[far] != NONE_L) { O.symbol(ETOPO_SPLIT); mention(far); }
			else {
				O.symbol(ETOPO_VERTEX);
				introduce(far, c_a, c_b, c_gate);
			}
			onto_front(h_a, left, h_b); onto_front(h_b, h_a, right);
			S.after[left] = (L)h_a; S.before[right] = (L)h_b;
			push_gate(h_b);
			pending = h_a;
		}
		S.coded[across] = 1; remaining--;
	}
	if(joined > O.max_front) O.max_front = joined;
}

// the whole mesh: groups in sequence over one state image (LDS or global), then the record
template <class L, class Team> ETOPO_HD void enc_topo_walk(Team &T, const EncTopoJob &J, uint8_t *image) {
	const L NONE_L = (L)~(L)0;
	const EncTopoState<L> S = enc_topo_carve<L>(image, J.nface, J.nvert);
	for(uint32_t v = T.tid; v < J.nvert; v += T.n) S.encoded[v] = NONE_L;
	uint32_t nface = J.rec->nface;
	if(nface > J.nface) nface = J.nface;
	EncTopoOut O;
	O.clers = J.clers; O.clers_cap = enc_topo_clers_cap(J.nface); O.nclers = 0;
	O.split = J.split; O.split_cap = enc_topo_split_cap(J.nface); O.nwords = 0; O.buff = 0; O.bits = 32; O.nbits = 0;
	O.quads = J.quads; O.nvert = J.nvert;
	O.current_vertex = 0; O.last_index = 0; O.max_front = 0;
	O.idbits = enc_topo_ilog2(J.rec->nused) + 1;
	O.status = CRTHIP_OK;
	uint32_t start = 0;
	for(uint32_t g = 0; g < J.ngroups; g++) {
		uint32_t end = J.gend_out[g];
		if(end > nface) end = nface;
		if(end < start) end = start;
		const uint32_t ntri = end - start, nh = 3*ntri;
		const uint32_t *gtwin = J.twin + (size_t)start*3;
		for(uint32_t h = T.tid; h < nh; h += T.n) {
			S.where[h] = ETOPO_OFF_FRONT; S.before[h] = 0; S.after[h] = 0;
			const uint32_t tw = gtwin[h];
			S.twin[h] = tw < nh ? (L)tw : NONE_L;
		}
		for(uint32_t t = T.tid; t < ntri; t += T.n) S.coded[t] = 0;
		T.sync();
		if(T.tid == 0) enc_topo_chain<L>(S, O, J.faces + (size_t)start*3, ntri);
		T.sync();
		start = end;
	}
	if(T.tid == 0) {
		O.flush();
		uint32_t off = 0;
		if(J.split_cursor && O.status == CRTHIP_OK && O.nwords) {
			off = T.add(J.split_cursor, O.nwords);
			for(uint32_t i = 0; i < O.nwords; i++) J.split_packed[(size_t)off + i] = J.split[i];
		}
		EncTopoRecord *r = J.rec;
		r->nvert = O.current_vertex; r->max_front = O.max_front; r->nclers = O.nclers;
		r->split_bits = (uint32_t)O.nbits; r->split_words = O.nwords; r->split_off = off;
		r->status = O.status;
	}
}

// ---- the team of one: the host runs the stages with this ----
struct EncTopoHostTeam {
	uint32_t tid = 0, n = 1;
	void sync() {}
	uint32_t scan(uint32_t v, uint32_t &total) { total = v; return 0; }
	uint32_t add(uint32_t *p, uint32_t v) { const uint32_t o = *p; *p = o + v; return o; }
	uint32_t order(uint32_t i, uint32_t count) { return count - 1 - i; }
};

} // namespace corto_hip
