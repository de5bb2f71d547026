// bvh_query_check.cpp — csrc/bvh_query.h on the host under AddressSanitizer and UBSan (tests/test_bvh_query_sanitize_cpu.py): a stand-alone
// program, host code only.  Every array of a set is a heap block of its own that ENDS exactly where the contract says the array ends: the
// nodes at the last of 2F - 1 records, the position at the last vertex's sixth byte (at stride 8: two bytes short of a whole record), the
// index at its last entry, the transform at its 48th byte, the boxes at their last record, the results at their last record and the lists
// at the last word of the last box's slice - a load or a store one byte past any of them is reported.  (The hook's own stack block is made
// at exactly the kernel's LDS size: a push past entry 64 is reported too.)  The trees are crthip_bvh_model's, both partitions, and corrupt
// ones: a cycle, a child id out of range, a leaf with a face id out of range, a chain deeper than 65, random bytes - each must end, and the
// hand-made ones with CRTHIP_QUERY_TREE.  The results are compared with a brute force over all faces on __int128, which takes all three
// projections an axis as the contract words it; the lists with that brute force in the order array's ranks.
// Built with csrc/bvh_query_host.cpp and csrc/bvh_host.cpp, whose one dependency on the library (ctx_fail) is defined here.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/corto_hip.h"
#include "bvh.h"
#include "bvh_query.h"

using namespace corto_hip;

namespace corto_hip {
int ctx_fail(int code, const char *) { return code; }
}

static int failures = 0;
#define CHECK(cond, ...) do { if(!(cond)) { failures++; printf("FAILED %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } while(0)

static uint64_t rng_state;
static uint64_t rng() { rng_state = rng_state*6364136223846793005ull + 1442695040888963407ull; return rng_state >> 16; }

// a block that ENDS at its last byte (aligned_alloc rounds a block to 16 bytes): the bytes, and the block to free.  (sz a multiple of 2 keeps
// the bytes 2-byte aligned, of 4 4-byte aligned, of 16 16-byte aligned.)
static uint8_t *ending_block(size_t sz, uint8_t **blk) {
	const size_t cap = sz ? (sz + 15)/16*16 : 16;
	*blk = (uint8_t *)aligned_alloc(16, cap);
	memset(*blk, 0xCD, cap);
	return *blk + (cap - sz);
}

typedef __int128 wide;
struct V3 { wide c[3]; };
static V3 sub(V3 a, V3 b) { return V3{{a.c[0] - b.c[0], a.c[1] - b.c[1], a.c[2] - b.c[2]}}; }
static wide dot(V3 a, V3 b) { return a.c[0]*b.c[0] + a.c[1]*b.c[1] + a.c[2]*b.c[2]; }
static V3 cross(V3 a, V3 b) { return V3{{a.c[1]*b.c[2] - a.c[2]*b.c[1], a.c[2]*b.c[0] - a.c[0]*b.c[2], a.c[0]*b.c[1] - a.c[1]*b.c[0]}}; }
static wide wabs(wide x) { return x < 0 ? -x : x; }

// the contract's rule for one present face, absolute coordinates
static bool brute_face(const int32_t *pos, const uint32_t *t, const crthip_box &b, uint32_t flags) {
	V3 V[3], h;
	for(int c = 0; c < 3; c++) h.c[c] = (wide)b.max[c] - b.min[c];
	for(int k = 0; k < 3; k++) for(int c = 0; c < 3; c++) V[k].c[c] = 2*(wide)pos[(size_t)t[k]*3 + c] - ((wide)b.min[c] + b.max[c]);
	bool overlap = true, inside = true;
	for(int c = 0; c < 3; c++) {
		wide mn = V[0].c[c], mx = V[0].c[c];
		for(int k = 1; k < 3; k++) { if(V[k].c[c] < mn) mn = V[k].c[c]; if(V[k].c[c] > mx) mx = V[k].c[c]; }
		if(mn > h.c[c] || mx < -h.c[c]) overlap = false;
		if(mn < -h.c[c] || mx > h.c[c]) inside = false;
	}
	if(flags & CRTHIP_QUERY_BOXES) return overlap;
	if(flags & CRTHIP_QUERY_INSIDE) return inside;
	if(!overlap) return false;
	const V3 e[3] = {sub(V[1], V[0]), sub(V[2], V[1]), sub(V[0], V[2])};
	const V3 n = cross(e[0], e[1]);
	if(wabs(dot(n, V[0])) > h.c[0]*wabs(n.c[0]) + h.c[1]*wabs(n.c[1]) + h.c[2]*wabs(n.c[2])) return false;
	for(int k = 0; k < 3; k++) for(int i = 0; i < 3; i++) {
		V3 u{{0, 0, 0}};
		u.c[k] = 1;
		const V3 a = cross(u, e[i]);
		const wide r = h.c[0]*wabs(a.c[0]) + h.c[1]*wabs(a.c[1]) + h.c[2]*wabs(a.c[2]);
		wide mn = dot(a, V[0]), mx = mn;
		for(int v = 1; v < 3; v++) { const wide p = dot(a, V[v]); if(p < mn) mn = p; if(p > mx) mx = p; }
		if(mn > r || mx < -r) return false;
	}
	return true;
}

// the contract by brute force: every face in rank order, no tree
static crthip_query_result brute(const int32_t *pos, uint32_t nvert, const uint32_t *idx, const std::vector<uint32_t> &order, const int32_t base[3], const crthip_box &b,
                                 uint32_t flags, uint32_t cap, std::vector<uint32_t> &list) {
	list.clear();
	for(int c = 0; c < 3; c++) {
		const int64_t p = (int64_t)b.min[c] - base[c], q = (int64_t)b.max[c] - base[c];
		if(p < -(1 << 19) || p >= (1 << 19) || q < -(1 << 19) || q >= (1 << 19)) return crthip_query_result{CRTHIP_QUERY_RANGE, 0, 0, 0};
	}
	if(b.min[0] > b.max[0] || b.min[1] > b.max[1] || b.min[2] > b.max[2]) return crthip_query_result{CRTHIP_QUERY_OK, 0, 0, 0};
	for(uint32_t f : order) {
		const uint32_t *t = idx + (size_t)f*3;
		if(t[0] >= nvert || t[1] >= nvert || t[2] >= nvert) continue;
		if(brute_face(pos, t, b, flags)) list.push_back(f);
	}
	const uint32_t count = (uint32_t)list.size(), written = (flags & CRTHIP_QUERY_COUNT) ? 0u : count < cap ? count : cap;
	return crthip_query_result{written < count && !(flags & CRTHIP_QUERY_COUNT) ? (uint32_t)CRTHIP_QUERY_CLIPPED : (uint32_t)CRTHIP_QUERY_OK, count, written, 0};
}

struct Blocks {
	uint8_t *nblk, *pblk, *iblk, *tblk, *bblk, *rblk, *fblk;
	crthip_bvh_query_set set;
	crthip_query_result *results;
	uint32_t *faces;
	void release() { free(nblk); free(pblk); free(iblk); free(tblk); free(bblk); free(rblk); free(fblk); }
};

// the set's arrays as blocks that end at their last byte; pos: absolute integers, base their minimum
static Blocks make(const std::vector<crthip_bvh_node> &nodes, const int32_t *pos, uint32_t nvert, const int32_t base[3], const uint32_t *idx, uint32_t F, int u16,
                   uint32_t stride, bool with_transform, const std::vector<crthip_box> &boxes, uint32_t flags, uint32_t cap) {
	Blocks b;
	memset(&b.set, 0, sizeof b.set);
	crthip_bvh_node *n = (crthip_bvh_node *)ending_block(nodes.size()*32, &b.nblk);
	memcpy(n, nodes.data(), nodes.size()*32);
	const uint32_t st = stride ? stride : 6;
	uint8_t *p = ending_block(nvert ? (size_t)(nvert - 1)*st + 6 : 0, &b.pblk);
	for(uint32_t v = 0; v < nvert; v++) for(int c = 0; c < 3; c++) { const uint16_t h = (uint16_t)(pos[(size_t)v*3 + c] - base[c]); memcpy(p + (size_t)v*st + 2*c, &h, 2); }
	uint8_t *ix = ending_block((size_t)F*3*(u16 ? 2 : 4), &b.iblk);
	for(size_t k = 0; k < (size_t)F*3; k++) { if(u16) ((uint16_t *)ix)[k] = (uint16_t)idx[k]; else ((uint32_t *)ix)[k] = idx[k]; }
	crthip_quant_transform *t = (crthip_quant_transform *)ending_block(sizeof(crthip_quant_transform), &b.tblk);
	memset(t, 0, sizeof *t);
	for(int c = 0; c < 3; c++) t->base[c] = base[c];
	t->components = 3; t->written = 1; t->q = 1.f;
	crthip_box *s = (crthip_box *)ending_block(boxes.size()*32, &b.bblk);
	memcpy(s, boxes.data(), boxes.size()*32);
	b.results = (crthip_query_result *)ending_block(boxes.size()*16, &b.rblk);
	const bool lists = cap && !(flags & CRTHIP_QUERY_COUNT);
	b.faces = (uint32_t *)ending_block(lists ? boxes.size()*(size_t)cap*4 : 0, &b.fblk);
	if(!lists) b.faces = nullptr;                                            // (legal: nothing is written under COUNT or at capacity 0)
	b.set.nodes = n; b.set.position = p; b.set.index = ix; b.set.transform = with_transform ? t : nullptr; b.set.boxes = s; b.set.results = b.results; b.set.faces = b.faces;
	for(int c = 0; c < 3; c++) b.set.base[c] = with_transform ? 0x5A5A5A5 : base[c];   // (with a record, base[] is not read)
	b.set.pos_stride = stride; b.set.nvert = nvert; b.set.nface = F; b.set.index_format = u16 ? CRTHIP_FMT_UINT16 : CRTHIP_FMT_UINT32;
	b.set.nbox = (uint32_t)boxes.size(); b.set.face_capacity = cap; b.set.flags = flags;
	return b;
}

static std::vector<crthip_box> some_boxes(const int32_t *pos, uint32_t nvert, const int32_t base[3], const int32_t lo[3], const int32_t hi[3], uint32_t n) {
	std::vector<crthip_box> boxes;
	for(uint32_t k = 0; k < n; k++) {
		crthip_box b;
		memset(&b, 0xEE, sizeof b);
		const uint32_t v = (uint32_t)(rng() % nvert);
		for(int c = 0; c < 3; c++) {
			const int32_t reach = k % 4 == 0 ? 0 : (int32_t)(rng() % 40);   // every fourth: the point box at a vertex
			b.min[c] = pos[(size_t)v*3 + c] - (k % 4 == 1 ? 0 : reach);     // the next: a corner at a vertex
			b.max[c] = pos[(size_t)v*3 + c] + reach;
		}
		if(k % 19 == 2) for(int c = 0; c < 3; c++) { b.min[c] = lo[c]; b.max[c] = hi[c]; }   // the whole mesh
		if(k % 17 == 5) b.max[k % 3] = base[k % 3] + (1 << 19);             // just out of range
		if(k % 17 == 6) b.min[k % 3] = base[k % 3] - (1 << 19);             // the range's first value
		if(k % 23 == 7) b.min[k % 3] = b.max[k % 3] + 1;                    // empty
		boxes.push_back(b);
	}
	return boxes;
}

// kind 0: a small patch of noise; 1: random strip; 2: with absent faces
static void one(uint32_t F, int kind, int u16, uint32_t stride) {
	rng_state = 0x9E3779B97F4A7C15ull ^ ((uint64_t)F*131u + kind*7u + u16);
	const uint32_t nvert = F + 2;
	std::vector<int32_t> pos((size_t)nvert*3);
	const uint32_t spread = kind == 0 ? 60 : 3000;
	for(size_t k = 0; k < pos.size(); k++) pos[k] = (int32_t)(rng() % spread) - (int32_t)(spread/2) + 70000;
	int32_t base[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, top[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
	for(uint32_t v = 0; v < nvert; v++) for(int c = 0; c < 3; c++) {
		if(pos[(size_t)v*3 + c] < base[c]) base[c] = pos[(size_t)v*3 + c];
		if(pos[(size_t)v*3 + c] > top[c]) top[c] = pos[(size_t)v*3 + c];
	}
	std::vector<uint32_t> idx((size_t)F*3);
	for(uint32_t f = 0; f < F; f++) {
		uint32_t id[3] = {f, f + 1, f + 2};
		if(kind == 2 && f % 5 == 1) id[f % 3] = u16 ? 0xFFFFu : nvert + (uint32_t)(rng() % 1000);
		if(kind == 1 && f % 7 == 3) id[1] = id[0];                          // a segment
		for(int c = 0; c < 3; c++) idx[(size_t)f*3 + c] = id[c];
	}
	const std::vector<crthip_box> boxes = some_boxes(pos.data(), nvert, base, base, top, 150);
	for(int which = 0; which < 2; which++) {
		if(which == 0 && !bvh_in_blob(F)) continue;
		std::vector<crthip_bvh_node> nodes(2*(size_t)F - 1);
		std::vector<uint32_t> order(F);
		crthip_bvh_node *nb = (crthip_bvh_node *)aligned_alloc(16, nodes.size()*32);
		CHECK(crthip_bvh_model(pos.data(), nvert, idx.data(), 0, F, nb, nullptr, order.data(), nullptr, which, 3) == CRTHIP_OK, "the tree of F %u", F);
		memcpy(nodes.data(), nb, nodes.size()*32);
		free(nb);
		const uint32_t flagset[6] = {0, 1, 2, 4, 3, 5};
		for(uint32_t fi = 0; fi < 6; fi++) {
			const uint32_t flags = flagset[fi], cap = fi == 2 ? 0u : fi == 3 ? 1u : 3u;
			Blocks b = make(nodes, pos.data(), nvert, base, idx.data(), F, u16, stride, fi & 1, boxes, flags, cap);
			const int err = crthip_bvh_query_model(&b.set, b.results, b.faces);
			CHECK(err == CRTHIP_OK, "F %u kind %d: %d", F, kind, err);
			uint32_t nmatch = 0;
			std::vector<uint32_t> list;
			for(size_t i = 0; i < boxes.size() && !err; i++) {
				const crthip_query_result w = brute(pos.data(), nvert, idx.data(), order, base, boxes[i], flags, cap, list);
				nmatch += w.count > 0;
				CHECK(memcmp(&w, &b.results[i], 16) == 0, "F %u kind %d u16 %d stride %u which %d flags %u box %zu: {%u %u %u %u}, expected {%u %u %u}", F, kind, u16,
				      stride, which, flags, i, b.results[i].status, b.results[i].count, b.results[i].written, b.results[i].reserved, w.status, w.count, w.written);
				for(uint32_t k = 0; k < cap && b.faces; k++) {
					const uint32_t got = b.faces[i*cap + k], want = k < w.written ? list[k] : 0xCDCDCDCDu;
					CHECK(got == want, "F %u kind %d which %d flags %u box %zu word %u: %u, expected %u", F, kind, which, flags, i, k, got, want);
				}
			}
			CHECK(nmatch > 0, "F %u kind %d flags %u: nothing matched", F, kind, flags);
			b.release();
		}
	}
}

static crthip_bvh_node node(int32_t lo, uint32_t left, int32_t hi, uint32_t right) { return crthip_bvh_node{{lo, lo, lo}, left, {hi, hi, hi}, right}; }

// corrupt trees over F copies of one face: kind 0 a cycle, 1 a node its own child, 2 a child id out of range, 3 a leaf's face out of range,
// 4 a chain of 70 down the left side, 5 random bytes
static void corrupt(int kind, uint32_t F) {
	rng_state = 77 + kind;
	const uint32_t nn = 2*F - 1;
	std::vector<crthip_bvh_node> nodes(nn, node(-100000, 0, 100000, CRTHIP_BVH_LEAF));
	if(kind == 0) { nodes[0] = node(-100000, 1, 100000, 2); nodes[1] = node(-100000, 0, 100000, 2); }
	if(kind == 1) nodes[0] = node(-100000, 0, 100000, 0);
	if(kind == 2) nodes[0] = node(-100000, 1, 100000, nn);
	if(kind == 3) { nodes[0] = node(-100000, 1, 100000, 2); nodes[1] = node(-100000, F, 100000, CRTHIP_BVH_LEAF); }
	if(kind == 4) for(uint32_t k = 0; k < 70; k++) nodes[k] = node(-100000, k + 1, 100000, 100 + k);
	if(kind == 5) {
		for(crthip_bvh_node &n : nodes) for(size_t w = 0; w < 8; w++) ((uint32_t *)&n)[w] = (uint32_t)rng();
		nodes[0].min[0] = nodes[0].min[1] = nodes[0].min[2] = INT32_MIN; nodes[0].max[0] = nodes[0].max[1] = nodes[0].max[2] = INT32_MAX;
	}
	const int32_t pos[9] = {0, 0, 500, 9, 0, 500, 0, 9, 500}, base[3] = {0, 0, 500};
	std::vector<uint32_t> idx((size_t)F*3);
	for(uint32_t f = 0; f < F; f++) { idx[(size_t)f*3] = 0; idx[(size_t)f*3 + 1] = 1; idx[(size_t)f*3 + 2] = 2; }
	std::vector<crthip_box> boxes(66);
	for(size_t k = 0; k < boxes.size(); k++) {                                // around the face, and from the 40th on beside it
		memset(&boxes[k], 0, 32);
		for(int c = 0; c < 3; c++) { boxes[k].min[c] = (k < 40 ? -5 : 100) - (int32_t)k + (c == 2 ? 500 : 0); boxes[k].max[c] = (k < 40 ? 5 : 120) + (int32_t)k + (c == 2 ? 500 : 0); }
	}
	const uint32_t flagset[4] = {0, 1, 2, 4};
	for(uint32_t flags : flagset) {
		const uint32_t cap = 2;
		Blocks b = make(nodes, pos, 3, base, idx.data(), F, 0, 8, false, boxes, flags, cap);
		const int err = crthip_bvh_query_model(&b.set, b.results, b.faces);
		CHECK(err == CRTHIP_OK, "corrupt %d: %d", kind, err);
		for(size_t i = 0; i < boxes.size() && !err; i++) {
			const crthip_query_result &r = b.results[i];
			if(kind < 5) CHECK(r.status == CRTHIP_QUERY_TREE && !r.count && !r.written && !r.reserved, "corrupt %d F %u box %zu: status %u", kind, F, i, r.status);
			else CHECK(r.status <= CRTHIP_QUERY_TREE && !r.reserved && r.written <= cap && (r.status < CRTHIP_QUERY_RANGE || (!r.count && !r.written)), "corrupt %d F %u box %zu: status %u", kind, F, i, r.status);
			for(uint32_t k = 0; k < cap && b.faces; k++) CHECK(b.faces[i*cap + k] < F || b.faces[i*cap + k] == 0xCDCDCDCDu, "corrupt %d F %u box %zu: word %u", kind, F, i, b.faces[i*cap + k]);
		}
		b.release();
	}
}

int main() {
	const uint32_t sizes[] = {1, 2, 3, 17, 257, BVH_BLOB_FACES, BVH_BLOB_FACES + 1};
	for(uint32_t F : sizes)
		for(int kind = 0; kind < 3; kind++) {
			if(F >= BVH_BLOB_FACES && kind != 0) continue;
			one(F, kind, (F + kind) & 1, (F + kind) % 3 == 0 ? 8 : (F + kind) % 3 == 1 ? 0 : 6);
		}
	corrupt(0, 2); corrupt(0, 300); corrupt(1, 2); corrupt(1, 40); corrupt(2, 2); corrupt(3, 2); corrupt(4, 100); corrupt(5, 1); corrupt(5, 2); corrupt(5, 77);
	// the set's own checks reach the hook too
	{
		crthip_bvh_query_set s;
		memset(&s, 0, sizeof s);
		CHECK(crthip_bvh_query_model(nullptr, nullptr, nullptr) == CRTHIP_E_ARGUMENT, "a null set");
		CHECK(crthip_bvh_query_model(&s, nullptr, nullptr) == CRTHIP_E_ARGUMENT, "no faces");
		s.nface = 1;
		CHECK(crthip_bvh_query_model(&s, nullptr, nullptr) == CRTHIP_OK, "no boxes");
		s.flags = 8;
		CHECK(crthip_bvh_query_model(&s, nullptr, nullptr) == CRTHIP_E_ARGUMENT, "unknown flags");
		s.flags = CRTHIP_QUERY_BOXES | CRTHIP_QUERY_INSIDE;
		CHECK(crthip_bvh_query_model(&s, nullptr, nullptr) == CRTHIP_E_ARGUMENT, "both rules");
	}
	if(failures) { printf("bvh_query_check: %d failures\n", failures); return 1; }
	printf("bvh_query_check ok\n");
	return 0;
}
