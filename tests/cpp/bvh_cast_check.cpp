// bvh_cast_check.cpp — csrc/bvh_cast.h on the host under AddressSanitizer and UBSan (tests/test_bvh_cast_sanitize_cpu.py): a stand-alone
// program, host code only.  Every array of a set is a heap block of its own that ENDS exactly where the contract says the array ends: the
// nodes at the last of 2F - 1 records, the position at the last vertex's sixth byte (at stride 8: two bytes short of a whole record), the
// index at its last entry, the transform at its 48th byte, the segments and the hits at their last record - a load or a store one byte
// past any of them is reported.  (The hook's own stack block is made at exactly the kernel's LDS size: a push past entry 64 is reported
// too.)  The trees are crthip_bvh_model's, both partitions, and corrupt ones: a cycle, a child id out of range, a leaf with a face id out
// of range, a chain deeper than 65, random bytes - each must end, and the hand-made ones with CRTHIP_CAST_TREE.  The results are compared
// with a brute force over all faces on __int128.
// Built with csrc/bvh_cast_host.cpp and csrc/bvh_host.cpp, whose one dependency on the library (ctx_fail) is defined here.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/corto_hip.h"
#include "bvh.h"
#include "bvh_cast.h"

using namespace corto_hip;

namespace corto_hip {
int ctx_fail(int code, const char *) { return code; }
}

static int failures = 0;
#define CHECK(cond, ...) do { if(!(cond)) { failures++; printf("FAILED %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } while(0)

static uint64_t rng_state;
static uint64_t rng() { rng_state = rng_state*6364136223846793005ull + 1442695040888963407ull; return rng_state >> 16; }

// a block that ENDS at its last byte (aligned_alloc rounds a block to 16 bytes): the bytes, and the block to free.  (sz a multiple of 2 keeps
// the bytes 2-byte aligned, of 16 keeps them 16-byte aligned.)
static uint8_t *ending_block(size_t sz, uint8_t **blk) {
	const size_t cap = sz ? (sz + 15)/16*16 : 16;
	*blk = (uint8_t *)aligned_alloc(16, cap);
	memset(*blk, 0xCD, cap);
	return *blk + (cap - sz);
}

typedef __int128 wide;
struct V3 { wide x, y, z; };
static V3 sub(V3 a, V3 b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }
static wide dot(V3 a, V3 b) { return a.x*b.x + a.y*b.y + a.z*b.z; }
static V3 cross(V3 a, V3 b) { return V3{a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z, a.x*b.y - a.y*b.x}; }
static wide wabs(wide x) { return x < 0 ? -x : x; }

// the contract by brute force: every face, no tree
static crthip_cast_hit brute(const int32_t *pos, uint32_t nvert, const uint32_t *idx, uint32_t F, const int32_t base[3], const crthip_segment &s, uint32_t flags) {
	crthip_cast_hit r{CRTHIP_CAST_MISS, CRTHIP_NO_FACE, 0, 0, 0, 0};
	for(int c = 0; c < 3; c++) {
		const int64_t p = (int64_t)s.p[c] - base[c], q = (int64_t)s.q[c] - base[c];
		if(p < -(1 << 19) || p >= (1 << 19) || q < -(1 << 19) || q >= (1 << 19)) { r.status = CRTHIP_CAST_RANGE; return r; }
	}
	const V3 P{s.p[0], s.p[1], s.p[2]}, Q{s.q[0], s.q[1], s.q[2]}, d = sub(Q, P);
	wide bk = 0, bd = 0;
	for(uint32_t f = 0; f < F; f++) {
		const uint32_t *t = idx + (size_t)f*3;
		if(t[0] >= nvert || t[1] >= nvert || t[2] >= nvert) continue;
		auto at = [&](uint32_t v) { return V3{pos[(size_t)v*3], pos[(size_t)v*3 + 1], pos[(size_t)v*3 + 2]}; };
		const V3 A = sub(at(t[0]), P), B = sub(at(t[1]), P), C = sub(at(t[2]), P), n = cross(sub(B, A), sub(C, A));
		const wide D = dot(d, n), K = dot(A, n), U = dot(d, cross(B, C)), V = dot(d, cross(C, A)), W = dot(d, cross(A, B));
		if(D == 0 || !((U >= 0 && V >= 0 && W >= 0) || (U <= 0 && V <= 0 && W <= 0))) continue;
		if(!(K == 0 || (K < 0) == (D < 0)) || wabs(K) > wabs(D)) continue;
		if((flags & CRTHIP_CAST_FRONT) && D >= 0) continue;
		if(r.status == CRTHIP_CAST_HIT && !(wabs(K)*bd < bk*wabs(D))) continue;
		bk = wabs(K); bd = wabs(D);
		r = crthip_cast_hit{CRTHIP_CAST_HIT, f, D < 0 ? 1u : 0u, 0, (uint64_t)bk, (uint64_t)bd};
	}
	if(r.status == CRTHIP_CAST_HIT && (flags & CRTHIP_CAST_ANY)) r = crthip_cast_hit{CRTHIP_CAST_HIT, CRTHIP_NO_FACE, 0, 0, 0, 0};
	return r;
}

struct Blocks {
	uint8_t *nblk, *pblk, *iblk, *tblk, *sblk, *hblk;
	crthip_bvh_cast_set set;
	crthip_cast_hit *hits;
	void release() { free(nblk); free(pblk); free(iblk); free(tblk); free(sblk); free(hblk); }
};

// the set's arrays as blocks that end at their last byte; pos: absolute integers, base their minimum
static Blocks make(const std::vector<crthip_bvh_node> &nodes, const int32_t *pos, uint32_t nvert, const int32_t base[3], const uint32_t *idx, uint32_t F, int u16,
                   uint32_t stride, bool with_transform, const std::vector<crthip_segment> &segs, uint32_t flags) {
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
	crthip_segment *s = (crthip_segment *)ending_block(segs.size()*32, &b.sblk);
	memcpy(s, segs.data(), segs.size()*32);
	b.hits = (crthip_cast_hit *)ending_block(segs.size()*32, &b.hblk);
	b.set.nodes = n; b.set.position = p; b.set.index = ix; b.set.transform = with_transform ? t : nullptr; b.set.segments = s; b.set.hits = b.hits;
	for(int c = 0; c < 3; c++) b.set.base[c] = with_transform ? 0x5A5A5A5 : base[c];   // (with a record, base[] is not read)
	b.set.pos_stride = stride; b.set.nvert = nvert; b.set.nface = F; b.set.index_format = u16 ? CRTHIP_FMT_UINT16 : CRTHIP_FMT_UINT32;
	b.set.nseg = (uint32_t)segs.size(); b.set.flags = flags;
	return b;
}

static std::vector<crthip_segment> some_segments(const int32_t *pos, uint32_t nvert, const int32_t base[3], uint32_t n) {
	std::vector<crthip_segment> segs;
	for(uint32_t k = 0; k < n; k++) {
		crthip_segment s;
		memset(&s, 0xEE, sizeof s);
		const uint32_t v = (uint32_t)(rng() % nvert), w = (uint32_t)(rng() % nvert);
		for(int c = 0; c < 3; c++) {
			const int32_t jitter = k % 3 == 0 ? 0 : (int32_t)(rng() % 41) - 20;
			s.p[c] = pos[(size_t)v*3 + c] + (c == 2 ? 30 : 0) + jitter;
			s.q[c] = pos[(size_t)(k % 2 ? v : w)*3 + c] - (c == 2 ? 30 : 0);
		}
		if(k % 17 == 5) s.p[k % 3] = base[k % 3] + (1 << 19);               // just out of range
		if(k % 17 == 6) s.q[k % 3] = base[k % 3] - (1 << 19);               // the range's first value
		segs.push_back(s);
	}
	return segs;
}

// kind 0: a lattice patch with noise; 1: random strip; 2: with absent faces
static void one(uint32_t F, int kind, int u16, uint32_t stride) {
	rng_state = 0x9E3779B97F4A7C15ull ^ ((uint64_t)F*131u + kind*7u + u16);
	const uint32_t nvert = F + 2;
	std::vector<int32_t> pos((size_t)nvert*3);
	const uint32_t spread = kind == 0 ? 60 : 3000;
	for(size_t k = 0; k < pos.size(); k++) pos[k] = (int32_t)(rng() % spread) - (int32_t)(spread/2) + 70000;
	int32_t base[3] = {INT32_MAX, INT32_MAX, INT32_MAX};
	for(uint32_t v = 0; v < nvert; v++) for(int c = 0; c < 3; c++) if(pos[(size_t)v*3 + c] < base[c]) base[c] = pos[(size_t)v*3 + c];
	std::vector<uint32_t> idx((size_t)F*3);
	for(uint32_t f = 0; f < F; f++) {
		uint32_t id[3] = {f, f + 1, f + 2};
		if(kind == 2 && f % 5 == 1) id[f % 3] = u16 ? 0xFFFFu : nvert + (uint32_t)(rng() % 1000);
		for(int c = 0; c < 3; c++) idx[(size_t)f*3 + c] = id[c];
	}
	const std::vector<crthip_segment> segs = some_segments(pos.data(), nvert, base, 150);
	for(int which = 0; which < 2; which++) {
		if(which == 0 && !bvh_in_blob(F)) continue;
		std::vector<crthip_bvh_node> nodes(2*(size_t)F - 1);
		crthip_bvh_node *nb = (crthip_bvh_node *)aligned_alloc(16, nodes.size()*32);
		CHECK(crthip_bvh_model(pos.data(), nvert, idx.data(), 0, F, nb, nullptr, nullptr, nullptr, which, 3) == CRTHIP_OK, "the tree of F %u", F);
		memcpy(nodes.data(), nb, nodes.size()*32);
		free(nb);
		for(uint32_t flags = 0; flags < 4; flags++) {
			Blocks b = make(nodes, pos.data(), nvert, base, idx.data(), F, u16, stride, flags & 1, segs, flags);
			const int err = crthip_bvh_cast_model(&b.set, b.hits);
			CHECK(err == CRTHIP_OK, "F %u kind %d: %d", F, kind, err);
			uint32_t nhit = 0;
			for(size_t i = 0; i < segs.size() && !err; i++) {
				const crthip_cast_hit w = brute(pos.data(), nvert, idx.data(), F, base, segs[i], flags);
				nhit += w.status == CRTHIP_CAST_HIT;
				CHECK(memcmp(&w, &b.hits[i], 32) == 0, "F %u kind %d u16 %d stride %u which %d flags %u segment %zu: {%u %u %u %llu %llu}, expected {%u %u %u %llu %llu}", F, kind, u16,
				      stride, which, flags, i, b.hits[i].status, b.hits[i].face, b.hits[i].side, (unsigned long long)b.hits[i].num, (unsigned long long)b.hits[i].den,
				      w.status, w.face, w.side, (unsigned long long)w.num, (unsigned long long)w.den);
			}
			CHECK(kind == 2 || nhit > 0, "F %u kind %d: nothing was hit", F, kind);
			b.release();
		}
	}
}

static crthip_bvh_node node(int32_t lo, uint32_t left, int32_t hi, uint32_t right) { return crthip_bvh_node{{lo, lo, lo}, left, {hi, hi, hi}, right}; }

// corrupt trees over F copies of one face that no segment meets: kind 0 a cycle, 1 a node its own child, 2 a child id out of range, 3 a leaf's
// face out of range, 4 a chain of 70 down the left side, 5 random bytes
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
	std::vector<crthip_segment> segs(66);
	for(size_t k = 0; k < segs.size(); k++) { memset(&segs[k], 0, 32); segs[k].p[0] = segs[k].q[0] = (int32_t)k; segs[k].p[2] = 510 + (int32_t)k; segs[k].q[2] = 520; }
	for(uint32_t flags = 0; flags < 2; flags++) {
		Blocks b = make(nodes, pos, 3, base, idx.data(), F, 0, 8, false, segs, flags);
		const int err = crthip_bvh_cast_model(&b.set, b.hits);
		CHECK(err == CRTHIP_OK, "corrupt %d: %d", kind, err);
		for(size_t i = 0; i < segs.size() && !err; i++) {
			const crthip_cast_hit &h = b.hits[i];
			if(kind < 5) CHECK(h.status == CRTHIP_CAST_TREE && h.face == CRTHIP_NO_FACE && !h.side && !h.reserved && !h.num && !h.den, "corrupt %d F %u segment %zu: status %u", kind, F, i, h.status);
			else CHECK(h.status <= CRTHIP_CAST_TREE && !h.reserved, "corrupt %d F %u segment %zu: status %u", kind, F, i, h.status);
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
		crthip_bvh_cast_set s;
		memset(&s, 0, sizeof s);
		CHECK(crthip_bvh_cast_model(nullptr, nullptr) == CRTHIP_E_ARGUMENT, "a null set");
		CHECK(crthip_bvh_cast_model(&s, nullptr) == CRTHIP_E_ARGUMENT, "no faces");
		s.nface = 1;
		CHECK(crthip_bvh_cast_model(&s, nullptr) == CRTHIP_OK, "no segments");
		s.flags = 4;
		CHECK(crthip_bvh_cast_model(&s, nullptr) == CRTHIP_E_ARGUMENT, "unknown flags");
	}
	if(failures) { printf("bvh_cast_check: %d failures\n", failures); return 1; }
	printf("bvh_cast_check ok\n");
	return 0;
}
