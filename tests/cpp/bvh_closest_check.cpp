// bvh_closest_check.cpp — csrc/bvh_closest.h on the host under AddressSanitizer and UBSan (tests/test_bvh_closest_sanitize_cpu.py): a
// stand-alone program, host code only.  Every array of a set is a heap block of its own that ENDS exactly where the contract says the array
// ends: the nodes at the last of 2F - 1 records, the position at the last vertex's sixth byte (at stride 8: two bytes short of a whole
// record), the index at its last entry, the transform at its 48th byte, the points at their last record and the hits at their last record -
// a load or a store one byte past any of them is reported.  (The hook's own stack block is made at exactly the kernel's LDS size: a push
// past entry 64 is reported too.)  The trees are crthip_bvh_model's, both partitions, in both child orders, and corrupt ones: a cycle, a
// child id out of range, a leaf with a face id out of range, a chain deeper than 65, random bytes - each must end, and the hand-made ones
// with CRTHIP_CLOSEST_TREE.  The records are compared with a brute force over all faces that words the contract's candidate rule on
// __int128 and compares two distances by limbs of its own - nothing of bvh_closest.h's arithmetic.
// Built with csrc/bvh_closest_host.cpp and csrc/bvh_host.cpp, whose one dependency on the library (ctx_fail) is defined here.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/corto_hip.h"
#include "bvh.h"
#include "bvh_closest.h"

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
typedef unsigned __int128 uwide;
struct V3 { wide c[3]; };
static V3 sub(V3 a, V3 b) { return V3{{a.c[0] - b.c[0], a.c[1] - b.c[1], a.c[2] - b.c[2]}}; }
static wide dot(V3 a, V3 b) { return a.c[0]*b.c[0] + a.c[1]*b.c[1] + a.c[2]*b.c[2]; }
static V3 cross(V3 a, V3 b) { return V3{{a.c[1]*b.c[2] - a.c[2]*b.c[1], a.c[2]*b.c[0] - a.c[0]*b.c[2], a.c[0]*b.c[1] - a.c[1]*b.c[0]}}; }

// a*b < c*d for values below 2^128: schoolbook on 32-bit limbs, eight a factor
static bool product_less(uwide a, uwide b, uwide c, uwide d) {
	auto mul = [](uwide x, uwide y, uint64_t out[8]) {
		uint64_t acc[9] = {0};
		for(int i = 0; i < 4; i++) {
			uint64_t carry = 0;
			for(int j = 0; j < 4; j++) {
				const uint64_t t = (uint64_t)(uint32_t)(x >> (32*i))*(uint64_t)(uint32_t)(y >> (32*j)) + acc[i + j] + carry;
				acc[i + j] = (uint32_t)t; carry = t >> 32;
			}
			acc[i + 4] += carry;
		}
		for(int k = 0; k < 8; k++) out[k] = acc[k];
	};
	uint64_t p[8], q[8];
	mul(a, b, p); mul(c, d, q);
	for(int k = 7; k >= 0; k--) if(p[k] != q[k]) return p[k] < q[k];
	return false;
}

struct Dist { uwide num, den; uint32_t feature; };

// the contract's candidate rule for one present face, the corners relative to the point
static Dist brute_face(const V3 A[3]) {
	Dist best{(uwide)dot(A[0], A[0]), 1, 0};
	for(uint32_t k = 1; k < 3; k++) if((uwide)dot(A[k], A[k]) < best.num) best = Dist{(uwide)dot(A[k], A[k]), 1, k};
	V3 e[3], c[3];
	for(int i = 0; i < 3; i++) { e[i] = sub(A[(i + 1) % 3], A[i]); c[i] = cross(A[i], e[i]); }
	for(uint32_t i = 0; i < 3; i++) {
		const wide ee = dot(e[i], e[i]), s = -dot(A[i], e[i]);
		if(ee > 0 && s >= 0 && s <= ee && product_less((uwide)dot(c[i], c[i]), best.den, best.num, (uwide)ee)) best = Dist{(uwide)dot(c[i], c[i]), (uwide)ee, 3 + i};
	}
	const V3 n = cross(e[0], e[1]);
	const wide nn = dot(n, n);
	if(nn > 0 && dot(c[0], n) >= 0 && dot(c[1], n) >= 0 && dot(c[2], n) >= 0) {
		const wide k = dot(n, A[0]);
		if(product_less((uwide)(k*k), best.den, best.num, (uwide)nn)) best = Dist{(uwide)(k*k), (uwide)nn, 6};
	}
	return best;
}

// the contract by brute force: every face, no tree
static crthip_closest_hit brute(const int32_t *pos, uint32_t nvert, const uint32_t *idx, uint32_t F, const int32_t base[3], const crthip_point &p, uint32_t flags) {
	const crthip_closest_hit none{CRTHIP_CLOSEST_MISS, CRTHIP_NO_FACE, 0, 0, 0, 0, 0, 0};
	for(int c = 0; c < 3; c++) {
		const int64_t x = (int64_t)p.p[c] - base[c];
		if(x < -(1 << 19) || x >= (1 << 19)) { crthip_closest_hit r = none; r.status = CRTHIP_CLOSEST_RANGE; return r; }
	}
	bool have = false;
	Dist best{0, 1, 0};
	uint32_t face = CRTHIP_NO_FACE;
	for(uint32_t f = 0; f < F; f++) {
		const uint32_t *t = idx + (size_t)f*3;
		if(t[0] >= nvert || t[1] >= nvert || t[2] >= nvert) continue;
		V3 A[3];
		for(int k = 0; k < 3; k++) for(int c = 0; c < 3; c++) A[k].c[c] = (wide)pos[(size_t)t[k]*3 + c] - p.p[c];
		const Dist d = brute_face(A);
		if(!have || product_less(d.num, best.den, best.num, d.den)) { best = d; face = f; have = true; }   // (ascending f: a tie keeps the lower id)
	}
	if(!have) return none;
	if(flags & CRTHIP_CLOSEST_WITHIN) {
		const uwide r = p.radius < (1u << 21) ? p.radius : (1u << 21);
		if(product_less(r*r, best.den, best.num, 1)) return none;
		if(flags & CRTHIP_CLOSEST_ANY) { crthip_closest_hit h = none; h.status = CRTHIP_CLOSEST_HIT; return h; }
	}
	return crthip_closest_hit{CRTHIP_CLOSEST_HIT, face, best.feature, 0, (uint64_t)best.num, (uint64_t)(best.num >> 64), (uint64_t)best.den, (uint64_t)(best.den >> 64)};
}

struct Blocks {
	uint8_t *nblk, *pblk, *iblk, *tblk, *sblk, *hblk;
	crthip_bvh_closest_set set;
	crthip_closest_hit *hits;
	void release() { free(nblk); free(pblk); free(iblk); free(tblk); free(sblk); free(hblk); }
};

// the set's arrays as blocks that end at their last byte; pos: absolute integers, base their minimum
static Blocks make(const std::vector<crthip_bvh_node> &nodes, const int32_t *pos, uint32_t nvert, const int32_t base[3], const uint32_t *idx, uint32_t F, int u16,
                   uint32_t stride, bool with_transform, const std::vector<crthip_point> &points, uint32_t flags) {
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
	crthip_point *s = (crthip_point *)ending_block(points.size()*16, &b.sblk);
	memcpy(s, points.data(), points.size()*16);
	b.hits = (crthip_closest_hit *)ending_block(points.size()*48, &b.hblk);
	b.set.nodes = n; b.set.position = p; b.set.index = ix; b.set.transform = with_transform ? t : nullptr; b.set.points = s; b.set.hits = b.hits;
	for(int c = 0; c < 3; c++) b.set.base[c] = with_transform ? 0x5A5A5A5 : base[c];   // (with a record, base[] is not read)
	b.set.pos_stride = stride; b.set.nvert = nvert; b.set.nface = F; b.set.index_format = u16 ? CRTHIP_FMT_UINT16 : CRTHIP_FMT_UINT32;
	b.set.npoint = (uint32_t)points.size(); b.set.flags = flags;
	return b;
}

static std::vector<crthip_point> some_points(const int32_t *pos, uint32_t nvert, const int32_t base[3], uint32_t n, int32_t reach) {
	std::vector<crthip_point> points;
	for(uint32_t k = 0; k < n; k++) {
		crthip_point p;
		const uint32_t v = (uint32_t)(rng() % nvert);
		for(int c = 0; c < 3; c++) p.p[c] = pos[(size_t)v*3 + c] + (k % 4 == 0 ? 0 : (int32_t)(rng() % (2*reach + 1)) - reach);   // every fourth: a vertex itself
		p.radius = k % 5 == 0 ? 0u : k % 5 == 1 ? 0xFFFFFFFFu : (uint32_t)(rng() % (2*reach));
		if(k % 17 == 5) p.p[k % 3] = base[k % 3] + (1 << 19);                   // just out of range
		if(k % 17 == 6) p.p[k % 3] = base[k % 3] - (1 << 19);                   // the range's first value
		if(k % 23 == 7) for(int c = 0; c < 3; c++) p.p[c] = base[c] + ((rng() & 1) ? (1 << 19) - 1 : -(1 << 19));   // a corner of the range
		points.push_back(p);
	}
	return points;
}

// kind 0: a small patch of noise; 1: random strip with segments; 2: with absent faces; 3: corners at 0 and 65 535 (products beyond 128 bits)
static void one(uint32_t F, int kind, int u16, uint32_t stride) {
	rng_state = 0x9E3779B97F4A7C15ull ^ ((uint64_t)F*131u + kind*7u + u16);
	const uint32_t nvert = F + 2;
	std::vector<int32_t> pos((size_t)nvert*3);
	const uint32_t spread = kind == 0 ? 60 : 3000;
	for(size_t k = 0; k < pos.size(); k++) pos[k] = kind == 3 ? ((rng() & 1) ? 65535 : 0) - 40000 : (int32_t)(rng() % spread) - (int32_t)(spread/2) + 70000;
	int32_t base[3] = {INT32_MAX, INT32_MAX, INT32_MAX};
	for(uint32_t v = 0; v < nvert; v++) for(int c = 0; c < 3; c++) if(pos[(size_t)v*3 + c] < base[c]) base[c] = pos[(size_t)v*3 + c];
	std::vector<uint32_t> idx((size_t)F*3);
	for(uint32_t f = 0; f < F; f++) {
		uint32_t id[3] = {f, f + 1, f + 2};
		if(kind == 2 && f % 5 == 1) id[f % 3] = u16 ? 0xFFFFu : nvert + (uint32_t)(rng() % 1000);
		if(kind == 1 && f % 7 == 3) id[1] = id[0];                          // a segment
		for(int c = 0; c < 3; c++) idx[(size_t)f*3 + c] = id[c];
	}
	const std::vector<crthip_point> points = some_points(pos.data(), nvert, base, 150, kind == 3 ? 400000 : kind == 0 ? 20 : 300);
	for(int which = 0; which < 2; which++) {
		if(which == 0 && !bvh_in_blob(F)) continue;
		std::vector<crthip_bvh_node> nodes(2*(size_t)F - 1);
		crthip_bvh_node *nb = (crthip_bvh_node *)aligned_alloc(16, nodes.size()*32);
		CHECK(crthip_bvh_model(pos.data(), nvert, idx.data(), 0, F, nb, nullptr, nullptr, nullptr, which, 3) == CRTHIP_OK, "the tree of F %u", F);
		memcpy(nodes.data(), nb, nodes.size()*32);
		free(nb);
		const uint32_t flagset[3] = {0, CRTHIP_CLOSEST_WITHIN, CRTHIP_CLOSEST_WITHIN | CRTHIP_CLOSEST_ANY};
		for(uint32_t fi = 0; fi < 3; fi++) for(uint32_t order = 0; order < 2; order++) {
			const uint32_t flags = flagset[fi];
			Blocks b = make(nodes, pos.data(), nvert, base, idx.data(), F, u16, stride, (fi + order) & 1, points, flags);
			uint64_t stats[2];
			const int err = crthip_bvh_closest_model_stats(&b.set, b.hits, stats, order);
			CHECK(err == CRTHIP_OK, "F %u kind %d: %d", F, kind, err);
			uint32_t nhit = 0;
			for(size_t i = 0; i < points.size() && !err; i++) {
				const crthip_closest_hit w = brute(pos.data(), nvert, idx.data(), F, base, points[i], flags), &g = b.hits[i];
				nhit += w.status == CRTHIP_CLOSEST_HIT;
				CHECK(memcmp(&w, &g, 48) == 0, "F %u kind %d u16 %d stride %u which %d flags %u order %u point %zu: {%u %u %u %u %llx:%llx / %llx:%llx}, expected {%u %u %u %llx:%llx / %llx:%llx}",
				      F, kind, u16, stride, which, flags, order, i, g.status, g.face, g.feature, g.reserved, (unsigned long long)g.num_hi, (unsigned long long)g.num_lo,
				      (unsigned long long)g.den_hi, (unsigned long long)g.den_lo, w.status, w.face, w.feature, (unsigned long long)w.num_hi, (unsigned long long)w.num_lo,
				      (unsigned long long)w.den_hi, (unsigned long long)w.den_lo);
			}
			CHECK(nhit > 0 || kind == 2, "F %u kind %d flags %u: nothing hit", F, kind, flags);
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
	std::vector<crthip_point> points(66);
	for(size_t k = 0; k < points.size(); k++) {                               // about the face, and from the 40th on far beside it
		for(int c = 0; c < 3; c++) points[k].p[c] = (k < 40 ? 3 : 3000) - (int32_t)k + (c == 2 ? 500 : 0);
		points[k].radius = (uint32_t)k*100;
	}
	const uint32_t flagset[3] = {0, CRTHIP_CLOSEST_WITHIN, CRTHIP_CLOSEST_WITHIN | CRTHIP_CLOSEST_ANY};
	for(uint32_t flags : flagset) for(uint32_t order = 0; order < 2; order++) {
		Blocks b = make(nodes, pos, 3, base, idx.data(), F, 0, 8, false, points, flags);
		const int err = crthip_bvh_closest_model_stats(&b.set, b.hits, nullptr, order);
		CHECK(err == CRTHIP_OK, "corrupt %d: %d", kind, err);
		for(size_t i = 0; i < points.size() && !err; i++) {
			const crthip_closest_hit &r = b.hits[i];
			const bool named = r.status == CRTHIP_CLOSEST_HIT && r.face != CRTHIP_NO_FACE;
			// (without a radius nothing is skipped before a bound trips; with one, a walk may rightly end on what it found first)
			if(kind < 5 && !flags) CHECK(r.status == CRTHIP_CLOSEST_TREE, "corrupt %d F %u point %zu: status %u", kind, F, i, r.status);
			CHECK(r.status <= CRTHIP_CLOSEST_TREE && !r.reserved && r.feature <= 6, "corrupt %d F %u point %zu: status %u", kind, F, i, r.status);
			if(named) CHECK(r.face < F && (r.den_lo | r.den_hi) && !(flags & CRTHIP_CLOSEST_ANY), "corrupt %d F %u point %zu: face %u", kind, F, i, r.face);
			else CHECK(r.face == CRTHIP_NO_FACE && !r.feature && !r.num_lo && !r.num_hi && !r.den_lo && !r.den_hi, "corrupt %d F %u point %zu: a record without a face holds one", kind, F, i);
		}
		b.release();
	}
}

int main() {
	const uint32_t sizes[] = {1, 2, 3, 17, 257, BVH_BLOB_FACES, BVH_BLOB_FACES + 1};
	for(uint32_t F : sizes)
		for(int kind = 0; kind < 4; kind++) {
			if(F >= BVH_BLOB_FACES && kind != 0) continue;
			if(kind == 3 && F > 17) continue;
			one(F, kind, (F + kind) & 1, (F + kind) % 3 == 0 ? 8 : (F + kind) % 3 == 1 ? 0 : 6);
		}
	corrupt(0, 2); corrupt(0, 300); corrupt(1, 2); corrupt(1, 40); corrupt(2, 2); corrupt(3, 2); corrupt(4, 100); corrupt(5, 1); corrupt(5, 2); corrupt(5, 77);
	// the set's own checks reach the hook too
	{
		crthip_bvh_closest_set s;
		memset(&s, 0, sizeof s);
		CHECK(crthip_bvh_closest_model(nullptr, nullptr) == CRTHIP_E_ARGUMENT, "a null set");
		CHECK(crthip_bvh_closest_model(&s, nullptr) == CRTHIP_E_ARGUMENT, "no faces");
		s.nface = 1;
		CHECK(crthip_bvh_closest_model(&s, nullptr) == CRTHIP_OK, "no points");
		s.flags = 4;
		CHECK(crthip_bvh_closest_model(&s, nullptr) == CRTHIP_E_ARGUMENT, "unknown flags");
		s.flags = CRTHIP_CLOSEST_ANY;
		CHECK(crthip_bvh_closest_model(&s, nullptr) == CRTHIP_E_ARGUMENT, "ANY without WITHIN");
		s.flags = 0;
		CHECK(crthip_bvh_closest_model_stats(&s, nullptr, nullptr, 2) == CRTHIP_E_ARGUMENT, "an unknown order");
	}
	if(failures) { printf("bvh_closest_check: %d failures\n", failures); return 1; }
	printf("bvh_closest_check ok\n");
	return 0;
}
