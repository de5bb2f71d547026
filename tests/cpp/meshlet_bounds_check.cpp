// meshlet_bounds_check.cpp — csrc/meshlet_bounds.h on the host under AddressSanitizer and UBSan (tests/test_meshlet_bounds_sanitize_cpu.py): a
// stand-alone program, host code only.  The meshlets come from crthip_meshlet_model; the positions, the three meshlet arrays and the records
// are heap blocks of their own that END exactly at what the contract lets the pass touch: nvert positions, the COUNTS of the three arrays, and
// counts.meshlets records (the grid is sized by the bound all the same, as the kernel's is).  A load or a store one byte past any of them is
// reported.  Every seed must leave the same bytes.  Built with csrc/meshlet_host.cpp and csrc/meshlet_bounds_host.cpp, whose one dependency
// on the library (ctx_fail) is defined here.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/corto_hip.h"
#include "meshlet_bounds.h"

using namespace corto_hip;

namespace corto_hip { int ctx_fail(int code, const char *) { return code; } }

static int failures = 0;
#define CHECK(cond, ...) do { if(!(cond)) { failures++; printf("FAILED %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } while(0)

static uint64_t rng_state;
static uint64_t rng() { rng_state = rng_state*6364136223846793005ull + 1442695040888963407ull; return rng_state >> 16; }

// a block whose last byte is the array's last byte
struct Tail {
	uint8_t *blk = nullptr, *arr = nullptr;
	Tail(size_t bytes, size_t align) { const size_t sz = (bytes + align - 1)/align*align, cap = sz ? (sz + 15)/16*16 : 16; blk = (uint8_t *)aligned_alloc(16, cap); memset(blk, 0xCD, cap); arr = blk + (cap - sz); }
	~Tail() { free(blk); }
};

static void one(uint32_t nface, uint32_t nvert, int kind, uint32_t absent, uint32_t mv, uint32_t mt, uint32_t sf, uint32_t seed) {
	rng_state = 0x9E3779B97F4A7C15ull ^ ((uint64_t)nface*131u + nvert*7u + seed);
	std::vector<uint32_t> faces((size_t)nface*3 + 1);
	for(size_t e = 0; e < (size_t)nface*3; e++) {
		uint32_t v = kind == 0 ? (uint32_t)(rng() % nvert) : kind == 1 ? (uint32_t)((e/3 + e%3) % nvert) : (uint32_t)(e % nvert);
		if(absent && rng() % absent == 0) v = rng() % 2 ? nvert + (uint32_t)(rng() % 5) : 0xFFFFFFFFu - (uint32_t)(rng() % 5);   // ids the positions do not have
		if(rng() % 13 == 0 && e%3) v = faces[e - 1];                           // a repeated corner: a degenerate face
		faces[e] = v;
	}
	crthip_meshlet_counts bound;
	CHECK(crthip_meshlet_bound(nface, 0, nullptr, mv, mt, sf, &bound) == 0, "bound nface %u", nface);
	Tail bm((size_t)bound.meshlets*16, 16), bv((size_t)bound.vertices*4, 4), bt(bound.triangle_bytes, 4);
	crthip_meshlet_binding m{};
	m.meshlets = (crthip_meshlet *)bm.arr; m.vertices = (uint32_t *)bv.arr; m.triangles = bt.arr;
	m.meshlet_capacity = bound.meshlets; m.vertex_capacity = bound.vertices; m.triangle_capacity = bound.triangle_bytes;
	m.max_vertices = mv; m.max_triangles = mt; m.segment_faces = sf;
	crthip_meshlet_counts c{};
	CHECK(crthip_meshlet_model(faces.data(), 0, nface, 0, nullptr, &m, &c, 0, seed) == 0, "meshlets nface %u", nface);
	// the inputs again, each in a block that ends at its count
	Tail pos((size_t)nvert*12, 4), am((size_t)c.meshlets*16, 16), av((size_t)c.vertices*4, 4), at(c.triangle_bytes, 4);
	int32_t *p = (int32_t *)pos.arr;
	for(size_t e = 0; e < (size_t)nvert*3; e++) {
		const uint64_t r = rng();
		p[e] = kind == 2 ? (int32_t)(uint32_t)(r % 7 == 0 ? 0x80000000u : r % 7 == 1 ? 0x7FFFFFFFu : (uint32_t)r) : (int32_t)(r % 20001) - 10000;   // kind 2: all of int32, its ends too
	}
	memcpy(am.arr, bm.arr, (size_t)c.meshlets*16); memcpy(av.arr, bv.arr, (size_t)c.vertices*4); memcpy(at.arr, bt.arr, c.triangle_bytes);
	std::vector<uint8_t> ref;
	for(uint32_t s = 0; s < 3; s++) {
		Tail out((size_t)c.meshlets*48, 16);
		const int rc = crthip_meshlet_bounds_model(nvert ? p : nullptr, nvert, (const crthip_meshlet *)am.arr, (const uint32_t *)av.arr, at.arr, &c,
			(crthip_meshlet_bounds *)out.arr, bound.meshlets, seed + s);
		CHECK(rc == 0, "rc %d nface %u", rc, nface);
		if(s == 0) ref.assign(out.arr, out.arr + (size_t)c.meshlets*48);
		else CHECK(ref.size() == (size_t)c.meshlets*48 && (ref.empty() || memcmp(ref.data(), out.arr, ref.size()) == 0), "records differ: nface %u seed %u", nface, seed + s);
		for(uint32_t k = 0; k < c.meshlets; k++) CHECK(((const crthip_meshlet_bounds *)out.arr)[k].reserved == 0, "reserved nface %u", nface);
	}
}

int main() {
	const uint32_t params[][3] = {{64, 124, 0}, {64, 124, 64}, {8, 4, 16}, {3, 1, 1}, {255, 512, 65536}, {4, 512, 0}, {64, 64, 63}, {255, 85, 65}};
	const uint32_t sizes[] = {0, 1, 2, 63, 64, 65, 128, 129, 700, 4097};
	uint32_t runs = 0;
	for(uint32_t nface : sizes) for(const auto &p : params) for(int kind = 0; kind < 3; kind++) {
		if(nface > 1000 && p[2] == 1) continue;                                // (keep the run short)
		const uint32_t nvert = runs%11 == 0 ? 1 : kind == 0 ? 40 + 50*(runs%7) : 300;
		one(nface, nvert, kind, runs%3 == 0 ? 0 : 4 + runs%9, p[0], p[1], p[2], runs); runs++;
	}
	if(failures) { printf("meshlet_bounds_check: %d failures\n", failures); return 1; }
	printf("meshlet_bounds_check ok (%u runs)\n", runs);
	return 0;
}
