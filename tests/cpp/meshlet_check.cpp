// meshlet_check.cpp — both partitions of csrc/meshlet.h on the host under AddressSanitizer and UBSan (tests/test_meshlets_sanitize_cpu.py): a
// stand-alone program, host code only.  The index, the group table and each of the three arrays is a heap block of its own.  A first run gets
// arrays that END exactly at crthip_meshlet_bound's capacities; a second one arrays that end exactly at the COUNTS the first reported (the
// capacities in the binding stay the bound's): a store one byte past what the contract allows is reported either way.  The two partitions
// must leave the same bytes under every seed.  Built with csrc/meshlet_host.cpp, whose one dependency on the library (ctx_fail) is defined here.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/corto_hip.h"
#include "meshlet.h"

using namespace corto_hip;

namespace corto_hip { int ctx_fail(int code, const char *) { return code; } }

static int failures = 0;
#define CHECK(cond, ...) do { if(!(cond)) { failures++; printf("FAILED %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } while(0)

static uint64_t rng_state;
static uint64_t rng() { rng_state = rng_state*6364136223846793005ull + 1442695040888963407ull; return rng_state >> 16; }

static void one(uint32_t nface, uint32_t nvert, int kind, bool u16, uint32_t ngroups, uint32_t mv, uint32_t mt, uint32_t sf, uint32_t seed) {
	rng_state = 0x9E3779B97F4A7C15ull ^ ((uint64_t)nface*131u + nvert*7u + seed);
	void *faces = malloc(nface ? (size_t)nface*3*(u16 ? 2 : 4) : 1);
	for(size_t e = 0; e < (size_t)nface*3; e++) {
		uint32_t v;
		if(kind == 0) v = (uint32_t)(rng() % nvert);                          // random
		else if(kind == 1) v = (uint32_t)(e/3 + e%3);                          // a strip
		else if(kind == 2) v = (uint32_t)e;                                    // three new vertices a face
		else v = 0xFFFFFFFFu - (uint32_t)(rng() % nvert);                      // ids at the top of 32 bits
		if(rng() % 13 == 0 && e%3) v = u16 ? ((uint16_t *)faces)[e - 1] : ((uint32_t *)faces)[e - 1];   // a repeated corner
		if(u16) ((uint16_t *)faces)[e] = (uint16_t)v; else ((uint32_t *)faces)[e] = v;
	}
	uint32_t *groups = (uint32_t *)malloc(ngroups ? ngroups*4 : 1);
	for(uint32_t g = 0; g < ngroups; g++) groups[g] = (uint32_t)(rng() % (nface + 3));    // unsorted, repeated, beyond nface
	crthip_meshlet_counts bound;
	CHECK(crthip_meshlet_bound(nface, ngroups, groups, mv, mt, sf, &bound) == 0, "bound nface %u", nface);
	std::vector<uint8_t> ref[3]; crthip_meshlet_counts refc{};
	for(int pass = 0; pass < 2; pass++) for(int which = 0; which < 2; which++) for(uint32_t s = 0; s < 2; s++) {
		// pass 0: blocks that end at the bound; pass 1: at the counts
		const size_t nb[3] = {pass ? (size_t)refc.meshlets*16 : (size_t)bound.meshlets*16, pass ? (size_t)refc.vertices*4 : (size_t)bound.vertices*4,
			pass ? (size_t)refc.triangle_bytes : (size_t)bound.triangle_bytes};
		// every array at the END of a block of its own (aligned_alloc rounds a block to 16 bytes): its last byte is the block's last byte
		uint8_t *blk[3], *arr[3];
		for(int a = 0; a < 3; a++) {
			const size_t al = a == 0 ? 16 : 4, sz = (nb[a] + al - 1)/al*al, cap = sz ? (sz + 15)/16*16 : 16;
			blk[a] = (uint8_t *)aligned_alloc(16, cap);
			memset(blk[a], 0xCD, cap);
			arr[a] = blk[a] + (cap - sz);
		}
		crthip_meshlet_binding m{};
		m.meshlets = (crthip_meshlet *)arr[0]; m.vertices = (uint32_t *)arr[1]; m.triangles = arr[2];
		m.meshlet_capacity = bound.meshlets; m.vertex_capacity = bound.vertices; m.triangle_capacity = bound.triangle_bytes;
		m.max_vertices = mv; m.max_triangles = mt; m.segment_faces = sf;
		crthip_meshlet_counts c{};
		const int rc = crthip_meshlet_model(faces, u16, nface, ngroups, groups, &m, &c, which, seed + s);
		CHECK(rc == 0, "rc %d nface %u which %d", rc, nface, which);
		CHECK(c.meshlets <= bound.meshlets && c.vertices <= bound.vertices && c.triangle_bytes <= bound.triangle_bytes && c.segments == bound.segments, "counts beyond the bound nface %u", nface);
		const size_t used[3] = {(size_t)c.meshlets*16, (size_t)c.vertices*4, (size_t)c.triangle_bytes};
		if(pass == 0 && which == 0 && s == 0) { refc = c; for(int a = 0; a < 3; a++) ref[a].assign(arr[a], arr[a] + used[a]); }
		else {
			CHECK(memcmp(&c, &refc, sizeof c) == 0, "counts differ nface %u which %d", nface, which);
			for(int a = 0; a < 3; a++) CHECK(used[a] == ref[a].size() && (used[a] == 0 || memcmp(ref[a].data(), arr[a], used[a]) == 0), "array %d differs: nface %u which %d seed %u pass %d", a, nface, which, seed + s, pass);
		}
		for(int a = 0; a < 3; a++) { for(size_t b = used[a]; b < nb[a]; b++) if(arr[a][b] != 0xCD) { CHECK(false, "array %d written past the counts nface %u", a, nface); break; } free(blk[a]); }
	}
	free(faces); free(groups);
}

int main() {
	const uint32_t params[][3] = {{64, 124, 0}, {64, 124, 64}, {8, 4, 16}, {3, 1, 1}, {255, 512, 65536}, {4, 512, 0}, {64, 64, 63}, {255, 85, 65}};
	const uint32_t sizes[] = {0, 1, 2, 63, 64, 65, 128, 129, 700, 4097, 9000};
	uint32_t runs = 0;
	for(uint32_t nface : sizes) for(const auto &p : params) for(int kind = 0; kind < 4; kind++) {
		if(nface > 1000 && (p[2] == 1 || kind == 3)) continue;                 // (keep the run short)
		const bool u16 = (runs & 1) && kind != 3 && 3ull*nface + 3 < 65536;
		one(nface, kind == 0 ? 40 + 50*(runs%7) : 90, kind, u16, runs%4 == 0 ? 0 : runs%5, p[0], p[1], p[2], runs); runs++;
	}
	if(failures) { printf("meshlet_check: %d failures\n", failures); return 1; }
	printf("meshlet_check ok (%u runs)\n", runs);
	return 0;
}
