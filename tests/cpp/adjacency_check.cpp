// adjacency_check.cpp — both partitions of csrc/adjacency.h on the host under AddressSanitizer and UBSan (tests/test_adjacency_sanitize_cpu.py): a
// stand-alone program, host code only.  The index, the twin array and the record are heap blocks of their own: the twin array ENDS exactly at
// 3*nface words and the record is a block of exactly 16 bytes, so a store one byte past what the contract allows is reported.  (The hook's own
// lists are vectors of exactly nvert + 1 ends and 3*nface entries: an id >= nvert used as an address is reported too.)  The indices hold ids
// at and beyond nvert and repeated corners.  The two partitions must leave the same bytes under every seed.  Built with
// csrc/adjacency_host.cpp, whose one dependency on the library (ctx_fail) is defined here.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/corto_hip.h"
#include "adjacency.h"

using namespace corto_hip;

namespace corto_hip { int ctx_fail(int code, const char *) { return code; } }

static int failures = 0;
#define CHECK(cond, ...) do { if(!(cond)) { failures++; printf("FAILED %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } while(0)

static uint64_t rng_state;
static uint64_t rng() { rng_state = rng_state*6364136223846793005ull + 1442695040888963407ull; return rng_state >> 16; }

static void one(uint32_t nface, uint32_t nvert, int kind, bool u16, uint32_t seed) {
	rng_state = 0x9E3779B97F4A7C15ull ^ ((uint64_t)nface*131u + nvert*7u + seed);
	void *faces = malloc(nface ? (size_t)nface*3*(u16 ? 2 : 4) : 1);
	for(size_t e = 0; e < (size_t)nface*3; e++) {
		uint32_t v;
		if(kind == 0) v = (uint32_t)(rng() % (nvert + nvert/8 + 1));           // random, an eighth of the ids at or beyond nvert
		else if(kind == 1) v = (uint32_t)((e/3 + e%3) % nvert);                 // a strip
		else if(kind == 2) v = e%3 == 0 ? 0u : (uint32_t)(1 + (e/3 + e%3 - 1) % (nvert - 1));   // a fan round vertex 0: one long list
		else v = rng() % 3 ? (uint32_t)(rng() % nvert) : 0xFFFFFFFFu - (uint32_t)(rng() % 5);   // ids at the top of 32 bits among good ones
		if(rng() % 13 == 0 && e%3) v = u16 ? ((uint16_t *)faces)[e - 1] : ((uint32_t *)faces)[e - 1];   // a repeated corner
		if(u16) ((uint16_t *)faces)[e] = (uint16_t)v; else ((uint32_t *)faces)[e] = v;
	}
	const size_t words = (size_t)nface*3;
	std::vector<uint32_t> ref; crthip_adjacency_counts refc{};
	for(int which = 0; which < 2; which++) for(uint32_t s = 0; s < 3; s++) {
		if(which == 0 && !adj_in_blob(nvert, nface)) continue;
		// the twin array at the END of a block of its own (aligned_alloc rounds a block to 16 bytes): its last byte is the block's last byte
		const size_t sz = words*4, cap = sz ? (sz + 15)/16*16 : 16;
		uint8_t *blk = (uint8_t *)aligned_alloc(16, cap);
		memset(blk, 0xCD, cap);
		uint32_t *twin = (uint32_t *)(blk + (cap - sz));
		crthip_adjacency_counts *rec = (crthip_adjacency_counts *)aligned_alloc(16, 16);
		memset(rec, 0xCD, 16);
		const int rc = crthip_adjacency_model(faces, u16, nface, nvert, nface ? twin : nullptr, rec, which, seed + s);
		CHECK(rc == 0, "rc %d nface %u which %d", rc, nface, which);
		CHECK(rec->halfedges == words && (uint64_t)rec->boundary + rec->invalid <= words && rec->duplicate <= words, "counts nface %u which %d", nface, which);
		for(size_t h = 0; h < words; h++) if(twin[h] != CRTHIP_NO_TWIN && twin[h] >= words) { CHECK(false, "twin[%zu] = %u nface %u", h, twin[h], nface); break; }
		if(ref.empty() && !refc.halfedges) { refc = *rec; ref.assign(twin, twin + words); }
		else {
			CHECK(memcmp(rec, &refc, sizeof refc) == 0, "counts differ nface %u which %d seed %u", nface, which, seed + s);
			CHECK(ref.size() == words && (words == 0 || memcmp(ref.data(), twin, sz) == 0), "twins differ: nface %u which %d seed %u", nface, which, seed + s);
		}
		for(uint8_t *p = blk; p < (uint8_t *)twin; p++) if(*p != 0xCD) { CHECK(false, "written in front of twin nface %u", nface); break; }
		free(blk); free(rec);
	}
	free(faces);
}

int main() {
	const uint32_t sizes[] = {0, 1, 2, 63, 64, 85, 86, 128, 255, 256, 257, 700, 4097, 9000, 21846};
	const uint32_t verts[] = {3, 40, 255, 256, 257, 1000, 70000};
	uint32_t runs = 0;
	for(uint32_t nface : sizes) for(uint32_t nvert : verts) for(int kind = 0; kind < 4; kind++) {
		if(nface > 1000 && (runs % 3)) { runs++; continue; }                     // (keep the run short)
		if(kind == 2 && nface > 700) { runs++; continue; }                       // (a fan's list is quadratic)
		const bool u16 = (runs & 1) && kind != 3 && nvert + nvert/8 + 1 < 65536;
		one(nface, nvert, kind, u16, runs); runs++;
	}
	if(failures) { printf("adjacency_check: %d failures\n", failures); return 1; }
	printf("adjacency_check ok (%u runs)\n", runs);
	return 0;
}
