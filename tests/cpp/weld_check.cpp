// weld_check.cpp — both partitions of csrc/weld.h on the host under AddressSanitizer and UBSan (tests/test_weld_sanitize_cpu.py): a stand-alone
// program, host code only.  The positions, the index, remap, the welded index and the record are heap blocks of their own: remap ENDS exactly
// at nvert words, the welded index at 3*nface words and the record is a block of exactly 16 bytes, so a store one byte past what the contract
// allows is reported.  (The hook's own table is a vector of exactly T words, the positions a block of exactly 3*nvert: a walk past the table, or
// an id >= nvert used as an address, is reported too.)  The positions are drawn from few values, so that many vertices coincide; the indices
// hold ids at and beyond nvert.  The two partitions must leave the same bytes under every seed.  Built with csrc/weld_host.cpp, whose one
// dependency on the library (ctx_fail) is defined here.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/corto_hip.h"
#include "weld.h"

using namespace corto_hip;

namespace corto_hip { int ctx_fail(int code, const char *) { return code; } }

static int failures = 0;
#define CHECK(cond, ...) do { if(!(cond)) { failures++; printf("FAILED %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } while(0)

static uint64_t rng_state;
static uint64_t rng() { rng_state = rng_state*6364136223846793005ull + 1442695040888963407ull; return rng_state >> 16; }

// a block that ENDS at its last word (aligned_alloc rounds a block to 16 bytes): the words, and the block to free
static uint32_t *ending_block(size_t words, uint8_t **blk) {
	const size_t sz = words*4, cap = sz ? (sz + 15)/16*16 : 16;
	*blk = (uint8_t *)aligned_alloc(16, cap);
	memset(*blk, 0xCD, cap);
	return (uint32_t *)(*blk + (cap - sz));
}

static void one(uint32_t nvert, uint32_t nface, int kind, bool u16, bool with_index, uint32_t seed) {
	rng_state = 0x9E3779B97F4A7C15ull ^ ((uint64_t)nface*131u + nvert*7u + seed);
	int32_t *pos = (int32_t *)malloc(nvert ? (size_t)nvert*12 : 1);
	for(size_t e = 0; e < (size_t)nvert*3; e++) {
		if(kind == 0) pos[e] = (int32_t)(rng() % 5) - 2;                            // 125 rows: heavy coincidence
		else if(kind == 1) pos[e] = (int32_t)(e/3 % 97)*(e%3 == 0) + (int32_t)(e/3/97)*(e%3 == 1);   // a lattice, every vertex its own row
		else if(kind == 2) pos[e] = 7;                                              // one point
		else pos[e] = rng() % 2 ? (int32_t)0x80000000 + (int32_t)(rng() % 3) : 0x7FFFFFFF - (int32_t)(rng() % 3);   // the ends of int32
	}
	void *faces = malloc(nface ? (size_t)nface*3*(u16 ? 2 : 4) : 1);
	for(size_t e = 0; e < (size_t)nface*3; e++) {
		uint32_t v = rng() % 7 ? (uint32_t)(rng() % (nvert + nvert/8 + 1)) : 0xFFFFFFFFu - (uint32_t)(rng() % 5);   // ids at and beyond nvert
		if(u16) ((uint16_t *)faces)[e] = (uint16_t)v; else ((uint32_t *)faces)[e] = v;
	}
	const size_t cwords = (size_t)nface*3;
	std::vector<uint32_t> ref_remap, ref_index; crthip_weld_counts refc{}; bool have = false;
	for(int which = 0; which < 2; which++) for(uint32_t s = 0; s < 3; s++) {
		if(which == 0 && !weld_in_blob(nvert)) continue;
		uint8_t *rblk, *iblk;
		uint32_t *remap = ending_block(nvert, &rblk), *windex = ending_block(cwords, &iblk);
		crthip_weld_counts *rec = (crthip_weld_counts *)aligned_alloc(16, 16);
		memset(rec, 0xCD, 16);
		uint64_t stats[2] = {0, 0};
		const int rc = crthip_weld_model(nvert ? pos : nullptr, nface ? faces : nullptr, u16, nface, nvert, nvert ? remap : nullptr,
			with_index && nface ? windex : nullptr, rec, stats, which, seed + s);
		CHECK(rc == 0, "rc %d nvert %u nface %u which %d", rc, nvert, nface, which);
		CHECK(rec->vertices == nvert && rec->unique <= nvert && (nvert == 0 || rec->unique >= 1) && rec->degenerate <= nface && rec->reserved == 0,
			"counts nvert %u which %d", nvert, which);
		CHECK(stats[0] >= nvert && stats[1] <= weld_slots(nvert), "stats nvert %u which %d", nvert, which);
		for(size_t v = 0; v < nvert; v++) if(remap[v] > v || remap[remap[v]] != remap[v] || memcmp(pos + 3*remap[v], pos + 3*v, 12)) { CHECK(false, "remap[%zu] = %u nvert %u", v, remap[v], nvert); break; }
		if(!have) { have = true; refc = *rec; ref_remap.assign(remap, remap + nvert); ref_index.assign(windex, windex + cwords); }
		else {
			CHECK(memcmp(rec, &refc, sizeof refc) == 0, "counts differ nvert %u which %d seed %u", nvert, which, seed + s);
			CHECK(nvert == 0 || memcmp(ref_remap.data(), remap, (size_t)nvert*4) == 0, "remap differs: nvert %u which %d seed %u", nvert, which, seed + s);
			CHECK(cwords == 0 || memcmp(ref_index.data(), windex, cwords*4) == 0, "index differs: nvert %u which %d seed %u", nvert, which, seed + s);
		}
		for(uint8_t *p = rblk; p < (uint8_t *)remap; p++) if(*p != 0xCD) { CHECK(false, "written in front of remap nvert %u", nvert); break; }
		for(uint8_t *p = iblk; p < (uint8_t *)windex; p++) if(*p != 0xCD) { CHECK(false, "written in front of index nface %u", nface); break; }
		if(!with_index) for(size_t k = 0; k < cwords; k++) if(windex[k] != 0xCDCDCDCDu) { CHECK(false, "an index nobody asked for nface %u", nface); break; }
		free(rblk); free(iblk); free(rec);
	}
	free(pos); free(faces);
}

int main() {
	const uint32_t verts[] = {0, 1, 3, 31, 32, 33, 255, 256, 257, 512, 513, 1000, 8191, 8192, 8193, 20000};
	const uint32_t faces[] = {0, 1, 85, 86, 700, 9000};
	uint32_t runs = 0;
	for(uint32_t nvert : verts) for(uint32_t nface : faces) for(int kind = 0; kind < 4; kind++) {
		if((nvert > 1000 || nface > 700) && (runs % 3)) { runs++; continue; }       // (keep the run short)
		const bool u16 = (runs & 1) && nvert + nvert/8 + 1 < 65536;
		one(nvert, nface, kind, u16, runs % 5 != 0, runs); runs++;
	}
	if(failures) { printf("weld_check: %d failures\n", failures); return 1; }
	printf("weld_check ok (%u runs)\n", runs);
	return 0;
}
