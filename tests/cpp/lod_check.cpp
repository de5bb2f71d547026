// lod_check.cpp — both partitions of csrc/lod.h on the host under AddressSanitizer and UBSan (tests/test_lod_sanitize_cpu.py): a stand-alone
// program, host code only.  The positions, the index, remap, the level's index and the record are heap blocks of their own: remap ENDS exactly at
// nvert words; the level's index ends at 3*nface words in the first run, which tells the kept count, and at exactly 3*faces words - a CAPACITY
// EQUAL TO THE KEPT COUNT - in every run behind it (through corto_hip::lod_model, behind the hook's capacity check); the record is a block of
// exactly 16 bytes.  So a store one byte past what the contract allows is reported.  (The hook's own scratch - the triples, the two tables, the
// block counts - are vectors of exactly the kernels' sizes, the positions a block of exactly 3*nvert: a walk past a table, or an id >= nvert used
// as an address, is reported too.)  The positions are drawn so that many vertices share a cell; the indices hold ids at and beyond nvert.  The
// two partitions must leave the same bytes under every seed.  Built with csrc/lod_host.cpp, whose one dependency on the library (ctx_fail) is
// defined here.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/corto_hip.h"
#include "lod.h"

using namespace corto_hip;

namespace corto_hip {
int ctx_fail(int code, const char *) { return code; }
void lod_model(const LodIn &J, uint32_t *remap, uint32_t *index, crthip_lod_counts *rec, LodStats *stats, int which, uint32_t seed);
}

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

static void one(uint32_t nvert, uint32_t nface, int kind, bool u16, uint32_t shift, uint32_t seed) {
	rng_state = 0x9E3779B97F4A7C15ull ^ ((uint64_t)nface*131u + nvert*7u + seed);
	int32_t *pos = (int32_t *)malloc(nvert ? (size_t)nvert*12 : 1);
	for(size_t e = 0; e < (size_t)nvert*3; e++) {
		if(kind == 0) pos[e] = (int32_t)(rng() % 41) - 20;                          // few cells at any shift: heavy clustering
		else if(kind == 1) pos[e] = (int32_t)(e/3 % 97)*(e%3 == 0) + (int32_t)(e/3/97)*(e%3 == 1);   // a lattice
		else if(kind == 2) pos[e] = -1 + (int32_t)(rng() % 2);                      // -1 and 0: never one cell
		else pos[e] = rng() % 2 ? (int32_t)0x80000000 + (int32_t)(rng() % 3) : 0x7FFFFFFF - (int32_t)(rng() % 3);   // the ends of int32
	}
	void *faces = malloc(nface ? (size_t)nface*3*(u16 ? 2 : 4) : 1);
	for(size_t e = 0; e < (size_t)nface*3; e++) {
		uint32_t v = rng() % 9 ? (uint32_t)(rng() % (nvert + nvert/8 + 1)) : 0xFFFFFFFFu - (uint32_t)(rng() % 5);   // ids at and beyond nvert
		if(u16) ((uint16_t *)faces)[e] = (uint16_t)v; else ((uint32_t *)faces)[e] = v;
	}
	LodIn J; J.w.position = pos; J.w.index = faces; J.w.index_u16 = u16; J.w.nface = nface; J.w.nvert = nvert; J.shift = shift;
	std::vector<uint32_t> ref_remap, ref_index; crthip_lod_counts refc{}; bool have = false;
	for(int which = 0; which < 2; which++) for(uint32_t s = 0; s < 3; s++) {
		if(which == 0 && !lod_in_blob(nvert, nface)) continue;
		// the first run of all: through the hook, 3*nface words; then the index ends at the kept count
		const size_t iwords = have ? (size_t)refc.faces*3 : (size_t)nface*3;
		uint8_t *rblk, *iblk;
		uint32_t *remap = ending_block(nvert, &rblk), *lindex = ending_block(iwords, &iblk);
		crthip_lod_counts *rec = (crthip_lod_counts *)aligned_alloc(16, 16);
		memset(rec, 0xCD, 16);
		uint64_t stats[4] = {0, 0, 0, 0};
		if(!have) {
			const int rc = crthip_lod_model(nvert ? pos : nullptr, nface ? faces : nullptr, u16, nface, nvert, shift, nvert ? remap : nullptr,
				nface ? lindex : nullptr, rec, stats, which, seed + s);
			CHECK(rc == 0, "rc %d nvert %u nface %u which %d", rc, nvert, nface, which);
			CHECK(stats[0] >= nvert && stats[1] <= weld_slots(nvert) && stats[3] <= weld_slots(nface), "stats nvert %u which %d", nvert, which);
		} else {
			LodStats st{0, 0, 0, 0};
			lod_model(J, remap, lindex, rec, &st, which, seed + s);
		}
		CHECK(rec->cells <= nvert && (nvert == 0 || rec->cells >= 1) && (uint64_t)rec->faces + rec->degenerate + rec->duplicate == nface,
			"counts nvert %u nface %u which %d", nvert, nface, which);
		for(size_t v = 0; v < nvert; v++) if(remap[v] > v || remap[remap[v]] != remap[v]) { CHECK(false, "remap[%zu] = %u nvert %u", v, remap[v], nvert); break; }
		if(!have) {
			have = true; refc = *rec; ref_remap.assign(remap, remap + nvert); ref_index.assign(lindex, lindex + (size_t)rec->faces*3);
			for(size_t k = (size_t)rec->faces*3; k < iwords; k++) if(lindex[k] != 0xCDCDCDCDu) { CHECK(false, "written behind the kept faces nface %u", nface); break; }
		} else {
			CHECK(memcmp(rec, &refc, sizeof refc) == 0, "counts differ nvert %u nface %u which %d seed %u", nvert, nface, which, seed + s);
			CHECK(nvert == 0 || memcmp(ref_remap.data(), remap, (size_t)nvert*4) == 0, "remap differs: nvert %u which %d seed %u", nvert, which, seed + s);
			CHECK(iwords == 0 || memcmp(ref_index.data(), lindex, iwords*4) == 0, "index differs: nvert %u nface %u which %d seed %u", nvert, nface, which, seed + s);
		}
		for(size_t k = 0; k < (size_t)refc.faces*3 && k < iwords; k++) if(lindex[k] >= nvert) { CHECK(false, "an index word that is no vertex nface %u", nface); break; }
		for(uint8_t *p = rblk; p < (uint8_t *)remap; p++) if(*p != 0xCD) { CHECK(false, "written in front of remap nvert %u", nvert); break; }
		for(uint8_t *p = iblk; p < (uint8_t *)lindex; p++) if(*p != 0xCD) { CHECK(false, "written in front of index nface %u", nface); break; }
		free(rblk); free(iblk); free(rec);
	}
	free(pos); free(faces);
}

int main() {
	const uint32_t verts[] = {0, 1, 3, 63, 64, 65, 255, 256, 257, 513, 1000, 8192, 8193, 20000};
	const uint32_t faces[] = {0, 1, 255, 256, 257, 700, 8192, 8193};
	const uint32_t shifts[] = {0, 1, 3, 31};
	uint32_t runs = 0;
	for(uint32_t nvert : verts) for(uint32_t nface : faces) for(int kind = 0; kind < 4; kind++) {
		if((nvert > 1000 || nface > 700) && (runs % 3)) { runs++; continue; }       // (keep the run short)
		const bool u16 = (runs & 1) && nvert + nvert/8 + 1 < 65536;
		one(nvert, nface, kind, u16, shifts[runs % 4], runs); runs++;
	}
	if(failures) { printf("lod_check: %d failures\n", failures); return 1; }
	printf("lod_check ok (%u runs)\n", runs);
	return 0;
}
