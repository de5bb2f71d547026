// cloud_lod_check.cpp — both partitions of csrc/cloud_lod.h on the host under AddressSanitizer and UBSan (tests/test_cloud_lod_sanitize_cpu.py): a
// stand-alone program, host code only.  The positions, remap, points, weight, the chunk records and the record are heap blocks of their own:
// remap ENDS exactly at nvert words; points, weight and chunks end at nvert words and ceil(nvert / K) records in the first run, which tells the
// counts, and at exactly `cells` words and ceil(cells / K) records - CAPACITIES EQUAL TO WHAT IS WRITTEN - in every run behind it (through
// corto_hip::cloud_lod_model, behind the hook's capacity check); the record is a block of exactly 16 bytes.  So a store one byte past what the
// contract allows is reported.  (The hook's own scratch - the table, the weight words, the block counts, the six words of a chunk's box - is made
// at exactly the kernels' sizes, the positions a block of exactly 3*nvert words: a walk past the table's end, a weight word or a box past the
// table's words, is reported too.)  The positions are drawn so that many points share a cell.  The two partitions must leave the same bytes under
// every seed.  Built with csrc/cloud_lod_host.cpp, whose one dependency on the library (ctx_fail) is defined here.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/corto_hip.h"
#include "cloud_lod.h"

using namespace corto_hip;

namespace corto_hip {
int ctx_fail(int code, const char *) { return code; }
void cloud_lod_model(const LodIn &J, uint32_t K, uint32_t *remap, uint32_t *points, uint32_t *weight, crthip_cloud_chunk *chunks, crthip_cloud_lod_counts *rec,
	LodStats *stats, int which, uint32_t seed);
}

static int failures = 0;
#define CHECK(cond, ...) do { if(!(cond)) { failures++; printf("FAILED %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } while(0)

static uint64_t rng_state;
static uint64_t rng() { rng_state = rng_state*6364136223846793005ull + 1442695040888963407ull; return rng_state >> 16; }

// a block that ENDS at its last byte (aligned_alloc rounds a block to 16 bytes): the bytes, and the block to free
static uint8_t *ending_block(size_t sz, uint8_t **blk) {
	const size_t cap = sz ? (sz + 15)/16*16 : 16;
	*blk = (uint8_t *)aligned_alloc(16, cap);
	memset(*blk, 0xCD, cap);
	return *blk + (cap - sz);
}

static void one(uint32_t nvert, int kind, uint32_t shift, uint32_t K, bool weights, uint32_t seed) {
	rng_state = 0x9E3779B97F4A7C15ull ^ ((uint64_t)nvert*7u + K*131u + seed);
	int32_t *pos = (int32_t *)malloc((size_t)nvert*12);
	for(size_t e = 0; e < (size_t)nvert*3; e++) {
		if(kind == 0) pos[e] = (int32_t)(rng() % 41) - 20;                          // few cells at any shift: heavy clustering
		else if(kind == 1) pos[e] = (int32_t)(e/3 % 97)*(e%3 == 0) + (int32_t)(e/3/97)*(e%3 == 1);   // a lattice: every point its own cell at shift 0
		else if(kind == 2) pos[e] = -1 + (int32_t)(rng() % 2);                      // -1 and 0: never one cell
		else pos[e] = rng() % 2 ? (int32_t)0x80000000 + (int32_t)(rng() % 3) : 0x7FFFFFFF - (int32_t)(rng() % 3);   // the ends of int32
	}
	LodIn J; J.w.position = pos; J.w.index = nullptr; J.w.index_u16 = 0; J.w.nface = 0; J.w.nvert = nvert; J.shift = shift;
	std::vector<uint32_t> ref_remap, ref_points, ref_weight; std::vector<uint8_t> ref_chunks; crthip_cloud_lod_counts refc{}; bool have = false;
	for(int which = 0; which < 2; which++) for(uint32_t s = 0; s < 3; s++) {
		if(which == 0 && !weld_in_blob(nvert)) continue;
		// the first run of all: through the hook, at the capacities; then every array ends at what is written
		const size_t pwords = have ? refc.cells : nvert, crecs = K ? (have ? refc.chunks : cloud_lod_chunks_of(nvert, K)) : 0;
		uint8_t *rblk, *pblk, *wblk, *cblk;
		uint32_t *remap = (uint32_t *)ending_block((size_t)nvert*4, &rblk), *points = (uint32_t *)ending_block(pwords*4, &pblk);
		uint32_t *weight = (uint32_t *)ending_block(pwords*4, &wblk);
		// (chunk records are 16-byte aligned and 32 bytes each: the block ends at the last one as it is)
		crthip_cloud_chunk *chunks = (crthip_cloud_chunk *)ending_block(crecs*32, &cblk);
		crthip_cloud_lod_counts *rec = (crthip_cloud_lod_counts *)aligned_alloc(16, 16);
		memset(rec, 0xCD, 16);
		if(!have) {
			uint64_t stats[2] = {0, 0};
			const int rc = crthip_cloud_lod_model(pos, nvert, shift, K, remap, points, weights ? weight : nullptr, K ? chunks : nullptr, rec, stats, which, seed + s);
			CHECK(rc == 0, "rc %d nvert %u which %d", rc, nvert, which);
			CHECK(stats[0] >= nvert && stats[1] <= weld_slots(nvert), "stats nvert %u which %d", nvert, which);
		} else {
			LodStats st{0, 0, 0, 0};
			cloud_lod_model(J, K, remap, points, weights ? weight : nullptr, K ? chunks : nullptr, rec, &st, which, seed + s);
		}
		CHECK(rec->points == nvert && rec->cells >= 1 && rec->cells <= nvert && rec->chunks == cloud_lod_chunks_of(rec->cells, K) && rec->reserved == 0,
			"counts nvert %u K %u which %d", nvert, K, which);
		for(size_t v = 0; v < nvert; v++) if(remap[v] > v || remap[remap[v]] != remap[v]) { CHECK(false, "remap[%zu] = %u nvert %u", v, remap[v], nvert); break; }
		uint64_t sum = 0;
		for(size_t j = 0; j < rec->cells && j < pwords; j++) {
			if(points[j] >= nvert || remap[points[j]] != points[j] || (j && points[j] <= points[j - 1])) { CHECK(false, "points[%zu] = %u nvert %u", j, points[j], nvert); break; }
			sum += weights ? weight[j] : 0;
		}
		CHECK(!weights || sum == nvert, "the weights sum to %llu, nvert %u which %d", (unsigned long long)sum, nvert, which);
		if(!have) {
			have = true; refc = *rec; ref_remap.assign(remap, remap + nvert); ref_points.assign(points, points + rec->cells);
			if(weights) ref_weight.assign(weight, weight + rec->cells);
			ref_chunks.assign((uint8_t *)chunks, (uint8_t *)chunks + (size_t)rec->chunks*32);
			for(size_t j = rec->cells; j < pwords; j++) if(points[j] != 0xCDCDCDCDu || weight[j] != 0xCDCDCDCDu) { CHECK(false, "written behind the kept points nvert %u", nvert); break; }
			for(const uint8_t *p = (const uint8_t *)(chunks + rec->chunks); p < (const uint8_t *)(chunks + crecs); p++) if(*p != 0xCD) { CHECK(false, "written behind the chunks nvert %u", nvert); break; }
		} else {
			CHECK(memcmp(rec, &refc, sizeof refc) == 0, "counts differ nvert %u which %d seed %u", nvert, which, seed + s);
			CHECK(memcmp(ref_remap.data(), remap, (size_t)nvert*4) == 0, "remap differs: nvert %u which %d seed %u", nvert, which, seed + s);
			CHECK(memcmp(ref_points.data(), points, pwords*4) == 0, "points differ: nvert %u which %d seed %u", nvert, which, seed + s);
			CHECK(!weights || memcmp(ref_weight.data(), weight, pwords*4) == 0, "weights differ: nvert %u which %d seed %u", nvert, which, seed + s);
			CHECK(crecs == 0 || memcmp(ref_chunks.data(), chunks, crecs*32) == 0, "chunks differ: nvert %u K %u which %d seed %u", nvert, K, which, seed + s);
		}
		if(!weights) for(size_t j = 0; j < pwords; j++) if(weight[j] != 0xCDCDCDCDu) { CHECK(false, "weights written without a weight array nvert %u", nvert); break; }
		for(uint8_t *p = rblk; p < (uint8_t *)remap; p++) if(*p != 0xCD) { CHECK(false, "written in front of remap nvert %u", nvert); break; }
		for(uint8_t *p = pblk; p < (uint8_t *)points; p++) if(*p != 0xCD) { CHECK(false, "written in front of points nvert %u", nvert); break; }
		for(uint8_t *p = wblk; p < (uint8_t *)weight; p++) if(*p != 0xCD) { CHECK(false, "written in front of weight nvert %u", nvert); break; }
		free(rblk); free(pblk); free(wblk); free(cblk); free(rec);
	}
	free(pos);
}

int main() {
	const uint32_t verts[] = {1, 2, 3, 31, 32, 33, 63, 64, 65, 255, 256, 257, 513, 1000, 8192, 8193, 20000, 66049};
	const uint32_t shifts[] = {0, 1, 3, 31};
	const uint32_t Ks[] = {32, 0, 33, 65536, 100};
	uint32_t runs = 0;
	for(uint32_t nvert : verts) for(int kind = 0; kind < 4; kind++) {
		if(nvert > 8193 && kind > 1) { runs++; continue; }                          // (keep the run short)
		one(nvert, kind, shifts[runs % 4], Ks[runs % 5], runs % 3 != 2, runs); runs++;
	}
	if(failures) { printf("cloud_lod_check: %d failures\n", failures); return 1; }
	printf("cloud_lod_check ok (%u runs)\n", runs);
	return 0;
}
