// compact_check.cpp — both partitions of csrc/compact.h and its gather on the host under AddressSanitizer and UBSan
// (tests/test_compact_sanitize_cpu.py): a stand-alone program, host code only.  newid, order, index, the gathered array and the record are heap
// blocks of their own: newid ENDS exactly at nvert words, order at vertex_capacity words, index at index_capacity words, the gathered array at
// its last gathered byte ((capacity - 1)*stride + E: a strided destination has no tail behind its last element) and the record is a block of
// exactly 16 bytes.  The capacities are `used` and 3*F in one run - CAPACITIES EQUAL TO WHAT IS WRITTEN - and used - 1, 3*F - 1 and 0 in others,
// so a store one byte past what the contract allows is reported.  (The hook's own scratch - the mask, the word-popcount scan, the block counts, a
// set's own order and newid - is made at exactly the kernels' sizes: a step past the mask's end is reported too.)  The source array ends at its
// last byte as well.  The two partitions must leave the bytes a sequential pass leaves, under every seed.  Built with csrc/compact_host.cpp,
// whose one dependency on the library (ctx_fail) is defined here.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/corto_hip.h"
#include "compact.h"

using namespace corto_hip;

namespace corto_hip {
int ctx_fail(int code, const char *) { return code; }
}

static int failures = 0;
#define CHECK(cond, ...) do { if(!(cond)) { failures++; printf("FAILED %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } while(0)

static bool same(const void *a, const void *b, size_t n) { return n == 0 || memcmp(a, b, n) == 0; }   // (an empty vector's data() may be null)

static uint64_t rng_state;
static uint64_t rng() { rng_state = rng_state*6364136223846793005ull + 1442695040888963407ull; return rng_state >> 16; }

// a block that ENDS at its last byte (aligned_alloc rounds a block to 16 bytes): the bytes, and the block to free
static uint8_t *ending_block(size_t sz, uint8_t **blk) {
	const size_t cap = sz ? (sz + 15)/16*16 : 16;
	*blk = (uint8_t *)aligned_alloc(16, cap);
	memset(*blk, 0xCD, cap);
	return *blk + (cap - sz);
}

// kind 0: every vertex; 1: every third vertex, in no order; 2: with ids >= nvert among them; 3: nothing (F = 0)
static void one(uint32_t nvert, uint32_t nface, int kind, uint32_t E, uint32_t sstride, uint32_t dstride, uint32_t seed) {
	rng_state = 0x9E3779B97F4A7C15ull ^ ((uint64_t)nvert*7u + nface*131u + seed);
	if(kind == 3) nface = 0;
	uint8_t *sblk, *ablk;
	uint32_t *src = (uint32_t *)ending_block((size_t)nface*12, &sblk);
	for(size_t k = 0; k < (size_t)nface*3; k++) {
		src[k] = kind == 0 ? (uint32_t)(k % nvert) : kind == 1 ? (uint32_t)(rng() % ((nvert + 2)/3))*3 : (uint32_t)(rng() % (2*(uint64_t)nvert));
		if(kind == 2 && k % 11 == 0) src[k] = 0xFFFFFFFFu;
		if(src[k] >= nvert && kind != 2) src[k] = nvert - 1;
	}
	const uint32_t S = sstride ? sstride : E, D = dstride ? dstride : E;
	uint8_t *attr = ending_block((size_t)(nvert - 1)*S + E, &ablk);
	for(size_t e = 0; e < (size_t)(nvert - 1)*S + E; e++) attr[e] = (uint8_t)rng();
	// the sequential pass
	std::vector<uint8_t> used(nvert, 0);
	for(size_t k = 0; k < (size_t)nface*3; k++) if(src[k] < nvert) used[src[k]] = 1;
	std::vector<uint32_t> ref_newid(nvert, 0xFFFFFFFFu), ref_order, ref_index((size_t)nface*3, 0xFFFFFFFFu);
	for(uint32_t v = 0; v < nvert; v++) if(used[v]) { ref_newid[v] = (uint32_t)ref_order.size(); ref_order.push_back(v); }
	for(size_t k = 0; k < (size_t)nface*3; k++) if(src[k] < nvert) ref_index[k] = ref_newid[src[k]];
	const uint32_t nused = (uint32_t)ref_order.size();
	const uint32_t vcaps[] = {nused, nused ? nused - 1 : 0, 0, nused + 1}, icaps[] = {nface*3, nface ? nface*3 - 1 : 0, 0, nface*3 + 1};
	for(int which = 0; which < 2; which++) for(uint32_t c = 0; c < 4; c++) {
		if(which == 0 && !compact_in_blob(nvert, nface)) continue;
		const uint32_t vcap = vcaps[c], icap = icaps[c];
		uint8_t *nblk, *oblk, *iblk, *dblk;
		uint32_t *newid = (uint32_t *)ending_block((size_t)nvert*4, &nblk), *order = (uint32_t *)ending_block((size_t)vcap*4, &oblk);
		uint32_t *index = (uint32_t *)ending_block((size_t)icap*4, &iblk);
		const size_t dbytes = vcap ? (size_t)(vcap - 1)*D + E : 0;
		uint8_t *dst = ending_block(dbytes, &dblk);
		crthip_compact_counts *rec = (crthip_compact_counts *)aligned_alloc(16, 16);
		memset(rec, 0xCD, 16);
		// (unit 16 needs 16-byte addresses: a block that ends at its last byte has them where its size is a multiple of 16)
		const crthip_compact_model_gather g{attr, dst, E, sstride, dstride, 0};
		const bool with_order = (seed + c) % 3 != 0;                               // (without: the hook keeps an order of its own for the gather)
		const int rc = crthip_compact_model(src, 0, nface, nface, nvert, newid, with_order ? order : nullptr, index, vcap, icap, rec, &g, 1, which, seed + c);
		CHECK(rc == 0, "rc %d nvert %u nface %u which %d", rc, nvert, nface, which);
		const uint32_t clipped = nused > vcap || (uint64_t)nface*3 > icap;
		CHECK(rec->vertices == nvert && rec->used == nused && rec->faces == nface && rec->clipped == clipped, "record %u %u %u %u nvert %u nface %u which %d cap %u",
			rec->vertices, rec->used, rec->faces, rec->clipped, nvert, nface, which, c);
		CHECK(same(newid, ref_newid.data(), (size_t)nvert*4), "newid differs nvert %u nface %u which %d", nvert, nface, which);
		const uint32_t nord = nused < vcap ? nused : vcap;
		const size_t nidx = (size_t)nface*3 < icap ? (size_t)nface*3 : icap;
		if(with_order) {
			CHECK(same(order, ref_order.data(), (size_t)nord*4), "order differs nvert %u nface %u which %d", nvert, nface, which);
			for(size_t j = nord; j < vcap; j++) if(order[j] != 0xCDCDCDCDu) { CHECK(false, "written behind order nvert %u", nvert); break; }
		} else for(size_t j = 0; j < vcap; j++) if(order[j] != 0xCDCDCDCDu) { CHECK(false, "order written without an order array nvert %u", nvert); break; }
		CHECK(same(index, ref_index.data(), nidx*4), "index differs nvert %u nface %u which %d", nvert, nface, which);
		for(size_t k = nidx; k < icap; k++) if(index[k] != 0xCDCDCDCDu) { CHECK(false, "written behind index nvert %u", nvert); break; }
		for(size_t j = 0; j < vcap; j++) {
			bool ok = true;
			for(uint32_t e = 0; e < D && j*D + e < dbytes; e++) {
				const uint8_t want = j < nord && e < E ? attr[(size_t)ref_order[j]*S + e] : 0xCD;
				if(dst[j*D + e] != want) ok = false;
			}
			if(!ok) { CHECK(false, "gathered record %zu differs nvert %u E %u strides %u %u which %d", j, nvert, E, S, D, which); break; }
		}
		for(uint8_t *p = nblk; p < (uint8_t *)newid; p++) if(*p != 0xCD) { CHECK(false, "written in front of newid nvert %u", nvert); break; }
		for(uint8_t *p = oblk; p < (uint8_t *)order; p++) if(*p != 0xCD) { CHECK(false, "written in front of order nvert %u", nvert); break; }
		for(uint8_t *p = iblk; p < (uint8_t *)index; p++) if(*p != 0xCD) { CHECK(false, "written in front of index nvert %u", nvert); break; }
		for(uint8_t *p = dblk; p < dst; p++) if(*p != 0xCD) { CHECK(false, "written in front of the gathered array nvert %u", nvert); break; }
		free(nblk); free(oblk); free(iblk); free(dblk); free(rec);
	}
	free(sblk); free(ablk);
}

// a cloud set: the level's points end at `cells` words, the record is the hook's
static void cloud(uint32_t nvert, uint32_t cells, uint32_t vcap) {
	uint8_t *pblk, *ablk, *dblk;
	uint32_t *points = (uint32_t *)ending_block((size_t)cells*4, &pblk);
	for(uint32_t j = 0; j < cells; j++) points[j] = (uint32_t)((uint64_t)j*nvert/cells);
	uint8_t *attr = ending_block((size_t)nvert*12, &ablk);
	for(size_t e = 0; e < (size_t)nvert*12; e++) attr[e] = (uint8_t)(e*7);
	const uint32_t n = cells < vcap ? cells : vcap;
	uint8_t *dst = ending_block((size_t)vcap*12, &dblk);
	crthip_compact_counts *rec = (crthip_compact_counts *)aligned_alloc(16, 16);
	const crthip_compact_model_gather g{attr, dst, 12, 0, 0, 0};
	const int rc = crthip_compact_model(points, 0, cells, cells, nvert, nullptr, nullptr, nullptr, vcap, 0, rec, &g, 1, 2, cells);
	CHECK(rc == 0 && rec->vertices == nvert && rec->used == cells && rec->faces == 0 && rec->clipped == (cells > vcap), "cloud rc %d nvert %u cells %u", rc, nvert, cells);
	for(uint32_t j = 0; j < n; j++) if(memcmp(dst + (size_t)j*12, attr + (size_t)points[j]*12, 12)) { CHECK(false, "cloud record %u differs", j); break; }
	for(size_t e = (size_t)n*12; e < (size_t)vcap*12; e++) if(dst[e] != 0xCD) { CHECK(false, "written behind the cloud's records"); break; }
	free(pblk); free(ablk); free(dblk); free(rec);
}

int main() {
	const uint32_t verts[] = {1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1000, 8192, 8193, 65537};
	const uint32_t Es[][3] = {{12, 0, 0}, {3, 0, 0}, {16, 0, 0}, {16, 32, 48}, {6, 8, 0}, {8, 0, 12}, {4, 4, 20}, {12, 16, 12}};
	uint32_t runs = 0;
	for(uint32_t nvert : verts) for(int kind = 0; kind < 4; kind++) {
		if(nvert > 8193 && kind > 1) { runs++; continue; }                          // (keep the run short)
		const uint32_t *e = Es[runs % 8];
		one(nvert, nvert > 8192 ? 9000 : nvert < 100 ? nvert + 5 : nvert/2, kind, e[0], e[1], e[2], runs); runs++;
	}
	one(100, 8193, 1, 12, 0, 0, 99); runs++;                                       // (the bound faces alone put a set beyond compact_blob)
	cloud(300, 100, 100); cloud(300, 100, 99); cloud(300, 100, 0); cloud(300, 300, 301); cloud(8193, 1, 1); runs += 5;
	if(failures) { printf("compact_check: %d failures\n", failures); return 1; }
	printf("compact_check ok (%u runs)\n", runs);
	return 0;
}
