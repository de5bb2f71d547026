// quant_out_check.cpp — the two partitions of csrc/quant_out.h on the host under AddressSanitizer and UBSan
// (tests/test_quantized_outputs_sanitize_cpu.py): a stand-alone program, host code only.  Every source and destination is a heap block of
// its own that ENDS exactly with the last value / the last vertex's halfwords, and the destination starts at each 2-byte offset of a
// 16-byte line in turn, so a read or a store one byte too far, or a vector store off its boundary, is reported.  The results are held
// against a plain loop.  Built with csrc/quant_out_host.cpp, whose one dependency on the library (ctx_fail) is defined here.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "quant_out.h"

using namespace corto_hip;

namespace corto_hip { int ctx_fail(int code, const char *) { return code; } }

static int failures = 0;
#define CHECK(cond, ...) do { if(!(cond)) { failures++; printf("FAILED %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } while(0)

static void one(uint32_t nvert, uint32_t N, uint32_t stride, uint32_t misalign, int which, uint32_t seed, int32_t lo, int64_t width) {
	const size_t nval = (size_t)nvert*N;
	int32_t *values = (int32_t *)malloc(nval ? nval*4 : 1);
	uint64_t x = 0x9E3779B97F4A7C15ull ^ (nvert*131u + N*7u + seed);
	for(size_t e = 0; e < nval; e++) {
		x = x*6364136223846793005ull + 1442695040888963407ull;
		values[e] = (int32_t)((int64_t)lo + (int64_t)((x >> 20) % (uint64_t)width));
	}
	if(nval) { values[0] = lo; values[nval - 1] = (int32_t)((int64_t)lo + width - 1); }   // (the span is exactly width - 1 where the two share a component)
	const uint32_t st = stride ? stride : 2*N;
	const size_t bytes = nvert ? (size_t)(nvert - 1)*st + 2*N : 0;
	// the block ends with the last halfword; its start is `misalign` bytes behind a 16-byte boundary (malloc gives one)
	uint8_t *block = (uint8_t *)malloc(bytes + misalign ? bytes + misalign : 1);
	uint8_t *out = block + misalign;
	memset(block, 0xA5, bytes + misalign);
	crthip_quant_transform t{};
	t.q = 0.25f;
	const int rc = crthip_quant_out_model(values, nvert, N, stride, out, &t, which, seed);
	CHECK(rc == 0, "rc %d nvert %u N %u", rc, nvert, N);
	// a plain loop
	int64_t mn[4] = {0, 0, 0, 0}, mx[4] = {0, 0, 0, 0};
	for(uint32_t c = 0; c < N && nvert; c++) { mn[c] = mx[c] = values[c]; }
	for(size_t v = 0; v < nvert; v++) for(uint32_t c = 0; c < N; c++) { const int64_t a = values[v*N + c]; if(a < mn[c]) mn[c] = a; if(a > mx[c]) mx[c] = a; }
	uint32_t written = 1;
	for(uint32_t c = 0; c < N; c++) if(mx[c] - mn[c] > 65535) written = 0;
	CHECK(t.written == written && (nvert == 0 || t.components == N), "written %u/%u nvert %u N %u which %d", t.written, written, nvert, N, which);
	for(uint32_t c = 0; c < N && nvert; c++) CHECK(t.base[c] == mn[c] && t.span[c] == (uint64_t)(mx[c] - mn[c]), "record c %u nvert %u N %u which %d", c, nvert, N, which);
	std::vector<uint8_t> want(bytes + misalign, 0xA5);
	if(written) for(size_t v = 0; v < nvert; v++) for(uint32_t c = 0; c < N; c++) {
		const uint16_t h = (uint16_t)(values[v*N + c] - mn[c]);
		memcpy(want.data() + misalign + v*st + 2*c, &h, 2);
	}
	CHECK(bytes + misalign == 0 || memcmp(want.data(), block, bytes + misalign) == 0, "bytes nvert %u N %u stride %u misalign %u which %d seed %u", nvert, N, stride, misalign, which, seed);
	free(block); free(values);
}

int main() {
	const uint32_t sizes[] = {0, 1, 2, 3, 7, 8, 9, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2049, 5000};
	uint32_t runs = 0;
	for(uint32_t nvert : sizes) for(uint32_t N = 1; N <= 4; N++) for(int which = 0; which < 2; which++) {
		const uint32_t strides[] = {0, 2*N, 2*N + 2, 16};
		for(uint32_t stride : strides) for(uint32_t misalign = 0; misalign < 16; misalign += 2) {
			one(nvert, N, stride, misalign, which, runs, -30000, 65536); runs++;
		}
		// a span that does not fit; the whole int32 range (the span in 64 bits)
		one(nvert, N, 0, 2, which, 7, -40000, 65537); one(nvert, N, 2*N + 2, 0, which, 8, INT32_MIN, 4294967296ll); runs += 2;
	}
	if(failures) { printf("quant_out_check: %d failures\n", failures); return 1; }
	printf("quant_out_check ok (%u runs)\n", runs);
	return 0;
}
