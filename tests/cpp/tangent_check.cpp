// tangent_check.cpp — both partitions of csrc/tangent.h on the host under AddressSanitizer and UBSan
// (tests/test_computed_tangents_sanitize_cpu.py): a stand-alone program, host code only.  Every input and the destination is a heap block of
// its own that ENDS exactly with the last element / the last vertex's record, so a read or a store one byte too far is reported; the inputs
// span all of int32 (the sums wrap: arithmetic on signed integers would be reported), indices beyond nvert and NaN normals are among them.
// The two partitions must leave the same bytes under every seed, and nothing between the records.  Built with csrc/tangent_host.cpp, whose
// one dependency on the library (ctx_fail) is defined here.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/corto_hip.h"
#include "tangent.h"

using namespace corto_hip;

namespace corto_hip { int ctx_fail(int code, const char *) { return code; } }

static int failures = 0;
#define CHECK(cond, ...) do { if(!(cond)) { failures++; printf("FAILED %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } while(0)

static uint64_t rng_state;
static uint64_t rng() { rng_state = rng_state*6364136223846793005ull + 1442695040888963407ull; return rng_state >> 16; }

template <typename T> static T *block(size_t n) { return (T *)malloc(n ? n*sizeof(T) : 1); }

static void one(uint32_t nvert, uint32_t nface, bool u16, bool normal_i16, uint32_t format, uint32_t stride, int bits, uint32_t seed) {
	rng_state = 0x9E3779B97F4A7C15ull ^ ((uint64_t)nvert*131u + nface*7u + seed);
	int32_t *P = block<int32_t>((size_t)nvert*3), *t = block<int32_t>((size_t)nvert*2);
	const uint64_t mask = bits >= 32 ? 0xFFFFFFFFull : (1ull << bits) - 1;
	for(size_t e = 0; e < (size_t)nvert*3; e++) P[e] = bits >= 32 ? (int32_t)(uint32_t)rng() : (int32_t)(rng() & mask) - (int32_t)(mask >> 1);
	for(size_t e = 0; e < (size_t)nvert*2; e++) t[e] = bits >= 32 ? (int32_t)(uint32_t)rng() : (int32_t)(rng() & mask) - (int32_t)(mask >> 1);
	void *faces = u16 ? (void *)block<uint16_t>((size_t)nface*3) : (void *)block<uint32_t>((size_t)nface*3);
	for(size_t e = 0; e < (size_t)nface*3; e++) {
		uint32_t v = nvert ? (uint32_t)(rng() % nvert) : 0u;
		if(rng() % 97 == 0) v = nvert + (uint32_t)(rng() % 5);               // out of range: the face adds nothing
		if(u16) ((uint16_t *)faces)[e] = (uint16_t)v; else ((uint32_t *)faces)[e] = v;
	}
	void *normal = normal_i16 ? (void *)block<int16_t>((size_t)nvert*3) : (void *)block<float>((size_t)nvert*3);
	for(size_t e = 0; e < (size_t)nvert*3; e++) {
		const int32_t v = (int32_t)(rng() % 65535) - 32767;
		if(normal_i16) ((int16_t *)normal)[e] = (int16_t)v;
		else ((float *)normal)[e] = rng() % 61 == 0 ? NAN : (float)v/32767.0f;
	}
	const uint32_t el = format == CRTHIP_FMT_INT16 ? 2u : 4u, st = stride ? stride : 4*el;
	const size_t bytes = nvert ? (size_t)(nvert - 1)*st + 4*el : 0;
	std::vector<uint8_t> first;
	for(int which = 0; which < 2; which++) for(uint32_t s = 0; s < 2; s++) {
		uint8_t *out = block<uint8_t>(bytes);                                // ends with the last vertex's record
		memset(out, 0xA5, bytes);
		const int rc = crthip_tangent_model(P, t, faces, u16, nvert, nface, normal, normal_i16 ? CRTHIP_FMT_INT16 : CRTHIP_FMT_FLOAT, 0, out, format, stride, which, seed + s);
		CHECK(rc == 0, "rc %d nvert %u nface %u", rc, nvert, nface);
		for(size_t v = 0; v + 1 < nvert; v++) for(size_t b = 4*el; b < st; b++) CHECK(out[v*st + b] == 0xA5, "padding nvert %u stride %u", nvert, stride);
		if(format == CRTHIP_FMT_FLOAT) for(size_t v = 0; v < nvert; v++) for(int c = 0; c < 4; c++) { float f; memcpy(&f, out + v*st + 4*c, 4); CHECK(!std::isnan(f), "NaN at %zu", v); }
		if(first.empty() && bytes) first.assign(out, out + bytes);
		else CHECK(bytes == 0 || memcmp(first.data(), out, bytes) == 0, "partitions differ: nvert %u nface %u which %d seed %u bits %d", nvert, nface, which, seed + s, bits);
		free(out);
	}
	free(P); free(t); free(faces); free(normal);
}

int main() {
	const uint32_t sizes[] = {0, 1, 3, 64, 255, 256, 257, 1025, 2304, 2305};
	uint32_t runs = 0;
	for(uint32_t nvert : sizes) for(int bits : {6, 14, 32}) for(int k = 0; k < 4; k++) {
		if(nvert > 2304) { continue; }                                       // (which 0 ends at 2 304 vertices)
		const uint32_t nface = nvert ? 2*nvert + (uint32_t)k*511u : 0u;
		const bool u16 = k & 1, ni16 = k & 2;
		one(nvert, nface, u16, ni16, CRTHIP_FMT_FLOAT, k == 3 ? 32u : 0u, bits, runs); runs++;
		one(nvert, nface, u16, ni16, CRTHIP_FMT_INT16, k == 2 ? 12u : 0u, bits, runs); runs++;
	}
	if(failures) { printf("tangent_check: %d failures\n", failures); return 1; }
	printf("tangent_check ok (%u runs)\n", runs);
	return 0;
}
