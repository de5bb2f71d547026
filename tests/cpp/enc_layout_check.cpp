// enc_layout_check.cpp — the host side of crthip_mesh_layout under AddressSanitizer / UBSan (tests/test_encode_layout_sanitize_cpu.py builds
// it with encoder.cpp, enc_input_host.cpp and enc_topology_host.cpp): the alignment and stride sweep of tests/test_encode_layout_cpu.py on
// heap blocks that END with the last element an array may be read at - [ptr, ptr + (nvert-1)*stride + one vertex's bytes), nface*3 uint16
// entries - so a read one byte behind a checked extent is a report.  Runs enc_input_check.h in the kernels' partition (which = 1) against the
// host loops (which = 0), enc_topology.h's compact stage on 16-bit entries, and crthip_encode_layout against crthip_encode_attrs.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/corto_hip.h"
#include "encoder_internal.h"

// what the three sources want from the rest of the library: the error slot, and the device stages the host encoder never reaches here
namespace corto_hip {
static std::string last_error;
int ctx_fail(int code, const char *msg) { last_error = msg ? msg : ""; return code; }
int quantize_device(crthip_ctx *, const std::vector<QuantRequest> &) { return CRTHIP_E_DEVICE; }
int encode_value_streams(crthip_ctx *, uint32_t, const std::vector<EncValueStream> &, Coded &, crthip_kernel_times *) { return CRTHIP_E_DEVICE; }
}

namespace {

int failures = 0;
#define CHECK(c) do { if(!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while(0)

uint32_t rnd_state = 12345;
uint32_t rnd() { rnd_state = rnd_state*1664525u + 1013904223u; return rnd_state >> 8; }
float rndf() { return (float)(rnd() & 0xFFFF)/65536.0f*4.0f - 2.0f; }

// a heap block that holds `bytes` bytes at `base` bytes past a 16-byte boundary and ends with them
struct Block {
	uint8_t *raw = nullptr, *p = nullptr;
	Block(size_t bytes, size_t base) {
		// the block's END is fixed by the sanitizer's allocator; place the data so that it ends there and check the start's offset
		for(size_t pad = 0; pad < 16; pad++) {
			raw = (uint8_t *)malloc(bytes + pad + 16);
			p = raw + pad + 16;                                  // data = the block's last `bytes` bytes
			if(((uintptr_t)p & 15u) == (base & 15u)) { memset(raw, 0xA5, pad + 16); return; }
			free(raw);
		}
		raw = p = nullptr;
	}
	~Block() { free(raw); }
	Block(const Block &) = delete;
};

bool same(const crthip_encode_input_result &a, const crthip_encode_input_result &b) { return memcmp(&a, &b, sizeof(a)) == 0; }

void sweep_positions() {
	const uint32_t nverts[] = {1, 3, 4, 5, 1023, 1024, 1025, 2049}, strides[] = {12, 16, 20, 32, 48}, bases[] = {0, 4, 8, 12};
	for(uint32_t nv : nverts) for(uint32_t stride : strides) for(uint32_t base : bases) {
		Block B((size_t)(nv - 1)*stride + 12, base);
		if(!B.p) { CHECK(!"no block at this offset"); continue; }
		std::vector<float> packed((size_t)nv*3);
		const bool special = ((nv + stride/4 + base/4) & 1u) != 0;   // NaNs and infinities for the models alone: the encoder promises no bytes for them
		for(uint32_t i = 0; i < nv; i++) {
			float v[3] = {rndf(), rndf(), rndf()};
			if(special && rnd()%97 == 0) v[rnd()%3] = NAN;
			if(special && rnd()%89 == 0) v[rnd()%3] = rnd()&1 ? INFINITY : -INFINITY;
			if(rnd()%83 == 0) v[rnd()%3] = rnd()&1 ? 0.0f : -0.0f;
			memcpy(B.p + (size_t)i*stride, v, 12);
			for(int k = 0; k < 3; k++) packed[(size_t)i*3 + k] = v[k] - (k == 0 ? 0.5f : k == 1 ? -2.0f : 0.125f);
		}
		crthip_mesh m;
		memset(&m, 0, sizeof(m));
		m.nvert = nv; m.position = (const float *)B.p; m.entropy = CRTHIP_ENTROPY_TUNSTALL;
		crthip_mesh_layout L;
		memset(&L, 0, sizeof(L));
		L.position_stride = stride; L.origin[0] = 0.5f; L.origin[1] = -2.0f; L.origin[2] = 0.125f;
		crthip_encode_input_result r0, r1, ry;
		CHECK(crthip_encode_input_model_layout(&m, &L, 0, &r0) == CRTHIP_OK && crthip_encode_input_model_layout(&m, &L, 1, &r1) == CRTHIP_OK);
		CHECK(same(r0, r1) && r0.recipe == 3);
		crthip_mesh y = m;
		y.position = packed.data();
		CHECK(crthip_encode_input_model(&y, 0, &ry) == CRTHIP_OK && same(r0, ry));
		// the encoder itself through the stride and the origin, against the packed arrays
		std::vector<uint8_t> a(64*nv + 65536), b(a.size());
		if(!special && nv > 1) {                                 // (one point has no volume: q = 0, and no bytes are promised for INT_MIN residuals)
			const int64_t na = crthip_encode_layout(&m, nullptr, &L, a.data(), a.size(), nullptr, nullptr), nb = crthip_encode_attrs(&y, nullptr, b.data(), b.size(), nullptr, nullptr);
			CHECK(na > 0 && na == nb && memcmp(a.data(), b.data(), (size_t)na) == 0);
		}
		memset(L.origin, 0, sizeof(L.origin));
		m.position_bits = 11;
		CHECK(crthip_encode_input_model_layout(&m, &L, 0, &r0) == CRTHIP_OK && crthip_encode_input_model_layout(&m, &L, 1, &r1) == CRTHIP_OK && same(r0, r1) && r0.recipe == 1);
	}
}

void sweep_index() {
	const uint32_t nv = 2049, entries[] = {3, 6, 9, 21, 24, 27, 4095, 4098, 8190, 3069, 3072, 3075};
	std::vector<float> pos((size_t)nv*3);
	for(float &v : pos) v = rndf();
	for(uint32_t n : entries) for(uint32_t off = 0; off < 16; off += 2) {
		const uint32_t nface = n/3;
		Block I((size_t)n*2, off), P((size_t)(nv - 1)*20 + 12, 4);
		if(!I.p || !P.p) { CHECK(!"no block at this offset"); continue; }
		for(uint32_t i = 0; i < nv; i++) memcpy(P.p + (size_t)i*20, &pos[(size_t)i*3], 12);
		std::vector<uint32_t> wide(n);
		for(uint32_t i = 0; i < n; i++) { wide[i] = rnd()%nv; const uint16_t w = (uint16_t)wide[i]; memcpy(I.p + (size_t)i*2, &w, 2); }
		crthip_mesh m;
		memset(&m, 0, sizeof(m));
		m.nvert = nv; m.nface = nface; m.position = (const float *)P.p; m.index = (const uint32_t *)I.p; m.entropy = CRTHIP_ENTROPY_TUNSTALL;
		crthip_mesh_layout L;
		memset(&L, 0, sizeof(L));
		L.flags = CRTHIP_IN_INDEX_UINT16; L.position_stride = 20;
		crthip_mesh y = m;
		y.position = pos.data(); y.index = wide.data();
		crthip_encode_input_result r0, r1, ry;
		CHECK(crthip_encode_input_model_layout(&m, &L, 0, &r0) == CRTHIP_OK && crthip_encode_input_model_layout(&m, &L, 1, &r1) == CRTHIP_OK);
		CHECK(same(r0, r1) && r0.recipe == 2 && !r0.index_out_of_range);
		CHECK(crthip_encode_input_model(&y, 0, &ry) == CRTHIP_OK && same(r0, ry));
		// the topology pass: 16-bit entries through the device source and (widened) the host pass, against the uint32 run
		std::vector<uint32_t> f0((size_t)n), f1(f0), q0((size_t)nv*4), q1(q0), s0(CRTHIP_TOPOLOGY_SPLIT_CAP(nface)), s1(s0);
		std::vector<uint8_t> c0(CRTHIP_TOPOLOGY_CLERS_CAP(nface)), c1(c0);
		uint32_t g0[1], g1[1];
		crthip_topology_result t0, t1;
		memset(&t0, 0, sizeof(t0)); memset(&t1, 0, sizeof(t1));
		t0.faces = f0.data(); t0.group_end = g0; t0.quads = q0.data(); t0.clers = c0.data(); t0.split_words = s0.data();
		t1.faces = f1.data(); t1.group_end = g1; t1.quads = q1.data(); t1.clers = c1.data(); t1.split_words = s1.data();
		for(int which = 0; which < 2; which++) {
			CHECK(crthip_encode_topology_model_layout(&m, &L, which, &t0) == CRTHIP_OK && crthip_encode_topology_model(&y, which, &t1) == CRTHIP_OK);
			CHECK(t0.nvert == t1.nvert && t0.nface == t1.nface && t0.nclers == t1.nclers && t0.nsplit_words == t1.nsplit_words && t0.max_front == t1.max_front);
			CHECK(memcmp(f0.data(), f1.data(), (size_t)t0.nface*12) == 0 && memcmp(c0.data(), c1.data(), t0.nclers) == 0);
			CHECK(memcmp(q0.data(), q1.data(), (size_t)t0.nvert*16) == 0 && memcmp(s0.data(), s1.data(), (size_t)t0.nsplit_words*4) == 0);
		}
		// one entry >= nvert: in the head, a group, the tail - wherever this offset puts entry `at`
		for(uint32_t at : {0u, n/2, n - 1}) {
			uint16_t keep, bad = (uint16_t)nv;
			memcpy(&keep, I.p + (size_t)at*2, 2); memcpy(I.p + (size_t)at*2, &bad, 2);
			CHECK(crthip_encode_input_model_layout(&m, &L, 0, &r0) == CRTHIP_OK && crthip_encode_input_model_layout(&m, &L, 1, &r1) == CRTHIP_OK);
			CHECK(same(r0, r1) && r0.index_out_of_range == 1 && r0.step == 0.0f);
			std::vector<uint8_t> out(16, 0x5A);
			CHECK(crthip_encode_layout(&m, nullptr, &L, out.data(), out.size(), nullptr, nullptr) == CRTHIP_E_ARGUMENT && out[0] == 0x5A);
			memcpy(I.p + (size_t)at*2, &keep, 2);
		}
	}
}

} // namespace

int main() {
	sweep_positions();
	sweep_index();
	if(failures) { printf("enc_layout_check: %d failures\n", failures); return 1; }
	printf("enc_layout_check ok\n");
	return 0;
}
