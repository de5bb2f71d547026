// output_layout_check.cpp — crthip_output_layout (corto_amd/csrc/host_probe.cpp) as a stand-alone host program, for a build under
// AddressSanitizer / UBSan (tests/test_output_layout_cpu.py).  Built with host_probe.cpp and crt_format.cpp alone: no HIP.
//   output_layout_check CORPUS
// CORPUS: u32 count, then per blob u32 len + bytes.  Every blob sits at the END of a heap block of exactly its length, so that a read past
// it is the sanitizer's.  Checked: the golden blobs one by one and as one list, with and without CRTHIP_LAYOUT_RENDER, against the rule
// restated from crthip_probe; every truncation of every blob's header; the NULL forms; unknown flag bits.  Prints "output_layout_check ok".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/corto_hip.h"

static int failures = 0;
#define CHECK(c) do { if(!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); failures++; } } while(0)

struct Blob { std::unique_ptr<uint32_t[]> mem; const uint8_t *p; uint32_t len; };
// `len` bytes of src at the end of their own 4-byte aligned block
static Blob tight(const uint8_t *src, uint32_t len) {
	Blob b;
	const uint32_t words = (len + 3)/4;
	b.mem.reset(new uint32_t[words ? words : 1]);
	uint8_t *base = (uint8_t *)b.mem.get();
	// (a length that is no multiple of 4 leaves up to 3 bytes of slack behind the blob: keep the start aligned, which crthip_probe asks for)
	std::memcpy(base, src, len);
	b.p = base; b.len = len;
	return b;
}

static uint64_t up256(uint64_t x) { return (x + 255) & ~(uint64_t)255; }

static void check_list(const std::vector<const uint8_t *> &ptrs, const std::vector<uint32_t> &lens, uint32_t flags) {
	const uint32_t n = (uint32_t)ptrs.size();
	std::vector<crthip_blob_info> infos(n);
	size_t nattr = 0;
	for(uint32_t i = 0; i < n; i++) { CHECK(crthip_probe(ptrs[i], lens[i], &infos[i]) == CRTHIP_OK); nattr += infos[i].nattr; }
	// exactly as many entries as the call may write
	std::unique_ptr<crthip_out_array[]> attr(new crthip_out_array[nattr ? nattr : 1]), index(new crthip_out_array[n ? n : 1]);
	uint64_t total = ~0ull, total2 = ~0ull;
	CHECK(crthip_output_layout(n, ptrs.data(), lens.data(), flags, attr.get(), index.get(), &total) == CRTHIP_OK);
	CHECK(crthip_output_layout(n, ptrs.data(), lens.data(), flags, nullptr, nullptr, &total2) == CRTHIP_OK);
	CHECK(total == total2);
	const bool render = (flags & CRTHIP_LAYOUT_RENDER) != 0;
	uint64_t end = 0;
	size_t k = 0;
	for(uint32_t i = 0; i < n; i++) {
		const crthip_blob_info &f = infos[i];
		for(uint32_t a = 0; a < f.nattr; a++, k++) {
			uint64_t bytes = (uint64_t)f.nvert*f.attr[a].components*4; uint32_t fmt = CRTHIP_FMT_FLOAT;
			if(f.attr[a].codec == CRTHIP_CODEC_NORMAL) { bytes = (uint64_t)f.nvert*(render ? 6 : 12); if(render) fmt = CRTHIP_FMT_INT16; }
			else if(f.attr[a].codec == CRTHIP_CODEC_COLOR) { bytes = (uint64_t)f.nvert*4; fmt = CRTHIP_FMT_UINT8; }
			CHECK(attr[k].offset == up256(end)); CHECK(attr[k].bytes == bytes); CHECK(attr[k].format == fmt);
			end = attr[k].offset + attr[k].bytes;
		}
		if(f.nface) {
			const bool u16 = render && f.nvert < 65536;
			CHECK(index[i].offset == up256(end)); CHECK(index[i].bytes == (uint64_t)f.nface*(u16 ? 6 : 12));
			CHECK(index[i].format == (u16 ? CRTHIP_FMT_UINT16 : CRTHIP_FMT_UINT32));
			end = index[i].offset + index[i].bytes;
		} else CHECK(index[i].bytes == 0);
	}
	CHECK(total == up256(end));
}

int main(int argc, char **argv) {
	if(argc < 2) { std::fprintf(stderr, "usage: output_layout_check CORPUS\n"); return 2; }
	FILE *f = std::fopen(argv[1], "rb");
	if(!f) { std::perror(argv[1]); return 2; }
	std::vector<std::vector<uint8_t>> corpus;
	uint32_t n = 0;
	if(std::fread(&n, 4, 1, f) != 1) return 2;
	for(uint32_t i = 0; i < n; i++) {
		uint32_t len = 0;
		if(std::fread(&len, 4, 1, f) != 1) return 2;
		std::vector<uint8_t> b(len);
		if(len && std::fread(b.data(), 1, len, f) != len) return 2;
		corpus.push_back(std::move(b));
	}
	std::fclose(f);

	std::vector<Blob> blobs;
	std::vector<const uint8_t *> ptrs; std::vector<uint32_t> lens;
	for(auto &c : corpus) { blobs.push_back(tight(c.data(), (uint32_t)c.size())); ptrs.push_back(blobs.back().p); lens.push_back(blobs.back().len); }
	for(uint32_t flags : {0u, CRTHIP_LAYOUT_RENDER}) {
		for(size_t i = 0; i < blobs.size(); i++) check_list({ptrs[i]}, {lens[i]}, flags);
		check_list(ptrs, lens, flags);
	}
	// no blobs
	uint64_t total = 7;
	CHECK(crthip_output_layout(0, nullptr, nullptr, 0, nullptr, nullptr, &total) == CRTHIP_OK && total == 0);
	// every truncation of every header (and a little of the body): a code or a layout, never a read past the bytes given
	uint64_t refused = 0, taken = 0;
	for(auto &c : corpus) {
		crthip_blob_info info;
		if(crthip_probe(ptrs[&c - corpus.data()], (uint32_t)c.size(), &info) != CRTHIP_OK) { failures++; continue; }
		const uint32_t upto = info.body_offset + 64 < c.size() ? info.body_offset + 64 : (uint32_t)c.size();
		for(uint32_t len = 0; len <= upto; len++) {
			Blob t = tight(c.data(), len);
			const uint8_t *p = t.p; uint32_t l = len;
			crthip_out_array attr[CRTHIP_MAX_ATTRS], index;
			const int code = crthip_output_layout(1, &p, &l, CRTHIP_LAYOUT_RENDER, attr, &index, &total);
			if(code == CRTHIP_OK) { taken++; CHECK(len >= info.body_offset); }
			else { refused++; CHECK(code == CRTHIP_E_TRUNCATED || code == CRTHIP_E_MAGIC || code == CRTHIP_E_ARGUMENT); CHECK(std::strstr(crthip_last_error(), "(blob 0)") || len == 0); }
		}
		// the failing blob is named by its place in the list
		Blob t = tight(c.data(), 3);
		const uint8_t *two[2] = {ptrs[&c - corpus.data()], t.p}; const uint32_t two_len[2] = {(uint32_t)c.size(), 3};
		CHECK(crthip_output_layout(2, two, two_len, 0, nullptr, nullptr, &total) < 0);
		CHECK(std::strstr(crthip_last_error(), "(blob 1)") != nullptr);
	}
	CHECK(refused > 0 && taken > 0);
	// flags and NULLs
	for(uint32_t flags : {2u, 3u, 0x80000000u, 0xFFFFFFFEu}) CHECK(crthip_output_layout(1, ptrs.data(), lens.data(), flags, nullptr, nullptr, &total) == CRTHIP_E_ARGUMENT);
	CHECK(crthip_output_layout(1, ptrs.data(), lens.data(), 0, nullptr, nullptr, nullptr) == CRTHIP_E_ARGUMENT);
	CHECK(crthip_output_layout(1, nullptr, lens.data(), 0, nullptr, nullptr, &total) == CRTHIP_E_ARGUMENT);
	CHECK(crthip_output_layout(1, ptrs.data(), nullptr, 0, nullptr, nullptr, &total) == CRTHIP_E_ARGUMENT);
	const uint8_t *null_blob = nullptr;
	CHECK(crthip_output_layout(1, &null_blob, lens.data(), 0, nullptr, nullptr, &total) == CRTHIP_E_ARGUMENT);
	if(failures) { std::printf("output_layout_check: %d failures\n", failures); return 1; }
	std::printf("output_layout_check ok: %zu blobs, %llu truncations refused, %llu taken\n", corpus.size(), (unsigned long long)refused, (unsigned long long)taken);
	return 0;
}
