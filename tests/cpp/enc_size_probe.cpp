// enc_size_probe.cpp — the encoders' tile and size-class limits, answered on the host with the library's own headers (device_plan.h,
// kernels.h, enc_topology.h, enc_splice.h), for tests/test_encode_size_classes_cpu.py and tests/test_encode_size_classes_gpu.py.  One query a
// line on stdin, one answer a line on stdout:
//   const NAME                 -> VALUE       ENC_PACK_MAX_N, ENC_STAGE, ENC_STAGE_PAD, ENC_HIST_CHUNK, ENC_TRIE_LDS_MAX, RS_TILE, RS_THREADS,
//                                             DENC_BLOCK, ETOPO_LDS_MAX, ESP_TILE; and, restated from .cpp / .hip files (see below):
//                                             DIRECT_BYTES, ENC_PACK_TILE_WORDS, ENC_PARSE_WINDOW, ENC_DELTA_SCAN, ENC_JOB_BLOCK
//   rs_blocks N                -> BLOCKS      workgroups of one radix pass over N records
//   rs_bits VBASE              -> BITS        key bits the corner sort runs over when the batch's estimated-normal vertices total VBASE
//   delta_blocks COUNT         -> BLOCKS      workgroups of k_enc_delta for an attribute of COUNT encoded vertices (not BORDER normals: one)
//   job_blocks COUNT           -> BLOCKS      256-thread blocks of a job of COUNT items (k_enc_quantize_batch, k_enc_corners, k_enc_est_normal)
//   hist_chunks SIZE           -> CHUNKS      k_enc_hist workgroups of a stream of SIZE bytes
//   parse SIZE                 -> ONE_WINDOW ONE_STAGE   k_enc_tun_parse: the stream is one 64-position window; its bytes are staged once
//   fits NVERT NFACE           -> 0|1         enc_topo_fits_lds
//   fits_last_closed           -> NVERT       the largest closed mesh (nface = 2*nvert - 4) that walks in LDS
//   parse_lds ENTRIES          -> BYTES       enc_parse_lds
//   trie NSYM L0 L1 ... L255   -> BOUND ENTRIES DEVICE    a stream's level_bound from its dictionary's word lengths, level_bound*nsym^2, and
//                                             whether the device builds its trie (entries <= ENC_TRIE_LDS_MAX)
//   trie_in_lds NTRIE LAUNCH   -> 0|1         k_enc_tun_parse keeps a stream's trie of NTRIE entries in LDS in a launch sized for LAUNCH
//   direct BYTES               -> 0|1         build_image sends an input of BYTES bytes straight from the caller's array
//   esp_tiles MISALIGN BYTES   -> TILES       esp_tiles of a piece whose destination is MISALIGN bytes past a 16-byte boundary
// What lives in a header is called; what lives inside a .cpp or .hip file is restated under RESTATED below, each with the line it restates -
// tests/test_encode_size_classes_cpu.py reads those lines from the sources and fails when one no longer says what is restated here.
#include <hip/hip_runtime.h>

#include "device_plan.h"
#include "enc_splice.h"
#include "enc_topology.h"
#include "kernels.h"

#include <iostream>
#include <sstream>
#include <string>

using namespace corto_hip;

// ---- RESTATED ----
// encode_batch.cpp: `constexpr uint64_t DIRECT_BYTES = 1u << 20;`
static const uint64_t R_DIRECT_BYTES = 1u << 20;
// encode_batch.cpp: `uint32_t rs_blocks(uint32_t n) { return std::max(1u, (n + RS_TILE - 1)/RS_TILE); }`
static uint32_t r_rs_blocks(uint32_t n) { return std::max(1u, (n + RS_TILE - 1)/RS_TILE); }
// encode_batch.cpp (stage_estimate): `uint32_t bits = 8;` / `while(bits < 32 && (vbase >> bits)) bits += 8;`
static uint32_t r_rs_bits(uint32_t vbase) { uint32_t bits = 8; while(bits < 32 && (vbase >> bits)) bits += 8; return bits; }
// k_encode.hip: `constexpr uint32_t ENC_PACK_TILE_WORDS = 256*ENC_PACK_MAX_N;` and `__shared__ uint32_t buf[ENC_PACK_TILE_WORDS + 4];`
static const uint32_t R_PACK_TILE_WORDS = 256*ENC_PACK_MAX_N + 4;
// k_encode.hip (enc_parse_body): a window is the 64 positions from `base` (`const uint32_t p = base + lane;`), the next one starts where the
// chain through it lands (data decides); `if(base + 64 + ENC_STAGE_PAD > s1 && s1 < size) {` stages source bytes from the window's first
// one, `s0 = base; s1 = min(size, s0 + ENC_STAGE + ENC_STAGE_PAD);` - so a stream within one stage is never staged again
static const uint32_t R_PARSE_WINDOW = 64;
static bool r_one_window(uint32_t size) { return size <= R_PARSE_WINDOW; }
static bool r_one_stage(uint32_t size) { return std::min(size, ENC_STAGE + ENC_STAGE_PAD) >= size; }
// k_encode.hip (k_enc_tables): `bound += l > 2 ? (l - 1)/2 : 0u;` / `E.level_bound = 1 + bound;`
// encode_gpu.cpp: `const uint64_t entries = (uint64_t)hd[1]*tabs[i].nsym*tabs[i].nsym;` / `if(entries <= ENC_TRIE_LDS_MAX) { dev_ids.push_back(i);`
static uint32_t r_level_bound(const uint32_t *len) { uint32_t b = 0; for(int c = 0; c < 256; c++) b += len[c] > 2 ? (len[c] - 1)/2 : 0u; return 1 + b; }
// k_encode.hip (k_enc_tun_parse): `if(S.ntrie <= trie_lds_entries) enc_parse_body<true>(S, as_lds(lds_));`
static bool r_trie_in_lds(uint32_t ntrie, uint32_t launch) { return ntrie <= launch; }
// k_encode_batch.hip (k_enc_delta): `for(uint32_t base = 0; base < J.count; base += 256) {` - BORDER's compaction scans 256 vertices a step
static const uint32_t R_DELTA_SCAN = 256;
// encode_batch.cpp (stage_estimate, and the quantiser's table alike): `fb += (J.nface + 255)/256; vb += (J.nvert + 255)/256;`
static const uint32_t R_JOB_BLOCK = 256;
// encode_batch.cpp (stage_delta): `blocks += J.kind == DENC_NRM_BORDER ? 1u : (J.count + DENC_BLOCK - 1)/DENC_BLOCK;`
static uint32_t r_delta_blocks(uint32_t count) { return (count + DENC_BLOCK - 1)/DENC_BLOCK; }
// encode_gpu.cpp: `for(uint32_t b = 0; b < sizes[i]; b += ENC_HIST_CHUNK) chunks.push_back(`
static uint32_t r_hist_chunks(uint32_t size) { uint32_t n = 0; for(uint64_t b = 0; b < size; b += ENC_HIST_CHUNK) n++; return n; }

int main() {
	std::string line;
	while(std::getline(std::cin, line)) {
		std::istringstream in(line);
		std::string q;
		if(!(in >> q)) continue;
		if(q == "const") {
			std::string n; in >> n;
			const uint64_t v = n == "ENC_PACK_MAX_N" ? ENC_PACK_MAX_N : n == "ENC_STAGE" ? ENC_STAGE : n == "ENC_STAGE_PAD" ? ENC_STAGE_PAD :
				n == "ENC_HIST_CHUNK" ? ENC_HIST_CHUNK : n == "ENC_TRIE_LDS_MAX" ? ENC_TRIE_LDS_MAX : n == "RS_TILE" ? RS_TILE : n == "RS_THREADS" ? RS_THREADS :
				n == "DENC_BLOCK" ? DENC_BLOCK : n == "ETOPO_LDS_MAX" ? ETOPO_LDS_MAX : n == "ESP_TILE" ? ESP_TILE : n == "DIRECT_BYTES" ? R_DIRECT_BYTES :
				n == "ENC_PACK_TILE_WORDS" ? R_PACK_TILE_WORDS : n == "ENC_PARSE_WINDOW" ? R_PARSE_WINDOW : n == "ENC_DELTA_SCAN" ? R_DELTA_SCAN :
				n == "ENC_JOB_BLOCK" ? R_JOB_BLOCK : ~0ull;
			if(v == ~0ull) std::cout << "?\n"; else std::cout << v << "\n";
		} else if(q == "rs_blocks") { uint32_t n; in >> n; std::cout << r_rs_blocks(n) << "\n"; }
		else if(q == "rs_bits") { uint32_t v; in >> v; std::cout << r_rs_bits(v) << "\n"; }
		else if(q == "delta_blocks") { uint32_t n; in >> n; std::cout << r_delta_blocks(n) << "\n"; }
		else if(q == "job_blocks") { uint32_t n; in >> n; std::cout << (n + R_JOB_BLOCK - 1)/R_JOB_BLOCK << "\n"; }
		else if(q == "hist_chunks") { uint32_t n; in >> n; std::cout << r_hist_chunks(n) << "\n"; }
		else if(q == "parse") { uint32_t n; in >> n; std::cout << r_one_window(n) << " " << r_one_stage(n) << "\n"; }
		else if(q == "fits") { uint32_t nv, nf; in >> nv >> nf; std::cout << enc_topo_fits_lds(nv, nf) << "\n"; }
		else if(q == "fits_last_closed") {
			uint32_t last = 0;
			for(uint32_t nv = 4; nv <= 70000; nv++) if(enc_topo_fits_lds(nv, 2*nv - 4)) last = nv;
			std::cout << last << "\n";
		} else if(q == "parse_lds") { uint32_t n; in >> n; std::cout << enc_parse_lds(n) << "\n"; }
		else if(q == "trie") {
			uint32_t nsym, len[256] = {0};
			in >> nsym;
			for(int c = 0; c < 256; c++) in >> len[c];
			const uint64_t bound = r_level_bound(len), entries = bound*nsym*nsym;
			std::cout << bound << " " << entries << " " << (entries <= ENC_TRIE_LDS_MAX) << "\n";
		} else if(q == "trie_in_lds") { uint32_t n, l; in >> n >> l; std::cout << r_trie_in_lds(n, l) << "\n"; }
		else if(q == "direct") { uint64_t b; in >> b; std::cout << (b >= R_DIRECT_BYTES) << "\n"; }
		else if(q == "esp_tiles") {
			uint64_t m, b; in >> m >> b;
			SpliceJob J{nullptr, (uint8_t *)(uintptr_t)(4096 + (m & 15u)), b};
			std::cout << esp_tiles(J) << "\n";
		} else std::cout << "?\n";
		std::cout.flush();
	}
	return 0;
}
