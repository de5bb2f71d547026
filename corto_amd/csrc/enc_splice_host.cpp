// enc_splice_host.cpp — the test hooks of crthip_encode_batch_to_device's splice (crthip_encode_splice_model, crthip_splice_copy_model,
// crthip_encode_splice_plan_model): the plan and the mover of enc_splice.h on the host, in k_encode_splice.hip's partition - one "wave" a
// tile, its 64 lanes walked in a loop, the tiles in a shuffled order (they are independent: any order gives the same bytes) - over payload
// that the host encoder's own writers made (encoder.cpp: encode_host_coded).  The payload lies in buffers of this file's own, each with
// the slack the mover's aligned reads need (enc_splice.h: SOURCES), and stands for what the coders leave in device memory.
#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/corto_hip.h"
#include "enc_splice.h"
#include "encoder_internal.h"

using namespace corto_hip;

namespace {

// every tile of every job once, in an order drawn from `seed`, lanes from the last to the first
void run_tiles(const std::vector<SpliceJob> &jobs, const std::vector<uint32_t> &tile_start, uint32_t seed) {
	const uint32_t tiles = tile_start.back();
	std::vector<uint32_t> order(tiles);
	for(uint32_t i = 0; i < tiles; i++) order[i] = i;
	uint64_t x = 0x9E3779B97F4A7C15ull ^ seed;
	for(uint32_t i = tiles; i > 1; i--) {                                // Fisher-Yates on a 64-bit LCG
		x = x*6364136223846793005ull + 1442695040888963407ull;
		std::swap(order[i - 1], order[(uint32_t)((x >> 33) % i)]);
	}
	for(uint32_t w : order) {
		const size_t j = (size_t)(std::upper_bound(tile_start.begin(), tile_start.end() - 1, w) - tile_start.begin()) - 1;   // enc_job_of
		for(uint32_t lane = ESP_LANES; lane-- > 0;) esp_copy_lane(jobs[j], w - tile_start[j], lane);
	}
}

// the payload of one item in the place of device memory: every part in a buffer with 16 bytes on either side, at a start that walks
// through the sixteen alignments
struct Payload {
	std::vector<std::vector<uint8_t>> bufs;
	uint32_t next = 0;
	const uint8_t *put(const void *p, size_t n) {
		const uint32_t a = next++ & 15u;
		bufs.emplace_back(n + 64, (uint8_t)0xEE);
		uint8_t *at = bufs.back().data() + 16;
		at += (16u - ((uintptr_t)at & 15u)) & 15u;
		at += a;
		if(n) memcpy(at, p, n);
		return at;
	}
};

// one item's payload out of the host encoder's buffers into the place of device memory
void rehome(HostCodedItem &h, Payload &pay) {
	for(CodedStream &x : h.coded.streams) {
		if(x.words) x.words = pay.put(x.words, (size_t)x.nwords*4);
		for(CodedBlock &b : x.blocks) if(b.bytes) b.payload = pay.put(b.payload, b.bytes);
	}
}

int64_t splice_model(const crthip_mesh *m, const crthip_attr_list *extra, uint32_t misalign, uint8_t *out, size_t cap) {
	HostCodedItem h;
	{ const int e = encode_host_coded(m, extra, h); if(e) return e; }
	Payload pay;
	rehome(h, pay);
	SplicePlan P;
	size_t used = 0;
	const uint64_t len = P.item(h.frame, h.slots, h.coded.streams.data(), h.split_words, used);
	const uint64_t total = P.at;
	if(!out || cap < total) return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_encode_splice_model: output buffer too small");
	// the literal buffer on a 4-byte boundary (all the device promises it: it follows the job table) with slack; the arena `misalign`
	// bytes off a 16-byte boundary, between two canaries
	std::vector<uint8_t> lit(P.literal.size() + 64, 0xEE), arena(total + 64, 0xC3);
	uint8_t *lb = lit.data() + 16; lb += (16u - ((uintptr_t)lb & 15u)) & 15u; lb += 4*(misalign & 3u);
	if(!P.literal.empty()) memcpy(lb, P.literal.data(), P.literal.size());
	uint8_t *ab = arena.data() + 16; ab += (16u - ((uintptr_t)ab & 15u)) & 15u; ab += misalign;
	std::vector<SpliceJob> jobs;
	std::vector<uint32_t> tile_start;
	splice_jobs(P, lb, ab, jobs, tile_start);
	run_tiles(jobs, tile_start, misalign + 1);
	for(const uint8_t *p = arena.data(); p < ab; p++) if(*p != 0xC3) return ctx_fail(CRTHIP_E_DEVICE, "crthip_encode_splice_model: a byte in front of the arena was written");
	for(const uint8_t *p = ab + total; p < arena.data() + arena.size(); p++) if(*p != 0xC3) return ctx_fail(CRTHIP_E_DEVICE, "crthip_encode_splice_model: a byte behind the arena was written");
	memcpy(out, ab, total);
	return (int64_t)len;
}

int64_t plan_model(uint32_t n, const crthip_mesh *meshes, const crthip_attr_list *extra, uint64_t *blob_offset, uint32_t *blob_len,
                   crthip_splice_stats *stats, uint64_t *pieces, size_t piece_cap, uint32_t chunk_items) {
	crthip_splice_stats S{};
	uint64_t at = 0;                                                     // the arena's running offset: a chunk's plan begins where the last one ended
	size_t npieces = 0;
	for(uint32_t first = 0; first < n; first += chunk_items ? chunk_items : n) {
		const uint32_t last = chunk_items && n - first > chunk_items ? first + chunk_items : n;
		SplicePlan P(at);
		std::vector<HostCodedItem> items(last - first);                  // (the plan's inputs point into them)
		Payload pay;
		for(uint32_t i = first; i < last; i++) {
			blob_len[i] = 0;
			HostCodedItem &h = items[i - first];
			if(encode_host_coded(&meshes[i], extra ? &extra[i] : nullptr, h)) continue;
			rehome(h, pay);
			size_t used = 0;
			blob_len[i] = (uint32_t)P.item(h.frame, h.slots, h.coded.streams.data(), h.split_words, used);
		}
		std::vector<SpliceJob> jobs;
		std::vector<uint32_t> tile_start;
		S.jobs += (uint32_t)splice_jobs(P, nullptr, nullptr, jobs, tile_start);
		S.pieces += (uint32_t)P.pieces.size(); S.literal_bytes += P.literal_bytes; S.device_bytes += P.device_bytes; S.launches++;
		for(const SplicePiece &p : P.pieces) {
			if(pieces && npieces < piece_cap) { pieces[3*npieces] = p.dst; pieces[3*npieces + 1] = p.bytes; pieces[3*npieces + 2] = p.literal; }
			npieces++;
		}
		at = P.at;
	}
	S.arena_bytes = at;
	if(crthip_arena_layout(n, blob_len, blob_offset) != at) return ctx_fail(CRTHIP_E_DEVICE, "crthip_encode_splice_plan_model: the plan and crthip_arena_layout disagree");
	if(stats) *stats = S;
	return (int64_t)npieces;
}

} // namespace

extern "C" int64_t crthip_encode_splice_model(const crthip_mesh *mesh, const crthip_attr_list *extra, uint32_t dst_misalign, uint8_t *out, size_t cap) {
	if(dst_misalign > 15) return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_encode_splice_model: dst_misalign must be 0..15");
	try {
		return splice_model(mesh, extra, dst_misalign, out, cap);
	} catch(const std::bad_alloc &) {
		return ctx_fail(CRTHIP_E_NOMEM, nullptr);
	} catch(...) {
		return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_encode_splice_model: internal error");
	}
}

extern "C" int crthip_splice_copy_model(const uint8_t *src, uint8_t *dst, uint64_t bytes, uint32_t seed) {
	if(bytes && (!src || !dst)) return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_splice_copy_model: null argument");
	try {
		std::vector<SpliceJob> jobs(1);
		jobs[0].src = src; jobs[0].dst = dst; jobs[0].bytes = bytes;
		std::vector<uint32_t> tile_start = {0u, esp_tiles(jobs[0])};
		run_tiles(jobs, tile_start, seed);
		return CRTHIP_OK;
	} catch(const std::bad_alloc &) {
		return ctx_fail(CRTHIP_E_NOMEM, nullptr);
	}
}

extern "C" int64_t crthip_encode_splice_plan_model(uint32_t n, const crthip_mesh *meshes, const crthip_attr_list *extra, uint64_t *blob_offset, uint32_t *blob_len,
                                                   crthip_splice_stats *stats, uint64_t *pieces, size_t piece_cap, uint32_t chunk_items) {
	if((n && !meshes) || !blob_offset || !blob_len) return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_encode_splice_plan_model: null argument");
	try {
		return plan_model(n, meshes, extra, blob_offset, blob_len, stats, pieces, piece_cap, chunk_items);
	} catch(const std::bad_alloc &) {
		return ctx_fail(CRTHIP_E_NOMEM, nullptr);
	} catch(...) {
		return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_encode_splice_plan_model: internal error");
	}
}
