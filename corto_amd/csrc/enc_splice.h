// enc_splice.h — the container splice of crthip_encode_batch_to_device: where every byte of every .crt of a chunk goes in the caller's
// device arena (the plan, host only) and how one piece gets there (the mover, __host__ __device__: k_encode_splice.hip runs it one wave a
// tile, crthip_encode_splice_model / crthip_splice_copy_model walk the same source on the host, lanes in a loop, tiles in a shuffled order;
// tests/test_encode_device_out_cpu.py holds both against crthip_encode_attrs).
//
// THE RULE.  A container is its frame (the container without its streams) with the coded streams (encoder_internal.h: Coded) put in at
// the slots its body recorded (Deferred, BatchStream: `at` in the frame, `kind`), in order: a bit stream is its word count, zeros to a
// 4-byte position OF THE CONTAINER, its words (OutStream::write(BitStream&), cstream.h:79-89); a value stream's words come before its
// blocks; a block is its header, then its payload; the slot of the CLERS split bits (kind BATCH_BITS) takes the split words, which the
// host has packed.  write_container below is the only place that knows this, for every encoder: it emits host-made bytes, zeros and
// payload by address into an output - a SplicePlan, or a ByteOut where the payload is in host memory.
//
// The plan.  The host knows every size without a payload byte: what it makes itself - frame bytes, word counts, the padding zeros, the
// split words, the block headers, the zeros between a blob's end and the next 16-byte multiple (the plan's own business, not the
// writer's) - goes into ONE literal buffer for the chunk, and the payload (bit words, codewords, raw logs and symbols) is named by its
// device address.  The result is a list of pieces {source, arena offset, bytes} in destination order that covers the arena once.
// Neighbouring literal bytes are one piece.  The literal buffer is packed: it holds the host-made bytes and nothing else, so what goes up
// is literal_bytes exactly, and a literal piece is moved from whatever alignment it has, like any other.
//
// The mover.  A piece is cut into tiles at 16-byte multiples of the DESTINATION, ESP_TILE bytes apart (a C2-sized stream is hundreds of
// tiles, not one wave's loop); the job table names pieces, tile_start[j] is the first tile of piece j (the block_start convention of the
// batch's other kernels), one wave takes one tile.  Within a tile: the bytes up to the destination's 16-byte boundary go by byte stores
// (only a piece's first tile has any), the body as one aligned 16-byte store a lane, the bytes behind the last whole 16 by byte stores
// (only its last tile).  The body's source is read as aligned dwords - or, where source and destination agree modulo 16, as aligned
// 16-byte loads - and funnel-shifted where they disagree modulo 4.  Two rules make tiles independent of each other and of launch order:
// every output byte is written by exactly one store of exactly one tile, and no destination byte is ever read.
//
// SOURCES.  The aligned reads of a body touch up to 3 bytes before a piece's first body byte and up to 3 behind its last.  Every source
// is a library allocation whose base is 256-byte aligned and which is allocated with at least 16 bytes behind its last region: the value
// coder's image and the Tunstall coder's (encode_gpu.cpp) and host mode's CLERS block (encode_batch.cpp), all three owned by the Coded
// object, the chunk image (encode_batch.cpp), the literal buffer (splice_to_device: 16 bytes of slack).  No piece ever sources from a caller's array.  Keep this true when a region moves.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include <hip/hip_runtime.h>

#include "device_plan.h"
#include "encoder_internal.h"

#define ESP_HD __host__ __device__ inline

namespace corto_hip {

constexpr uint32_t ESP_THREADS = 256;                     // a workgroup: four waves, four neighbouring tiles
constexpr uint32_t ESP_LANES = 64;
constexpr uint32_t ESP_TILE = 4096;                       // destination bytes a wave moves: four 16-byte stores a lane

// ---- the mover ----

ESP_HD uint32_t esp_tiles(const SpliceJob &J) {
	return (uint32_t)((((uint64_t)(uintptr_t)J.dst & 15u) + J.bytes + ESP_TILE - 1)/ESP_TILE);
}
// tile t of a piece: its bytes [lo, hi).  Every cut between two tiles is a 16-byte multiple of the destination.
ESP_HD void esp_tile_range(const SpliceJob &J, uint32_t t, uint64_t &lo, uint64_t &hi) {
	const uint64_t m = (uint64_t)(uintptr_t)J.dst & 15u;
	lo = t ? (uint64_t)t*ESP_TILE - m : 0;
	hi = (uint64_t)(t + 1)*ESP_TILE - m;
	if(hi > J.bytes) hi = J.bytes;
}
// the dword at byte `shift` (0..3) of the pair hi:lo
ESP_HD uint32_t esp_funnel(uint32_t lo, uint32_t hi, uint32_t shift) {
#if defined(__HIP_DEVICE_COMPILE__)
	return __builtin_amdgcn_alignbyte(hi, lo, shift);
#else
	return shift ? (lo >> (8*shift)) | (hi << (32 - 8*shift)) : lo;
#endif
}
struct EspVec { uint32_t w[4]; };
ESP_HD uint32_t esp_load4(const uint8_t *p) {             // p is 4-byte aligned
#if defined(__HIP_DEVICE_COMPILE__)
	return *(const uint32_t *)p;
#else
	uint32_t v; memcpy(&v, p, 4); return v;
#endif
}
ESP_HD EspVec esp_load16(const uint8_t *p) {              // p is 16-byte aligned
	EspVec v;
#if defined(__HIP_DEVICE_COMPILE__)
	const uint4 x = *(const uint4 *)p;
	v.w[0] = x.x; v.w[1] = x.y; v.w[2] = x.z; v.w[3] = x.w;
#else
	memcpy(v.w, p, 16);
#endif
	return v;
}
ESP_HD void esp_store16(uint8_t *p, const EspVec &v) {    // p is 16-byte aligned
#if defined(__HIP_DEVICE_COMPILE__)
	*(uint4 *)p = make_uint4(v.w[0], v.w[1], v.w[2], v.w[3]);
#else
	memcpy(p, v.w, 16);
#endif
}

// what lane `lane` of the wave that has tile t of piece J does
ESP_HD void esp_copy_lane(const SpliceJob &J, uint32_t t, uint32_t lane) {
	uint64_t lo, hi;
	esp_tile_range(J, t, lo, hi);
	if(lo >= hi) return;
	const uint8_t *s = J.src + lo;
	uint8_t *d = J.dst + lo;
	const uint64_t n = hi - lo;
	uint64_t head = (16u - ((uint64_t)(uintptr_t)d & 15u)) & 15u;
	if(head > n) head = n;
	const uint64_t nvec = (n - head)/16, tail = n - head - nvec*16;
	if(lane < head) d[lane] = s[lane];                                           // (head <= 15: the lanes of the tail are others)
	if(lane >= 32 && lane - 32 < tail) { const uint64_t o = head + nvec*16 + (lane - 32); d[o] = s[o]; }
	const uint8_t *sb = s + head;
	uint8_t *db = d + head;
	if((((uintptr_t)sb) & 15u) == 0) {                                           // source and destination agree modulo 16
		for(uint64_t v = lane; v < nvec; v += ESP_LANES) esp_store16(db + 16*v, esp_load16(sb + 16*v));
		return;
	}
	const uint32_t shift = (uint32_t)((uintptr_t)sb & 3u);
	const uint8_t *sa = sb - shift;
	for(uint64_t v = lane; v < nvec; v += ESP_LANES) {
		const uint8_t *p = sa + 16*v;
		const uint32_t w0 = esp_load4(p), w1 = esp_load4(p + 4), w2 = esp_load4(p + 8), w3 = esp_load4(p + 12);
		const uint32_t w4 = shift ? esp_load4(p + 16) : 0u;                         // (agreeing modulo 4: nothing is read beyond the 16 bytes)
		EspVec o;
		o.w[0] = esp_funnel(w0, w1, shift); o.w[1] = esp_funnel(w1, w2, shift); o.w[2] = esp_funnel(w2, w3, shift); o.w[3] = esp_funnel(w3, w4, shift);
		esp_store16(db + 16*v, o);
	}
}

// ---- the container writer (host) ----

// One container into `o`: o.lit(p, n) takes host-made bytes (p == nullptr: zeros), o.payload(p, n) payload that lies at p.  Returns how
// many of `streams` it used: one per slot but the split bits.
template <class Out, class SlotT>
size_t write_container(Out &o, const std::vector<uint8_t> &frame, const std::vector<SlotT> &slots, const CodedStream *streams,
                       const std::vector<uint32_t> &split_words) {
	uint64_t n = 0;                                       // bytes of this container so far
	auto lit = [&](const void *p, uint64_t b) { o.lit(p, b); n += b; };
	auto count = [&](uint32_t nwords) { lit(&nwords, 4); lit(nullptr, (4u - (n & 3u)) & 3u); };
	size_t prev = 0, r = 0;
	for(const SlotT &s : slots) {
		lit(frame.data() + prev, s.at - prev); prev = s.at;
		if(s.kind == BATCH_BITS) { count((uint32_t)split_words.size()); lit(split_words.data(), split_words.size()*4); continue; }
		const CodedStream &x = streams[r++];
		if(s.kind != CRTHIP_ENC_SYMBOLS) { count(x.nwords); o.payload(x.words, (uint64_t)x.nwords*4); n += (uint64_t)x.nwords*4; }
		for(const CodedBlock &b : x.blocks) { lit(b.head.data(), b.head.size()); o.payload(b.payload, b.bytes); n += b.bytes; }
	}
	lit(frame.data() + prev, frame.size() - prev);
	return r;
}

// the output over host memory: every payload pointer is a host pointer (Coded::on_device == false)
struct ByteOut {
	std::vector<uint8_t> &b;
	void lit(const void *p, uint64_t n) { if(p) b.insert(b.end(), (const uint8_t *)p, (const uint8_t *)p + n); else b.insert(b.end(), (size_t)n, (uint8_t)0); }
	void payload(const uint8_t *p, uint64_t n) { if(n) b.insert(b.end(), p, p + n); }
};

// ---- the plan (host) ----

struct SplicePiece { uint64_t src, dst, bytes; uint32_t literal, pad; };   // src: an offset in the literal buffer, or a device address

struct SplicePlan {
	std::vector<uint8_t> literal;
	std::vector<SplicePiece> pieces;                      // destination order, no gap, no overlap, from the arena offset the plan began at
	uint64_t at = 0;                                      // the arena's running offset: where the next blob starts
	uint64_t literal_bytes = 0, device_bytes = 0;

	explicit SplicePlan(uint64_t begin = 0) : at(begin) {}
	void lit(const void *p, uint64_t n) {                 // p == nullptr: zeros
		if(!n) return;
		if(pieces.empty() || !pieces.back().literal) pieces.push_back(SplicePiece{literal.size(), at, 0, 1u, 0u});
		if(p) literal.insert(literal.end(), (const uint8_t *)p, (const uint8_t *)p + n); else literal.insert(literal.end(), (size_t)n, (uint8_t)0);
		pieces.back().bytes += n; at += n; literal_bytes += n;
	}
	void payload(const uint8_t *p, uint64_t n) {          // p: a device address (Coded::on_device)
		if(!n) return;
		pieces.push_back(SplicePiece{(uint64_t)(uintptr_t)p, at, n, 0u, 0u});
		at += n; device_bytes += n;
	}
	// one container at the running offset (a multiple of 16), then the zeros to the next one; returns the blob's length and adds the
	// streams it used to `used`
	template <class SlotT>
	uint64_t item(const std::vector<uint8_t> &frame, const std::vector<SlotT> &slots, const CodedStream *streams, const std::vector<uint32_t> &split_words, size_t &used) {
		const uint64_t begin = at;
		used += write_container(*this, frame, slots, streams, split_words);
		const uint64_t len = at - begin;
		lit(nullptr, (16u - (at & 15u)) & 15u);
		return len;
	}
};

// the job table of a plan once its literal buffer has an address (lit_base: 4-byte aligned, inside an allocation) and the arena has one (arena: the address
// of arena offset 0); returns the tiles, tile_start gets one entry more than jobs
inline uint64_t splice_jobs(const SplicePlan &P, const uint8_t *lit_base, uint8_t *arena, std::vector<SpliceJob> &jobs, std::vector<uint32_t> &tile_start) {
	jobs.clear(); tile_start.clear();
	uint64_t tiles = 0;
	for(const SplicePiece &p : P.pieces) {
		SpliceJob J;
		J.src = p.literal ? lit_base + p.src : (const uint8_t *)(uintptr_t)p.src;
		J.dst = arena + p.dst; J.bytes = p.bytes;
		jobs.push_back(J); tile_start.push_back((uint32_t)tiles);
		tiles += esp_tiles(J);
	}
	tile_start.push_back((uint32_t)tiles);
	return tiles;
}

} // namespace corto_hip
