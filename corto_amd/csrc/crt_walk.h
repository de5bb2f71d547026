// crt_walk.h — walk_blob (crt_format.cpp) restated for ONE blob as __host__ __device__ code that writes a fixed-capacity record instead
// of a BlobLayout.  k_walk.hip runs it one wave per blob over blobs that live only in device memory (crthip_batch_create_resident);
// crt_format.cpp's record_to_layout turns a record back into the BlobLayout walk_blob returns for the same bytes (tests/cpp/walk_probe.cpp
// holds the two side by side).  Same reads in the same order, same CRTHIP_E_* precedence: header() -> groups -> index block -> attribute
// blocks, truncation checked where walk_blob checks it.
//
// The record (rec_cap bytes, a multiple of 16):
//   WalkHead                                      status, end offset, max_front, split, where the rest is
//   blob bytes [0, prefix_len)                    header + groups, 16-byte padded: the host parses exif, names and group properties from
//                                                 them with header() itself
//   body items                                    [clers WalkStream if nface]  then per attribute in name order: WalkAttrItem, its log streams
// A walk that succeeds but does not fit (kilobytes of exif, hundreds of log streams) sets WALK_OVERFLOW: the host walks that blob itself.
// A walk that fails writes its code only, whatever it would have needed.
// Reads go through R: byte(pos) for pos < len and copy(dst, n), which may write dst[0, round16(n)) - the walker never asks for a byte at
// or past len, so a reader that bounds its loads by the 16-byte-rounded extent never leaves the blob.
#pragma once
#include <stdint.h>

#include "../../include/corto_hip.h"
#include "crt_format.h"

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define CRT_HD __host__ __device__ __attribute__((always_inline))
#else
#define CRT_HD __attribute__((always_inline))
#endif

namespace corto_hip {

constexpr uint32_t WALK_RECORD_BYTES = 1024;   // a blob's record: what a resident create copies back per blob
constexpr uint32_t WALK_OVERFLOW = 1u;         // WalkHead.flags: walked fine, did not fit the record
constexpr int WALK_FALLBACK = 1;               // record_to_layout: walk this blob on the host

struct WalkHead {
	int32_t status;
	uint32_t flags;
	uint32_t end_offset, prefix_len, items_off, items_len;
	uint32_t max_front, split_off, split_nwords;
	uint32_t nattr;                            // attributes after the std::map collapse
	uint32_t pad[2];
};
static_assert(sizeof(WalkHead) == 48, "WalkHead is the record's first 48 bytes");

struct WalkAttrItem { uint32_t bits_off, bits_nwords, nlogs; uint8_t normal_prediction, qc[4], pad[3]; };
struct WalkStream {                            // a StreamRef; nprobs bytes of its table follow, padded to 4
	uint8_t mode, nsym, fill, max_sym;
	uint32_t probs_off, size, csize, payload_off;
	uint32_t nprobs;
};

struct WalkAttr { uint32_t name_off, name_len, codec, N, strategy; };
struct WalkWork { WalkAttr attr[CRTHIP_MAX_ATTRS]; };    // the walker's sorted attribute table (LDS on the device)

// the bounds-checked cursor of crt_format.cpp over a reader
template <class R> struct WalkCursor {
	R r;                                       // (held by value: on the device its fields stay in registers)
	uint32_t len, pos = 0;
	bool bad = false;
	CRT_HD WalkCursor(const R &r_, uint32_t len_) : r(r_), len(len_) {}
	CRT_HD bool need(uint64_t n) {
		if(bad || n > len || pos > len - n) { bad = true; return false; }
		return true;
	}
	CRT_HD uint32_t u8() { return need(1) ? r.byte(pos++) : 0u; }
	CRT_HD uint32_t u16() { if(!need(2)) return 0; uint32_t v = r.byte(pos) | (r.byte(pos + 1) << 8); pos += 2; return v; }
	CRT_HD uint32_t u32() {
		if(!need(4)) return 0;
		uint32_t v = r.byte(pos) | (r.byte(pos + 1) << 8) | (r.byte(pos + 2) << 16) | (r.byte(pos + 3) << 24);
		pos += 4; return v;
	}
	CRT_HD void str(uint32_t &off, uint32_t &slen) {     // u16 count incl. NUL + bytes; the string ends at the first NUL
		off = 0; slen = 0;
		uint32_t n = u16();
		if(!need(n)) return;
		off = pos;
		while(slen < n && r.byte(pos + slen)) slen++;
		pos += n;
	}
	CRT_HD bool skip(uint64_t n) { if(!need(n)) return false; pos += (uint32_t)n; return true; }
};

// record space, handed out front to back; once something does not fit, nothing more is written
struct WalkOut {
	uint8_t *rec; uint32_t cap, off; bool overflow;
	CRT_HD uint8_t *take(uint32_t bytes) {
		if(overflow || bytes > cap - off) { overflow = true; return nullptr; }
		uint8_t *p = rec + off; off += bytes; return p;
	}
};

// std::string's operator< on two names of the blob (unsigned bytes, a prefix first)
template <class R> CRT_HD inline int walk_name_cmp(R &r, const WalkAttr &a, uint32_t off, uint32_t len) {
	const uint32_t n = a.name_len < len ? a.name_len : len;
	for(uint32_t k = 0; k < n; k++) {
		const uint32_t x = r.byte(a.name_off + k), y = r.byte(off + k);
		if(x != y) return x < y ? -1 : 1;
	}
	return a.name_len < len ? -1 : a.name_len > len ? 1 : 0;
}

// "BITS" block (crt_format.cpp: bits_block)
template <class R> CRT_HD inline void walk_bits(WalkCursor<R> &c, uint32_t &off, uint32_t &nwords) {
	nwords = c.u32();
	const uint32_t pad = c.pos & 3;
	if(pad) c.skip(4 - pad);
	off = c.pos;
	c.skip((uint64_t)nwords * 4);
}

// entropy-coded byte array (crt_format.cpp: byte_block), written to the record when there is room
template <class R> CRT_HD inline void walk_stream(WalkCursor<R> &c, uint32_t entropy, int &err, WalkOut &out) {
	WalkStream s = {STREAM_EMPTY, 0, 0, 255, 0, 0, 0, 0, 0};
	uint32_t nsym = 0;
	if(entropy == CRTHIP_ENTROPY_NONE) {
		s.size = s.csize = c.u32();
		s.payload_off = c.pos;
		c.skip(s.size);
		s.mode = s.size ? STREAM_RAW : STREAM_EMPTY;
		if(!s.size) s.max_sym = 0;
	} else if(entropy != CRTHIP_ENTROPY_TUNSTALL) {
		err = CRTHIP_E_ENTROPY;
	} else {
		nsym = c.u8();
		s.nsym = (uint8_t)nsym;
		s.probs_off = c.pos;
		const bool have = c.need((uint64_t)nsym * 2);
		if(have && nsym >= 1) {
			s.fill = (uint8_t)c.r.byte(c.pos);
			uint32_t m = 0;
			for(uint32_t k = 0; k < nsym; k++) { const uint32_t v = c.r.byte(c.pos + 2*k); m = v > m ? v : m; }
			s.max_sym = (uint8_t)m;
		}
		if(have && nsym >= 2 && nsym <= 16) s.nprobs = nsym*2;
		c.skip((uint64_t)nsym * 2);
		s.size = c.u32();
		s.csize = c.u32();
		s.payload_off = c.pos;
		c.skip(s.csize);
		if(s.size == 0) s.mode = STREAM_EMPTY;
		else if(nsym == 1) s.mode = STREAM_FILL;
		else if(nsym == 0 || s.csize == 0) { s.mode = STREAM_EMPTY; err = err ? err : CRTHIP_E_TRUNCATED; }
		else s.mode = STREAM_TUNSTALL;
	}
	uint8_t *p = out.take((uint32_t)sizeof(WalkStream) + ((s.nprobs + 3) & ~3u));
	if(!p) return;
	*(WalkStream *)p = s;
	for(uint32_t k = 0; k < s.nprobs; k++) p[sizeof(WalkStream) + k] = (uint8_t)c.r.byte(s.probs_off + k);
}

// One blob: returns its status; rec[0, rec_cap) receives the record (rec 16-byte aligned, rec_cap a multiple of 16, >= 64).
template <class R> CRT_HD inline int walk_record(const R &reader, uint32_t len, uint8_t *rec, uint32_t rec_cap, WalkWork &w) {
	WalkCursor<R> c(reader, len);
	WalkHead h = {};
	WalkOut out = {rec, rec_cap, (uint32_t)sizeof(WalkHead), false};
	int err = CRTHIP_OK;
	uint32_t nattr = 0, nface = 0, entropy = 0;
	// ---- header (crt_format.cpp: header)
	if(c.u32() != 0x787A6300u || c.bad) { err = CRTHIP_E_MAGIC; goto done; }
	c.u32();                                                  // version
	entropy = c.u8();
	{
		const uint32_t nexif = c.u32();
		for(uint32_t i = 0; i < nexif && !c.bad; i++) { uint32_t o, l; c.str(o, l); c.str(o, l); }
		const uint32_t nraw = c.u32();
		bool limit = false;                                   // a 17th distinct name, or a name of CRTHIP_NAME_MAX bytes or more
		for(uint32_t i = 0; i < nraw && !c.bad; i++) {
			WalkAttr a;
			c.str(a.name_off, a.name_len);
			a.codec = c.u32(); c.u32(); a.N = c.u8(); c.u8(); a.strategy = c.u8();
			if(a.codec != CRTHIP_CODEC_NORMAL && a.codec != CRTHIP_CODEC_COLOR) a.codec = CRTHIP_CODEC_GENERIC;
			if(c.bad || limit) continue;
			if(a.name_len >= CRTHIP_NAME_MAX) { limit = true; continue; }   // stays in the map whatever follows: CRTHIP_E_LIMIT
			uint32_t k = 0;
			int cmp = -1;
			while(k < nattr && (cmp = walk_name_cmp(c.r, w.attr[k], a.name_off, a.name_len)) < 0) k++;
			if(k < nattr && cmp == 0) { w.attr[k] = a; continue; }           // std::map: the last one of a name wins
			if(nattr == CRTHIP_MAX_ATTRS) { limit = true; continue; }
			for(uint32_t j = nattr; j > k; j--) w.attr[j] = w.attr[j - 1];
			w.attr[k] = a; nattr++;
		}
		c.u32();                                              // nvert
		nface = c.u32();
		if(c.bad) { err = CRTHIP_E_TRUNCATED; goto done; }
		if(limit) { err = CRTHIP_E_LIMIT; goto done; }
	}
	// ---- groups (crt_format.cpp: groups)
	{
		const uint32_t ngroups = c.u32();
		if(!c.need((uint64_t)ngroups * 5)) { err = CRTHIP_E_TRUNCATED; goto done; }
		for(uint32_t g = 0; g < ngroups && !c.bad; g++) {
			c.u32();
			const uint32_t np = c.u8();
			for(uint32_t k = 0; k < np && !c.bad; k++) { uint32_t o, l; c.str(o, l); c.str(o, l); }
		}
	}
	h.prefix_len = c.pos;
	if(!c.bad) {
		uint8_t *p = out.take((c.pos + 15) & ~15u);
		if(p) c.r.copy(p, c.pos);
	}
	h.items_off = out.off;
	// ---- index block
	if(nface > 0) {
		h.max_front = c.u32();
		walk_stream(c, entropy, err, out);
		walk_bits(c, h.split_off, h.split_nwords);
	}
	// ---- attribute blocks, in name order
	for(uint32_t i = 0; i < nattr && !c.bad && !err; i++) {
		const WalkAttr &a = w.attr[i];
		WalkAttrItem it = {0, 0, 1, 0, {4, 4, 4, 8}, {0, 0, 0}};
		uint8_t *slot = out.take((uint32_t)sizeof(WalkAttrItem));
		if(a.codec == CRTHIP_CODEC_NORMAL) {
			it.normal_prediction = (uint8_t)c.u8();
			walk_bits(c, it.bits_off, it.bits_nwords);
			walk_stream(c, entropy, err, out);
		} else if(a.codec == CRTHIP_CODEC_COLOR) {
			for(uint32_t k = 0; k < a.N; k++) { const uint32_t q = c.u8(); if(k < 4) it.qc[k] = (uint8_t)q; }
			walk_bits(c, it.bits_off, it.bits_nwords);
			it.nlogs = a.N;
			for(uint32_t k = 0; k < a.N; k++) walk_stream(c, entropy, err, out);
		} else if(a.strategy & CRTHIP_CORRELATED) {
			walk_bits(c, it.bits_off, it.bits_nwords);
			walk_stream(c, entropy, err, out);
		} else {
			walk_bits(c, it.bits_off, it.bits_nwords);
			it.nlogs = a.N;
			for(uint32_t k = 0; k < a.N; k++) walk_stream(c, entropy, err, out);
		}
		if(slot) *(WalkAttrItem *)slot = it;
	}
	if(!err && c.bad) err = CRTHIP_E_TRUNCATED;
	h.end_offset = c.pos;
	h.items_len = out.off - h.items_off;
	h.nattr = nattr;
	h.flags = out.overflow ? WALK_OVERFLOW : 0u;
done:
	h.status = err;
	if(err) h.flags = 0;
	*(WalkHead *)rec = h;
	return err;
}

} // namespace corto_hip
