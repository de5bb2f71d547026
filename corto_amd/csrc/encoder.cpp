// encoder.cpp — host-side .crt writer: lets tests and bench.py synthesise inputs on the GPU
// box without the reference library.  Byte-identical to upstream's crt::Encoder for the attribute set the decoder path
// covers (positions, normals in all three prediction modes, rgb/rgba colours, uvs, one generic "radius" attribute,
// generic attributes of any name, 1..16 components, either strategy bit and FLOAT / DOUBLE / INT32 / INT16 / INT8 input
// (Encoder::addAttribute, crthip_encode_attrs), groups, exif, entropy NONE/TUNSTALL, meshes and point clouds);
// tests/test_encoder_cpu.py and tests/test_encode_generic_cpu.py pin that against the reference-made golden blobs and, where
// oracle/_ref exists, against the reference on a random corpus.
//
// What it restates (upstream file:line):
//   container + stage order   src/encoder.cpp:207-296 (encode, encodePointCloud), :311-381 (encodeMesh)
//   quantisation              src/encoder.cpp:49-100, include/corto/vertex_attribute.h:79-128, src/normal_attribute.cpp:61-111,
//                             src/color_attribute.cpp:23-70
//   value coding              include/corto/cstream.h:105-204 (needed, encodeValues, encodeArray), src/bitstream.cpp:86-101,123-129
//   Tunstall                  src/tunstall.cpp:83-115 (getProbabilities), :125-256 (dictionary), :335-428 (encoding trie, compress),
//                             src/cstream.cpp:89-109 (block framing)
//   topology                  src/encoder.cpp:383-504 (buildTopology), :522-722 (encodeFaces)
//   normals                   src/normal_attribute.cpp:113-176 (preDelta, deltaEncode, encode)
// Where the reference's output depends on std::sort's handling of ties (probability order, edge buckets, Morton order)
// the same std::sort call on the same element sequence is made, which reproduces it exactly.
#include <cfloat>
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <map>
#include <new>
#include <string>
#include <vector>

#include "../../include/corto_hip.h"
#include "encoder_internal.h"
#include "device_plan.h"
#include "enc_splice.h"
#include "enc_topology.h"

using corto_hip::QK_FLOAT;
using corto_hip::QK_NORMAL;
using corto_hip::QK_COLOR;
using corto_hip::QK_INT;
using corto_hip::QK_DOUBLE;

namespace {

int ilog2u(uint64_t p) { int k = 0; while(p >>= 1) ++k; return k; }                  // src/cstream.cpp:31-35

int32_t f2i(float x) {                                                                 // x86 cvttss2si
	if(!(x > -2147483904.0f && x < 2147483648.0f)) return INT_MIN;
	return (int32_t)x;
}

int32_t d2i(double x) {                                                                // x86 cvttsd2si
	if(!(x > -2147483649.0 && x < 2147483648.0)) return INT_MIN;
	return (int32_t)x;
}

// ---- streams left to the device (crthip_encode_gpu): recorded instead of written, spliced in at `at` afterwards ----
struct Deferred : corto_hip::BatchStream {   // at: position in the sink's bytes where the stream belongs; kind: CRTHIP_ENC_*, or BATCH_BITS
                                             // for a bit stream that is already packed (CLERS split bits); count, N
	std::vector<uint8_t> bytes;         // symbols / int8 values
	std::vector<int32_t> ints;          // int32 values
	std::vector<uint32_t> words;        // BATCH_BITS
};

// ---- byte sink (OutStream, include/corto/cstream.h:42-105) ----
struct Sink {
	std::vector<uint8_t> b;
	std::vector<Deferred> *defer = nullptr;   // non-null: value / symbol / bit streams are recorded, not written
	bool shape_only = false;                  // (crthip_encode_batch) ... and only their kind and size: the values live on the device
	struct Block { size_t at, head, payload; };
	std::vector<Block> *blocks = nullptr;     // non-null: where every entropy-coded block lies in b, and where its header ends (encode_host_coded)
	void u8(uint32_t v) { b.push_back((uint8_t)v); }
	void u16(uint32_t v) { u8(v); u8(v >> 8); }
	void u32(uint32_t v) { u8(v); u8(v >> 8); u8(v >> 16); u8(v >> 24); }
	void f32(float f) { uint32_t u; memcpy(&u, &f, 4); u32(u); }
	void str(const std::string &s) { u16((uint32_t)s.size() + 1); b.insert(b.end(), s.begin(), s.end()); u8(0); }
	void raw(const void *p, size_t n) { const uint8_t *q = (const uint8_t *)p; b.insert(b.end(), q, q + n); }
};

// ---- MSB-first bit writer over u32 words (src/bitstream.cpp:86-101, 123-129) ----
struct BitWriter {
	std::vector<uint32_t> words;
	uint32_t buff = 0;
	int bits = 32;                      // free bits in buff
	void write(uint32_t value, int n) {
		if(n >= bits) {
			buff = (bits == 32 ? 0u : (buff << bits)) | (value >> (n - bits));
			words.push_back(buff);
			const int rest = n - bits;
			value &= rest >= 32 ? 0xFFFFFFFFu : ((1u << rest) - 1u);
			n = rest; bits = 32; buff = 0;
		}
		if(n > 0) { buff = (buff << n) | value; bits -= n; }
	}
	void flush() { if(bits != 32) { words.push_back(buff << bits); buff = 0; bits = 32; } }
	void emit(Sink &s) {                // OutStream::write(BitStream&), cstream.h:79-89
		flush();
		if(s.defer) { Deferred d; d.at = s.b.size(); d.kind = corto_hip::BATCH_BITS; d.words = words; s.defer->push_back(std::move(d)); return; }
		s.u32((uint32_t)words.size());
		while(s.b.size() & 3) s.u8(0);
		for(uint32_t w : words) s.u32(w);
	}
};

// ---- Tunstall encoder ----
struct Sym { uint8_t symbol, probability; };

struct Tunstall {
	std::vector<Sym> probs;
	std::vector<int> index, lengths;    // 256 words after build()
	std::vector<uint8_t> table;
	std::vector<int> offsets;           // 2-symbol-step trie (createEncodingTables)
	std::vector<uint8_t> remap;

	void probabilities(const uint8_t *data, int size) {                               // tunstall.cpp:83-115
		std::vector<int> cnt(256, 0);
		for(int i = 0; i < size; i++) cnt[data[i]]++;
		from_counts(cnt, size);
	}
	void from_counts(const std::vector<int> &cnt, int size) {
		probs.clear();
		for(int i = 0; i < 256; i++) if(cnt[i] > 0) probs.push_back(Sym{(uint8_t)i, (uint8_t)(cnt[i]*255/size)});
		std::sort(probs.begin(), probs.end(), [](const Sym &a, const Sym &b) -> bool { return a.probability > b.probability; });
	}

	void build() {                                                                     // tunstall.cpp:125-256
		const uint32_t n = (uint32_t)probs.size();
		if(n <= 1) return;
		std::vector<uint32_t> q(1024, 0), head(n);
		index.assign(1024, 0); lengths.assign(1024, 0);
		table.assign(8192 + 1024, 0);
		std::vector<uint32_t> P(n);
		for(uint32_t i = 0; i < n; i++) P[i] = (uint32_t)probs[i].probability << 8;
		uint32_t count = 2, run = (P[0]*P[0]) >> 16, max_count = 255/(n - 1), pos = 0, end = 0, nwords = 0;
		while(run > P[1] && count < max_count) { run = (run*P[0]) >> 16; count++; }
		if(count >= 16) {
			table[pos++] = probs[0].symbol;
			for(uint32_t k = 1; k < n; k++) { for(uint32_t i = 0; i + 1 < count; i++) table[pos++] = probs[0].symbol; table[pos++] = probs[k].symbol; }
			head[0] = (count - 1)*n;
			for(uint32_t k = 1; k < n; k++) head[k] = k;
			uint32_t pw = 0;
			for(uint32_t col = 0; col < count; col++) {
				for(uint32_t row = 1; row < n; row++) {
					const uint32_t e = row + col*n;
					q[e] = col == 0 ? P[row] : (pw*P[row]) >> 16;
					index[e] = (int)(row*count - col); lengths[e] = (int)(col + 1);
				}
				pw = col == 0 ? P[0] : (pw*P[0]) >> 16;
			}
			const uint32_t first = (count - 1)*n;
			q[first] = pw; index[first] = 0; lengths[first] = (int)count;
			nwords = 1 + count*(n - 1); end = count*n;
		} else {
			for(uint32_t i = 0; i < n; i++) { head[i] = i; q[end] = P[i]; index[end] = (int)pos; lengths[end] = 1; end++; table[pos++] = probs[i].symbol; }
			nwords = n;
		}
		while(nwords < 256) {
			uint32_t best = 0, maxp = 0;
			for(uint32_t i = 0; i < n; i++) { const uint32_t p = head[i] < q.size() ? q[head[i]] : 0; if(p > maxp) { best = i; maxp = p; } }
			const uint32_t parent = head[best], pp = q[parent], po = (uint32_t)index[parent], pl = (uint32_t)lengths[parent];
			uint32_t r = 0;
			for(; r < n; r++) {
				q[end] = (pp*P[r]) >> 16; index[end] = (int)pos; lengths[end] = (int)pl + 1; end++;
				memmove(&table[pos], &table[po], pl); pos += pl;
				table[pos++] = probs[r].symbol;
				if(nwords + r == 255) break;
			}
			if(r == n) head[best] += n;
			nwords += n - 1;
		}
		size_t w = 0;
		for(size_t e = 0; e < end && w < 256; e++) { if(head[e % n] > e) continue; index[w] = index[e]; lengths[w] = lengths[e]; w++; }
		index.resize(256); lengths.resize(256);
	}

	void code(const uint8_t *w, int length, int &low, int &high) const {              // wordCode, tunstall.h:117-132 (lookup_size 2)
		const int n = (int)probs.size();
		int c = 0;
		for(int i = 0; i < length && i < 2; i++) c = c*n + remap[w[i]];
		low = c; high = c + 1;
		for(int i = length; i < 2; i++) { low *= n; high *= n; }
	}

	void trie() {                                                                      // createEncodingTables, tunstall.cpp:335-382
		const int n = (int)probs.size();
		if(n <= 1) return;
		const int span = n*n;
		remap.assign(256, 0);
		for(int i = 0; i < n; i++) remap[probs[i].symbol] = (uint8_t)i;
		offsets.assign(span, 0xffffff);
		for(size_t i = 0; i < index.size(); i++) {
			int low, high, off = 0, toff = 0;
			for(;;) {
				code(&table[index[i] + off], lengths[i] - off, low, high);
				if(lengths[i] - off <= 2) { for(int k = low; k < high; k++) offsets[toff + k] = (int)i; break; }
				const int w = offsets[toff + low];
				if(w >= 0) { offsets[toff + low] = -(int)offsets.size(); offsets.resize(offsets.size() + span, w); }
				toff = -offsets[toff + low];
				off += 2;
			}
		}
	}

	std::vector<uint8_t> compress(const uint8_t *data, int size) const {               // tunstall.cpp:384-428
		std::vector<uint8_t> out;
		if(probs.size() == 1) return out;
		int in = 0, woff = 0, off = 0;
		while(in < size) {
			const int d = std::min(size - in, 2);
			int low, high;
			code(data + in, d, low, high);
			off = offsets[-off + low];
			if(off >= 0) { out.push_back((uint8_t)off); in += lengths[off] - woff; off = 0; woff = 0; }
			else { woff += 2; in += 2; }
		}
		if(off < 0) { while(off < 0) off = offsets[-off]; out.push_back((uint8_t)off); }
		return out;
	}
};

// entropy-coded byte array (OutStream::compress / tunstall_compress, cstream.cpp:43-64, 89-109)
void put_symbols(Sink &s, uint32_t entropy, const uint8_t *data, uint32_t size) {
	if(s.defer) { Deferred d; d.at = s.b.size(); d.kind = CRTHIP_ENC_SYMBOLS; d.count = size; if(!s.shape_only) d.bytes.assign(data, data + size); s.defer->push_back(std::move(d)); return; }
	const size_t at = s.b.size();
	if(entropy == CRTHIP_ENTROPY_NONE) { s.u32(size); if(s.blocks) s.blocks->push_back({at, 4, size}); s.raw(data, size); return; }
	Tunstall t;
	t.probabilities(data, (int)size);
	t.build();
	t.trie();
	const std::vector<uint8_t> c = t.compress(data, (int)size);
	s.u8((uint32_t)t.probs.size());
	for(const Sym &p : t.probs) { s.u8(p.symbol); s.u8(p.probability); }
	s.u32(size);
	s.u32((uint32_t)c.size());
	if(s.blocks) s.blocks->push_back({at, s.b.size() - at, c.size()});
	s.raw(c.data(), c.size());
}

int needed(int a) {                                                                    // cstream.h:105-112
	if(a == 0) return 0;
	if(a == -1) return 1;
	if(a < 0) a = -a - 1;
	int n = 2;
	while(a >>= 1) n++;
	return n;
}

// encodeValues (cstream.h:115-141): component-major logs, sign folding
template <class T> void put_values(Sink &s, uint32_t entropy, uint32_t size, const T *values, int N) {
	if(s.defer) {
		Deferred d; d.at = s.b.size(); d.count = size; d.N = (uint32_t)N;
		if(sizeof(T) == 1) { d.kind = CRTHIP_ENC_VALUES_I8; if(!s.shape_only) d.bytes.assign((const uint8_t *)values, (const uint8_t *)values + (size_t)size*N); }
		else { d.kind = CRTHIP_ENC_VALUES_I32; if(!s.shape_only) d.ints.assign((const int32_t *)values, (const int32_t *)values + (size_t)size*N); }
		s.defer->push_back(std::move(d)); return;
	}
	BitWriter bw;
	std::vector<std::vector<uint8_t>> logs((size_t)N, std::vector<uint8_t>(size));
	for(int c = 0; c < N; c++) for(uint32_t i = 0; i < size; i++) {
		int val = values[(size_t)i*N + c];
		if(val == 0) { logs[c][i] = 0; continue; }
		const int ret = ilog2u((uint64_t)std::abs(val)) + 1;
		logs[c][i] = (uint8_t)ret;
		const int middle = (1 << ret) >> 1;
		if(val < 0) val = -val - middle;
		bw.write((uint32_t)val, ret);
	}
	bw.emit(s);
	for(int c = 0; c < N; c++) put_symbols(s, entropy, logs[c].data(), size);
}

// encodeArray (cstream.h:143-164): one log per element
void put_array(Sink &s, uint32_t entropy, uint32_t size, const int32_t *values, int N) {
	if(s.defer) { Deferred d; d.at = s.b.size(); d.kind = CRTHIP_ENC_ARRAY; d.count = size; d.N = (uint32_t)N; if(!s.shape_only) d.ints.assign(values, values + (size_t)size*N); s.defer->push_back(std::move(d)); return; }
	BitWriter bw;
	std::vector<uint8_t> logs(size);
	for(uint32_t i = 0; i < size; i++) {
		const int32_t *p = values + (size_t)i*N;
		int diff = needed(p[0]);
		for(int c = 1; c < N; c++) diff = std::max(diff, needed(p[c]));
		logs[i] = (uint8_t)diff;
		if(diff == 0) continue;
		const int mx = 1 << (diff - 1);
		for(int c = 0; c < N; c++) bw.write((uint32_t)(p[c] + mx), diff);
	}
	bw.emit(s);
	put_symbols(s, entropy, logs.data(), size);
}

struct Quad { uint32_t t, a, b, c; };

// normals: octahedral map (include/corto/normal_attribute.h:75-85)
void to_octa(const float v[3], int unit, int32_t o[2]) {
	float s = std::fabs(v[0]) + std::fabs(v[1]); s = s + std::fabs(v[2]);
	float px = v[0]/s, py = v[1]/s;
	if(v[2] < 0) {
		const float qx = 1.0f - std::fabs(py), qy = 1.0f - std::fabs(px);
		px = qx; py = qy;
		if(v[0] < 0) px = -px;
		if(v[1] < 0) py = -py;
	}
	o[0] = f2i(px*(float)unit); o[1] = f2i(py*(float)unit);
}

struct Attr {
	std::string name;
	int codec = CRTHIP_CODEC_GENERIC, N = 0, format = CRTHIP_FMT_FLOAT, strategy = 0;
	float q = 0;
	std::vector<int32_t> values, diffs;        // generic + normal (normal: 2 per vertex)
	std::vector<uint8_t> cvalues, cdiffs;      // colour
	int qc[4] = {4, 4, 4, 8};
	int prediction = 0;                        // normals
	std::vector<int32_t> boundary;
};

// ---- face adjacency: every directed side of a triangle is a HALF-EDGE, id 3*face + side, side s running opposite corner s
// (side 0 = corners 1->2, side 1 = 2->0, side 2 = 0->1); twin[h] = the half-edge of the neighbouring face running the other way
// along the same two vertices, or NO_TWIN.  Same result as upstream's buildTopology (src/encoder.cpp:450-504) - including on
// non-manifold input, where WHICH two of several candidates get paired depends on the order std::sort leaves equal keys in:
// so the half-edges are bucketed by their smaller vertex in the same order, and every bucket goes through std::sort with an
// equivalent strict-weak order on (smaller vertex, larger vertex).  std::sort's permutation is a function of the comparison
// results alone, so a different element type does not change it.
constexpr uint32_t NO_TWIN = 0xffffffffu;
struct SideKey {
	uint32_t lo, hi;        // the side's two vertices, lo < hi
	uint32_t half;          // 3*face + side
	uint32_t flipped;       // the side runs hi -> lo
	bool operator<(const SideKey &o) const { return lo != o.lo ? lo < o.lo : hi < o.hi; }
};

static void pair_half_edges(const uint32_t *corner, size_t ntri, uint32_t nvert, std::vector<uint32_t> &twin) {
	twin.assign(ntri*3, NO_TWIN);
	// bucket b = sides whose smaller vertex is b, filled face by face, side 0, 1, 2
	std::vector<uint32_t> fill(nvert + 1, 0);
	auto ends = [&](size_t t, int side, uint32_t &from, uint32_t &to) { from = corner[3*t + (side + 1)%3]; to = corner[3*t + (side + 2)%3]; };
	for(size_t t = 0; t < ntri; t++)
		for(int side = 0; side < 3; side++) { uint32_t a, b; ends(t, side, a, b); fill[std::min(a, b) + 1]++; }
	for(uint32_t v = 0; v < nvert; v++) fill[v + 1] += fill[v];
	std::vector<uint32_t> first(fill.begin(), fill.end() - 1);              // bucket starts (fill[] becomes the write cursors)
	std::vector<SideKey> sides(ntri*3);
	for(size_t t = 0; t < ntri; t++)
		for(int side = 0; side < 3; side++) {
			uint32_t a, b; ends(t, side, a, b);
			SideKey k; k.lo = std::min(a, b); k.hi = std::max(a, b); k.half = (uint32_t)(3*t + side); k.flipped = a > b;
			sides[fill[k.lo]++] = k;
		}
	// (upstream skips every bucket after the first that starts at offset 0 - i.e. while no smaller vertex had a side of its own,
	// src/encoder.cpp:481-485 - so the sides of the first non-empty bucket stay unsorted, and pair only where they happen to lie
	// next to each other, when vertex 0 is not the smaller end of any side; byte identity needs the same)
	for(uint32_t v = 0; v < nvert; v++) { if(v > 0 && first[v] == 0) continue; std::sort(sides.begin() + first[v], sides.begin() + fill[v]); }
	// a side pairs with the candidate kept from before it when they run opposite ways along the same vertices and neither has a
	// twin yet; any side that does not pair becomes the candidate
	const SideKey *cand = nullptr;
	for(const SideKey &k : sides) {
		if(cand && cand->lo == k.lo && cand->hi == k.hi && cand->flipped != k.flipped) {
			if(twin[k.half] == NO_TWIN && twin[cand->half] == NO_TWIN) { twin[k.half] = cand->half; twin[cand->half] = k.half; }
		} else cand = &k;
	}
}

enum { VERTEX = 0, LEFT = 1, RIGHT = 2, END = 3, BOUNDARY = 4, DELAY = 5, SPLIT = 6 };

struct Encoder {
	uint32_t nvert, nface, entropy;
	std::vector<uint32_t> faces;                 // original indexing, degenerate faces removed in encode_mesh
	std::vector<uint32_t> group_end;
	std::vector<std::map<std::string, std::string>> group_props;
	std::map<std::string, std::string> exif;
	std::map<std::string, Attr> data;            // std::map: alphabetical like upstream
	std::vector<uint8_t> clers;
	BitWriter split;
	uint32_t max_front = 0, current_vertex = 0, last_index = 0;
	std::vector<int> encoded;
	std::vector<Quad> prediction;
	Sink s;

	// The CLERS writer for faces [start, end) (one group): the region-growing walk of upstream's encodeFaces (src/encoder.cpp:522-722)
	// - same symbols, same split / vertex-id bits, same vertex numbering and parallelogram corners - on this repo's own terms:
	// the advancing front is a circular list threaded THROUGH the half-edges (a half-edge joins the front at most once, so
	// before[] / after[] / where[] are indexed by half-edge id and there is no separate edge store), gates wait in a FIFO of
	// half-edge ids, postponed ones on a stack.
	void encode_faces(int start, int end) {
		const size_t ntri = (size_t)(end - start);
		const uint32_t *corner = faces.data() + (size_t)start*3;
		std::vector<uint32_t> twin;
		pair_half_edges(corner, ntri, nvert, twin);

		enum : uint8_t { OFF_FRONT = 0, ON_FRONT = 1, CLOSED = 2 };
		std::vector<uint8_t> where(ntri*3, OFF_FRONT);                    // a half-edge's life: not reached / on the front / swallowed by a later face
		std::vector<uint32_t> before(ntri*3, 0), after(ntri*3, 0);        // its neighbours along the front
		std::vector<uint8_t> coded(ntri, 0);                              // faces already written
		std::vector<uint32_t> gates, postponed;
		size_t gate_cursor = 0, seed_cursor = 0, remaining = ntri;
		uint32_t joined = 0;                                              // half-edges that ever joined the front (upstream's front.size())
		uint32_t pending = NO_TWIN;                                       // the front edge the previous step made: always the next gate

		std::vector<uint8_t> used(nvert, 0);
		for(uint32_t v : faces) used[v] = 1;
		uint32_t nused = 0; for(uint8_t u : used) nused += u;
		const int idbits = ilog2u(nused) + 1;                              // bits of a known vertex's number in the split stream

		auto onto_front = [&](uint32_t h, uint32_t p, uint32_t n) { where[h] = ON_FRONT; before[h] = p; after[h] = n; joined++; };
		auto introduce = [&](uint32_t v, uint32_t a, uint32_t b, uint32_t c) {      // a vertex seen for the first time gets the next number
			prediction[current_vertex] = Quad{v, a, b, c};
			encoded[v] = (int)current_vertex++;
			last_index = v;
		};
		auto mention = [&](uint32_t v) { split.write((uint32_t)encoded[v], idbits); };

		while(remaining) {
			uint32_t gate;
			if(pending != NO_TWIN) { gate = pending; pending = NO_TWIN; }
			else if(gate_cursor < gates.size()) gate = gates[gate_cursor++];
			else if(!postponed.empty()) { gate = postponed.back(); postponed.pop_back(); }
			else {
				// nothing left to grow from: start a new component with the first face not written yet
				while(seed_cursor < ntri && coded[seed_cursor]) seed_cursor++;
				if(seed_cursor == ntri) break;
				const uint32_t t = (uint32_t)seed_cursor;
				const uint32_t *c3 = corner + 3*(size_t)t;
				uint32_t known = 0;
				for(int k = 0; k < 3; k++) if(encoded[c3[k]] != -1) known |= 1u << k;
				if(known) { clers.push_back(SPLIT); split.write(known, 3); } else clers.push_back(VERTEX);
				for(int k = 0; k < 3; k++) {
					if(encoded[c3[k]] != -1) mention(c3[k]);
					else introduce(c3[k], last_index, last_index, last_index);
				}
				const uint32_t h = 3*t;                                      // its three sides circle the face: side 0 -> 1 -> 2 -> 0
				onto_front(h, h + 2, h + 1); onto_front(h + 1, h, h + 2); onto_front(h + 2, h + 1, h);
				gates.push_back(h); gates.push_back(h + 1); gates.push_back(h + 2);
				coded[t] = 1; remaining--;
				continue;
			}
			if(where[gate] == CLOSED) continue;
			const uint32_t tw = twin[gate];
			if(tw == NO_TWIN || coded[tw/3]) { clers.push_back(BOUNDARY); continue; }
			const uint32_t across = tw/3;                                    // the face on the other side of the gate
			const uint32_t s_far = tw%3, s_a = (s_far + 1)%3, s_b = (s_a + 1)%3;   // its corner opposite the gate, then the gate's two ends
			const uint32_t left = before[gate], right = after[gate];
			const bool zip_left = twin[left] != NO_TWIN && twin[left]/3 == across;
			const bool zip_right = twin[right] != NO_TWIN && twin[right]/3 == across;
			const uint32_t h_a = 3*across + s_a, h_b = 3*across + s_b;       // the two sides of `across` that may join the front
			if(zip_left && zip_right) {                                      // the face closes a triangular hole
				clers.push_back(END);
				const uint32_t ll = before[left], rr = after[right];
				where[left] = CLOSED; where[right] = CLOSED;
				after[ll] = rr; before[rr] = ll;
			} else if(zip_left) {
				clers.push_back(LEFT);
				const uint32_t ll = before[left];
				where[left] = CLOSED;
				onto_front(h_b, ll, right);
				after[ll] = h_b; before[right] = h_b;
				pending = h_b;
			} else if(zip_right) {
				clers.push_back(RIGHT);
				const uint32_t rr = after[right];
				where[right] = CLOSED;
				onto_front(h_a, left, rr);
				before[rr] = h_a; after[left] = h_a;
				pending = h_a;
			} else {
				const uint32_t far = corner[3*(size_t)across + s_far];
				if(encoded[far] != -1 && gate_cursor < gates.size()) {          // a known vertex while gates are still waiting: come back to this one later
					postponed.push_back(gate); clers.push_back(DELAY);
					continue;
				}
				if(encoded[far] != -1) { clers.push_back(SPLIT); mention(far); }
				else {
					clers.push_back(VERTEX);
					// parallelogram corners: the gate's two ends and the corner of the gate's own face opposite it
					introduce(far, corner[3*(size_t)across + s_a], corner[3*(size_t)across + s_b], corner[gate]);
				}
				onto_front(h_a, left, h_b); onto_front(h_b, h_a, right);
				after[left] = h_a; before[right] = h_b;
				gates.push_back(h_b);
				pending = h_a;
			}
			coded[across] = 1; remaining--;
		}
		max_front = std::max(max_front, joined);
	}

	// NormalAttr::preDelta (normal_attribute.cpp:113-143): uses ORIGINAL vertex ids and quantised positions
	void normal_predelta(Attr &a) {
		if(a.prediction == 0) return;
		auto it = data.find("position");
		const std::vector<int32_t> &coords = it->second.values;
		std::vector<float> est((size_t)nvert*3, 0.f);
		a.boundary.assign(nvert, 0);
		for(uint32_t f = 0; f < nface; f++) {
			const uint32_t i0 = faces[(size_t)f*3], i1 = faces[(size_t)f*3 + 1], i2 = faces[(size_t)f*3 + 2];
			const int32_t *p0 = &coords[(size_t)i0*3], *p1 = &coords[(size_t)i1*3], *p2 = &coords[(size_t)i2*3];
			const float ax = (float)p1[0] - (float)p0[0], ay = (float)p1[1] - (float)p0[1], az = (float)p1[2] - (float)p0[2];
			const float bx = (float)p2[0] - (float)p0[0], by = (float)p2[1] - (float)p0[1], bz = (float)p2[2] - (float)p0[2];
			const float n[3] = {ay*bz - az*by, az*bx - ax*bz, ax*by - ay*bx};
			for(int k = 0; k < 3; k++) est[(size_t)i0*3 + k] += n[k];
			for(int k = 0; k < 3; k++) est[(size_t)i1*3 + k] += n[k];
			for(int k = 0; k < 3; k++) est[(size_t)i2*3 + k] += n[k];
			if(a.prediction == 2) {
				a.boundary[i0] ^= (int32_t)i1; a.boundary[i0] ^= (int32_t)i2; a.boundary[i1] ^= (int32_t)i2;
				a.boundary[i1] ^= (int32_t)i0; a.boundary[i2] ^= (int32_t)i0; a.boundary[i2] ^= (int32_t)i1;
			}
		}
		const int unit = f2i(a.q);
		for(uint32_t i = 0; i < nvert; i++) {
			int32_t o[2]; to_octa(&est[(size_t)i*3], unit, o);
			a.values[(size_t)i*2] = (int32_t)((uint32_t)a.values[(size_t)i*2] - (uint32_t)o[0]);
			a.values[(size_t)i*2 + 1] = (int32_t)((uint32_t)a.values[(size_t)i*2 + 1] - (uint32_t)o[1]);
		}
	}

	void delta_encode(Attr &a) {
		const std::vector<Quad> &ctx = prediction;
		if(a.codec == CRTHIP_CODEC_NORMAL) {                                            // normal_attribute.cpp:145-176
			if(a.prediction == 0) {
				a.diffs.assign(ctx.size()*2, 0);
				if(ctx.empty()) return;
				a.diffs[0] = a.values[(size_t)ctx[0].t*2]; a.diffs[1] = a.values[(size_t)ctx[0].t*2 + 1];
				for(size_t i = 1; i < ctx.size(); i++) for(int c = 0; c < 2; c++)
					a.diffs[i*2 + c] = (int32_t)((uint32_t)a.values[(size_t)ctx[i].t*2 + c] - (uint32_t)a.values[(size_t)ctx[i].a*2 + c]);
			} else {
				a.diffs.clear();
				for(const Quad &q : ctx) if(a.prediction != 2 || a.boundary[q.t] != 0) { a.diffs.push_back(a.values[(size_t)q.t*2]); a.diffs.push_back(a.values[(size_t)q.t*2 + 1]); }
			}
			return;
		}
		const int N = a.N;
		if(a.codec == CRTHIP_CODEC_COLOR) {                                             // GenericAttr<uchar>::deltaEncode, strategy 0
			a.cdiffs.assign(ctx.size()*(size_t)N, 0);
			if(ctx.empty()) return;
			for(int c = 0; c < N; c++) a.cdiffs[c] = a.cvalues[(size_t)ctx[0].t*N + c];
			for(size_t i = 1; i < ctx.size(); i++) {
				const Quad &q = ctx[i];
				for(int c = 0; c < N; c++) {
					if(q.a != q.b && (a.strategy & CRTHIP_PARALLEL)) a.cdiffs[i*N + c] = (uint8_t)(a.cvalues[(size_t)q.t*N + c] - (a.cvalues[(size_t)q.a*N + c] + a.cvalues[(size_t)q.b*N + c] - a.cvalues[(size_t)q.c*N + c]));
					else a.cdiffs[i*N + c] = (uint8_t)(a.cvalues[(size_t)q.t*N + c] - a.cvalues[(size_t)q.a*N + c]);
				}
			}
			return;
		}
		a.diffs.assign(ctx.size()*(size_t)N, 0);                                        // vertex_attribute.h:130-144
		if(ctx.empty()) return;
		for(int c = 0; c < N; c++) a.diffs[c] = a.values[(size_t)ctx[0].t*N + c];
		for(size_t i = 1; i < ctx.size(); i++) {
			const Quad &q = ctx[i];
			for(int c = 0; c < N; c++) {
				const uint32_t t = (uint32_t)a.values[(size_t)q.t*N + c], va = (uint32_t)a.values[(size_t)q.a*N + c];
				if(q.a != q.b && (a.strategy & CRTHIP_PARALLEL)) a.diffs[i*N + c] = (int32_t)(t - (va + (uint32_t)a.values[(size_t)q.b*N + c] - (uint32_t)a.values[(size_t)q.c*N + c]));
				else a.diffs[i*N + c] = (int32_t)(t - va);
			}
		}
	}

	void attr_encode(Attr &a) {
		if(a.codec == CRTHIP_CODEC_NORMAL) { s.u8((uint32_t)a.prediction); put_array(s, entropy, (uint32_t)(a.diffs.size()/2), a.diffs.data(), 2); return; }
		if(a.codec == CRTHIP_CODEC_COLOR) {
			for(int c = 0; c < a.N; c++) s.u8((uint32_t)a.qc[c]);
			put_values<int8_t>(s, entropy, nvert, (const int8_t *)a.cdiffs.data(), a.N);
			return;
		}
		if(a.strategy & CRTHIP_CORRELATED) put_array(s, entropy, nvert, a.diffs.data(), a.N);
		else put_values<int32_t>(s, entropy, nvert, a.diffs.data(), a.N);
	}

	void header() {                                                                    // src/encoder.cpp:207-229
		s.u32(0x787A6300); s.u32(1); s.u8(entropy);
		s.u32((uint32_t)exif.size());
		for(auto &kv : exif) { s.str(kv.first); s.str(kv.second); }
		s.u32((uint32_t)data.size());
		for(auto &kv : data) { const Attr &a = kv.second; s.str(kv.first); s.u32((uint32_t)a.codec); s.f32(a.q); s.u8((uint32_t)a.N); s.u8((uint32_t)a.format); s.u8((uint32_t)a.strategy); }
	}

	// IndexAttribute::encodeGroups (include/corto/index_attribute.h:71-81): properties in std::map order = sorted by key
	void groups() {
		s.u32((uint32_t)group_end.size());
		for(size_t g = 0; g < group_end.size(); g++) {
			s.u32(group_end[g]);
			if(g < group_props.size()) {
				s.u8((uint8_t)group_props[g].size());
				for(auto &kv : group_props[g]) { s.str(kv.first); s.str(kv.second); }
			} else s.u8(0);
		}
	}

	// The topology pass (src/encoder.cpp:311-376 up to the attributes): degenerate faces dropped per group, the CLERS walk of every
	// group, split bits, max_front, the prediction quads and current_vertex.  Reads the index alone; nvert stays the input's.
	void topology() {
		encoded.assign(nvert, -1);
		if(group_end.empty()) group_end.push_back(nface);
		uint32_t start = 0, count = 0;
		for(uint32_t &g : group_end) {
			for(uint32_t i = start; i < g; i++) {
				const uint32_t *f = &faces[(size_t)i*3];
				if(f[0] == f[1] || f[0] == f[2] || f[1] == f[2]) continue;
				if(count != i) { faces[(size_t)count*3] = f[0]; faces[(size_t)count*3 + 1] = f[1]; faces[(size_t)count*3 + 2] = f[2]; }
				count++;
			}
			start = g; g = count;
		}
		faces.resize((size_t)count*3);
		nface = count;
		prediction.assign(nvert, Quad{0, 0, 0, 0});
		start = 0;
		for(uint32_t g : group_end) { encode_faces((int)start, (int)g); start = g; }
	}

	void encode_mesh() {                                                               // src/encoder.cpp:311-381
		topology();
		for(auto &kv : data) if(kv.second.codec == CRTHIP_CODEC_NORMAL) normal_predelta(kv.second);
		nvert = current_vertex;
		prediction.resize(nvert);
		for(auto &kv : data) delta_encode(kv.second);
		mesh_body();
	}

	// everything of a mesh after the header: counts, groups, CLERS, split bits, attributes
	void mesh_body() {
		s.u32(nvert); s.u32(nface);
		groups();
		s.u32(max_front);
		put_symbols(s, entropy, clers.data(), (uint32_t)clers.size());
		split.emit(s);
		for(auto &kv : data) attr_encode(kv.second);
	}

	void encode_cloud() {                                                              // src/encoder.cpp:238-296
		std::vector<uint32_t> order;
		corto_hip::morton_order_host(data.find("position")->second.values.data(), nvert, order);
		prediction.resize(nvert);
		if(nvert) prediction[0] = Quad{order[0], 0xffffffff, 0xffffffff, 0xffffffff};
		for(uint32_t i = 1; i < nvert; i++) prediction[i] = Quad{order[i], order[i - 1], order[i - 1], order[i - 1]};
		for(auto &kv : data) if(kv.second.codec == CRTHIP_CODEC_NORMAL) normal_predelta(kv.second);
		for(auto &kv : data) delta_encode(kv.second);
		cloud_body();
	}

	void cloud_body() {                                                                // (the sort and the residuals write nothing)
		s.u32(nvert); s.u32(0);
		groups();
		for(auto &kv : data) attr_encode(kv.second);
	}
};

struct ZPoint { uint64_t bits; uint32_t pos; bool operator<(const ZPoint &z) const { return bits > z.bits; } };

} // namespace

// Arguments are checked before anything is indexed with them (upstream trusts its caller: an index >= nvert writes past its
// vectors, src/encoder.cpp:341-347).
int corto_hip::encode_check(const crthip_mesh *m, bool index_on_host) {
	if(!m || !m->position) return corto_hip::ctx_fail(CRTHIP_E_ARGUMENT, "crthip_encode: no mesh / no positions");
	if(m->index && m->nface) {
		if((uint64_t)m->nface*3 > 0xFFFFFFFFull) return corto_hip::ctx_fail(CRTHIP_E_LIMIT, "crthip_encode: too many faces");
		if(index_on_host)                                           // (else the device compares them: k_encode_check.hip)
			for(size_t i = 0; i < (size_t)m->nface*3; i++)
				if(m->index[i] >= m->nvert) return corto_hip::ctx_fail(CRTHIP_E_ARGUMENT, "crthip_encode: face index out of range");
	}
	if(m->color) {
		if(m->color_components != 3 && m->color_components != 4) return corto_hip::ctx_fail(CRTHIP_E_ARGUMENT, "crthip_encode: color_components must be 3 or 4");
		for(int k = 0; k < m->color_components; k++)
			if(m->color_bits[k] < 1 || m->color_bits[k] > 8) return corto_hip::ctx_fail(CRTHIP_E_ARGUMENT, "crthip_encode: color_bits must be 1..8");
	}
	if(m->normal && (m->normal_bits < 1 || m->normal_bits > 16 || m->normal_prediction < 0 || m->normal_prediction > 2))
		return corto_hip::ctx_fail(CRTHIP_E_ARGUMENT, "crthip_encode: normal_bits must be 1..16, normal_prediction 0..2");
	if(m->position_bits > 31) return corto_hip::ctx_fail(CRTHIP_E_ARGUMENT, "crthip_encode: position_bits must be < 32");
	if(m->entropy != CRTHIP_ENTROPY_NONE && m->entropy != CRTHIP_ENTROPY_TUNSTALL) return corto_hip::ctx_fail(CRTHIP_E_ENTROPY, nullptr);
	if(m->ngroups) {
		if(!m->group_end || m->ngroups > (1u << 24)) return corto_hip::ctx_fail(CRTHIP_E_ARGUMENT, "crthip_encode: groups");
		uint32_t prev = 0;
		for(uint32_t g = 0; g < m->ngroups; g++) {
			// (a point cloud's group table is written as given and never used to index anything, src/encoder.cpp:238-296)
			if(m->group_end[g] < prev || (m->index && m->nface && m->group_end[g] > m->nface)) return corto_hip::ctx_fail(CRTHIP_E_ARGUMENT, "crthip_encode: group ends must be ascending and <= nface");
			prev = m->group_end[g];
			if(m->group_nprops && m->group_nprops[g] > 255) return corto_hip::ctx_fail(CRTHIP_E_LIMIT, "crthip_encode: more than 255 properties in a group");
		}
	}
	return CRTHIP_OK;
}

// crthip_encode_attrs's rules for the extra attributes (include/corto_hip.h).  Upstream throws "Unsupported format." for the unsigned
// formats (vertex_attribute.h:107) and silently drops an attribute whose name is taken (src/encoder.cpp:188); both are refused here.
int corto_hip::encode_check_attrs(const crthip_mesh *m, const crthip_attr_list *extra, bool device) {
	if(!extra || extra->nattr == 0) return CRTHIP_OK;
	if(!extra->attr) return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_encode_attrs: null attribute array");
	std::vector<std::string> taken{"position"};
	if(m->normal) taken.push_back("normal");
	if(m->color) taken.push_back("color");
	if(m->uv) taken.push_back("uv");
	if(m->radius) taken.push_back("radius");
	if((uint64_t)taken.size() + extra->nattr > CRTHIP_MAX_ATTRS) return ctx_fail(CRTHIP_E_LIMIT, "crthip_encode_attrs: more than CRTHIP_MAX_ATTRS attributes");
	for(uint32_t k = 0; k < extra->nattr; k++) {
		const crthip_generic_attr &g = extra->attr[k];
		if(!g.name) return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_encode_attrs: null name");
		const size_t len = strnlen(g.name, CRTHIP_NAME_MAX);
		if(len == 0 || len >= CRTHIP_NAME_MAX) return ctx_fail(CRTHIP_E_LIMIT, "crthip_encode_attrs: a name must have 1..63 bytes");
		if(g.format != CRTHIP_FMT_FLOAT && g.format != CRTHIP_FMT_DOUBLE && g.format != CRTHIP_FMT_INT32 && g.format != CRTHIP_FMT_INT16 && g.format != CRTHIP_FMT_INT8)
			return ctx_fail(CRTHIP_E_FORMAT, "Unsupported format.");
		if(g.components == 0 || g.components > ENC_PACK_MAX_N) return ctx_fail(CRTHIP_E_LIMIT, "crthip_encode_attrs: components must be 1..16");
		if(!(std::isfinite(g.q) && g.q > 0.0f)) return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_encode_attrs: q must be finite and > 0");
		if(g.strategy & ~(uint32_t)(CRTHIP_PARALLEL | CRTHIP_CORRELATED)) return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_encode_attrs: unknown strategy bits");
		if(!g.values && m->nvert) return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_encode_attrs: null values");
		const std::string name(g.name, len);
		if(std::find(taken.begin(), taken.end(), name) != taken.end()) return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_encode_attrs: attribute name already in use");
		taken.push_back(name);
		const uint64_t elems = (uint64_t)m->nvert*g.components;
		if(elems > 0xFFFFFFFFull) return ctx_fail(CRTHIP_E_LIMIT, "crthip_encode_attrs: nvert*components beyond 2^32");
		if(device && elems > (1u << 26)) return ctx_fail(CRTHIP_E_LIMIT, "crthip_encode_attrs: nvert*components beyond the device value coder's 2^26");
	}
	return CRTHIP_OK;
}

uint32_t corto_hip::generic_esize(uint32_t format) {
	return format == CRTHIP_FMT_DOUBLE ? 8u : format == CRTHIP_FMT_INT16 ? 2u : format == CRTHIP_FMT_INT8 ? 1u : 4u;
}

// crthip_mesh_layout's rules (include/corto_hip.h).  Strides have no upstream counterpart; the flags and the origin are upstream's overloads
// (src/encoder.cpp:77-81, 114-119, 151-158), whose addPositionsBits takes no origin.
int corto_hip::layout_resolve(const crthip_mesh *m, const crthip_attr_list *extra, const crthip_mesh_layout *L, MeshRead &rd) {
	rd = MeshRead{};
	rd.color = m->color ? (uint32_t)m->color_components : 0u;
	const uint32_t nattr = extra ? extra->nattr : 0;
	for(uint32_t k = 0; k < nattr; k++) rd.attr.push_back(extra->attr[k].components*generic_esize(extra->attr[k].format));
	if(!L) return CRTHIP_OK;
	if(L->flags & ~(uint32_t)(CRTHIP_IN_INDEX_UINT16 | CRTHIP_IN_NORMAL_INT16)) return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_mesh_layout: unknown flag bits");
	for(int k = 0; k < 3; k++) if(!std::isfinite(L->origin[k])) return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_mesh_layout: the origin must be finite");
	rd.has_origin = L->origin[0] != 0.0f || L->origin[1] != 0.0f || L->origin[2] != 0.0f;
	if(rd.has_origin && m->position_bits > 0) return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_mesh_layout: position_bits > 0 takes no origin (Encoder::addPositionsBits has none)");
	for(int k = 0; k < 3; k++) rd.origin[k] = L->origin[k];
	rd.index16 = (L->flags & CRTHIP_IN_INDEX_UINT16) && m->index && m->nface;
	rd.normal16 = (L->flags & CRTHIP_IN_NORMAL_INT16) && m->normal;
	if(rd.index16 && ((uintptr_t)m->index & 1u)) return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_mesh_layout: a uint16 index must be 2-byte aligned");
	if(rd.normal16 && ((uintptr_t)m->normal & 1u)) return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_mesh_layout: int16 normals must be 2-byte aligned");
	if(rd.normal16) rd.normal = 6;
	bool ok = true, strided = false;
	auto stride = [&](uint32_t given, uint32_t &resolved, uint32_t align, bool present) {   // resolved comes in as one vertex's bytes
		if(!given || !present) return;
		if(given % align || given < resolved) ok = false;
		strided = strided || given != resolved;
		resolved = given;
	};
	stride(L->position_stride, rd.position, 4, true);
	stride(L->normal_stride, rd.normal, rd.normal16 ? 2 : 4, m->normal != nullptr);
	stride(L->color_stride, rd.color, 1, m->color != nullptr);
	stride(L->uv_stride, rd.uv, 4, m->uv != nullptr);
	stride(L->radius_stride, rd.radius, 4, m->radius != nullptr);
	if(L->attr_stride) for(uint32_t k = 0; k < nattr; k++) stride(L->attr_stride[k], rd.attr[k], generic_esize(extra->attr[k].format), true);
	if(!ok) return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_mesh_layout: a stride must be a multiple of the element's alignment and at least one vertex's bytes");
	rd.plain = !(rd.index16 || rd.normal16 || rd.has_origin || strided);
	return CRTHIP_OK;
}

int corto_hip::index_range_host(const crthip_mesh *m, const MeshRead &rd) {
	if(!m->index || !m->nface) return CRTHIP_OK;
	const size_t n = (size_t)m->nface*3;
	bool bad = false;
	if(rd.index16) { const uint16_t *ix = (const uint16_t *)m->index; for(size_t i = 0; i < n; i++) bad |= ix[i] >= m->nvert; }
	else for(size_t i = 0; i < n; i++) bad |= m->index[i] >= m->nvert;
	return bad ? ctx_fail(CRTHIP_E_ARGUMENT, "crthip_encode: face index out of range") : CRTHIP_OK;
}

corto_hip::EncInputJob corto_hip::enc_input_job(const crthip_mesh *m, const MeshRead *rd) {
	EncInputJob J{};
	J.position = m->position; J.index = m->index; J.nvert = m->nvert; J.nface = m->index ? m->nface : 0;
	J.recipe = enc_in_recipe(m->position_bits, m->position_q, m->nvert, J.nface);
	J.pos_stride = rd ? rd->position : 12u;
	J.index16 = rd && rd->index16;
	J.has_origin = rd && rd->has_origin;
	if(rd) for(int k = 0; k < 3; k++) J.origin[k] = rd->origin[k];
	return J;
}

// The position step's two halves (src/encoder.cpp:49-100): the loops over the mesh's arrays, and the formulas over what they leave.  The
// loops are upstream's, in upstream's order; crthip_encode_batch_resident runs them on the device (enc_input_check.h) and the formulas here.
void corto_hip::input_stats_host(const crthip_mesh *m, uint32_t recipe, EncInputRecord &r, const MeshRead *rd) {
	memset(&r, 0, sizeof(r));
	const uint32_t nv = m->nvert, nface = m->index ? m->nface : 0;
	float *mn = r.box.mn, *mx = r.box.mx;
	// the arrays as the layout says they lie (none: packed floats, uint32 entries, origin 0)
	const size_t stride = rd ? rd->position : 12;
	const bool i16 = rd && rd->index16;
	const float zero[3] = {0.0f, 0.0f, 0.0f}, *o = rd ? rd->origin : zero;
	auto P = [&](size_t i) { return (const float *)((const uint8_t *)m->position + i*stride); };
	auto I = [&](size_t i) { return i16 ? (uint32_t)((const uint16_t *)m->index)[i] : m->index[i]; };
	if(recipe == EIN_STEP_BOX_FIRST) {
		for(int k = 0; k < 3; k++) mn[k] = mx[k] = P(0)[k];
		for(uint32_t i = 0; i < nv; i++) for(int k = 0; k < 3; k++) { const float v = P(i)[k]; if(v < mn[k]) mn[k] = v; if(v > mx[k]) mx[k] = v; }
	} else if(recipe == EIN_STEP_EDGE) {                        // the length of each face's first edge (src/encoder.cpp:105-110), on the raw positions
		double average = 0;
		for(uint32_t f = 0; f < nface; f++) {
			const float *a = P(I((size_t)f*3)), *b = P(I((size_t)f*3 + 1));
			const float d[3] = {a[0] - b[0], a[1] - b[1], a[2] - b[2]};
			average += (float)sqrt((double)(d[0]*d[0] + d[1]*d[1] + d[2]*d[2]));   // Point3f::norm, include/corto/point.h:111
		}
		r.sum = average;
	} else if(recipe == EIN_STEP_BOX_MAX) {                     // point cloud: the bounding box of input - o (src/encoder.cpp:80-91)
		for(int k = 0; k < 3; k++) { mn[k] = FLT_MAX; mx[k] = -FLT_MAX; }
		for(uint32_t i = 0; i < nv; i++) for(int k = 0; k < 3; k++) { const float v = P(i)[k] - o[k]; if(v < mn[k]) mn[k] = v; if(v > mx[k]) mx[k] = v; }
	}
}

float corto_hip::position_step(const crthip_mesh *m, uint32_t recipe, const EncInputRecord &r) {
	const uint32_t nv = m->nvert, nface = m->index ? m->nface : 0;
	if(recipe == EIN_STEP_BOX_FIRST) {
		const float intervals = powf(2.0f, (float)m->position_bits);
		float e[3]; for(int k = 0; k < 3; k++) { e[k] = r.box.mx[k] - r.box.mn[k]; e[k] /= intervals; }
		return std::max(std::max(e[0], e[1]), e[2]);
	}
	if(recipe == EIN_STEP_EDGE) return (float)(r.sum/nface)/20.0f;   // a twentieth of the mean
	if(recipe == EIN_STEP_BOX_MAX) {                            // from the bounding box volume
		float mx[3]; for(int k = 0; k < 3; k++) { mx[k] = r.box.mx[k]; mx[k] -= r.box.mn[k]; }
		return (float)(0.02*pow(mx[0]*mx[1]*mx[2], 2.0/3.0)/nv);
	}
	return m->position_q;
}

uint64_t corto_hip::quant_in_bytes(const QuantRequest &r) {
	const uint64_t n = r.count;
	switch(r.kind) {
	case QK_NORMAL: return n*((r.flags & corto_hip::QF_NORMAL_I16) ? 6 : 12);
	case QK_COLOR: return n*r.N;
	case QK_DOUBLE: return n*8;
	case QK_INT: return n*(r.format == CRTHIP_FMT_INT8 ? 1 : r.format == CRTHIP_FMT_INT16 ? 2 : 4);
	default: return n*4;
	}
}

uint64_t corto_hip::quant_vertex_bytes(const QuantRequest &r) {
	QuantRequest one = r;
	one.count = r.kind == QK_NORMAL || r.kind == QK_COLOR ? 1u : r.comps;
	return quant_in_bytes(one);
}

uint64_t corto_hip::quant_out_bytes(const QuantRequest &r) {
	const uint64_t n = r.count;
	return r.kind == QK_NORMAL ? n*8 : r.kind == QK_COLOR ? n*r.N : n*4;
}

extern "C" {


// Encode a mesh / point cloud into a .crt blob (host only).  Returns the blob size (also when out == NULL or cap is too
// small: call twice), or <0.  out_nvert/out_nface = counts after unreferenced vertices / degenerate faces are dropped.
// Everything encode_impl knows before the topology pass: exif, groups, the faces, and per attribute its parameters and its
// quantisation request (in the order the attributes are added; `alloc`: size the value arrays the requests write into).
// `step`: the position step when the caller has it already (crthip_encode_batch: computed once, before the device quantises).
struct NamedQuant { std::string name; corto_hip::QuantRequest r; };
// `extra`: the caller's generic attributes (Encoder::addAttribute, src/encoder.cpp:187-197), checked by encode_check_attrs.
// `faces`: copy the index into E.faces (only the host's topology pass reads it; with faces == false and a step m's data arrays are not read at all).
// `rd`: the mesh's arrays are read through this layout (the batch encoder: the requests carry it to the staging copies and the quantiser;
// with faces == true the index must be uint32 all the same).
static void setup(const crthip_mesh *m, const crthip_attr_list *extra, Encoder &E, std::vector<NamedQuant> &quant, bool alloc, const float *step, bool faces = true,
                  const corto_hip::MeshRead *rd = nullptr) {
	E.nvert = m->nvert; E.nface = m->index ? m->nface : 0; E.entropy = (uint32_t)m->entropy;
	const char *p = m->exif;
	for(uint32_t i = 0; i < m->nexif; i++) { std::string k(p); p += k.size() + 1; std::string v(p); p += v.size() + 1; E.exif[k] = v; }
	for(uint32_t g = 0; g < m->ngroups; g++) E.group_end.push_back(m->group_end[g]);
	if(m->group_nprops && m->group_props) {
		const char *gp = m->group_props;
		E.group_props.resize(m->ngroups);
		for(uint32_t g = 0; g < m->ngroups; g++)
			for(uint32_t i = 0; i < m->group_nprops[g]; i++) {
				std::string k(gp); gp += k.size() + 1;
				std::string v(gp); gp += v.size() + 1;
				E.group_props[g][k] = v;
			}
	}
	if(E.nface && faces) E.faces.assign(m->index, m->index + (size_t)E.nface*3);
	const uint32_t nv = m->nvert;
	auto request = [&](const char *name, Attr &a, corto_hip::QuantRequest r, size_t elems, size_t esize, uint32_t stride = 0, uint32_t comps = 1) {
		if(rd) { r.stride = stride; r.comps = comps; }
		if(alloc) { if(esize == 1) a.cvalues.resize(elems); else a.values.resize(elems); r.out = esize == 1 ? (void *)a.cvalues.data() : (void *)a.values.data(); }
		quant.push_back(NamedQuant{name, r});
	};
	{	// positions (src/encoder.cpp:49-100, vertex_attribute.h:79-128)
		float q = m->position_q;
		if(step) q = *step;
		else {
			const uint32_t recipe = corto_hip::enc_in_recipe(m->position_bits, m->position_q, nv, E.nface);
			corto_hip::EncInputRecord r;
			corto_hip::input_stats_host(m, recipe, r, rd);
			q = corto_hip::position_step(m, recipe, r);
		}
		Attr &a = E.data["position"];
		a.name = "position"; a.N = 3; a.q = q; a.format = CRTHIP_FMT_FLOAT;
		a.strategy = CRTHIP_CORRELATED | (E.nface > 0 ? CRTHIP_PARALLEL : 0);
		corto_hip::QuantRequest r; r.kind = QK_FLOAT; r.count = nv*3; r.in = m->position; r.q = q;
		if(rd && rd->has_origin) { r.flags |= corto_hip::QF_ORIGIN; for(int k = 0; k < 3; k++) r.origin[k] = rd->origin[k]; }
		request("position", a, r, (size_t)nv*3, 4, rd ? rd->position : 0, 3);
	}
	if(m->normal) {
		Attr &a = E.data["normal"];
		a.name = "normal"; a.codec = CRTHIP_CODEC_NORMAL; a.N = 3; a.q = powf(2.0f, (float)(m->normal_bits - 1));
		a.format = CRTHIP_FMT_FLOAT; a.strategy = CRTHIP_CORRELATED; a.prediction = m->normal_prediction;
		corto_hip::QuantRequest r; r.kind = QK_NORMAL; r.count = nv; r.in = m->normal; r.unit = f2i(a.q);
		if(rd && rd->normal16) r.flags |= corto_hip::QF_NORMAL_I16;                    // (the format byte stays FLOAT: upstream converts, then addNormals(float *))
		request("normal", a, r, (size_t)nv*2, 4, rd ? rd->normal : 0);
	}
	if(m->color) {
		Attr &a = E.data["color"];
		a.name = "color"; a.codec = CRTHIP_CODEC_COLOR; a.N = m->color_components; a.format = CRTHIP_FMT_UINT8; a.strategy = 0; a.q = 0;
		for(int k = 0; k < 3; k++) a.qc[k] = 1 << (8 - m->color_bits[k]);
		a.qc[3] = m->color_components == 3 ? 1 : 1 << (8 - m->color_bits[3]);           // addColors3: setQ(r, g, b, 8)
		corto_hip::QuantRequest r; r.kind = QK_COLOR; r.count = nv; r.N = (uint32_t)a.N; r.in = m->color; for(int k = 0; k < 4; k++) r.qc[k] = (uint32_t)a.qc[k];
		request("color", a, r, (size_t)nv*a.N, 1, rd ? rd->color : 0);
	}
	// GenericAttr<int>::quantize (vertex_attribute.h:79-104): the recipe follows the input format, the header keeps it as the format byte
	auto generic = [&](const char *name, const void *buf, int N, float q, uint32_t format, uint32_t strategy, uint32_t stride) {
		Attr &a = E.data[name];
		a.name = name; a.N = N; a.q = q; a.format = (int)format; a.strategy = (int)strategy;
		corto_hip::QuantRequest r;
		r.kind = format == CRTHIP_FMT_FLOAT ? QK_FLOAT : format == CRTHIP_FMT_DOUBLE ? QK_DOUBLE : QK_INT;
		r.format = format; r.count = nv*(uint32_t)N; r.in = buf; r.q = q;
		request(name, a, r, (size_t)nv*N, 4, stride, (uint32_t)N);
	};
	if(m->uv) generic("uv", m->uv, 2, m->uv_q, CRTHIP_FMT_FLOAT, 0, rd ? rd->uv : 0);
	if(m->radius) generic("radius", m->radius, 1, m->radius_q, CRTHIP_FMT_FLOAT, 0, rd ? rd->radius : 0);
	if(extra)
		for(uint32_t k = 0; k < extra->nattr; k++) {
			const crthip_generic_attr &g = extra->attr[k];
			generic(g.name, g.values, (int)g.components, g.q, g.format, g.strategy, rd && k < rd->attr.size() ? rd->attr[k] : 0);
		}
}

// the host's quantisation of one request (what k_enc_quantize does on the device, enc_quant.h)
static void quantize_host(const corto_hip::QuantRequest &r) {
	if(r.kind == QK_FLOAT) {                                                         // vertex_attribute.h:97-99
		const float *in = (const float *)r.in; int32_t *o = (int32_t *)r.out;
		for(size_t i = 0; i < r.count; i++) o[i] = f2i((in[i] - 0.0f)/r.q);
	} else if(r.kind == QK_INT) {                                                    // vertex_attribute.h:85-96: int -> float, float division
		int32_t *o = (int32_t *)r.out;
		if(r.format == CRTHIP_FMT_INT8) { const int8_t *in = (const int8_t *)r.in; for(size_t i = 0; i < r.count; i++) o[i] = f2i((float)in[i]/r.q); }
		else if(r.format == CRTHIP_FMT_INT16) { const int16_t *in = (const int16_t *)r.in; for(size_t i = 0; i < r.count; i++) o[i] = f2i((float)in[i]/r.q); }
		else { const int32_t *in = (const int32_t *)r.in; for(size_t i = 0; i < r.count; i++) o[i] = f2i((float)in[i]/r.q); }
	} else if(r.kind == QK_DOUBLE) {                                                 // vertex_attribute.h:100-102: double division
		const double *in = (const double *)r.in; int32_t *o = (int32_t *)r.out;
		for(size_t i = 0; i < r.count; i++) o[i] = d2i(in[i]/(double)r.q);
	} else if(r.kind == QK_NORMAL) {
		for(uint32_t i = 0; i < r.count; i++) to_octa((const float *)r.in + (size_t)i*3, r.unit, (int32_t *)r.out + (size_t)i*2);
	} else {                                                                         // color_attribute.cpp:30-44, point.h:213
		const uint8_t *in = (const uint8_t *)r.in; uint8_t *o = (uint8_t *)r.out;
		const int N = (int)r.N;
		for(uint32_t i = 0; i < r.count; i++) {
			uint8_t y[4] = {0, 0, 0, 0};
			for(int k = 0; k < N; k++) y[k] = (uint8_t)(in[(size_t)i*N + k]/(int)r.qc[k]);
			const uint8_t ycc[4] = {y[1], (uint8_t)(y[2] - y[1]), (uint8_t)(y[0] - y[1]), y[3]};
			for(int k = 0; k < N; k++) o[(size_t)i*N + k] = ycc[k];
		}
	}
}

static int64_t encode_impl(const crthip_mesh *m, const crthip_attr_list *extra, uint8_t *out, size_t cap, uint32_t *out_nvert, uint32_t *out_nface,
                           crthip_ctx *gpu, const float *step = nullptr) {
	if(!m || !m->position) return CRTHIP_E_ARGUMENT;
	Encoder E;
	std::vector<Deferred> deferred;
	if(gpu) E.s.defer = &deferred;
	std::vector<NamedQuant> named;
	setup(m, extra, E, named, true, step);
	std::vector<corto_hip::QuantRequest> quant;                     // (device path) the attributes' quantisation, collected and run in one call
	for(const NamedQuant &q : named) { if(gpu) quant.push_back(q.r); else quantize_host(q.r); }
	if(gpu) { const int qerr = corto_hip::quantize_device(gpu, quant); if(qerr) return qerr; }   // every attribute's quantisation in one device call (k_enc_quantize)
	E.header();
	if(E.nface > 0) E.encode_mesh(); else E.encode_cloud();
	if(out_nvert) *out_nvert = E.nvert;
	if(out_nface) *out_nface = E.nface;
	if(gpu) {
		// the recorded streams go through the device stages in one call, then the container is written from the frame and their results
		// (enc_splice.h: write_container - the zero padding in front of every bit stream depends on the final position)
		std::vector<corto_hip::EncValueStream> in;
		for(const Deferred &d : deferred) {
			if(d.kind == corto_hip::BATCH_BITS) continue;
			corto_hip::EncValueStream v;
			v.kind = d.kind; v.count = d.count; v.components = d.N;
			v.values = d.kind == CRTHIP_ENC_SYMBOLS || d.kind == CRTHIP_ENC_VALUES_I8 ? (const void *)d.bytes.data() : (const void *)d.ints.data();
			in.push_back(v);
		}
		corto_hip::Coded res;
		const int err = corto_hip::encode_value_streams(gpu, E.entropy, in, res, nullptr);
		if(err) return err;
		const std::vector<uint32_t> none, *split_words = &none;       // (a mesh records one packed bit stream, its CLERS split bits; a cloud none)
		for(const Deferred &d : deferred) if(d.kind == corto_hip::BATCH_BITS) split_words = &d.words;
		std::vector<uint8_t> f;
		corto_hip::ByteOut o{f};
		corto_hip::write_container(o, E.s.b, deferred, res.streams.data(), *split_words);
		E.s.b.swap(f);
	}
	if(out && cap >= E.s.b.size()) memcpy(out, E.s.b.data(), E.s.b.size());
	return (int64_t)E.s.b.size();
}

// nothing is thrown across the C boundary
static int64_t encode_checked(const crthip_mesh *m, const crthip_attr_list *extra, uint8_t *out, size_t cap, uint32_t *out_nvert, uint32_t *out_nface,
                              crthip_ctx *gpu) {
	{ const int e = corto_hip::encode_check(m); if(e) return e; }
	{ const int e = corto_hip::encode_check_attrs(m, extra, gpu != nullptr); if(e) return e; }
	try {
		return encode_impl(m, extra, out, cap, out_nvert, out_nface, gpu);
	} catch(const std::bad_alloc &) {
		return corto_hip::ctx_fail(CRTHIP_E_NOMEM, nullptr);
	} catch(...) {
		return corto_hip::ctx_fail(CRTHIP_E_ARGUMENT, "crthip_encode: internal error");
	}
}

int64_t crthip_encode_attrs(const crthip_mesh *m, const crthip_attr_list *extra, uint8_t *out, size_t cap, uint32_t *out_nvert, uint32_t *out_nface) {
	return encode_checked(m, extra, out, cap, out_nvert, out_nface, nullptr);
}

int64_t crthip_encode(const crthip_mesh *m, uint8_t *out, size_t cap, uint32_t *out_nvert, uint32_t *out_nface) {
	return crthip_encode_attrs(m, nullptr, out, cap, out_nvert, out_nface);
}

// crthip_encode_layout: the mesh's HOST arrays converted into packed ones - upstream's own conversions, each one float operation
// (src/encoder.cpp:80-81, 116-117, 156) - and handed to the encoder above.  A mesh's first-edge step is taken from the raw positions
// (:105-110 runs before the origin is subtracted), so it is computed here and passed along.
namespace {
struct PackedMesh {
	crthip_mesh m;
	crthip_attr_list list{0, nullptr};
	std::vector<crthip_generic_attr> attrs;
	std::vector<float> pos, nrm, uv, rad;
	std::vector<uint32_t> idx;
	std::vector<uint8_t> col;
	std::vector<std::vector<uint8_t>> extra;
};
void gather(void *dst, const void *src, size_t n, size_t stride, size_t bytes) {
	for(size_t i = 0; i < n; i++) memcpy((uint8_t *)dst + i*bytes, (const uint8_t *)src + i*stride, bytes);
}
void pack_layout_host(const crthip_mesh *m, const crthip_attr_list *extra, const corto_hip::MeshRead &rd, PackedMesh &P) {
	const size_t nv = m->nvert;
	P.m = *m;
	P.pos.resize(nv*3);
	gather(P.pos.data(), m->position, nv, rd.position, 12);
	if(rd.has_origin) for(size_t i = 0; i < nv*3; i++) P.pos[i] = P.pos[i] - rd.origin[i%3];
	P.pos.resize(nv*3 + 3);                                     // (position stays non-null for an empty mesh)
	P.m.position = P.pos.data();
	if(m->index && m->nface) {
		P.idx.resize((size_t)m->nface*3);
		if(rd.index16) { const uint16_t *ix = (const uint16_t *)m->index; for(size_t i = 0; i < P.idx.size(); i++) P.idx[i] = ix[i]; }
		else memcpy(P.idx.data(), m->index, P.idx.size()*4);
		P.m.index = P.idx.data();
	}
	if(m->normal) {
		P.nrm.resize(nv*3 + 3);
		if(rd.normal16) {
			for(size_t i = 0; i < nv; i++) {
				int16_t v[3];
				memcpy(v, (const uint8_t *)m->normal + i*rd.normal, 6);
				for(int k = 0; k < 3; k++) P.nrm[i*3 + k] = (float)v[k]/32767.0f;
			}
		} else gather(P.nrm.data(), m->normal, nv, rd.normal, 12);
		P.m.normal = P.nrm.data();
	}
	if(m->color) { P.col.resize(nv*m->color_components + 4); gather(P.col.data(), m->color, nv, rd.color, (size_t)m->color_components); P.m.color = P.col.data(); }
	if(m->uv) { P.uv.resize(nv*2 + 2); gather(P.uv.data(), m->uv, nv, rd.uv, 8); P.m.uv = P.uv.data(); }
	if(m->radius) { P.rad.resize(nv + 1); gather(P.rad.data(), m->radius, nv, rd.radius, 4); P.m.radius = P.rad.data(); }
	if(extra && extra->nattr) {
		P.attrs.assign(extra->attr, extra->attr + extra->nattr);
		P.extra.resize(extra->nattr);
		for(uint32_t k = 0; k < extra->nattr; k++) {
			const size_t bytes = (size_t)P.attrs[k].components*corto_hip::generic_esize(P.attrs[k].format);
			P.extra[k].resize(nv*bytes + 8);
			gather(P.extra[k].data(), P.attrs[k].values, nv, rd.attr[k], bytes);
			P.attrs[k].values = P.extra[k].data();
		}
		P.list.nattr = extra->nattr; P.list.attr = P.attrs.data();
	}
}
} // namespace

int64_t crthip_encode_layout(const crthip_mesh *m, const crthip_attr_list *extra, const crthip_mesh_layout *layout, uint8_t *out, size_t cap,
                             uint32_t *out_nvert, uint32_t *out_nface) {
	using namespace corto_hip;
	{ const int e = encode_check(m, false); if(e) return e; }
	{ const int e = encode_check_attrs(m, extra, false); if(e) return e; }
	MeshRead rd;
	{ const int e = layout_resolve(m, extra, layout, rd); if(e) return e; }
	if(rd.plain) return encode_checked(m, extra, out, cap, out_nvert, out_nface, nullptr);
	{ const int e = index_range_host(m, rd); if(e) return e; }
	try {
		float step = 0;
		const uint32_t recipe = enc_in_recipe(m->position_bits, m->position_q, m->nvert, m->index ? m->nface : 0);
		const bool raw_step = recipe == EIN_STEP_EDGE && rd.has_origin;
		if(raw_step) { EncInputRecord r; input_stats_host(m, recipe, r, &rd); step = position_step(m, recipe, r); }
		PackedMesh P;
		pack_layout_host(m, extra, rd, P);
		return encode_impl(&P.m, extra ? &P.list : nullptr, out, cap, out_nvert, out_nface, nullptr, raw_step ? &step : nullptr);
	} catch(const std::bad_alloc &) {
		return ctx_fail(CRTHIP_E_NOMEM, nullptr);
	} catch(...) {
		return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_encode_layout: internal error");
	}
}

// crthip_encode with the value coding (bit widths, bit packing) and the entropy coder on the device (encode_gpu.cpp)
int64_t crthip_encode_gpu_attrs(crthip_ctx *ctx, const crthip_mesh *m, const crthip_attr_list *extra, uint8_t *out, size_t cap,
                                uint32_t *out_nvert, uint32_t *out_nface) {
	if(!ctx) return corto_hip::ctx_fail(CRTHIP_E_ARGUMENT, "crthip_encode_gpu: null context (there is no CPU fallback: use crthip_encode for the host encoder)");
	return encode_checked(m, extra, out, cap, out_nvert, out_nface, ctx);
}

int64_t crthip_encode_gpu(crthip_ctx *ctx, const crthip_mesh *m, uint8_t *out, size_t cap, uint32_t *out_nvert, uint32_t *out_nface) {
	return crthip_encode_gpu_attrs(ctx, m, nullptr, out, cap, out_nvert, out_nface);
}

} // extern "C"


// the encoder-side Tunstall tables of one stream, from its byte histogram (for the GPU encoder stages, encode_gpu.cpp)
void corto_hip::tun_encoder_tables(const uint32_t counts[256], uint32_t size, TunEncoderTables &out) {
	Tunstall t;
	std::vector<int> cnt(counts, counts + 256);
	t.from_counts(cnt, (int)size);
	t.build();
	t.trie();
	out.nsym = (uint32_t)t.probs.size();
	for(uint32_t i = 0; i < out.nsym; i++) { out.probs[2*i] = t.probs[i].symbol; out.probs[2*i + 1] = t.probs[i].probability; }
	memset(out.remap, 0, sizeof(out.remap));
	memset(out.lengths, 0, sizeof(out.lengths));
	for(size_t i = 0; i < t.remap.size() && i < 256; i++) out.remap[i] = t.remap[i];
	for(size_t i = 0; i < t.lengths.size() && i < 256; i++) out.lengths[i] = (uint16_t)t.lengths[i];
	out.offsets.assign(t.offsets.begin(), t.offsets.end());
}

// crthip_encode_splice_model's front: crthip_encode_gpu's deferred run with the quantisation on the host, then every recorded stream through
// the writers crthip_encode itself uses (put_symbols / put_array / put_values into a sink of its own: at position 0 a bit stream needs no
// padding, so its words follow its count).  The sink's bytes become a buffer of o.coded, the stream points into it: the words behind the
// count, each block where put_symbols wrote it, cut where put_symbols ended its header.  `o` comes fresh.
int corto_hip::encode_host_coded(const crthip_mesh *m, const crthip_attr_list *extra, HostCodedItem &o) {
	{ const int e = encode_check(m); if(e) return e; }
	{ const int e = encode_check_attrs(m, extra, false); if(e) return e; }
	Encoder E;
	std::vector<Deferred> deferred;
	E.s.defer = &deferred;
	std::vector<NamedQuant> named;
	setup(m, extra, E, named, true, nullptr);
	for(const NamedQuant &q : named) quantize_host(q.r);
	E.header();
	if(E.nface > 0) E.encode_mesh(); else E.encode_cloud();
	o.entropy = E.entropy; o.nvert = E.nvert; o.nface = E.nface;
	for(const Deferred &d : deferred) {
		o.slots.push_back(d);
		if(d.kind == BATCH_BITS) { o.split_words = d.words; continue; }
		Sink t;
		std::vector<Sink::Block> blocks;
		t.blocks = &blocks;
		if(d.kind == CRTHIP_ENC_SYMBOLS) put_symbols(t, E.entropy, d.bytes.data(), d.count);
		else if(d.kind == CRTHIP_ENC_ARRAY) put_array(t, E.entropy, d.count, d.ints.data(), (int)d.N);
		else if(d.kind == CRTHIP_ENC_VALUES_I8) put_values<int8_t>(t, E.entropy, d.count, (const int8_t *)d.bytes.data(), (int)d.N);
		else put_values<int32_t>(t, E.entropy, d.count, d.ints.data(), (int)d.N);
		CodedStream x;
		if(d.kind != CRTHIP_ENC_SYMBOLS) { memcpy(&x.nwords, t.b.data(), 4); x.words = t.b.data() + 4; }
		for(const Sink::Block &k : blocks) {
			CodedBlock b;
			b.head.assign(t.b.begin() + k.at, t.b.begin() + k.at + k.head);
			b.payload = t.b.data() + k.at + k.head; b.bytes = (uint32_t)k.payload;
			x.blocks.push_back(std::move(b));
		}
		o.coded.streams.push_back(std::move(x));
		o.coded.h_made.push_back(std::move(t.b));                 // (the bytes stay where they are: the pointers hold)
	}
	o.frame.swap(E.s.b);
	return CRTHIP_OK;
}

// ---- crthip_encode_batch's host half (encode_batch.cpp runs the rest on the device) ----

void corto_hip::morton_order_host(const int32_t *coords, uint32_t nvert, std::vector<uint32_t> &order) {   // src/encoder.cpp:238-262
	int32_t mn[3] = {0, 0, 0};
	for(uint32_t i = 0; i < nvert; i++) for(int k = 0; k < 3; k++) mn[k] = std::min(mn[k], coords[(size_t)i*3 + k]);
	std::vector<ZPoint> z(nvert);
	for(uint32_t i = 0; i < nvert; i++) {
		const uint64_t x = (uint64_t)(int64_t)(coords[(size_t)i*3] - mn[0]), y = (uint64_t)(int64_t)(coords[(size_t)i*3 + 1] - mn[1]), w = (uint64_t)(int64_t)(coords[(size_t)i*3 + 2] - mn[2]);
		uint64_t bits = 0; const uint64_t l = 1;
		for(int k = 0; k < 21; k++) bits |= (x & l << k) << (2*k) | (y & l << k) << (2*k + 1) | (w & l << k) << (2*k + 2);   // include/corto/zpoint.h:34-38
		z[i] = ZPoint{bits, i};
	}
	std::sort(z.rbegin(), z.rend());
	order.resize(nvert);
	for(uint32_t i = 0; i < nvert; i++) order[i] = z[i].pos;
}

void corto_hip::batch_setup(const crthip_mesh *m, const crthip_attr_list *extra, BatchItem &it, const float *step, const MeshRead *rd) {
	Encoder E;
	std::vector<NamedQuant> named;
	setup(m, extra, E, named, false, step, false, rd);
	it.index16 = rd && rd->index16;
	it.entropy = E.entropy; it.nvert_in = m->nvert; it.nface_in = E.nface;
	it.attrs.clear();
	for(auto &kv : E.data) {                                     // the container's order (std::map)
		const Attr &a = kv.second;
		BatchAttr b;
		b.codec = (uint32_t)a.codec; b.N = (uint32_t)a.N; b.prediction = (uint32_t)a.prediction; b.strategy = (uint32_t)a.strategy;
		if(kv.first == "position") it.pos = (uint32_t)it.attrs.size();
		for(const NamedQuant &q : named) if(q.name == kv.first) b.quant = q.r;
		it.attrs.push_back(b);
	}
}

// the stream table of an item from the slots its body recorded (mesh: CLERS symbols, split bits, then the attributes)
static void batch_streams(const Encoder &E, const std::vector<Deferred> &deferred, bool mesh, corto_hip::BatchItem &it) {
	using namespace corto_hip;
	it.streams.clear();
	const size_t first_attr = mesh ? 2 : 0;
	for(size_t k = 0; k < deferred.size(); k++) {
		const Deferred &d = deferred[k];
		BatchStream b = d;
		b.attr = k < first_attr ? (k == 0 ? -1 : -2) : (int32_t)(k - first_attr);
		if(d.kind == BATCH_BITS) it.split_words = d.words;
		else if(b.attr >= 0 && it.attrs[b.attr].codec == CRTHIP_CODEC_NORMAL)         // the residuals' count: every vertex, or (BORDER) the device's
			b.count = it.attrs[b.attr].prediction == 2 ? 0u : E.nvert;
		it.streams.push_back(b);
	}
}

void corto_hip::batch_topology(const crthip_mesh *m, const crthip_attr_list *extra, BatchItem &it) {
	Encoder E;
	std::vector<NamedQuant> named;
	float step = it.attrs[it.pos].quant.q;
	setup(m, extra, E, named, false, &step);
	std::vector<Deferred> deferred;
	E.s.defer = &deferred; E.s.shape_only = true;
	E.header();
	const bool mesh = E.nface > 0;
	if(mesh) {
		E.topology();
		E.nvert = E.current_vertex;
		E.prediction.resize(E.nvert);
		E.mesh_body();
		it.faces.swap(E.faces);
		it.quads.resize((size_t)E.nvert*4);
		if(E.nvert) memcpy(it.quads.data(), E.prediction.data(), (size_t)E.nvert*16);
		it.clers.swap(E.clers);
	} else E.cloud_body();
	it.nvert = E.nvert; it.nface = E.nface; it.nclers = (uint32_t)it.clers.size();
	it.frame.swap(E.s.b);
	batch_streams(E, deferred, mesh, it);
}

void corto_hip::batch_frame(const crthip_mesh *m, const crthip_attr_list *extra, BatchItem &it, const EncTopoRecord &rec, const uint32_t *group_end,
                            const uint32_t *split_words) {
	Encoder E;
	std::vector<NamedQuant> named;
	float step = it.attrs[it.pos].quant.q;
	setup(m, extra, E, named, false, &step, false);           // (the device pass has the faces: m->index may be a device pointer)
	std::vector<Deferred> deferred;
	E.s.defer = &deferred; E.s.shape_only = true;
	E.header();
	const size_t ngroups = std::max<size_t>(E.group_end.size(), 1);
	E.group_end.assign(group_end, group_end + ngroups);
	E.nvert = rec.nvert; E.nface = rec.nface; E.max_front = rec.max_front;
	E.split.words.assign(split_words, split_words + rec.split_words);     // flushed on the device: emit() finds nothing to add
	// mesh_body with the CLERS symbols' count in place of the symbols
	E.s.u32(E.nvert); E.s.u32(E.nface);
	E.groups();
	E.s.u32(E.max_front);
	put_symbols(E.s, E.entropy, nullptr, rec.nclers);
	E.split.emit(E.s);
	for(auto &kv : E.data) E.attr_encode(kv.second);
	it.nvert = E.nvert; it.nface = E.nface; it.nclers = rec.nclers;
	it.frame.swap(E.s.b);
	batch_streams(E, deferred, true, it);
}

void corto_hip::topology_host_model(const crthip_mesh *m, TopologyModel &out) {
	Encoder E;
	std::vector<NamedQuant> named;
	float step = 1.0f;
	setup(m, nullptr, E, named, false, &step);
	E.topology();
	out.split_bits = (uint64_t)E.split.words.size()*32 + (uint64_t)(32 - E.split.bits);
	E.split.flush();
	out.nvert = E.current_vertex; out.nface = E.nface; out.max_front = E.max_front;
	out.faces.swap(E.faces); out.group_end.swap(E.group_end); out.clers.swap(E.clers); out.split_words.swap(E.split.words);
	out.quads.resize((size_t)out.nvert*4);
	if(out.nvert) memcpy(out.quads.data(), E.prediction.data(), (size_t)out.nvert*16);
}
