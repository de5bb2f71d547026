// walk_probe.cpp — crt_walk.h's walker (run on the host through a bounds-counting reader) + record_to_layout against walk_blob, for
// tests/test_resident_walk_cpu.py.  Built with the library's own crt_format.cpp:
//   walk_probe CORPUS CAP golden              every blob of the corpus as it is
//   walk_probe CORPUS CAP trunc I             every truncation length 0..len of blob I
//   walk_probe CORPUS CAP edits I             byte edits at every header and framing field offset of blob I (six values each)
//   walk_probe CORPUS CAP fuzz SEED COUNT     COUNT random multi-byte corruptions of random corpus blobs
// CORPUS: u32 count, then per blob u32 len + bytes.  CAP: the record capacity in bytes (a multiple of 16, >= 64).
// FALLBACK lines (golden: the blobs that went to the host walk, up to 32), then one summary line:  n=.. ok=.. fallback=.. mismatch=.. oob=.. guard=.. codes=CODE:COUNT,...   (after up to 8 "MISMATCH ..." lines)
// mismatch: a status or a layout that differs; oob: reads the walker asked for at or past the blob's length; guard: record bytes written
// past CAP.
#include "crt_walk.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <vector>

using namespace corto_hip;

struct HostReader {
	const uint8_t *p; uint32_t len; uint64_t *oob;
	uint32_t byte(uint32_t pos) { if(pos >= len) { (*oob)++; return 0; } return p[pos]; }
	void copy(uint8_t *dst, uint32_t n) { if(n > len) { (*oob)++; n = len; } std::memcpy(dst, p, n); }
};

static std::string diff_stream(const StreamRef &a, const StreamRef &b) {
	if(a.mode != b.mode || a.nsym != b.nsym || a.probs_off != b.probs_off || a.size != b.size || a.csize != b.csize ||
	   a.payload_off != b.payload_off || a.fill != b.fill || a.max_sym != b.max_sym || std::memcmp(a.probs16, b.probs16, 32))
		return "stream";
	return "";
}

static std::string diff_layout(const BlobLayout &a, const BlobLayout &b) {
	const BlobHeader &x = a.h, &y = b.h;
	if(x.version != y.version || x.entropy != y.entropy || x.nvert != y.nvert || x.nface != y.nface || x.body_offset != y.body_offset)
		return "header fields";
	if(x.exif != y.exif) return "exif";
	if(x.attrs.size() != y.attrs.size()) return "attribute count";
	for(size_t i = 0; i < x.attrs.size(); i++) {
		const AttrHeader &p = x.attrs[i], &q = y.attrs[i];
		if(p.name != q.name || p.codec != q.codec || std::memcmp(&p.q, &q.q, 4) || p.N != q.N || p.format != q.format || p.strategy != q.strategy)
			return "attribute " + std::to_string(i);
	}
	if(a.group_end != b.group_end || a.group_props != b.group_props) return "groups";
	if(a.max_front != b.max_front || a.split.words_off != b.split.words_off || a.split.nwords != b.split.nwords) return "index block";
	if(!diff_stream(a.clers, b.clers).empty()) return "clers stream";
	if(a.attrs.size() != b.attrs.size()) return "attribute blocks";
	for(size_t i = 0; i < a.attrs.size(); i++) {
		const AttrStreams &p = a.attrs[i], &q = b.attrs[i];
		if(p.bits.words_off != q.bits.words_off || p.bits.nwords != q.bits.nwords || p.normal_prediction != q.normal_prediction ||
		   std::memcmp(p.qc, q.qc, sizeof(p.qc)) || p.logs.size() != q.logs.size())
			return "attribute block " + std::to_string(i);
		for(size_t k = 0; k < p.logs.size(); k++)
			if(!diff_stream(p.logs[k], q.logs[k]).empty()) return "attribute " + std::to_string(i) + " log " + std::to_string(k);
	}
	if(a.end_offset != b.end_offset) return "end offset";
	return "";
}

struct Tally {
	uint64_t n = 0, ok = 0, fallback = 0, mismatch = 0, oob = 0, guard = 0;
	std::map<int, uint64_t> codes;
};

static bool report_fallbacks = false;                      // golden: name the blobs that went to the host walk

static void check(const std::vector<uint8_t> &blob, uint32_t cap, Tally &t, const std::string &tag) {
	const uint32_t len = (uint32_t)blob.size();
	std::vector<uint32_t> buf(len/4 + 2);                   // 4-byte aligned, as walk_blob wants
	std::memcpy(buf.data(), blob.data(), len);
	const uint8_t *p = (const uint8_t *)buf.data();
	BlobLayout want;
	const int s_host = walk_blob(p, len, want);
	std::vector<uint32_t> recw(cap/4 + 16);
	uint8_t *rec = (uint8_t *)recw.data();
	std::memset(rec, 0xCD, cap + 64);
	HostReader r{p, len, &t.oob};
	WalkWork w;
	const int s_walk = walk_record(r, len, rec, cap, w);
	for(uint32_t k = cap; k < cap + 64; k++) if(rec[k] != 0xCD) { t.guard++; break; }
	BlobLayout got;
	const int s_rec = record_to_layout(rec, cap, got);
	t.n++; t.codes[s_host]++;
	std::string why;
	if(s_walk != s_host) why = "status " + std::to_string(s_walk) + " vs walk_blob " + std::to_string(s_host);
	else if(s_rec == WALK_FALLBACK) {
		if(t.fallback++ < 32 && report_fallbacks) std::printf("FALLBACK %s\n", tag.c_str());
		if(s_host) why = "a failed walk asked for the host walk";
	}
	else if(s_rec != s_host) why = "record status " + std::to_string(s_rec) + " vs walk_blob " + std::to_string(s_host);
	else if(s_host == CRTHIP_OK) why = diff_layout(got, want);
	if(why.empty()) { if(s_host == CRTHIP_OK && s_rec == CRTHIP_OK) t.ok++; return; }
	if(t.mismatch++ < 8) std::printf("MISMATCH %s: %s\n", tag.c_str(), why.c_str());
}

// every byte of the header and groups, and of the framing of each block: a window in front of every bits block and stream (the count
// words, padding, a normal's prediction byte and a colour's quantisation bytes) and each Tunstall stream's table and two size words
static std::set<uint32_t> framing(const std::vector<uint8_t> &blob) {
	std::set<uint32_t> at;
	const uint32_t len = (uint32_t)blob.size();
	std::vector<uint32_t> buf(len/4 + 2);
	std::memcpy(buf.data(), blob.data(), len);
	BlobLayout L;
	if(walk_blob((const uint8_t *)buf.data(), len, L)) return at;
	uint64_t oob = 0;
	HostReader r{(const uint8_t *)buf.data(), len, &oob};
	std::vector<uint32_t> recw(WALK_RECORD_BYTES/4 + 16);
	WalkWork w;
	walk_record(r, len, (uint8_t *)recw.data(), WALK_RECORD_BYTES, w);
	const uint32_t prefix = ((const WalkHead *)recw.data())->prefix_len;
	for(uint32_t k = 0; k < prefix; k++) at.insert(k);
	auto window = [&](uint32_t end, uint32_t before) { for(uint32_t k = end > before ? end - before : 0; k < end; k++) at.insert(k); };
	auto stream = [&](const StreamRef &s) {
		if(L.h.entropy == CRTHIP_ENTROPY_NONE) { window(s.payload_off, 8); return; }
		window(s.probs_off, 8);
		for(uint32_t k = s.probs_off; k < s.probs_off + 2*s.nsym + 8; k++) at.insert(k);
	};
	if(L.h.nface) { window(L.split.words_off, 8); stream(L.clers); }
	for(auto &a : L.attrs) { window(a.bits.words_off, 12); for(auto &s : a.logs) stream(s); }
	at.insert(L.end_offset ? L.end_offset - 1 : 0);
	std::set<uint32_t> in;
	for(uint32_t k : at) if(k < len) in.insert(k);
	return in;
}

static uint64_t rng_state;
static uint64_t next() {                                   // splitmix64
	uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
	return z ^ (z >> 31);
}

int main(int argc, char **argv) {
	if(argc < 4) { std::fprintf(stderr, "usage: walk_probe CORPUS CAP golden|trunc I|edits I|fuzz SEED COUNT\n"); return 2; }
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
	const uint32_t cap = (uint32_t)std::atoi(argv[2]);
	if(cap < 64 || cap % 16) { std::fprintf(stderr, "CAP: a multiple of 16, >= 64\n"); return 2; }
	const std::string cmd = argv[3];
	Tally t;
	if(cmd == "golden") {
		report_fallbacks = true;
		for(size_t i = 0; i < corpus.size(); i++) check(corpus[i], cap, t, "blob " + std::to_string(i));
	} else if(cmd == "trunc" && argc > 4) {
		const auto &b = corpus.at((size_t)std::atoi(argv[4]));
		for(size_t k = 0; k <= b.size(); k++) check(std::vector<uint8_t>(b.begin(), b.begin() + k), cap, t, "length " + std::to_string(k));
	} else if(cmd == "edits" && argc > 4) {
		const auto &b = corpus.at((size_t)std::atoi(argv[4]));
		for(uint32_t at : framing(b)) {
			const uint8_t v0 = b[at];
			for(uint8_t v : {(uint8_t)(v0 ^ 0xFF), (uint8_t)0, (uint8_t)0xFF, (uint8_t)(v0 + 1), (uint8_t)(v0 - 1), (uint8_t)(v0 ^ 0x80)}) {
				if(v == v0) continue;
				std::vector<uint8_t> e = b;
				e[at] = v;
				check(e, cap, t, "byte " + std::to_string(at) + " = " + std::to_string(v));
			}
		}
	} else if(cmd == "fuzz" && argc > 5) {
		rng_state = std::strtoull(argv[4], nullptr, 10);
		const uint64_t count = std::strtoull(argv[5], nullptr, 10);
		for(uint64_t c = 0; c < count; c++) {
			std::vector<uint8_t> e = corpus[next() % corpus.size()];
			if(e.empty()) continue;
			const uint32_t edits = 2 + (uint32_t)(next() % 7);
			for(uint32_t k = 0; k < edits; k++) {
				// half of them in the first KiB, where the header and most framing words are
				const uint32_t span = (next() & 1) ? (uint32_t)std::min<size_t>(e.size(), 1024) : (uint32_t)e.size();
				e[next() % span] = (uint8_t)next();
			}
			if(next() % 8 == 0) e.resize(next() % (e.size() + 1));
			check(e, cap, t, "fuzz case " + std::to_string(c));
		}
	} else { std::fprintf(stderr, "unknown command\n"); return 2; }
	std::printf("n=%llu ok=%llu fallback=%llu mismatch=%llu oob=%llu guard=%llu codes=", (unsigned long long)t.n, (unsigned long long)t.ok,
	            (unsigned long long)t.fallback, (unsigned long long)t.mismatch, (unsigned long long)t.oob, (unsigned long long)t.guard);
	bool first = true;
	for(auto &kv : t.codes) { std::printf("%s%d:%llu", first ? "" : ",", kv.first, (unsigned long long)kv.second); first = false; }
	std::printf("\n");
	return 0;
}
