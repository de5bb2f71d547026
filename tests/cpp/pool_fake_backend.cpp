// pool_fake_backend.cpp — the pool's schedule (corto_amd/csrc/pool.cpp) on a machine without a GPU (tests/test_pool_schedule_cpu.py).
// Built from pool.cpp, host_probe.cpp, crt_format.cpp and this file alone.  This file DEFINES what the pool calls - the crthip_ctx_* /
// crthip_batch_* entry points it uses, corto_hip's pool_internal.h, and a handful of HIP calls (memory as malloc / free, pointer queries
// answered from a table) - and every definition appends a record to the calling lane's log.  It is a log and a table of answers, not a
// model of the library; it never reaches a HIP runtime.  crthip_probe and the output layout are the real ones (host_probe.cpp).
//   pool_fake_backend CORPUS [--threaded-only] [--dump FILE]
// CORPUS: u32 count, then per blob u32 len + bytes (real .crt blobs).  Every scenario's invariants - stated in pool.cpp, corto_hip.h
// ("Groups", crthip_pool_decode) and DESIGN.md §7 - are asserted from the log; --dump writes the per-lane logs of the single-threaded
// scenarios, pointers as offsets into named blocks, for a byte-for-byte comparison of two builds of pool.cpp.  Prints "pool_fake_backend ok".
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <vector>

#include "../../corto_amd/csrc/pool_internal.h"

static int failures = 0;
static const char *scenario = "";
#define CHECK(c) do { if(!(c)) { std::printf("FAILED %s line %d: %s\n", scenario, __LINE__, #c); failures++; } } while(0)

// ---- the switches of one scenario, the log, the table of memory blocks ----
struct Cfg {
	bool pipelines = true;
	uint32_t carriable_max_blobs = ~0u;   // batch_carriable: the batch has at most this many blobs
	int drain_on = -1;                    // this carrying call (counted from 0) leaves its `next` batch's entropy stage undone
	int device_fault_on = -1;             // this mesh stage (counted from 0) returns CRTHIP_E_DEVICE, once
	const uint8_t *marked = nullptr;      // a batch whose blob list holds it is refused: an item fault
	unsigned poll_seed = 0;               // 0: crthip_batch_done answers 1 at once; else after a small seeded number of polls
	uint32_t group = 0;                   // $CORTO_POOL_GROUP for the pool of this scenario (0: unset, the pool's own G)
	int resident_item = -1;               // this item alone has a device arena: it fits no group of uploaded items
	bool to_host = false;                 // crthip_pool_run with crthip_pool_set_outputs_to_host: every step ends with a D2H copy into the lane's pinned mirror
};
static Cfg g;
static std::atomic<int> g_carries{0}, g_meshes{0};
static std::atomic<uint64_t> g_seq{0};

enum Fn { CTX_CREATE, CTX_DESTROY, SINGLE, PACKED, B_CREATE, B_DESTROY, B_FILL, B_FILL_AT, PARITY, BIND, DECODE, ENTROPY, MESH_NEXT, MESH_ALONE, SYNC, POLL, FILL, D2H,
          DEV_ALLOC, DEV_FREE, PIN_ALLOC, PIN_FREE };
static const char *const FN[] = {"ctx_create", "ctx_destroy", "set_single_stream", "set_packed_host_blobs", "batch_create", "batch_destroy", "batch_fill", "batch_fill_at",
	"set_parity", "bind_all", "decode", "decode_with_next(null,next)", "decode_with_next(cur,next)", "decode_with_next(cur,null)", "sync", "done", "fill_async", "copy_to_host_async",
	"hipMalloc", "hipFree", "hipHostMalloc", "hipHostFree"};
struct Rec { int fn = 0; uint64_t seq = 0; int batch = -1, next = -1, rc = 0; uint32_t nblobs = 0; uint64_t bytes = 0, value = 0; std::vector<const void *> ptr; std::vector<std::string> name; std::vector<uint64_t> num;
             void add(const void *p); };   // a pointer and, for the dump, its name as of now
struct LaneLog { int device = 0; std::vector<Rec> recs; };
static std::vector<LaneLog *> g_lanes;    // in crthip_ctx_create order: the pool's lane order

enum Kind { PLAIN, PINNED, DEVICE };
struct Block { std::string name; uintptr_t base = 0; size_t size = 0; Kind kind = PLAIN; int device = 0; };
static std::mutex g_blocks_m;
static std::map<uintptr_t, Block> g_blocks;
static int g_ndev = 0, g_npin = 0;
static void add_block(const std::string &name, const void *p, size_t size, Kind kind, int device = 0) {
	std::lock_guard<std::mutex> lock(g_blocks_m);
	g_blocks[(uintptr_t)p] = Block{name, (uintptr_t)p, size, kind, device};
}
static bool find_block(const void *p, Block &out) {
	std::lock_guard<std::mutex> lock(g_blocks_m);
	auto it = g_blocks.upper_bound((uintptr_t)p);
	if(it == g_blocks.begin()) return false;
	--it;
	if((uintptr_t)p - it->second.base >= std::max<size_t>(it->second.size, 1)) return false;
	out = it->second;
	return true;
}
static std::string name_of(const void *p) {
	if(!p) return "null";
	Block b;
	if(!find_block(p, b)) return "?";
	return b.name + "+" + std::to_string((uintptr_t)p - b.base);
}

void Rec::add(const void *p) { ptr.push_back(p); name.push_back(name_of(p)); }

struct crthip_ctx { int lane = 0; int device = 0; int nbatch = 0; unsigned rng = 1; };
struct crthip_batch { crthip_ctx *ctx = nullptr; int ord = 0; std::vector<const uint8_t *> blobs; std::vector<uint32_t> lens, nattr;
                      std::vector<void *> first_out; bool entropy_done = false; int polls = 0; };
static thread_local crthip_ctx *t_ctx = nullptr;   // the lane this thread last called: an allocation belongs to its log
static thread_local int t_device = 0;
static Rec &rec(crthip_ctx *c, int fn, const crthip_batch *b = nullptr) {
	t_ctx = c;
	std::vector<Rec> &L = g_lanes[(size_t)c->lane]->recs;
	L.emplace_back();
	L.back().fn = fn; L.back().seq = g_seq++; L.back().batch = b ? b->ord : -1;
	return L.back();
}

// ---- the public calls the pool makes ----
extern "C" int crthip_ctx_create(int device, crthip_ctx **out) {
	crthip_ctx *c = new crthip_ctx();
	c->lane = (int)g_lanes.size(); c->device = device; c->rng = g.poll_seed*2654435761u + (unsigned)c->lane + 1u;
	g_lanes.push_back(new LaneLog()); g_lanes.back()->device = device;
	rec(c, CTX_CREATE).value = (uint64_t)device;
	*out = c;
	return CRTHIP_OK;
}
extern "C" void crthip_ctx_destroy(crthip_ctx *c) { rec(c, CTX_DESTROY); t_ctx = nullptr; delete c; }
extern "C" int crthip_ctx_set_single_stream(crthip_ctx *c, int on) { rec(c, SINGLE).value = (uint64_t)on; return CRTHIP_OK; }
extern "C" int crthip_ctx_set_packed_host_blobs(crthip_ctx *c, int on) { rec(c, PACKED).value = (uint64_t)on; return CRTHIP_OK; }

static int fill(crthip_batch *b, int fn, uint32_t n, const uint8_t *const *blobs, const uint32_t *lens, const void *arena, const uint64_t *dev_off) {
	Rec &r = rec(b->ctx, fn, b);
	r.nblobs = n; r.add(arena);
	b->blobs.assign(blobs, blobs + n); b->lens.assign(lens, lens + n); b->nattr.assign(n, 0); b->first_out.assign(n, nullptr); b->entropy_done = false;
	for(uint32_t i = 0; i < n; i++) {
		r.add(blobs[i]); r.num.push_back(lens[i]); if(dev_off) r.num.push_back(dev_off[i]);
		crthip_blob_info info;
		if(blobs[i] == g.marked || crthip_probe(blobs[i], lens[i], &info) != CRTHIP_OK) { b->blobs.clear(); r.rc = CRTHIP_E_MAGIC; }
		else b->nattr[i] = info.nattr;
	}
	return r.rc ? corto_hip::ctx_fail(r.rc, "fake: a refused blob") : CRTHIP_OK;
}
extern "C" int crthip_batch_create(crthip_ctx *c, uint32_t n, const uint8_t *const *blobs, const uint32_t *lens, const void *arena, crthip_batch **out) {
	crthip_batch *b = new crthip_batch();
	b->ctx = c; b->ord = c->nbatch++;
	rec(c, B_CREATE, b);
	const int err = n ? fill(b, B_FILL, n, blobs, lens, arena, nullptr) : CRTHIP_OK;
	if(err) { c->nbatch--; delete b; return err; }   // (as the real call: no object when the fill fails)
	*out = b;
	return CRTHIP_OK;
}
extern "C" void crthip_batch_destroy(crthip_batch *b) { rec(b->ctx, B_DESTROY, b); delete b; }
extern "C" int crthip_batch_reset(crthip_batch *b, uint32_t n, const uint8_t *const *blobs, const uint32_t *lens, const void *arena) { return fill(b, B_FILL, n, blobs, lens, arena, nullptr); }
int corto_hip::batch_reset_at(crthip_batch *b, uint32_t n, const uint8_t *const *blobs, const uint32_t *lens, const void *base, const uint64_t *dev_off) { return fill(b, B_FILL_AT, n, blobs, lens, base, dev_off); }
extern "C" int crthip_batch_set_parity(crthip_batch *b, uint32_t parity) { rec(b->ctx, PARITY, b).value = parity; return CRTHIP_OK; }
extern "C" uint32_t crthip_batch_size(const crthip_batch *b) { return (uint32_t)b->blobs.size(); }
extern "C" int crthip_batch_info(const crthip_batch *b, uint32_t i, crthip_blob_info *info) { return crthip_probe(b->blobs[i], b->lens[i], info); }
extern "C" int crthip_batch_get_stats(const crthip_batch *, crthip_batch_stats *s) { memset(s, 0, sizeof *s); return CRTHIP_OK; }
extern "C" int crthip_batch_bind_all(crthip_batch *b, const crthip_attr_binding *attrs, void *const *index, const uint32_t *index_format) {
	Rec &r = rec(b->ctx, BIND, b);
	r.nblobs = (uint32_t)b->blobs.size();
	size_t a = 0;
	for(size_t i = 0; i < b->blobs.size(); i++) {
		b->first_out[i] = b->nattr[i] ? attrs[a].buffer : nullptr;
		for(uint32_t k = 0; k < b->nattr[i]; k++, a++) { r.add(attrs[a].buffer); r.num.push_back(attrs[a].format | (uint64_t)attrs[a].out_components << 8); }
		r.add(index[i]); r.num.push_back(index_format[i]);
	}
	return CRTHIP_OK;
}
static uint64_t tag_of(const uint8_t *blob) { return 0x7A6F000000000000ull ^ (uint64_t)(uintptr_t)blob; }
// a mesh stage "runs": every blob leaves its tag at the head of its first output array, so that a mixed-up binding or copy shows
static int mesh_stage(crthip_batch *b, Rec &r) {
	if(g_meshes++ == g.device_fault_on) { r.rc = CRTHIP_E_DEVICE; return corto_hip::ctx_fail(CRTHIP_E_DEVICE, "fake: a device fault"); }
	for(size_t i = 0; i < b->blobs.size(); i++) if(b->first_out[i]) { const uint64_t t = tag_of(b->blobs[i]); memcpy(b->first_out[i], &t, 8); }
	if(g.poll_seed) { b->ctx->rng = b->ctx->rng*1664525u + 1013904223u; b->polls = (int)(b->ctx->rng >> 28 & 3u); }
	return CRTHIP_OK;
}
extern "C" int crthip_batch_decode(crthip_batch *b) { Rec &r = rec(b->ctx, DECODE, b); r.nblobs = (uint32_t)b->blobs.size(); return mesh_stage(b, r); }
extern "C" int crthip_batch_decode_with_next(crthip_batch *cur, crthip_batch *next) {
	Rec &r = rec((cur ? cur : next)->ctx, !cur ? ENTROPY : next ? MESH_NEXT : MESH_ALONE, cur ? cur : next);
	r.nblobs = (uint32_t)(cur ? cur : next)->blobs.size();
	if(cur && next) r.next = next->ord;
	if(next) next->entropy_done = !(cur && g_carries++ == g.drain_on);
	return cur ? mesh_stage(cur, r) : CRTHIP_OK;
}
extern "C" int crthip_batch_sync(crthip_batch *b, int32_t *status) {
	rec(b->ctx, SYNC, b).nblobs = (uint32_t)b->blobs.size();
	for(size_t i = 0; i < b->blobs.size(); i++) status[i] = 0;
	return CRTHIP_OK;
}
extern "C" int crthip_batch_done(crthip_batch *b) {
	const int d = b->polls > 0 ? (b->polls--, 0) : 1;
	rec(b->ctx, POLL, b).value = (uint64_t)d;
	return d;
}

// ---- pool_internal.h ----
bool corto_hip::ctx_pipelines(crthip_ctx *) { return g.pipelines; }
bool corto_hip::batch_carriable(const crthip_batch *b) { return b->blobs.size() <= g.carriable_max_blobs; }
bool corto_hip::batch_entropy_done(const crthip_batch *b) { return b->entropy_done; }
int corto_hip::ctx_fill_async(crthip_ctx *c, void *dst, size_t bytes, int value) {
	Rec &r = rec(c, FILL); r.add(dst); r.bytes = bytes; r.value = (uint64_t)value;
	memset(dst, value, bytes);
	return CRTHIP_OK;
}
int corto_hip::ctx_copy_to_host_async(crthip_ctx *c, void *host_dst, const void *dev_src, size_t bytes) {
	Rec &r = rec(c, D2H); r.add(host_dst); r.add(dev_src); r.bytes = bytes;
	memcpy(host_dst, dev_src, bytes);
	return CRTHIP_OK;
}
bool corto_hip::resident_array_ok(const void *p, uint64_t bytes, uint32_t align, int device) {
	Block b;
	if(!bytes) return true;
	if(!p || ((uintptr_t)p & (align - 1)) || !find_block(p, b)) return false;
	return b.kind == DEVICE && b.device == device && bytes <= b.size && (uintptr_t)p - b.base <= b.size - bytes;
}

// ---- HIP: memory is malloc's, the pointer queries read the table ----
static void *take(const char *prefix, int &count, size_t bytes, Kind kind, int fn) {
	void *p = aligned_alloc(256, (bytes + 255) & ~(size_t)255);
	std::string name;
	{ std::lock_guard<std::mutex> lock(g_blocks_m); name = prefix + std::to_string(count++); }
	add_block(name, p, bytes, kind, t_device);
	if(t_ctx) { Rec &r = rec(t_ctx, fn); r.add(p); r.bytes = bytes; }
	return p;
}
static void give(void *p, int fn) {
	if(t_ctx) rec(t_ctx, fn).add(p);
	{ std::lock_guard<std::mutex> lock(g_blocks_m); g_blocks.erase((uintptr_t)p); }
	free(p);
}
extern "C" hipError_t hipSetDevice(int device) { t_device = device; return hipSuccess; }
extern "C" hipError_t hipGetLastError(void) { return hipSuccess; }
extern "C" hipError_t hipDeviceGetPCIBusId(char *, int, int) { return hipErrorInvalidDevice; }
extern "C" hipError_t hipMalloc(void **p, size_t bytes) { *p = take("dev", g_ndev, bytes, DEVICE, DEV_ALLOC); return hipSuccess; }
extern "C" hipError_t hipFree(void *p) { give(p, DEV_FREE); return hipSuccess; }
extern "C" hipError_t hipHostMalloc(void **p, size_t bytes, unsigned) { *p = take("pin", g_npin, bytes, PINNED, PIN_ALLOC); return hipSuccess; }
extern "C" hipError_t hipHostFree(void *p) { give(p, PIN_FREE); return hipSuccess; }
extern "C" hipError_t hipMemcpy(void *dst, const void *src, size_t bytes, hipMemcpyKind) { memcpy(dst, src, bytes); return hipSuccess; }
extern "C" hipError_t hipPointerGetAttributes(hipPointerAttribute_t *a, const void *p) {
	Block b;
	if(!find_block(p, b) || b.kind == PLAIN) return hipErrorInvalidValue;
	a->type = b.kind == DEVICE ? hipMemoryTypeDevice : hipMemoryTypeHost; a->device = b.device;
	return hipSuccess;
}
extern "C" hipError_t hipMemGetAddressRange(hipDeviceptr_t *base, size_t *size, hipDeviceptr_t p) {
	Block b;
	if(!find_block(p, b)) return hipErrorInvalidValue;
	*base = (hipDeviceptr_t)b.base; *size = b.size;
	return hipSuccess;
}

// ================================================ the scenarios ================================================
static std::vector<std::vector<uint8_t>> corpus;
static FILE *dump = nullptr;
constexpr uint32_t BLOBS = 2, G = 2;      // blobs an item; the group size of pipelined lanes
static uint64_t up(uint64_t x, uint64_t a) { return (x + a - 1) & ~(a - 1); }

enum Mode { PACKED_HOST, RESIDENT, GATHERED };
struct Items {
	uint8_t *host = nullptr, *arena_mem = nullptr;
	std::vector<uint8_t *> arenas, dsts;
	std::vector<const uint8_t *> ptrs; std::vector<uint32_t> lens; std::vector<const void *> arena_of;
	std::vector<crthip_pool_item> items;
	std::vector<crthip_pool_dest> dests;
	std::vector<uint64_t> total; std::vector<std::vector<uint64_t>> tag_at;   // the item's layout total; where blob i's first output array begins
	int empty = -1, truncated = -1, marked = -1;
	Mode mode = PACKED_HOST;
	~Items() { free(host); free(arena_mem); for(uint8_t *d : dsts) free(d); std::lock_guard<std::mutex> lock(g_blocks_m); g_blocks.clear(); }
	int item_of(const void *blob) const { for(size_t j = 0; j < items.size(); j++) for(uint32_t i = 0; i < items[j].nblobs; i++) if(items[j].blobs[i] == blob) return (int)j; return -1; }
};
// n items of BLOBS blobs each, every blob a copy of its own in one host block (adjacent in arena layout: one run an item); decode: with destinations
// that cycle device / pinned / pageable (a slot's device items are drawn first, so the groups of a short list are theirs) or, host_only, pinned / pageable
static void make_items(Items &I, uint32_t n, Mode mode, bool decode, uint32_t ndevices = 1, bool host_only = false) {
	I.mode = mode;
	size_t bytes = 0;
	for(uint32_t k = 0; k < n*BLOBS; k++) bytes += up(corpus[k % corpus.size()].size(), 16);
	I.host = (uint8_t *)aligned_alloc(256, up(bytes, 256));
	add_block("host", I.host, bytes, PINNED);
	I.ptrs.resize(n*BLOBS); I.lens.resize(n*BLOBS); I.arena_of.assign((size_t)n*ndevices, nullptr); I.items.resize(n);
	size_t off = 0;
	for(uint32_t k = 0; k < n*BLOBS; k++) {
		const std::vector<uint8_t> &c = corpus[k % corpus.size()];
		memcpy(I.host + off, c.data(), c.size());
		I.ptrs[k] = I.host + off; I.lens[k] = (uint32_t)c.size(); off += up(c.size(), 16);
	}
	if(decode && n > 15) { I.empty = 9; I.truncated = 11; I.marked = host_only ? 4 : 2; I.lens[(size_t)I.truncated*BLOBS] = 10; g.marked = I.ptrs[(size_t)I.marked*BLOBS]; }
	for(uint32_t j = 0; j < n; j++) {
		I.items[j] = crthip_pool_item{(int)j == I.empty ? 0u : BLOBS, I.ptrs.data() + j*BLOBS, I.lens.data() + j*BLOBS, nullptr};
		if(mode == RESIDENT || (int)j == g.resident_item) {
			// (the arenas are blocks of their own in the table, at fixed distances in one allocation: a group's offsets are the same in every run)
			const size_t ab = up(I.lens[j*BLOBS], 16) + up(I.lens[j*BLOBS + 1], 16), pitch = up(bytes, 256) + 256;
			if(!I.arena_mem) I.arena_mem = (uint8_t *)aligned_alloc(256, pitch*n);
			I.arenas.push_back(I.arena_mem + pitch*j);
			add_block("arena" + std::to_string(j), I.arenas.back(), ab, DEVICE);
			for(uint32_t d = 0; d < ndevices; d++) I.arena_of[(size_t)j*ndevices + d] = I.arenas.back();
			I.items[j].device_arena = I.arena_of.data() + (size_t)j*ndevices;
		}
		uint64_t total = 0;
		std::vector<crthip_out_array> attr(BLOBS*CRTHIP_MAX_ATTRS), index(BLOBS);
		std::vector<uint64_t> at;
		if((int)j != I.truncated && crthip_output_layout(I.items[j].nblobs, I.items[j].blobs, I.items[j].lens, 0, attr.data(), index.data(), &total) == CRTHIP_OK) {
			size_t a = 0;
			for(uint32_t i = 0; i < I.items[j].nblobs; i++) { crthip_blob_info info; crthip_probe(I.items[j].blobs[i], I.items[j].lens[i], &info); at.push_back(attr[a].offset); a += info.nattr; }
		}
		I.total.push_back(total); I.tag_at.push_back(at);
		if(!decode) continue;
		const size_t cap = (size_t)total + 256;
		I.dsts.push_back((uint8_t *)aligned_alloc(256, cap));
		memset(I.dsts.back(), 0xEE, cap);
		const Kind kind = host_only ? (j % 2 ? PINNED : PLAIN) : j % 3 == 0 ? DEVICE : j % 3 == 1 ? PINNED : PLAIN;
		add_block("dst" + std::to_string(j), I.dsts.back(), cap, kind);
		I.dests.push_back(crthip_pool_dest{I.dsts.back(), cap, kind == DEVICE ? (int32_t)(j % ndevices) : CRTHIP_POOL_DEST_HOST, 0});
	}
}

struct Done { uint32_t item, slot; bool tags_ok; };
static std::mutex g_done_m;
static std::vector<Done> g_done;
static bool tags_in(const Items &I, uint32_t j, const uint8_t *block) {
	for(uint32_t i = 0; i < I.items[j].nblobs; i++) { const uint64_t t = tag_of(I.items[j].blobs[i]); if(memcmp(block + I.tag_at[j][i], &t, 8)) return false; }
	return true;
}
static void on_done(void *user, uint32_t item, uint32_t slot, const int32_t *status) {
	const Items &I = *(const Items *)user;
	bool ok = true;                                                   // an item's outputs are final when `done` is called: a pageable destination has its bytes
	if(I.items[item].nblobs && status[0] == 0) ok = tags_in(I, item, (const uint8_t *)I.dests[item].out);
	std::lock_guard<std::mutex> lock(g_done_m);
	g_done.push_back(Done{item, slot, ok});
}

static void print_rec(const Rec &r) {
	std::fprintf(dump, "  %s b%d", FN[r.fn], r.batch);
	if(r.next >= 0) std::fprintf(dump, " next=b%d", r.next);
	std::fprintf(dump, " n=%u rc=%d bytes=%llu v=%llu", r.nblobs, r.rc, (unsigned long long)r.bytes, (unsigned long long)r.value);
	for(const std::string &nm : r.name) std::fprintf(dump, " %s", nm.c_str());
	for(uint64_t v : r.num) std::fprintf(dump, " %llu", (unsigned long long)v);
	std::fprintf(dump, "\n");
}
static uint64_t g_dumped = 0;
static void dump_lanes() {
	if(!dump) return;
	for(size_t l = 0; l < g_lanes.size(); l++) {
		std::fprintf(dump, " lane %zu\n", l);
		for(const Rec &r : g_lanes[l]->recs) { print_rec(r); g_dumped++; }
	}
}

// ---- the invariants, from the log ----
struct Expect {
	const Items *I = nullptr;
	uint32_t lanes = 3, group = G;
	bool pipelined = true, decode = false, to_host = false, faulted = false, ordered = true;   // ordered: one thread, so the records' order is the tickets'
	uint64_t total = 0, poison_from = ~0ull, stride = 0;
};
struct BatchState { bool planned = false, staged = false, inflight = false, ran = false, synced = false; std::vector<int> items; uint64_t last_step = 0; };
struct Counts { uint64_t synced_members = 0, grouped = 0, meshes = 0, refused_groups = 0; std::map<int, int> launches; };

static bool is_fill(const Rec &r) { return (r.fn == B_FILL || r.fn == B_FILL_AT) && r.nblobs; }
static void check_lanes(const Expect &E, Counts &C) {
	const Items &I = *E.I;
	// one thread: the successful plans in call order carry the tickets in draw order, so a batch's last step number is a running count
	std::map<uint64_t, uint64_t> last_step;
	std::set<int> solo, drawn;
	if(E.ordered) {
		std::vector<const Rec *> fills;
		for(LaneLog *L : g_lanes) for(const Rec &r : L->recs) if(is_fill(r)) fills.push_back(&r);
		std::sort(fills.begin(), fills.end(), [](const Rec *a, const Rec *b) { return a->seq < b->seq; });
		uint64_t steps = 0;
		for(const Rec *r : fills) {
			const uint32_t members = r->nblobs/BLOBS;
			if(!r->rc) { steps += members; last_step[r->seq] = steps - 1; }
			if(!E.decode) continue;
			// no extra ticket is drawn once fewer than 2 x lanes x G are undrawn (the items that launch nothing are drawn behind the groups here)
			std::set<int> fresh;
			for(uint32_t i = 0; i < r->nblobs; i += BLOBS) { const int j = I.item_of(r->ptr[1 + i]); if(!drawn.count(j)) fresh.insert(j); }
			if(fresh.size() > 1) CHECK(E.total - (drawn.size() + fresh.size() - 1) >= 2ull*E.lanes*E.group);
			drawn.insert(fresh.begin(), fresh.end());
		}
	}
	for(size_t l = 0; l < g_lanes.size(); l++) {
		const std::vector<Rec> &R = g_lanes[l]->recs;
		std::map<int, BatchState> B;
		const void *out = nullptr, *mirror = nullptr;
		bool first_plan = true;
		auto busy = [&] { for(auto &kv : B) if(kv.second.inflight || kv.second.staged) return true; return false; };
		auto inflight = [&] { for(auto &kv : B) if(kv.second.inflight) return true; return false; };
		for(size_t k = 0; k < R.size(); k++) {
			const Rec &r = R[k];
			BatchState &S = B[r.batch];
			switch(r.fn) {
			case B_FILL: case B_FILL_AT: {
				if(!r.nblobs) break;
				CHECK(!S.inflight && !S.staged);
				S.planned = false; S.ran = false; S.synced = false; S.items.clear();
				CHECK(r.nblobs % BLOBS == 0);
				for(uint32_t i = 0; i < r.nblobs; i++) { const int j = I.item_of(r.ptr[1 + i]); CHECK(j >= 0 && r.ptr[1 + i] == I.items[j].blobs[i % BLOBS]); if(i % BLOBS == 0) S.items.push_back(j); }
				const size_t n = S.items.size();
				CHECK(n >= 1 && n <= E.group);                            // a group never exceeds G members,
				for(int j : S.items) CHECK(!I.items[j].device_arena == !I.items[S.items[0]].device_arena);   // which are all resident or all uploaded,
				CHECK((r.fn == B_FILL_AT) == (n > 1 && I.items[S.items[0]].device_arena));
				if(n > 1) CHECK(I.mode != GATHERED && n <= 8);            // in no more than 8 runs (one an item here; gathered blobs count 9),
				if(n > 1) for(int j : S.items) CHECK(!solo.count(j));     // and none of them a refused group's member;
				if(E.pipelined && first_plan) CHECK(n == 1);               // a pipelined lane's first batch of a run is one item
				first_plan = false;
				if(r.rc && n > 1) { C.refused_groups++; for(int j : S.items) solo.insert(j); }
				if(r.rc) CHECK(E.decode && std::count(S.items.begin(), S.items.end(), I.marked));
				if(!r.rc && E.ordered) S.last_step = last_step[r.seq];
				break; }
			case BIND: {
				CHECK(!S.inflight && !S.staged && out);
				S.planned = true;
				size_t a = 0;                                              // member k's bindings lie k strides into the lane's block, or in the item's device destination
				for(uint32_t i = 0; i < r.nblobs; i++) {
					const int j = S.items[i/BLOBS];
					const bool to_dev = E.decode && I.dests[j].device_slot >= 0;
					const uint8_t *base = to_dev ? (const uint8_t *)I.dests[j].out : (const uint8_t *)out + (i/BLOBS)*E.stride;
					crthip_blob_info info; crthip_probe(I.items[j].blobs[i % BLOBS], I.items[j].lens[i % BLOBS], &info);
					CHECK(r.ptr[a] == base + I.tag_at[j][i % BLOBS]);
					for(uint32_t q = 0; q <= info.nattr; q++, a++) if(r.ptr[a]) CHECK((const uint8_t *)r.ptr[a] >= base && (const uint8_t *)r.ptr[a] < base + I.total[j]);
				}
				break; }
			case DEV_ALLOC: CHECK(!busy()); out = r.ptr[0]; break;     // the output block is never freed or reallocated under a busy lane or a staged batch
			case DEV_FREE: CHECK(!busy()); out = nullptr; break;
			case PIN_ALLOC: mirror = r.ptr[0]; break;
			case FILL:
				CHECK(!E.decode && r.ptr[0] == out && r.value == 0xA5);
				CHECK(k + 1 < R.size() && (R[k + 1].fn == DECODE || R[k + 1].fn == MESH_NEXT || R[k + 1].fn == MESH_ALONE));
				break;
			case ENTROPY: CHECK(E.pipelined && S.planned && !S.staged && !S.inflight && !S.ran); S.staged = true; break;
			case DECODE: case MESH_NEXT: case MESH_ALONE: {
				CHECK(S.planned && !inflight());                           // at most one mesh stage between two syncs
				if(r.fn == DECODE) CHECK(!S.staged); else CHECK(E.pipelined);
				const bool poisoned = k > 0 && R[k - 1].fn == FILL;
				if(E.ordered && !E.decode) CHECK(poisoned == (S.ran || S.last_step >= E.poison_from));   // a fill precedes every mesh stage whose step is >= poison_from, and a repeat
				S.staged = false;
				if(!r.rc) { S.inflight = true; S.ran = true; C.meshes++; for(int j : S.items) C.launches[j]++; }
				if(r.fn == MESH_NEXT) { BatchState &N = B[r.next]; CHECK(N.planned && !N.staged && !N.inflight && !N.ran); N.staged = true; }
				// one copy a host-bound member behind the stage: its destination (or the lane's pinned mirror), its place in the block, its bytes
				size_t c = k + 1;
				for(size_t m = 0; m < S.items.size() && (E.decode || E.to_host) && !r.rc; m++) {
					const int j = S.items[m];
					if(E.decode && I.dests[j].device_slot >= 0) continue;
					Block blk; const bool pinned = E.decode && find_block(I.dests[j].out, blk) && blk.kind == PINNED;
					CHECK(c < R.size() && R[c].fn == D2H);
					if(c < R.size() && R[c].fn == D2H) {
						CHECK(R[c].ptr[0] == (pinned ? (const uint8_t *)I.dests[j].out : (const uint8_t *)mirror + m*E.stride));
						CHECK(R[c].ptr[1] == (const uint8_t *)out + m*E.stride && R[c].bytes == I.total[j]);
					}
					c++;
				}
				CHECK(c >= R.size() || R[c].fn != D2H);
				break; }
			case D2H: CHECK(inflight()); break;
			case SYNC:
				CHECK(S.inflight); S.inflight = false;
				if(!S.synced) C.synced_members += S.items.size();      // (a repeat from a poisoned block is a sync of its own and nobody's step)
				S.synced = true;
				if(S.items.size() > 1) C.grouped += S.items.size();
				break;
			case B_DESTROY: CHECK(!S.inflight); break;
			default: break;
			}
		}
		// every planned batch is decoded and synced before the call returns (a device fault: what is in flight is still synced)
		for(auto &kv : B) { CHECK(!kv.second.inflight); if(!E.faulted) CHECK(!kv.second.staged && (!kv.second.planned || kv.second.ran)); }
	}
}

static crthip_pool *make_pool(uint32_t ndevices, uint32_t threads, Mode mode) {
	if(g.group) setenv("CORTO_POOL_GROUP", std::to_string(g.group).c_str(), 1); else unsetenv("CORTO_POOL_GROUP");   // (read by crthip_pool_create)
	for(LaneLog *L : g_lanes) delete L;
	g_lanes.clear(); g_ndev = g_npin = 0; g_carries = 0; g_meshes = 0; g_done.clear();
	static const int devs[2] = {0, 0};
	crthip_pool *p = nullptr;
	CHECK(crthip_pool_create(ndevices, devs, threads, 3, &p) == CRTHIP_OK && crthip_pool_lanes(p) == ndevices*threads*3);
	CHECK(crthip_pool_set_packed_host_blobs(p, mode != GATHERED) == CRTHIP_OK);
	CHECK(crthip_pool_set_outputs_to_host(p, g.to_host) == CRTHIP_OK);
	return p;
}
static void begin(const char *name, const Cfg &cfg) { scenario = name; g = cfg; if(dump) std::fprintf(dump, "== %s\n", name); }

static void run_scenario(const char *name, Cfg cfg, Mode mode, uint32_t ndevices = 1, uint32_t threads = 1) {
	begin(name, cfg);
	const bool ordered = ndevices*threads == 1;
	const uint32_t lanes = ndevices*threads*3, nitems = 3;
	const uint64_t warmup = 5, steps = 4*3*2 + 1;
	crthip_pool *p = make_pool(ndevices, threads, mode);
	Items I;
	make_items(I, nitems, mode, false, ndevices);
	crthip_pool_report rep;
	std::vector<double> completion(steps);
	CHECK(crthip_pool_run(p, nitems, I.items.data(), steps, warmup, &rep, completion.data()) == CRTHIP_OK);
	Expect E;
	E.I = &I; E.lanes = lanes; E.pipelined = cfg.pipelines; E.group = cfg.pipelines ? G : 1; E.ordered = ordered;
	E.to_host = cfg.to_host;
	E.total = warmup + steps + lanes*(cfg.pipelines ? 2u : 1u); E.poison_from = cfg.to_host ? warmup + steps : warmup + steps - lanes;   // (to the host: the tail only)
	uint64_t need = 0;
	for(uint64_t t : I.total) need = std::max(need, t + 256);
	E.stride = up(need, 256);
	Counts C;
	check_lanes(E, C);
	// completed == total, and the report agrees with the log (a repeat from a poisoned block is a sync of its own, nobody's step)
	CHECK((ordered ? C.synced_members == E.total : C.synced_members >= E.total) && rep.steps == steps && rep.failed_blobs == 0 && rep.first_error == 0);
	uint64_t per_dev = 0;
	for(uint32_t d = 0; d < ndevices; d++) per_dev += rep.steps_per_device[d];
	CHECK(per_dev == steps && rep.grouped_steps == C.grouped && rep.poisoned_lanes == lanes);
	if(mode == GATHERED || !cfg.pipelines) CHECK(C.grouped == 0); else if(ordered && cfg.carriable_max_blobs == ~0u) CHECK(C.grouped > 0);
	if(dump && ordered) {
		dump_lanes();
		std::fprintf(dump, " report steps=%llu tris=%llu verts=%llu failed=%llu used=%u per_dev0=%llu poisoned=%u grouped=%llu\n", (unsigned long long)rep.steps, (unsigned long long)rep.triangles,
			(unsigned long long)rep.vertices, (unsigned long long)rep.failed_blobs, rep.devices_used, (unsigned long long)rep.steps_per_device[0], rep.poisoned_lanes, (unsigned long long)rep.grouped_steps);
	}
	// what every lane holds afterwards: its last item's arrays, by the sizes of the output layout, and a poisoned tail
	for(uint32_t l = 0; l < lanes; l++) {
		uint32_t slot = 99;
		const int64_t j = crthip_pool_lane_item(p, l, &slot);
		CHECK(j >= 0 && j < nitems && slot == l/(threads*3));
		std::vector<uint8_t> buf(1 << 16);
		for(uint32_t b = 0; b < BLOBS && j >= 0; b++) {
			const uint64_t t = tag_of(I.items[(size_t)j].blobs[b]);
			int tagged = 0;                                               // the blob's first array (whichever attribute that is) begins with its tag
			for(const char *what : {"position", "normal", "color", "uv", "index", "#tail"}) {
				const int64_t n = crthip_pool_lane_read(p, l, b, what, buf.data(), buf.size());
				if(dump && ordered) std::fprintf(dump, " lane_read %u %u %s %lld\n", l, b, what, (long long)n);
				if(n >= 8 && !memcmp(buf.data(), &t, 8)) tagged++;
				if(!strcmp(what, "position")) CHECK(n >= 12);
				if(!strcmp(what, "#tail")) CHECK(n == 256 && buf[0] == 0xA5 && buf[255] == 0xA5);
			}
			CHECK(tagged == 1);
		}
	}
	crthip_pool_destroy(p);
}

static void decode_scenario(const char *name, Cfg cfg, uint32_t nitems, uint32_t ndevices = 1, uint32_t threads = 1, bool host_only = false) {
	begin(name, cfg);
	const bool ordered = ndevices*threads == 1;
	const uint32_t lanes = ndevices*threads*3;
	crthip_pool *p = make_pool(ndevices, threads, PACKED_HOST);
	Items I;
	make_items(I, nitems, PACKED_HOST, true, ndevices, host_only);    // (sets g.marked)
	size_t nstatus = 0;
	for(auto &it : I.items) nstatus += it.nblobs;
	std::vector<int32_t> status(nstatus, 0x7777);
	crthip_pool_report rep;
	const int rc = crthip_pool_decode(p, nitems, I.items.data(), I.dests.data(), status.data(), on_done, &I, &rep);
	Expect E;
	E.I = &I; E.lanes = lanes; E.pipelined = cfg.pipelines; E.group = cfg.group ? cfg.group : cfg.pipelines ? G : 1; E.ordered = ordered; E.decode = true; E.total = nitems;
	E.faulted = cfg.device_fault_on >= 0;
	uint64_t need = 0;
	for(uint32_t j = 0; j < nitems; j++) if(I.dests[j].device_slot < 0) need = std::max(need, I.total[j]);
	E.stride = up(need, 256);
	Counts C;
	check_lanes(E, C);
	if(E.faulted) {
		// the call returns the code and hands out no further ticket: nothing is planned behind the faulting stage
		CHECK(rc == CRTHIP_E_DEVICE);
		uint64_t fault_seq = ~0ull, last_plan = 0;
		for(LaneLog *L : g_lanes) for(const Rec &r : L->recs) { if(r.rc == CRTHIP_E_DEVICE) fault_seq = r.seq; if(is_fill(r)) last_plan = std::max(last_plan, r.seq); }
		CHECK(fault_seq != ~0ull && last_plan < fault_seq);
	} else {
		CHECK(rc == CRTHIP_OK && rep.steps == nitems);
		// every item is settled exactly once: one `done`, its outputs final by then, every status entry written, launched once unless it cannot launch
		std::vector<int> dones(nitems, 0);
		for(const Done &d : g_done) { dones[d.item]++; CHECK(d.tags_ok && d.slot < ndevices); if(I.dests[d.item].device_slot >= 0) CHECK((int32_t)d.slot == I.dests[d.item].device_slot); }
		size_t at = 0;
		uint64_t per_dev = 0, failed = 0;
		for(uint32_t j = 0; j < nitems; j++) {
			const int32_t want = (int)j == I.truncated ? CRTHIP_E_TRUNCATED : (int)j == I.marked ? CRTHIP_E_MAGIC : 0;
			CHECK(dones[j] == 1);
			for(uint32_t i = 0; i < I.items[j].nblobs; i++, at++) { CHECK(status[at] == want); if(want) failed++; }
			const bool launches = !want && I.items[j].nblobs;
			CHECK(C.launches[(int)j] == (launches ? 1 : 0));
			if(launches) CHECK(tags_in(I, j, I.dsts[j])); else CHECK(I.dsts[j][0] == 0xEE && I.dsts[j][I.total[j] ? I.total[j] - 1 : 0] == 0xEE);   // a failed item's destination is not written
			CHECK(I.dsts[j][I.total[j]] == 0xEE);                        // nor anything behind an item's total
		}
		for(uint32_t d = 0; d < ndevices; d++) per_dev += rep.steps_per_device[d];
		CHECK(per_dev == nitems && rep.failed_blobs == failed && rep.grouped_steps == C.grouped && rep.poisoned_lanes == 0);
		CHECK((rep.first_error != 0) == (failed != 0));
		if(nitems < 2*lanes*E.group || !cfg.pipelines) CHECK(C.grouped == 0); else if(!cfg.group) CHECK(C.grouped > 0);
		if(host_only && ordered) CHECK(C.refused_groups == 1 && (cfg.group || C.grouped == 2));
	}
	if(dump && ordered) {
		dump_lanes();
		std::fprintf(dump, " rc=%d report steps=%llu tris=%llu verts=%llu failed=%llu first_error=%d per_dev0=%llu grouped=%llu\n status", rc, (unsigned long long)rep.steps, (unsigned long long)rep.triangles,
			(unsigned long long)rep.vertices, (unsigned long long)rep.failed_blobs, rep.first_error, (unsigned long long)rep.steps_per_device[0], (unsigned long long)rep.grouped_steps);
		for(int32_t s : status) std::fprintf(dump, " %d", s);
		std::fprintf(dump, "\n done");
		for(const Done &d : g_done) std::fprintf(dump, " %u@%u", d.item, d.slot);
		std::fprintf(dump, "\n");
	}
	CHECK(crthip_pool_lane_item(p, 0, nullptr) == -1);
	crthip_pool_destroy(p);
}

int main(int argc, char **argv) {
	if(argc < 2) { std::fprintf(stderr, "usage: pool_fake_backend CORPUS [--threaded-only] [--dump FILE]\n"); return 2; }
	bool threaded_only = false;
	for(int a = 2; a < argc; a++) { if(!strcmp(argv[a], "--threaded-only")) threaded_only = true; else if(!strcmp(argv[a], "--dump") && a + 1 < argc) dump = std::fopen(argv[++a], "w"); }
	// crthip_pool_create reads two variables of the environment.  They are only REMOVED here, for this process, which has no GPU and starts no
	// other: with neither set, 3 lanes stand against the default of 4 queues and are single-stream contexts, and G = 2 where they pipeline
	unsetenv("GPU_MAX_HW_QUEUES"); unsetenv("CORTO_POOL_GROUP");
	FILE *f = std::fopen(argv[1], "rb");
	if(!f) { std::perror(argv[1]); return 2; }
	uint32_t n = 0;
	if(std::fread(&n, 4, 1, f) != 1) return 2;
	for(uint32_t i = 0; i < n; i++) {
		uint32_t len = 0;
		if(std::fread(&len, 4, 1, f) != 1) return 2;
		corpus.emplace_back(len);
		if(len && std::fread(corpus.back().data(), 1, len, f) != len) return 2;
	}
	std::fclose(f);

	Cfg plain, serial, solo_only, drain, fault, polled, to_host, three;
	three.group = 3; three.resident_item = 5;
	to_host.to_host = true;
	serial.pipelines = false;
	solo_only.carriable_max_blobs = BLOBS;                             // single items carry, groups do not
	drain.drain_on = 3;
	fault.device_fault_on = 4;
	polled.poll_seed = 7;
	int scenarios = 0;
	if(!threaded_only) {
		run_scenario("run, non-pipelined", serial, PACKED_HOST); scenarios++;
		run_scenario("run, pipelined, packed", plain, PACKED_HOST); scenarios++;
		run_scenario("run, pipelined, resident", plain, RESIDENT); scenarios++;
		run_scenario("run, pipelined, gathered", plain, GATHERED); scenarios++;
		run_scenario("run, outputs to host", to_host, PACKED_HOST); scenarios++;
		decode_scenario("decode, 7 items", plain, 7); scenarios++;
		run_scenario("run, groups not carriable", solo_only, PACKED_HOST); scenarios++;
		decode_scenario("decode, groups not carriable", solo_only, 17); scenarios++;
		run_scenario("run, a batch drained", drain, PACKED_HOST); scenarios++;
		decode_scenario("decode, a batch drained", drain, 17); scenarios++;
		decode_scenario("decode, a device fault", fault, 17); scenarios++;
		decode_scenario("decode, non-pipelined", serial, 17); scenarios++;
	}
	decode_scenario("decode, 17 items", plain, 17); scenarios++;
	// (a lane's first batch is one item, so of 17 tickets only the fifth and sixth can share a call; 12 + 7 give two groups: the one with the marked
	// blob is refused and planned member by member, the other has a pinned and a pageable member)
	decode_scenario("decode, 19 host items", plain, 19, 1, 1, true); scenarios++;
	// G = 3 (threshold 18, so 25 items): tickets 3 and 4 gather, ticket 5 is resident and waits in `held`; the group is refused for ticket 4's marked
	// blob and its members wait behind ticket 5, solo: ticket 5 is then planned alone - the one order of `held` in which a solo ticket stands behind
	// a ticket that could head a group.  (Here the residency rule would keep them apart as well: with two blobs an item no group overflows its runs)
	if(!threaded_only) { decode_scenario("decode, G = 3, a solo ticket behind a held one", three, 25, 1, 1, true); scenarios++; }
	decode_scenario("decode, threaded", polled, 40, 2, 2); scenarios++;
	run_scenario("run, threaded", polled, PACKED_HOST, 2, 2); scenarios++;
	if(dump) { std::fprintf(dump, "== %llu records\n", (unsigned long long)g_dumped); std::fclose(dump); }
	if(failures) { std::printf("pool_fake_backend: %d failures\n", failures); return 1; }
	std::printf("pool_fake_backend ok: %d scenarios\n", scenarios);
	return 0;
}
