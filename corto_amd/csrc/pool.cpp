// pool.cpp — the multi-GPU decode pool of include/corto_hip.h: a list of independent batches of .crt blobs
// decoded by every GPU of the node, one shared work queue, no collective.  Built on the public C ABI (crthip_ctx / crthip_batch_*), the
// few helpers of pool_internal.h and hipMalloc for the lanes' output blocks: tests/cpp/pool_fake_backend.cpp stands in for all three.
//
// Reference anchor: independent crt::Decoder objects, src/decoder.cpp:126-196 (nothing shared between two decodes).
#include <cstdlib>
#include <hip/hip_runtime.h>
#include <pthread.h>
#include <sched.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/corto_hip.h"
#include "output_layout.h"
#include "pool_internal.h"

using corto_hip::ctx_fail;

namespace {

// One item of a group: a Slot's batch object decodes up to `group` items (crthip_pool) as ONE batch, their blobs concatenated, first member first
struct Member {
	int64_t item = -1;              // the item
	uint64_t step = 0;              // its global step number
	uint32_t first = 0, nblobs = 0; // its blobs in the batch object
	uint8_t *base = nullptr;        // the block its bindings point into: the lane's `out` + lane_off, or (crthip_pool_decode) the item's device destination
	size_t lane_off = 0;            // member k's place in the lane's block (and its pinned mirror): k strides in
	size_t out_used = 0;            // a member that ends with a D2H copy: the first out_used bytes of its part of the lane's block are copied behind the decode
	bool to_host = false;           // ... it does: crthip_pool_set_outputs_to_host, or a host destination
	void *pinned_dst = nullptr;     // crthip_pool_decode: the copy goes straight here (a pinned destination); else into the lane's pinned mirror,
	void *pageable_dst = nullptr;   // ... from where the worker moves it here when it harvests the step
};
struct Ticket { uint32_t j = 0; uint64_t step = 0; bool solo = false; };   // a drawn item; solo: it was in a group that could not be planned and is planned alone
struct Slot {                       // a batch object and the group of items it is planned for
	crthip_batch *batch = nullptr;
	std::vector<Member> mem;
	std::vector<const uint8_t *> gblobs; std::vector<uint32_t> glens; std::vector<uint64_t> goff;   // a group of several: its members' blob lists, joined
	// bindings of the items the batch object is planned for
	std::vector<crthip_attr_binding> binds;
	std::vector<void *> index_ptr;
	std::vector<uint32_t> index_fmt;
	std::vector<uint32_t> first_attr;            // first binding entry of blob i
	std::vector<int32_t> status;
	int64_t item = -1;              // member 0's item (-1: planned for nothing)
	uint64_t step = 0;              // the LAST member's global step number (the highest)
};
// One context = one call in flight.  A pipelined lane (crthip_batch_decode_with_next) holds TWO batch objects and one output block: s[cur] is the
// batch whose mesh stage is in flight or ran last - the only one that writes `out` - and, `staged`, s[cur ^ 1] the next one, planned, uploaded and
// with its entropy stage carried by the same call.  Any other lane uses s[cur] alone.
struct Lane {
	uint32_t slot = 0;              // pool device index
	int device = 0;
	crthip_ctx *ctx = nullptr;
	Slot s[2]; uint32_t cur = 0; bool staged = false;
	// A lane pipelines only while it pays: `pipe` - the batch it decoded last could be carried and could carry (a lane starts every run one batch a
	// call); `drain` - the call just enqueued could NOT carry the planned batch, which then runs alone, whole, and the lane is back to one batch a call
	bool pipe = false, drain = false;
	// ... and groups only while that pays: `single_ok` - the last batch of ONE item it decoded was carriable (a pipelined lane's first batch of a run is
	// one item, so it knows); `alone` - a group then came out not carriable (two items' dictionaries can be too many): one item a call for the rest of the run
	bool single_ok = false, alone = false;
	void *out = nullptr; size_t out_cap = 0;
	void *host_out = nullptr; size_t host_cap = 0;   // outputs_to_host: the pinned mirror of `out`
	bool busy = false;
	bool poisoned = false;          // the output block was filled with POISON on the context's stream right before the mesh stage in flight / last executed
	void begin_run() {                  // (an item id means this call's items[] only; `poisoned` a mesh stage of this run)
		busy = staged = poisoned = pipe = drain = single_ok = alone = false;
		for(Slot &S : s) { S.item = -1; S.binds.clear(); S.mem.clear(); }
	}
};
constexpr int POISON = 0xA5;
constexpr uint32_t GROUP_MAX = 4;   // the most items a lane call decodes as one batch object ($CORTO_POOL_GROUP)

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

} // namespace

struct crthip_pool {
	uint32_t ndevices = 0, threads_per_device = 0, depth = 0;
	std::vector<int> devices;
	std::vector<Lane> lanes;        // [device][thread][depth]
	std::vector<std::vector<int>> cpus;   // per pool device: the host CPUs of the GPU's NUMA node (empty: unknown, threads are not pinned)
	std::string warning;            // what crthip_pool_create had to say about hardware queues (empty: nothing)
	bool render = false;            // crthip_pool_set_render_layouts: int16 normals, uint16 index where the blob's vertex ids fit
	bool to_host = false;           // crthip_pool_set_outputs_to_host: every step ends with a D2H copy of its outputs into the lane's pinned block
	bool pipelined = false;         // every lane is a single-stream context and $CORTO_CARRY is not 0: the lanes run two batches each (Lane)
	// Items a lane call decodes as one batch object.  A hardware queue runs one kernel at a time and a launch lasts as long as its slowest blob's
	// chain, whatever the number of blobs: lanes that share queues pay a launch set's queue time once per GROUP (profiles/pool_group.md).  2 where
	// the lanes are pipelined (they outnumber the queues), else 1; $CORTO_POOL_GROUP = 1 .. 4 overrides
	uint32_t group = 1;
	bool packed = false;            // crthip_pool_set_packed_host_blobs: the contexts upload runs of adjacent host blobs in place
	size_t out_need = 0;            // the largest output block any item of the run asks for: a pipelined lane's block is not moved under a planned batch
	bool decoded = false;           // the last call was crthip_pool_decode: the lanes hold nothing for crthip_pool_lane_item / _read
	// state of one run
	std::atomic<uint64_t> next{0}, completed{0};
	std::mutex m;
	int error = CRTHIP_OK; std::string error_msg;
};

static void destroy_lane(Lane &L) {
	(void)hipSetDevice(L.device);
	for(Slot &S : L.s) { if(S.batch) crthip_batch_destroy(S.batch); S.batch = nullptr; }
	if(L.ctx) crthip_ctx_destroy(L.ctx);
	if(L.out) (void)hipFree(L.out);
	if(L.host_out) (void)hipHostFree(L.host_out);
	L.ctx = nullptr; L.out = nullptr; L.out_cap = 0; L.host_out = nullptr; L.host_cap = 0;
}

// the host CPUs next to a GPU: PCI bus id -> /sys/bus/pci/devices/<id>/numa_node -> /sys/devices/system/node/node<N>/cpulist (empty: unknown)
static std::vector<int> numa_cpus(int device) {
	std::vector<int> cpus; char bus[64] = {0};
	if(hipDeviceGetPCIBusId(bus, (int)sizeof bus, device) != hipSuccess) { (void)hipGetLastError(); return cpus; }
	for(char *c = bus; *c; c++) if(*c >= 'A' && *c <= 'F') *c = (char)(*c - 'A' + 'a');
	char path[192]; int node = -1;
	snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/numa_node", bus);
	if(FILE *f = fopen(path, "r")) { if(fscanf(f, "%d", &node) != 1) node = -1; fclose(f); }
	if(node < 0) return cpus;
	snprintf(path, sizeof path, "/sys/devices/system/node/node%d/cpulist", node);
	if(FILE *f = fopen(path, "r")) {
		int a, b; char sep;
		while(fscanf(f, "%d", &a) == 1) {
			b = a;
			if(fscanf(f, "%c", &sep) == 1 && sep == '-') { if(fscanf(f, "%d", &b) != 1) b = a; if(fscanf(f, "%c", &sep) != 1) sep = 0; }
			for(int c = a; c <= b && c < CPU_SETSIZE; c++) cpus.push_back(c);
			if(sep != ',') break;
		}
		fclose(f);
	}
	return cpus;
}

extern "C" int crthip_pool_create(uint32_t ndevices, const int *devices, uint32_t threads_per_device, uint32_t depth, crthip_pool **out) {
	if(!out || ndevices == 0 || ndevices > 16 || threads_per_device == 0 || depth == 0 || threads_per_device*depth > 64) return ctx_fail(CRTHIP_E_ARGUMENT, nullptr);
	crthip_pool *p = new crthip_pool();
	p->ndevices = ndevices; p->threads_per_device = threads_per_device; p->depth = depth;
	for(uint32_t d = 0; d < ndevices; d++) p->devices.push_back(devices ? devices[d] : (int)d);
	p->lanes.resize((size_t)ndevices*threads_per_device*depth);
	uint32_t hw_queues = 4;                                      // ROCm's default
	bool hw_queues_set = false;
	{ const char *e = getenv("GPU_MAX_HW_QUEUES"); if(e && atoi(e) > 0) { hw_queues = (uint32_t)atoi(e); hw_queues_set = true; } }
	// contexts per PHYSICAL device: a device id may repeat (several pool devices on one GPU), and it is the GPU's hardware queues
	// that the contexts' streams share
	std::map<int, uint32_t> ctx_per_gpu;
	for(uint32_t d = 0; d < ndevices; d++) ctx_per_gpu[p->devices[d]] += threads_per_device*depth;
	for(size_t i = 0; i < p->lanes.size(); i++) {
		Lane &L = p->lanes[i];
		L.slot = (uint32_t)(i/((size_t)threads_per_device*depth)); L.device = p->devices[L.slot];
		int err = crthip_ctx_create(L.device, &L.ctx);
		// two HIP streams per context only while every stream of the GPU gets a hardware queue of its own (corto_hip.h).  A single-stream
		// context never makes its second stream, and the runtime gives each new stream the queue with the fewest streams: lanes made in
		// [device][thread][depth] order take the queues in turn, so a thread's batches in flight sit on different queues and every queue
		// carries about as many lanes (profiles/r08_what_was_measured.txt)
		if(!err && 2*ctx_per_gpu[L.device] > hw_queues) err = crthip_ctx_set_single_stream(L.ctx, 1);   // (+ the LDS-lean normals, profiles/r08_what_was_measured.txt)
		if(err) { for(auto &x : p->lanes) destroy_lane(x); delete p; return err; }
	}
	p->pipelined = true;
	for(auto &L : p->lanes) p->pipelined = p->pipelined && corto_hip::ctx_pipelines(L.ctx);
	p->group = p->pipelined ? 2u : 1u;
	{ const char *e = getenv("CORTO_POOL_GROUP"); if(e && atoi(e) >= 1 && atoi(e) <= (int)GROUP_MAX) p->group = (uint32_t)atoi(e); }
	for(auto &kv : ctx_per_gpu)
		if(kv.second > hw_queues && p->warning.empty()) {
			char buf[320];
			snprintf(buf, sizeof buf, "corto_hip pool: %u contexts on GPU %d but %u hardware queues (%s): streams that share a queue serialise each other's kernels; "
			         "export GPU_MAX_HW_QUEUES=%u before the process first touches HIP", kv.second, kv.first, hw_queues,
			         hw_queues_set ? "GPU_MAX_HW_QUEUES" : "ROCm's default; GPU_MAX_HW_QUEUES is not set", kv.second > 20 ? 20u : kv.second);   // (20 contexts on 20 queues measured best; 24 on 24 is slower)
			p->warning = buf;
			fprintf(stderr, "%s\n", buf);
		}
	for(uint32_t d = 0; d < ndevices; d++) p->cpus.push_back(numa_cpus(p->devices[d]));
	*out = p;
	return CRTHIP_OK;
}

extern "C" void crthip_pool_destroy(crthip_pool *p) {
	if(!p) return;
	for(auto &L : p->lanes) destroy_lane(L);
	delete p;
}

extern "C" uint32_t crthip_pool_lanes(const crthip_pool *p) { return p ? (uint32_t)p->lanes.size() : 0; }
extern "C" const char *crthip_pool_warning(const crthip_pool *p) { return p ? p->warning.c_str() : ""; }
extern "C" int64_t crthip_pool_device_cpus(const crthip_pool *p, uint32_t device_slot, int32_t *cpus, size_t cap) {
	if(!p || device_slot >= p->ndevices) return ctx_fail(CRTHIP_E_ARGUMENT, nullptr);
	const std::vector<int> &c = p->cpus[device_slot];
	for(size_t i = 0; i < c.size() && i < cap && cpus; i++) cpus[i] = c[i];
	return (int64_t)c.size();
}
extern "C" int crthip_pool_set_outputs_to_host(crthip_pool *p, int on) {
	if(!p) return ctx_fail(CRTHIP_E_ARGUMENT, nullptr);
	p->to_host = on != 0;
	return CRTHIP_OK;
}
extern "C" int crthip_pool_set_render_layouts(crthip_pool *p, int on) {
	if(!p) return ctx_fail(CRTHIP_E_ARGUMENT, nullptr);
	p->render = on != 0;
	for(auto &L : p->lanes) for(Slot &S : L.s) { S.binds.clear(); S.item = -1; }      // the lanes lay their outputs out again
	return CRTHIP_OK;
}
extern "C" int crthip_pool_set_packed_host_blobs(crthip_pool *p, int on) {
	if(!p) return ctx_fail(CRTHIP_E_ARGUMENT, nullptr);
	for(auto &L : p->lanes) { const int err = crthip_ctx_set_packed_host_blobs(L.ctx, on); if(err) return err; }
	p->packed = on != 0;
	return CRTHIP_OK;
}

// Host-resident items (SURVEY.md 8d's primary region: .crt blobs in pinned host memory -> decoded outputs in HBM): crthip_batch_reset uploads
// a step's blobs itself, with ONE DMA copy at the head of the context's own stream.  Round 4 built and measured four ways of taking that
// copy off the step (C4 batch, 4 x 4 contexts; resident inputs 0.080 ms a step, this path 0.093, PCIe alone 0.075: tools/h2d_probe.py):
// a copy stream per worker thread with an event the context waits for (0.125, and 7 ms stalls), the lane's NEXT batch queued behind the
// running batch's kernels on the lane's own stream (0.15-0.20: a DMA copy queued behind kernels is started late), the same two with a
// copy KERNEL reading the pinned buffer over PCIe (0.13 / 0.156).  All slower; removed.  What does help a little is one more lane per
// thread's worth of contexts (5 x 4: 0.091): the lane whose blobs are on their way is idle for the GPU.
// An item's outputs, from the blobs' headers alone: where every array lies in the item's block - corto_hip::layout_blob, the rule of
// crthip_output_layout - and what a call reports for it.  Made once per item in front of a call; lane_plan binds from it.
struct ItemPlan {
	int err = CRTHIP_OK;                         // the first failing blob's code: the item cannot be planned
	std::string err_msg;
	uint64_t total = 0;                          // crthip_output_layout's total
	uint64_t tris = 0, verts = 0;
	std::vector<crthip_out_array> attr, index;   // sum(nattr) / nblobs entries
	std::vector<uint32_t> first_attr;            // first attr entry of blob i
	uint32_t runs = 0;                           // stretches of blobs adjacent in host memory in arena layout (batch.cpp: a copy each when packed host blobs are on)
	// crthip_pool_decode
	size_t status_at = 0;                        // the item's first entry in the call's status array
	bool pinned = false;                         // a host destination that is pinned memory
};
static int item_plan(const crthip_pool *p, const crthip_pool_item &it, ItemPlan &P) {
	const uint32_t flags = p->render ? CRTHIP_LAYOUT_RENDER : 0u;
	uint64_t off = 0;
	crthip_blob_info info;
	P.index.resize(it.nblobs); P.first_attr.resize(it.nblobs);
	for(uint32_t i = 0; i < it.nblobs; i++) {
		const int err = crthip_probe(it.blobs[i], it.lens[i], &info);
		if(err) { P.err = err; P.err_msg = std::string(crthip_strerror(err)) + " (blob " + std::to_string(i) + ")"; return ctx_fail(err, P.err_msg.c_str()); }
		if(corto_hip::packed_run_starts(it.blobs, it.lens, i)) P.runs++;
		P.first_attr[i] = (uint32_t)P.attr.size();
		P.attr.resize(P.attr.size() + info.nattr);
		corto_hip::layout_blob(info, flags, off, P.attr.data() + P.first_attr[i], &P.index[i]);
		P.tris += info.nface; P.verts += info.nvert;
	}
	P.total = corto_hip::layout_total(off);
	return CRTHIP_OK;
}

// One call's work.  crthip_pool_run (dests null): warmup + steps + a tail of tickets, items drawn cyclically, every lane's block poisoned
// in front of its last steps.  crthip_pool_decode (dests set): every item once, into its destination.  The workers, their pinning, the
// lane they refill next and the pipelining of a lane are the same code for both.
struct PoolJob {
	uint32_t nitems = 0;
	const crthip_pool_item *items = nullptr;
	std::vector<ItemPlan> plans;
	// crthip_pool_run
	uint64_t steps = 0, warmup = 0;
	double *completion_s = nullptr;
	// crthip_pool_decode
	const crthip_pool_dest *dests = nullptr;
	int32_t *status = nullptr;
	crthip_pool_done_fn done = nullptr; void *user = nullptr;
};

// plan the group S.mem (the members' item, step and destination filled in; one member is an item alone) on one of the lane's batch objects
// and bind its outputs: member k into the lane's device block, k strides in (the block holds `group` strides and the call's slack
// afterwards), or straight into its device destination.  *item_fault: the failure is an item's own - a blob the host walk refuses - and
// the lane is as it was, but for an empty-handed batch object
static int lane_plan(crthip_pool *p, Lane &L, Slot &S, const PoolJob &job, bool *item_fault) {
	const bool dec = job.dests != nullptr;
	const size_t n = S.mem.size();
	const crthip_pool_item &it0 = job.items[S.mem[0].item];
	const ItemPlan &P0 = job.plans[(size_t)S.mem[0].item];
	int err = CRTHIP_OK;
	*item_fault = false;
	if(!S.batch && (&S == &L.s[1] || n > 1)) {                   // the lane's second object lives on the context's other set of per-call blocks
		err = crthip_batch_create(L.ctx, 0, nullptr, nullptr, nullptr, &S.batch);
		if(!err && &S == &L.s[1]) err = crthip_batch_set_parity(S.batch, 1);
		if(err) return err;
	}
	S.item = -1;
	uint32_t nblobs = it0.nblobs;
	if(n == 1) {
		const void *arena = it0.device_arena ? it0.device_arena[L.slot] : nullptr;
		err = S.batch ? crthip_batch_reset(S.batch, it0.nblobs, it0.blobs, it0.lens, arena)
		              : crthip_batch_create(L.ctx, it0.nblobs, it0.blobs, it0.lens, arena, &S.batch);
	} else {
		// the members' blob lists, joined.  Host blobs: packed ones go up as a run a member (crthip_ctx_set_packed_host_blobs).  Resident blobs (every
		// member has an arena on this device, or none has: the draw sees to it): the lowest arena is the batch's, the others' blobs lie 64-bit offsets above it
		S.gblobs.clear(); S.glens.clear(); S.goff.clear();
		const uint8_t *lowest = nullptr;
		for(const Member &m : S.mem) {
			const crthip_pool_item &it = job.items[m.item];
			const uint8_t *a = it.device_arena ? (const uint8_t *)it.device_arena[L.slot] : nullptr;
			if(a && (!lowest || a < lowest)) lowest = a;
		}
		for(const Member &m : S.mem) {
			const crthip_pool_item &it = job.items[m.item];
			uint64_t off = lowest ? (uint64_t)((const uint8_t *)it.device_arena[L.slot] - lowest) : 0;
			for(uint32_t i = 0; i < it.nblobs; i++) {
				S.gblobs.push_back(it.blobs[i]); S.glens.push_back(it.lens[i]);
				if(lowest) { S.goff.push_back(off); off += ((uint64_t)it.lens[i] + 15) & ~15ull; }
			}
		}
		nblobs = (uint32_t)S.gblobs.size();
		err = lowest ? corto_hip::batch_reset_at(S.batch, nblobs, S.gblobs.data(), S.glens.data(), lowest, S.goff.data())
		             : crthip_batch_reset(S.batch, nblobs, S.gblobs.data(), S.glens.data(), nullptr);
	}
	if(err) { *item_fault = err != CRTHIP_E_DEVICE && err != CRTHIP_E_NOMEM; return err; }
	const size_t stride = (p->out_need + 255) & ~(size_t)255;
	const size_t block_need = (size_t)(p->group - 1)*stride + (dec ? p->out_need : std::max((size_t)P0.total + 256, p->out_need));
	if(block_need > L.out_cap) {
		// (never under a batch that is planned or running: out_need covers every item of the call, so a lane's block is made by its first plan)
		if(L.busy || L.staged) return ctx_fail(CRTHIP_E_ARGUMENT, "corto_hip pool: a lane's output block would move under a planned batch");
		if(L.out) (void)hipFree(L.out);
		L.out = nullptr; L.out_cap = 0;
		if(hipMalloc(&L.out, block_need + block_need/8) != hipSuccess) return ctx_fail(CRTHIP_E_NOMEM, nullptr);
		L.out_cap = block_need + block_need/8;
	}
	S.first_attr.clear(); S.binds.clear(); S.index_ptr.clear(); S.index_fmt.clear();
	bool mirror = false;
	uint32_t first = 0;
	for(size_t k = 0; k < n; k++) {
		Member &m = S.mem[k];
		const crthip_pool_item &it = job.items[m.item];
		const ItemPlan &P = job.plans[(size_t)m.item];
		m.first = first; m.nblobs = it.nblobs; first += it.nblobs;
		m.lane_off = k*stride;
		if(!m.base) m.base = (uint8_t *)L.out + m.lane_off;
		m.out_used = (size_t)P.total;
		mirror = mirror || (m.to_host && !m.pinned_dst);
		const uint32_t attr0 = (uint32_t)S.binds.size();
		for(uint32_t f : P.first_attr) S.first_attr.push_back(attr0 + f);
		for(size_t a = 0; a < P.attr.size(); a++) {
			crthip_attr_binding b;
			b.buffer = m.base + P.attr[a].offset; b.format = P.attr[a].format; b.stride = 0; b.reserved = 0;
			b.out_components = P.attr[a].format == CRTHIP_FMT_UINT8 ? P.attr[a].out_components : 0;   // (colour: 4 of them, whatever the stream holds)
			S.binds.push_back(b);
		}
		for(uint32_t i = 0; i < it.nblobs; i++) { S.index_ptr.push_back(P.index[i].bytes ? m.base + P.index[i].offset : nullptr); S.index_fmt.push_back(P.index[i].format); }
	}
	S.status.assign(nblobs, 0);
	if(mirror && L.host_cap < L.out_cap) {                        // (first use: 32 MB of pinned memory a lane for a C4 item)
		if(L.host_out) (void)hipHostFree(L.host_out);
		L.host_out = nullptr; L.host_cap = 0;
		if(hipHostMalloc(&L.host_out, L.out_cap, hipHostMallocDefault) != hipSuccess) return ctx_fail(CRTHIP_E_NOMEM, nullptr);
		L.host_cap = L.out_cap;
	}
	S.item = S.mem[0].item; S.step = S.mem[n - 1].step;
	return crthip_batch_bind_all(S.batch, S.binds.data(), S.index_ptr.data(), S.index_fmt.data());
}

// One call's shared state: the work lists and their cursors, the completion stamps, the counters of the report.  Nothing here belongs to a thread.
struct Run {
	crthip_pool *const p; PoolJob &job;
	const bool dec;                                              // crthip_pool_decode
	uint64_t timed_end, total, poison_from;                      // total: the tickets of the call (the constructor sets them; constant afterwards)
	// home shard first: pool device d owns the items j with j % ndevices == d (its shard is resident there), and a device without a home
	// item takes from the others' ("stealing" in a cyclic run: it is the work list that is shared, a faster GPU simply draws more tickets).
	// crthip_pool_decode: the home lists hold the host-destination items, `bound` a slot's device-destination items, which nobody else may
	// draw; every list is drawn once, front to back, and a slot whose own lists are empty takes from the other slots' home lists
	std::vector<std::vector<uint32_t>> home, bound;
	std::vector<std::atomic<uint64_t>> home_next, bound_next;
	std::atomic<uint64_t> stolen{0};
	std::vector<double> stamps;                                  // stamps[c] = time at which the c-th completion happened (1-based)
	std::atomic<uint64_t> failed{0}, fallbacks{0}, tris{0}, verts{0}, grouped{0};
	std::vector<std::atomic<uint64_t>> per_dev;
	std::atomic<int32_t> first_error{0};
	std::atomic<uint64_t> host_ns{0}, host_steps{0}, wait_ns{0}, finish_ns{0}, plan_ns{0}, plan_max_ns{0}, launch_max_ns{0};
	Run(crthip_pool *pool, PoolJob &j) : p(pool), job(j), dec(j.dests != nullptr), home(pool->ndevices), bound(pool->ndevices),
		home_next(pool->ndevices), bound_next(pool->ndevices), per_dev(pool->ndevices) {
		timed_end = dec ? 0 : j.warmup + j.steps;
		// the tail keeps every context busy until the last timed completion (a pipelined lane has two tickets drawn and not completed)
		total = dec ? j.nitems : timed_end + p->lanes.size()*(p->pipelined ? 2u : 1u);
		// the last round of timed steps and the tail behind them (outputs_to_host: the tail only - poisoning the pinned mirror is 32 MB of memset on the worker thread)
		poison_from = dec ? ~0ull : p->to_host ? timed_end : timed_end > p->lanes.size() ? timed_end - p->lanes.size() : 0;
		stamps.assign(timed_end + 1, 0.0);
		for(uint32_t i = 0; i < j.nitems; i++) {
			if(dec && j.dests[i].device_slot >= 0) bound[(uint32_t)j.dests[i].device_slot].push_back(i);
			else home[i % p->ndevices].push_back(i);
		}
		for(auto *v : {&home_next, &bound_next, &per_dev}) for(auto &x : *v) x = 0;
	}
	static void raise_max(std::atomic<uint64_t> &m, uint64_t v) { uint64_t cur = m.load(); while(v > cur && !m.compare_exchange_weak(cur, v)) { } }
	static bool take(const std::vector<uint32_t> &q, std::atomic<uint64_t> &at, uint32_t &j) {
		if(at.load() >= q.size()) return false;
		const uint64_t k = at.fetch_add(1);
		if(k >= q.size()) return false;
		j = q[k];
		return true;
	}
	bool draw_once(uint32_t slot, uint32_t &j) {
		if(take(bound[slot], bound_next[slot], j) || take(home[slot], home_next[slot], j)) return true;
		for(uint32_t d = 1; d < p->ndevices; d++) { const uint32_t o = (slot + d) % p->ndevices; if(take(home[o], home_next[o], j)) return true; }
		return false;
	}
	// crthip_pool_decode: item j is final - `code` in every status entry (it could not be planned, or holds no blob), or S's statuses
	// (the statuses of its blobs, which begin at `first` in the group's batch object)
	void settle(uint32_t slot, uint32_t j, int32_t code, const Slot *S, uint32_t first) {
		const ItemPlan &P = job.plans[j];
		int32_t *st = job.status + P.status_at;
		for(uint32_t i = 0; i < job.items[j].nblobs; i++) st[i] = S ? S->status[first + i] : code;
		if(!S) {
			++p->completed;
			if(code) { failed += job.items[j].nblobs; int32_t z = 0; first_error.compare_exchange_strong(z, code); }
		}
		per_dev[slot]++;
		if(job.done) job.done(job.user, j, slot, st);
	}
	// one ticket from the work lists for a thread of `slot`.  0: none left; 1: `k` is drawn; 2 (crthip_pool_decode): an item with nothing to
	// launch was drawn and settled
	int draw(uint32_t slot, Ticket &k) {
		k.solo = false;
		if(!dec) {
			k.step = p->next.fetch_add(1);
			if(k.step >= total) return 0;
			if(!home[slot].empty()) k.j = home[slot][home_next[slot].fetch_add(1) % home[slot].size()];
			else k.j = (uint32_t)(stolen.fetch_add(1) % job.nitems);
			return 1;
		}
		if(p->next.load() >= total || !draw_once(slot, k.j)) return 0;
		k.step = p->next.fetch_add(1);
		if(job.plans[k.j].err || job.items[k.j].nblobs == 0) { settle(slot, k.j, job.plans[k.j].err, nullptr, 0); return 2; }
		return 1;
	}
	// a drawn ticket as a group member: where its outputs go
	Member member_of(const Ticket &k) const {
		Member m;
		m.item = (int64_t)k.j; m.step = k.step; m.to_host = p->to_host;
		if(!dec) return m;
		const crthip_pool_dest &D = job.dests[k.j];
		m.to_host = D.device_slot < 0;
		if(!m.to_host) m.base = (uint8_t *)D.out;
		else if(job.plans[k.j].pinned) m.pinned_dst = D.out;
		else m.pageable_dst = D.out;
		return m;
	}
	void fill_report(crthip_pool_report &rep, double call_s) const {
		rep.elapsed_s = dec ? call_s : stamps[timed_end] - stamps[job.warmup];
		rep.steps = dec ? job.nitems : job.steps; rep.triangles = tris; rep.vertices = verts;
		rep.failed_blobs = failed; rep.first_error = first_error; rep.topology_fallbacks = fallbacks; rep.grouped_steps = grouped;
		for(uint32_t d = 0; d < p->ndevices; d++) { rep.steps_per_device[d] = per_dev[d]; if(per_dev[d]) rep.devices_used++; }
		if(!dec) for(auto &L : p->lanes) if(L.s[L.cur].item >= 0 && L.poisoned) rep.poisoned_lanes++;
		rep.host_us_per_step = host_steps ? (float)((double)host_ns/1e3/(double)host_steps) : 0.f;
		if(host_steps) {
			rep.host_wait_us = (float)((double)wait_ns/1e3/(double)host_steps); rep.host_finish_us = (float)((double)finish_ns/1e3/(double)host_steps);
			rep.host_plan_us = (float)((double)plan_ns/1e3/(double)host_steps);
			rep.host_plan_max_us = (float)((double)plan_max_ns/1e3); rep.host_launch_max_us = (float)((double)launch_max_ns/1e3);
		}
		for(uint32_t d = 0; d < p->ndevices; d++) if(!p->cpus[d].empty()) rep.pinned_devices++;
		if(job.completion_s) for(uint64_t c = 0; c < job.steps; c++) job.completion_s[c] = stamps[job.warmup + 1 + c] - stamps[job.warmup];
	}
};

using Clock = std::chrono::steady_clock;
static uint64_t ns_since(Clock::time_point t0) { return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(Clock::now() - t0).count(); }

// One host thread of a run: `depth` lanes of one pool device, refilled in turn.  A pipelined lane plans a ticket on its free batch object and
// enqueues [mesh stage of the batch planned one refill ago + entropy stage of this one]; its first ticket of a run only enqueues an entropy
// stage, and it draws the next one at once.  (crthip_pool_decode: the two objects are then bound to two different items' blocks.  That is
// safe: an entropy stage writes its batch's own scratch and nothing else - corto_hip.h, crthip_batch_decode_with_next - so only the mesh
// stage in flight writes a block.)
struct Worker {
	Run &r; crthip_pool *const p; const uint32_t slot; Lane *const mine;   // `mine`: the thread's `depth` lanes
	// `held` is consumed before the work lists and `tickets` goes false only when it is empty and the lists are dry: no drawn ticket is lost.
	// Solo tickets (a refused group's members) and tickets that did not fit a group wait here alike; a solo one is never joined to a group
	std::vector<Ticket> held;                                    // drawn and not planned yet: a ticket that did not fit the group it was drawn for, the members of a group that was refused
	bool tickets = true; int err = CRTHIP_OK;
	Worker(Run &run, uint32_t slot_, uint32_t t) : r(run), p(run.p), slot(slot_), mine(&run.p->lanes[((size_t)slot_*run.p->threads_per_device + t)*run.p->depth]) { }
	// the next lane to refill: a free one, else whichever of the busy ones finishes first (they mostly finish in the order they
	// were launched, but a thread that waited on the oldest while a younger one was done left that context idle)
	Lane *pick_lane(uint64_t n) {
		for(uint32_t k = 0; k < p->depth; k++) if(!mine[(n + k) % p->depth].busy) return &mine[(n + k) % p->depth];
		for(uint32_t spins = 0; ; spins++) {
			for(uint32_t k = 0; k < p->depth; k++) {
				Lane &C = mine[(n + k) % p->depth];
				const int d = crthip_batch_done(C.s[C.cur].batch);
				if(d < 0) { err = d; return nullptr; }
				if(d) return &C;
			}
			if(spins < 64) std::this_thread::yield(); else std::this_thread::sleep_for(std::chrono::microseconds(5));
		}
	}
	// harvest the lane's batch in flight: every member of the group is a step of its own
	int finish(Lane &L) {
		Slot &S = L.s[L.cur];
		const int rc = crthip_batch_sync(S.batch, S.status.data());
		L.busy = false;
		// a completion and a stamp each (the same instant), counted by its own step number
		const double t_done = now_s();
		if(S.mem.size() > 1) r.grouped += S.mem.size();
		for(const Member &m : S.mem) {
			const uint64_t c = ++p->completed;                   // completion order
			if(c <= r.timed_end) r.stamps[c] = t_done;
			if(!r.dec && m.step >= r.job.warmup && m.step < r.timed_end) { r.per_dev[slot]++; r.tris += r.job.plans[(size_t)m.item].tris; r.verts += r.job.plans[(size_t)m.item].verts; }
		}
		uint64_t bad = 0;
		for(int32_t st_ : S.status) if(st_) { bad++; int32_t z = 0; r.first_error.compare_exchange_strong(z, st_); }
		r.failed += bad;
		crthip_batch_stats st;
		if(crthip_batch_get_stats(S.batch, &st) == CRTHIP_OK) r.fallbacks += st.topology_fallbacks;
		if(rc == CRTHIP_E_DEVICE || rc == CRTHIP_E_NOMEM) return rc;
		if(r.dec) for(const Member &m : S.mem) {
			if(m.pageable_dst) memcpy(m.pageable_dst, (const uint8_t *)L.host_out + m.lane_off, m.out_used);   // (the copy into the lane's mirror is what the sync waited for)
			r.tris += r.job.plans[(size_t)m.item].tris; r.verts += r.job.plans[(size_t)m.item].verts;
			r.settle(slot, (uint32_t)m.item, 0, &S, m.first);
		}
		return CRTHIP_OK;
	}
	// what the batch just synced says about the lane's next calls (Lane: pipe, single_ok, alone)
	void note_carry(Lane &L) {
		if(!p->pipelined || L.staged || L.s[L.cur].item < 0) return;
		L.pipe = corto_hip::batch_carriable(L.s[L.cur].batch);
		if(L.s[L.cur].mem.size() == 1) L.single_ok = L.pipe;
		else if(!L.pipe && L.single_ok) L.alone = true;          // (one item a call pipelines again)
	}
	// The mesh stage of s[cur] and, behind it, the D2H copies of a step of outputs_to_host or of items with host destinations.  DECODE: s[cur]'s
	// whole decode; ALONE: its mesh stage (its whole decode, had its entropy stage not been carried) and nothing else; WITH_NEXT: its mesh
	// stage + the entropy stage of s[cur ^ 1], and `drain` says whether that was carried.
	// A step that is due one starts from a poisoned block: the outputs every lane holds after the run were written by a mesh stage that STARTED
	// from one, so the post-run bit-exact check cannot pass on bytes an earlier step left behind (on the context's own stream: ordered before
	// the stage's kernels)
	enum class Mesh { DECODE, ALONE, WITH_NEXT };
	int enqueue_mesh(Lane &L, Mesh how) {
		Slot &S = L.s[L.cur];
		crthip_batch *const next = L.s[L.cur ^ 1u].batch;
		int e = CRTHIP_OK;
		L.poisoned = false;
		if(S.step >= r.poison_from && L.out) {
			e = corto_hip::ctx_fill_async(L.ctx, L.out, L.out_cap, POISON);
			if(!e && p->to_host && L.host_out) for(const Member &m : S.mem) memset((uint8_t *)L.host_out + m.lane_off, POISON, m.out_used);
			L.poisoned = !e;
		}
		if(!e) e = how == Mesh::DECODE ? crthip_batch_decode(S.batch) : crthip_batch_decode_with_next(S.batch, how == Mesh::WITH_NEXT ? next : nullptr);
		if(!e && how == Mesh::WITH_NEXT) L.drain = !corto_hip::batch_entropy_done(next);
		for(const Member &m : S.mem) {                           // (one copy a member: each has its own destination)
			if(e || !m.to_host) continue;
			e = corto_hip::ctx_copy_to_host_async(L.ctx, m.pinned_dst ? m.pinned_dst : (uint8_t *)L.host_out + m.lane_off, (const uint8_t *)L.out + m.lane_off, m.out_used);
		}
		if(!e) L.busy = true;
		return e;
	}
	// the lane's planned batch becomes its current one and runs its mesh stage alone
	int launch_staged(Lane &L) { L.cur ^= 1u; L.staged = false; return enqueue_mesh(L, Mesh::ALONE); }
	bool resident(uint32_t j) const { return r.job.items[j].device_arena && r.job.items[j].device_arena[slot]; }
	// Blobs that must be gathered (scattered host blobs, or packed host blobs off) are not grouped: the gathering is a memcpy on this thread
	// while its other lanes wait, and two items' worth of it in one piece cost `scattered_pageable_blobs` 29 % (profiles/pool_group.md)
	uint32_t runs_of(uint32_t j) const { return resident(j) ? 0u : p->packed ? r.job.plans[j].runs : corto_hip::PACKED_RUNS_MAX + 1; }
	// The tickets of the lane's next call, 0: none left.  A first ticket, then up to group - 1 more while the lists are long - at least
	// 2 x lanes x group tickets undrawn, so that the end of a run and a short crthip_pool_decode still spread over all lanes, one item a call.
	// Members are all resident on this device or all uploaded; crthip_pool_decode's lists hold this slot's own device-destination items and
	// host items only, so no group mixes slots
	uint32_t gather(const Lane &L, Ticket *tk) {
		if(!held.empty()) { tk[0] = held.front(); held.erase(held.begin()); }
		else for(int d = 2; d == 2; ) { d = r.draw(slot, tk[0]); if(d == 0) return 0; }
		uint32_t ntk = 1;
		const bool first_batch = p->pipelined && !L.staged && L.s[L.cur].item < 0;   // (of this lane in this run: one item, to learn whether such a batch can be carried)
		uint32_t runs = runs_of(tk[0].j);
		const uint32_t want = tk[0].solo || L.alone || first_batch || runs > corto_hip::PACKED_RUNS_MAX ? 1u : p->group;
		while(ntk < want) {
			Ticket x;
			if(!held.empty()) { if(held.front().solo) break; x = held.front(); held.erase(held.begin()); }
			else {
				const uint64_t nx = p->next.load();
				if(nx >= r.total || r.total - nx < 2ull*p->lanes.size()*p->group) break;
				const int d = r.draw(slot, x);
				if(d == 0) break;
				if(d == 2) continue;
			}
			if(resident(x.j) != resident(tk[0].j) || runs + runs_of(x.j) > corto_hip::PACKED_RUNS_MAX) { held.push_back(x); break; }
			runs += runs_of(x.j);
			tk[ntk++] = x;
		}
		return ntk;
	}
	// one call on a lane that is not busy: gather its tickets, plan them on the free batch object, enqueue.  false: no ticket is left
	bool refill(Lane &L) {
		Ticket tk[GROUP_MAX];
		const uint32_t ntk = gather(L, tk);
		if(!ntk) { tickets = false; return false; }
		const auto h0 = Clock::now();
		const bool lp = p->pipelined && (L.pipe || L.staged);       // this refill pipelines
		const uint32_t t = lp ? (L.staged ? L.cur : L.cur ^ 1u) : L.cur;   // the free batch object
		Slot &T = L.s[t];
		T.mem.clear();
		for(uint32_t k = 0; k < ntk; k++) T.mem.push_back(r.member_of(tk[k]));
		bool item_fault = false;
		err = lane_plan(p, L, T, r.job, &item_fault);
		{ const uint64_t ns_ = ns_since(h0); r.plan_ns += ns_; Run::raise_max(r.plan_max_ns, ns_); }
		if(err && item_fault && ntk > 1) {                           // one member's own failure: each of them alone, so that the bad item alone gets the code
			for(uint32_t k = 0; k < ntk; k++) { tk[k].solo = true; held.push_back(tk[k]); }
			err = CRTHIP_OK; return true;
		}
		if(err && r.dec && item_fault) { r.settle(slot, tk[0].j, err, nullptr, 0); err = CRTHIP_OK; return true; }   // the item's own failure: the lane draws the next one
		if(err) return true;
		const auto d0 = Clock::now();
		if(lp && !L.staged) { err = crthip_batch_decode_with_next(nullptr, T.batch); L.staged = !err; }   // the lane's first ticket of a run: its entropy stage alone
		else {
			L.cur = lp ? L.cur ^ 1u : t;                             // whose mesh stage runs now: the batch planned one refill ago, else this one
			err = enqueue_mesh(L, lp ? Mesh::WITH_NEXT : Mesh::DECODE);
		}
		Run::raise_max(r.launch_max_ns, ns_since(d0));
		r.host_ns += ns_since(h0); r.host_steps += ntk;             // (per ticket)
		return true;
	}
	void flush() { for(uint32_t k = 0; k < p->depth; k++) if(mine[k].busy) { const int e2 = finish(mine[k]); if(!err) err = e2; } }
	// A context whose thread drew none of the last 2 x lanes tickets (descheduled while the others emptied the queue: seen with
	// 32-blob items) repeats its last step from a poisoned block, behind the timed region: what lane_read returns is then ALWAYS
	// a poisoned step's output, not only almost always
	void repeat_unpoisoned() {
		for(uint32_t k = 0; k < p->depth && !err; k++) {
			Lane &L = mine[k];
			Slot &S = L.s[L.cur];
			if(S.item < 0) {                                         // ... and one that drew no ticket at all (a 28-step run on a cold box) decodes its device's first item
				bool item_fault = false;
				Ticket k0; k0.j = r.home[slot].empty() ? 0u : r.home[slot][0]; k0.step = r.total;
				S.mem.assign(1, r.member_of(k0));
				err = lane_plan(p, L, S, r.job, &item_fault);
				if(err) break;
			}
			if(L.poisoned || !L.out) continue;
			S.step = r.total;                                        // (a repeat is nobody's timed step, and past poison_from)
			for(Member &m : S.mem) m.step = r.total;
			err = enqueue_mesh(L, Mesh::DECODE);
			if(!err) err = finish(L);
		}
	}
	void run() {
		(void)hipSetDevice(p->devices[slot]);
		if(!p->cpus[slot].empty()) {                                 // next to the GPU: plan + launch are ~200 us of host work per step and thread
			cpu_set_t set; CPU_ZERO(&set);
			for(int c : p->cpus[slot]) CPU_SET(c, &set);
			(void)pthread_setaffinity_np(pthread_self(), sizeof set, &set);   // (a cpuset that forbids them: stay where we are)
		}
		for(uint64_t n = 0; !err && tickets; n++) {
			const auto w0 = Clock::now();
			Lane *const picked = pick_lane(n);
			if(!picked) break;
			Lane &L = *picked;
			r.wait_ns += ns_since(w0);
			const auto f0 = Clock::now();
			if(L.busy) err = finish(L);
			r.finish_ns += ns_since(f0);
			if(!err) note_carry(L);
			if(!err && L.staged && L.drain) {                        // the planned batch was not carried: its whole decode alone, no ticket drawn
				L.drain = false; L.pipe = false;
				err = launch_staged(L);
			}
			while(!err && !L.busy && refill(L)) { }
		}
		flush();
		for(uint32_t k = 0; k < p->depth && !err; k++) if(mine[k].staged) err = launch_staged(mine[k]);   // no ticket left: the mesh stage of every lane's planned batch, alone
		flush();
		if(!r.dec) repeat_unpoisoned();
		if(err) {
			std::lock_guard<std::mutex> lock(p->m);
			if(!p->error) { p->error = err; p->error_msg = crthip_last_error(); }
			p->next = r.total;                                       // stop handing out work
		}
	}
};

static int pool_work(crthip_pool *p, PoolJob &job, crthip_pool_report *report) {
	p->next = 0; p->completed = 0; p->error = CRTHIP_OK; p->error_msg.clear();
	for(auto &L : p->lanes) L.begin_run();
	Run r(p, job);
	const double t_launch = r.stamps[0] = now_s();
	std::vector<std::thread> threads;
	for(uint32_t d = 0; d < p->ndevices; d++)
		for(uint32_t t = 0; t < p->threads_per_device; t++) threads.emplace_back([&r, d, t] { Worker(r, d, t).run(); });
	for(auto &th : threads) th.join();
	const double t_joined = now_s();
	if(r.dec) for(auto &L : p->lanes) for(Slot &S : L.s) { S.item = -1; S.binds.clear(); }   // (the destinations are the caller's again)
	if(p->error) return ctx_fail(p->error, p->error_msg.c_str());
	if(report) r.fill_report(*report, t_joined - t_launch);
	return CRTHIP_OK;
}

extern "C" int crthip_pool_run(crthip_pool *p, uint32_t nitems, const crthip_pool_item *items, uint64_t steps, uint64_t warmup,
                               crthip_pool_report *report, double *completion_s) {
	if(!p || !items || nitems == 0 || !report) return ctx_fail(CRTHIP_E_ARGUMENT, nullptr);
	memset(report, 0, sizeof(*report));
	PoolJob job;
	job.nitems = nitems; job.items = items; job.steps = steps; job.warmup = warmup; job.completion_s = completion_s;
	// triangles / vertices and the output layout of every item (header parse only)
	job.plans.resize(nitems);
	p->out_need = 0;
	for(uint32_t j = 0; j < nitems; j++) {
		const int err = item_plan(p, items[j], job.plans[j]);
		if(err) return err;
		// (crthip_pool_run's own 256 bytes behind the block: what "#tail" reads)
		if(p->pipelined || p->group > 1) p->out_need = std::max(p->out_need, (size_t)job.plans[j].total + 256);
	}
	p->decoded = false;
	return pool_work(p, job, report);
}

extern "C" int crthip_pool_decode(crthip_pool *p, uint32_t nitems, const crthip_pool_item *items, const crthip_pool_dest *dests,
                                  int32_t *status, crthip_pool_done_fn done, void *user, crthip_pool_report *report) {
	if(!p || (nitems && (!items || !dests))) return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_pool_decode: null argument");
	if(report) memset(report, 0, sizeof(*report));
	PoolJob job;
	job.nitems = nitems; job.items = items; job.dests = dests; job.done = done; job.user = user;
	job.plans.resize(nitems);
	size_t nstatus = 0;
	p->out_need = 0;
	auto bad = [](uint32_t j, const char *what) {
		const std::string msg = "crthip_pool_decode: item " + std::to_string(j) + ": " + what;
		return ctx_fail(CRTHIP_E_ARGUMENT, msg.c_str());
	};
	// every destination before the first launch: a refused call has written nothing
	for(uint32_t j = 0; j < nitems; j++) {
		ItemPlan &P = job.plans[j];
		const crthip_pool_dest &D = dests[j];
		if(items[j].nblobs && (!items[j].blobs || !items[j].lens)) return bad(j, "null blob list");
		P.status_at = nstatus; nstatus += items[j].nblobs;
		if(D.reserved) return bad(j, "reserved must be 0");
		if(D.device_slot != CRTHIP_POOL_DEST_HOST && (D.device_slot < 0 || (uint32_t)D.device_slot >= p->ndevices)) return bad(j, "device_slot names no pool device");
		if((uintptr_t)D.out & 255) return bad(j, "out is not 256-byte aligned");
		if(item_plan(p, items[j], P)) continue;                  // the item's own failure: reported in its statuses, its destination is not written
		if(P.total && !D.out) return bad(j, "null out");
		if(D.cap < P.total) return bad(j, "cap is smaller than the layout's total");
		if(!P.total) continue;
		if(D.device_slot >= 0) {
			// device memory of the slot's GPU, [out, out + total) inside one allocation (the resident encoder's check, encode_batch.cpp)
			if(!corto_hip::resident_array_ok(D.out, P.total, 1, p->devices[(uint32_t)D.device_slot]))
				return bad(j, "out is not device memory of the slot's GPU, or [out, out + total) leaves its allocation");
		} else {
			hipPointerAttribute_t a;
			memset(&a, 0, sizeof(a));
			if(hipPointerGetAttributes(&a, D.out) != hipSuccess) { (void)hipGetLastError(); a.type = hipMemoryTypeUnregistered; }   // (plain host memory)
			if(a.type == hipMemoryTypeDevice) return bad(j, "a host destination that is device memory");
			P.pinned = a.type == hipMemoryTypeHost;
			p->out_need = std::max(p->out_need, (size_t)P.total);   // the lanes' blocks: sized once for the largest host item
		}
	}
	std::vector<int32_t> own_status;
	if(!status) { own_status.assign(std::max<size_t>(nstatus, 1), 0); status = own_status.data(); }
	job.status = status;
	p->decoded = true;
	if(nitems == 0) return CRTHIP_OK;
	return pool_work(p, job, report);
}

extern "C" int64_t crthip_pool_lane_item(const crthip_pool *p, uint32_t lane, uint32_t *device_slot) {
	if(!p || lane >= p->lanes.size()) return ctx_fail(CRTHIP_E_ARGUMENT, nullptr);
	if(device_slot) *device_slot = p->lanes[lane].slot;
	if(p->decoded) return -1;                                    // (crthip_pool_decode delivered every item: a lane holds nothing)
	return p->lanes[lane].s[p->lanes[lane].cur].item;           // (a pipelined lane: the batch whose mesh stage ran last)
}

extern "C" int64_t crthip_pool_lane_read(crthip_pool *p, uint32_t lane, uint32_t blob, const char *what, void *host_out, size_t cap) {
	if(!p || lane >= p->lanes.size() || !what || !host_out || p->decoded) return ctx_fail(CRTHIP_E_ARGUMENT, nullptr);
	Lane &L = p->lanes[lane];
	Slot &S = L.s[L.cur];                                        // (a pipelined lane: the batch whose mesh stage ran last)
	if(!S.batch || S.item < 0 || blob >= crthip_batch_size(S.batch)) return ctx_fail(CRTHIP_E_ARGUMENT, nullptr);
	crthip_blob_info info;
	int err = crthip_batch_info(S.batch, blob, &info);
	if(err) return err;
	// what the arrays hold is the layout's business (output_layout.h): the blob's entries under the pool's flags give the byte counts
	crthip_out_array arrays[CRTHIP_MAX_ATTRS], index; uint64_t end = 0;
	corto_hip::layout_blob(info, p->render ? CRTHIP_LAYOUT_RENDER : 0u, end, arrays, &index);
	const uint8_t *src = nullptr; size_t n = 0;
	if(!strcmp(what, "#tail")) { n = L.out_cap < 256 ? L.out_cap : 256; src = (const uint8_t *)L.out + (L.out_cap - n); }   // the block's last bytes: behind every output array
	else if(!strcmp(what, "index")) { if(!info.nface) return 0; src = (const uint8_t *)S.index_ptr[blob]; n = (size_t)index.bytes; }
	else {
		for(uint32_t k = 0; k < info.nattr; k++) if(!strcmp(info.attr[k].name, what)) { src = (const uint8_t *)S.binds[S.first_attr[blob] + k].buffer; n = (size_t)arrays[k].bytes; }
		if(!src) return ctx_fail(CRTHIP_E_ARGUMENT, "no such attribute");
	}
	if(n > cap) n = cap;
	// outputs_to_host: what the step's own D2H copy left in the lane's pinned block (the tail lies behind the copied range: from the device)
	if(p->to_host && L.host_out && strcmp(what, "#tail")) { memcpy(host_out, (const uint8_t *)L.host_out + (src - (const uint8_t *)L.out), n); return (int64_t)n; }
	if(hipSetDevice(L.device) != hipSuccess || hipMemcpy(host_out, src, n, hipMemcpyDeviceToHost) != hipSuccess) return ctx_fail(CRTHIP_E_DEVICE, nullptr);
	return (int64_t)n;
}
