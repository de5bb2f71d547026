// encode_batch.cpp — crthip_encode_batch: a batch of meshes and point clouds in, one .crt per item out, every blob byte-identical
// to crthip_encode of that item.
//
// The serial part - the CLERS topology pass, which reads the index alone - runs on a pool of host threads while the device
// quantises (encoder.cpp: batch_topology), or, where the context asks for it (crthip_ctx_set_encode_topology), on the device behind the
// quantiser (k_encode_topo.hip, enc_topology.h): the compacted faces, the quads and the CLERS symbols are then written where the next
// kernels read them, and one record per mesh comes back for its frame (encoder.cpp: batch_frame).  Everything per vertex runs on the device and stays resident until the coded streams
// come back (k_encode_batch.hip): quantisation, estimated normals, residuals, the point clouds' Morton sort (one cloud after
// another: each has its own launches), then the value and
// Tunstall coders (encode_gpu.cpp: encode_value_streams_device).  The host splices every container from its frame and the coded
// streams.  One device image per chunk of the batch; no allocation per mesh or per stream.
#include <hip/hip_runtime.h>
#include <sched.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/corto_hip.h"
#include "device_plan.h"
#include "enc_topology.h"
#include "encoder_internal.h"
#include "kernels.h"

using namespace corto_hip;

namespace {

#define BT_TRY(expr) do { hipError_t e_ = (expr); if(e_ != hipSuccess) return ctx_fail(CRTHIP_E_DEVICE, (std::string(#expr ": ") + hipGetErrorString(e_)).c_str()); } while(0)

using Clock = std::chrono::steady_clock;
double ms_since(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }

struct DevMem { void *p = nullptr; ~DevMem() { if(p) (void)hipFree(p); } uint8_t *u8() const { return (uint8_t *)p; } };

uint32_t default_threads() {
	cpu_set_t set;
	CPU_ZERO(&set);
	uint32_t n = 0;
	if(sched_getaffinity(0, sizeof(set), &set) == 0) n = (uint32_t)CPU_COUNT(&set);
	if(n == 0) n = 1;
	return std::min<uint32_t>(16, n);
}

// run f(i) for i in [0, n) on up to `threads` threads (fewer if the system gives fewer: the calling thread takes what is left).
// f must not throw.
template <class F> void parallel_for(uint32_t n, uint32_t threads, F f) {
	std::atomic<uint32_t> next{0};
	auto work = [&]() { for(uint32_t i; (i = next.fetch_add(1)) < n;) f(i); };
	std::vector<std::thread> pool;
	try {
		pool.reserve(threads);
		for(uint32_t t = 1; t < std::min(threads, n); t++) pool.emplace_back(work);
	} catch(...) {}
	work();
	for(std::thread &t : pool) t.join();
}

// what a worker's exception becomes: the item's status (nothing leaves a worker thread)
template <class F> int32_t item_guard(F f) {
	try { f(); return CRTHIP_OK; }
	catch(const std::bad_alloc &) { return CRTHIP_E_NOMEM; }
	catch(...) { return CRTHIP_E_ARGUMENT; }
}

uint64_t al(uint64_t x) { return (x + 255) & ~255ull; }
uint32_t rs_blocks(uint32_t n) { return std::max(1u, (n + RS_TILE - 1)/RS_TILE); }
bool is_mesh(const BatchItem &it) { return it.nface_in > 0; }
// normals whose residuals are against the estimate (a cloud's estimate is all zeros: its ESTIMATED normals still subtract toOcta of it)
bool est_of(const BatchItem &it, const BatchAttr &a) { return a.codec == CRTHIP_CODEC_NORMAL && (a.prediction == 1 || (a.prediction == 2 && is_mesh(it))); }
constexpr uint64_t DIRECT_BYTES = 1u << 20;               // inputs from this size up go to the device straight from the caller's array
                                                          // (any element size and byte count: slots are 256-byte aligned, a copy is bytes)

// where one item lives in the chunk's device image
struct Slot {
	std::vector<uint64_t> in, q, d;       // per attribute: raw input, quantised values, residuals
	uint64_t faces = 0, quads = 0, boundary = 0, count = 0;
	uint64_t zkeys[2] = {0, 0}, zvals[2] = {0, 0}, zhist = 0, zmn = 0;
	uint64_t clers = 0;
	uint64_t idx = 0, gend_in = 0, gend_out = 0, first = 0, cursor = 0, sides = 0, twin = 0, state = 0, split = 0;   // the device topology pass
	uint32_t fbase = 0;                   // first face in the faces region (faces units)
};

// the device bytes of one item (for chunking), the same sums the layout below makes
uint64_t item_bytes(const BatchItem &it) {
	uint64_t b = 0;
	for(const BatchAttr &a : it.attrs) b += al(quant_in_bytes(a.quant)) + 2*al(quant_out_bytes(a.quant)) + 256;
	if(is_mesh(it)) {
		b += al((uint64_t)it.nface_in*12) + al((uint64_t)it.nvert_in*16) + al((uint64_t)it.nvert_in*4) + al(it.nface_in*8ull + 64);
		for(const BatchAttr &a : it.attrs) if(est_of(it, a)) b += 2*(al((uint64_t)it.nface_in*12) + al((uint64_t)it.nface_in*12)) + al(256ull*4*rs_blocks(3*it.nface_in));
	} else b += 2*al((uint64_t)it.nvert_in*8) + 2*al((uint64_t)it.nvert_in*4) + al((uint64_t)it.nvert_in*16) + al(256ull*4*rs_blocks(it.nvert_in)) + 512;
	// the device topology pass: raw index and group ends, bucket tables, sides, twins, the walk's global image, split words (private and
	// packed), record; in every mode but HOST the CLERS symbols have their place in the image
	if(it.topo_device) {
		const uint64_t nf = it.nface_in, nv = it.nvert_in;
		b += al(nf*12) + 2*al(it.topo_groups*4ull) + al((nv + 1)*4) + al(nv*4) + al(nf*3*sizeof(EncTopoSide)) + al(nf*12) + 2*al(enc_topo_split_cap(it.nface_in)*4) + 1024;
		if(!it.topo_lds) b += al(enc_topo_state_bytes<uint32_t>(it.nface_in, it.nvert_in));
	}
	if(it.topo_image) b += al(enc_topo_clers_cap(it.nface_in));
	return b + 4096;
}

struct Timer {
	hipEvent_t a = nullptr, b = nullptr; bool used = false;
	~Timer() { if(a) (void)hipEventDestroy(a); if(b) (void)hipEventDestroy(b); }
	int begin(hipStream_t st) { if(!a) { BT_TRY(hipEventCreate(&a)); BT_TRY(hipEventCreate(&b)); } used = true; BT_TRY(hipEventRecord(a, st)); return 0; }
	int end(hipStream_t st) { BT_TRY(hipEventRecord(b, st)); return 0; }
	float ms() { float m = 0; if(used && hipEventElapsedTime(&m, a, b) != hipSuccess) m = 0; return m; }
};
struct BatchTimes { float quant = 0, est = 0, delta = 0, zkeys = 0, zsort = 0, topo_c = 0, topo_p = 0, topo_w = 0;
                    uint32_t n_quant = 0, n_est = 0, n_delta = 0, n_zkeys = 0, n_zsort = 0, n_topo_c = 0, n_topo_p = 0, n_topo_w = 0; };
struct Event {
	hipEvent_t e = nullptr;
	~Event() { if(e) (void)hipEventDestroy(e); }
	int record(hipStream_t st) { if(!e) BT_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming)); BT_TRY(hipEventRecord(e, st)); return 0; }
};

// LSD radix sort of n records in (k0, v0) by key bits [0, bits), ping-ponging through (k1, v1); returns which buffer holds the result
template <typename K>
int radix_sort(hipStream_t st, K *k0, uint32_t *v0, K *k1, uint32_t *v1, uint32_t *hist, uint32_t n, uint32_t bits, int &where, uint32_t &launches) {
	where = 0;
	if(n < 2) return 0;
	const uint32_t nb = rs_blocks(n);
	for(uint32_t shift = 0; shift < bits; shift += 8) {
		K *ki = where ? k1 : k0, *ko = where ? k0 : k1;
		uint32_t *vi = where ? v1 : v0, *vo = where ? v0 : v1;
		hipLaunchKernelGGL(k_enc_rs_hist<K>, dim3(nb), dim3(RS_THREADS), 0, st, (const K *)ki, n, shift, hist);
		hipLaunchKernelGGL(k_enc_rs_scan, dim3(1), dim3(1024), 0, st, hist, 256u*nb);
		hipLaunchKernelGGL(k_enc_rs_scatter<K>, dim3(nb), dim3(RS_THREADS), 0, st, (const K *)ki, (const uint32_t *)vi, ko, vo, n, shift, (const uint32_t *)hist);
		where ^= 1;
		launches += 3;
	}
	BT_TRY(hipGetLastError());
	return 0;
}

// the device half of one chunk: items[ids] have been set up; their topology passes run here on the pool, overlapping the device
int run_chunk(crthip_ctx *ctx, const crthip_mesh *meshes, const crthip_attr_list *extra, std::vector<BatchItem> &items, const std::vector<uint32_t> &ids, uint32_t threads,
              std::vector<std::vector<uint8_t>> &blobs, crthip_encode_batch_stats &S, BatchTimes &bt, EncStageTimes &tm) {
	hipStream_t st = ctx_stream(ctx);
	const uint32_t n = (uint32_t)ids.size();
	const int mode = ctx_encode_topology(ctx);
	// whose topology pass runs where: devk on the device (CRTHIP_TOPOLOGY_DEVICE: every mesh, _SPLIT: those that walk in LDS), hostk
	// (the other meshes, and every cloud's frame) on the host
	std::vector<uint32_t> hostk, devk;
	for(uint32_t k = 0; k < n; k++) (items[ids[k]].topo_device ? devk : hostk).push_back(k);
	// topology passes (meshes) and frames (everything) on the pool, started first: they need the index alone
	std::vector<uint8_t> ready(n, 0);
	for(uint32_t k : devk) ready[k] = 1;
	std::mutex mu; std::condition_variable cv;
	double topo_ms = 0;
	const auto t_topo = Clock::now();
	auto host_pass = [&](uint32_t k) {
		const int32_t e = item_guard([&] { batch_topology(&meshes[ids[k]], extra ? &extra[ids[k]] : nullptr, items[ids[k]]); });
		if(e) items[ids[k]].status = e;                      // read by this thread's caller only after the join
		{ std::lock_guard<std::mutex> g(mu); ready[k] = 1; }
		cv.notify_all();
	};
	std::thread pool;
	if(mode != CRTHIP_TOPOLOGY_DEVICE) pool = std::thread([&]() {      // (device mode starts no thread: the clouds' frames are made inline below)
		parallel_for((uint32_t)hostk.size(), threads, [&](uint32_t j) { host_pass(hostk[j]); });
		std::lock_guard<std::mutex> g(mu);
		topo_ms = ms_since(t_topo);
	});
	struct Joiner { std::thread &t; ~Joiner() { if(t.joinable()) t.join(); } } joiner{pool};

	// ---- layout: raw inputs first (one upload), then everything else ----
	std::vector<Slot> slot(n);
	uint64_t o = 0;
	struct RawIn { const void *src; uint64_t bytes; uint64_t *off; };
	std::vector<RawIn> raw;                                  // every raw attribute; for a mesh of the device pass also its index and group ends
	std::vector<uint32_t> whole(n, 0);                       // the one group of a mesh given without groups
	for(uint32_t k = 0; k < n; k++) {
		const BatchItem &it = items[ids[k]];
		slot[k].in.resize(it.attrs.size()); slot[k].q.resize(it.attrs.size()); slot[k].d.resize(it.attrs.size());
		for(size_t a = 0; a < it.attrs.size(); a++) raw.push_back(RawIn{it.attrs[a].quant.in, quant_in_bytes(it.attrs[a].quant), &slot[k].in[a]});
		if(it.topo_device) {
			const crthip_mesh &m = meshes[ids[k]];
			whole[k] = it.nface_in;
			raw.push_back(RawIn{m.index, (uint64_t)it.nface_in*12, &slot[k].idx});
			raw.push_back(RawIn{m.ngroups ? (const void *)m.group_end : (const void *)&whole[k], (uint64_t)it.topo_groups*4, &slot[k].gend_in});
		}
	}
	for(int big = 0; big < 2; big++)                          // the small inputs first: they go up staged, in one copy
		for(const RawIn &r : raw) if((r.bytes >= DIRECT_BYTES) == (big == 1)) { *r.off = o; o += al(r.bytes); }
	uint64_t staged_total = 0;
	for(const RawIn &r : raw) if(r.bytes < DIRECT_BYTES) staged_total = std::max(staged_total, *r.off + r.bytes);
	const uint64_t o_zero = o;                               // zeroed: BORDER XORs, counts, cloud minima and flags
	for(uint32_t k = 0; k < n; k++) {
		const BatchItem &it = items[ids[k]];
		slot[k].count = o; o += 256;
		if(is_mesh(it)) { for(const BatchAttr &a : it.attrs) if(est_of(it, a) && a.prediction == 2) { slot[k].boundary = o; o += al((uint64_t)it.nvert_in*4); } }
		else { slot[k].zmn = o; o += 256; }
	}
	const uint64_t o_zflags = o; o += al((uint64_t)n*4);    // every cloud's equal-key flag, read back in one copy
	// the device topology pass reports here, read back in one copy: the split words' count, a record per mesh, the new group ends
	const uint64_t o_back = o;
	if(!devk.empty()) {
		o += 256 + al(devk.size()*sizeof(EncTopoRecord));
		for(uint32_t k : devk) { slot[k].gend_out = o; o += (uint64_t)items[ids[k]].topo_groups*4; }
		o = al(o);
	}
	const uint64_t back_bytes = o - o_back;
	const uint64_t zero_bytes = o - o_zero;
	uint32_t faces_total = 0, corners_total = 0;
	for(uint32_t k = 0; k < n; k++) {
		const BatchItem &it = items[ids[k]];
		for(size_t a = 0; a < it.attrs.size(); a++) { slot[k].q[a] = o; o += al(quant_out_bytes(it.attrs[a].quant)); slot[k].d[a] = o; o += al(quant_out_bytes(it.attrs[a].quant)); }
		if(is_mesh(it)) {
			slot[k].fbase = faces_total; faces_total += it.nface_in;
			for(const BatchAttr &a : it.attrs) if(est_of(it, a)) corners_total += 3*it.nface_in;
		} else {
			for(int b = 0; b < 2; b++) { slot[k].zkeys[b] = o; o += al((uint64_t)it.nvert_in*8); slot[k].zvals[b] = o; o += al((uint64_t)it.nvert_in*4); }
			slot[k].quads = o; o += al((uint64_t)it.nvert_in*16);
			slot[k].zhist = o; o += al(256ull*4*rs_blocks(it.nvert_in));
		}
	}
	const uint64_t o_mquads = o;                             // the meshes' quads back to back, and their faces: one upload each
	for(uint32_t k = 0; k < n; k++) if(is_mesh(items[ids[k]])) { slot[k].quads = o; o += (uint64_t)items[ids[k]].nvert_in*16; }
	const uint64_t mquads_bytes = o - o_mquads;
	o = al(o);
	const uint64_t o_faces = o; o += al((uint64_t)faces_total*12);
	uint64_t o_ck[2], o_cv[2];
	for(int b = 0; b < 2; b++) { o_ck[b] = o; o += al((uint64_t)corners_total*4); o_cv[b] = o; o += al((uint64_t)corners_total*4); }
	const uint64_t o_chist = o; o += al(256ull*4*rs_blocks(corners_total));
	// the device topology pass's scratch, and (every mode but HOST) each mesh's CLERS symbols where the value coder reads them
	uint64_t split_cap_total = 0;
	for(uint32_t k : devk) {
		const BatchItem &it = items[ids[k]];
		const uint64_t nf = it.nface_in, nv = it.nvert_in;
		slot[k].first = o; o += al((nv + 1)*4);
		slot[k].cursor = o; o += al(nv*4);
		slot[k].sides = o; o += al(nf*3*sizeof(EncTopoSide));
		slot[k].twin = o; o += al(nf*12);
		if(!it.topo_lds) { slot[k].state = o; o += al(enc_topo_state_bytes<uint32_t>(it.nface_in, it.nvert_in)); }
		slot[k].split = o; o += al(enc_topo_split_cap(it.nface_in)*4);
		split_cap_total += enc_topo_split_cap(it.nface_in);
	}
	const uint64_t o_spack = o; o += al(split_cap_total*4);
	for(uint32_t k = 0; k < n; k++) if(items[ids[k]].topo_image) { slot[k].clers = o; o += al(enc_topo_clers_cap(items[ids[k]].nface_in)); }
	const uint64_t o_jobs = o; o += 1u << 16;                // job tables, rewritten stage by stage (stream-ordered)
	std::vector<uint8_t> jobbuf;
	uint64_t job_bytes = 0;
	for(uint32_t k = 0; k < n; k++) job_bytes += items[ids[k]].attrs.size()*(sizeof(QuantJob) + sizeof(DeltaEncJob) + sizeof(EstJob) + 8) + 16;
	job_bytes += devk.size()*(sizeof(EncTopoJob) + 8);
	o += al(3*job_bytes);
	DevMem dev;
	{ const auto t0 = Clock::now(); BT_TRY(hipMalloc(&dev.p, o + 256)); S.alloc_ms += ms_since(t0); }
	uint8_t *base = dev.u8();
	struct Drain { hipStream_t st; ~Drain() { (void)hipStreamSynchronize(st); } } drain{st};   // every way out waits for the work queued on the image first
	auto sync = [&]() -> hipError_t { const auto t0 = Clock::now(); const hipError_t e = hipStreamSynchronize(st); S.sync_wait_ms += ms_since(t0); return e; };
	uint64_t job_cursor = o_jobs;
	std::vector<std::vector<uint8_t>> keep;                  // the job tables' host copies live until the chunk has finished
	bool jobs_fit = true;
	auto put_jobs = [&](const void *p, size_t bytes) -> uint8_t * {
		uint8_t *d = base + job_cursor;
		if(job_cursor + bytes > o) { jobs_fit = false; return nullptr; }
		if(bytes) {
			keep.emplace_back((const uint8_t *)p, (const uint8_t *)p + bytes);
			if(hipMemcpyAsync(d, keep.back().data(), bytes, hipMemcpyHostToDevice, st) != hipSuccess) jobs_fit = false;
			S.bytes_to_device += bytes;
		}
		job_cursor += al(bytes);
		return d;
	};

	// ---- raw inputs up: small ones staged into one copy, large ones straight from the caller ----
	{
		const auto t_stage = Clock::now();
		std::vector<uint8_t> stage(staged_total);
		for(const RawIn &r : raw) {
			const uint64_t b = r.bytes;
			if(!b) continue;
			if(b < DIRECT_BYTES) memcpy(stage.data() + *r.off, r.src, b);
			else { const auto t0 = Clock::now(); BT_TRY(hipMemcpyAsync(base + *r.off, r.src, b, hipMemcpyHostToDevice, st)); S.upload_ms += ms_since(t0); }
			if(b >= DIRECT_BYTES) S.bytes_to_device += b;
		}
		S.host_stage_ms += ms_since(t_stage);
		{ const auto t0 = Clock::now(); if(staged_total) BT_TRY(hipMemcpyAsync(base, stage.data(), staged_total, hipMemcpyHostToDevice, st)); S.upload_ms += ms_since(t0); }
		S.bytes_to_device += staged_total;
		BT_TRY(sync());
	}
	if(zero_bytes) BT_TRY(hipMemsetAsync(base + o_zero, 0, zero_bytes, st));

	// ---- K-ENC-Q ----
	Timer tq;
	{
		std::vector<QuantJob> qj; std::vector<uint32_t> start;
		uint32_t blocks = 0;
		for(uint32_t k = 0; k < n; k++) {
			const BatchItem &it = items[ids[k]];
			for(size_t a = 0; a < it.attrs.size(); a++) {
				const QuantRequest &r = it.attrs[a].quant;
				if(!r.count) continue;
				QuantJob J{};
				J.in = base + slot[k].in[a]; J.out = base + slot[k].q[a]; J.count = r.count; J.kind = r.kind; J.N = r.N; J.q = r.q; J.unit = r.unit; J.format = r.format;
				for(int c = 0; c < 4; c++) J.qc[c] = r.qc[c] ? r.qc[c] : 1u;
				qj.push_back(J); start.push_back(blocks); blocks += (r.count + 255)/256;
			}
		}
		if(!qj.empty()) {
			start.push_back(blocks);
			const QuantJob *dj = (const QuantJob *)put_jobs(qj.data(), qj.size()*sizeof(QuantJob));
			const uint32_t *ds = (const uint32_t *)put_jobs(start.data(), start.size()*4);
			if(!jobs_fit) return ctx_fail(CRTHIP_E_DEVICE, "crthip_encode_batch: job tables");
			if(tq.begin(st)) return CRTHIP_E_DEVICE;
			hipLaunchKernelGGL(k_enc_quantize_batch, dim3(blocks), dim3(256), 0, st, dj, ds, (uint32_t)qj.size());
			if(tq.end(st)) return CRTHIP_E_DEVICE;
			BT_TRY(hipGetLastError());
			bt.n_quant++;
		}
	}

	// ---- K-ENC-TOPO: the topology pass of the meshes in devk, behind the quantiser; their records start back at once ----
	Timer ttc, ttp, ttw;
	Event ev_back;
	std::vector<uint8_t> back(back_bytes);
	const auto t_dtopo = Clock::now();
	if(!devk.empty()) {
		std::vector<EncTopoJob> tj(devk.size());
		std::vector<uint32_t> walk_ids;                          // the LDS-resident walks first, then the global ones
		uint32_t nlds = 0, lds_bytes = 0;
		for(int pass = 0; pass < 2; pass++) for(uint32_t j = 0; j < devk.size(); j++) if(items[ids[devk[j]]].topo_lds == (pass == 0)) walk_ids.push_back(j);
		for(uint32_t j = 0; j < devk.size(); j++) {
			const uint32_t k = devk[j];
			const BatchItem &it = items[ids[k]];
			EncTopoJob &J = tj[j];
			memset(&J, 0, sizeof(J));
			J.index = (const uint32_t *)(base + slot[k].idx); J.gend_in = (const uint32_t *)(base + slot[k].gend_in);
			J.faces = (uint32_t *)(base + o_faces) + (size_t)slot[k].fbase*3; J.gend_out = (uint32_t *)(base + slot[k].gend_out);
			J.first = (uint32_t *)(base + slot[k].first); J.cursor = (uint32_t *)(base + slot[k].cursor);
			J.sides = (EncTopoSide *)(base + slot[k].sides); J.twin = (uint32_t *)(base + slot[k].twin);
			J.state = it.topo_lds ? nullptr : base + slot[k].state;
			J.quads = (uint32_t *)(base + slot[k].quads); J.clers = base + slot[k].clers; J.split = (uint32_t *)(base + slot[k].split);
			J.split_packed = (uint32_t *)(base + o_spack); J.split_cursor = (uint32_t *)(base + o_back);
			J.rec = (EncTopoRecord *)(base + o_back + 256) + j;
			J.nvert = it.nvert_in; J.nface = it.nface_in; J.ngroups = it.topo_groups;
			if(it.topo_lds) { nlds++; lds_bytes = std::max(lds_bytes, (uint32_t)enc_topo_state_bytes<uint16_t>(it.nface_in, it.nvert_in)); }
		}
		const EncTopoJob *dj = (const EncTopoJob *)put_jobs(tj.data(), tj.size()*sizeof(EncTopoJob));
		const uint32_t *dw = (const uint32_t *)put_jobs(walk_ids.data(), walk_ids.size()*4);
		if(!jobs_fit) return ctx_fail(CRTHIP_E_DEVICE, "crthip_encode_batch: job tables");
		const uint32_t nd = (uint32_t)devk.size();
		if(ttc.begin(st)) return CRTHIP_E_DEVICE;
		hipLaunchKernelGGL(k_enc_topo_compact, dim3(nd), dim3(ETOPO_THREADS), 0, st, dj, nd);
		if(ttc.end(st) || ttp.begin(st)) return CRTHIP_E_DEVICE;
		hipLaunchKernelGGL(k_enc_topo_pair, dim3(nd), dim3(ETOPO_THREADS), 0, st, dj, nd);
		if(ttp.end(st) || ttw.begin(st)) return CRTHIP_E_DEVICE;
		if(nlds) hipLaunchKernelGGL(k_enc_topo_walk<true>, dim3(nlds), dim3(ETOPO_THREADS), lds_bytes, st, dj, dw, nlds);
		if(nd > nlds) hipLaunchKernelGGL(k_enc_topo_walk<false>, dim3(nd - nlds), dim3(ETOPO_THREADS), 0, st, dj, dw + nlds, nd - nlds);
		if(ttw.end(st)) return CRTHIP_E_DEVICE;
		BT_TRY(hipGetLastError());
		bt.n_topo_c++; bt.n_topo_p++; bt.n_topo_w += (nlds ? 1u : 0u) + (nd > nlds ? 1u : 0u);
		BT_TRY(hipMemcpyAsync(back.data(), base + o_back, back_bytes, hipMemcpyDeviceToHost, st));
		if(ev_back.record(st)) return CRTHIP_E_DEVICE;
		S.bytes_from_device += back_bytes;
		S.topology_device += nd; S.topology_lds += nlds;
	}

	// ---- point clouds: Morton keys and the radix sort ----
	std::vector<uint32_t> clouds;
	for(uint32_t k = 0; k < n; k++) if(!is_mesh(items[ids[k]])) clouds.push_back(k);
	std::vector<Timer> tzk(clouds.size()), tzs(clouds.size());
	for(size_t c = 0; c < clouds.size(); c++) {
		const uint32_t k = clouds[c];
		const BatchItem &it = items[ids[k]];
		if(it.nvert_in == 0) continue;
		ZJob Z{};
		Z.coords = (const int32_t *)(base + slot[k].q[0]);
		for(size_t a = 0; a < it.attrs.size(); a++) if(it.attrs[a].position) Z.coords = (const int32_t *)(base + slot[k].q[a]);
		Z.mn = (int32_t *)(base + slot[k].zmn); Z.flag = (uint32_t *)(base + o_zflags) + k; Z.n = it.nvert_in;
		Z.keys = (uint64_t *)(base + slot[k].zkeys[0]); Z.vals = (uint32_t *)(base + slot[k].zvals[0]);
		const uint32_t g = (it.nvert_in + 255)/256;
		if(tzk[c].begin(st)) return CRTHIP_E_DEVICE;
		hipLaunchKernelGGL(k_enc_zmin, dim3(g), dim3(256), 0, st, Z);
		hipLaunchKernelGGL(k_enc_zkeys, dim3(g), dim3(256), 0, st, Z);
		if(tzk[c].end(st)) return CRTHIP_E_DEVICE;
		bt.n_zkeys += 2;
		int where = 0; uint32_t launches = 0;
		if(tzs[c].begin(st)) return CRTHIP_E_DEVICE;
		{ const int e = radix_sort(st, Z.keys, Z.vals, (uint64_t *)(base + slot[k].zkeys[1]), (uint32_t *)(base + slot[k].zvals[1]),
		                           (uint32_t *)(base + slot[k].zhist), it.nvert_in, 64, where, launches); if(e) return e; }
		Z.keys = (uint64_t *)(base + slot[k].zkeys[where]); Z.vals = (uint32_t *)(base + slot[k].zvals[where]);
		Z.quads = (uint32_t *)(base + slot[k].quads);
		hipLaunchKernelGGL(k_enc_zflag, dim3(g), dim3(256), 0, st, Z);
		if(tzs[c].end(st)) return CRTHIP_E_DEVICE;
		BT_TRY(hipGetLastError());
		bt.n_zsort += launches + 1;
	}

	// ---- the device pass's records: each mesh's frame from its counts, group ends and split words (those came packed: a second copy)
	if(mode == CRTHIP_TOPOLOGY_DEVICE) { for(uint32_t k : hostk) host_pass(k); topo_ms = ms_since(t_topo); }   // (the clouds' frames)
	if(!devk.empty()) {
		{ const auto t0 = Clock::now(); BT_TRY(hipEventSynchronize(ev_back.e)); S.sync_wait_ms += ms_since(t0); }
		S.device_topology_ms += (float)ms_since(t_dtopo);
		uint32_t nwords = 0;
		memcpy(&nwords, back.data(), 4);
		std::vector<uint32_t> words(nwords);
		if(nwords > split_cap_total) return ctx_fail(CRTHIP_E_DEVICE, "crthip_encode_batch: the device topology pass's split words");
		if(nwords) {
			BT_TRY(hipMemcpyAsync(words.data(), base + o_spack, (size_t)nwords*4, hipMemcpyDeviceToHost, st));
			BT_TRY(sync());
			S.bytes_from_device += (uint64_t)nwords*4;
		}
		const auto t0 = Clock::now();
		for(uint32_t j = 0; j < devk.size(); j++) {
			const uint32_t k = devk[j];
			BatchItem &it = items[ids[k]];
			EncTopoRecord R;
			memcpy(&R, back.data() + 256 + (size_t)j*sizeof(EncTopoRecord), sizeof(R));
			if(R.status || R.nvert > it.nvert_in || R.nface > it.nface_in || (uint64_t)R.split_off + R.split_words > nwords || R.nclers > enc_topo_clers_cap(it.nface_in)) {
				it.status = ctx_fail(CRTHIP_E_DEVICE, "crthip_encode_batch: the device topology pass stopped at a bound");
				continue;
			}
			const int32_t e = item_guard([&] {
				batch_frame(&meshes[ids[k]], extra ? &extra[ids[k]] : nullptr, it, R, (const uint32_t *)(back.data() + (slot[k].gend_out - o_back)), words.data() + R.split_off);
			});
			if(e) it.status = e;
		}
		S.host_frame_ms += (float)ms_since(t0);
	}
	// ---- the host's topology passes as they finish: each mesh's faces and quads are staged as soon as its pass is done, and go up in
	// two copies (one copy per mesh measured slower: 24.5 against 20.4 ms for 256 C4 units, tools/encode_batch_rate.py)
	std::vector<uint8_t> up_quads(mquads_bytes), up_faces((size_t)faces_total*12);
	for(uint32_t k = 0; k < n; k++) {
		{ const auto tw = Clock::now(); std::unique_lock<std::mutex> g(mu); cv.wait(g, [&] { return ready[k] != 0; }); S.topology_wait_ms += ms_since(tw); }
		BatchItem &it = items[ids[k]];
		if(!is_mesh(it) || it.topo_device) continue;
		const auto t0 = Clock::now();
		const size_t fb = std::min(it.faces.size()*4, (size_t)it.nface_in*12), qb = std::min(it.quads.size()*4, (size_t)it.nvert_in*16);
		if(fb) memcpy(up_faces.data() + (size_t)slot[k].fbase*12, it.faces.data(), fb);
		if(qb) memcpy(up_quads.data() + (slot[k].quads - o_mquads), it.quads.data(), qb);
		S.host_stage_ms += ms_since(t0);
	}
	{
		// one copy each per run of neighbouring meshes the host made (all of them, without a device pass)
		const auto t0 = Clock::now();
		std::vector<uint32_t> mk;
		for(uint32_t k = 0; k < n; k++) if(is_mesh(items[ids[k]])) mk.push_back(k);
		for(size_t a = 0; a < mk.size();) {
			if(items[ids[mk[a]]].topo_device) { a++; continue; }
			size_t b = a;
			while(b + 1 < mk.size() && !items[ids[mk[b + 1]]].topo_device) b++;
			const BatchItem &last = items[ids[mk[b]]];
			const uint64_t q0 = slot[mk[a]].quads, q1 = slot[mk[b]].quads + (uint64_t)last.nvert_in*16;
			const uint64_t f0 = (uint64_t)slot[mk[a]].fbase*12, f1 = ((uint64_t)slot[mk[b]].fbase + last.nface_in)*12;
			if(q1 > q0) BT_TRY(hipMemcpyAsync(base + q0, up_quads.data() + (q0 - o_mquads), q1 - q0, hipMemcpyHostToDevice, st));
			if(f1 > f0) BT_TRY(hipMemcpyAsync(base + o_faces + f0, up_faces.data() + f0, f1 - f0, hipMemcpyHostToDevice, st));
			S.bytes_to_device += (q1 - q0) + (f1 - f0);
			a = b + 1;
		}
		S.upload_ms += ms_since(t0);
	}
	BT_TRY(sync());
	if(pool.joinable()) pool.join();
	S.host_topology_ms += (float)topo_ms;
	for(uint32_t k = 0; k < n; k++) {                                     // Tunstall streams over 2^23 symbols: the reference's count*255 overflow
		BatchItem &it = items[ids[k]];
		if(it.entropy == CRTHIP_ENTROPY_TUNSTALL && (it.nclers > (1u << 23) || it.nvert > (1u << 23)))
			it.status = ctx_fail(CRTHIP_E_LIMIT, "crthip_encode_batch: a Tunstall stream longer than 2^23 symbols");
	}

	// ---- K-ENC-EST ----
	Timer te;
	{
		std::vector<EstJob> ej; std::vector<uint32_t> fstart, vstart;
		uint32_t fb = 0, vb = 0, vbase = 0, cbase = 0;
		for(uint32_t k = 0; k < n; k++) {
			const BatchItem &it = items[ids[k]];
			if(it.status) continue;
			int pos = 0;
			for(size_t a = 0; a < it.attrs.size(); a++) if(it.attrs[a].position) pos = (int)a;
			for(size_t a = 0; a < it.attrs.size(); a++) {
				if(!est_of(it, it.attrs[a])) continue;
				EstJob J{};
				J.faces = (const uint32_t *)(base + o_faces) + (size_t)slot[k].fbase*3;
				J.coords = (const int32_t *)(base + slot[k].q[pos]);
				J.normals = (int32_t *)(base + slot[k].q[a]);
				J.boundary = it.attrs[a].prediction == 2 ? (int32_t *)(base + slot[k].boundary) : nullptr;
				J.nface = it.nface; J.nvert = it.nvert_in;
				J.vbase = vbase; J.fbase = slot[k].fbase; J.cbase = cbase; J.unit = it.attrs[a].quant.unit;
				ej.push_back(J); fstart.push_back(fb); vstart.push_back(vb);
				fb += (J.nface + 255)/256; vb += (J.nvert + 255)/256;
				vbase += J.nvert; cbase += 3*J.nface;
			}
		}
		if(!ej.empty()) {
			fstart.push_back(fb); vstart.push_back(vb);
			const EstJob *dj = (const EstJob *)put_jobs(ej.data(), ej.size()*sizeof(EstJob));
			const uint32_t *dfs = (const uint32_t *)put_jobs(fstart.data(), fstart.size()*4);
			const uint32_t *dvs = (const uint32_t *)put_jobs(vstart.data(), vstart.size()*4);
			if(!jobs_fit) return ctx_fail(CRTHIP_E_DEVICE, "crthip_encode_batch: job tables");
			uint32_t *ck0 = (uint32_t *)(base + o_ck[0]), *ck1 = (uint32_t *)(base + o_ck[1]);
			uint32_t *cv0 = (uint32_t *)(base + o_cv[0]), *cv1 = (uint32_t *)(base + o_cv[1]);
			if(te.begin(st)) return CRTHIP_E_DEVICE;
			if(fb) hipLaunchKernelGGL(k_enc_corners, dim3(fb), dim3(256), 0, st, dj, dfs, (uint32_t)ej.size(), ck0, cv0);
			uint32_t bits = 8, launches = 0;
			while(bits < 32 && (vbase >> bits)) bits += 8;
			int where = 0;
			{ const int e = radix_sort(st, ck0, cv0, ck1, cv1, (uint32_t *)(base + o_chist), cbase, bits, where, launches); if(e) return e; }
			if(vb) hipLaunchKernelGGL(k_enc_est_normal, dim3(vb), dim3(256), 0, st, dj, dvs, (uint32_t)ej.size(), (const uint32_t *)(where ? ck1 : ck0),
			                          (const uint32_t *)(where ? cv1 : cv0), cbase, (const uint32_t *)(base + o_faces));
			if(te.end(st)) return CRTHIP_E_DEVICE;
			BT_TRY(hipGetLastError());
			bt.n_est += launches + 2;
		}
	}

	// ---- clouds whose sorted keys have equal neighbours: the host's std::sort decides their order ----
	std::vector<uint32_t> zflags(n, 0);
	if(!clouds.empty()) {
		BT_TRY(hipMemcpyAsync(zflags.data(), base + o_zflags, (size_t)n*4, hipMemcpyDeviceToHost, st));
		BT_TRY(sync());
		S.bytes_from_device += (uint64_t)n*4;
	}
	for(uint32_t k : clouds) {
		BatchItem &it = items[ids[k]];
		if(it.nvert_in == 0 || it.status) continue;
		if(!zflags[k]) { S.clouds_device_sorted++; continue; }
		int pos = 0;
		for(size_t a = 0; a < it.attrs.size(); a++) if(it.attrs[a].position) pos = (int)a;
		std::vector<int32_t> coords((size_t)it.nvert_in*3);
		BT_TRY(hipMemcpyAsync(coords.data(), base + slot[k].q[pos], coords.size()*4, hipMemcpyDeviceToHost, st));
		BT_TRY(sync());
		S.bytes_from_device += coords.size()*4;
		std::vector<uint32_t> order;
		morton_order_host(coords.data(), it.nvert_in, order);
		std::vector<uint32_t> quads((size_t)it.nvert_in*4);
		for(uint32_t i = 0; i < it.nvert_in; i++) {
			const uint32_t prev = i ? order[i - 1] : 0xffffffffu;
			quads[(size_t)i*4] = order[i]; quads[(size_t)i*4 + 1] = prev; quads[(size_t)i*4 + 2] = prev; quads[(size_t)i*4 + 3] = prev;
		}
		BT_TRY(hipMemcpyAsync(base + slot[k].quads, quads.data(), quads.size()*4, hipMemcpyHostToDevice, st));
		BT_TRY(sync());
		S.bytes_to_device += quads.size()*4;
		S.clouds_host_sorted++;
	}

	// ---- K-ENC-DELTA ----
	Timer td;
	{
		std::vector<DeltaEncJob> dj; std::vector<uint32_t> start;
		uint32_t blocks = 0;
		for(uint32_t k = 0; k < n; k++) {
			const BatchItem &it = items[ids[k]];
			if(it.status) continue;
			for(size_t a = 0; a < it.attrs.size(); a++) {
				const BatchAttr &A = it.attrs[a];
				DeltaEncJob J{};
				J.values = base + slot[k].q[a]; J.quads = (const uint32_t *)(base + slot[k].quads); J.out = base + slot[k].d[a];
				J.count = it.nvert; J.N = A.N; J.parallel = (A.strategy & CRTHIP_PARALLEL) ? 1u : 0u;
				J.out_count = (uint32_t *)(base + slot[k].count) + a;
				if(A.codec == CRTHIP_CODEC_COLOR) J.kind = DENC_U8;
				else if(A.codec == CRTHIP_CODEC_NORMAL) {
					J.N = 2;
					J.kind = A.prediction == 0 ? DENC_NRM_DIFF : A.prediction == 1 ? DENC_NRM_EST : DENC_NRM_BORDER;
					if(J.kind == DENC_NRM_BORDER) J.boundary = (const int32_t *)(base + slot[k].boundary);
					if(J.kind == DENC_NRM_BORDER && !is_mesh(it)) { J.kind = DENC_NRM_EST; J.count = 0; }   // a cloud has no faces: no vertex is on a border
				} else J.kind = DENC_I32;
				if(J.kind != DENC_NRM_BORDER && J.count == 0) continue;
				dj.push_back(J); start.push_back(blocks);
				blocks += J.kind == DENC_NRM_BORDER ? 1u : (J.count + DENC_BLOCK - 1)/DENC_BLOCK;
			}
		}
		if(!dj.empty()) {
			start.push_back(blocks);
			const DeltaEncJob *d = (const DeltaEncJob *)put_jobs(dj.data(), dj.size()*sizeof(DeltaEncJob));
			const uint32_t *ds = (const uint32_t *)put_jobs(start.data(), start.size()*4);
			if(!jobs_fit) return ctx_fail(CRTHIP_E_DEVICE, "crthip_encode_batch: job tables");
			if(td.begin(st)) return CRTHIP_E_DEVICE;
			hipLaunchKernelGGL(k_enc_delta, dim3(blocks), dim3(256), 0, st, d, ds, (uint32_t)dj.size());
			if(td.end(st)) return CRTHIP_E_DEVICE;
			BT_TRY(hipGetLastError());
			bt.n_delta++;
		}
	}
	// BORDER counts back (mesh k's attributes from count_at[k] on)
	std::vector<size_t> count_at(n + 1, 0);
	for(uint32_t k = 0; k < n; k++) count_at[k + 1] = count_at[k] + items[ids[k]].attrs.size();
	std::vector<uint32_t> counts(count_at[n] + 1, 0);
	for(uint32_t k = 0; k < n; k++) {
		const BatchItem &it = items[ids[k]];
		if(it.status) continue;
		for(const BatchAttr &A : it.attrs) if(A.codec == CRTHIP_CODEC_NORMAL && A.prediction == 2 && is_mesh(it)) {
			BT_TRY(hipMemcpyAsync(&counts[count_at[k]], base + slot[k].count, 4*it.attrs.size(), hipMemcpyDeviceToHost, st));
			S.bytes_from_device += 4*it.attrs.size();
		}
	}
	BT_TRY(sync());
	bt.quant += tq.ms(); bt.est += te.ms(); bt.delta += td.ms();
	bt.topo_c += ttc.ms(); bt.topo_p += ttp.ms(); bt.topo_w += ttw.ms();
	for(size_t c = 0; c < clouds.size(); c++) { bt.zkeys += tzk[c].ms(); bt.zsort += tzs[c].ms(); }

	// ---- value + entropy coding: every stream of every mesh in one call; the CLERS symbols go up in one copy ----
	std::vector<uint64_t> clers_at(n, 0);
	uint64_t cl = 0;
	const bool clers_in_image = mode != CRTHIP_TOPOLOGY_HOST;     // the device pass wrote its meshes' symbols there; the host's follow them
	if(clers_in_image) {
		const auto t0 = Clock::now();
		bool any = false;
		for(uint32_t k = 0; k < n; k++) {
			const BatchItem &it = items[ids[k]];
			if(it.topo_device || it.clers.empty() || !it.topo_image) continue;
			BT_TRY(hipMemcpyAsync(base + slot[k].clers, it.clers.data(), it.clers.size(), hipMemcpyHostToDevice, st));
			S.bytes_to_device += it.clers.size();
			any = true;
		}
		S.upload_ms += ms_since(t0);
		if(any) BT_TRY(sync());
	} else for(uint32_t k = 0; k < n; k++) { clers_at[k] = cl; cl += al(items[ids[k]].clers.size()); }
	DevMem dclers;
	if(cl) {
		const auto t0 = Clock::now();
		std::vector<uint8_t> h(cl);
		for(uint32_t k = 0; k < n; k++) if(!items[ids[k]].clers.empty()) memcpy(h.data() + clers_at[k], items[ids[k]].clers.data(), items[ids[k]].clers.size());
		S.host_stage_ms += ms_since(t0);
		BT_TRY(hipMalloc(&dclers.p, cl));
		BT_TRY(hipMemcpyAsync(dclers.p, h.data(), cl, hipMemcpyHostToDevice, st));
		BT_TRY(sync());
		S.bytes_to_device += cl;
	}
	std::vector<DevValueStream> vs;
	for(uint32_t k = 0; k < n; k++) {
		BatchItem &it = items[ids[k]];
		if(it.status) continue;
		for(BatchStream &b : it.streams) {
			if(b.kind == BATCH_BITS) continue;
			DevValueStream v;
			v.kind = b.kind; v.entropy = it.entropy; v.components = b.N;
			if(b.attr == -1) { v.count = it.nclers; v.values = clers_in_image ? base + slot[k].clers : dclers.u8() + clers_at[k]; }
			else {
				const BatchAttr &A = it.attrs[b.attr];
				if(A.codec == CRTHIP_CODEC_NORMAL && A.prediction == 2 && is_mesh(it)) b.count = counts[count_at[k] + b.attr];
				v.count = b.count;
				v.values = base + slot[k].d[b.attr];
			}
			vs.push_back(v);
		}
	}
	std::vector<EncValueResult> res;
	{
		const auto t0 = Clock::now();
		const int e = encode_value_streams_device(ctx, vs, res, tm);
		S.value_coder_ms += ms_since(t0);
		if(e) return e;
	}
	S.value_streams += (uint32_t)vs.size();

	// ---- splice: the frame, with every stream where it belongs; zero padding to 4 bytes before a bit stream's words ----
	const auto t_frame = Clock::now();
	size_t r = 0;
	for(uint32_t k = 0; k < n; k++) {
		BatchItem &it = items[ids[k]];
		if(it.status) continue;
		std::vector<uint8_t> &f = blobs[ids[k]];
		f.clear();
		f.reserve(it.frame.size() + 64);
		auto u32 = [&](uint32_t v) { const uint8_t b[4] = {(uint8_t)v, (uint8_t)(v >> 8), (uint8_t)(v >> 16), (uint8_t)(v >> 24)}; f.insert(f.end(), b, b + 4); };
		auto bits = [&](const std::vector<uint32_t> &w) { u32((uint32_t)w.size()); while(f.size() & 3) f.push_back(0); for(uint32_t x : w) u32(x); };
		size_t prev = 0;
		for(const BatchStream &b : it.streams) {
			f.insert(f.end(), it.frame.begin() + prev, it.frame.begin() + b.at); prev = b.at;
			if(b.kind == BATCH_BITS) { bits(it.split_words); continue; }
			const EncValueResult &x = res[r++];
			if(b.kind != CRTHIP_ENC_SYMBOLS) bits(x.words);
			for(const std::vector<uint8_t> &blk : x.blocks) f.insert(f.end(), blk.begin(), blk.end());
		}
		f.insert(f.end(), it.frame.begin() + prev, it.frame.end());
	}
	S.host_frame_ms += (float)ms_since(t_frame);
	return CRTHIP_OK;
}

} // namespace

static int64_t encode_batch_impl(crthip_ctx *ctx, uint32_t n, const crthip_mesh *meshes, const crthip_attr_list *extra, uint32_t host_threads,
                                 uint8_t *out, size_t cap, uint64_t *blob_offset, uint32_t *out_nvert, uint32_t *out_nface,
                                 int32_t *status, crthip_encode_batch_stats *stats, crthip_kernel_times *times) {
	const auto t0 = Clock::now();
	if(!ctx) return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_encode_batch: null context (there is no CPU fallback: use crthip_encode for the host encoder)");
	if(!blob_offset || (n && !meshes)) return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_encode_batch: null argument");
	crthip_encode_batch_stats S;
	memset(&S, 0, sizeof(S));
	if(times) memset(times, 0, sizeof(*times));
	blob_offset[0] = 0;
	if(n == 0) { if(stats) *stats = S; return 0; }
	const uint32_t threads = host_threads ? host_threads : default_threads();
	BT_TRY(hipSetDevice(ctx_device(ctx)));
	{ const int e = ctx_quiesce(ctx); if(e) return e; }

	// per-mesh argument checks; what fails gets its code and an empty range
	std::vector<BatchItem> items(n);
	std::vector<uint32_t> ok;
	for(uint32_t i = 0; i < n; i++) {
		const crthip_mesh *m = &meshes[i];
		int e = encode_check(m);
		if(!e) e = encode_check_attrs(m, extra ? &extra[i] : nullptr, true);
		if(!e && (uint64_t)m->nvert*3 > (1u << 26)) e = ctx_fail(CRTHIP_E_LIMIT, "crthip_encode_batch: too many vertices for the value coder");
		if(!e && m->entropy == CRTHIP_ENTROPY_TUNSTALL && m->nvert > (1u << 23))
			e = ctx_fail(CRTHIP_E_LIMIT, "crthip_encode_batch: a Tunstall stream longer than 2^23 symbols");
		items[i].status = e;
		if(!e) ok.push_back(i);
	}
	// position steps and attribute tables (the steps' sums are the host's, in its order)
	parallel_for((uint32_t)ok.size(), threads, [&](uint32_t k) { items[ok[k]].status = item_guard([&] { batch_setup(&meshes[ok[k]], extra ? &extra[ok[k]] : nullptr, items[ok[k]]); }); });
	ok.erase(std::remove_if(ok.begin(), ok.end(), [&](uint32_t i) { return items[i].status != CRTHIP_OK; }), ok.end());
	// where each mesh's topology pass runs: from the context's mode and the mesh's sizes alone
	const int topo_mode = ctx_encode_topology(ctx);
	if(topo_mode != CRTHIP_TOPOLOGY_HOST)
		for(uint32_t i : ok) {
			BatchItem &it = items[i];
			if(!is_mesh(it)) continue;
			it.topo_image = true;
			it.topo_groups = std::max(meshes[i].ngroups, 1u);
			it.topo_lds = enc_topo_fits_lds(it.nvert_in, it.nface_in);
			it.topo_device = topo_mode == CRTHIP_TOPOLOGY_DEVICE || it.topo_lds;
		}
	S.host_check_ms = ms_since(t0);

	// chunks that fit the device
	size_t free_b = 0, total_b = 0;
	BT_TRY(hipMemGetInfo(&free_b, &total_b));
	const uint64_t budget = free_b/2;
	std::vector<std::vector<uint8_t>> blobs(n);
	BatchTimes bt;
	EncStageTimes tm;
	for(size_t k = 0; k < ok.size();) {
		std::vector<uint32_t> ids;
		uint64_t bytes = 0;
		while(k < ok.size() && (ids.empty() || bytes + item_bytes(items[ok[k]]) <= budget)) { bytes += item_bytes(items[ok[k]]); ids.push_back(ok[k]); k++; }
		if(bytes > budget) return ctx_fail(CRTHIP_E_LIMIT, "crthip_encode_batch: a mesh too big for the device image");
		const int e = run_chunk(ctx, meshes, extra, items, ids, threads, blobs, S, bt, tm);
		if(e) return e;
	}

	uint64_t w = 0;
	for(uint32_t i = 0; i < n; i++) {
		blob_offset[i] = w;
		if(status) status[i] = items[i].status;
		if(out_nvert) out_nvert[i] = items[i].status ? 0 : items[i].nvert;
		if(out_nface) out_nface[i] = items[i].status ? 0 : items[i].nface;
		if(items[i].status) continue;
		if(out && w + blobs[i].size() <= cap) memcpy(out + w, blobs[i].data(), blobs[i].size());
		w += blobs[i].size();
	}
	blob_offset[n] = w;
	S.bytes_to_device += tm.bytes_to_device; S.bytes_from_device += tm.bytes_from_device;
	S.wall_ms = (float)ms_since(t0);
	if(stats) *stats = S;
	if(times) {
		uint32_t c = 0;
		auto add = [&](const char *nm, float ms, uint32_t launches) { if(!launches) return; times->name[c] = nm; times->ms[c] = ms; times->launches[c] = launches; c++; };
		add("enc_quantize_batch", bt.quant, bt.n_quant);
		add("enc_topo_compact", bt.topo_c, bt.n_topo_c);
		add("enc_topo_pair", bt.topo_p, bt.n_topo_p);
		add("enc_topo_walk", bt.topo_w, bt.n_topo_w);
		add("enc_est_normal", bt.est, bt.n_est);
		add("enc_delta", bt.delta, bt.n_delta);
		add("enc_zkeys", bt.zkeys, bt.n_zkeys);
		add("enc_zsort", bt.zsort, bt.n_zsort);
		times->count = c;
		enc_report_times(times, tm);
	}
	return (int64_t)w;
}

// nothing is thrown across the C boundary
extern "C" int64_t crthip_encode_batch_attrs(crthip_ctx *ctx, uint32_t n, const crthip_mesh *meshes, const crthip_attr_list *extra, uint32_t host_threads,
                                             uint8_t *out, size_t cap, uint64_t *blob_offset, uint32_t *out_nvert, uint32_t *out_nface,
                                             int32_t *status, crthip_encode_batch_stats *stats, crthip_kernel_times *times) {
	try {
		return encode_batch_impl(ctx, n, meshes, extra, host_threads, out, cap, blob_offset, out_nvert, out_nface, status, stats, times);
	} catch(const std::bad_alloc &) {
		return ctx_fail(CRTHIP_E_NOMEM, nullptr);
	} catch(...) {
		return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_encode_batch: internal error");
	}
}

extern "C" int64_t crthip_encode_batch(crthip_ctx *ctx, uint32_t n, const crthip_mesh *meshes, uint32_t host_threads,
                                       uint8_t *out, size_t cap, uint64_t *blob_offset, uint32_t *out_nvert, uint32_t *out_nface,
                                       int32_t *status, crthip_encode_batch_stats *stats, crthip_kernel_times *times) {
	return crthip_encode_batch_attrs(ctx, n, meshes, nullptr, host_threads, out, cap, blob_offset, out_nvert, out_nface, status, stats, times);
}
