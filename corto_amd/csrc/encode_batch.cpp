// encode_batch.cpp — crthip_encode_batch: a batch of meshes and point clouds in, one .crt per item out, every blob byte-identical
// to crthip_encode of that item.
//
// The serial part - the CLERS topology pass, which reads the index alone - runs on a pool of host threads while the device
// quantises (encoder.cpp: batch_topology), or, where the context asks for it (crthip_ctx_set_encode_topology), on the device behind the
// quantiser (k_encode_topo.hip, enc_topology.h): the compacted faces, the quads and the CLERS symbols are then written where the next
// kernels read them, and one record per mesh comes back for its frame (encoder.cpp: batch_frame).  Everything per vertex runs on the
// device and stays resident until the coded streams come back (k_encode_batch.hip): quantisation, estimated normals, residuals, the
// point clouds' Morton sort (one cloud after another: each has its own launches), then the value and Tunstall coders (encode_gpu.cpp:
// encode_value_streams_device), which bring their payload back.  The host writes every container from its frame and the coded streams
// (enc_splice.h: write_container, into a ByteOut).  One device image per chunk of the batch; no allocation per mesh or per stream.
//
// crthip_encode_batch_to_device shares every stage and differs in one argument of code_values and in the tail: the coders leave their
// payload on the device, the same writer runs into a SplicePlan - where every byte of every container goes in the caller's device arena
// (enc_splice.h) - the host uploads what it made itself as one literal buffer beside the job table, and k_enc_splice moves the pieces
// (splice_to_device).
//
// crthip_encode_batch_resident is the same path for data arrays that live in device memory: the pointers are vouched for by the runtime
// (resident_check), what the host would have read through them comes from K-ENC-CHECK (input_pass: k_encode_check.hip), the quantiser
// and the device topology pass read the caller's arrays in place, and only the index of a mesh the host pool walks comes back
// (fetch_indices).
//
// crthip_encode_batch_layout is the same path again for arrays read through a crthip_mesh_layout (strides, a uint16 index, int16 normals, an
// origin): layout_resolve leaves a MeshRead per item, the requests and jobs carry its fields, host arrays are packed by upload_inputs'
// staging copy and resident ones are read where they lie; its host output is the device arena's form (HostArena).
//
// How the file is laid out: ChunkImage / build_image say where everything lives in a chunk's device image (the one place that does: the
// chunker sizes a chunk by building its image); Chunk is what every stage works on; the stages follow, one function each, in the order
// encode_chunk calls them.  Each stage's comment names the regions of the image it reads (R) and writes (W) and says whether it returns
// with the stream synchronised.
#include <hip/hip_runtime.h>
#include <sched.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <initializer_list>
#include <mutex>
#include <thread>
#include <vector>

#include "../../include/corto_hip.h"
#include "device_plan.h"
#include "enc_splice.h"
#include "enc_topology.h"
#include "encoder_internal.h"
#include "kernels.h"
#include "pool_internal.h"

using namespace corto_hip;

namespace {

using Clock = std::chrono::steady_clock;
double ms_since(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }

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

uint32_t rs_blocks(uint32_t n) { return std::max(1u, (n + RS_TILE - 1)/RS_TILE); }
bool is_mesh(const BatchItem &it) { return it.nface_in > 0; }
// normals whose residuals are against the estimate (a cloud's estimate is all zeros: its ESTIMATED normals still subtract toOcta of it)
bool est_of(const BatchItem &it, const BatchAttr &a) { return a.codec == CRTHIP_CODEC_NORMAL && (a.prediction == 1 || (a.prediction == 2 && is_mesh(it))); }
bool border_of(const BatchItem &it, const BatchAttr &a) { return a.codec == CRTHIP_CODEC_NORMAL && a.prediction == 2 && is_mesh(it); }   // BORDER normals: the device counts their residuals
constexpr uint64_t DIRECT_BYTES = 1u << 20;               // inputs from this size up go to the device straight from the caller's array
                                                          // (any element size and byte count: slots are 256-byte aligned, a copy is bytes)

// ---- the chunk's device image ----

// where one item lives in it
struct Slot {
	std::vector<uint64_t> in, q, d;       // per attribute: raw input, quantised values, residuals
	uint64_t quads = 0, boundary = 0, count = 0;
	uint64_t zkeys[2] = {0, 0}, zvals[2] = {0, 0}, zhist = 0, zmn = 0;
	uint64_t clers = 0;
	uint64_t idx = 0, gend_in = 0, gend_out = 0, first = 0, cursor = 0, sides = 0, twin = 0, state = 0, split = 0;   // the device topology pass
	uint32_t fbase = 0;                   // first face in the faces region (faces units)
};
// stride != 0: a host array read through a crthip_mesh_layout - `elem` bytes a vertex, `stride` apart - that the staging copy packs
struct RawIn {
	const void *src; uint64_t bytes, off; uint32_t stride = 0, elem = 0;
	bool direct() const { return bytes >= DIRECT_BYTES && !stride; }    // goes up straight from the caller's array
};

// Every offset of one chunk's image and the totals its copies need.  Items are named by k, their place in ids.
struct ChunkImage {
	std::vector<uint32_t> ids;            // the chunk's items (indices of the batch)
	// whose topology pass runs where: devk on the device (CRTHIP_TOPOLOGY_DEVICE: every mesh, _SPLIT: those that walk in LDS), hostk (the
	// other meshes, and every cloud's frame) on the host
	std::vector<uint32_t> devk, hostk, clouds;
	std::vector<Slot> slot;
	std::vector<RawIn> raw;               // every raw attribute; for a mesh of the device pass also its index and group ends (given
	                                      // without groups it is one group, which ends at its face count)
	uint64_t zero = 0, zflags = 0, back = 0, mquads = 0, faces = 0, ck[2] = {0, 0}, cv[2] = {0, 0}, chist = 0, spack = 0, jobs = 0, total = 0;
	uint64_t staged_total = 0, zero_bytes = 0, back_bytes = 0, mquads_bytes = 0, split_cap_total = 0;
	uint32_t faces_total = 0, corners_total = 0;
	bool resident = false;                // crthip_encode_batch_resident: the caller's arrays are read where they are - raw holds the group ends alone
	uint64_t rec(size_t j) const { return back + 256 + j*sizeof(EncTopoRecord); }   // the record of mesh devk[j]
};

// The image of items[ids], without touching the device.  Every region starts on 256 bytes unless it says otherwise.
ChunkImage build_image(const crthip_mesh *meshes, const std::vector<BatchItem> &items, std::vector<uint32_t> ids, bool resident) {
	ChunkImage L;
	L.resident = resident;
	Carver c;
	auto here = [&] { return c.take(0); };                  // where the next region starts
	const uint32_t n = (uint32_t)ids.size();
	L.ids = std::move(ids);
	L.slot.resize(n);
	std::vector<uint64_t *> raw_off;                         // raw[i]'s offset in its slot
	uint64_t job_bytes = 0;
	for(uint32_t k = 0; k < n; k++) {
		const BatchItem &it = items[L.ids[k]];
		Slot &s = L.slot[k];
		(it.topo_device ? L.devk : L.hostk).push_back(k);
		if(!is_mesh(it)) L.clouds.push_back(k);
		s.in.resize(it.attrs.size()); s.q.resize(it.attrs.size()); s.d.resize(it.attrs.size());
		if(!resident) for(size_t a = 0; a < it.attrs.size(); a++) {
			const QuantRequest &r = it.attrs[a].quant;
			const uint32_t elem = (uint32_t)quant_vertex_bytes(r);
			L.raw.push_back(RawIn{r.in, quant_in_bytes(r), 0, r.stride == elem ? 0u : r.stride, elem}); raw_off.push_back(&s.in[a]);
		}
		if(it.topo_device) {
			const crthip_mesh &m = meshes[L.ids[k]];
			if(!resident) { L.raw.push_back(RawIn{m.index, (uint64_t)it.nface_in*(it.index16 ? 6 : 12), 0}); raw_off.push_back(&s.idx); }
			L.raw.push_back(RawIn{m.ngroups ? (const void *)m.group_end : (const void *)&it.nface_in, (uint64_t)it.topo_groups*4, 0}); raw_off.push_back(&s.gend_in);
		}
		job_bytes += it.attrs.size()*(sizeof(QuantJob) + sizeof(DeltaEncJob) + sizeof(EstJob) + 8) + 16 + (it.topo_device ? sizeof(EncTopoJob) + 8 : 0);
	}
	// INVARIANT: the raw inputs below DIRECT_BYTES are contiguous at the front of the image - they go up staged, in one copy of
	// staged_total bytes from offset 0 - and the large ones follow
	// (a resident call's are the group ends alone: words, packed)
	for(int big = 0; big < 2; big++)
		for(size_t i = 0; i < L.raw.size(); i++) if(L.raw[i].direct() == (big == 1)) *raw_off[i] = L.raw[i].off = c.take(L.raw[i].bytes, resident ? 4 : 256);
	for(const RawIn &r : L.raw) if(!r.direct()) L.staged_total = std::max(L.staged_total, r.off + r.bytes);
	// INVARIANT: the zeroed words (BORDER XORs, counts, cloud minima), the clouds' flags and the device topology pass's report are
	// contiguous - one memset of zero_bytes from `zero` - and the report is one block: it comes back in one copy of back_bytes from `back`
	L.zero = here();
	for(uint32_t k = 0; k < n; k++) {
		const BatchItem &it = items[L.ids[k]];
		L.slot[k].count = c.take(256);
		if(is_mesh(it)) { for(const BatchAttr &a : it.attrs) if(border_of(it, a)) L.slot[k].boundary = c.take((uint64_t)it.nvert_in*4); }
		else L.slot[k].zmn = c.take(256);
	}
	L.zflags = c.take((uint64_t)n*4);                        // every cloud's equal-key flag, read back in one copy
	L.back = here();                                         // the report: the split words' count, a record per mesh (rec()), the new group ends (packed)
	if(!L.devk.empty()) {
		c.take(256); c.take(L.devk.size()*sizeof(EncTopoRecord));
		here();                                              // (the group ends start on 256 and are packed from there)
		for(uint32_t k : L.devk) L.slot[k].gend_out = c.take((uint64_t)items[L.ids[k]].topo_groups*4, 4);
	}
	L.back_bytes = here() - L.back;
	L.zero_bytes = here() - L.zero;
	for(uint32_t k = 0; k < n; k++) {
		const BatchItem &it = items[L.ids[k]];
		Slot &s = L.slot[k];
		for(size_t a = 0; a < it.attrs.size(); a++) { s.q[a] = c.take(quant_out_bytes(it.attrs[a].quant)); s.d[a] = c.take(quant_out_bytes(it.attrs[a].quant)); }
		if(is_mesh(it)) {
			s.fbase = L.faces_total; L.faces_total += it.nface_in;
			for(const BatchAttr &a : it.attrs) if(est_of(it, a)) L.corners_total += 3*it.nface_in;
		} else {
			for(int b = 0; b < 2; b++) { s.zkeys[b] = c.take((uint64_t)it.nvert_in*8); s.zvals[b] = c.take((uint64_t)it.nvert_in*4); }
			s.quads = c.take((uint64_t)it.nvert_in*16);
			s.zhist = c.take(256ull*4*rs_blocks(it.nvert_in));
		}
	}
	// INVARIANT: the meshes' quads lie back to back in item order (16-byte records, no padding between meshes), and so do their faces
	// (fbase): one upload each per run of neighbouring meshes the host made
	L.mquads = here();
	for(uint32_t k = 0; k < n; k++) if(is_mesh(items[L.ids[k]])) L.slot[k].quads = c.take((uint64_t)items[L.ids[k]].nvert_in*16, 16);
	L.mquads_bytes = c.off - L.mquads;
	L.faces = c.take((uint64_t)L.faces_total*12);
	for(int b = 0; b < 2; b++) { L.ck[b] = c.take((uint64_t)L.corners_total*4); L.cv[b] = c.take((uint64_t)L.corners_total*4); }
	L.chist = c.take(256ull*4*rs_blocks(L.corners_total));
	// the device topology pass's scratch, and (every mode but HOST) each mesh's CLERS symbols where the value coder reads them
	for(uint32_t k : L.devk) {
		const BatchItem &it = items[L.ids[k]];
		const uint64_t nf = it.nface_in, nv = it.nvert_in;
		Slot &s = L.slot[k];
		s.first = c.take((nv + 1)*4);
		s.cursor = c.take(nv*4);
		s.sides = c.take(nf*3*sizeof(EncTopoSide));
		s.twin = c.take(nf*12);
		if(!it.topo_lds) s.state = c.take(enc_topo_state_bytes<uint32_t>(it.nface_in, it.nvert_in));
		s.split = c.take(enc_topo_split_cap(it.nface_in)*4);
		L.split_cap_total += enc_topo_split_cap(it.nface_in);
	}
	L.spack = c.take(L.split_cap_total*4);
	for(uint32_t k = 0; k < n; k++) if(items[L.ids[k]].topo_image) L.slot[k].clers = c.take(enc_topo_clers_cap(items[L.ids[k]].nface_in));
	L.jobs = c.take(1u << 16);                               // job tables, rewritten stage by stage (stream-ordered): Chunk::put_jobs
	c.take(3*job_bytes);
	L.total = here();
	return L;
}

// host mode's CLERS symbols go up in an allocation of their own, sized once the passes have made them: item k's at at[k] (one entry
// per item); returns its bytes
uint64_t clers_layout(const std::vector<BatchItem> &items, const ChunkImage &img, std::vector<uint64_t> &at) {
	Carver c;
	for(size_t k = 0; k < at.size(); k++) at[k] = c.take(items[img.ids[k]].clers.size());
	return c.take(0);
}

// ---- what every stage works on ----

// the batch's kernels as crthip_kernel_times names them, in the order they are reported; up to K_STAGES one timer per chunk, then one per cloud
enum { K_IN_CHECK, K_IN_REDUCE, K_QUANT, K_TOPO_C, K_TOPO_P, K_TOPO_W, K_EST, K_DELTA, K_STAGES, K_ZKEYS = K_STAGES, K_ZSORT, K_COUNT };
const char *const KERNEL_NAME[K_COUNT] = {"enc_input_check", "enc_input_reduce", "enc_quantize_batch", "enc_topo_compact", "enc_topo_pair", "enc_topo_walk", "enc_est_normal", "enc_delta", "enc_zkeys", "enc_zsort"};
struct BatchTimes { float ms[K_COUNT] = {}; uint32_t launches[K_COUNT] = {}; };
struct Event {
	hipEvent_t e = nullptr;
	~Event() { if(e) (void)hipEventDestroy(e); }
	int record(hipStream_t st) { if(!e) ENC_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming)); ENC_TRY(hipEventRecord(e, st)); return 0; }
};

// One chunk in flight.  encode_chunk owns it together with the guards (Joiner, DevMem, Drain); a stage that returns early relies on those
// and releases nothing itself.  Host buffers that a queued copy reads or writes live here, so they outlive the Drain.
struct Chunk {
	crthip_ctx *ctx; hipStream_t st;
	const crthip_mesh *meshes; const crthip_attr_list *extra;
	std::vector<BatchItem> &items; const ChunkImage &img;
	crthip_encode_batch_stats &S; BatchTimes &bt; EncStageTimes &tm;
	// the host's topology passes: what the pool thread and the stages share (the pool thread's lambdas hold references to this Chunk)
	std::vector<uint8_t> ready = std::vector<uint8_t>(img.ids.size(), 0);   // per k: its pass (a mesh) or its frame (a cloud) is done; guarded by mu, signalled on cv
	std::mutex mu; std::condition_variable cv;
	Clock::time_point t_topo = Clock::now();
	double topo_ms = 0;                                      // from t_topo until the last pass finished
	uint8_t *base = nullptr;
	Carver job_cursor{img.jobs};                             // the job tables' region: [img.jobs, img.total)
	std::vector<std::vector<uint8_t>> keep;                  // the job tables' host copies live until the chunk has finished
	bool jobs_fit = true;
	EventTimer t[K_STAGES];
	std::vector<EventTimer> tzk, tzs;                             // per cloud
	Event ev_back;                                           // behind the copy of the device topology pass's report into `back`
	std::vector<uint8_t> back = std::vector<uint8_t>(img.back_bytes);
	Clock::time_point t_dtopo;
	// a resident call: every item's descriptor again, with the index of a mesh the host pool walks pointing into host_index (fetch_indices)
	std::vector<crthip_mesh> shadow;
	std::vector<uint32_t> host_index;
	std::vector<uint16_t> host_index16;                      // a resident call's uint16 indices as they came back, before they are widened

	uint32_t n() const { return (uint32_t)img.ids.size(); }
	BatchItem &item(uint32_t k) const { return items[img.ids[k]]; }
	const crthip_mesh *mesh(uint32_t k) const { return shadow.empty() ? &meshes[img.ids[k]] : &shadow[k]; }
	const crthip_attr_list *attrs(uint32_t k) const { return extra ? &extra[img.ids[k]] : nullptr; }
	template <class T> T *at(uint64_t off) const { return (T *)(base + off); }
	hipError_t sync() { const auto t0 = Clock::now(); const hipError_t e = hipStreamSynchronize(st); S.sync_wait_ms += ms_since(t0); return e; }
	uint8_t *put_jobs(const void *p, size_t bytes) {
		const uint64_t off = job_cursor.take(bytes);
		if(off + bytes > img.total) { jobs_fit = false; return nullptr; }
		if(bytes) {
			keep.emplace_back((const uint8_t *)p, (const uint8_t *)p + bytes);
			if(hipMemcpyAsync(base + off, keep.back().data(), bytes, hipMemcpyHostToDevice, st) != hipSuccess) jobs_fit = false;
			S.bytes_to_device += bytes;
		}
		return base + off;
	}
	// the topology pass (a mesh) or the frame (a cloud) of item k on the host; runs on the pool, or inline (device mode's clouds)
	void host_pass(uint32_t k) {
		const int32_t e = item_guard([&] { batch_topology(mesh(k), attrs(k), item(k)); });
		if(e) item(k).status = e;                                // read by this thread's caller only after the join
		{ std::lock_guard<std::mutex> g(mu); ready[k] = 1; }
		cv.notify_all();
	}
};

// A stage's job table and its block-start arrays go up behind the previous stage's; `launch(jobs, starts)` then runs between the events
// of the timers `first` and `last` (K_*; one timer for most stages).  launch returns 0 or the error it has reported.
template <class J, class L>
int launch_jobs(Chunk &C, const std::vector<J> &jobs, std::initializer_list<const std::vector<uint32_t> *> starts, int first, int last, L launch) {
	const J *dj = (const J *)C.put_jobs(jobs.data(), jobs.size()*sizeof(J));
	const uint32_t *ds[3] = {nullptr, nullptr, nullptr};
	size_t i = 0;
	for(const std::vector<uint32_t> *s : starts) ds[i++] = (const uint32_t *)C.put_jobs(s->data(), s->size()*4);
	if(!C.jobs_fit) return ctx_fail(CRTHIP_E_DEVICE, "crthip_encode_batch: job tables");
	if(C.t[first].begin(C.st)) return CRTHIP_E_DEVICE;
	{ const int e = launch(dj, ds); if(e) return e; }
	if(C.t[last].end(C.st)) return CRTHIP_E_DEVICE;
	ENC_TRY(hipGetLastError());
	return 0;
}

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
	ENC_TRY(hipGetLastError());
	return 0;
}

// ---- the stages, in the order encode_chunk runs them ----

// Meshes whose topology pass runs on the host pool (hostk) need a uint32 index in host memory.  A resident call's is copied back - one copy
// each into one host buffer, a uint16 index as it is - and after one wait the 16-bit ones are widened; a host call's uint16 index is
// widened where it lies.  The pool works on descriptors whose index is that copy.  Attributes never come back.  R: the caller's index
// arrays.  Synchronised on every way out (the buffers are the chunk's, the copies are queued).
int fetch_indices(Chunk &C) {
	struct Wait { hipStream_t st; ~Wait() { (void)hipStreamSynchronize(st); } } wait{C.st};
	std::vector<uint64_t> at(C.n(), 0), at16(C.n(), 0);
	uint64_t words = 0, narrow = 0;
	for(uint32_t k : C.img.hostk) {
		const BatchItem &it = C.item(k);
		if(!is_mesh(it) || !(C.img.resident || it.index16)) continue;
		at[k] = words; words += (uint64_t)it.nface_in*3;
		if(C.img.resident && it.index16) { at16[k] = narrow; narrow += (uint64_t)it.nface_in*3; }
	}
	C.host_index.resize(words); C.host_index16.resize(narrow);
	std::vector<crthip_mesh> shadow(C.n());
	for(uint32_t k = 0; k < C.n(); k++) shadow[k] = C.meshes[C.img.ids[k]];
	for(uint32_t k : C.img.hostk) {
		const BatchItem &it = C.item(k);
		if(!is_mesh(it) || !(C.img.resident || it.index16)) continue;
		const uint64_t entries = (uint64_t)it.nface_in*3;
		if(!C.img.resident) {
			const uint16_t *ix = (const uint16_t *)shadow[k].index;
			for(uint64_t i = 0; i < entries; i++) C.host_index[at[k] + i] = ix[i];
		} else {
			const uint64_t bytes = entries*(it.index16 ? 2 : 4);
			void *dst = it.index16 ? (void *)(C.host_index16.data() + at16[k]) : (void *)(C.host_index.data() + at[k]);
			ENC_TRY(hipMemcpyAsync(dst, shadow[k].index, bytes, hipMemcpyDeviceToHost, C.st));
			C.S.bytes_from_device += bytes;
		}
		shadow[k].index = C.host_index.data() + at[k];
	}
	if(words && C.img.resident) ENC_TRY(C.sync());
	for(uint32_t k : C.img.hostk) {
		const BatchItem &it = C.item(k);
		if(!is_mesh(it) || !C.img.resident || !it.index16) continue;
		for(uint64_t i = 0; i < (uint64_t)it.nface_in*3; i++) C.host_index[at[k] + i] = C.host_index16[at16[k] + i];
	}
	C.shadow.swap(shadow);
	return 0;
}

// Raw inputs up: small ones staged into one copy, large ones straight from the caller; then the zeroed block is cleared.
// W: every raw input (slot.in, idx, gend_in), [zero, zero + zero_bytes).  Synchronised after the copies (the staging buffer is a local);
// the memset is left queued.
int upload_inputs(Chunk &C) {
	const auto t_stage = Clock::now();
	std::vector<uint8_t> stage(C.img.staged_total);
	for(const RawIn &r : C.img.raw) {
		const uint64_t b = r.bytes;
		if(!b) continue;
		if(r.stride) for(uint64_t v = 0; v < b/r.elem; v++) memcpy(stage.data() + r.off + v*r.elem, (const uint8_t *)r.src + v*r.stride, r.elem);   // (packed here)
		else if(b < DIRECT_BYTES) memcpy(stage.data() + r.off, r.src, b);
		else { const auto t0 = Clock::now(); ENC_TRY(hipMemcpyAsync(C.base + r.off, r.src, b, hipMemcpyHostToDevice, C.st)); C.S.upload_ms += ms_since(t0); }
		if(r.direct()) C.S.bytes_to_device += b;
	}
	C.S.host_stage_ms += ms_since(t_stage);
	{ const auto t0 = Clock::now(); if(C.img.staged_total) ENC_TRY(hipMemcpyAsync(C.base, stage.data(), C.img.staged_total, hipMemcpyHostToDevice, C.st)); C.S.upload_ms += ms_since(t0); }
	C.S.bytes_to_device += C.img.staged_total;
	ENC_TRY(C.sync());
	if(C.img.zero_bytes) ENC_TRY(hipMemsetAsync(C.base + C.img.zero, 0, C.img.zero_bytes, C.st));
	return 0;
}

// K-ENC-Q: every attribute of every item in one launch.  R: slot.in (a resident call: the caller's arrays).  W: slot.q, job tables.  Not synchronised.
int stage_quantise(Chunk &C) {
	std::vector<QuantJob> qj; std::vector<uint32_t> start;
	uint32_t blocks = 0;
	for(uint32_t k = 0; k < C.n(); k++) {
		const BatchItem &it = C.item(k);
		for(size_t a = 0; a < it.attrs.size(); a++) {
			const QuantRequest &r = it.attrs[a].quant;
			if(!r.count) continue;
			qj.push_back(quant_job(r, C.img.resident ? r.in : C.base + C.img.slot[k].in[a], C.base + C.img.slot[k].q[a], !C.img.resident)); start.push_back(blocks); blocks += (r.count + 255)/256;
		}
	}
	if(qj.empty()) return 0;
	start.push_back(blocks);
	const int e = launch_jobs(C, qj, {&start}, K_QUANT, K_QUANT, [&](const QuantJob *dj, const uint32_t *const *ds) {
		hipLaunchKernelGGL(k_enc_quantize_batch, dim3(blocks), dim3(256), 0, C.st, dj, ds[0], (uint32_t)qj.size());
		return 0;
	});
	if(!e) C.bt.launches[K_QUANT]++;
	return e;
}

// K-ENC-TOPO: the topology pass of the meshes in devk, behind the quantiser; their report starts back at once.
// R: slot.idx (a resident call: the caller's index), gend_in.  W: faces, slot.quads, clers, gend_out, the records and the split cursor (the report), spack, the pass's scratch
// (first, cursor, sides, twin, state, split), job tables.  Not synchronised: ev_back says when the report is in C.back.
int stage_topology(Chunk &C) {
	C.t_dtopo = Clock::now();
	const uint32_t nd = (uint32_t)C.img.devk.size();
	if(!nd) return 0;
	std::vector<EncTopoJob> tj(nd);
	std::vector<uint32_t> walk_ids;                          // the LDS-resident walks first, then the global ones
	uint32_t nlds = 0, lds_bytes = 0;
	for(int pass = 0; pass < 2; pass++) for(uint32_t j = 0; j < nd; j++) if(C.item(C.img.devk[j]).topo_lds == (pass == 0)) walk_ids.push_back(j);
	for(uint32_t j = 0; j < nd; j++) {
		const BatchItem &it = C.item(C.img.devk[j]);
		const Slot &s = C.img.slot[C.img.devk[j]];
		EncTopoJob &J = tj[j];
		memset(&J, 0, sizeof(J));
		J.index = C.img.resident ? (const void *)C.mesh(C.img.devk[j])->index : C.at<const void>(s.idx); J.index16 = it.index16; J.gend_in = C.at<const uint32_t>(s.gend_in);
		J.faces = C.at<uint32_t>(C.img.faces) + (size_t)s.fbase*3; J.gend_out = C.at<uint32_t>(s.gend_out);
		J.first = C.at<uint32_t>(s.first); J.cursor = C.at<uint32_t>(s.cursor);
		J.sides = C.at<EncTopoSide>(s.sides); J.twin = C.at<uint32_t>(s.twin);
		J.state = it.topo_lds ? nullptr : C.base + s.state;
		J.quads = C.at<uint32_t>(s.quads); J.clers = C.base + s.clers; J.split = C.at<uint32_t>(s.split);
		J.split_packed = C.at<uint32_t>(C.img.spack); J.split_cursor = C.at<uint32_t>(C.img.back);
		J.rec = C.at<EncTopoRecord>(C.img.rec(j));
		J.nvert = it.nvert_in; J.nface = it.nface_in; J.ngroups = it.topo_groups;
		if(it.topo_lds) { nlds++; lds_bytes = std::max(lds_bytes, (uint32_t)enc_topo_state_bytes<uint16_t>(it.nface_in, it.nvert_in)); }
	}
	const int e = launch_jobs(C, tj, {&walk_ids}, K_TOPO_C, K_TOPO_W, [&](const EncTopoJob *dj, const uint32_t *const *ds) {
		hipLaunchKernelGGL(k_enc_topo_compact, dim3(nd), dim3(ETOPO_THREADS), 0, C.st, dj, nd);
		if(C.t[K_TOPO_C].end(C.st) || C.t[K_TOPO_P].begin(C.st)) return (int)CRTHIP_E_DEVICE;
		hipLaunchKernelGGL(k_enc_topo_pair, dim3(nd), dim3(ETOPO_THREADS), 0, C.st, dj, nd);
		if(C.t[K_TOPO_P].end(C.st) || C.t[K_TOPO_W].begin(C.st)) return (int)CRTHIP_E_DEVICE;
		if(nlds) hipLaunchKernelGGL(k_enc_topo_walk<true>, dim3(nlds), dim3(ETOPO_THREADS), lds_bytes, C.st, dj, ds[0], nlds);
		if(nd > nlds) hipLaunchKernelGGL(k_enc_topo_walk<false>, dim3(nd - nlds), dim3(ETOPO_THREADS), 0, C.st, dj, ds[0] + nlds, nd - nlds);
		return 0;
	});
	if(e) return e;
	C.bt.launches[K_TOPO_C]++; C.bt.launches[K_TOPO_P]++; C.bt.launches[K_TOPO_W] += (nlds ? 1u : 0u) + (nd > nlds ? 1u : 0u);
	ENC_TRY(hipMemcpyAsync(C.back.data(), C.base + C.img.back, C.img.back_bytes, hipMemcpyDeviceToHost, C.st));
	if(C.ev_back.record(C.st)) return CRTHIP_E_DEVICE;
	C.S.bytes_from_device += C.img.back_bytes;
	C.S.topology_device += nd; C.S.topology_lds += nlds;
	return 0;
}

// The clouds' Morton keys and radix sort, one cloud after another.  R: slot.q of the position.  W: zmn, zkeys, zvals, zhist, slot.quads
// (the sorted order as a prediction), the cloud's flag in zflags.  Not synchronised.
int stage_cloud_sort(Chunk &C) {
	C.tzk = std::vector<EventTimer>(C.img.clouds.size()); C.tzs = std::vector<EventTimer>(C.img.clouds.size());
	for(size_t c = 0; c < C.img.clouds.size(); c++) {
		const uint32_t k = C.img.clouds[c];
		const BatchItem &it = C.item(k);
		const Slot &s = C.img.slot[k];
		if(it.nvert_in == 0) continue;
		ZJob Z{};
		Z.coords = C.at<const int32_t>(s.q[it.pos]);
		Z.mn = C.at<int32_t>(s.zmn); Z.flag = C.at<uint32_t>(C.img.zflags) + k; Z.n = it.nvert_in;
		Z.keys = C.at<uint64_t>(s.zkeys[0]); Z.vals = C.at<uint32_t>(s.zvals[0]);
		const uint32_t g = (it.nvert_in + 255)/256;
		if(C.tzk[c].begin(C.st)) return CRTHIP_E_DEVICE;
		hipLaunchKernelGGL(k_enc_zmin, dim3(g), dim3(256), 0, C.st, Z);
		hipLaunchKernelGGL(k_enc_zkeys, dim3(g), dim3(256), 0, C.st, Z);
		if(C.tzk[c].end(C.st)) return CRTHIP_E_DEVICE;
		C.bt.launches[K_ZKEYS] += 2;
		int where = 0; uint32_t launches = 0;
		if(C.tzs[c].begin(C.st)) return CRTHIP_E_DEVICE;
		{ const int e = radix_sort(C.st, Z.keys, Z.vals, C.at<uint64_t>(s.zkeys[1]), C.at<uint32_t>(s.zvals[1]), C.at<uint32_t>(s.zhist), it.nvert_in, 64, where, launches); if(e) return e; }
		Z.keys = C.at<uint64_t>(s.zkeys[where]); Z.vals = C.at<uint32_t>(s.zvals[where]);
		Z.quads = C.at<uint32_t>(s.quads);
		hipLaunchKernelGGL(k_enc_zflag, dim3(g), dim3(256), 0, C.st, Z);
		if(C.tzs[c].end(C.st)) return CRTHIP_E_DEVICE;
		ENC_TRY(hipGetLastError());
		C.bt.launches[K_ZSORT] += launches + 1;
	}
	return 0;
}

// The device pass's report: each mesh's frame from its counts, group ends and split words (those came packed: a second copy).
// R: the report (through C.back), spack.  Waits for ev_back; synchronised only if split words came back.
int collect_device_passes(Chunk &C) {
	const ChunkImage &I = C.img;
	{ const auto t0 = Clock::now(); ENC_TRY(hipEventSynchronize(C.ev_back.e)); C.S.sync_wait_ms += ms_since(t0); }
	C.S.device_topology_ms += (float)ms_since(C.t_dtopo);
	uint32_t nwords = 0;
	memcpy(&nwords, C.back.data(), 4);
	std::vector<uint32_t> words(nwords);
	if(nwords > I.split_cap_total) return ctx_fail(CRTHIP_E_DEVICE, "crthip_encode_batch: the device topology pass's split words");
	if(nwords) {
		ENC_TRY(hipMemcpyAsync(words.data(), C.base + I.spack, (size_t)nwords*4, hipMemcpyDeviceToHost, C.st));
		ENC_TRY(C.sync());
		C.S.bytes_from_device += (uint64_t)nwords*4;
	}
	const auto t0 = Clock::now();
	for(uint32_t j = 0; j < I.devk.size(); j++) {
		const uint32_t k = I.devk[j];
		BatchItem &it = C.item(k);
		EncTopoRecord R;
		memcpy(&R, C.back.data() + (I.rec(j) - I.back), sizeof(R));
		if(R.status || R.nvert > it.nvert_in || R.nface > it.nface_in || (uint64_t)R.split_off + R.split_words > nwords || R.nclers > enc_topo_clers_cap(it.nface_in)) {
			it.status = ctx_fail(CRTHIP_E_DEVICE, "crthip_encode_batch: the device topology pass stopped at a bound");
			continue;
		}
		const int32_t e = item_guard([&] {
			batch_frame(C.mesh(k), C.attrs(k), it, R, (const uint32_t *)(C.back.data() + (I.slot[k].gend_out - I.back)), words.data() + R.split_off);
		});
		if(e) it.status = e;
	}
	C.S.host_frame_ms += (float)ms_since(t0);
	return 0;
}

// The topology passes' results.  Device mode's clouds get their frames here, inline; then the device pass's report
// (collect_device_passes); then the host's passes as they finish: each mesh's faces and quads are staged as soon as its pass is done, and
// go up in two copies per run of neighbouring meshes the host made (all of them, without a device pass; one copy per mesh measured
// slower: 24.5 against 20.4 ms for 256 C4 units, tools/encode_batch_rate.py).  W: faces, slot.quads of those meshes.  Synchronised (the
// staging buffers are locals); every host pass has finished when it returns.
int collect_passes(Chunk &C, int mode) {
	const ChunkImage &I = C.img;
	if(mode == CRTHIP_TOPOLOGY_DEVICE) { for(uint32_t k : I.hostk) C.host_pass(k); C.topo_ms = ms_since(C.t_topo); }   // (the clouds' frames)
	if(!I.devk.empty()) { const int e = collect_device_passes(C); if(e) return e; }
	std::vector<uint8_t> up_quads(I.mquads_bytes), up_faces((size_t)I.faces_total*12);
	for(uint32_t k = 0; k < C.n(); k++) {
		{ const auto tw = Clock::now(); std::unique_lock<std::mutex> g(C.mu); C.cv.wait(g, [&] { return C.ready[k] != 0; }); C.S.topology_wait_ms += ms_since(tw); }
		BatchItem &it = C.item(k);
		if(!is_mesh(it) || it.topo_device) continue;
		const auto t0 = Clock::now();
		const size_t fb = std::min(it.faces.size()*4, (size_t)it.nface_in*12), qb = std::min(it.quads.size()*4, (size_t)it.nvert_in*16);
		if(fb) memcpy(up_faces.data() + (size_t)I.slot[k].fbase*12, it.faces.data(), fb);
		if(qb) memcpy(up_quads.data() + (I.slot[k].quads - I.mquads), it.quads.data(), qb);
		C.S.host_stage_ms += ms_since(t0);
	}
	const auto t0 = Clock::now();
	std::vector<uint32_t> mk;
	for(uint32_t k = 0; k < C.n(); k++) if(is_mesh(C.item(k))) mk.push_back(k);
	for(size_t a = 0; a < mk.size();) {
		if(C.item(mk[a]).topo_device) { a++; continue; }
		size_t b = a;
		while(b + 1 < mk.size() && !C.item(mk[b + 1]).topo_device) b++;
		const BatchItem &last = C.item(mk[b]);
		const uint64_t q0 = I.slot[mk[a]].quads, q1 = I.slot[mk[b]].quads + (uint64_t)last.nvert_in*16;
		const uint64_t f0 = (uint64_t)I.slot[mk[a]].fbase*12, f1 = ((uint64_t)I.slot[mk[b]].fbase + last.nface_in)*12;
		if(q1 > q0) ENC_TRY(hipMemcpyAsync(C.base + q0, up_quads.data() + (q0 - I.mquads), q1 - q0, hipMemcpyHostToDevice, C.st));
		if(f1 > f0) ENC_TRY(hipMemcpyAsync(C.base + I.faces + f0, up_faces.data() + f0, f1 - f0, hipMemcpyHostToDevice, C.st));
		C.S.bytes_to_device += (q1 - q0) + (f1 - f0);
		a = b + 1;
	}
	C.S.upload_ms += ms_since(t0);
	ENC_TRY(C.sync());
	return 0;
}

// K-ENC-EST: the estimated normals of every mesh attribute that predicts from them (corners -> sort by vertex -> sum per vertex).
// R: faces, slot.q of the position.  W: slot.q of the normals (the estimate is subtracted in place), slot.boundary, ck, cv, chist, job
// tables.  Not synchronised.
int stage_estimate(Chunk &C) {
	std::vector<EstJob> ej; std::vector<uint32_t> fstart, vstart;
	uint32_t fb = 0, vb = 0, vbase = 0, cbase = 0;
	for(uint32_t k = 0; k < C.n(); k++) {
		const BatchItem &it = C.item(k);
		const Slot &s = C.img.slot[k];
		if(it.status) continue;
		for(size_t a = 0; a < it.attrs.size(); a++) {
			if(!est_of(it, it.attrs[a])) continue;
			EstJob J{};
			J.faces = C.at<const uint32_t>(C.img.faces) + (size_t)s.fbase*3;
			J.coords = C.at<const int32_t>(s.q[it.pos]);
			J.normals = C.at<int32_t>(s.q[a]);
			J.boundary = it.attrs[a].prediction == 2 ? C.at<int32_t>(s.boundary) : nullptr;
			J.nface = it.nface; J.nvert = it.nvert_in;
			J.vbase = vbase; J.fbase = s.fbase; J.cbase = cbase; J.unit = it.attrs[a].quant.unit;
			ej.push_back(J); fstart.push_back(fb); vstart.push_back(vb);
			fb += (J.nface + 255)/256; vb += (J.nvert + 255)/256;
			vbase += J.nvert; cbase += 3*J.nface;
		}
	}
	if(ej.empty()) return 0;
	fstart.push_back(fb); vstart.push_back(vb);
	uint32_t launches = 0;
	const int e = launch_jobs(C, ej, {&fstart, &vstart}, K_EST, K_EST, [&](const EstJob *dj, const uint32_t *const *ds) {
		uint32_t *ck0 = C.at<uint32_t>(C.img.ck[0]), *ck1 = C.at<uint32_t>(C.img.ck[1]);
		uint32_t *cv0 = C.at<uint32_t>(C.img.cv[0]), *cv1 = C.at<uint32_t>(C.img.cv[1]);
		if(fb) hipLaunchKernelGGL(k_enc_corners, dim3(fb), dim3(256), 0, C.st, dj, ds[0], (uint32_t)ej.size(), ck0, cv0);
		uint32_t bits = 8;
		while(bits < 32 && (vbase >> bits)) bits += 8;
		int where = 0;
		{ const int e = radix_sort(C.st, ck0, cv0, ck1, cv1, C.at<uint32_t>(C.img.chist), cbase, bits, where, launches); if(e) return e; }
		if(vb) hipLaunchKernelGGL(k_enc_est_normal, dim3(vb), dim3(256), 0, C.st, dj, ds[1], (uint32_t)ej.size(), (const uint32_t *)(where ? ck1 : ck0),
		                          (const uint32_t *)(where ? cv1 : cv0), cbase, C.at<const uint32_t>(C.img.faces));
		return 0;
	});
	if(!e) C.bt.launches[K_EST] += launches + 2;
	return e;
}

// Clouds whose sorted keys have equal neighbours: the host's std::sort decides their order.  R: zflags, slot.q of the position.
// W: slot.quads of those clouds.  Synchronised if the chunk has a cloud (every copy here is waited for: its buffer is a local).
int resort_tied_clouds(Chunk &C) {
	std::vector<uint32_t> zflags(C.n(), 0);
	if(!C.img.clouds.empty()) {
		ENC_TRY(hipMemcpyAsync(zflags.data(), C.base + C.img.zflags, (size_t)C.n()*4, hipMemcpyDeviceToHost, C.st));
		ENC_TRY(C.sync());
		C.S.bytes_from_device += (uint64_t)C.n()*4;
	}
	for(uint32_t k : C.img.clouds) {
		BatchItem &it = C.item(k);
		if(it.nvert_in == 0 || it.status) continue;
		if(!zflags[k]) { C.S.clouds_device_sorted++; continue; }
		std::vector<int32_t> coords((size_t)it.nvert_in*3);
		ENC_TRY(hipMemcpyAsync(coords.data(), C.base + C.img.slot[k].q[it.pos], coords.size()*4, hipMemcpyDeviceToHost, C.st));
		ENC_TRY(C.sync());
		C.S.bytes_from_device += coords.size()*4;
		std::vector<uint32_t> order;
		morton_order_host(coords.data(), it.nvert_in, order);
		std::vector<uint32_t> quads((size_t)it.nvert_in*4);
		for(uint32_t i = 0; i < it.nvert_in; i++) {
			const uint32_t prev = i ? order[i - 1] : 0xffffffffu;
			quads[(size_t)i*4] = order[i]; quads[(size_t)i*4 + 1] = prev; quads[(size_t)i*4 + 2] = prev; quads[(size_t)i*4 + 3] = prev;
		}
		ENC_TRY(hipMemcpyAsync(C.base + C.img.slot[k].quads, quads.data(), quads.size()*4, hipMemcpyHostToDevice, C.st));
		ENC_TRY(C.sync());
		C.S.bytes_to_device += quads.size()*4;
		C.S.clouds_host_sorted++;
	}
	return 0;
}

// K-ENC-DELTA: every attribute's residuals in one launch.  R: slot.q, slot.quads, slot.boundary.  W: slot.d, slot.count (BORDER normals:
// how many residuals), job tables.  Not synchronised.
int stage_delta(Chunk &C) {
	std::vector<DeltaEncJob> dj; std::vector<uint32_t> start;
	uint32_t blocks = 0;
	for(uint32_t k = 0; k < C.n(); k++) {
		const BatchItem &it = C.item(k);
		const Slot &s = C.img.slot[k];
		if(it.status) continue;
		for(size_t a = 0; a < it.attrs.size(); a++) {
			const BatchAttr &A = it.attrs[a];
			DeltaEncJob J{};
			J.values = C.base + s.q[a]; J.quads = C.at<const uint32_t>(s.quads); J.out = C.base + s.d[a];
			J.count = it.nvert; J.N = A.N; J.parallel = (A.strategy & CRTHIP_PARALLEL) ? 1u : 0u;
			J.out_count = C.at<uint32_t>(s.count) + a;
			if(A.codec == CRTHIP_CODEC_COLOR) J.kind = DENC_U8;
			else if(A.codec == CRTHIP_CODEC_NORMAL) {
				J.N = 2;
				J.kind = A.prediction == 0 ? DENC_NRM_DIFF : A.prediction == 1 ? DENC_NRM_EST : DENC_NRM_BORDER;
				if(J.kind == DENC_NRM_BORDER) J.boundary = C.at<const int32_t>(s.boundary);
				if(J.kind == DENC_NRM_BORDER && !is_mesh(it)) { J.kind = DENC_NRM_EST; J.count = 0; }   // a cloud has no faces: no vertex is on a border
			} else J.kind = DENC_I32;
			if(J.kind != DENC_NRM_BORDER && J.count == 0) continue;
			dj.push_back(J); start.push_back(blocks);
			blocks += J.kind == DENC_NRM_BORDER ? 1u : (J.count + DENC_BLOCK - 1)/DENC_BLOCK;
		}
	}
	if(dj.empty()) return 0;
	start.push_back(blocks);
	const int e = launch_jobs(C, dj, {&start}, K_DELTA, K_DELTA, [&](const DeltaEncJob *d, const uint32_t *const *ds) {
		hipLaunchKernelGGL(k_enc_delta, dim3(blocks), dim3(256), 0, C.st, d, ds[0], (uint32_t)dj.size());
		return 0;
	});
	if(!e) C.bt.launches[K_DELTA]++;
	return e;
}

// BORDER counts back, then value + entropy coding: every stream of every item in one call (encode_gpu.cpp).  With the counts the stream
// is waited for, and the stages' times are read.  The host-made CLERS symbols then go up: into the image beside the device pass's (every
// mode but HOST), else into an allocation of their own, in one copy.  R: slot.count, slot.d, slot.clers.  W: slot.clers of the host-made
// meshes, coded.clers.  Synchronised (the value coder ends so).
// fetch == false (crthip_encode_batch_to_device): the coded payload stays on the device.
int code_values(Chunk &C, int mode, bool fetch, Coded &coded) {
	const uint32_t n = C.n();
	std::vector<size_t> count_at(n + 1, 0);                  // mesh k's attributes from count_at[k] on
	for(uint32_t k = 0; k < n; k++) count_at[k + 1] = count_at[k] + C.item(k).attrs.size();
	std::vector<uint32_t> counts(count_at[n] + 1, 0);
	for(uint32_t k = 0; k < n; k++) {
		const BatchItem &it = C.item(k);
		if(it.status) continue;
		for(const BatchAttr &A : it.attrs) if(border_of(it, A)) {
			ENC_TRY(hipMemcpyAsync(&counts[count_at[k]], C.base + C.img.slot[k].count, 4*it.attrs.size(), hipMemcpyDeviceToHost, C.st));
			C.S.bytes_from_device += 4*it.attrs.size();
		}
	}
	ENC_TRY(C.sync());
	for(int i = 0; i < K_STAGES; i++) C.t[i].add_to(C.bt.ms[i]);
	for(size_t c = 0; c < C.tzk.size(); c++) { C.tzk[c].add_to(C.bt.ms[K_ZKEYS]); C.tzs[c].add_to(C.bt.ms[K_ZSORT]); }

	std::vector<uint64_t> clers_at(n, 0);
	uint64_t cl = 0;
	const bool clers_in_image = mode != CRTHIP_TOPOLOGY_HOST;     // the device pass wrote its meshes' symbols there; the host's follow them
	if(clers_in_image) {
		const auto t0 = Clock::now();
		bool any = false;
		for(uint32_t k = 0; k < n; k++) {
			const BatchItem &it = C.item(k);
			if(it.topo_device || it.clers.empty() || !it.topo_image) continue;
			ENC_TRY(hipMemcpyAsync(C.base + C.img.slot[k].clers, it.clers.data(), it.clers.size(), hipMemcpyHostToDevice, C.st));
			C.S.bytes_to_device += it.clers.size();
			any = true;
		}
		C.S.upload_ms += ms_since(t0);
		if(any) ENC_TRY(C.sync());
	} else cl = clers_layout(C.items, C.img, clers_at);
	DevMem &dclers = coded.clers;                                 // under entropy NONE the symbols are a source of the device splice
	if(cl) {
		const auto t0 = Clock::now();
		std::vector<uint8_t> h(cl);
		for(uint32_t k = 0; k < n; k++) if(!C.item(k).clers.empty()) memcpy(h.data() + clers_at[k], C.item(k).clers.data(), C.item(k).clers.size());
		C.S.host_stage_ms += ms_since(t0);
		ENC_TRY(hipMalloc(&dclers.p, cl + 16));                   // (a source of the device splice: enc_splice.h, SOURCES)
		ENC_TRY(hipMemcpyAsync(dclers.p, h.data(), cl, hipMemcpyHostToDevice, C.st));
		ENC_TRY(C.sync());
		C.S.bytes_to_device += cl;
	}
	std::vector<DevValueStream> vs;
	for(uint32_t k = 0; k < n; k++) {
		BatchItem &it = C.item(k);
		if(it.status) continue;
		for(BatchStream &b : it.streams) {
			if(b.kind == BATCH_BITS) continue;
			DevValueStream v;
			v.kind = b.kind; v.entropy = it.entropy; v.components = b.N;
			if(b.attr == -1) { v.count = it.nclers; v.values = clers_in_image ? C.base + C.img.slot[k].clers : dclers.u8() + clers_at[k]; }
			else {
				if(border_of(it, it.attrs[b.attr])) b.count = counts[count_at[k] + b.attr];
				v.count = b.count;
				v.values = C.base + C.img.slot[k].d[b.attr];
			}
			vs.push_back(v);
		}
	}
	const auto t0 = Clock::now();
	const int e = encode_value_streams_device(C.ctx, vs, fetch, coded, C.tm);
	C.S.value_coder_ms += ms_since(t0);
	if(e) return e;
	C.S.value_streams += (uint32_t)vs.size();
	return 0;
}

// crthip_encode_batch_to_device: where the blobs go and what the call has to say about them
struct DeviceOut {
	uint8_t *arena = nullptr;                                // the caller's device_out, checked; null: the call only sizes
	uint64_t cap = 0;
	uint64_t at = 0;                                         // the arena's running offset: chunks continue it
	std::vector<uint32_t> len;                               // per item of the batch (0: failed)
	crthip_splice_stats st{};
	float kernel_ms = 0;
};

// The tail of a device-output chunk: the plan of every container (enc_splice.h) from the frames and from where `coded` says the payload
// lies, one upload of job table + literal buffer, one launch of k_enc_splice.  Nothing is launched when the call only sizes or the arena
// would not hold the chunk.  R: the value coder's images, slot.clers (entropy NONE).  W: the caller's arena.  Synchronised.
int splice_to_device(Chunk &C, const Coded &coded, DeviceOut &D) {
	const auto t_plan = Clock::now();
	SplicePlan P(D.at);
	size_t r = 0;
	for(uint32_t k = 0; k < C.n(); k++) {
		const BatchItem &it = C.item(k);
		if(it.status) continue;
		const uint64_t len = P.item(it.frame, it.streams, coded.streams.data() + r, it.split_words, r);
		if(len > 0xFFFFFFFFull) return ctx_fail(CRTHIP_E_LIMIT, "crthip_encode_batch_to_device: a blob of 4 GiB or more");
		D.len[C.img.ids[k]] = (uint32_t)len;
	}
	D.at = P.at;
	std::vector<SpliceJob> jobs;
	std::vector<uint32_t> tile_start;
	const bool write = D.arena && P.at <= D.cap && !P.pieces.empty();
	// one host image, packed: jobs | tile_start | literal - what goes up is the job table and the literal bytes, nothing else (the jobs are
	// multiples of 8 bytes, the tile starts of 4; the literal buffer follows the tables, so its first piece's aligned reads stay inside)
	const uint64_t o_tiles = P.pieces.size()*sizeof(SpliceJob), o_lit = o_tiles + (P.pieces.size() + 1)*4;
	const uint64_t up_bytes = o_lit + P.literal.size();
	DevMem dev;
	std::vector<uint8_t> h;
	// `h` and `dev` are read by the queued copy and the launch: every way out below waits for the stream before they go
	struct Wait { hipStream_t st; ~Wait() { (void)hipStreamSynchronize(st); } } wait{C.st};
	uint64_t tiles = 0;
	if(write) {
		ENC_TRY(hipMalloc(&dev.p, up_bytes + 16));
		tiles = splice_jobs(P, dev.u8() + o_lit, D.arena, jobs, tile_start);
		if(tiles >= (1ull << 32) - 4) return ctx_fail(CRTHIP_E_LIMIT, "crthip_encode_batch_to_device: too many tiles");
		h.resize(up_bytes);
		memcpy(h.data(), jobs.data(), jobs.size()*sizeof(SpliceJob));
		memcpy(h.data() + o_tiles, tile_start.data(), tile_start.size()*4);
		if(!P.literal.empty()) memcpy(h.data() + o_lit, P.literal.data(), P.literal.size());
	} else tiles = splice_jobs(P, nullptr, nullptr, jobs, tile_start);       // (the statistics of a sizing call: the arena's alignment is the one promised)
	C.S.host_frame_ms += (float)ms_since(t_plan);
	D.st.pieces += (uint32_t)P.pieces.size(); D.st.jobs += (uint32_t)tiles;
	D.st.literal_bytes += P.literal_bytes; D.st.device_bytes += P.device_bytes;
	if(!write) return 0;
	EventTimer t;
	ENC_TRY(hipMemcpyAsync(dev.p, h.data(), up_bytes, hipMemcpyHostToDevice, C.st));
	C.S.bytes_to_device += up_bytes;
	if(t.begin(C.st)) return CRTHIP_E_DEVICE;
	hipLaunchKernelGGL(k_enc_splice, dim3((uint32_t)((tiles + ESP_THREADS/ESP_LANES - 1)/(ESP_THREADS/ESP_LANES))), dim3(ESP_THREADS), 0, C.st,
	                   (const SpliceJob *)dev.p, (const uint32_t *)(dev.u8() + o_tiles), (uint32_t)jobs.size());
	if(t.end(C.st)) return CRTHIP_E_DEVICE;
	ENC_TRY(hipGetLastError());
	ENC_TRY(C.sync());
	t.add_to(D.kernel_ms);
	D.st.launches++;
	return 0;
}

// the device half of one chunk: the items of img.ids have been set up; their topology passes run here, on the pool (overlapping the
// device) or on the device
int encode_chunk(crthip_ctx *ctx, const crthip_mesh *meshes, const crthip_attr_list *extra, std::vector<BatchItem> &items, const ChunkImage &img, uint64_t budget,
                 uint32_t threads, std::vector<std::vector<uint8_t>> &blobs, crthip_encode_batch_stats &S, BatchTimes &bt, EncStageTimes &tm,
                 DeviceOut *dout = nullptr) {
	const int mode = ctx_encode_topology(ctx);
	// the chunker sized this chunk by this very image, so only a single item can still be beyond the budget: nothing is allocated for it
	if(img.total > budget) return ctx_fail(CRTHIP_E_LIMIT, "crthip_encode_batch: a mesh too big for the device image");
	// Lifetimes, by declaration order (destruction runs upwards).  The pool thread's lambdas hold references to C (ready / mu / cv /
	// topo_ms are its members) and through it to items and img: all declared before the thread, whose Joiner joins it on every way out.
	// The image's memory is freed by DevMem only after Drain has waited for the work queued on it, and C's host buffers go after that.
	// `coded` comes first: its device images are read by the splice's launch and its host buffers written by the value coder's queued
	// copies, so it goes last, after the Drain.
	Coded coded;
	Chunk C{ctx, ctx_stream(ctx), meshes, extra, items, img, S, bt, tm};
	for(uint32_t k : img.devk) C.ready[k] = 1;
	bool widen = img.resident;
	for(uint32_t k : img.hostk) widen = widen || C.item(k).index16;
	if(widen) { const int e = fetch_indices(C); if(e) return e; }
	// topology passes (meshes) and frames (everything) on the pool, started first: they need the index alone
	std::thread pool;
	struct Joiner { std::thread &t; ~Joiner() { if(t.joinable()) t.join(); } } joiner{pool};
	if(mode != CRTHIP_TOPOLOGY_DEVICE) pool = std::thread([&]() {      // (device mode starts no thread: the clouds' frames are made inline, collect_passes)
		parallel_for((uint32_t)img.hostk.size(), threads, [&](uint32_t j) { C.host_pass(img.hostk[j]); });
		std::lock_guard<std::mutex> g(C.mu);
		C.topo_ms = ms_since(C.t_topo);
	});
	DevMem dev;
	{ const auto t0 = Clock::now(); ENC_TRY(hipMalloc(&dev.p, img.total + 256)); S.alloc_ms += ms_since(t0); }
	C.base = dev.u8();
	struct Drain { hipStream_t st; ~Drain() { (void)hipStreamSynchronize(st); } } drain{C.st};   // every way out waits for the work queued on the image first

	int e = upload_inputs(C);
	if(!e) e = stage_quantise(C);
	if(!e) e = stage_topology(C);
	if(!e) e = stage_cloud_sort(C);
	if(!e) e = collect_passes(C, mode);
	if(e) return e;
	if(pool.joinable()) pool.join();
	S.host_topology_ms += (float)C.topo_ms;
	for(uint32_t id : img.ids)                                         // Tunstall streams over 2^23 symbols: the reference's count*255 overflow
		if(items[id].entropy == CRTHIP_ENTROPY_TUNSTALL && (items[id].nclers > (1u << 23) || items[id].nvert > (1u << 23)))
			items[id].status = ctx_fail(CRTHIP_E_LIMIT, "crthip_encode_batch: a Tunstall stream longer than 2^23 symbols");
	e = stage_estimate(C);
	if(!e) e = resort_tied_clouds(C);
	if(!e) e = stage_delta(C);
	if(!e) e = code_values(C, mode, !dout, coded);
	if(e) return e;
	if(coded.on_device) return splice_to_device(C, coded, *dout);

	// every container from its frame and its coded streams, in item order
	const auto t_frame = Clock::now();
	size_t r = 0;
	for(uint32_t id : img.ids) {
		if(items[id].status) continue;
		blobs[id].clear();
		ByteOut o{blobs[id]};
		r += write_container(o, items[id].frame, items[id].streams, coded.streams.data() + r, items[id].split_words);
	}
	S.host_frame_ms += (float)ms_since(t_frame);
	return CRTHIP_OK;
}

// ---- a resident call's front: the caller's pointers, then what the host would have read through them ----

// every data array of one mesh (after encode_check / encode_check_attrs / layout_resolve): no launch reads a pointer that has not passed
// here.  An array's extent is what the kernels touch of it: [ptr, ptr + (nvert - 1)*stride + one vertex's bytes).
int resident_check(const crthip_mesh *m, const crthip_attr_list *extra, const MeshRead &rd, int device) {
	const uint64_t nv = m->nvert;
	auto extent = [&](uint32_t stride, uint64_t vertex_bytes) { return nv ? (nv - 1)*stride + vertex_bytes : 0; };
	bool ok = resident_array_ok(m->position, extent(rd.position, 12), 4, device);
	if(m->index && m->nface) ok = ok && resident_array_ok(m->index, (uint64_t)m->nface*(rd.index16 ? 6 : 12), rd.index16 ? 2 : 4, device);
	if(m->normal) ok = ok && resident_array_ok(m->normal, extent(rd.normal, rd.normal16 ? 6 : 12), rd.normal16 ? 2 : 4, device);
	if(m->color) ok = ok && resident_array_ok(m->color, extent(rd.color, (uint64_t)m->color_components), 1, device);
	if(m->uv) ok = ok && resident_array_ok(m->uv, extent(rd.uv, 8), 4, device);
	if(m->radius) ok = ok && resident_array_ok(m->radius, extent(rd.radius, 4), 4, device);
	if(extra) for(uint32_t k = 0; k < extra->nattr && ok; k++) {
		const crthip_generic_attr &g = extra->attr[k];
		const uint32_t esize = generic_esize(g.format);
		ok = resident_array_ok(g.values, extent(rd.attr[k], (uint64_t)g.components*esize), esize, device);
	}
	return ok ? CRTHIP_OK : ctx_fail(CRTHIP_E_ARGUMENT, "crthip_encode_batch_resident: a data array is not element-aligned device memory of the context's device, "
	                                                    "or leaves its allocation");
}

// K-ENC-CHECK (k_encode_check.hip): the index range, the bounding boxes and the first-edge sums of meshes[ok[..]], whichever its step's
// recipe needs, in two launches; recs[k] is item ok[k]'s record.  The pass has a small allocation of its own - records, partial boxes,
// job tables - because a chunk's image is laid out from what batch_setup leaves, and batch_setup needs the step.  One copy back, one wait.
int input_pass(crthip_ctx *ctx, const crthip_mesh *meshes, const std::vector<MeshRead> &reads, const std::vector<uint32_t> &ok, std::vector<EncInputRecord> &recs,
               crthip_encode_batch_stats &S, BatchTimes &bt) {
	const uint32_t n = (uint32_t)ok.size();
	recs.assign(n, EncInputRecord{});
	std::vector<EncInputJob> jobs;
	std::vector<uint32_t> tables, box_ids;                        // tables: block_start, then box_ids
	std::vector<uint64_t> rec_of, part_of;                        // per job: its item's place in ok, its first partial
	uint64_t blocks = 0, nparts = 0;
	for(uint32_t k = 0; k < n; k++) {
		const crthip_mesh &m = meshes[ok[k]];
		const uint32_t nface = m.index ? m.nface : 0;
		EncInputJob J = enc_input_job(&m, &reads[ok[k]]);
		auto add = [&](uint32_t kind, uint64_t nblocks) {
			J.kind = kind;
			jobs.push_back(J); rec_of.push_back(k); part_of.push_back(nparts); tables.push_back((uint32_t)blocks);
			blocks += nblocks;
		};
		if(nface) add(EIN_JOB_RANGE, (uint64_t)nface*3/EIN_INDEX_TILE + 1);
		if((J.recipe == EIN_STEP_BOX_FIRST || J.recipe == EIN_STEP_BOX_MAX) && m.nvert) {
			const uint64_t tiles = ((uint64_t)m.nvert + EIN_TILE - 1)/EIN_TILE;
			box_ids.push_back((uint32_t)jobs.size());
			add(EIN_JOB_BOX, tiles);
			nparts += tiles;
		}
		if(J.recipe == EIN_STEP_EDGE) add(EIN_JOB_EDGE, 1);
	}
	if(jobs.empty()) return 0;
	if(blocks >= (1ull << 31)) return ctx_fail(CRTHIP_E_LIMIT, "crthip_encode_batch_resident: too many workgroups for the input pass");
	tables.push_back((uint32_t)blocks);
	const size_t ids_at = tables.size();
	tables.insert(tables.end(), box_ids.begin(), box_ids.end());

	Carver c;
	const uint64_t rec_off = c.take((uint64_t)n*sizeof(EncInputRecord)), part_off = c.take(nparts*sizeof(EncInputBox));
	const uint64_t job_off = c.take(jobs.size()*sizeof(EncInputJob)), tab_off = c.take(tables.size()*4);
	DevMem dev;
	{ const auto t0 = Clock::now(); ENC_TRY(hipMalloc(&dev.p, c.take(0) + 256)); S.alloc_ms += ms_since(t0); }
	const hipStream_t st = ctx_stream(ctx);
	struct Drain { hipStream_t st; ~Drain() { (void)hipStreamSynchronize(st); } } drain{st};
	for(size_t j = 0; j < jobs.size(); j++) {
		jobs[j].rec = (EncInputRecord *)(dev.u8() + rec_off) + rec_of[j];
		jobs[j].partials = (EncInputBox *)(dev.u8() + part_off) + part_of[j];
	}
	const EncInputJob *dj = (const EncInputJob *)(dev.u8() + job_off);
	const uint32_t *dt = (const uint32_t *)(dev.u8() + tab_off);
	ENC_TRY(hipMemsetAsync(dev.u8() + rec_off, 0, (size_t)n*sizeof(EncInputRecord), st));
	ENC_TRY(hipMemcpyAsync(dev.u8() + job_off, jobs.data(), jobs.size()*sizeof(EncInputJob), hipMemcpyHostToDevice, st));
	ENC_TRY(hipMemcpyAsync(dev.u8() + tab_off, tables.data(), tables.size()*4, hipMemcpyHostToDevice, st));
	S.bytes_to_device += jobs.size()*sizeof(EncInputJob) + tables.size()*4;
	EventTimer t_check, t_reduce;
	if(t_check.begin(st)) return CRTHIP_E_DEVICE;
	hipLaunchKernelGGL(k_enc_input_check, dim3((uint32_t)blocks), dim3(EIN_THREADS), 0, st, dj, dt, (uint32_t)jobs.size());
	if(t_check.end(st)) return CRTHIP_E_DEVICE;
	bt.launches[K_IN_CHECK]++;
	if(!box_ids.empty()) {
		if(t_reduce.begin(st)) return CRTHIP_E_DEVICE;
		hipLaunchKernelGGL(k_enc_input_reduce, dim3((uint32_t)box_ids.size()), dim3(EIN_FOLD_LANES), 0, st, dj, dt + ids_at, (uint32_t)box_ids.size());
		if(t_reduce.end(st)) return CRTHIP_E_DEVICE;
		bt.launches[K_IN_REDUCE]++;
	}
	ENC_TRY(hipGetLastError());
	ENC_TRY(hipMemcpyAsync(recs.data(), dev.u8() + rec_off, (size_t)n*sizeof(EncInputRecord), hipMemcpyDeviceToHost, st));
	{ const auto t0 = Clock::now(); ENC_TRY(hipStreamSynchronize(st)); S.sync_wait_ms += ms_since(t0); }
	S.bytes_from_device += (uint64_t)n*sizeof(EncInputRecord);
	t_check.add_to(bt.ms[K_IN_CHECK]); t_reduce.add_to(bt.ms[K_IN_REDUCE]);
	return 0;
}

} // namespace

// one array of a resident call: element-aligned device memory of the context's device, its whole extent inside one allocation
// (pool_internal.h: crthip_pool_decode checks its device destinations with it too)
bool corto_hip::resident_array_ok(const void *p, uint64_t bytes, uint32_t align, int device) {
	if(!bytes) return true;
	if(!p || ((uintptr_t)p & (align - 1))) return false;
	hipPointerAttribute_t a;
	memset(&a, 0, sizeof(a));
	if(hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }   // (memory the runtime has never seen)
	if(a.type != hipMemoryTypeDevice || a.device != device) return false;                          // pinned and managed memory included
	hipDeviceptr_t base = nullptr;
	size_t size = 0;
	if(hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess) { (void)hipGetLastError(); return false; }
	const uintptr_t b = (uintptr_t)base, q = (uintptr_t)p;
	return q >= b && bytes <= size && q - b <= size - bytes;
}

// what encode_batch_impl refuses a mesh for before any device work; rd: the mesh's layout, resolved here; resident_device >= 0: its data
// arrays are that device's memory
static int batch_item_check(const crthip_mesh *m, const crthip_attr_list *extra, const crthip_mesh_layout *layout, MeshRead &rd, bool index_on_host,
                            int resident_device = -1) {
	const bool index16 = layout && (layout->flags & CRTHIP_IN_INDEX_UINT16);   // (encode_check scans uint32 entries: a uint16 index is scanned behind the layout's own checks)
	int e = encode_check(m, index_on_host && !index16);
	if(!e) e = encode_check_attrs(m, extra, true);
	if(!e) e = layout_resolve(m, extra, layout, rd);
	if(!e && index_on_host && index16) e = index_range_host(m, rd);
	if(!e && resident_device >= 0) e = resident_check(m, extra, rd, resident_device);
	if(!e && (uint64_t)m->nvert*3 > (1u << 26)) e = ctx_fail(CRTHIP_E_LIMIT, "crthip_encode_batch: too many vertices for the value coder");
	if(!e && m->entropy == CRTHIP_ENTROPY_TUNSTALL && m->nvert > (1u << 23))
		e = ctx_fail(CRTHIP_E_LIMIT, "crthip_encode_batch: a Tunstall stream longer than 2^23 symbols");
	return e;
}

// crthip_encode_batch_layout with host output: where the blobs go in the caller's host arena
struct HostArena { uint8_t *out = nullptr; size_t cap = 0; std::vector<uint32_t> len; };

// resident: the data arrays of meshes / extra are DEVICE pointers (crthip_encode_batch_resident); dout: the blobs stay on the device
// (crthip_encode_batch_to_device: out / cap / blob_offset are then unused); layouts: n crthip_mesh_layout or null; harena: the blobs go
// into a host arena laid out as the device one (crthip_encode_batch_layout; out / cap unused); everything else is the one path
static int64_t encode_batch_impl(crthip_ctx *ctx, uint32_t n, const crthip_mesh *meshes, const crthip_attr_list *extra, uint32_t host_threads,
                                 uint8_t *out, size_t cap, uint64_t *blob_offset, uint32_t *out_nvert, uint32_t *out_nface,
                                 int32_t *status, crthip_encode_batch_stats *stats, crthip_kernel_times *times, bool resident, DeviceOut *dout = nullptr,
                                 const crthip_mesh_layout *layouts = nullptr, HostArena *harena = nullptr) {
	const auto t0 = Clock::now();
	if(!ctx) return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_encode_batch: null context (there is no CPU fallback: use crthip_encode for the host encoder)");
	if(!blob_offset || (n && !meshes)) return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_encode_batch: null argument");
	crthip_encode_batch_stats S;
	memset(&S, 0, sizeof(S));
	if(times) memset(times, 0, sizeof(*times));
	blob_offset[0] = 0;
	if(n == 0) { if(stats) *stats = S; return 0; }
	const uint32_t threads = host_threads ? host_threads : default_threads();
	ENC_TRY(hipSetDevice(ctx_device(ctx)));
	{ const int e = ctx_quiesce(ctx); if(e) return e; }

	// per-mesh argument checks; what fails gets its code and an empty range
	std::vector<BatchItem> items(n);
	std::vector<MeshRead> reads(n);
	std::vector<uint32_t> ok;
	for(uint32_t i = 0; i < n; i++) {
		items[i].status = batch_item_check(&meshes[i], extra ? &extra[i] : nullptr, layouts ? &layouts[i] : nullptr, reads[i], !resident, resident ? ctx_device(ctx) : -1);
		if(!items[i].status) ok.push_back(i);
	}
	// position steps and attribute tables (the steps' sums are the host's, in its order: a resident call gets them, and the index check
	// encode_check left out, from the device's records)
	BatchTimes bt;
	std::vector<float> steps;
	if(resident) {
		std::vector<EncInputRecord> recs;
		{ const int e = input_pass(ctx, meshes, reads, ok, recs, S, bt); if(e) return e; }
		steps.resize(ok.size());
		for(size_t k = 0; k < ok.size(); k++) {
			const crthip_mesh &m = meshes[ok[k]];
			if(recs[k].bad_index) items[ok[k]].status = ctx_fail(CRTHIP_E_ARGUMENT, "crthip_encode: face index out of range");
			else steps[k] = position_step(&m, enc_in_recipe(m.position_bits, m.position_q, m.nvert, m.index ? m.nface : 0), recs[k]);
		}
	}
	parallel_for((uint32_t)ok.size(), threads, [&](uint32_t k) {
		if(items[ok[k]].status) return;
		items[ok[k]].status = item_guard([&] { batch_setup(&meshes[ok[k]], extra ? &extra[ok[k]] : nullptr, items[ok[k]], resident ? &steps[k] : nullptr, &reads[ok[k]]); });
	});
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
	ENC_TRY(hipMemGetInfo(&free_b, &total_b));
	uint64_t budget = free_b/2;
	if(const uint64_t b = ctx_encode_image_budget(ctx)) budget = std::min(budget, b);   // (test hook: several chunks from a small batch)
	std::vector<std::vector<uint8_t>> blobs(n);
	EncStageTimes tm;
	// Device output in several chunks: a chunk is spliced before the next one is coded, so the total is not known when the first one is
	// written.  Where the arena is not known to hold any outcome (cap below crthip_encode_batch_bound) the call sizes first - the batch
	// is encoded twice - and writes only if the total fits: nothing is written to an arena that proves too small.
	if(dout && dout->arena && ok.size() > 1 && build_image(meshes, items, ok, resident).total > budget && dout->cap < crthip_encode_batch_bound(n, meshes, extra)) {
		DeviceOut sizing;
		sizing.cap = dout->cap; sizing.len.assign(n, 0);
		const int64_t total = encode_batch_impl(ctx, n, meshes, extra, host_threads, nullptr, 0, blob_offset, out_nvert, out_nface, status, stats, times, resident, &sizing, layouts);
		if(total < 0 || (uint64_t)total > dout->cap) { dout->len = sizing.len; dout->at = sizing.at; dout->st = sizing.st; return total; }
	}
	for(size_t k = 0; k < ok.size();) {
		// a chunk is sized by building its image: of every item that is left (the usual case), else of half as many until the image fits
		// (an image only grows with another item).  A single item beyond the budget fails where encode_chunk allocates.
		size_t take = ok.size() - k;
		ChunkImage img = build_image(meshes, items, std::vector<uint32_t>(ok.begin() + k, ok.end()), resident);
		while(img.total > budget && take > 1) { take = (take + 1)/2; img = build_image(meshes, items, std::vector<uint32_t>(ok.begin() + k, ok.begin() + k + take), resident); }
		const int e = encode_chunk(ctx, meshes, extra, items, img, budget, threads, blobs, S, bt, tm, dout);
		if(e) return e;
		k += take;
	}

	uint64_t w = 0;
	for(uint32_t i = 0; i < n; i++) {
		blob_offset[i] = w;
		if(status) status[i] = items[i].status;
		if(out_nvert) out_nvert[i] = items[i].status ? 0 : items[i].nvert;
		if(out_nface) out_nface[i] = items[i].status ? 0 : items[i].nface;
		if(items[i].status) { if(dout) dout->len[i] = 0; continue; }
		if(out && w + blobs[i].size() <= cap) memcpy(out + w, blobs[i].data(), blobs[i].size());
		w += blobs[i].size();
	}
	blob_offset[n] = w;
	if(dout) w = dout->at;
	if(harena) {                                                       // the device arena's form in host memory: crthip_arena_layout, zeros to each next 16
		harena->len.assign(n, 0);
		for(uint32_t i = 0; i < n; i++) if(!items[i].status) harena->len[i] = (uint32_t)blobs[i].size();
		std::vector<uint64_t> at(n);
		w = crthip_arena_layout(n, harena->len.data(), at.data());
		if(harena->out && w <= harena->cap)
			for(uint32_t i = 0; i < n; i++) {
				const uint64_t len = harena->len[i];
				if(len) memcpy(harena->out + at[i], blobs[i].data(), len);
				memset(harena->out + at[i] + len, 0, ((len + 15) & ~15ull) - len);
			}
	}
	S.bytes_to_device += tm.bytes_to_device; S.bytes_from_device += tm.bytes_from_device;
	S.wall_ms = (float)ms_since(t0);
	if(stats) *stats = S;
	if(times) {
		uint32_t c = 0;
		for(int i = 0; i < K_COUNT; i++) if(bt.launches[i]) { times->name[c] = KERNEL_NAME[i]; times->ms[c] = bt.ms[i]; times->launches[c] = bt.launches[i]; c++; }
		times->count = c;
		enc_report_times(times, tm);
		if(dout && dout->st.launches && times->count < CRTHIP_MAX_KERNELS) {
			const uint32_t k = times->count++;
			times->name[k] = "enc_splice"; times->ms[k] = dout->kernel_ms; times->launches[k] = dout->st.launches;
		}
	}
	return (int64_t)w;
}

// nothing is thrown across the C boundary
extern "C" int64_t crthip_encode_batch_attrs(crthip_ctx *ctx, uint32_t n, const crthip_mesh *meshes, const crthip_attr_list *extra, uint32_t host_threads,
                                             uint8_t *out, size_t cap, uint64_t *blob_offset, uint32_t *out_nvert, uint32_t *out_nface,
                                             int32_t *status, crthip_encode_batch_stats *stats, crthip_kernel_times *times) {
	try {
		return encode_batch_impl(ctx, n, meshes, extra, host_threads, out, cap, blob_offset, out_nvert, out_nface, status, stats, times, false);
	} catch(const std::bad_alloc &) {
		return ctx_fail(CRTHIP_E_NOMEM, nullptr);
	} catch(...) {
		return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_encode_batch: internal error");
	}
}

extern "C" int64_t crthip_encode_batch_resident(crthip_ctx *ctx, uint32_t n, const crthip_mesh *meshes, const crthip_attr_list *extra, uint32_t host_threads,
                                                uint8_t *out, size_t cap, uint64_t *blob_offset, uint32_t *out_nvert, uint32_t *out_nface,
                                                int32_t *status, crthip_encode_batch_stats *stats, crthip_kernel_times *times) {
	try {
		return encode_batch_impl(ctx, n, meshes, extra, host_threads, out, cap, blob_offset, out_nvert, out_nface, status, stats, times, true);
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

// ---- crthip_encode_batch_to_device ----

extern "C" int64_t crthip_encode_batch_to_device(crthip_ctx *ctx, uint32_t n, const crthip_mesh *meshes, const crthip_attr_list *extra, uint32_t host_threads,
                                                 uint32_t flags, void *device_out, size_t cap, uint64_t *blob_offset, uint32_t *blob_len,
                                                 uint32_t *out_nvert, uint32_t *out_nface, int32_t *status, crthip_encode_batch_stats *stats,
                                                 crthip_kernel_times *times) {
	try {
		if(flags & ~CRTHIP_ENCODE_INPUTS_RESIDENT) return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_encode_batch_to_device: unknown flag bits");
		if(n == 0) {                                                    // nothing is read or written, the context included
			if(stats) memset(stats, 0, sizeof(*stats));
			if(times) memset(times, 0, sizeof(*times));
			if(ctx) ctx_splice_stats(ctx) = crthip_splice_stats{};
			return 0;
		}
		if(!ctx) return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_encode_batch_to_device: null context (there is no CPU fallback)");
		if(!blob_offset || !blob_len || !meshes) return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_encode_batch_to_device: null argument");
		ctx_splice_stats(ctx) = crthip_splice_stats{};
		ENC_TRY(hipSetDevice(ctx_device(ctx)));
		if(device_out && !resident_array_ok(device_out, cap ? cap : 1, 16, ctx_device(ctx)))
			return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_encode_batch_to_device: device_out is not 16-byte aligned device memory of the context's device, "
			                                   "or [device_out, device_out + cap) leaves its allocation");
		DeviceOut D;
		D.arena = (uint8_t *)device_out; D.cap = cap; D.len.assign(n, 0);
		std::vector<uint64_t> unused(n + 1, 0);
		const int64_t total = encode_batch_impl(ctx, n, meshes, extra, host_threads, nullptr, 0, unused.data(), out_nvert, out_nface, status, stats, times,
		                                        (flags & CRTHIP_ENCODE_INPUTS_RESIDENT) != 0, &D);
		if(total < 0) return total;
		memcpy(blob_len, D.len.data(), (size_t)n*4);
		const uint64_t laid = crthip_arena_layout(n, blob_len, blob_offset);
		if(laid != (uint64_t)total) return ctx_fail(CRTHIP_E_DEVICE, "crthip_encode_batch_to_device: the plan and crthip_arena_layout disagree");
		D.st.arena_bytes = (uint64_t)total; D.st.splice_kernel_us = D.kernel_ms*1000.0f;
		ctx_splice_stats(ctx) = D.st;
		return total;
	} catch(const std::bad_alloc &) {
		return ctx_fail(CRTHIP_E_NOMEM, nullptr);
	} catch(...) {
		return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_encode_batch_to_device: internal error");
	}
}

// ---- crthip_encode_batch_layout ----

extern "C" int64_t crthip_encode_batch_layout(crthip_ctx *ctx, uint32_t n, const crthip_mesh *meshes, const crthip_attr_list *extra, const crthip_mesh_layout *layouts,
                                              uint32_t host_threads, uint32_t flags, void *out, size_t cap, uint64_t *blob_offset, uint32_t *blob_len,
                                              uint32_t *out_nvert, uint32_t *out_nface, int32_t *status, crthip_encode_batch_stats *stats,
                                              crthip_kernel_times *times) {
	try {
		if(flags & ~(CRTHIP_ENCODE_INPUTS_RESIDENT | CRTHIP_ENCODE_OUTPUT_DEVICE)) return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_encode_batch_layout: unknown flag bits");
		const bool resident = (flags & CRTHIP_ENCODE_INPUTS_RESIDENT) != 0, device_out = (flags & CRTHIP_ENCODE_OUTPUT_DEVICE) != 0;
		if(n == 0) {                                                    // nothing is read or written, the context included
			if(stats) memset(stats, 0, sizeof(*stats));
			if(times) memset(times, 0, sizeof(*times));
			if(ctx && device_out) ctx_splice_stats(ctx) = crthip_splice_stats{};
			return 0;
		}
		if(!ctx) return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_encode_batch_layout: null context (there is no CPU fallback: crthip_encode_layout is the host encoder)");
		if(!blob_offset || !blob_len || !meshes) return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_encode_batch_layout: null argument");
		std::vector<uint64_t> unused(n + 1, 0);
		DeviceOut D;
		HostArena H;
		if(device_out) {
			ctx_splice_stats(ctx) = crthip_splice_stats{};
			ENC_TRY(hipSetDevice(ctx_device(ctx)));
			if(out && !resident_array_ok(out, cap ? cap : 1, 16, ctx_device(ctx)))
				return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_encode_batch_layout: out is not 16-byte aligned device memory of the context's device, "
				                                   "or [out, out + cap) leaves its allocation");
			D.arena = (uint8_t *)out; D.cap = cap; D.len.assign(n, 0);
		} else { H.out = (uint8_t *)out; H.cap = cap; }
		const int64_t total = encode_batch_impl(ctx, n, meshes, extra, host_threads, nullptr, 0, unused.data(), out_nvert, out_nface, status, stats, times,
		                                        resident, device_out ? &D : nullptr, layouts, device_out ? nullptr : &H);
		if(total < 0) return total;
		memcpy(blob_len, device_out ? D.len.data() : H.len.data(), (size_t)n*4);
		const uint64_t laid = crthip_arena_layout(n, blob_len, blob_offset);
		if(laid != (uint64_t)total) return ctx_fail(CRTHIP_E_DEVICE, "crthip_encode_batch_layout: the plan and crthip_arena_layout disagree");
		if(device_out) {
			D.st.arena_bytes = (uint64_t)total; D.st.splice_kernel_us = D.kernel_ms*1000.0f;
			ctx_splice_stats(ctx) = D.st;
		}
		return total;
	} catch(const std::bad_alloc &) {
		return ctx_fail(CRTHIP_E_NOMEM, nullptr);
	} catch(...) {
		return ctx_fail(CRTHIP_E_ARGUMENT, "crthip_encode_batch_layout: internal error");
	}
}

// one item's share of crthip_encode_batch_bound: its frame as batch_frame / batch_topology make it from the descriptor (every field of it has
// a fixed width), and per slot the bounds the coders themselves check
static uint64_t item_bound(const crthip_mesh *m, const crthip_attr_list *extra) {
	MeshRead rd;
	if(batch_item_check(m, extra, nullptr, rd, false)) return 0;
	BatchItem it;
	const float step = 1.0f;                                           // (its four bytes are in the frame whatever it is; no array is read)
	batch_setup(m, extra, it, &step);
	if(is_mesh(it)) {
		EncTopoRecord R;
		memset(&R, 0, sizeof(R));
		R.nvert = m->nvert; R.nface = m->nface;
		std::vector<uint32_t> gend(std::max(m->ngroups, 1u), m->nface);
		batch_frame(m, extra, it, R, m->ngroups ? m->group_end : gend.data(), gend.data());
	} else batch_topology(m, extra, it);
	const bool tun = it.entropy == CRTHIP_ENTROPY_TUNSTALL;
	auto block = [&](uint64_t size) { return tun ? 9 + 2*256 + size + 1 : 4 + size; };
	auto bits = [&](uint64_t words) { return 4 + 3 + 4*words; };
	uint64_t b = it.frame.size() + 15;
	for(const BatchStream &s : it.streams) {
		if(s.kind == BATCH_BITS) b += bits(CRTHIP_TOPOLOGY_SPLIT_CAP(m->nface));
		else if(s.attr == -1) b += block(CRTHIP_TOPOLOGY_CLERS_CAP(m->nface));
		else if(s.kind == CRTHIP_ENC_SYMBOLS) b += block(m->nvert);
		else b += bits((uint64_t)m->nvert*s.N + 1) + (s.kind == CRTHIP_ENC_ARRAY ? 1u : s.N)*block(m->nvert);
	}
	return (b + 15) & ~15ull;
}

extern "C" uint64_t crthip_encode_batch_bound(uint32_t n, const crthip_mesh *meshes, const crthip_attr_list *extra) {
	if(!meshes) return 0;
	uint64_t total = 0;
	for(uint32_t i = 0; i < n; i++) {
		try { total += item_bound(&meshes[i], extra ? &extra[i] : nullptr); } catch(...) {}
	}
	return total;
}
