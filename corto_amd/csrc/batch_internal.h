// batch_internal.h — what the pieces of the decode path's host side share: the context and batch objects, the plan of one decode call and
// the
// staged Planner (batch.cpp: the C ABI, context, harvest; batch_bind.cpp: the bind calls and what reads a decode's records - no HIP call, so a
// program without the runtime links them; plan_carve.cpp / plan_jobs.cpp / plan_group.cpp: the planner's stages up to and with upload(), which
// calls no kernel and no stream either; plan_launch.cpp: the schedule's shape (Planner::shape), launch() and its stage members - entropy, front,
// delta, cloud, normals, derived, finish -, tun_chain, the stats).  Round 5 split batch.cpp (1 640 lines) along the Planner's stages.  A blob's derived bindings -
// computed normals, tangents, meshlets, meshlet bounds, adjacency, weld, levels of detail - are one record, DerivedBindings.  Not part of the C ABI.
#pragma once
#include <chrono>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/corto_hip.h"
#include "crt_format.h"
#include "debug_config.h"
#include "device_plan.h"
#include "encoder_internal.h"
#include "kernels.h"
#include "plan_feedback.h"
#include "quant_out.h"
#include "tangent.h"
#include "meshlet.h"
#include "meshlet_bounds.h"
#include "adjacency.h"
#include "weld.h"
#include "lod.h"
#include "cloud_lod.h"
#include "compact.h"
#include "bvh.h"

using namespace corto_hip;

// errors: the thread's last message (crthip_last_error) and the code handed back
int fail(int code, const std::string &msg);
int fail(int code);
void fill_info(const BlobHeader &h, crthip_blob_info *info);   // host_probe.cpp: what crthip_probe / crthip_batch_info hand out
#define HIP_TRY(expr) \
	do { hipError_t e_ = (expr); if(e_ != hipSuccess) return fail(CRTHIP_E_DEVICE, std::string(#expr ": ") + hipGetErrorString(e_)); } while(0)
inline double now_us() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// ------------------------------------------------------------------------------------------------
struct DeviceBuf {
	void *p = nullptr; size_t cap = 0;
	int reserve(size_t n) {
		if(n <= cap) return CRTHIP_OK;
		if(p) { (void)hipFree(p); p = nullptr; cap = 0; }
		size_t want = std::max(n + n/4, (size_t)1 << 20);
		if(hipMalloc(&p, want) != hipSuccess) { p = nullptr; return CRTHIP_E_NOMEM; }
		cap = want;
		return CRTHIP_OK;
	}
	void release() { if(p) (void)hipFree(p); p = nullptr; cap = 0; }
};
struct PinnedBuf {
	void *p = nullptr; size_t cap = 0;
	int reserve(size_t n) {
		if(n <= cap) return CRTHIP_OK;
		if(p) { (void)hipHostFree(p); p = nullptr; cap = 0; }
		size_t want = std::max(n + n/4, (size_t)1 << 16);
		if(hipHostMalloc(&p, want, hipHostMallocDefault) != hipSuccess) { p = nullptr; return CRTHIP_E_NOMEM; }
		cap = want;
		return CRTHIP_OK;
	}
	void release() { if(p) (void)hipHostFree(p); p = nullptr; cap = 0; }
};

struct KernelTimer {
	std::vector<hipEvent_t> pool;
	struct Rec { const char *name; size_t e0, e1; };
	std::vector<Rec> recs;
	size_t used = 0;
	hipEvent_t get() {
		if(used == pool.size()) { hipEvent_t e; (void)hipEventCreate(&e); pool.push_back(e); }
		return pool[used++];
	}
	void reset() { used = 0; recs.clear(); }
	void release() { for(auto e : pool) (void)hipEventDestroy(e); pool.clear(); reset(); }
};

template <typename T> struct HostArr {  // host image of a device array + where it goes
	std::vector<T> v; uint64_t dev_off = 0;
};
static inline void push_blocks(HostArr<uint32_t> &map, uint32_t id, uint32_t count) { map.v.insert(map.v.end(), count, id); }   // `count` blocks of job `id` on a block -> job map

struct AttrScratch {
	// vals: int32 workspace of a generic attribute bound with a stride; facen: the fused normal kernel's face normals when not in LDS
	// qrange: the eight min | max words of a quantised attribute beyond QOUT_BLOB_MAX (k_quant_range)
	uint64_t color = ~0ull, diffs = ~0ull, vals = ~0ull, facen = ~0ull, qrange = ~0ull; std::vector<uint64_t> sym;
	void reset() { color = diffs = vals = facen = qrange = ~0ull; sym.clear(); }
};
struct BlobScratch {
	uint64_t clers = ~0ull, pred = ~0ull, front_a = ~0ull, front_b = ~0ull, order = ~0ull, delayed = ~0ull, faces = ~0ull;
	uint64_t progress = ~0ull;                              // the automaton's progress word (zeroed): blobs with an attribute too big for K-DELTA's LDS records
	uint32_t front_cap = 0, aux_groups = 0;
	uint64_t tan_acc = ~0ull;                               // computed tangents (DerivedBindings::tangents) of a blob beyond TANGENT_BLOB_MAX: 6 x int64 a vertex, inside the zeroed region
	uint64_t mlt = ~0ull;                                   // meshlets (DerivedBindings::meshlets) of a blob of more than one segment: mlt_scratch_layout's block
	uint64_t mlt_counts = ~0ull;                            // meshlet bounds (DerivedBindings::bounds) over a meshlet binding without a device counts record: 16 bytes for one
	uint64_t adj = ~0ull;                                   // adjacency (DerivedBindings::adjacency) of a blob beyond adj_in_blob: adj_scratch_layout's block
	uint64_t weld = ~0ull;                                  // weld (DerivedBindings::weld) of a blob beyond weld_in_blob: weld_scratch_layout's block
	uint64_t lod[CRTHIP_LOD_MAX_LEVELS] = {~0ull, ~0ull, ~0ull, ~0ull};   // levels of detail (DerivedBindings::lod): a level's lod_scratch_layout block
	uint64_t cloud_lod[CRTHIP_CLOUD_LOD_MAX_LEVELS] = {~0ull, ~0ull, ~0ull, ~0ull};   // a cloud's levels of detail (DerivedBindings::cloud_lod) beyond weld_in_blob: a level's cloud_lod_scratch_layout block
	uint64_t compact[CRTHIP_COMPACT_MAX_SETS] = {~0ull, ~0ull, ~0ull, ~0ull};   // compaction (DerivedBindings::compact): a set's compact_scratch_layout block
	uint64_t bvh = ~0ull;                                   // the BVH (DerivedBindings::bvh) of a blob beyond bvh_in_blob: bvh_scratch_layout's block
	uint64_t cn_facen = ~0ull;                              // computed normals (DerivedBindings::normals) by the fused kernel without its face normals in LDS: AttrScratch::facen's counterpart
	std::vector<AttrScratch> attr;
	size_t nattr = 0;                                       // attr[0..nattr) are this decode's (the vector only grows)
	void reset() { clers = pred = front_a = front_b = order = delayed = faces = progress = cn_facen = tan_acc = mlt = mlt_counts = adj = weld = bvh = ~0ull; for(uint64_t &l : lod) l = ~0ull; for(uint64_t &l : cloud_lod) l = ~0ull; for(uint64_t &l : compact) l = ~0ull; front_cap = 0; aux_groups = 0; nattr = 0; }
	void set_attrs(size_t n) { if(attr.size() < n) attr.resize(n); for(size_t k = nattr; k < n; k++) attr[k].reset();
		if(n > nattr) nattr = n; }
};

struct Plan {
	// job arrays
	// tun_dict: one entry per DISTINCT probability table (shared dictionaries)
	HostArr<TunStream> tun, tun_dict; HostArr<uint32_t> tun_chunk_stream;
	// streams by dictionary, in groups of one dictionary each (k_tun_stream_grouped)
	HostArr<uint32_t> tun_group_ids; HostArr<TunGroup> tun_groups; uint32_t clers_groups = 0;
	HostArr<FillJob> fill;
	HostArr<TopoJob> topo; HostArr<uint32_t> aux_u32;     // group_end lists
	// LDS automata in two size classes, one launch each
	HostArr<uint32_t> topo_lds_ids, topo_big_ids, topo_glob_ids; uint32_t topo_lds = 0, topo_big_lds = 0;
	// LDS bytes of topo_lds_ids' entries until they are split into the two classes
	std::vector<uint32_t> topo_need;
	// (unpack_wave_ids: the streams of small bit blocks, one wave each: k_unpack_wave)
	HostArr<UnpackJob> unpack; HostArr<uint32_t> unpack_chunk_job, unpack_wave_ids;
	HostArr<DeltaJob> delta;
	HostArr<DeltaGroup> delta_groups;                       // blobs whose attributes share one k_delta_lds16 workgroup
	HostArr<CloudJob> cloud; HostArr<uint32_t> cloud_chunk_job;
	HostArr<NormalJob> normal; HostArr<uint32_t> nv_block_job, nv_block_first, nf_block_job, nf_block_first, normal_fused_ids, normal_computed_ids;
	uint32_t normal_fused_lds = 0, normal_computed_lds = 0;   // (computed: k_normal_blob<true>'s id list and LDS request)
	HostArr<DequantJob> dequant; HostArr<uint32_t> dequant_block_job;
	// CRTHIP_BIND_QUANTIZED: jobs of up to QOUT_BLOB_MAX vertices by id (k_quant_out_blob), the others by block (k_quant_range, k_quant_store)
	HostArr<QuantOutJob> quant; HostArr<uint32_t> quant_blob_ids, quant_block_job;
	// crthip_batch_bind_computed_tangents: blobs of up to TANGENT_BLOB_MAX vertices by id (k_tangent_blob), the others by block (k_tangent_faces, k_tangent_vertex)
	HostArr<TangentJob> tangent; HostArr<uint32_t> tangent_blob_ids, tan_fblock_job, tan_vblock_job; uint32_t tangent_lds = 0;
	// crthip_batch_bind_meshlets: blobs of up to MESHLET_BLOB_SEGS segments by id (k_meshlet_blob, meshlet_waves the most segments among them), the
	// others a block a segment (k_meshlet_segments, k_meshlet_place); the segment tables are in aux_u32
	HostArr<MeshletJob> meshlet; HostArr<uint32_t> meshlet_blob_ids, mlt_block_job; uint32_t meshlet_waves = 0;
	// crthip_batch_bind_meshlet_bounds: (capacity + 3)/4 blocks a blob (k_meshlet_bounds)
	HostArr<MeshletBoundsJob> meshlet_bounds; HostArr<uint32_t> mlb_block_job;
	// crthip_batch_bind_adjacency: blobs whose lists fit LDS by id (k_adjacency_blob, adjacency_lds the largest request among them), the others by id
	// for the scan (k_adjacency_offsets) and 256 half-edges a block for the rest (k_adjacency_count, _fill, _twin)
	HostArr<AdjacencyJob> adjacency; HostArr<uint32_t> adjacency_blob_ids, adj_big_ids, adj_block_job; uint32_t adjacency_lds = 0;
	// crthip_batch_bind_weld: blobs whose table fits LDS by id (k_weld_blob, weld_lds the largest request among them), the others 256 vertices a
	// block (k_weld_insert, _lookup) and, those with an index output, 256 corners a block (k_weld_index)
	HostArr<WeldJob> weld; HostArr<uint32_t> weld_blob_ids, weld_vblock_job, weld_cblock_job; uint32_t weld_lds = 0;
	// crthip_batch_bind_lod: a job a bound level.  Jobs whose tables fit LDS by id (k_lod_blob, lod_lds the largest request among them), the others
	// by id for the scan (k_lod_offsets), 256 vertices a block (k_lod_insert, _lookup) and 256 faces a block (k_lod_faces, _keep, _scatter)
	HostArr<LodJob> lod; HostArr<uint32_t> lod_blob_ids, lod_big_ids, lod_vblock_job, lod_fblock_job; uint32_t lod_lds = 0;
	// crthip_batch_bind_cloud_lod: a job a bound level of a cloud.  Jobs whose table fits LDS by id (k_cloud_lod_blob, cloud_lod_lds the largest request
	// among them), the others by id for the scan (k_cloud_lod_offsets), 256 vertices a block (k_cloud_lod_insert, _lookup, _scatter) and, those with
	// a chunks array, a block a chunk of the capacity (k_cloud_lod_chunks)
	HostArr<CloudLodJob> cloud_lod; HostArr<uint32_t> cloud_lod_blob_ids, cloud_lod_big_ids, cloud_lod_vblock_job, cloud_lod_cblock_job; uint32_t cloud_lod_lds = 0;
	// crthip_batch_bind_compact: a job a bound MESH set.  Sets within compact_in_blob by id (k_compact_blob), the others by id for the scan
	// (k_compact_offsets), 256 vertices a block (k_compact_count, _place) and 256 corners a block (k_compact_mark, _index); and a job a GATHER of every
	// set, clouds' too, 256 copy units a block (k_compact_gather)
	HostArr<CompactJob> compact; HostArr<uint32_t> compact_blob_ids, compact_big_ids, compact_vblock_job, compact_cblock_job;
	HostArr<CompactGatherJob> compact_gather; HostArr<uint32_t> compact_gblock_job;
	// crthip_batch_bind_bvh: blobs within bvh_in_blob by id (k_bvh_blob, bvh_lds the largest request among them), the others by id for the scan
	// (k_bvh_sort_offsets), 256 faces a block (k_bvh_boxes, _keys, _tree, _refit) and a sort tile a block (k_bvh_sort_count, _scatter)
	HostArr<BvhJob> bvh; HostArr<uint32_t> bvh_blob_ids, bvh_big_ids, bvh_fblock_job, bvh_tblock_job; uint32_t bvh_lds = 0;
	bool meshlet_records = false;                           // a crthip_meshlet_counts a blob behind the quant records: a batch with a meshlet binding
	uint32_t quant_records = 0;                             // records behind the status words: sum(nattr) of a batch with a quantised binding, else 0
	// scratch regions (offsets)
	uint64_t zero_begin = 0, zero_end = 0;
	uint64_t tables_off = 0, tun_partial_off = 0, unpack_partial_off = 0, cloud_partial_off = 0;
	uint64_t facen_off = 0, cnt_off = 0, cursor_off = 0, bnd_off = 0, start_off = 0, flag_off = 0, slot_off = 0, adj_off = 0,
		nscan_partial_off = 0;
	uint64_t jobs_begin = 0, jobs_bytes = 0;
	uint32_t est_nvert = 0, est_nface = 0;                // totals over ESTIMATED/BORDER jobs
	uint32_t delta16_lds = 0;                              // largest LDS request among the k_delta_lds16 groups
	bool tun_multi_chunk = false, any_diff_normal = false, any_est_normal = false;
	uint32_t tun_max_nchunks = 0;
	uint64_t total = 0;
	// every job array, in the order they are placed in the block (Planner::group) - reset, placed and staged through here
	template <class F> void each_array(F f) {
		f(tun); f(tun_dict); f(tun_chunk_stream); f(tun_group_ids); f(tun_groups); f(fill); f(topo); f(aux_u32); f(topo_lds_ids); f(topo_big_ids);
		f(topo_glob_ids); f(unpack); f(unpack_chunk_job); f(unpack_wave_ids);
		f(delta); f(delta_groups); f(cloud); f(cloud_chunk_job); f(normal); f(nv_block_job); f(nv_block_first); f(nf_block_job); f(nf_block_first);
		f(normal_fused_ids); f(normal_computed_ids); f(dequant); f(dequant_block_job); f(quant); f(quant_blob_ids); f(quant_block_job);
		f(tangent); f(tangent_blob_ids); f(tan_fblock_job); f(tan_vblock_job);
		f(meshlet); f(meshlet_blob_ids); f(mlt_block_job); f(meshlet_bounds); f(mlb_block_job);
	}
	// ... and behind them the arrays that are placed only where a batch has them: a batch without an adjacency, a weld or a level-of-detail binding keeps its block byte for byte
	// (an empty array of each_array's still takes 16 bytes of the block; tests/cpp/plan_dump.cpp names those one by one)
	template <class F> void each_optional_array(F f) { f(adjacency); f(adjacency_blob_ids); f(adj_big_ids); f(adj_block_job); f(weld); f(weld_blob_ids); f(weld_vblock_job); f(weld_cblock_job); }
	// ... and, by the same rule, the arrays of the levels of detail.  They are a list of their own because tests/cpp/plan_dump.cpp names
	// each_optional_array's eight one by one
	template <class F> void each_lod_array(F f) { f(lod); f(lod_blob_ids); f(lod_big_ids); f(lod_vblock_job); f(lod_fblock_job); }
	// ... and of the clouds' levels of detail, behind them
	template <class F> void each_cloud_lod_array(F f) { f(cloud_lod); f(cloud_lod_blob_ids); f(cloud_lod_big_ids); f(cloud_lod_vblock_job); f(cloud_lod_cblock_job); }
	// ... and of the compaction, behind them
	template <class F> void each_compact_array(F f) { f(compact); f(compact_blob_ids); f(compact_big_ids); f(compact_vblock_job); f(compact_cblock_job); f(compact_gather); f(compact_gblock_job); }
	// ... and of the BVH, behind them
	template <class F> void each_bvh_array(F f) { f(bvh); f(bvh_blob_ids); f(bvh_big_ids); f(bvh_fblock_job); f(bvh_tblock_job); }
	void reset() {                                          // keep every vector's capacity
		each_array([](auto &a) { a.v.clear(); a.dev_off = 0; });
		each_optional_array([](auto &a) { a.v.clear(); a.dev_off = 0; });
		each_lod_array([](auto &a) { a.v.clear(); a.dev_off = 0; });
		each_cloud_lod_array([](auto &a) { a.v.clear(); a.dev_off = 0; });
		each_compact_array([](auto &a) { a.v.clear(); a.dev_off = 0; });
		each_bvh_array([](auto &a) { a.v.clear(); a.dev_off = 0; });
		clers_groups = 0; topo_need.clear(); quant_records = 0; meshlet_waves = 0; meshlet_records = false;
		topo_lds = topo_big_lds = normal_fused_lds = normal_computed_lds = tangent_lds = adjacency_lds = weld_lds = lod_lds = cloud_lod_lds = bvh_lds = 0;
		zero_begin = zero_end = tables_off = tun_partial_off = unpack_partial_off = cloud_partial_off = 0;
		facen_off = cnt_off = cursor_off = bnd_off = start_off = flag_off = slot_off = adj_off = nscan_partial_off = 0;
		jobs_begin = jobs_bytes = 0; est_nvert = est_nface = 0; delta16_lds = 0;
		tun_multi_chunk = any_diff_normal = any_est_normal = false; total = 0; tun_max_nchunks = 0;
	}
};

struct crthip_ctx {
	int device = 0;
	hipStream_t stream = nullptr;
	hipStream_t stream2 = nullptr;  // attribute streams (Tunstall + bit-unpack) run here while the main stream does topology; made by
	                                // the first launch that forks (ctx_stream2), never on a context that stays single-stream
	hipEvent_t ev_fork = nullptr, ev_join = nullptr;
	// recorded behind a decode's last kernel: what sync / done wait for, so that work a caller queues on the stream BEHIND a decode
	// does not delay the harvest of this one
	hipEvent_t ev_done = nullptr;
	DebugConfig dbg;                // every environment switch, read once when the context is made (debug_config.h)
	// largest LDS request for which K-NRM keeps its face normals in LDS (0 for a context that is one of many: crthip_ctx_set_single_stream)
	uint32_t normal_fn_max = NORMAL_FN_LDS_MAX;
	uint8_t single_stream = 0;                        // crthip_ctx_set_single_stream: no second HIP stream for the attribute streams
	// crthip_batch_create_resident: the walk's jobs + records on the device and their pinned host image; its two timing events (made on first use)
	DeviceBuf walk_dev;
	PinnedBuf walk_pin;
	hipEvent_t ev_walk0 = nullptr, ev_walk1 = nullptr;
	bool profiling = false;
	KernelTimer timer;
	crthip_batch *in_flight = nullptr;   // decode enqueued, status not harvested yet
	// crthip_ctx_set_packed_host_blobs: blobs laid out as an arena in the caller's pinned memory go up from there
	bool packed_host = false;
	crthip_splice_stats enc_splice{};                 // crthip_ctx_encode_splice_stats: the last crthip_encode_batch_to_device
	int encode_topology = CRTHIP_TOPOLOGY_HOST;       // crthip_ctx_set_encode_topology: where crthip_encode_batch runs the CLERS topology pass
	crthip_batch *last_decoded = nullptr;// whose intermediates the scratch block holds (crthip_batch_debug_read)
	// crthip_bvh_cast: the call's job-table blocks, pinned and on the device, made by the first cast and rotated (bvh_cast.cpp)
	struct CastState *cast = nullptr;
	// crthip_bvh_query: the same for the box queries, blocks of their own (bvh_query.cpp)
	struct QueryState *query = nullptr;
	// crthip_bvh_closest: and for the closest-face queries (bvh_closest.cpp)
	struct ClosestState *closest = nullptr;
	// crthip_decode_host: everything a one-blob decode with host buffers needs, kept from call to call (no hipMalloc / create in the
	// steady state) and guarded by a mutex so that callers may share a context between threads
	std::mutex host_mutex;
	crthip_batch *host_batch = nullptr;
	DeviceBuf host_out;       // decoded outputs of the one blob, back to back
	PinnedBuf host_pin;       // ... and their landing zone in pinned host memory (one async D2H copy)
	// what harvest() learns from a batch's flags (plan_feedback.h): K-DELTA's layout, the automaton's LDS edge slots
	DeltaFeedback delta;
	TopoFeedback topo;
	// planner state reused from one decode call to the next (batch.cpp: build_and_launch)
	std::vector<const uint8_t *> plan_clers, plan_logs;
	// streams of a batch that carry the same probability table share one dictionary: exact match on the table's bytes (alphabets of up
	// to 16 symbols; bigger ones hardly ever repeat and are quick to build), open addressing on a hash of them
	struct DictKey { uint8_t n, bytes[32]; };
	std::vector<DictKey> dict_keys;
	std::vector<uint32_t> dict_slots, dict_used, dict_ids, dict_count;
	// What ONE decode call owns, by the batch object's parity (crthip_batch_set_parity).  crthip_batch_decode_with_next keeps two batches alive on
	// the context - one in its mesh stage, the next one's entropy stage beside it - so there are two sets, and every use names the batch whose set
	// it means: ctx_set(ctx, b).  A Planner binds its batch's set for life.  A context whose batches all have parity 0 (every lone context, the
	// facade) never touches set[1], whose buffers are allocated on first use.  Shared by both: the stream, in_flight / ev_done (one call in
	// flight), and what harvest() learns - a batch planned before its predecessor's flags were read learns from them one batch late.
	struct Half {
		DeviceBuf scratch;        // symbols, tables, fronts, predictions, job arrays ...
		PinnedBuf staging;        // host image of the job arrays
		PinnedBuf arena_pin;      // host image of a batch's blobs on their way to the device (batch_fill: one H2D copy, not waited for)
		PinnedBuf status_host;    // StatusWords, and the quant records behind them
		// arena_pin uploads enqueued so far / how many of them sit IN FRONT of ev_done (harvest may only call those complete)
		uint32_t upload_seq = 0, done_covers_seq = 0;
		// a batch's blobs are (perhaps still) on their way from arena_pin: cleared by whoever synchronises the stream
		bool arena_upload_pending = false;
		Plan plan; std::vector<BlobScratch> plan_scratch;
		void release() { scratch.release(); staging.release(); arena_pin.release(); status_host.release(); }
	} set[2];
};

// bytes per component of a generic attribute's caller buffer: upstream decodes in place as int32 whatever the format and DOUBLE widens
// in place (include/corto/vertex_attribute.h:184-228), so every format's buffer is nvert*N*4 bytes but DOUBLE's
static inline size_t generic_work_bytes(uint32_t format) { return format == CRTHIP_FMT_DOUBLE ? 8u : 4u; }

struct Binding { void *buffer = nullptr; uint32_t format = CRTHIP_FMT_FLOAT, out_components = 4, stride = 0; bool stream_values = false, quantized = false; };   // stream_values: CRTHIP_BIND_STREAM_VALUES; quantized: CRTHIP_BIND_QUANTIZED
// a generic attribute decoded as int32 in device scratch and finished by a job of its own: a stride, DOUBLE, or uint16 grid values
static inline bool generic_in_scratch(const Binding &bd) { return bd.stride || bd.format == CRTHIP_FMT_DOUBLE || bd.quantized; }

// The outputs derived from a blob's decoded data, each bound by a call of its own behind crthip_batch_bind.  A call drops what was bound on top of what
// it changes: the three functions are that rule, and the only place it is written
struct DerivedBindings {
	Binding normals;                       // crthip_batch_bind_computed_normals: where the normals of a blob that stores (or binds) none go
	Binding tangents;                      // crthip_batch_bind_computed_tangents: where the blob's tangents go (out_components 4)
	crthip_meshlet_binding meshlets{};     // crthip_batch_bind_meshlets: meshlets.meshlets != null - where the blob's meshlets go
	crthip_meshlet_bounds *bounds = nullptr;   // crthip_batch_bind_meshlet_bounds: a record a meshlet
	crthip_adjacency_binding adjacency{};  // crthip_batch_bind_adjacency: adjacency.twin != null - where the blob's twins go (reads the index alone)
	crthip_weld_binding weld{};            // crthip_batch_bind_weld: weld.remap != null - where the blob's weld map goes (reads the integer positions and the index)
	crthip_lod_binding lod{};              // crthip_batch_bind_lod: lod.levels != 0 - where the blob's levels of detail go (reads the integer positions and the index)
	crthip_cloud_lod_binding cloud_lod{};  // crthip_batch_bind_cloud_lod: cloud_lod.levels != 0 - where a cloud's levels of detail go (reads the integer positions)
	crthip_compact_binding compact{};      // crthip_batch_bind_compact: compact.sets != 0 - where the blob's compact sets go (reads other bindings' outputs: the functions below)
	crthip_bvh_binding bvh{};              // crthip_batch_bind_bvh: bvh.nodes != null - where the blob's BVH goes (reads the integer positions and the index)
	void clear() { *this = DerivedBindings{}; }       // a bind (and a blob adopted by a fill): all of them read what it binds
	// a normals call: the tangents' normal source may change; a compaction that gathers either goes with them
	void normals_change() { tangents = Binding{}; if(compact_gathers(CRTHIP_COMPACT_COMPUTED_NORMALS) || compact_gathers(CRTHIP_COMPACT_COMPUTED_TANGENTS)) compact = crthip_compact_binding{}; }
	void tangents_change() { if(compact_gathers(CRTHIP_COMPACT_COMPUTED_TANGENTS)) compact = crthip_compact_binding{}; }   // a tangents call
	void meshlets_change() { bounds = nullptr; }      // a meshlets call: the bounds' arrays and capacity change
	void source_change(uint32_t source) { if(compact_reads(source)) compact = crthip_compact_binding{}; }   // a weld, lod or cloud lod call that sets, replaces or removes: a compaction that names it goes
	bool compact_reads(uint32_t source) const { for(uint32_t s = 0; s < compact.sets && s < CRTHIP_COMPACT_MAX_SETS; s++) if(compact.set[s].source == source) return true; return false; }
	bool compact_gathers(uint32_t what) const {
		for(uint32_t s = 0; s < compact.sets && s < CRTHIP_COMPACT_MAX_SETS; s++)
			for(uint32_t q = 0; q < compact.set[s].ngather && q < CRTHIP_COMPACT_MAX_GATHERS; q++) if(compact.set[s].gather[q].source == what) return true;
		return false;
	}
	// the compaction reads level k of the lod (cloud: the cloud lod) binding, so its record must exist somewhere: the set that does, or -1
	int compact_set_of(uint32_t source, uint32_t level) const {
		for(uint32_t s = 0; s < compact.sets && s < CRTHIP_COMPACT_MAX_SETS; s++) if(compact.set[s].source == source && compact.set[s].level == level) return (int)s;
		return -1;
	}
};

struct BlobPlan {
	BlobLayout L;
	uint64_t arena_off = 0;
	uint32_t len = 0;
	std::vector<Binding> bind;
	void *index = nullptr; uint32_t index_u16 = 0;
	DerivedBindings derived;
	int32_t host_status = 0;   // set by the planner (e.g. unsupported format), overrides device status
	// debug handles (scratch offsets valid after decode)
	uint64_t dbg_clers = ~0ull, dbg_pred = ~0ull; uint32_t dbg_nclers = 0;
	bool clers_in_arena = false;
};

struct crthip_batch {
	crthip_ctx *ctx = nullptr;
	std::vector<BlobPlan> blobs;
	const uint8_t *d_arena = nullptr;
	DeviceBuf own_arena;
	uint64_t arena_bytes = 0;
	bool dirty = true;
	crthip_batch_stats stats{};
	crthip_walk_stats walk{};
	std::vector<int32_t> status;
	bool decoded = false;
	bool planned_wide = false;          // the decode in flight was planned with K-DELTA's 32-bit layout
	bool carriable = false;             // (account) the decode's entropy stage fits another batch's grids AND its own grids can carry one: what a pool lane asks before it pipelines
	uint8_t parity = 0;                 // which of the context's two sets of per-call blocks this object uses (crthip_batch_set_parity)
	// crthip_batch_decode_with_next planned this batch as `next`: its planner, kept until the call that runs its mesh stage (e_done: its entropy
	// stage has been enqueued; else that call runs the whole schedule)
	struct Planner *staged = nullptr;
	// CRTHIP_BIND_QUANTIZED: the caller's device record array (crthip_batch_bind_quant_transforms); the last decode's records as harvest
	// found them in the status block and which of them belong to a quantised binding (crthip_batch_bind_all's order)
	void *quant_dev = nullptr;
	std::vector<crthip_quant_transform> quant_recs; std::vector<uint8_t> quant_bound;
	// crthip_batch_bind_meshlets: which blobs of the last decode had a binding, and their records as harvest found them
	std::vector<uint8_t> meshlet_bound; std::vector<crthip_meshlet_counts> meshlet_recs;
};
void drop_staged(crthip_batch *b);      // (batch.cpp)
inline crthip_ctx::Half &ctx_set(crthip_ctx *ctx, const crthip_batch *b) { return ctx->set[b->parity]; }   // the batch's set of per-call blocks

// The per-blob status block: four int32 words a blob in the pinned host memory of the batch's set (status_host), written by the kernels, zeroed by
// Planner::upload, read by harvest
struct StatusWords {
	size_t n, quant_records = 0; bool meshlets = false;            // blobs; Plan::quant_records; Plan::meshlet_records
	size_t status(size_t i) const { return i; }                    // the blob's CRTHIP_* code (k_topology*, k_normal*, k_delta_tiles)
	size_t topo_flags(size_t i) const { return n + i; }            // bit 0: the automaton was redone on the HBM front; above it the slots it needed
	size_t delta_flags(size_t i) const { return 2*n + 2*i; }       // two words: an attribute's values left int16 / an attribute took the walk
	// behind them (16-byte aligned): the crthip_quant_transform records of a batch with a quantised binding, one an attribute
	size_t records() const { return n*16; }
	// ... and behind those (16-byte aligned) a crthip_meshlet_counts a blob of a batch with a meshlet binding
	size_t meshlet_record(size_t i) const { return ((n*16 + quant_records*sizeof(crthip_quant_transform) + 15) & ~(size_t)15) + i*sizeof(crthip_meshlet_counts); }
	size_t bytes() const { return meshlet_record(meshlets ? n : 0); }  // the whole block
};

int harvest(crthip_ctx *ctx);     // wait for the batch in flight on the context, keep its per-blob status, learn from its flags (batch.cpp)
int ctx_stream2(crthip_ctx *ctx, hipStream_t *out);   // the context's second stream, made on first use (batch.cpp)
void cast_state_release(crthip_ctx *ctx);               // a context's cast blocks go with it (bvh_cast.cpp)
void query_state_release(crthip_ctx *ctx);              // ... and its query blocks (bvh_query.cpp)
void closest_state_release(crthip_ctx *ctx);            // ... and its closest-face blocks (bvh_closest.cpp)

// ------------------------------------------------------------------------------------------------
// planner: what turns the walked layouts + bindings into job arrays inside one scratch block
// (Carver, the bump allocator over the scratch block: encoder_internal.h - the batch encoder carves its image with it too)

// the two launch classes of K-DELTA (k_delta.hip): values + prediction graph fit LDS, one wave per attribute (k_delta_lds16) - as int16 relative to
// vertex 0, or - `wide`: a context that met values beyond int16 - as int32; else tiles out of an LDS ring (k_delta_tiles: meshes beyond LDS,
// attributes of more than four components)
static inline bool delta_hosts_a(const DeltaJob &d) { return !d.is_u8 && d.N == 3; }
static inline uint64_t delta_lds_need(const DeltaJob &d, bool wide) {          // alone in a workgroup; ~0: not eligible
	if(d.nvert > DELTA16_NVERT_MAX || d.N < 1 || d.N > 4) return ~0ull;
	return (uint64_t)delta_vbytes(d.nvert, d.N, d.is_u8 != 0, wide) + delta16_graph_lds(d.nvert, delta_hosts_a(d));
}
static inline bool delta_in_lds(const DeltaJob &d, bool wide) { return delta_lds_need(d, wide) <= DELTA16_LDS_MAX; }
// the computed normals of a blob: bound, a mesh, and no stored "normal" attribute bound beside them (the bind call sees to all three)
static inline bool computes_normals(const BlobPlan &P) {
	if(!P.derived.normals.buffer || P.L.h.nface == 0) return false;
	for(size_t k = 0; k < P.bind.size(); k++) if(P.L.h.attrs[k].name == "normal" && P.bind[k].buffer) return false;
	return true;
}
static bool normal_fused(uint32_t nvert, uint32_t nface) { return nvert <= 32767 && (uint64_t)3*nface <= 65535 && normal_blob_lds(nvert,
	nface) <= NORMAL_LDS_MAX; }

// computed tangents (crthip_batch_bind_computed_tangents): blobs of up to TANGENT_BLOB_MAX vertices take k_tangent_blob - one workgroup and 24 bytes of
// LDS a vertex, 54 KB at the limit, which holds a 2 112-vertex C4 blob and is what a lane of TAN_BLOB_SLOTS vertices in registers covers - the
// others k_tangent_faces / k_tangent_vertex.  The bind call made sure of a mesh, a position, a uv and a normal source
constexpr uint32_t TANGENT_BLOB_MAX = TAN_BLOB_SLOTS*TAN_THREADS;          // 2 304
static inline bool computes_tangents(const BlobPlan &P) { return P.derived.tangents.buffer && P.L.h.nface > 0; }
static inline bool tangent_in_blob(uint32_t nvert) { return nvert <= TANGENT_BLOB_MAX; }

// meshlets (crthip_batch_bind_meshlets): a blob of up to MESHLET_BLOB_SEGS segments takes k_meshlet_blob - one workgroup, a wave a segment, so a
// workgroup's four waves; more segments would queue behind one another in a workgroup while the chip has idle CUs - the others
// k_meshlet_segments / k_meshlet_place, a workgroup a segment
constexpr uint32_t MESHLET_BLOB_SEGS = 4;
static inline bool builds_meshlets(const BlobPlan &P) { return P.derived.meshlets.meshlets && P.L.h.nface > 0; }
static inline bool bounds_meshlets(const BlobPlan &P) { return P.derived.bounds && builds_meshlets(P); }
namespace corto_hip { const char *meshlet_binding_error(const crthip_meshlet_binding *m, bool have_bound, const crthip_meshlet_counts &bound); }
// the cuts and the capacity bound of a blob's index under a meshlet binding (the blob's own, or the one a bind call is about to take)
static inline bool mlt_plan_of(const BlobPlan &P, const crthip_meshlet_binding &m, std::vector<MltSeg> *segs, crthip_meshlet_counts &bound) {
	return mlt_plan(P.L.h.nface, (uint32_t)P.L.group_end.size(), P.L.group_end.data(), m.max_vertices, m.max_triangles, m.segment_faces, segs, bound);
}

// adjacency (crthip_batch_bind_adjacency): a blob whose ends and 16-bit entries fit ADJ_BLOB_LDS_MAX takes k_adjacency_blob, the others the four
// kernels over scratch (adjacency.h: adj_in_blob)
static inline bool binds_adjacency(const BlobPlan &P) { return P.derived.adjacency.twin && P.L.h.nface > 0; }

// weld (crthip_batch_bind_weld): a blob whose table fits WELD_BLOB_LDS_MAX takes k_weld_blob, the others the three kernels over scratch (weld.h:
// weld_in_blob).  welds_adjacency: the blob's adjacency kernels read the welded index (CRTHIP_WELD_ADJACENCY, looked at when a decode is planned)
static inline bool binds_weld(const BlobPlan &P) { return P.derived.weld.remap && P.L.h.nface > 0; }
static inline bool welds_adjacency(const BlobPlan &P) { return binds_weld(P) && binds_adjacency(P) && (P.derived.weld.flags & CRTHIP_WELD_ADJACENCY) && P.derived.weld.index; }

// levels of detail (crthip_batch_bind_lod): a job a level; one whose tables fit LOD_BLOB_LDS_MAX takes k_lod_blob, the others the six kernels over
// scratch (lod.h: lod_in_blob)
static inline bool binds_lod(const BlobPlan &P) { return P.derived.lod.levels && P.L.h.nface > 0; }

// a cloud's levels of detail (crthip_batch_bind_cloud_lod): a job a level; one whose table fits WELD_BLOB_LDS_MAX takes k_cloud_lod_blob, the
// others the five kernels over scratch (cloud_lod.h; weld.h: weld_in_blob)
static inline bool binds_cloud_lod(const BlobPlan &P) { return P.derived.cloud_lod.levels && P.L.h.nface == 0 && P.L.h.nvert > 0; }

// compaction (crthip_batch_bind_compact): a job a mesh set - one within compact_in_blob takes k_compact_blob, the others the five kernels over
// scratch - and a job a gather of every set (compact.h)
static inline bool binds_compact(const BlobPlan &P) { return P.derived.compact.sets != 0; }

// the BVH (crthip_batch_bind_bvh): a blob within bvh_in_blob takes k_bvh_blob, the others the kernels over scratch (bvh.h)
static inline bool binds_bvh(const BlobPlan &P) { return P.derived.bvh.nodes && P.L.h.nface > 0; }

// where the derived outputs and the estimated normals take their inputs.  An attribute by name: the last one of that name, or -1
static inline int attr_named(const BlobPlan &P, const char *name) {
	int k = -1;
	for(size_t j = 0; j < P.bind.size(); j++) if(P.L.h.attrs[j].name == name) k = (int)j;
	return k;
}
// attribute k can serve as an integer source: generic, N components, bound, and not as stream values (upstream throws there too, normal_attribute.cpp:210-213)
static inline bool generic_source_ok(const BlobPlan &P, int k, uint32_t N) {
	return k >= 0 && P.L.h.attrs[k].codec == CRTHIP_CODEC_GENERIC && P.L.h.attrs[k].N == N && P.bind[k].buffer && !P.bind[k].stream_values;
}
// the normals a blob's tangents read: the computed binding, else the first bound attribute named "normal" that is coded as one; or null
static inline const Binding *tangent_normal_source(const BlobPlan &P) {
	if(computes_normals(P)) return &P.derived.normals;
	for(size_t k = 0; k < P.bind.size(); k++)
		if(P.L.h.attrs[k].name == "normal" && P.L.h.attrs[k].codec == CRTHIP_CODEC_NORMAL && P.bind[k].buffer) return &P.bind[k];
	return nullptr;
}
// what a gather of crthip_batch_bind_compact copies: the source's own buffer as bound, its element size E, E's alignment A and the byte distance
// of two vertices; or the error, in the header's order (a number out of range, unbound or missing: ARGUMENT; outside the table: FORMAT)
struct CompactSource { const void *buffer; uint32_t E, A, stride; int err; const char *why; };
static inline CompactSource compact_source_of(const BlobPlan &P, uint32_t source) {
	auto of = [](const Binding &bd, uint32_t E, uint32_t A) { return CompactSource{bd.buffer, E, A, bd.stride ? bd.stride : E, CRTHIP_OK, nullptr}; };
	if(source == CRTHIP_COMPACT_COMPUTED_NORMALS) {
		if(!computes_normals(P)) return CompactSource{nullptr, 0, 0, 0, CRTHIP_E_ARGUMENT, "the blob has no computed normals binding"};
		const bool i16 = P.derived.normals.format == CRTHIP_FMT_INT16;
		return of(P.derived.normals, i16 ? 6u : 12u, i16 ? 2u : 4u);
	}
	if(source == CRTHIP_COMPACT_COMPUTED_TANGENTS) {
		if(!computes_tangents(P)) return CompactSource{nullptr, 0, 0, 0, CRTHIP_E_ARGUMENT, "the blob has no computed tangents binding"};
		const bool i16 = P.derived.tangents.format == CRTHIP_FMT_INT16;
		return of(P.derived.tangents, i16 ? 8u : 16u, i16 ? 2u : 4u);
	}
	if(source >= P.bind.size()) return CompactSource{nullptr, 0, 0, 0, CRTHIP_E_ARGUMENT, "the attribute number is out of range"};
	const Binding &bd = P.bind[source];
	const AttrHeader &a = P.L.h.attrs[source];
	if(!bd.buffer) return CompactSource{nullptr, 0, 0, 0, CRTHIP_E_ARGUMENT, "the attribute is not bound"};
	if(a.codec == CRTHIP_CODEC_NORMAL) { const bool i16 = bd.format == CRTHIP_FMT_INT16; return of(bd, i16 ? 6u : 12u, i16 ? 2u : 4u); }
	if(a.codec == CRTHIP_CODEC_COLOR) return of(bd, bd.out_components, 1u);
	if(bd.stream_values) return CompactSource{nullptr, 0, 0, 0, CRTHIP_E_FORMAT, "the attribute is bound with CRTHIP_BIND_STREAM_VALUES: a work array, not vertex records"};
	if(bd.quantized) return of(bd, 2u*a.N, 2u);
	if(bd.format != CRTHIP_FMT_FLOAT) return CompactSource{nullptr, 0, 0, 0, CRTHIP_E_FORMAT, "the attribute is bound in an integer format or DOUBLE: a work array, not vertex records"};
	return of(bd, 4u*a.N, 4u);
}
int compact_binding_error(const BlobPlan &P, const crthip_compact_binding *c, std::string &why);   // (batch_bind.cpp: every check of the bind call)
// a set's block of scratch: a newid of its own where a bigger set has an index and no newid, an order of its own where a mesh set has gathers and no order
static inline CompactScratchLayout compact_layout_of(const BlobPlan &P, const crthip_compact_set &t) {
	const bool cloud = t.source == CRTHIP_COMPACT_CLOUD_LOD;
	return compact_scratch_layout(P.L.h.nvert, P.L.h.nface, cloud, !t.newid && t.index, !cloud && !t.order && t.ngather ? std::min(t.vertex_capacity, P.L.h.nvert) : 0u);
}

struct Launch {
	crthip_ctx *ctx;
	hipStream_t cur = nullptr;
	void begin(const char *name, hipStream_t s = nullptr) {
		cur = s ? s : ctx->stream;
		if(!ctx->profiling) return;
		hipEvent_t e = ctx->timer.get();
		(void)hipEventRecord(e, cur);
		ctx->timer.recs.push_back({name, ctx->timer.used - 1, 0});
	}
	void end() {
		if(!ctx->profiling) return;
		hipEvent_t e = ctx->timer.get();
		(void)hipEventRecord(e, cur);
		ctx->timer.recs.back().e1 = ctx->timer.used - 1;
	}
	// one kernel under one record (a record that spans several launches keeps its own begin / end around them)
	template <class K, class... A> void run(const char *name, K kernel, dim3 grid, dim3 block, uint32_t lds, hipStream_t s, A... args) {
		begin(name, s); hipLaunchKernelGGL(kernel, grid, block, lds, s, args...); end();
	}
};
// the long-stream Tunstall chain (plan_launch.cpp): K-TAB, and for streams of several chunks (`multi`) the chunk sums, the stream scan beyond 256
// chunks a stream and the staged decode - else k_tun_decode, a chunk a stream; then k_fill.  `tun`: the host image of `streams`
int tun_chain(Launch &LT, hipStream_t st, const std::vector<TunStream> &tun, const TunStream *streams, const uint32_t *chunk_stream, uint32_t chunks,
	TunTable *tables, uint64_t *partial, uint32_t max_nchunks, bool multi, const FillJob *fill, uint32_t nfill);

// The planner of one decode call, stage by stage (round 4: this was one function of 660 lines).  carve() lays the batch's scratch out
// (pass 1: sizes and offsets only), jobs() writes the job descriptors of every stage (pass 2), group() sorts streams by dictionary and
// attributes into K-DELTA workgroups and places the job arrays, upload() reserves the blocks, resolves the pointers and stages the arrays,
// launch() enqueues the kernels in the order of crt::Decoder::decodeMesh / decodePointCloud (src/decoder.cpp:133-196), account() fills
// crthip_batch_stats.
// Planning overlaps the batch in flight, so jobs() runs before the scratch block is reserved: a descriptor's pointer into scratch is
// SP(offset), the offset with bit 63 set, and upload() passes every pointer field through resolve(), which turns those into base + offset
// and leaves every other pointer (the arena, the caller's buffers, the pinned status words, null) as it is.  A user-space address on
// x86-64 never has bit 63 set.  The one exception: TopoJob.group_end holds a byte offset into aux_u32 (placed after jobs()).
// the next batch's K-TAB / K-STREAM arguments, for the grids of the batch that carries them (plan_launch.cpp)
struct Carry {
	const TunStream *dicts; uint32_t ndicts; TunTable *tables;
	const TunStream *streams; const uint32_t *ids; const TunGroup *groups; uint32_t ngroups;
};
// what Planner::launch enqueues: the descriptor copy and the zeroing | K-TAB, K-STREAM | k_fill (stage E) | everything else (stage M)
enum : uint32_t { PH_UP = 1, PH_TUN = 2, PH_FILL = 4, PH_MESH = 8, PH_ENTROPY = PH_UP | PH_TUN | PH_FILL, PH_ALL = 15 };
struct Planner {
	crthip_batch *b; crthip_ctx *ctx; crthip_ctx::Half &set; Plan &pl; std::vector<BlobScratch> &bs;   // set: the batch's (ctx_set); pl, bs: its plan and scratch offsets
	// wide: K-DELTA with 32-bit values in LDS (this context met values beyond int16)
	const uint32_t nblobs; const bool wide; const uint8_t *arena;
	Carver cv;
	uint64_t unpack_state_words = 1, n_tun = 0, stat_tin = 0, stat_tout = 0, stat_tt = 0, stat_dicts = 0;
	uint32_t tun_chunks = 0, unpack_chunks = 0, cloud_chunks = 0;
	// the CLERS streams come first in every stream / chunk / fill / dictionary array
	uint32_t clers_tun = 0, clers_chunks = 0, clers_fill = 0, clers_dict = 0;
	bool share_clers = false, share_attrs = false;
	int32_t *hs_base = nullptr; StatusWords hs;                              // per-blob status words in pinned host memory
	uint8_t *base = nullptr, *stage = nullptr;                               // the scratch block; the host image of the job arrays

	uint32_t dict_group0 = 0; QuantOutRecord *quant_rec_host = nullptr;      // jobs(): first dictionary of the current launch group (CLERS / attribute streams); the quant records behind the status words
	Planner(crthip_batch *b_) : b(b_), ctx(b_->ctx), set(ctx_set(b_->ctx, b_)), pl(set.plan), bs(set.plan_scratch), nblobs((uint32_t)b_->blobs.size()),
		wide(b_->ctx->delta.wide), arena(b_->d_arena), hs{b_->blobs.size()} {}
	static uint8_t *SP(uint64_t off) { return (uint8_t *)(uintptr_t)(off | (1ull << 63)); }   // a scratch offset in a pointer field
	template <class T> void resolve(T *&p) const {
		const uintptr_t v = (uintptr_t)p;
		if(v >> 63) p = (T *)(base + (v & ~(1ull << 63)));
	}
	// FillJobs that zero the scratch range [off, off + bytes) in stage E (a FillJob's size is 32 bits: 2^30 bytes a job at most)
	void zero_fill(uint64_t off, uint64_t bytes) { for(uint64_t o = 0; o < bytes; o += 1u << 30) pl.fill.v.push_back(FillJob{SP(off + o), (uint32_t)std::min<uint64_t>(bytes - o, 1u << 30), 0u}); }
	bool e_done = false;                                                     // stage E has been enqueued (by an earlier call)
	int carve(); int jobs(); void group(); int upload(); int launch(uint32_t phases = PH_ALL, const Carry *carry = nullptr); int mark_done(); void account();
	uint32_t qout_blob_max() const { return ctx->dbg.qout_blob_max ? ctx->dbg.qout_blob_max : QOUT_BLOB_MAX; }   // a quantised attribute's size class
	// The schedule's shape, decided in one place (plan_launch.cpp).  LongStreams: a stream of several chunks - one scan over all chunks, no separate
	// entropy stage.  Forked: a mesh batch with attribute work on a context with two streams - the attribute streams beside the automata.  OneStream:
	// everything else - the entropy stage (PH_*) in front of the mesh stage on the main stream; the only shape that splits() and that carries
	enum class Shape { LongStreams, Forked, OneStream };
	Shape shape() const;
	bool splits() const { return shape() == Shape::OneStream; }
	bool takes_front() const; bool carry_args(Carry &c) const; bool hosts_carry() const;
	// launch() by stage (plan_launch.cpp), in the order they are enqueued
	Launch LT{ctx};
	uint32_t nbig = 0, nslices = 0; bool tiles_launched = false;             // K-DELTA's jobs too big for the LDS records (sorted to the front; the slices: the last nslices of them)
	template <class T> T *D(HostArr<T> &arr) const { return (T *)(base + arr.dev_off); }   // a job array on the device
	// the (jobs, ids, n) launch on the main stream: a workgroup an id, nothing for an empty list
	template <class K, class J, class... A> void by_ids(const char *name, K kernel, uint32_t threads, uint32_t lds, HostArr<J> &jobs, HostArr<uint32_t> &ids, A... more) {
		const uint32_t n = (uint32_t)ids.v.size();
		if(n) LT.run(name, kernel, dim3(n), dim3(threads), lds, ctx->stream, D(jobs), D(ids), n, more...);
	}
	int fork(hipStream_t *s2); int join(hipStream_t s2);
	void entropy(hipStream_t s, uint32_t phases, uint32_t t0, uint32_t t1, uint32_t f0, uint32_t f1); int long_streams(); int forked();
	void topology(); void unpack(hipStream_t s); void front(const Carry *carry); void delta_tiles(hipStream_t s); void delta(const Carry *carry);
	void cloud(); void normals(); void derived(); void finish();
	// a blob's integer sources as a job takes them: attribute k's values where K-DELTA leaves them and the index where the automaton does - the caller's, or scratch
	int32_t *ints_of(uint32_t i, size_t k) const { const Binding &bd = b->blobs[i].bind[k]; return (int32_t *)(generic_in_scratch(bd) ? SP(bs[i].attr[k].vals) : bd.buffer); }
	struct Faces { void *p; uint8_t u16; };
	Faces faces_of(uint32_t i) const { const BlobPlan &P = b->blobs[i]; return P.index ? Faces{P.index, (uint8_t)P.index_u16} : Faces{SP(bs[i].faces), 0}; }
	// jobs() by stage (plan_jobs.cpp): the streams of the entropy stage, then what one blob contributes
	struct BlobView; struct BitBlock;
	uint32_t est_vbase = 0, est_fbase = 0;                                   // the unfused normal jobs' slices of the batch-wide arrays, in job order
	void clear_dict_table(); uint32_t dict_of(const StreamRef &s, const TunStream &t); const uint8_t *add_stream(const StreamRef &s, uint64_t sym_off, uint64_t blob_off);
	void push_unpack(const BitBlock &bb, const StreamRef &s, const uint8_t *logs, void *out, uint8_t mode, uint16_t fields, uint16_t stride, uint16_t comp, uint8_t out_kind);
	BlobView view_of(uint32_t i, size_t rec0); void topo_job(const BlobView &v); void attr_jobs(const BlobView &v, size_t k);
	bool inverse_job(const BlobView &v, size_t k, void *values, uint32_t N, bool para, uint8_t is_u8, bool hand_i16);
	void stored_normal_job(const BlobView &v, size_t k, bool hand_i16); void quant_job(const BlobView &v, size_t k); void dequant_job(const BlobView &v, size_t k);
	bool estimated_normal_tail(const BlobView &v, NormalJob &n, HostArr<uint32_t> &fused_ids, uint32_t &fused_lds, uint64_t facen);
	bool computed_normal_job(const BlobView &v); bool tangent_job(const BlobView &v); void meshlet_jobs(const BlobView &v); void weld_jobs(const BlobView &v); void adjacency_jobs(const BlobView &v); void lod_jobs(const BlobView &v); void cloud_lod_jobs(const BlobView &v); void compact_jobs(const BlobView &v); void bvh_jobs(const BlobView &v);
};

