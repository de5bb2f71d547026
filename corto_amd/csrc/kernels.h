// kernels.h — declarations of the HIP kernels (k_tunstall.hip, k_stream.hip, k_mesh.hip, k_normal.hip)
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "device_plan.h"

namespace corto_hip {

// k_tunstall.hip
__global__ void k_tun_tables(const TunStream *streams, uint32_t nstreams, TunTable *tables);
__global__ void k_tun_stream(const TunStream *streams, uint32_t nstreams);   // short streams: dictionary + decode by one wave, the dictionary never leaves LDS
__global__ void k_tun_stream_grouped(const TunStream *streams, const uint32_t *ids, const TunGroup *groups, uint32_t ngroups, const TunTable *tables);   // ... streams of ONE dictionary, up to TUN_GROUP_MAX per workgroup, from one copy of it in LDS
__global__ void k_tun_stream_scan(const TunStream *streams, uint32_t nstreams, uint64_t *chunk_out);   // one stream's quarter sums -> its quarter offsets (one workgroup per stream)
__global__ void k_tun_chunk_sums(const TunStream *streams, const uint32_t *chunk_stream, uint32_t nchunks, const TunTable *tables,
                                 uint64_t *chunk_out, uint32_t chunk_base);
__global__ void k_tun_decode(const TunStream *streams, const uint32_t *chunk_stream, uint32_t nchunks, const TunTable *tables,
                             const uint64_t *chunk_out, uint32_t chunk_base);
// Dwords of a word's zero-padded copy the staged decode composes from (k_tunstall.hip): by the dictionary's longest word;
// steps of fewer than 8 codewords per lane (mean word length > 8) are only compiled for 4.
__host__ __device__ inline uint32_t tun_width(uint32_t cpl, uint32_t maxlen) { return cpl < 8 || maxlen > 8 ? 4u : maxlen > 4 ? 2u : 1u; }
int launch_tun_decode_staged(hipStream_t stream, const TunStream *streams, const uint32_t *chunk_stream, uint32_t nchunks, const TunTable *tables,
                             uint64_t *chunk_out, uint32_t sums_only);    // words <= 4 bytes, <= 8 bytes, longer: three bodies of one kernel
// blocks of a launch whose kernel takes its job by xcd_slot() (kernels_common.h: every XCD a contiguous eighth of the jobs)
__host__ __device__ inline uint32_t xcd_grid(uint32_t n) { return 8u*((n + 7u) >> 3); }
__global__ void k_fill(const FillJob *jobs, uint32_t njobs);
__global__ void k_fill_block(uint8_t *dst, uint64_t bytes, uint32_t value);

// k_walk.hip: one wave per blob walks the blob at base + off (16-byte aligned) and writes its crt_walk.h record to records + i*rec_cap
struct WalkJob { uint64_t off; uint32_t len, pad; };
__global__ void k_walk_blobs(const uint8_t *base, const WalkJob *jobs, uint32_t nblobs, uint8_t *records, uint32_t rec_cap);

// k_stream.hip
__global__ void k_scan_u64(uint64_t *a, uint32_t n);
__global__ void k_u32_chunk_sums(const uint32_t *a, uint32_t n, uint64_t *partial);
__global__ void k_u32_chunk_apply(const uint32_t *a, uint32_t *out, uint32_t n, const uint64_t *partial);
__global__ void k_unpack_extract(const UnpackJob *jobs, const uint32_t *chunk_job, uint32_t nchunks, uint64_t *state);   // state: nchunks + 1 zeroed words (look-back)
__global__ void k_unpack_wave(const UnpackJob *jobs, const uint32_t *job_ids, uint32_t njobs);   // ... the log streams of small bit blocks: one wave per stream, lanes interleaved, no look-back
__global__ void k_cloud_sums(const CloudJob *jobs, const uint32_t *chunk_job, uint32_t nchunks, uint64_t *partial);
__global__ void k_cloud_apply(const CloudJob *jobs, const uint32_t *chunk_job, uint32_t nchunks, const uint64_t *partial);
__global__ void k_dequant(const DequantJob *jobs, const uint32_t *block_job, uint32_t nblocks);

// k_quant_out.hip (CRTHIP_BIND_QUANTIZED): jobs of up to QOUT_BLOB_MAX vertices by one workgroup each, from an id list (both passes, the values
// re-read through L2); bigger ones - big meshes, clouds - in blocks of QOUT_BLOCK vertices (quant_out.h) from a block -> job map, the range
// by integer atomics into the job's scratch words, then the store.  Measured on one lone job (profiles/quantized_outputs.md): the one-workgroup
// kernel costs 9 us at 1 024 vertices and 4 us more every 1 024, the two launches 13 us whatever the size up to 16 384: it wins at 2 048, loses at 3 072
constexpr uint32_t QOUT_BLOB_MAX = 2304;
__global__ void k_quant_out_blob(const QuantOutJob *jobs, const uint32_t *job_ids, uint32_t njobs);
__global__ void k_quant_range(const QuantOutJob *jobs, const uint32_t *block_job, uint32_t nblocks);
__global__ void k_quant_store(const QuantOutJob *jobs, const uint32_t *block_job, uint32_t nblocks);

// k_tangent.hip (crthip_batch_bind_computed_tangents; tangent.h has the arithmetic): blobs of up to TANGENT_BLOB_MAX vertices (batch_internal.h) by one
// workgroup each, from an id list, with one 3 x int64 accumulator a vertex in `lds_bytes` of dynamic LDS (tangent_blob_lds); bigger ones in blocks of
// TAN_BLOCK faces, then of TAN_BLOCK vertices, from block -> job maps, the sums in the job's zeroed scratch words
__global__ void k_tangent_blob(const TangentJob *jobs, const uint32_t *job_ids, uint32_t njobs);
__global__ void k_tangent_faces(const TangentJob *jobs, const uint32_t *block_job, uint32_t nblocks);
__global__ void k_tangent_vertex(const TangentJob *jobs, const uint32_t *block_job, uint32_t nblocks);
__host__ __device__ inline uint32_t tangent_blob_lds(uint32_t nvert) { return (nvert*24u + 15u) & ~15u; }

// k_meshlet.hip (crthip_batch_bind_meshlets; meshlet.h has the builder): blobs of up to MESHLET_BLOB_SEGS segments (batch_internal.h) by one workgroup
// each, a wave a segment, from an id list, with sizeof(MltWaveMem) of dynamic LDS a wave (launch 64 x the most segments a listed blob has); bigger
// ones a wave a segment from a block -> job map into the job's scratch, then a workgroup a segment moves the pieces
__global__ void k_meshlet_blob(const MeshletJob *jobs, const uint32_t *job_ids, uint32_t njobs);
__global__ void k_meshlet_segments(const MeshletJob *jobs, const uint32_t *block_job, uint32_t nblocks);
__global__ void k_meshlet_place(const MeshletJob *jobs, const uint32_t *block_job, uint32_t nblocks);

// k_meshlet_bounds.hip (crthip_batch_bind_meshlet_bounds; meshlet_bounds.h has the arithmetic): a wave a meshlet, four waves a workgroup, from a
// block -> job map with (capacity + 3)/4 blocks a job; waves at or past the blob's count on the device return
__global__ void k_meshlet_bounds(const MeshletBoundsJob *jobs, const uint32_t *block_job, uint32_t nblocks);

// k_adjacency.hip (crthip_batch_bind_adjacency; adjacency.h has the rule and both partitions): blobs whose lists fit ADJ_BLOB_LDS_MAX by one
// workgroup each from an id list, with adj_blob_lds(nvert, nface) of dynamic LDS (the launch asks for the largest among them); bigger ones
// 256 half-edges a block from a block -> job map, with one workgroup a blob (an id list) for the scan between count and fill
__global__ void k_adjacency_blob(const AdjacencyJob *jobs, const uint32_t *job_ids, uint32_t njobs);
__global__ void k_adjacency_count(const AdjacencyJob *jobs, const uint32_t *block_job, uint32_t nblocks);
__global__ void k_adjacency_offsets(const AdjacencyJob *jobs, const uint32_t *job_ids, uint32_t njobs);
__global__ void k_adjacency_fill(const AdjacencyJob *jobs, const uint32_t *block_job, uint32_t nblocks);
__global__ void k_adjacency_twin(const AdjacencyJob *jobs, const uint32_t *block_job, uint32_t nblocks);

// k_weld.hip (crthip_batch_bind_weld; weld.h has the method and both partitions): blobs whose table fits WELD_BLOB_LDS_MAX by one workgroup each
// from an id list, with weld_slots(nvert)*4 bytes of dynamic LDS (the launch asks for the largest among them); bigger ones 256 vertices a block
// from a block -> job map (insert, lookup) and 256 corners a block from a second one (index: blobs with an index output only)
__global__ void k_weld_blob(const WeldJob *jobs, const uint32_t *job_ids, uint32_t njobs);
__global__ void k_weld_insert(const WeldJob *jobs, const uint32_t *block_job, uint32_t nblocks);
__global__ void k_weld_lookup(const WeldJob *jobs, const uint32_t *block_job, uint32_t nblocks);
__global__ void k_weld_index(const WeldJob *jobs, const uint32_t *block_job, uint32_t nblocks);

// k_lod.hip (crthip_batch_bind_lod; lod.h has the method and both partitions): a job is one level of one blob.  Jobs whose tables fit
// LOD_BLOB_LDS_MAX by one workgroup each from an id list, with 4*max(weld_slots(nvert), weld_slots(nface)) bytes of dynamic LDS (the launch asks
// for the largest among them); bigger ones 256 vertices a block from a block -> job map (insert, lookup), 256 faces a block from a second one
// (faces, keep, scatter) and one workgroup a job from an id list (offsets)
__global__ void k_lod_blob(const LodJob *jobs, const uint32_t *job_ids, uint32_t njobs);
__global__ void k_lod_insert(const LodJob *jobs, const uint32_t *block_job, uint32_t nblocks);
__global__ void k_lod_lookup(const LodJob *jobs, const uint32_t *block_job, uint32_t nblocks);
__global__ void k_lod_faces(const LodJob *jobs, const uint32_t *block_job, uint32_t nblocks);
__global__ void k_lod_keep(const LodJob *jobs, const uint32_t *block_job, uint32_t nblocks);
__global__ void k_lod_offsets(const LodJob *jobs, const uint32_t *job_ids, uint32_t njobs);
__global__ void k_lod_scatter(const LodJob *jobs, const uint32_t *block_job, uint32_t nblocks);

// k_cloud_lod.hip (crthip_batch_bind_cloud_lod; cloud_lod.h has the method and both partitions): a job is one level of one cloud.  Jobs whose
// table fits WELD_BLOB_LDS_MAX by one workgroup each from an id list, with weld_slots(nvert)*4 bytes of dynamic LDS (the launch asks for the
// largest among them); bigger ones 256 vertices a block from a block -> job map (insert, lookup, scatter), one workgroup a job from an id list
// (offsets) and a workgroup a chunk of the capacity from a second map (chunks: jobs with a chunks array only)
__global__ void k_cloud_lod_blob(const CloudLodJob *jobs, const uint32_t *job_ids, uint32_t njobs);
__global__ void k_cloud_lod_insert(const CloudLodJob *jobs, const uint32_t *block_job, uint32_t nblocks);
__global__ void k_cloud_lod_lookup(const CloudLodJob *jobs, const uint32_t *block_job, uint32_t nblocks);
__global__ void k_cloud_lod_offsets(const CloudLodJob *jobs, const uint32_t *job_ids, uint32_t njobs);
__global__ void k_cloud_lod_scatter(const CloudLodJob *jobs, const uint32_t *block_job, uint32_t nblocks);
__global__ void k_cloud_lod_chunks(const CloudLodJob *jobs, const uint32_t *block_job, uint32_t nblocks);

// k_compact.hip (crthip_batch_bind_compact; compact.h has the method and both partitions): a job is one mesh set of one blob.  Sets of up to
// 8 192 vertices and bound faces by one workgroup each from an id list (2 KiB of static LDS); bigger ones 256 corners a block from a block -> job
// map (mark, index), 256 vertices a block from a second map (count, place) and one workgroup a set from an id list (offsets).  k_compact_gather:
// a job is one gather of one set, mesh or cloud, 256 copy units a block from a map of its own
__global__ void k_compact_blob(const CompactJob *jobs, const uint32_t *job_ids, uint32_t njobs);
__global__ void k_compact_mark(const CompactJob *jobs, const uint32_t *block_job, uint32_t nblocks);
__global__ void k_compact_count(const CompactJob *jobs, const uint32_t *block_job, uint32_t nblocks);
__global__ void k_compact_offsets(const CompactJob *jobs, const uint32_t *job_ids, uint32_t njobs);
__global__ void k_compact_place(const CompactJob *jobs, const uint32_t *block_job, uint32_t nblocks);
__global__ void k_compact_index(const CompactJob *jobs, const uint32_t *block_job, uint32_t nblocks);
__global__ void k_compact_gather(const CompactGatherJob *jobs, const uint32_t *block_job, uint32_t nblocks);

// k_bvh.hip (crthip_batch_bind_bvh; bvh.h has the method and both partitions): blobs of up to 4 096 faces by one workgroup each from an id
// list, with bvh_blob_lds_bytes(nface) bytes of dynamic LDS (the launch asks for the largest among them); bigger ones 256 faces a block from a
// block -> job map (boxes, keys, tree, refit), a sort tile a block from a second map (sort_count, sort_scatter: four passes, `pass` says which)
// and one workgroup a blob from an id list (sort_offsets)
__global__ void k_bvh_blob(const BvhJob *jobs, const uint32_t *job_ids, uint32_t njobs);
__global__ void k_bvh_boxes(const BvhJob *jobs, const uint32_t *block_job, uint32_t nblocks);
__global__ void k_bvh_keys(const BvhJob *jobs, const uint32_t *block_job, uint32_t nblocks);
__global__ void k_bvh_sort_count(const BvhJob *jobs, const uint32_t *block_job, uint32_t nblocks, uint32_t pass);
__global__ void k_bvh_sort_offsets(const BvhJob *jobs, const uint32_t *job_ids, uint32_t njobs);
__global__ void k_bvh_sort_scatter(const BvhJob *jobs, const uint32_t *block_job, uint32_t nblocks, uint32_t pass);
__global__ void k_bvh_tree(const BvhJob *jobs, const uint32_t *block_job, uint32_t nblocks);
__global__ void k_bvh_refit(const BvhJob *jobs, const uint32_t *block_job, uint32_t nblocks);

// k_bvh_cast.hip (crthip_bvh_cast; bvh_cast.h has the tests and the walk): a thread a segment, 64 segments a workgroup, through a block_start
// table over the call's sets (njobs entries are read); 16 640 bytes of static LDS hold the 64 traversal stacks
struct CastJob;
__global__ void k_bvh_cast(const CastJob *jobs, const uint32_t *block_start, uint32_t njobs);

// k_bvh_query.hip (crthip_bvh_query; bvh_query.h has the face rules and the walk): a thread a box, 64 boxes a workgroup, through a block_start
// table over the call's sets (njobs entries are read); the cast's 16 640 bytes of static LDS hold the 64 traversal stacks
struct QueryJob;
__global__ void k_bvh_query(const QueryJob *jobs, const uint32_t *block_start, uint32_t njobs);

// k_bvh_closest.hip (crthip_bvh_closest; bvh_closest.h has the wide arithmetic, the face rule and the walk): a thread a point, 64 points a
// workgroup, through a block_start table over the call's sets (njobs entries are read); the cast's 16 640 bytes of static LDS hold the stacks
struct ClosestJob;
__global__ void k_bvh_closest(const ClosestJob *jobs, const uint32_t *block_start, uint32_t njobs);

// k_mesh.hip
__global__ void k_topology(const TopoJob *jobs, const uint32_t *job_ids, uint32_t njobs);
__global__ void k_topology_lds(const TopoJob *jobs, const uint32_t *job_ids, uint32_t njobs);
__global__ void k_topology_lds_big(const TopoJob *jobs, const uint32_t *job_ids, uint32_t njobs);   // the same automaton keeping a progress word (k_mesh.hip)
// k_topology_lds and k_unpack_wave in one grid (single-stream contexts): front_topo_blocks(ntopo) automata first, then xcd_grid(nunpack) K-BIT waves
__host__ __device__ inline uint32_t front_topo_blocks(uint32_t ntopo) { return (ntopo + 7u) & ~7u; }
__global__ void k_front(const TopoJob *jobs, const uint32_t *topo_ids, uint32_t ntopo, const UnpackJob *ujobs, const uint32_t *unpack_ids, uint32_t nunpack);
// ... and the dictionaries of the lane's NEXT batch behind them (crthip_batch_decode_with_next): ndicts more blocks, their growth state carved from
// the automata's dynamic LDS request, which therefore has to be at least TUN_CARRY_GROW_LDS
__global__ void k_front_carry(const TopoJob *jobs, const uint32_t *topo_ids, uint32_t ntopo, const UnpackJob *ujobs, const uint32_t *unpack_ids, uint32_t nunpack,
                              const TunStream *dicts, uint32_t ndicts, TunTable *tables);
constexpr uint32_t TUN_CARRY_GROW_LDS = TUN_ENTRY_CAP*6 + 3*512 + 256;       // sizeof(TunGrow), tun_tables.h
constexpr uint32_t TUN_CARRY_DICTS_MAX = 512;                               // the most dictionaries a k_front grid carries (plan_launch.cpp: carry_args)
constexpr uint32_t TUN_CARRY_GROUP_LDS = 512 + 256 + TUN_TABLE_BYTES;       // TUN_GROUP_LDS, tun_stream.h
// (K-BIT's waves hold the automata's LDS request too: k_front only while that is small)
constexpr uint32_t FRONT_LDS_MAX = 32*1024;
// dynamic LDS bytes k_topology_lds needs for a front of `cap` edges and `nclers` symbols
constexpr uint32_t TOPO_SPLIT_LDS = 256;          // words of the split / vertex-id bit block staged in LDS
// LDS of one blob's CLERS automaton (k_mesh.hip): records of the LIVE front only - a ring for the queued edges, a pool for
// surviving chain ends - plus the DELAY stack and a window of nibble-packed symbols.
inline uint32_t topo_lds_bytes(uint32_t ring, uint32_t pool, uint32_t dcap, uint32_t symwin) {
	return (ring + pool)*16 + ((pool + 7) & ~7u)*2 + ((dcap + 7) & ~7u)*2 + symwin/2 + 8 + 32 + TOPO_SPLIT_LDS*4 + 16;
}
constexpr uint32_t TOPO_SYMWIN_MAX = 8192;
// The queue of a sphere-like mesh peaks near 3*sqrt(nface) (189 for 4 096 faces, 1 497 for 256 000): the RING gets `slots`*sqrt(nface) rounded up to a
// power of two (at least 256, at most `ring_max`) times what the context has learnt (`ring_scale`, a power of two: a torus' queue is ten times a sphere's).
// The POOL is sized on its own (round 5; rounds 2-4 had pool = ring), and the context learns a factor for it too (`pool_q8`, in eighths) from what
// redone blobs report.  What does not fit is redone on the HBM front.
// slots = 8 for a few big meshes (LDS is not contended: leave room), 4 for a batch of many blobs: a 4K-triangle blob then takes 12.5 KB,
// and that it is NOT MORE THAN THE 16 KB of a K-STREAM wave matters more than the size itself: the automaton's workgroups are dispatched
// while the attribute streams' 2 000 waves fill every CU ten to a CU, and a 16 KB hole opens whenever one of those ends - a 22 KB
// request waits for two neighbouring ones (0.237 -> 0.200 ms per C4 batch unpipelined, +5 % pipelined).
// `pool_cap` (0: none): the most pool slots any redone blob has reported (+ an eighth) - a launch's LDS request is its largest blob's, so the factor is
// not applied beyond what the neediest blob seen so far would have needed
inline void topo_lds_geometry(uint32_t nface, uint32_t nclers, uint32_t ring_max, uint32_t ring_scale, uint32_t pool_q8, uint32_t slots,
                              uint32_t &ring, uint32_t &pool, uint32_t &symwin, uint32_t pool_cap = 0) {
	uint32_t want = 256;
	while((uint64_t)want*want < (uint64_t)slots*slots*nface && want < ring_max) want <<= 1;
	const uint32_t base = want;
	while(ring_scale > 1 && want < ring_max) { want <<= 1; ring_scale >>= 1; }
	ring = want;
	// round 6: the BOUNDARY edges share ONE slot (the sink, k_mesh.hip), so the pool holds the DELAYed edges while they wait + that slot: 65 for a C4 blob
	// (222 with a record per BOUNDARY edge), 131 with flipped diagonals, 194 for a Delaunay disc with holes (469), 511 for a holey disc (1 325) - half the
	// ring's base to begin with, times what the context learns from the blobs that outgrow it.
	uint64_t p = std::max<uint64_t>(64, base/2);
	const uint64_t p1 = p;
	p = (p*pool_q8 + 7)/8;
	if(pool_cap && p > pool_cap) p = std::max<uint64_t>(p1, pool_cap);
	p = (p + 63) & ~63ull;                                                        // (whole 16-byte vectors of free-list and DELAY-stack halfwords)
	pool = (uint32_t)std::min<uint64_t>(p, ring_max);
	const uint32_t all = (nclers + 64 + 31) & ~31u;       // whole 16-byte vectors of nibbles (k_mesh.hip: TOPO_FILL_WINDOW)
	symwin = all < TOPO_SYMWIN_MAX ? all : TOPO_SYMWIN_MAX;
}
constexpr uint32_t TOPO_SLOTS_MAX = 4096;       // ring and pool slots of the automaton's LDS form: the planner's and the feedback's `ring_max`
inline uint32_t topo_slots(uint32_t nblobs) { return nblobs >= 32 ? 4u : 8u; }   // ... and their `slots`: a batch of many blobs keeps them small
constexpr uint32_t TOPO_LDS_MAX = 156*1024;     // of the CU's 160 KiB
// k_delta.hip: every K-DELTA job beyond the LDS records below - big meshes, attributes of more than four components - in tiles of DELTA_THREADS
// vertices out of an LDS ring of recent values, one workgroup a job (round 6).  SLICES: the jobs of attributes of more than four components, a slice
// of four each
constexpr uint32_t DELTA_THREADS = 1024;
template <bool SLICES> __global__ void k_delta_tiles(const DeltaJob *jobs, uint32_t njobs);
constexpr uint32_t DELTA_GROUP_MAX = 4;
struct DeltaGroup { uint32_t first, count; };     // DeltaJob entries [first, first + count) of one blob
// k_delta.hip: one workgroup per blob, one wave per attribute (up to four) + one that builds the prediction graph they share: 16-bit values
// relative to vertex 0 (bytes for colours), a 4-byte graph word and one out-of-order window loop.  Records: 2 / 4 / 8 / 8 bytes for 1 / 2 / 3 / 4 int16 components, 4 bytes for up to four colour bytes.
constexpr uint32_t DELTA16_LDS_MAX = 128*1024, DELTA16_NVERT_MAX = 32767;
__host__ __device__ inline uint32_t delta16_rec(uint32_t N, bool is_u8) { return is_u8 ? 4u : N == 1 ? 2u : N == 2 ? 4u : 8u; }
__host__ __device__ inline uint32_t delta16_vbytes(uint32_t nvert, uint32_t N, bool is_u8) { return (nvert*delta16_rec(N, is_u8) + 15u) & ~15u; }
// ... or 32-bit components (a context that met values beyond int16): records of 4 / 8 / 16 / 16 bytes; colours stay four bytes
__host__ __device__ inline uint32_t delta_rec(uint32_t N, bool is_u8, bool wide) { return !wide || is_u8 ? delta16_rec(N, is_u8) : N == 1 ? 4u : N == 2 ? 8u : 16u; }
__host__ __device__ inline uint32_t delta_vbytes(uint32_t nvert, uint32_t N, bool is_u8, bool wide) { return (nvert*delta_rec(N, is_u8, wide) + 15u) & ~15u; }
__host__ __device__ inline bool delta16_eligible(uint32_t nvert, uint32_t N, bool is_u8) { return nvert <= DELTA16_NVERT_MAX && N >= 1 && N <= 4 && (is_u8 || true); }
// graph: 4 bytes a vertex + (unless a three-component int16 attribute of the group lends its spare halfwords) 2 bytes a vertex of `a`
__host__ __device__ inline uint32_t delta16_graph_lds(uint32_t nvert, bool a_embedded) {
	return ((4u*nvert + 15u) & ~15u) + (a_embedded ? 0u : ((2u*nvert + 15u) & ~15u)) + 16u;
}
__global__ void k_delta_lds16(const DeltaJob *jobs, const DeltaGroup *groups, uint32_t ngroups);
// ... with the stream groups of the lane's NEXT batch behind this batch's blobs: block ranges [blobs | stream groups], the carried groups' dictionary
// copy at the head of the dynamic block (the launch asks for at least TUN_CARRY_GROUP_LDS)
__global__ void k_delta_lds16_carry(const DeltaJob *jobs, const DeltaGroup *groups, uint32_t ngroups, const TunStream *streams, const uint32_t *ids,
                                    const TunGroup *tun_groups, uint32_t ntun_groups, const TunTable *tables);

// k_normal.hip
__global__ void k_normal_diff(const NormalJob *jobs, const uint32_t *block_job, const uint32_t *block_first, uint32_t nblocks);
__global__ void k_normal_faces(const NormalJob *jobs, const uint32_t *block_job, const uint32_t *block_first, uint32_t nblocks,
                               float *facen, uint32_t *cnt, uint32_t *bnd);
__global__ void k_normal_fill(const NormalJob *jobs, const uint32_t *block_job, const uint32_t *block_first, uint32_t nblocks,
                              const uint32_t *start, uint32_t *cursor, uint32_t *adj);
__global__ void k_normal_flags(const NormalJob *jobs, const uint32_t *block_job, const uint32_t *block_first, uint32_t nblocks,
                               const uint32_t *bnd, uint32_t *flag);
__global__ void k_normal_vertex(const NormalJob *jobs, const uint32_t *block_job, const uint32_t *block_first, uint32_t nblocks,
                                const float *facen, const uint32_t *start, const uint32_t *cnt, const uint32_t *adj,
                                const uint32_t *flag, const uint32_t *slot);

// <false>: stored ESTIMATED / BORDER normals; <true>: jobs of prediction 3 (COMPUTED: crthip_batch_bind_computed_normals), in the same LDS layout
template <bool COMPUTED> __global__ void k_normal_blob(const NormalJob *jobs, const uint32_t *job_ids, uint32_t njobs, uint32_t lds_bytes);
// (head: cursors u16 | flag bitmap u32 | its prefix counts u16; then the boundary XORs u32 per vertex, later the adjacency u16 per corner)
__host__ __device__ inline uint32_t normal_blob_lds_head(uint32_t nvert) { const uint32_t ndw = 2*((nvert + 63)/64); return (((nvert + 2) & ~1u)*2 + ndw*4 + ndw*2 + 15u) & ~15u; }
__host__ __device__ inline uint32_t normal_blob_lds(uint32_t nvert, uint32_t nface) { const uint32_t adj = (3*nface*2 + 15) & ~15u, bnd = nvert*4; return normal_blob_lds_head(nvert) + (adj > bnd ? adj : bnd) + 64; }
constexpr uint32_t NORMAL_LDS_MAX = 150*1024;
// with the blob's face normals kept in LDS too (3 x f32 per face, behind the layout above): small blobs only
__host__ __device__ inline uint32_t normal_blob_lds_fn(uint32_t nvert, uint32_t nface) { return ((normal_blob_lds(nvert, nface) + 15u) & ~15u) + 12u*nface; }
constexpr uint32_t NORMAL_FN_LDS_MAX = 100*1024;


// k_encode.hip
__global__ void k_enc_hist(const EncChunk *chunks, uint32_t nchunks, uint32_t *counts);
__global__ void k_enc_pack(const PackJob *jobs, uint32_t njobs);
__global__ void k_enc_tun_parse(const EncStream *streams, uint32_t nstreams, uint32_t trie_lds_entries);
// probabilities in std::sort's order + the 256-word dictionary of every stream (one wave each), then the encoding trie of the
// streams listed in ids[] (built in LDS, at most trie_cap entries, written to streams[j].trie; streams[j].ntrie = its size,
// ~0u if it did not fit)
__global__ void k_enc_quantize(QuantJob job);           // float / byte attribute -> quantised integers, elementwise
__global__ void k_enc_tables(const uint32_t *counts, const uint32_t *sizes, uint32_t nstreams, EncTab *tabs);
__global__ void k_enc_trie(const EncTab *tabs, const uint32_t *ids, EncStream *streams, uint32_t nids, uint32_t trie_cap);
inline uint32_t enc_parse_lds(uint32_t trie_entries) { return 768 + ENC_STAGE + ENC_STAGE_PAD + 2*((trie_entries + 7) & ~7u); }
constexpr uint32_t ENC_TRIE_LDS_MAX = 24*1024;         // entries (48 KiB) of trie kept in LDS at most; bigger tries are walked in L2
__global__ void k_enc_gather(const CopyJob *jobs, uint32_t njobs);

// k_encode_batch.hip (crthip_encode_batch).  block_start[j]: the first workgroup of job j (njobs + 1 entries)
__global__ void k_enc_quantize_batch(const QuantJob *jobs, const uint32_t *block_start, uint32_t njobs);
__global__ void k_enc_corners(const EstJob *jobs, const uint32_t *block_start, uint32_t njobs, uint32_t *keys, uint32_t *vals);
__global__ void k_enc_est_normal(const EstJob *jobs, const uint32_t *block_start, uint32_t njobs, const uint32_t *keys, const uint32_t *vals,
                                 uint32_t ncorners, const uint32_t *faces);
__global__ void k_enc_delta(const DeltaEncJob *jobs, const uint32_t *block_start, uint32_t njobs);
__global__ void k_enc_zmin(ZJob job);
__global__ void k_enc_zkeys(ZJob job);
__global__ void k_enc_zflag(ZJob job);
// LSD radix sort of (u32 or u64 key, u32 value) records by the 8 key bits at `shift`: stable.  hist: 256 x nblocks counts, digit-major
template <typename K> __global__ void k_enc_rs_hist(const K *keys, uint32_t n, uint32_t shift, uint32_t *hist);
__global__ void k_enc_rs_scan(uint32_t *hist, uint32_t len);
template <typename K> __global__ void k_enc_rs_scatter(const K *keys, const uint32_t *vals, K *keys_out, uint32_t *vals_out, uint32_t n, uint32_t shift,
                                                       const uint32_t *hist);

// k_encode_topo.hip (crthip_ctx_set_encode_topology): the stages of enc_topology.h, one workgroup of ETOPO_THREADS per mesh.
// k_enc_topo_walk<true> takes the state image's bytes (enc_topo_state_bytes<uint16_t>) as dynamic LDS, up to ETOPO_LDS_MAX
struct EncTopoJob;
constexpr uint32_t ENC_TOPO_LDS_MAX = 156*1024;       // = ETOPO_LDS_MAX (enc_topology.h), of the CU's 160 KiB
__global__ void k_enc_topo_compact(const EncTopoJob *jobs, uint32_t njobs);
__global__ void k_enc_topo_pair(const EncTopoJob *jobs, uint32_t njobs);
template <bool LDS> __global__ void k_enc_topo_walk(const EncTopoJob *jobs, const uint32_t *ids, uint32_t nids);

// k_encode_check.hip (crthip_encode_batch_resident): index range, bounding boxes and first-edge sums of arrays in device memory
// (enc_input_check.h); workgroups of EIN_THREADS from a job table, then one wave per item with a box
struct EncInputJob;
__global__ void k_enc_input_check(const EncInputJob *jobs, const uint32_t *block_start, uint32_t njobs);
__global__ void k_enc_input_reduce(const EncInputJob *jobs, const uint32_t *ids, uint32_t nids);


// k_encode_splice.hip (crthip_encode_batch_to_device): the containers' pieces into the caller's device arena (enc_splice.h); one wave per
// tile of ESP_TILE destination bytes, tile_start[j]: the first tile of job j (njobs + 1 entries)
struct SpliceJob;
__global__ void k_enc_splice(const SpliceJob *jobs, const uint32_t *tile_start, uint32_t njobs);

} // namespace corto_hip
