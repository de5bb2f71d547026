// device_plan.h — POD descriptors shared by the host planner (batch.cpp) and the HIP kernels.
// All pointers are DEVICE addresses.  One array of each job type per batch, uploaded in one H2D copy.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdlib>

namespace corto_hip {

constexpr uint32_t TUN_TABLE_BYTES = 8192 + 1024;  // reference buffer is 8192 B (src/tunstall.cpp:137); +3 B padding per word
constexpr uint32_t TUN_ENTRY_CAP = 768;            // creation-order entries; the reference reaches <= 510
constexpr uint32_t CHUNK = 1024;                   // elements per scan chunk (256 threads x 4)

// Decode table of one Tunstall stream as the decode kernel wants it (K-TAB output)
struct TunTable {
	uint16_t off[256];             // word start in bytes[]            (Tunstall::index)
	uint8_t len[256];              // word length                      (Tunstall::lengths)
	uint32_t used;                 // bytes of bytes[] any word reaches
	uint32_t maxlen;               // longest word
	uint32_t pad[2];
	uint8_t bytes[TUN_TABLE_BYTES];
};

struct TunStream {
	const uint8_t *src;            // codewords
	uint8_t *dst;                  // decoded symbols
	const uint8_t *probs;          // nsym x (symbol, probability)
	uint32_t csize, size, nsym;
	uint32_t table;                // TunTable slot
	uint32_t chunk0;               // first entry of this stream in the chunk arrays (long streams)
	uint32_t nchunks;
	uint32_t chunk_codes;          // codewords per chunk (= per K-TUN workgroup), a multiple of 256*cpl
	uint32_t cpl;                  // staged decode: codewords per lane per step (8, 4, 2 or 1)
	uint32_t dict;                 // k_tun_stream_grouped: TunTable slot of the dictionary this stream decodes from
	uint32_t pad_;
};

// Chunk geometry of one stream, from its mean word length size/csize (both are in the stream header): workgroups are
// balanced by OUTPUT bytes (a two-symbol dictionary expands 60x, a flat one 2x), and a wave's step of 64*cpl codewords
// is sized so that its decoded bytes fit the wave's LDS window (k_tunstall.hip).
constexpr uint32_t TUN_CHUNK_CODES = 32768;   // largest chunk
inline void tun_pick_geometry(TunStream &t) {
	const uint32_t avg = t.csize ? (uint32_t)(((uint64_t)t.size + t.csize - 1)/t.csize) : 1;
	t.cpl = avg <= 8 ? 8 : avg <= 16 ? 4 : avg <= 32 ? 2 : 1;
	uint32_t codes = TUN_CHUNK_CODES;
	while(codes > 256*t.cpl && (uint64_t)codes*avg > 256*1024) codes >>= 1;   // a wave's quarter chunk stays whole steps of 64*cpl
	t.chunk_codes = codes;
	t.nchunks = (t.csize + codes - 1)/codes;
}

// streams [first, first + count) of the launch's by-dictionary order (an index array): all of one dictionary, decoded by one workgroup
struct TunGroup { uint32_t first, count; };
constexpr uint32_t TUN_GROUP_MAX = 8;

struct FillJob { uint8_t *dst; uint32_t size; uint32_t value; };

// CLERS automaton input/output of one mesh blob (src/decoder.cpp:204-358)
struct TopoJob {
	const uint8_t *clers;
	const uint32_t *split_words;
	const uint32_t *group_end;
	void *faces;                   // nface*3 u32 or u16
	uint32_t *pred;                // nvert*3
	uint4 *front_a;                // (v0, v1, v2, deleted)
	uint2 *front_b;                // (prev, next)
	uint32_t *order;               // FIFO of edge ids
	uint32_t *delayed;             // LIFO of edge ids
	int32_t *status;
	int32_t *flags;                // bit 0: the LDS path ran out of edge slots and the blob was redone on the HBM front
	uint32_t nclers, split_nwords, ngroups;
	uint32_t nvert, nface, front_cap, faces_u16;
	uint32_t opts;                 // TOPO_OPT_*
	// LDS path (k_mesh.hip): ring of queued-edge records (a power of two; 0: not eligible), pool of surviving-edge records,
	// DELAY stack entries, symbols in the LDS window (a multiple of 8)
	uint32_t lds_ring, lds_pool, lds_delayed_cap, lds_symwin;
};
// TopoJob.opts, bit 1: the automaton keeps a PROGRESS WORD for a consumer that runs BESIDE it (k_delta_tiles on a lone context's second
// stream) - the number of vertices whose prediction triple has been written and has arrived (published every 4 096 vertices and at every slide of the
// symbol window), 0xFFFFFFFF when it is done.  The word sits 16 bytes in front of the triples (zeroed by the host before the launch): no pointer of its
// own - the automaton's ISA block has no scalar register to spare for one (a TopoJob eight bytes longer cost the C4 batch's automata 3 %).
constexpr uint32_t TOPO_OPT_PROGRESS = 2u;
constexpr uint32_t TOPO_PROGRESS_BYTES = 16u;

// one log stream to turn into values (include/corto/cstream.h:294-360)
struct UnpackJob {
	const uint8_t *logs;
	const uint32_t *words;
	void *out;                     // int32*, uint8* or int16*: out_kind
	uint32_t count;                // logs in the stream
	uint32_t nwords;
	uint32_t out_limit;            // never write element index >= out_limit (nvert)
	uint32_t chunk0;               // first chunk of this job in the chunk arrays
	uint32_t chain_chunk0;         // first chunk of the bit block this job shares (component-major chaining); k_unpack_wave: the first JOB of the bit block
	uint16_t fields;               // ARRAY: N fields per log; VALUES: 1
	uint16_t stride;               // output elements per vertex
	uint16_t comp;                 // VALUES: component
	uint8_t mode;                  // 0 ARRAY, 1 VALUES
	uint8_t out_kind;              // UNPACK_OUT_*
};
// UNPACK_OUT_I16: k_unpack_wave only - a stream whose table holds no width above 16 bits, read by k_delta_lds16 / k_normal_blob
enum : uint8_t { UNPACK_OUT_I32 = 0, UNPACK_OUT_U8 = 1, UNPACK_OUT_I16 = 2 };

constexpr uint32_t UNPACK_WAVE_MAX_LOGS = 16384;   // bit blocks of at most this many logs (all streams together): one wave per stream (k_unpack_wave); else chunks of 1 024 with look-back

// parallelogram / first-neighbour delta over a mesh (include/corto/vertex_attribute.h:160-176,
// src/normal_attribute.cpp:193-201)
struct DeltaJob {
	void *values;                  // int32* or uint8*, stride N
	const uint32_t *pred;
	uint8_t *progress;             // k_delta_tiles: the automaton's progress word (TopoJob.opts: TOPO_OPT_PROGRESS) or null
	uint32_t nvert, N;
	uint8_t parallelogram, is_u8;
	uint8_t in_i16;                // `values` holds the raw deltas as int16 (K-BIT's UNPACK_OUT_I16), packed at the front of the buffer the results go to
	uint8_t wide;                  // k_delta_lds16 keeps 32-bit records in LDS (the whole group says the same)
	// k_delta_lds16 finishes the attribute on its way out of LDS (no k_dequant launch, no second trip through HBM):
	uint32_t deq;                  // 0: write the integers back; 1: generic, packed: (float)v*q in place (vertex_attribute.h:190-193);
	                               // 2: colour: YCC -> RGB x qc into `out` (color_attribute.cpp:76-95)
	float q;
	uint32_t qc[4];
	uint32_t first;                // k_delta_tiles: the first component of this job - 0, or a slice of four of an attribute of more (records of N)
	void *out;                     // colour destination
	uint32_t out_components, out_stride;
	int32_t *flags;                // k_delta_lds16: set to 1 when the attribute's values relative to vertex 0 left int16 and were redone in HBM
	uint32_t rounds;               // the round loop from vertex 1 (test hook: $CORTO_DELTA_ROUNDS)
	uint32_t status_back;          // k_delta_tiles: words from the blob's status word forward to `flags`
};

// point-cloud running sum, one job per (blob, attribute) (vertex_attribute.h:177-181, normal_attribute.cpp:202-207)
struct CloudJob {
	void *values;
	uint32_t nvert, N;
	uint32_t chunk0;               // N * ceil(nvert/CHUNK) chunks: component-major
	uint8_t is_u8, pad[3];
};

struct NormalJob {
	int32_t *diffs;                // 2 ints per (corrected) vertex
	void *out;                     // nvert*3 f32 or i16
	const int32_t *position;       // delta-decoded integer positions (3 per vertex), ESTIMATED/BORDER only
	const void *faces;             // ESTIMATED/BORDER only: u32 or, with faces_u16, u16 triples
	uint32_t nvert, nface, ndiffs;
	uint32_t vbase, fbase;         // offsets into the batch-wide per-vertex / per-face scratch arrays
	int32_t unit;                  // (int)q
	uint8_t prediction, out_i16, faces_u16, fused;   // prediction: 0 DIFF, 1 ESTIMATED, 2 BORDER as stored; 3 COMPUTED: no stored attribute, no diffs (crthip_batch_bind_computed_normals)
	                                                 // fused: handled by k_normal_blob<false> / <true> (whole pipeline in one workgroup)
	int32_t *status;
	uint32_t out_stride;           // bytes from one vertex's normal to the next (12 or 6 when packed)
	// k_normal_blob is the last reader of the integer positions and turns them into floats itself (no k_dequant launch):
	uint32_t pos_stride;           // bytes from one vertex to the next in pos_out (12 = packed, in place when pos_out == position)
	void *pos_out;                 // null: leave the positions alone
	float pos_q;
	uint32_t diffs_i16;            // k_normal_blob: `diffs` holds int16 pairs (K-BIT's UNPACK_OUT_I16)
	float *fn_scratch;             // k_normal_blob without its face normals in LDS: 3 floats per face in HBM scratch (null: recompute them per incident vertex)
};

struct DequantJob {
	void *buffer;                  // destination (generic, packed: the int32 values are here already and turn into floats in place)
	const uint8_t *src;            // colour: delta-decoded N-component bytes; generic with a stride: the int32 values (packed scratch)
	float q;
	uint32_t nvert, N, out_components;
	uint32_t qc[4];
	uint32_t block0;               // first block of this job in the block->job map
	uint8_t is_color;
	uint8_t format;                // generic attributes: the CRTHIP_FMT_* of `buffer` (FLOAT: (float)v*q; the integer formats and DOUBLE: upstream's
	                               // in-place "*= q" through a pointer of that type, vertex_attribute.h:195-228 - k_dequant restates what the compiled reference does)
	uint8_t pad[2];
	uint32_t stride;               // bytes from one vertex to the next in `buffer`; 0 = packed
	uint32_t pad2;
};

// a generic attribute bound with CRTHIP_BIND_QUANTIZED (k_quant_out.hip, quant_out.h): the delta-decoded integers -> uint16 relative to the
// per-component minimum, and the record that takes them back
struct QuantOutRecord;                                   // = crthip_quant_transform (include/corto_hip.h), 48 bytes
struct QuantOutJob {
	const int32_t *values;         // nvert*N int32, packed (scratch)
	void *buffer;                  // the caller's uint16 destination
	QuantOutRecord *rec_host;      // the record in the batch's pinned status block
	QuantOutRecord *rec_dev;       // ... and in the caller's device array (crthip_batch_bind_quant_transforms), or null
	int32_t *status;               // the blob's status word
	uint32_t *range;               // k_quant_range / k_quant_store: eight words of scratch, min | max a component (seeded by FillJobs), else null
	uint32_t stride;               // bytes from one vertex to the next in `buffer`; 0 = packed
	uint32_t nvert, N;
	uint32_t block0;               // first block of this job in the block->job map (jobs beyond QOUT_BLOB_MAX)
	float q;
	uint32_t pad;
};

// a blob bound with crthip_batch_bind_computed_tangents (k_tangent.hip, tangent.h): the integer positions and uvs, the index and the blob's final
// normals -> a tangent and its handedness a vertex
struct TangentJob {
	const int32_t *position, *uv;  // delta-decoded integers, packed: the caller's packed buffer before k_dequant, or scratch
	const void *faces;             // u32 or, with faces_u16, u16 triples
	const void *normal;            // the normal's bound buffer (stored or computed)
	void *out;                     // 4 f32 or 4 i16 a vertex
	uint64_t *acc;                 // tangent_faces / tangent_vertex: 6 x int64 a vertex of zeroed scratch (T | B), else null
	uint32_t nvert, nface;
	uint32_t normal_stride, out_stride;   // bytes from one vertex to the next (never 0 here)
	uint32_t fblock0, vblock0;     // first block of this job in the face / vertex block->job maps (jobs beyond TANGENT_BLOB_MAX)
	uint8_t faces_u16, normal_i16, out_i16, pad[5];
};

// a blob bound with crthip_batch_bind_meshlets (k_meshlet.hip, meshlet.h): the index and the host's segment table -> the caller's three arrays
// and the blob's record.  A blob of one segment is written in place; the others go through `scratch` (mlt_scratch_layout) and are moved
struct MeshletJob {
	const void *faces;             // u32 or, with faces_u16, u16 triples: the caller's index, or scratch
	const void *segs;              // nseg MltSeg (in aux_u32; a byte offset into it until upload)
	void *meshlets, *vertices, *triangles;   // the binding's arrays
	uint8_t *scratch;              // provisional arrays and a count a segment; null for a blob of one segment
	void *rec_host, *rec_dev;      // crthip_meshlet_counts: the pinned status block's, and the binding's optional device copy
	uint32_t nface, nseg, max_vertices, max_triangles;
	uint32_t sc_vertices, sc_triangles, sc_counts;   // byte offsets of scratch's parts (its meshlet records are at 0)
	uint32_t block0;               // first block of this job in the block -> job map (meshlet_segments, meshlet_place)
	uint8_t faces_u16, pad[7];
};

// a blob bound with crthip_batch_bind_meshlet_bounds (k_meshlet_bounds.hip, meshlet_bounds.h): the integer positions and the meshlet binding's final
// arrays -> a record a meshlet.  The grid is sized by `capacity`, the bound; the blob's count is read on the device
struct MeshletBoundsJob {
	const int32_t *position;       // nvert x 3 delta-decoded integers, packed: the caller's FLOAT buffer in front of k_dequant, or scratch
	const void *meshlets, *vertices, *triangles;   // the meshlet binding's arrays, final behind the meshlet kernels
	const void *counts;            // the blob's crthip_meshlet_counts in DEVICE memory: MeshletJob::rec_dev
	void *out;                     // crthip_meshlet_bounds records
	uint32_t nvert, capacity;      // capacity: crthip_meshlet_bound's .meshlets (the records the caller's array has at least)
	uint32_t block0;               // first block of this job in the block -> job map
	uint32_t pad;
};

// a blob bound with crthip_batch_bind_adjacency (k_adjacency.hip, adjacency.h): the index -> the caller's twin array and the blob's record.  A
// blob whose lists fit LDS (adj_in_blob) needs nothing else; the others keep their ends and entries in scratch
struct AdjacencyJob {
	const void *index;             // u32 or, with index_u16, u16 triples: the caller's index, or scratch
	uint32_t *twin;                // the binding's 3*nface words
	void *counts;                  // crthip_adjacency_counts in DEVICE memory: the binding's, or (bigger blobs only) scratch; null: none wanted
	uint32_t *ends, *list;         // bigger blobs: nvert + 1 words zeroed by a FillJob, and 3*nface entries
	uint32_t nface, nvert;
	uint32_t block0;               // first block of this job in the block -> job map (adjacency_count, _fill, _twin)
	uint8_t index_u16, pad[3];
};

// a blob bound with crthip_batch_bind_weld (k_weld.hip, weld.h): the integer positions and the index -> the caller's remap, its welded index and
// the blob's record.  A blob whose table fits LDS (weld_in_blob) needs nothing else; the others keep their table in scratch
struct WeldJob {
	const int32_t *position;       // nvert x 3 int32 as K-DELTA leaves them: the caller's packed buffer, or scratch
	const void *index;             // u32 or, with index_u16, u16 triples: the caller's index, or scratch
	uint32_t *remap;               // the binding's nvert words
	uint32_t *windex;              // the binding's 3*nface words; null: no welded index
	void *counts;                  // crthip_weld_counts in DEVICE memory: the binding's, or (bigger blobs only) scratch; null: none wanted
	uint32_t *table;               // bigger blobs: weld_slots(nvert) words zeroed by a FillJob
	uint32_t nface, nvert;
	uint32_t vblock0, cblock0;     // first block of this job in the two block -> job maps (weld_insert and _lookup; weld_index)
	uint8_t index_u16, pad[7];
};

// one LEVEL of a blob bound with crthip_batch_bind_lod (k_lod.hip, lod.h): the integer positions and the index -> the level's remap, its index of
// kept faces and its record.  The clustered triples are in scratch for every job; a job beyond lod_in_blob keeps its two tables and its block
// counts there too
struct LodJob {
	const int32_t *position;       // nvert x 3 int32 as K-DELTA leaves them: the caller's packed buffer, or scratch
	const void *index;             // u32 or, with index_u16, u16 triples: the caller's index, or scratch
	uint32_t *remap;               // the level's nvert words
	uint32_t *lod_index;           // the level's index: 3*faces words are written
	void *counts;                  // crthip_lod_counts in DEVICE memory: the level's, or (bigger jobs only) scratch; null: none wanted
	uint32_t *triples;             // scratch: 3*nface words
	uint32_t *vtable, *ftable;     // bigger jobs: weld_slots(nvert) and weld_slots(nface) words zeroed by one FillJob
	uint32_t *blocks;              // bigger jobs: a word a block of LOD_BLOCK faces - its kept count, then its base
	uint32_t nface, nvert;
	uint32_t vblock0, fblock0;     // first block of this job in the two block -> job maps (lod_insert and _lookup; lod_faces, _keep and _scatter)
	uint32_t shift;
	uint8_t index_u16, pad[3];
};

// one LEVEL of a cloud bound with crthip_batch_bind_cloud_lod (k_cloud_lod.hip, cloud_lod.h): the integer positions -> the level's remap, its kept
// points, their weights, a box a chunk of them and its record.  A job within weld_in_blob needs nothing else; the others keep their table, their
// weight words and their block counts in scratch
struct CloudLodJob {
	const int32_t *position;       // nvert x 3 int32 as k_cloud_apply leaves them: the caller's packed buffer, or scratch
	uint32_t *remap;               // the level's nvert words
	uint32_t *points;              // the level's kept points: `cells` words are written
	uint32_t *weight;              // ... and their weights; null: none wanted
	void *chunks;                  // crthip_cloud_chunk records; null: none wanted
	void *counts;                  // crthip_cloud_lod_counts in DEVICE memory: the level's, or (bigger jobs only) scratch; null: none wanted
	uint32_t *table, *wacc;        // bigger jobs: weld_slots(nvert) words and nvert weight words, one range zeroed by one FillJob
	uint32_t *blocks;              // bigger jobs: a word a block of LOD_BLOCK vertices - its kept count, then its base
	uint32_t nvert, shift;
	uint32_t chunk_points;         // K (read only with chunks)
	uint32_t vblock0, cblock0;     // first block of this job in the two block -> job maps (cloud_lod_insert, _lookup and _scatter; cloud_lod_chunks)
	uint32_t pad;
};
static_assert(sizeof(CloudLodJob) == 96, "decode job layout");

// one MESH SET of a blob bound with crthip_batch_bind_compact (k_compact.hip, compact.h): an id list -> the set's newid, order, renumbered index
// and record.  A set within compact_in_blob needs nothing else; the others keep their mask and their block counts in scratch
struct CompactJob {
	const void *src;               // the id list, u32 or, with src_u16, u16: the blob's index (the caller's, or scratch), the weld's index, a level's index
	const uint32_t *src_rec;       // the record whose word 1 is the list's face count (a level's crthip_lod_counts: the caller's, or scratch); null: nface
	uint32_t *newid;               // nvert words: the set's, or (bigger sets with an index) scratch; null: none wanted
	uint32_t *order;               // the set's, or (a set with gathers) scratch: min(vcap, nvert) words at most are written; null: none wanted
	uint32_t *index;               // the set's: min(3*F, icap) words are written; null: none wanted
	void *counts;                  // crthip_compact_counts in DEVICE memory: the set's, or scratch
	uint32_t *mask, *blocks;       // bigger sets: ceil(nvert/32) words zeroed by one FillJob; a word a block of 256 vertices - its count, then its base
	uint32_t nface, nvert;         // nface: the BOUND the grids and the source array were sized from
	uint32_t vcap, icap;           // vertex_capacity, index_capacity
	uint32_t vblock0, cblock0;     // first block of this job in the two block -> job maps (compact_count and _place; compact_mark and _index)
	uint8_t src_u16, clip_v, pad[6];   // clip_v: the set has an order or a gather
};
// one GATHER of a set (k_compact_gather): E bytes of vertex order[j] of a final vertex output -> record j of a compact array
struct CompactGatherJob {
	const uint8_t *src;            // the source's own buffer, as bound
	uint8_t *dst;
	const uint32_t *order;         // the set's order (the caller's, or scratch); a cloud set's: its level's points
	const uint32_t *count_rec;     // the record whose word 1 is `used`: the set's; a cloud set's: its level's (the caller's, or scratch)
	void *cloud_rec;               // a cloud set's first gather: the set's record, which this kernel stores; else null
	uint32_t E, sstride, dstride;  // element bytes (0: a cloud set without gathers - the record alone) and the two strides as byte distances
	uint32_t unit;                 // compact_unit's choice
	uint32_t vcap, nvert;
	uint32_t block0;               // first block of this job in the block -> job map
	uint8_t clip_v, pad[3];
};
static_assert(sizeof(CompactJob) == 96 && sizeof(CompactGatherJob) == 72, "decode job layout");

// a blob bound with crthip_batch_bind_bvh (k_bvh.hip, bvh.h): the integer positions and the index -> the caller's nodes, its parent and order
// arrays and the blob's record.  A blob within bvh_in_blob needs nothing else; the others keep bvh_scratch_layout's block in scratch
struct BvhJob {
	const int32_t *position;       // nvert*3 delta-decoded integers (the caller's buffer or scratch)
	const void *index;             // nface*3 u32 or, with index_u16, u16 (the caller's buffer or scratch)
	void *nodes;                   // the binding's crthip_bvh_node array: 2*nface - 1 records are written
	uint32_t *parent;              // 2*nface - 1 words: the binding's, or (bigger blobs only) scratch; null: none wanted
	uint32_t *order;               // the binding's nface words; null: none wanted
	void *counts;                  // crthip_bvh_counts in DEVICE memory: the binding's; null: none wanted
	uint8_t *scratch;              // bigger blobs: the block, whose first zero_bytes (the extent, the arrival counters) one FillJob zeroes
	uint32_t nface, nvert;
	uint32_t fblock0, tblock0;     // first block of this job in the two block -> job maps (256 faces a block; a sort tile a block)
	uint8_t index_u16, pad[7];
};
static_assert(sizeof(BvhJob) == 80, "decode job layout");

// the layout the kernels read, pinned (TopoJob's size is performance-critical: TOPO_OPT_PROGRESS above)
static_assert(sizeof(TunStream) == 64 && sizeof(FillJob) == 16 && sizeof(TopoJob) == 136 && sizeof(UnpackJob) == 56 && sizeof(DeltaJob) == 96 &&
              sizeof(CloudJob) == 24 && sizeof(NormalJob) == 104 && sizeof(DequantJob) == 64 && sizeof(QuantOutJob) == 72 && sizeof(TangentJob) == 80 &&
              sizeof(MeshletJob) == 104 && sizeof(MeshletBoundsJob) == 64 && sizeof(AdjacencyJob) == 56 && sizeof(WeldJob) == 72 && sizeof(LodJob) == 96, "decode job layout");
static_assert(offsetof(TopoJob, opts) == 116 && offsetof(UnpackJob, out_kind) == 51 && offsetof(NormalJob, faces_u16) == 58, "decode job layout");
static_assert(offsetof(DeltaJob, in_i16) == 34 && offsetof(DeltaJob, wide) == 35 && offsetof(DeltaJob, rounds) == 88 &&
              offsetof(DeltaJob, status_back) == 92, "decode job layout");

// ---- encoder stages (k_encode.hip, encode_gpu.cpp) ----
// a piece of a source stream for the byte histogram (src/tunstall.cpp:83-115)
struct EncChunk { const uint8_t *src; uint32_t size, stream; };

// one stream for the Tunstall coder (src/tunstall.cpp:384-428): the host-made encoder tables and where the codewords go
struct EncStream {
	const uint8_t *src;            // size symbols
	uint8_t *dst;                  // room for size + 64 codewords
	int16_t *trie;                 // the reference's 2-symbol-step trie, levels of nsym*nsym entries: >= 0 codeword, < 0 minus the next level's number
	                               // (made on the host, or by k_enc_trie in place: then ntrie is what that kernel wrote)
	const uint8_t *remap;          // 256: symbol -> index
	const uint16_t *lengths;       // 256: word length by codeword
	uint32_t *csize;               // out: number of codewords
	uint32_t size, nsym, ntrie, pad;
};
// one attribute to quantise (k_enc_quantize): include/corto/vertex_attribute.h:79-128, src/normal_attribute.cpp:61-111,
// src/color_attribute.cpp:23-70
// kinds: GENERIC from float, int32 / int16 / int8 (QK_INT, element format in `format`) or double input, NORMAL, COLOR
enum : uint32_t { QK_FLOAT = 0, QK_NORMAL = 1, QK_COLOR = 2, QK_INT = 3, QK_DOUBLE = 4 };
struct QuantJob {
	const void *in;                // FLOAT: count floats; INT: count elements of `format`; DOUBLE: count doubles (8-byte aligned);
	                               // NORMAL: count x 3 floats; COLOR: count x N bytes
	void *out;                     // GENERIC: count int32; NORMAL: count x 2 int32 (octahedral); COLOR: count x N bytes (YCC)
	uint32_t count, kind, N;       // kind: QK_*
	float q;                       // GENERIC: the step
	int32_t unit;                  // NORMAL: (int)q
	uint32_t qc[4];                // COLOR: per-channel divisors
	uint32_t format;               // QK_INT: CRTHIP_FMT_INT32 / INT16 / INT8
	// crthip_mesh_layout (all zero: the packed arrays above, read as before)
	uint32_t stride;               // bytes from one vertex's elements to the next's; 0: packed
	uint32_t comps;                // FLOAT / INT / DOUBLE with a stride or an origin: elements a vertex has (count = vertices * comps)
	uint32_t flags;                // QF_*
	float origin[3];               // QF_ORIGIN (FLOAT, comps == 3): x - origin[component], upstream's coords[i] = input[i] - o
};
enum : uint32_t { QF_ORIGIN = 1, QF_NORMAL_I16 = 2 };   // QF_NORMAL_I16: NORMAL reads int16 triples, (float)v/32767.0f (src/encoder.cpp:151-158)
// what k_enc_tables leaves per stream for the Tunstall coder: the block header (probabilities) and the encoder tables
struct EncTab {
	uint32_t nsym;                 // symbols that occur (0: empty stream, 1: no payload)
	uint32_t level_bound;          // upper bound on the levels of the stream's trie: 1 + sum over words of (length - 1)/2
	uint32_t used;                 // dictionary bytes
	uint32_t pad;
	uint8_t probs[512];            // nsym x (symbol, probability) in the reference's order (std::sort of src/tunstall.cpp:111-112)
	uint8_t remap[256];            // symbol -> index in probs
	uint16_t lengths[256];         // word lengths by codeword
	uint16_t index[256];           // word starts in words[]
	uint8_t words[TUN_TABLE_BYTES];
};
// one value array for the bit-width + bit-packing kernel (include/corto/cstream.h:115-164)
struct PackJob {
	const void *values;            // count*N int32 (ARRAY, VALUES_I32) or int8 (VALUES_I8)
	uint8_t *logs;                 // ARRAY: count bytes; VALUES: N arrays of count bytes, component-major
	uint32_t *words;               // MSB-first bit stream (src/bitstream.cpp:86-101)
	uint32_t *nwords;              // out
	uint32_t count, N, kind, pad;  // kind: CRTHIP_ENC_ARRAY / VALUES_I32 / VALUES_I8
};
constexpr uint32_t ENC_PACK_MAX_N = 16;                          // components per element the packing tile is sized for
constexpr uint32_t ENC_STAGE = 4096, ENC_STAGE_PAD = 576;      // bytes staged in LDS per refill; look-ahead a 64-byte window may need (words <= 255 symbols)
constexpr uint32_t ENC_HIST_CHUNK = 1u << 18;
// one piece the value coder copies back compacted (k_enc_gather)
struct CopyJob { const uint8_t *src; uint8_t *dst; uint64_t bytes, dst_off; };

// ---- crthip_encode_batch (k_encode_batch.hip, encode_batch.cpp) ----
// estimated normals of one mesh (src/normal_attribute.cpp:113-143): faces in ORIGINAL vertex ids, degenerate ones dropped
struct EstJob {
	const uint32_t *faces;         // nface x 3
	const int32_t *coords;         // quantised positions, nvert x 3
	int32_t *normals;              // quantised octahedral normals, nvert x 2: the estimate is subtracted in place
	int32_t *boundary;             // BORDER: nvert XORs of neighbour ids (zeroed), else null
	uint32_t nface, nvert;
	uint32_t vbase;                // the mesh's first vertex in the batch's numbering (the corner sort's key)
	uint32_t fbase;                // its first face in the faces region (the corner sort's payload)
	uint32_t cbase;                // its first corner in the corner arrays
	int32_t unit;
	uint32_t pad[2];
};
// residuals of one attribute (GenericAttr::deltaEncode, vertex_attribute.h:130-144; NormalAttr::deltaEncode, normal_attribute.cpp:145-176)
enum : uint32_t { DENC_I32 = 0, DENC_U8 = 1, DENC_NRM_DIFF = 2, DENC_NRM_EST = 3, DENC_NRM_BORDER = 4 };
struct DeltaEncJob {
	const void *values;            // quantised: count_in x N int32, or bytes (colour)
	const uint32_t *quads;         // (t, a, b, c) per encoded vertex
	void *out;                     // residuals, count x N (BORDER: the boundary vertices' values, compacted)
	const int32_t *boundary;       // BORDER
	uint32_t *out_count;           // BORDER: residuals written
	uint32_t count, N, kind, parallel;
};
// Morton order of one point cloud (src/encoder.cpp:238-262)
struct ZJob {
	const int32_t *coords;         // quantised positions, n x 3
	int32_t *mn;                   // 3: min(0, coordinate), by integer atomics
	uint64_t *keys; uint32_t *vals;   // n records
	uint32_t *flag;                // out: adjacent equal keys after the sort
	uint32_t *quads;               // out: the prediction (t, prev, prev, prev)
	uint32_t n, pad;
};
// ---- crthip_encode_batch_to_device (k_encode_splice.hip, enc_splice.h) ----
// one piece of the arena: `bytes` bytes from a library allocation (the value coder's image, the chunk image, the literal buffer) to their
// place in the caller's arena, any alignment on both sides; tile_start[j] is the first tile (wave) of job j, as block_start is elsewhere
struct SpliceJob { const uint8_t *src; uint8_t *dst; uint64_t bytes; };
static_assert(sizeof(SpliceJob) == 24, "splice job layout");

constexpr uint32_t RS_THREADS = 256, RS_ITEMS = 16, RS_TILE = RS_THREADS*RS_ITEMS;   // radix sort: 8-bit digits, a tile of 4 096 records a workgroup
constexpr uint32_t DENC_BLOCK = 1024;                                                  // encoded vertices a workgroup of k_enc_delta

} // namespace corto_hip
