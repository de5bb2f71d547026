/* corto_hip.h — C ABI of the MI355X-native corto decode path (libcorto_hip.so).
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++/torch/HIP types.
 * Reference citations are relative to the upstream tree (cnr-isti-vclab/corto @ 2025-10-03).
 *
 * What it replaces
 *   crt::Decoder::Decoder(len, input)           src/decoder.cpp:41-89        -> crthip_probe / crthip_batch_create
 *   crt::Decoder::setPositions/Normals/Uvs/
 *        setColors/setAttribute/setIndex         include/corto/decoder.h:50-61 -> crthip_batch_bind[_all]
 *   crt::Decoder::decode()                       src/decoder.cpp:126-196      -> crthip_batch_decode (+ _sync)
 *   the legacy one-blob veneers CreateDecoder/DecodeMesh (src/corto_codec.h:41-43) and the WASM glue
 *   (html/js/emscripten/emcorto.cpp:14-89) map onto crthip_decode_host(), see INTEGRATION.md.
 *
 * Error behaviour: every entry point returns CRTHIP_OK (0) or a negative CRTHIP_E_* code and never
 * throws; crthip_last_error() returns the message, which for the conditions the reference throws on
 * is the reference's own string literal ("Not a crt file.", "Memory must be alignegned on 4 bytes.",
 * "Decoding topology failed", "Unknown entropy", ...).
 *
 * There is NO CPU fallback behind this ABI: if no HIP device is usable the calls fail with
 * CRTHIP_E_DEVICE.
 *
 * Device buffers: a context decodes on its own NON-BLOCKING HIP streams, which do not wait for the null stream or for any
 * stream of the caller.  Work the caller queued on the buffers it hands over (a fill of the output block, an upload of the
 * arena on another stream) must have completed before crthip_batch_decode / crthip_tunstall_decode_blocks is called, and the
 * outputs are complete when crthip_batch_sync (or the host-output call) returns - the same contract as handing a buffer to
 * any library that owns its streams.
 */
#ifndef CORTO_HIP_H
#define CORTO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CRTHIP_ABI_VERSION 6   /* 2: crthip_attr_binding.stride, crthip_mesh.group_props, crthip_pool_*; 3: crthip_pool_report grew, crthip_pool_warning;
                                  4: integer / DOUBLE output formats of generic attributes, crthip_pool_device_cpus; 5: crthip_pool_set_outputs_to_host;
                                  6: crthip_pool_set_render_layouts, crthip_kernel_times names are the kernels' (unpack_wave, delta_lds16);
                                     added within 6: crthip_generic_attr, crthip_attr_list, crthip_encode_attrs, crthip_encode_gpu_attrs,
                                     crthip_encode_batch_attrs, crthip_batch_create_resident, crthip_batch_reset_resident, crthip_batch_exif,
                                     crthip_batch_groups, crthip_batch_group_props, crthip_batch_walk_stats, crthip_batch_decode_with_next,
                                     crthip_batch_set_parity, crthip_encode_batch_resident, crthip_encode_input_model,
                                     crthip_encode_batch_to_device, crthip_encode_batch_bound, crthip_ctx_encode_splice_stats,
                                     crthip_output_layout, crthip_pool_decode (crthip_pool_dest, crthip_pool_done_fn), crthip_mesh_layout,
                                     crthip_encode_layout, crthip_encode_batch_layout, crthip_encode_input_model_layout,
                                     crthip_encode_topology_model_layout; crthip_batch_stats and crthip_pool_report grew at their ends
                                     (upload_copies, upload_gathered_bytes; grouped_steps); crthip_batch_bind_computed_normals (a new
                                     call and nothing else: the number stays 6); CRTHIP_BIND_QUANTIZED, crthip_quant_transform,
                                     crthip_batch_quant_transform, crthip_batch_bind_quant_transforms (a flag that was refused before and
                                     two new calls: the number stays 6); crthip_batch_bind_computed_tangents, crthip_tangent_model (two
                                     new calls and nothing else: the number stays 6); crthip_meshlet, crthip_meshlet_counts,
                                     crthip_meshlet_binding, crthip_meshlet_bound, crthip_batch_bind_meshlets, crthip_batch_meshlet_counts,
                                     crthip_meshlet_model (new calls and their structs, nothing else: the number stays 6);
                                     crthip_meshlet_bounds, crthip_batch_bind_meshlet_bounds, crthip_meshlet_bounds_model (a struct and two
                                     new calls, nothing else: the number stays 6); CRTHIP_NO_TWIN, crthip_adjacency_counts,
                                     crthip_adjacency_binding, crthip_batch_bind_adjacency, crthip_adjacency_model (two structs and two
                                     new calls, nothing else: the number stays 6); CRTHIP_WELD_ADJACENCY, crthip_weld_counts,
                                     crthip_weld_binding, crthip_batch_bind_weld, crthip_weld_model (two structs and two new calls,
                                     nothing else: the number stays 6); CRTHIP_LOD_MAX_LEVELS, crthip_lod_counts, crthip_lod_level,
                                     crthip_lod_binding, crthip_batch_bind_lod, crthip_lod_model (three structs and two new calls,
                                     nothing else: the number stays 6); CRTHIP_CLOUD_LOD_MAX_LEVELS, crthip_cloud_lod_counts,
                                     crthip_cloud_chunk, crthip_cloud_lod_level, crthip_cloud_lod_binding, crthip_batch_bind_cloud_lod,
                                     crthip_cloud_lod_model (four structs and two new calls, nothing else: the number stays 6);
                                     CRTHIP_COMPACT_MAX_SETS, CRTHIP_COMPACT_MAX_GATHERS, CRTHIP_NO_VERTEX, CRTHIP_COMPACT_*,
                                     crthip_compact_counts, crthip_compact_gather, crthip_compact_set, crthip_compact_binding,
                                     crthip_batch_bind_compact, crthip_compact_model_gather, crthip_compact_model (five structs and two
                                     new calls, nothing else: the number stays 6); CRTHIP_BVH_LEAF, CRTHIP_NO_NODE, crthip_bvh_node,
                                     crthip_bvh_counts, crthip_bvh_binding, crthip_batch_bind_bvh, crthip_bvh_model (three structs and two
                                     new calls, nothing else: the number stays 6); CRTHIP_CAST_ANY, CRTHIP_CAST_FRONT, CRTHIP_NO_FACE,
                                     CRTHIP_CAST_*, crthip_segment, crthip_cast_hit, crthip_bvh_cast_set, crthip_bvh_cast,
                                     crthip_bvh_cast_model, crthip_bvh_cast_model_stats (three structs and three new calls, nothing else:
                                     the number stays 6); CRTHIP_QUERY_COUNT, CRTHIP_QUERY_BOXES, CRTHIP_QUERY_INSIDE, CRTHIP_QUERY_*,
                                     crthip_box, crthip_query_result, crthip_bvh_query_set, crthip_bvh_query, crthip_bvh_query_model,
                                     crthip_bvh_query_model_stats (three structs and three new calls, nothing else: the number stays 6);
                                     CRTHIP_CLOSEST_WITHIN, CRTHIP_CLOSEST_ANY, CRTHIP_CLOSEST_*, crthip_point, crthip_closest_hit,
                                     crthip_bvh_closest_set, crthip_bvh_closest, crthip_bvh_closest_model, crthip_bvh_closest_model_stats
                                     (three structs and three new calls, nothing else: the number stays 6) */

/* VertexAttribute::Format, include/corto/vertex_attribute.h:32 */
enum { CRTHIP_FMT_UINT32 = 0, CRTHIP_FMT_INT32 = 1, CRTHIP_FMT_UINT16 = 2, CRTHIP_FMT_INT16 = 3,
       CRTHIP_FMT_UINT8 = 4, CRTHIP_FMT_INT8 = 5, CRTHIP_FMT_FLOAT = 6, CRTHIP_FMT_DOUBLE = 7 };
/* VertexAttribute::CODEC, include/corto/vertex_attribute.h:34 */
enum { CRTHIP_CODEC_GENERIC = 1, CRTHIP_CODEC_NORMAL = 2, CRTHIP_CODEC_COLOR = 3 };
/* VertexAttribute::Strategy, include/corto/vertex_attribute.h:33 */
enum { CRTHIP_PARALLEL = 1, CRTHIP_CORRELATED = 2 };
/* Stream::Entropy, include/corto/cstream.h:35 */
enum { CRTHIP_ENTROPY_NONE = 0, CRTHIP_ENTROPY_TUNSTALL = 1 };

enum {
	CRTHIP_OK = 0,
	CRTHIP_E_ALIGN = -1,        /* "Memory must be alignegned on 4 bytes."  src/decoder.cpp:44 */
	CRTHIP_E_MAGIC = -2,        /* "Not a crt file."                        src/decoder.cpp:51 */
	CRTHIP_E_TRUNCATED = -3,    /* stream runs past len (the reference never checks) */
	CRTHIP_E_ENTROPY = -4,      /* "Unknown entropy"                        src/cstream.cpp:82 */
	CRTHIP_E_TOPOLOGY = -5,     /* "Decoding topology failed"               src/decoder.cpp:274 */
	CRTHIP_E_NORMAL_NEEDS_POSITION = -6, /* src/normal_attribute.cpp:219-227 */
	CRTHIP_E_FORMAT = -7,       /* output format not supported for that attribute */
	CRTHIP_E_ARGUMENT = -8,
	CRTHIP_E_DEVICE = -9,       /* no usable HIP device / HIP runtime error */
	CRTHIP_E_NOMEM = -10,
	CRTHIP_E_LIMIT = -11        /* more attributes / components than this build supports */
};

#define CRTHIP_MAX_ATTRS 16
#define CRTHIP_NAME_MAX 64

typedef struct {
	char name[CRTHIP_NAME_MAX];  /* NUL-terminated */
	uint32_t codec;              /* CRTHIP_CODEC_* (anything else is treated as GENERIC, src/decoder.cpp:77-79) */
	float q;                     /* quantisation step as stored */
	uint32_t components;         /* N as stored (normals always decode 2 octahedral ints -> 3 outputs) */
	uint32_t format;             /* encoder-side format byte as stored (informational) */
	uint32_t strategy;           /* CRTHIP_PARALLEL | CRTHIP_CORRELATED */
} crthip_attr_info;

typedef struct {
	uint32_t version, entropy;
	uint32_t nvert, nface;
	uint32_t nattr;                              /* attributes in std::map order = sorted by name */
	crthip_attr_info attr[CRTHIP_MAX_ATTRS];
	uint32_t nexif;
	uint32_t body_offset;                        /* first byte after the header */
} crthip_blob_info;

/* Per-attribute output binding (Decoder::setAttribute, src/decoder.cpp:96-123).
 * buffer == NULL leaves the attribute unbound: its streams are skipped, like the reference does.
 * Buffers are DEVICE pointers for the batch API (crthip_batch_*) and HOST pointers for crthip_decode_host.
 *   generic (position, uv, radius, ...): FLOAT - nvert*components*4 bytes (decoded in place as int32 first) - is what upstream's callers use;
 *            the other formats of Decoder::setAttribute(name, buffer, format) (src/decoder.cpp:96-102) are taken too (ABI v4): the integer
 *            formats leave upstream's in-place "*= q" over the int32 array (nvert*components*4 bytes), DOUBLE widens it (nvert*components*8
 *            bytes) - what the compiled reference leaves there, include/corto/vertex_attribute.h:195-228; packed only (stride 0), 4-byte
 *            aligned (DOUBLE: 8)
 *   FLOAT buffers must be 4-byte aligned and INT16 ones 2-byte aligned (what a float* / int16_t* is), else CRTHIP_E_ARGUMENT
 *   normal : FLOAT (nvert*3 f32) or INT16 (nvert*3 i16)
 *   color  : UINT8, out_components = 3 or 4 (>= stored components); nvert*out_components bytes        */
typedef struct {
	void *buffer;
	uint32_t format;
	uint32_t out_components;
	uint32_t stride;             /* bytes from one vertex to the next; 0 = tightly packed (the layouts above).  A stride lets several
	                                attributes land in ONE interleaved vertex buffer (buffer = base + the attribute's offset in the
	                                vertex record): SURVEY.md 8f-3, the render-ready form of Decoder::setNormals(int16_t*) /
	                                setIndex(uint16_t*) (include/corto/decoder.h:53,61).  Must be a multiple of 4 for FLOAT outputs, of 2
	                                for INT16 normals, and at least the element's size; with a stride the attribute is decoded in device
	                                scratch and only its final values touch the buffer (a packed generic buffer doubles as int32 workspace) */
	uint32_t reserved;           /* flags: 0, CRTHIP_BIND_STREAM_VALUES or CRTHIP_BIND_QUANTIZED */
} crthip_attr_binding;
/* crthip_attr_binding.reserved, generic attributes only (ABI 6): stop behind the stream decode - `buffer` (nvert*N int32, packed, format
 * CRTHIP_FMT_INT32) receives the values as the stream holds them, i.e. what upstream's GenericAttr<int>::decode leaves in the buffer
 * (include/corto/vertex_attribute.h:151-156: InStream::decodeArray / decodeValues) BEFORE deltaDecode and dequantize.  This is the device
 * half of a caller-supplied codec object (Decoder::setAttribute(name, buffer, VertexAttribute *), src/decoder.cpp:104-114): its
 * deltaDecode / postDelta / dequantize are host code and run on these values (include/corto/decoder.h of this repo).  A position bound this
 * way cannot feed ESTIMATED / BORDER normals (upstream throws "Position attr has been overloaded" there, src/normal_attribute.cpp:210-213):
 * the blob fails with CRTHIP_E_NORMAL_NEEDS_POSITION. */
#define CRTHIP_BIND_STREAM_VALUES 1u

/* crthip_attr_binding.reserved, generic attributes only (added within ABI 6): quantised output.  `buffer` receives, for vertex i and
 * component c, (uint16_t)(v[i][c] - base[c]): v is the delta-decoded integer value - what upstream's GenericAttr::deltaDecode leaves
 * before dequantize (include/corto/vertex_attribute.h:160-193) - and base[c] the minimum of component c over the blob's vertices, as
 * signed int32.  These are the 16-bit integer attributes of a KHR_mesh_quantization-style vertex buffer; the per-blob scale and offset the
 * vertex shader applies are in the blob's crthip_quant_transform (below), which also holds the attribute's exact bounding box.
 * Checked when the blob is bound:
 *   CRTHIP_E_FORMAT    a format other than CRTHIP_FMT_UINT16; a normal or a colour
 *   CRTHIP_E_ARGUMENT  together with CRTHIP_BIND_STREAM_VALUES, or with its format CRTHIP_FMT_INT32 (the code that combination had before the
 *                      flag existed); out_components other than 0 or the stored N; a buffer that is not 2-byte
 *                      aligned; a stride that is non-zero and below 2*N, or odd
 *   CRTHIP_E_LIMIT     more than four stored components
 * stride 0 (or exactly 2*N) is the packed layout, nvert*N halfwords.  With a stride only the 2*N bytes of each vertex are written - the
 * rule of every strided binding - so a position uint16 x 3 at stride 8 lands in an interleaved record.
 * One error is left to decode time, because it depends on the values: if max - min of any component exceeds 65535, nothing is written to
 * that attribute's buffer, its record is filled with written = 0, and the blob's status becomes CRTHIP_E_FORMAT unless the blob already
 * failed (an earlier code stays).  The blob's other arrays and the batch's other blobs decode as usual.
 * A quantised position feeds stored ESTIMATED / BORDER normals and crthip_batch_bind_computed_normals as a FLOAT one does: they read the
 * integers.  Not part of crthip_pool_* / crthip_output_layout, crthip_decode_host (the flag is ignored there), the crt::Decoder facade or
 * the veneers, which keep upstream's host contract; no INT16 / UINT8 / UINT32 variant. */
#define CRTHIP_BIND_QUANTIZED 2u
/* What takes a quantised attribute's halfwords back, one record per (blob, attribute).  The contract:
 *   (float)(int32_t)(base[c] + out[i][c]) * q   is bit for bit the CRTHIP_FMT_FLOAT output of the same attribute,
 * so a shader computes position = (float(base) + float(out)) * q where that sum is exact in float (|values| < 2^24), and
 * [base*q, (base + span)*q] is the attribute's bounding box.  span[c] = max - min of component c (computed in 64 bits, always fits);
 * components beyond `components` are zero.  nvert == 1: base = the value, span 0.  nvert == 0: the record is all zero but written = 1. */
typedef struct {
	int32_t base[4];
	uint32_t span[4];
	float q;                     /* the attribute's step as stored */
	uint32_t components;         /* N as stored */
	uint32_t written;            /* 1: the halfwords were stored; 0: a span beyond 65535, the buffer was left alone */
	uint32_t reserved;
} crthip_quant_transform;

typedef struct crthip_ctx crthip_ctx;       /* one per device; owns streams + scratch pool */
typedef struct crthip_batch crthip_batch;   /* a planned batch of independent .crt blobs */

uint32_t crthip_abi_version(void);
const char *crthip_last_error(void);         /* thread-local message of the last failing call */
const char *crthip_strerror(int code);

/* Header parse only; host-only, needs no GPU.  blob must be 4-byte aligned (src/decoder.cpp:43-44). */
int crthip_probe(const uint8_t *blob, size_t len, crthip_blob_info *info);
/* exif pairs / group table of one blob, host-only.  Strings are copied into out (NUL-separated
 * key\0value\0...); returns bytes needed, or <0. */
int64_t crthip_probe_exif(const uint8_t *blob, size_t len, char *out, size_t cap);
/* groups: writes min(cap, ngroups) end-face markers, returns ngroups or <0 (include/corto/index_attribute.h:89-99) */
int64_t crthip_probe_groups(const uint8_t *blob, size_t len, uint32_t *group_end, size_t cap);
/* properties of group g as key\0value\0... (Group::properties); returns bytes needed, or <0 */
int64_t crthip_probe_group_props(const uint8_t *blob, size_t len, uint32_t g, char *out, size_t cap);

int crthip_ctx_create(int device, crthip_ctx **out);
void crthip_ctx_destroy(crthip_ctx *ctx);
/* A context decodes a batch on two HIP streams (CLERS streams + topology on one, the attribute streams' entropy decode and bit-unpack
 * on the other, joined before the delta stage): the shortest latency for one batch.  The second stream is made by the first decode
 * that forks onto it, so a context that is switched to one stream before it decodes holds one HIP stream only (switching it back
 * later is fine: the next decode that forks makes the stream).  With many contexts on one GPU the streams
 * outnumber the hardware queues ($GPU_MAX_HW_QUEUES, ROCm default 4) and streams that share a queue serialise each other's kernels:
 * from about queues/2 contexts up, one stream per context is faster (12 contexts, 16 queues: +15 %; crthip_pool chooses by itself).
 * The same switch selects the LDS-lean layout of the normals kernel (29 KB instead of 78 KB per blob: slower alone, but with many
 * batches in flight a kernel's wait for LDS is what its latency is made of: +10 %). */
int crthip_ctx_set_single_stream(crthip_ctx *ctx, int on);
/* Blobs that already sit in pinned host memory (hipHostMalloc / hipHostRegister / torch pin_memory) in the arena's own layout: with this
 * switch on, crthip_batch_create / _reset upload them straight from there - no gathering into the library's own pinned image first (3.7 MB
 * of memcpy per C4 batch: 150 us of a from-host step's host time).  The blob list is cut into RUNS: a run is a stretch of consecutive
 * blobs that follow one another in host memory as crthip_arena_layout places them (blob i + 1 at blob i + its length rounded up to 16).
 * Every run goes up with ONE DMA copy from the caller's memory to its place in the device arena.  All blobs in one buffer laid out by
 * crthip_arena_layout are one run and one copy; the blobs of two such buffers, one list after the other, are two.  A list that falls
 * into more than 8 runs takes the gathering path, as does every list while the switch is off (crthip_batch_stats: upload_copies,
 * upload_gathered_bytes say which path ran).  The caller's promise, for EVERY buffer a run lies in: it stays valid and unchanged until the
 * batch has been synced, the padding between a run's blobs included (it is copied along).  A run in pageable memory is still decoded
 * correctly (the runtime stages it), but its copy may block the calling thread.  (No reference counterpart: crt::Decoder reads its one
 * blob from the caller's memory in place, src/decoder.cpp:41-48.) */
int crthip_ctx_set_packed_host_blobs(crthip_ctx *ctx, int on);
int crthip_device_count(void);

/* Plan a batch: parse every header, walk every body (validating all extents against lens[i]),
 * stage the blobs into one 16-byte-aligned device arena and upload the stream descriptors.
 * blobs[i] are HOST pointers (borrowed only for the duration of this call).
 * device_arena: NULL -> the library uploads the blobs itself;
 *               else  -> DEVICE pointer to the blobs already resident in HBM, laid out back to back with each
 *                        blob starting at the next 16-byte multiple (offsets via crthip_arena_layout). */
int crthip_batch_create(crthip_ctx *ctx, uint32_t nblobs, const uint8_t *const *blobs, const uint32_t *lens,
                        const void *device_arena, crthip_batch **out);
/* Re-plan an existing batch object for a new list of blobs (same meaning as destroy + create, bindings are cleared) reusing
 * its allocations: what a serving loop that decodes batch after batch on one context calls instead of create / destroy. */
int crthip_batch_reset(crthip_batch *b, uint32_t nblobs, const uint8_t *const *blobs, const uint32_t *lens, const void *device_arena);
/* Blobs that live ONLY in device memory (a VRAM cache of compressed tiles, bytes read straight into a device tensor, another kernel's
 * output): blob i is the lens[i] bytes at device_base + offsets[i].  offsets / lens are HOST arrays; the offsets need not follow
 * crthip_arena_layout, ascend or be contiguous - a batch may pick any subset of a large buffer, a blob more than once.  The walk of
 * crthip_batch_create runs on the device (one wave per blob, on the context's main stream) and only a fixed record per blob comes back
 * (crthip_batch_walk_stats); a blob whose layout does not fit its record (kilobytes of exif, hundreds of log streams) is copied back
 * alone and walked on the host.  The call waits for that walk: one synchronisation of the context's main stream, so a create on a
 * context whose other batch is still decoding waits behind that decode (the round-robin pattern of INTEGRATION.md §3 finds the
 * stream idle).
 * The caller's rules:
 *   - device_base and every offset are multiples of 16, else CRTHIP_E_ARGUMENT (as is a NULL device_base with nblobs > 0);
 *   - [offset, offset + lens[i] rounded up to 16) lies inside one allocation (the device reads whole 16-byte words);
 *   - the caller's writes to the buffer have completed before the call ("Device buffers" above), and the buffer stays unchanged
 *     until the batch has been synced.
 * Errors as for crthip_batch_create: the first failing blob's code, "(blob i)" in crthip_last_error().  A failed reset leaves the
 * object empty-handed.  Afterwards info, bind, decode, sync, stats and crthip_batch_reset work as for a host-created batch, and one
 * object may switch between host and resident resets. */
int crthip_batch_create_resident(crthip_ctx *ctx, uint32_t nblobs, const void *device_base, const uint64_t *offsets, const uint32_t *lens,
                                 crthip_batch **out);
int crthip_batch_reset_resident(crthip_batch *b, uint32_t nblobs, const void *device_base, const uint64_t *offsets, const uint32_t *lens);
/* offsets[i] = arena byte offset of blob i under the rule above; returns total arena bytes */
uint64_t crthip_arena_layout(uint32_t nblobs, const uint32_t *lens, uint64_t *offsets);
void crthip_batch_destroy(crthip_batch *b);

uint32_t crthip_batch_size(const crthip_batch *b);
int crthip_batch_info(const crthip_batch *b, uint32_t i, crthip_blob_info *info);
/* crthip_probe_exif / _groups / _group_props of blob i of a planned batch, from what its walk stored: the same for a batch created
 * from host or from device memory. */
int64_t crthip_batch_exif(const crthip_batch *b, uint32_t i, char *out, size_t cap);
int64_t crthip_batch_groups(const crthip_batch *b, uint32_t i, uint32_t *group_end, size_t cap);
int64_t crthip_batch_group_props(const crthip_batch *b, uint32_t i, uint32_t g, char *out, size_t cap);
/* Where the last create / reset walked the blobs. */
typedef struct {
	uint32_t device_walked;      /* blobs walked on the device (a resident create) */
	uint32_t host_walked;        /* blobs walked on the host: every blob of a host create, a resident create's fallbacks */
	uint64_t bytes_to_host;      /* device-to-host bytes of the create: the walk records and the fallback blobs */
	float walk_kernel_us;        /* device time of the walk kernel (0 for a host create) */
	uint32_t reserved;
} crthip_walk_stats;
int crthip_batch_walk_stats(const crthip_batch *b, crthip_walk_stats *s);

/* Bind outputs of blob i. attrs has info.nattr entries in info.attr order. index: DEVICE pointer to
 * nface*3 entries of index_format (CRTHIP_FMT_UINT32 or CRTHIP_FMT_UINT16), NULL for point clouds. */
int crthip_batch_bind(crthip_batch *b, uint32_t i, const crthip_attr_binding *attrs, void *index, uint32_t index_format);
/* Bind every blob in one call: attrs holds sum(nattr) entries blob after blob; index/index_format have nblobs entries. */
int crthip_batch_bind_all(crthip_batch *b, const crthip_attr_binding *attrs, void *const *index, const uint32_t *index_format);
/* Normals for a mesh whose blob stores none, or whose stored "normal" is left unbound: what upstream's decoder leaves at a vertex
 * that takes no correction (src/normal_attribute.cpp:294-302, 320-323), at EVERY vertex - the GPU's answer to what upstream's callers
 * do after such a decode (README.md: if(!geometry.attributes.normal) geometry.computeVertexNormals()).  Added within ABI 6.
 *   est[v] = sum over the faces f incident to v, in ascending f, of cross(P[b]-P[a], P[c]-P[a])      (estimateNormals, :40-59)
 *   len    = sqrtf((ex*ex + ey*ey) + ez*ez)
 * over the INTEGER (delta-decoded, not dequantised) positions as floats, without FMA; a face that lists v twice adds twice.
 *   CRTHIP_FMT_FLOAT: nvert*3 f32, est/len;   CRTHIP_FMT_INT16: nvert*3 i16, (int16_t)(est*(32767.0f/len)) per component.
 * One deliberate difference from upstream's branch: a vertex whose estimate is zero (no face, or faces that cancel; with integer positions
 * len is 0 or at least 1) gets (0,0,1) / (0,0,32767) - upstream's evident intention - where upstream's FLOAT path divides 0 by 0 and its
 * INT16 path sets (0,0,1) and never stores it.  A renderer gets neither NaNs nor stale bytes: every element of the array is written.
 * buffer: DEVICE pointer; stride and alignment exactly as for a stored normal's crthip_attr_binding.  Call it AFTER crthip_batch_bind /
 * _bind_all for blob i: a later bind of that blob drops it, as does crthip_batch_reset*; buffer == NULL removes it.  Every error is
 * returned here and nothing new can fail at decode time:
 *   CRTHIP_E_ARGUMENT  i out of range; a point cloud; the blob has a "normal" attribute with a bound buffer; a stride or an alignment a
 *                      normal binding would refuse
 *   CRTHIP_E_FORMAT    a format other than FLOAT / INT16
 *   CRTHIP_E_NORMAL_NEEDS_POSITION  "position" missing, not generic with 3 components, unbound, or bound with CRTHIP_BIND_STREAM_VALUES
 *                      (the rule of a stored ESTIMATED normal)
 * crthip_last_error() names the blob.  Not part of crthip_pool_* / crthip_output_layout, crthip_decode_host or the crt::Decoder facade. */
int crthip_batch_bind_computed_normals(crthip_batch *b, uint32_t i, void *buffer, uint32_t format, uint32_t stride);

/* Tangents for a mesh blob: the one vertex attribute a normal-mapped material needs that .crt does not store (upstream computes none).
 * Added within ABI 6.  The decoder holds what a caller's own pass no longer has - positions and uvs as INTEGERS - so the per-face terms are
 * summed exactly and the result does not depend on the order in which faces are visited.
 * Inputs: p[v], the delta-decoded integer position (3 x int32); t[v], the delta-decoded integer value of the attribute named "uv"
 * (2 x int32); the decoded index; n[v], the vertex's final normal as the decode leaves it in its bound buffer, as three floats (bound as
 * INT16: the three int16 values converted to float, not rescaled).
 * Per face f = (a, b, c), on 64-bit two's-complement integers - differences are widened first, products and sums wrap modulo 2^64:
 *   e1 = p[b]-p[a]   e2 = p[c]-p[a]   (s1,r1) = t[b]-t[a]   (s2,r2) = t[c]-t[a]
 *   det = s1*r2 - s2*r1      sg = (det>0) - (det<0)
 *   Tf = sg*(e1*r2 - e2*r1)  Bf = sg*(e2*s1 - e1*s2)
 * Tf and Bf are added to the accumulators T[v], B[v] of a, b and c (modulo 2^64); a face that names a vertex twice adds twice; a face
 * with det == 0 adds nothing.  This is the uv-area-weighted tangent.  No intermediate exceeds 63 bits for positions and uvs of up to 24
 * bits at any realistic valence, and then the sums are exact; the wrap rule defines the value for every other input.
 * Per vertex, in float32, every product, sum and difference rounded on its own (no FMA):
 *   scale       k = max(0, bitlength(max |x| over the six components of T[v], B[v]) - 24); every component becomes
 *               sign(x)*(|x| >> k) - truncated toward zero, so that mirrored uvs give mirrored tangents - and then a float, exactly
 *   Gram-Schmidt, invariant to the scale of n (INT16 normals need no division):
 *               nn = (nx*nx + ny*ny) + nz*nz      nt = (nx*Tx + ny*Ty) + nz*Tz
 *               u = T*nn - n*nt   (a component: two products, one subtraction)      len = sqrtf((ux*ux + uy*uy) + uz*uz)
 *   handedness  c = cross(n, u) = (ny*uz - nz*uy, nz*ux - nx*uz, nx*uy - ny*ux);  h = (cx*Bx + cy*By) + cz*Bz;  w = h < 0 ? -1 : +1
 *               - glTF's meaning: bitangent = cross(normal, tangent.xyz)*w.  The uv v-flip convention is the caller's.
 *   fallback    len not a finite value greater than 0 (a vertex no face names, uvs without area, a tangent parallel to the normal, a NaN
 *               normal, a T that the common shift k leaves at zero - every component of T[v] 2^24 times below the largest of B[v]):
 *               (1, 0, 0, +1).  Every element of the array is written, and never with a NaN.
 *   CRTHIP_FMT_FLOAT: 4 x f32 a vertex, (u/len, w).   CRTHIP_FMT_INT16: 4 x i16 a vertex, l = 32767.0f/len, (int16_t)(u*l) a component
 *   by truncation (the rule of the INT16 normals), w = +-32767; the fallback is (32767, 0, 0, 32767).
 * buffer: DEVICE pointer.  stride 0 = packed, 16 bytes a vertex (FLOAT) or 8 (INT16).  FLOAT: a 4-byte aligned buffer, a stride that is a
 * multiple of 4 and at least 16; INT16: 2-byte aligned, an even stride of at least 8.  With a stride only the vertex's own 16 or 8 bytes
 * are written, as by every strided binding.
 * Call it AFTER crthip_batch_bind / _bind_all for blob i and AFTER crthip_batch_bind_computed_normals if that is the normals' source: a
 * later bind or computed-normals call for blob i drops it, as does crthip_batch_reset*; buffer == NULL removes it.  position and uv may
 * be bound as FLOAT (packed or strided), in any integer format or with CRTHIP_BIND_QUANTIZED - the kernels read the integers in every
 * case, as estimated normals do; the index may be uint32, uint16 or unbound.  Every error is returned here and nothing new can fail at
 * decode time:
 *   CRTHIP_E_ARGUMENT  b NULL or i out of range; a point cloud; no attribute named "uv" that is generic with 2 stored components and bound
 *                      without CRTHIP_BIND_STREAM_VALUES; no normal source (neither a stored "normal" bound as FLOAT or INT16 nor a
 *                      computed-normals binding); a stride or an alignment that breaks the rules above
 *   CRTHIP_E_FORMAT    a format other than FLOAT / INT16
 *   CRTHIP_E_NORMAL_NEEDS_POSITION  "position" missing, not generic with 3 components, unbound, or bound with CRTHIP_BIND_STREAM_VALUES
 * crthip_last_error() names the blob.  Kernels tangent_blob (blobs of up to 2 304 vertices) and tangent_faces, tangent_vertex in
 * crthip_kernel_times.  Not part of crthip_pool_* / crthip_output_layout, crthip_decode_host, the crt::Decoder facade or the veneers. */
int crthip_batch_bind_computed_tangents(crthip_batch *b, uint32_t i, void *buffer, uint32_t format, uint32_t stride);

/* Meshlets from the blob's decoded index, built on the GPU in the decode call (kernels meshlet_blob, meshlet_segments, meshlet_place in
 * crthip_kernel_times; csrc/meshlet.h has the source the kernels and the test hook share).  Pure integer work on the index: the bytes are
 * defined exactly, need no position, uv or float, and no vertex id is ever used as an address - any index content gives defined output,
 * that of a blob whose topology failed included.
 * Inputs: the blob's nface triples of vertex ids, read as uint32 whether the index is bound as uint32, as uint16 or not at all (then from
 * scratch); the blob's group table (crthip_batch_groups); max_vertices 3..255; max_triangles 1..512; segment_faces 0 (= 4096) or 1..65536.
 * Cuts: sort the set {nface} + {min(group_end[g], nface)}; with 0 in front, every stretch [s, e) between neighbouring values is cut further
 *   at s + k*segment_faces, k >= 1, while that is below e.  A SEGMENT is a non-empty stretch between neighbouring cuts; no meshlet crosses a
 *   cut.  So a group (a draw range) is a whole number of meshlets, segments are independent (what makes a big mesh parallel), and the
 *   price is at most one under-filled meshlet a segment.
 * Within a segment faces are taken in index order.  The state is an ordered list V (empty) and a count t (0).  For face f = (a, b, c):
 *   1. d = the distinct ids among a, b, c that are not in V, in corner order;
 *   2. if t + 1 > max_triangles or |V| + |d| > max_vertices: emit the meshlet, clear V and t, recompute d;
 *   3. append d to V;   4. the face's three bytes are the positions of a, b, c in V;   5. t += 1.
 *   At the segment's end, emit if t > 0.  A face that names a vertex twice references it once and repeats the local id; max_vertices >= 3
 *   guarantees that a lone face fits.
 * Emission: meshlets in face order over the whole blob.  Meshlet k is a crthip_meshlet with meshopt_Meshlet's field meanings:
 *   vertex_offset = the sum of vertex_count of the earlier meshlets; triangle_offset = the sum of (3*triangle_count + 3) & ~3 of the earlier
 *   meshlets, a 4-byte aligned BYTE offset into triangles; vertices[vertex_offset + j] = V[j], uint32 ids into the blob's vertex arrays;
 *   triangles[triangle_offset + 3*i + c] = the local id of corner c of the meshlet's face i; the pad bytes are written as 0.
 *   A crthip_meshlet_counts a blob holds the totals.  Nothing beyond `meshlets` records, `vertices` words and `triangle_bytes` bytes is touched.
 * Capacity (derived): a meshlet that is not the last of its segment was closed by the triangle limit (t == max_triangles) or by the vertex
 *   limit (|V| >= max_vertices - 2 as |d| <= 3, and |V| <= 3t, so t >= ceil((max_vertices - 2)/3)).  With tmin = min(max_triangles,
 *   ceil((max_vertices - 2)/3)):  meshlets <= sum over segments of ceil(len/tmin);  vertices <= 3*nface;
 *   triangle_bytes <= 3*nface + 3*(that meshlet bound).  crthip_meshlet_bound computes it; it is reached at (3, 1, 1). */
typedef struct crthip_meshlet { uint32_t vertex_offset, triangle_offset, vertex_count, triangle_count; } crthip_meshlet;
typedef struct crthip_meshlet_counts { uint32_t meshlets, vertices, triangle_bytes, segments; } crthip_meshlet_counts;
typedef struct crthip_meshlet_binding {
	crthip_meshlet *meshlets;          /* DEVICE, 16-byte aligned, room for meshlet_capacity records */
	uint32_t *vertices;                /* DEVICE, 4-byte aligned, room for vertex_capacity words */
	uint8_t *triangles;                /* DEVICE, 4-byte aligned, room for triangle_capacity bytes */
	crthip_meshlet_counts *counts;     /* optional DEVICE copy of the blob's record for GPU-driven consumers: 16 bytes, 16-byte aligned; or NULL */
	uint32_t meshlet_capacity, vertex_capacity, triangle_capacity;   /* records, words, bytes: each at least crthip_meshlet_bound's */
	uint32_t max_vertices, max_triangles, segment_faces;
} crthip_meshlet_binding;
/* Host only, no device: the capacity bound above for an index of nface faces and a group table (group_end may be NULL when ngroups is 0;
 * ends beyond nface and repeated ones are allowed).  out->segments is the exact number of segments.  CRTHIP_E_ARGUMENT: out NULL, group_end
 * NULL with ngroups > 0, a parameter outside its range, or a bound beyond 32 bits. */
int crthip_meshlet_bound(uint32_t nface, uint32_t ngroups, const uint32_t *group_end, uint32_t max_vertices, uint32_t max_triangles,
                         uint32_t segment_faces, crthip_meshlet_counts *out);
/* Blob i's meshlets go to m's buffers in the decode.  Call it AFTER crthip_batch_bind / _bind_all for blob i: a later bind of that blob
 * drops it, as does crthip_batch_reset*; m == NULL removes it.  Independent of the computed-normals and tangent bindings.  Every error is
 * returned here and nothing new can fail at decode time.  CRTHIP_E_ARGUMENT: b NULL or i out of range; a point cloud; a parameter outside
 * the ranges above; a NULL or misaligned buffer (meshlets 16-byte aligned, vertices and triangles 4-byte aligned, counts 16-byte aligned
 * when given); any capacity below crthip_meshlet_bound for that blob.  crthip_last_error() names the blob.  Blobs without a meshlet
 * binding launch nothing new.  Not part of crthip_pool_* / crthip_output_layout, crthip_decode_host, the crt::Decoder facade or the veneers. */
int crthip_batch_bind_meshlets(crthip_batch *b, uint32_t i, const crthip_meshlet_binding *m);
/* Blob i's totals.  Valid after crthip_batch_sync of a decode in which blob i had a meshlet binding: the kernels write the record into the
 * batch's pinned status block, behind the quant records.  Otherwise CRTHIP_E_ARGUMENT. */
int crthip_batch_meshlet_counts(const crthip_batch *b, uint32_t i, crthip_meshlet_counts *out);

/* Culling data a meshlet - a bounding box, a bounding sphere and a normal cone, what meshopt_computeMeshletBounds gives - computed on the GPU
 * in the decode call from the blob's delta-decoded INTEGER positions and its final meshlet arrays (kernel meshlet_bounds in
 * crthip_kernel_times; csrc/meshlet_bounds.h has the source the kernel and the test hook share).  A decoded position is int * q with the one
 * positive scalar q of the position attribute, so box, centre and radius in grid units scale to world units by q - the world sphere has the
 * centre (float)center*q and the radius (float)radius*q - and directions are the same in both spaces.  The record is defined to the byte.
 * Record k belongs to meshlet k of the blob's final `meshlets` array; exactly counts.meshlets records are written and nothing behind them
 * is touched.  V is the meshlet's vertex list, p[v] the integer position of vertex v.  A vertex id >= nvert is ABSENT: it is never used as an
 * address (such ids exist only in blobs whose topology failed and in the hook's synthetic inputs).  A meshlet without a present vertex gets
 * a record that is all zero except cone_cutoff = 127.
 * Box: box_min[c] / box_max[c] are the minimum and maximum of p[v][c] over the present v in V.
 * Sphere: span[c] = (uint32)box_max[c] - (uint32)box_min[c]; center[c] = (int32)((uint32)box_min[c] + (span[c] >> 1));
 *   r2 = the maximum over the present v of the sum over c of ((int64)p[v][c] - center[c])^2, computed on uint64 modulo 2^64 (exact whenever
 *   every span is below 2^31; defined but meaningless beyond); radius = the smallest r in [0, 2^32 - 1] with r*r >= r2 as uint64, or
 *   2^32 - 1 if there is none.  The sphere holds every present vertex.
 * Cone: a face (a, b, c) of the meshlet (global ids through V) is a CONE FACE if all three ids are present and
 *   N = cross(p[b] - p[a], p[c] - p[a]) != 0, with the differences widened to 64 bits and products and sums on uint64 modulo 2^64 (exact
 *   whenever every coordinate difference is below 2^31 in magnitude).  Step 1 is integer work, the others float32, every operation rounded
 *   on its own:
 *   1. S = the sum of N over the cone faces, modulo 2^64 (associative: no order changes it);
 *   2. kS = max(0, bitlength(max_c |S[c]|) - 24), where |INT64_MIN| is 2^63;   3. s[c] = (float)(sign(S[c]) * (|S[c]| >> kS));
 *   4. L = sqrtf((s0*s0 + s1*s1) + s2*s2);
 *   5. without a cone face, or if !(L > 0): cone_axis = (0, 0, 0), cone_cutoff = 127, done;
 *   6. t = (s[c] / L) * 127.0f; cone_axis[c] = (int8)(int32)(t + (t < 0 ? -0.5f : 0.5f)), the conversion truncating;
 *   7. with A[c] = (float)cone_axis[c], the STORED axis (so the cutoff accounts for its quantisation), for every cone face: n[c] = N scaled
 *      by its own shift kN as in 2-3; d = ((A0*n0 + A1*n1) + A2*n2) / (sqrtf((A0*A0 + A1*A1) + A2*A2) * sqrtf((n0*n0 + n1*n1) + n2*n2));
 *   8. m = the minimum of d over the cone faces (every d is finite; a float minimum is exact in any order);
 *   9. if !(m > 0.1f): cone_cutoff = 127; else w = 1.0f - m*m, taken as 0 if !(w > 0) (m can round to a step above 1), and
 *      cone_cutoff = min(127, (int32)(sqrtf(w) * 127.0f) + 2).  Truncation plus 2 leaves a margin between 1/127 and 2/127 above the true
 *      value, orders of magnitude above the float error of step 7: the cone is conservative by construction.
 * Meaning: every non-degenerate face normal lies within the angle acos(m) of the stored axis.  With v the unit direction from the eye to
 *   the meshlet, all its faces are back-facing if dot(normalize(cone_axis), v) >= cone_cutoff/127; for perspective this is meshoptimizer's
 *   sphere form, dot(center - eye, axis) >= cutoff*|center - eye| + radius with the normalised axis, cutoff = cone_cutoff/127 and the world
 *   sphere above.  cone_cutoff 127 means "do not cull".  No cone apex is given. */
typedef struct crthip_meshlet_bounds {      /* 48 bytes; arrays of them are 16-byte aligned */
	int32_t  box_min[3], box_max[3];        /* grid units */
	int32_t  center[3];  uint32_t radius;   /* grid units: a sphere that holds every vertex */
	int8_t   cone_axis[3]; int8_t cone_cutoff;
	uint32_t reserved;                      /* written as 0 */
} crthip_meshlet_bounds;
/* Blob i's records go to `bounds` (DEVICE, 16-byte aligned, room for `capacity` records) in the decode.  Call it AFTER
 * crthip_batch_bind_meshlets for blob i: whatever drops the meshlet binding drops this one too - a later crthip_batch_bind of that blob,
 * crthip_batch_bind_meshlets(b, i, NULL), a new meshlet binding, crthip_batch_reset* - and bounds == NULL removes it.  Every error is
 * returned here and nothing new can fail at decode time; crthip_last_error() names the blob.  CRTHIP_E_ARGUMENT: b NULL or i out of range;
 * no meshlet binding on blob i; bounds not 16-byte aligned; capacity below crthip_meshlet_bound's .meshlets for this blob and the meshlet
 * binding's parameters.  CRTHIP_E_NORMAL_NEEDS_POSITION: "position" missing, not generic with 3 components, unbound, or bound with
 * CRTHIP_BIND_STREAM_VALUES (the rule of crthip_batch_bind_computed_tangents).  A packed FLOAT position is read in place in front of its
 * dequantisation, every other binding from scratch; the position's own output is unchanged.  Blobs without the binding launch nothing new.
 * Not part of crthip_pool_* / crthip_output_layout, crthip_decode_host, the crt::Decoder facade or the veneers. */
int crthip_batch_bind_meshlet_bounds(crthip_batch *b, uint32_t i, crthip_meshlet_bounds *bounds, uint32_t capacity);

/* Connectivity: the half-edge twins of the blob's decoded index, found on the GPU in the decode call (kernels adjacency_blob, and
 * adjacency_count, adjacency_offsets, adjacency_fill, adjacency_twin in crthip_kernel_times; csrc/adjacency.h has the source the kernels and
 * the test hook share).  Pure integer work on the final index: no position, no float, no hash of coordinates; the bytes are defined exactly.
 * A HALF-EDGE is h = 3*f + s, face f, side s in 0..2.  It runs from index[3f + s] to index[3f + (s + 1) % 3].
 * A face is INVALID if two of its corners are equal or a corner is >= nvert (such an index comes only from a blob whose topology failed;
 *   an id >= nvert is never used as an address); its three half-edges are INVALID.
 * twin[h] of a valid half-edge a -> b is the LEAST valid half-edge that runs b -> a, or CRTHIP_NO_TWIN if there is none.
 * twin[h] of an invalid half-edge is CRTHIP_NO_TWIN, and invalid half-edges are nobody's twin.
 * Groups play no part: a twin may lie in another group.
 * crthip_adjacency_counts: halfedges = 3*nface; boundary = the valid half-edges without a twin; duplicate = the valid half-edges whose
 *   directed edge a -> b is also that of a LOWER valid half-edge; invalid = the invalid half-edges.
 * What this buys: if duplicate == 0 every directed edge occurs once, so twin is an involution on the paired half-edges
 *   (twin[twin[h]] == h) and the blob is an oriented manifold with border; it is closed if also boundary == 0.
 * Exactly 3*nface words of twin and the 16 bytes of counts are written, nothing beyond them.
 * In a decode where the blob also has a weld binding with CRTHIP_WELD_ADJACENCY (below), "the index" is that binding's welded index. */
#define CRTHIP_NO_TWIN 0xFFFFFFFFu
typedef struct crthip_adjacency_counts { uint32_t halfedges, boundary, duplicate, invalid; } crthip_adjacency_counts;
typedef struct crthip_adjacency_binding {
	uint32_t *twin;                    /* DEVICE, 4-byte aligned, room for `capacity` words */
	crthip_adjacency_counts *counts;   /* optional DEVICE record for GPU-driven consumers: 16 bytes, 16-byte aligned; or NULL.  There is no host record */
	uint32_t capacity;                 /* words of twin: at least 3*nface */
	uint32_t reserved;                 /* 0 */
} crthip_adjacency_binding;
/* Blob i's twins go to a's buffers in the decode.  a == NULL removes the binding; a later crthip_batch_bind of that blob drops it, as does
 * crthip_batch_reset*.  It needs neither the index nor any attribute to be bound (an unbound index is read from scratch) and is independent
 * of every other derived binding.  Every error is returned here, in this order, and nothing new can fail at decode time.
 * CRTHIP_E_ARGUMENT: b NULL or i out of range; a point cloud (nface == 0); twin NULL or not 4-byte aligned, or counts not 16-byte aligned;
 * reserved != 0; capacity < 3*nface.  crthip_last_error() names the blob.  Blobs without the binding launch nothing new.
 * Not part of crthip_pool_* / crthip_output_layout, crthip_decode_host, the crt::Decoder facade or the veneers. */
int crthip_batch_bind_adjacency(crthip_batch *b, uint32_t i, const crthip_adjacency_binding *a);

/* A weld by position: for every vertex the least vertex at the same position, and the blob's index through that map, found on the GPU in the
 * decode call (kernels weld_blob, and weld_insert, weld_lookup, weld_index in crthip_kernel_times; csrc/weld.h has the source the kernels and
 * the test hook share).  A mesh that carries uvs or hard normals has its vertices split along every seam: crthip_batch_bind_adjacency
 * reports each seam as a border, and the welded index is what silhouettes, crack-free subdivision, a depth-only or shadow index
 * (meshopt_generateShadowIndexBuffer) and a closedness test need.  Integer work only; the bytes are defined exactly.
 * p[v] is the delta-decoded INTEGER position of vertex v, three int32: what crthip_batch_bind_computed_tangents and
 *   crthip_batch_bind_meshlet_bounds read.  Every decoded float position is int * q, so equality of the integers is the meaningful one.
 * remap[v] = the LEAST u with p[u] == p[v] in all three components, for every v < nvert: remap[v] <= v and remap[remap[v]] == remap[v].
 * index[k] (optional, always uint32, 3*nface words) = remap[id] if id < nvert, else id unchanged, where id is corner k of the blob's final
 *   index.  An id >= nvert is compared and never used as an address, as in adjacency.
 * crthip_weld_counts: vertices = nvert; unique = the number of v with remap[v] == v; degenerate = the number of faces whose WELDED triple
 *   has two equal corners or a corner >= nvert - adjacency's "invalid" rule on the welded index - and 0 for a binding without `index`, which
 *   forms no welded triple; reserved is written as 0.
 * Exactly nvert words of remap, 3*nface words of index and the 16 bytes of counts are written, nothing beyond them.  The position's own
 * output is unchanged, whatever its format (FLOAT packed or strided, an integer format, CRTHIP_BIND_QUANTIZED).
 * CRTHIP_WELD_ADJACENCY: in a decode where the blob has both this flag and an adjacency binding, the adjacency kernels read the welded index
 *   instead of the blob's own: twin and crthip_adjacency_counts are those of the welded index by adjacency's unchanged rule, and a face the
 *   weld collapses is an invalid face there (adjacency.invalid == 3 * weld.degenerate).  The flag is looked at when the decode is planned:
 *   the order of the two bind calls does not matter, and removing either binding removes the effect. */
#define CRTHIP_WELD_ADJACENCY 1u
typedef struct crthip_weld_counts { uint32_t vertices, unique, degenerate, reserved; } crthip_weld_counts;
typedef struct crthip_weld_binding {
	uint32_t *remap;                   /* DEVICE, 4-byte aligned, room for `remap_capacity` words */
	uint32_t *index;                   /* optional DEVICE array of the welded index, 4-byte aligned, room for `index_capacity` words; or NULL */
	crthip_weld_counts *counts;        /* optional DEVICE record for GPU-driven consumers: 16 bytes, 16-byte aligned; or NULL.  There is no host record */
	uint32_t remap_capacity;           /* words of remap: at least nvert */
	uint32_t index_capacity;           /* words of index: at least 3*nface when index is given */
	uint32_t flags;                    /* 0 or CRTHIP_WELD_ADJACENCY */
	uint32_t reserved;                 /* 0 */
} crthip_weld_binding;
/* Blob i's weld goes to w's buffers in the decode.  Call it after crthip_batch_bind of blob i; w == NULL removes the binding; a later
 * crthip_batch_bind of that blob drops it, as does crthip_batch_reset*.  The index itself may be bound as uint32, as uint16 or not at all (it
 * is then read from scratch).  Independent of every other derived binding's lifetime.  Every error is returned here, in this order, and
 * nothing new can fail at decode time.
 * CRTHIP_E_ARGUMENT: b NULL or i out of range; a point cloud (nface == 0); remap NULL or not 4-byte aligned; index not 4-byte aligned or
 * counts not 16-byte aligned; remap_capacity < nvert, or index given and index_capacity < 3*nface; unknown flag bits; reserved != 0;
 * CRTHIP_WELD_ADJACENCY without index.  CRTHIP_E_NORMAL_NEEDS_POSITION: no bound three-component generic "position", or one bound with
 * CRTHIP_BIND_STREAM_VALUES (the rule of crthip_batch_bind_meshlet_bounds).  crthip_last_error() names the blob.  Blobs without the binding
 * launch nothing new.
 * Not part of crthip_pool_* / crthip_output_layout, crthip_decode_host, the crt::Decoder facade or the veneers. */
int crthip_batch_bind_weld(crthip_batch *b, uint32_t i, const crthip_weld_binding *w);

/* Clustered levels of detail: up to CRTHIP_LOD_MAX_LEVELS coarser INDEX buffers into the blob's unchanged vertex buffers, built on the GPU in the
 * decode call by vertex clustering (meshopt_simplifySloppy's contract; kernels lod_blob, and lod_insert, lod_lookup, lod_faces, lod_keep,
 * lod_offsets, lod_scatter in crthip_kernel_times; csrc/lod.h has the source the kernels and the test hook share).  Integer work only; the bytes
 * are defined exactly.  p[v] is the delta-decoded INTEGER position of vertex v, as the weld reads it.
 * A binding has 1 to CRTHIP_LOD_MAX_LEVELS levels, each with a `shift` in 0..31, strictly increasing.  For one level of shift s:
 * cell(v) = (floor(p[v].x / 2^s), floor(p[v].y / 2^s), floor(p[v].z / 2^s)): an arithmetic shift of the signed coordinate.  -1 and 0 are never
 *   in one cell; -1 and -2^s are.
 * remap[v] (nvert words) = the LEAST vertex in v's cell.  With shift 0 it is the weld's remap to the byte.
 * The CLUSTERED TRIPLE of face f: each corner's id goes to remap[id] if id < nvert, else it stays as it is (compared, never used as an
 *   address); the face's own corner order is kept.  f is DEGENERATE if two of the three are equal or one is >= nvert.  Otherwise its KEY is the
 *   triple rotated so that its least id comes first, the orientation kept: (a,b,c), (b,c,a) and (c,a,b) are one key, (a,c,b) is another.  f is
 *   a DUPLICATE if a face below f has the same key.  Otherwise f is KEPT.
 * index holds the kept faces in increasing f, three uint32 words each: the clustered triple, not rotated.  Exactly 3*faces words are written
 *   and no word beyond them; every written word is < nvert.  The capacity must be at least 3*nface all the same.
 * crthip_lod_counts: cells = the number of v with remap[v] == v; faces, degenerate, duplicate as above: faces + degenerate + duplicate == nface.
 *   The record is optional and device-only, for indirect draws; as with the weld there is no host record.
 * The position's own output and every other output are unchanged. */
#define CRTHIP_LOD_MAX_LEVELS 4
typedef struct crthip_lod_counts { uint32_t cells, faces, degenerate, duplicate; } crthip_lod_counts;
typedef struct crthip_lod_level {
	uint32_t *remap;                   /* DEVICE, 4-byte aligned, room for `remap_capacity` words */
	uint32_t *index;                   /* DEVICE, 4-byte aligned, room for `index_capacity` words */
	crthip_lod_counts *counts;         /* optional DEVICE record: 16 bytes, 16-byte aligned; or NULL */
	uint32_t remap_capacity;           /* words of remap: at least nvert */
	uint32_t index_capacity;           /* words of index: at least 3*nface */
	uint32_t shift;                    /* 0..31, above the level's before */
	uint32_t reserved;                 /* 0 */
} crthip_lod_level;
typedef struct crthip_lod_binding {
	crthip_lod_level level[CRTHIP_LOD_MAX_LEVELS];
	uint32_t levels;                   /* 1..CRTHIP_LOD_MAX_LEVELS: level[0..levels) are read */
	uint32_t flags;                    /* 0 */
	uint32_t reserved[2];              /* 0 */
} crthip_lod_binding;
/* Blob i's levels go to l's buffers in the decode.  Call it after crthip_batch_bind of blob i; l == NULL removes the binding; a later
 * crthip_batch_bind of that blob drops it, as does crthip_batch_reset*.  The index itself may be bound as uint32, as uint16 or not at all.
 * Independent of every other derived binding.  Every error is returned here, in this order, and nothing new can fail at decode time.
 * CRTHIP_E_ARGUMENT: b NULL or i out of range; a point cloud (nface == 0); levels not in 1..CRTHIP_LOD_MAX_LEVELS; then per level, in level
 * order: remap or index NULL or not 4-byte aligned; counts not 16-byte aligned; remap_capacity < nvert or index_capacity < 3*nface; shift > 31;
 * shift not above the level's before; reserved != 0; then unknown flags or a reserved word not 0.  CRTHIP_E_NORMAL_NEEDS_POSITION: by the
 * weld's rule.  crthip_last_error() names the blob.  Blobs without the binding launch nothing new.
 * Not part of crthip_pool_* / crthip_output_layout, crthip_decode_host, the crt::Decoder facade or the veneers. */
int crthip_batch_bind_lod(crthip_batch *b, uint32_t i, const crthip_lod_binding *l);

/* Levels of detail of a POINT CLOUD: up to CRTHIP_CLOUD_LOD_MAX_LEVELS coarser point lists into the blob's unchanged vertex buffers, each a
 * subset of the points chosen on the integer grid, with a weight a kept point and a bounding box a run of kept points for GPU-driven culling,
 * built on the GPU in the decode call (kernels cloud_lod_blob, and cloud_lod_insert, cloud_lod_lookup, cloud_lod_offsets, cloud_lod_scatter,
 * cloud_lod_chunks in crthip_kernel_times; csrc/cloud_lod.h has the source the kernels and the test hook share).  Integer work only; the
 * bytes are defined exactly, for any order of the points.  p[v] is the delta-decoded INTEGER position of vertex v, as the weld reads it.
 * A binding has 1 to CRTHIP_CLOUD_LOD_MAX_LEVELS levels, each with a `shift` in 0..31, strictly increasing, and one chunk size K =
 * chunk_points for all of them.  For one level of shift s:
 * cell(v) is crthip_batch_bind_lod's: the arithmetic p[v] >> s a component.  -1 and 0 are never in one cell; -1 and -2^s are.
 * remap[v] (nvert words) = the LEAST vertex in v's cell: to the byte what crthip_lod_model gives as remap for the same positions, and with
 *   shift 0 the weld's remap.
 * points[j], j < cells: the vertices with remap[v] == v in increasing v.  Exactly `cells` words are written.
 * weight[j] (optional) = the number of v with remap[v] == points[j].  Exactly `cells` words are written; their sum is nvert.
 * chunks[c] (optional), c < ceil(cells / K): first = c*K; count = min(K, cells - first); min and max = the signed minimum and maximum a
 *   component of p[points[j]] over first <= j < first + count.  Exactly that many records are written.  A box over EVERY original point of
 *   those cells follows from it without another pass: (min >> s) << s and ((max >> s) << s) + 2^s - 1, a component.
 * counts (optional) = {points: nvert, cells, chunks: ceil(cells / K) if the level has a `chunks` array, else 0, reserved: 0}.  The record is
 *   device-only, for indirect draws; as with the weld there is no host record.
 * Nothing beyond the words named is written.  The position's own output and every other output are unchanged, whatever the position's
 * format (FLOAT packed or strided, an integer format, CRTHIP_BIND_QUANTIZED).
 * Across the levels k, k + 1 of one binding: remap_{k+1}[v] == remap_{k+1}[remap_k[v]], and the set points_{k+1} is a subset of points_k. */
#define CRTHIP_CLOUD_LOD_MAX_LEVELS 4
typedef struct crthip_cloud_lod_counts { uint32_t points, cells, chunks, reserved; } crthip_cloud_lod_counts;
typedef struct crthip_cloud_chunk { int32_t min[3]; uint32_t first; int32_t max[3]; uint32_t count; } crthip_cloud_chunk;
typedef struct crthip_cloud_lod_level {
	uint32_t *remap;                   /* DEVICE, 4-byte aligned, room for `capacity` words */
	uint32_t *points;                  /* DEVICE, 4-byte aligned, room for `capacity` words */
	uint32_t *weight;                  /* optional DEVICE array, 4-byte aligned, room for `capacity` words; or NULL */
	crthip_cloud_chunk *chunks;        /* optional DEVICE array, 16-byte aligned, room for `chunks_capacity` records; or NULL */
	crthip_cloud_lod_counts *counts;   /* optional DEVICE record: 16 bytes, 16-byte aligned; or NULL.  There is no host record */
	uint32_t capacity;                 /* words of remap, points and weight: at least nvert */
	uint32_t chunks_capacity;          /* records of chunks: at least ceil(nvert / chunk_points) when chunks is given */
	uint32_t shift;                    /* 0..31, above the level's before */
	uint32_t reserved;                 /* 0 */
} crthip_cloud_lod_level;
typedef struct crthip_cloud_lod_binding {
	crthip_cloud_lod_level level[CRTHIP_CLOUD_LOD_MAX_LEVELS];
	uint32_t levels;                   /* 1..CRTHIP_CLOUD_LOD_MAX_LEVELS: level[0..levels) are read */
	uint32_t chunk_points;             /* K: 32..65536, any integer; read only if some level has chunks, else it must be 0 or in that range */
	uint32_t flags;                    /* 0 */
	uint32_t reserved;                 /* 0 */
} crthip_cloud_lod_binding;
/* Blob i's levels go to l's buffers in the decode.  Call it after crthip_batch_bind of blob i; l == NULL removes the binding; a later
 * crthip_batch_bind of that blob drops it, as does crthip_batch_reset*.  Independent of every other derived binding.  Every error is returned
 * here, in this order, and nothing new can fail at decode time.
 * CRTHIP_E_ARGUMENT: b NULL or i out of range; a mesh (nface > 0: not a point cloud); nvert == 0; levels not in
 * 1..CRTHIP_CLOUD_LOD_MAX_LEVELS; chunk_points neither 0 nor in 32..65536, or 0 while some level has chunks; then per level, in level order:
 * remap or points NULL or not 4-byte aligned; weight not 4-byte aligned; chunks or counts not 16-byte aligned; capacity < nvert; chunks given
 * and chunks_capacity < ceil(nvert / chunk_points); shift > 31; shift not above the level's before; reserved != 0; then unknown flags or a
 * reserved word not 0.  CRTHIP_E_NORMAL_NEEDS_POSITION: by the weld's rule.  crthip_last_error() names the blob.  Blobs without the binding
 * launch nothing new; crthip_batch_bind_lod and the other derived bindings keep refusing a point cloud.
 * Not part of crthip_pool_* / crthip_output_layout, crthip_decode_host, the crt::Decoder facade or the veneers. */
int crthip_batch_bind_cloud_lod(crthip_batch *b, uint32_t i, const crthip_cloud_lod_binding *l);

/* COMPACTION: a level's own vertex buffers.  Every derived binding above ends in ids into the blob's unchanged, full-size vertex arrays; this
 * one renumbers the vertices an id list uses to 0..used-1, in vertex order, and copies the blob's FINAL vertex outputs of those vertices into
 * small contiguous arrays, on the GPU in the decode call (kernels compact_blob, and compact_mark, compact_count, compact_offsets,
 * compact_place, compact_index, and compact_gather in crthip_kernel_times; csrc/compact.h has the source the kernels and the test hook share).
 * It is meshopt_optimizeVertexFetchRemap's job in ascending order followed by meshopt_remapVertexBuffer's.  Integer and byte work only; every
 * byte is defined exactly, for any execution order.
 * A binding holds 1..CRTHIP_COMPACT_MAX_SETS sets; a set is one independent job and names a SOURCE, whose words are src[k]:
 *   CRTHIP_COMPACT_INDEX      the blob's final index (bound as uint32 or uint16, or unbound), k < 3*F with F = nface
 *   CRTHIP_COMPACT_WELD       the `index` of the blob's crthip_batch_bind_weld, F = nface
 *   CRTHIP_COMPACT_LOD        the `index` of level `level` of the blob's crthip_batch_bind_lod, F = that level's `faces`, read on the device
 *   CRTHIP_COMPACT_CLOUD_LOD  the `points` of level `level` of the blob's crthip_batch_bind_cloud_lod (a point cloud; see below)
 * For the three mesh sources:
 * vertex v < nvert is USED if some src[k] == v.  An id >= nvert is compared and never used as an address.
 * newid[v] (optional, nvert words) = the number of used u < v if v is used, else CRTHIP_NO_VERTEX.
 * order[j] (optional), j < used = the v with newid[v] == j: strictly ascending.
 * index[k] (optional), k < 3*F = newid[src[k]] if src[k] < nvert, else CRTHIP_NO_VERTEX.
 * counts (optional device record) = {vertices: nvert, used, faces: F, clipped}.  There is no host record, as with the weld.
 * For CRTHIP_COMPACT_CLOUD_LOD: used is the level's `cells` and order IS the level's `points`; newid, order and index must be NULL; the record
 * ({nvert, cells, 0, clipped}) and the gathers are all that is produced.
 * GATHERS: up to CRTHIP_COMPACT_MAX_GATHERS a set.  A gather names one of the blob's vertex outputs - attribute k of crthip_batch_info's
 * order, CRTHIP_COMPACT_COMPUTED_NORMALS or CRTHIP_COMPACT_COMPUTED_TANGENTS -, a DEVICE dst and a dst_stride S (0: packed, S = E).  The
 * element size E and its alignment A follow from the source's own binding: generic FLOAT 4*N and 4; generic CRTHIP_BIND_QUANTIZED 2*N and 2;
 * normal FLOAT 12 and 4; normal INT16 6 and 2; colour out_components and 1; tangents FLOAT 16 and 4; tangents INT16 8 and 2.  For
 * j < min(used, vertex_capacity) the E bytes at dst + j*S equal the E bytes of vertex order[j] in the source's buffer (packed or strided) at
 * the end of the decode.  With a stride only those E bytes are written, so several gathers of a set may fill one interleaved record.  dst
 * overlapping a source is the caller's error and is not checked.
 * CAPACITIES CLIP, they do not fail: vertex_capacity (records of order and of every gather's dst) and index_capacity (words of index) may be
 * any value.  order[j] and a gather's record j are written for j < min(used, vertex_capacity) only, index[k] for k < min(3*F, index_capacity)
 * only; nothing behind a capacity is ever touched.  clipped = 1 if used > vertex_capacity in a set with an order or a gather, or
 * 3*F > index_capacity in a set with an index; else 0.  used and faces are always the true values; the decode's status does not change.
 * Nothing beyond the bytes named is written, and no other output changes. */
#define CRTHIP_COMPACT_MAX_SETS 4
#define CRTHIP_COMPACT_MAX_GATHERS 8
#define CRTHIP_NO_VERTEX 0xFFFFFFFFu
enum { CRTHIP_COMPACT_INDEX = 0, CRTHIP_COMPACT_WELD = 1, CRTHIP_COMPACT_LOD = 2, CRTHIP_COMPACT_CLOUD_LOD = 3 };
#define CRTHIP_COMPACT_COMPUTED_NORMALS 0xFFFFFFFEu   /* a gather's source: what crthip_batch_bind_computed_normals bound */
#define CRTHIP_COMPACT_COMPUTED_TANGENTS 0xFFFFFFFDu  /* ... and crthip_batch_bind_computed_tangents */
typedef struct crthip_compact_counts { uint32_t vertices, used, faces, clipped; } crthip_compact_counts;
typedef struct crthip_compact_gather {
	void *dst;                         /* DEVICE, aligned to A, room for vertex_capacity records of stride S */
	uint32_t source;                   /* an attribute number, or CRTHIP_COMPACT_COMPUTED_NORMALS / _TANGENTS */
	uint32_t dst_stride;               /* 0: packed; else at least E and a multiple of A */
} crthip_compact_gather;
typedef struct crthip_compact_set {
	uint32_t *newid;                   /* optional DEVICE array, 4-byte aligned, room for newid_capacity words; or NULL */
	uint32_t *order;                   /* optional DEVICE array, 4-byte aligned, room for vertex_capacity words; or NULL */
	uint32_t *index;                   /* optional DEVICE array, 4-byte aligned, room for index_capacity words; or NULL */
	crthip_compact_counts *counts;     /* optional DEVICE record: 16 bytes, 16-byte aligned; or NULL.  There is no host record */
	uint32_t newid_capacity;           /* words of newid: at least nvert when newid is given */
	uint32_t vertex_capacity;          /* records of order and of every gather's dst: any value (it clips) */
	uint32_t index_capacity;           /* words of index: any value (it clips) */
	uint32_t source;                   /* CRTHIP_COMPACT_INDEX, _WELD, _LOD or _CLOUD_LOD */
	uint32_t level;                    /* the level of a _LOD or _CLOUD_LOD source; else 0 */
	uint32_t ngather;                  /* 0..CRTHIP_COMPACT_MAX_GATHERS: gather[0..ngather) are read */
	uint32_t reserved[2];              /* 0 */
	crthip_compact_gather gather[CRTHIP_COMPACT_MAX_GATHERS];
} crthip_compact_set;
typedef struct crthip_compact_binding {
	crthip_compact_set set[CRTHIP_COMPACT_MAX_SETS];
	uint32_t sets;                     /* 1..CRTHIP_COMPACT_MAX_SETS: set[0..sets) are read */
	uint32_t flags;                    /* 0 */
	uint32_t reserved[2];              /* 0 */
} crthip_compact_binding;
/* Blob i's sets go to c's buffers in the decode.  Call it after crthip_batch_bind of blob i, after the weld, lod or cloud lod binding a set
 * names and after the computed normals or tangents binding a gather names; c == NULL removes the binding.  The WHOLE binding is dropped by a
 * later crthip_batch_bind of that blob, by crthip_batch_reset*, and by any later call that sets, replaces or removes a binding it names
 * (crthip_batch_bind_weld, _lod, _cloud_lod, _computed_normals - which also drops the tangents -, _computed_tangents).  Every error is
 * returned here, in this order, and nothing new can fail at decode time.
 * CRTHIP_E_ARGUMENT: b NULL or i out of range; sets not in 1..CRTHIP_COMPACT_MAX_SETS, unknown flags, a reserved word of the binding not 0.
 * Then per set, in set order, CRTHIP_E_ARGUMENT: an unknown source, or a reserved word of the set not 0; a mesh source on a point cloud or the
 * cloud source on a mesh; the named weld binding missing or without `index`, the named lod or cloud lod level missing; for the cloud source
 * any of newid, order, index not NULL; newid, order or index not 4-byte aligned, or counts not 16-byte aligned; newid given and
 * newid_capacity < nvert; ngather > CRTHIP_COMPACT_MAX_GATHERS.  Then per gather of that set, in gather order: an attribute number out of
 * range (CRTHIP_E_ARGUMENT); a source that is unbound or missing (CRTHIP_E_ARGUMENT); a generic source in an integer format or DOUBLE, or
 * bound with CRTHIP_BIND_STREAM_VALUES - their buffers are upstream's in-place work arrays, not vertex records - (CRTHIP_E_FORMAT); dst NULL
 * or not A-aligned, or dst_stride neither 0 nor at least E and a multiple of A (CRTHIP_E_ARGUMENT).
 * crthip_last_error() names the blob, the set and the gather.  Blobs without the binding plan, upload, zero and launch nothing new.
 * Not part of crthip_pool_* / crthip_output_layout, crthip_decode_host, the crt::Decoder facade or the veneers. */
int crthip_batch_bind_compact(crthip_batch *b, uint32_t i, const crthip_compact_binding *c);

/* A binary triangle BVH of the blob's faces, built on the GPU in the decode call (kernels bvh_blob, and bvh_boxes, bvh_keys, bvh_sort_count,
 * bvh_sort_offsets, bvh_sort_scatter, bvh_tree, bvh_refit in crthip_kernel_times; csrc/bvh.h has the source the kernels and the hook share).
 * It is the structure for spatial queries - ray casts, picking, collision, box and frustum queries, a software ray tracer's bottom level -
 * and it is built from the INTEGER positions, so every byte below is defined exactly.
 * p[v] is the delta-decoded INTEGER position of vertex v, as the weld reads it; the index is the blob's final one; F = nface >= 1.  A face
 * is ABSENT if a corner is >= nvert (compared, never an address: only blobs whose topology failed have one); a face with two equal corners
 * is an ordinary face.
 * Box: bmin[f][c], bmax[f][c] = the signed minimum and maximum of component c over the three corners; an absent face has the EMPTY box,
 *   min = INT32_MAX and max = INT32_MIN in every component - the identity of the union, on which every overlap test fails.
 * Key: m[f][c] = (int32)(((int64)bmin[f][c] + bmax[f][c]) >> 1) (arithmetic); L[c], H[c] = the minimum and maximum of m[f][c] over the PRESENT
 *   faces; E = max over c of (uint32)H[c] - (uint32)L[c]; k = max(0, bitlength(E) - 10); cell[f][c] = ((uint32)m[f][c] - (uint32)L[c]) >> k
 *   (below 2^10); key[f] takes bit i of cell[f][0] at bit 3i + 2, of cell[f][1] at 3i + 1, of cell[f][2] at 3i, i in 0..9 (a 30-bit Morton
 *   code); an absent face has key 0x80000000.  If no face is present, L and H play no part.
 * Order: order[j] = the face of rank j when the faces are sorted by (key, f) ascending.
 * Tree (Karras 2012, stated without the algorithm): leaf j holds face order[j], its code is c_j = ((uint64)key[order[j]] << 32) | j.  For a
 *   range [a, b], a < b, let P = clz64(c_a ^ c_b); the split is the LARGEST m in [a, b - 1] with clz64(c_a ^ c_m) > P (clz64(0) = 64); the left
 *   child covers [a, m], the right [m + 1, b]; a range of one is a leaf; the root covers [0, F - 1].
 * Node ids: the root is node 0; an internal node reached as the LEFT child of a node with split m has id m, as the RIGHT child id m + 1; leaf
 *   j is node F - 1 + j; for F == 1 the only node is leaf 0 at id 0.  The internal ids fill 0..F - 2 exactly, and the longest root-to-leaf
 *   path has at most 64 edges.
 * nodes[n], n < 2F - 1: an internal node's left and right are its children's node ids and its box is the union of theirs (the empty box over
 *   absent faces only); a leaf's left is the face id, its right CRTHIP_BVH_LEAF, its box the face's.  A box is in grid units: the world box is
 *   (float)min * q to (float)max * q with the position's one step q, as with the meshlet bounds.
 * parent[n] (optional, 2F - 1 words) = the parent's node id, CRTHIP_NO_NODE for node 0.  order (optional, F words): what
 *   meshopt_spatialSortTriangles is called for.  counts (optional device record) = {nodes: 2F - 1, faces: F, absent, height}; height is the
 *   number of edges on the longest root-to-leaf path (0 for F == 1): a traversal stack of height + 1 entries suffices.  There is no host
 *   record, as with the weld.  Nothing beyond these is written, and no other output of the blob changes, whatever the position's format.
 * Chosen, not tuned: one workgroup builds a blob of up to 4 096 faces; bigger blobs sort in tiles of 2 048 faces, 8 bits a pass.
 * Left out: a BVH of the welded index or of a LOD level (flags is kept for that), refitting an existing tree, wide (4- or 8-way) nodes, SAH
 *   splits or treelet rotations, float boxes, point clouds. */
#define CRTHIP_BVH_LEAF 0xFFFFFFFFu
#define CRTHIP_NO_NODE 0xFFFFFFFFu
typedef struct crthip_bvh_node { int32_t min[3]; uint32_t left; int32_t max[3]; uint32_t right; } crthip_bvh_node;
typedef struct crthip_bvh_counts { uint32_t nodes, faces, absent, height; } crthip_bvh_counts;
typedef struct crthip_bvh_binding {
	crthip_bvh_node *nodes;            /* DEVICE array, 16-byte aligned, room for `node_capacity` records; 2*nface - 1 are written */
	uint32_t *parent;                  /* optional DEVICE array, 4-byte aligned, room for `node_capacity` words; or NULL */
	uint32_t *order;                   /* optional DEVICE array, 4-byte aligned, room for `order_capacity` words; or NULL */
	crthip_bvh_counts *counts;         /* optional DEVICE record: 16 bytes, 16-byte aligned; or NULL.  There is no host record */
	uint32_t node_capacity;            /* at least 2*nface - 1 */
	uint32_t order_capacity;           /* with order: at least nface */
	uint32_t flags;                    /* 0 */
	uint32_t reserved;                 /* 0 */
} crthip_bvh_binding;
/* Blob i's BVH goes to v's buffers in the decode.  Call it after crthip_batch_bind of blob i; v == NULL removes the binding; a later
 * crthip_batch_bind of that blob drops it, and so does crthip_batch_reset*.  It is independent of every other derived binding.  Every error
 * is returned here, in this order, and nothing new can fail at decode time.
 * CRTHIP_E_ARGUMENT: b NULL or i out of range; a point cloud; nodes NULL or not 16-byte aligned; parent or order not 4-byte aligned, or
 * counts not 16-byte aligned; node_capacity < 2*nface - 1; order given and order_capacity < nface; flags != 0 or reserved != 0.
 * CRTHIP_E_NORMAL_NEEDS_POSITION: by the weld's rule.  crthip_last_error() names the blob.  Blobs without the binding plan, upload, zero
 * and launch nothing new.  Not part of crthip_pool_* / crthip_output_layout, crthip_decode_host, the crt::Decoder facade or the veneers. */
int crthip_batch_bind_bvh(crthip_batch *b, uint32_t i, const crthip_bvh_binding *v);

/* SEGMENT CASTS against a blob's BVH: the nearest face a segment meets, or whether it meets any (kernel bvh_cast; csrc/bvh_cast.h has the
 * source the kernel and the hook share).  A stand-alone call on plain device pointers - the nodes crthip_batch_bind_bvh wrote, the blob's
 * position bound with CRTHIP_BIND_QUANTIZED (the one form in which the integers survive the decode), its index and the position's base -,
 * no part of a batch's plan: a batch that never casts launches what it launched before.  Everything is an integer in grid units, so every
 * byte below is defined exactly, for any traversal order; a segment through a shared edge or a vertex of a closed surface cannot slip through.
 * Frame: p[v][c] = base[c] + position[v][c] (the uint16 of the buffer).  With `transform`, base is transform->base, read on the DEVICE, and
 *   transform->written == 0 (a span beyond 65 535: there is no such buffer) gives every segment of the set CRTHIP_CAST_RANGE.
 * Range: a segment P -> Q is in range iff -2^19 <= E[c] - base[c] < 2^19 for both endpoints E and every c (in 64 bits).  Otherwise its record
 *   is {CRTHIP_CAST_RANGE, CRTHIP_NO_FACE, 0, 0, 0, 0} and nothing is tested.  In range every difference below is under 2^20 in magnitude.
 * Face test, a, b, c the corners of face f: d = Q - P, A = a - P, B = b - P, C = c - P, n = (B - A) x (C - A) (|n[c]| < 2^33), D = d . n and
 *   K = A . n (below 2^55 in magnitude), U = d . (B x C), V = d . (C x A), W = d . (A x B) (below 2^63 in magnitude; U + V + W = D).
 *   The segment HITS f iff D != 0; and U, V, W are all >= 0 or all <= 0; and K is 0 or has D's sign, and |K| <= |D| (t = K/D is in [0, 1]);
 *   and, under CRTHIP_CAST_FRONT, D < 0.  Edges, vertices and both endpoints are inclusive.  A face with a corner >= nvert is absent and
 *   never hit (the corner is compared, never an address); a face with two equal or three collinear corners has n = 0 and is never hit; a
 *   segment in a face's plane has D = 0 and misses it.
 * Nearest: among the hit faces the one with the least (t, f), where t1 < t2 iff |K1|*|D2| < |K2|*|D1| as 128-bit products.  Its record is
 *   {CRTHIP_CAST_HIT, f, side = (D < 0), 0, num = |K|, den = |D|} (not reduced); no hit: {CRTHIP_CAST_MISS, CRTHIP_NO_FACE, 0, 0, 0, 0}.
 * CRTHIP_CAST_ANY: {CRTHIP_CAST_HIT, CRTHIP_NO_FACE, 0, 0, 0, 0} if some face is hit, else the miss record (which face is found first
 *   changes with the schedule, so none is reported).
 * Tree: only a way to skip faces.  With the nodes crthip_batch_bind_bvh wrote for this index and these positions no answer depends on them.
 *   ANY bytes in `nodes` are survived: a child id >= 2*nface - 1, a leaf whose face id is >= nface, a traversal stack deeper than 65 entries
 *   or more than 2*nface - 1 nodes taken from it give {CRTHIP_CAST_TREE, CRTHIP_NO_FACE, 0, 0, 0, 0}; no access leaves the arrays and no
 *   loop is unbounded.
 * Chosen, not tuned: one thread a segment, one wave of 64 a workgroup, the stack in LDS.
 * Left out: float or world-space rays; infinite rays (clip to the range box); barycentric outputs; positions in any form but quantised
 *   uint16; instancing and a top-level structure over blobs; frustum queries (boxes: crthip_bvh_query, the closest face: crthip_bvh_closest); any-hit
 *   face ids; the pool, the facade
 *   and the veneers. */
#define CRTHIP_CAST_ANY    1u   /* any hit instead of the nearest */
#define CRTHIP_CAST_FRONT  2u   /* only faces the segment meets against their normal (D < 0) */
#define CRTHIP_NO_FACE 0xFFFFFFFFu
enum { CRTHIP_CAST_MISS = 0, CRTHIP_CAST_HIT = 1, CRTHIP_CAST_RANGE = 2, CRTHIP_CAST_TREE = 3 };
typedef struct crthip_segment  { int32_t p[3]; uint32_t user0; int32_t q[3]; uint32_t user1; } crthip_segment;   /* 32 bytes; the user words never reach a result */
typedef struct crthip_cast_hit { uint32_t status, face, side, reserved; uint64_t num, den; } crthip_cast_hit;    /* 32 bytes */
typedef struct crthip_bvh_cast_set {
	const crthip_bvh_node *nodes;          /* DEVICE, 16-byte aligned, 2*nface - 1 records as crthip_batch_bind_bvh wrote them */
	const void *position;                  /* DEVICE, uint16 x 3 a vertex (CRTHIP_BIND_QUANTIZED), 2-byte aligned */
	const void *index;                     /* DEVICE, nface*3 entries of index_format, aligned to an entry */
	const crthip_quant_transform *transform; /* DEVICE record of that position (crthip_batch_bind_quant_transforms), 16-byte aligned; or NULL: base[] */
	const crthip_segment *segments;        /* DEVICE, 16-byte aligned, nseg records */
	crthip_cast_hit *hits;                 /* DEVICE, 16-byte aligned, nseg records; nothing else is written */
	int32_t base[3]; uint32_t pos_stride;  /* 0 or 6: packed; else even and >= 6 */
	uint32_t nvert, nface, index_format, nseg;
	uint32_t flags, reserved;
} crthip_bvh_cast_set;
/* Casts every set - many blobs, any number of segments each - in ONE launch, asynchronously, on the context's main stream: behind everything
 * the context enqueued before (a crthip_batch_decode's last kernels run on that stream, so a decode followed by a cast with a `transform`
 * needs no host wait in between); crthip_ctx_sync waits for it.  `sets` is read before the call returns.  nsets == 0 and sets with
 * nseg == 0 write nothing.  Every error comes from this call, before anything is enqueued, in this order:
 * CRTHIP_E_ARGUMENT: ctx NULL; sets NULL with nsets > 0; then per set, in set order: with nseg > 0, nodes, position, index, segments or hits
 * NULL or misaligned, or transform misaligned; nface == 0 or beyond 2^31 - 1; index_format neither CRTHIP_FMT_UINT32 nor CRTHIP_FMT_UINT16;
 * pos_stride neither 0 nor even and >= 6; flags beyond the two; reserved != 0; then, with nseg > 0, an array that is not device memory of
 * the context's device with its whole extent inside one allocation (nodes (2*nface - 1)*32 bytes, position up to the last vertex's sixth
 * byte, index, the 48 bytes of transform, segments and hits nseg*32 bytes each).  CRTHIP_E_LIMIT: more than 2^31 - 1 workgroups of 64
 * segments in all.  crthip_last_error() names the set and the field. */
int crthip_bvh_cast(crthip_ctx *ctx, uint32_t nsets, const crthip_bvh_cast_set *sets);

/* BOX QUERIES against a blob's BVH: the faces that share a point with an axis-aligned box - rubber-band selection, a collision broad phase
 * of many small boxes, brick occupancy, "which faces lie in this tile" (kernel bvh_query; csrc/bvh_query.h has the source the kernel and the
 * hook share).  A stand-alone call like crthip_bvh_cast, on the same device pointers and in the same frame, no part of a batch's plan: a batch
 * that never queries launches what it launched before.  Everything is an integer in grid units and stays in signed 64 bits, so every byte
 * below is defined exactly.
 * Frame: crthip_bvh_cast's.  With `transform`, base is transform->base, read on the DEVICE, and transform->written == 0 gives every box of
 *   the set CRTHIP_QUERY_RANGE.
 * Range: a box is in range iff -2^19 <= E[c] - base[c] < 2^19 for both corners E = min, max and every c (in 64 bits).  Otherwise its record is
 *   {CRTHIP_QUERY_RANGE, 0, 0, 0} and nothing is tested.
 * Empty: an in-range box with min[c] > max[c] on some axis holds no point.  Its record is {CRTHIP_QUERY_OK, 0, 0, 0} and nothing is walked.
 * Match (default): face f matches iff it is present - every corner < nvert; the corner is compared, never an address - and its CLOSED triangle,
 *   the convex hull of its three corners, shares a point with the CLOSED box.  A face with equal or collinear corners is the segment or the
 *   point that it is.  Decided by separating axes on DOUBLED coordinates: c2 = min + max and h = max - min of the box, the corners
 *   V = 2p - c2 (|V[c]| < 2^21), the edges e0 = V1 - V0, e1 = V2 - V1, e2 = V0 - V2 (|e[c]| < 2^18).  NO match iff on a box axis c
 *   min V[c] > h[c] or max V[c] < -h[c]; or |n . V0| > sum h[c]|n[c]| for n = e0 x e1 (|n[c]| < 2^36, both sides below 2^59); or on one of
 *   the nine axes a = u_k x e_i (u_k the unit vector of axis k) the interval of the three a . V lies wholly beyond +-sum h[c]|a[c]| (below
 *   2^41).  Touching counts: a box that meets a face in one vertex, along an edge or in its plane only matches it.
 * CRTHIP_QUERY_BOXES: a present face matches iff its corner box overlaps the closed box on all three axes (the first of the tests above
 *   alone: a conservative broad phase).  CRTHIP_QUERY_INSIDE: a present face matches iff all three corners lie in the closed box.
 * Result of an in-range, non-empty box: count is the number of matching faces, whatever the capacity; written = min(count, face_capacity),
 *   or 0 under CRTHIP_QUERY_COUNT; the box's slice of `faces` holds the first `written` matching faces in ascending BVH RANK - the j of
 *   crthip_batch_bind_bvh's order[j], that is (key, f) ascending: the order in which a left-first walk of the tree meets them, a property of
 *   the tree and not of the schedule; status is CRTHIP_QUERY_CLIPPED if written < count without CRTHIP_QUERY_COUNT, else CRTHIP_QUERY_OK.
 *   The record is {status, count, written, 0}.  The words of a slice beyond `written` are not touched; nothing outside the `results` and
 *   `faces` extents is written.
 * Tree: only a way to skip faces - a node is taken iff its box (minus base, in 64 bits) overlaps the closed query box, the one use of the
 *   nodes.  With the nodes crthip_batch_bind_bvh wrote for this index and these positions no answer depends on them.  ANY bytes in `nodes` are
 *   survived under crthip_bvh_cast's four bounds: a child id >= 2*nface - 1, a leaf whose face id is >= nface, a traversal stack deeper than
 *   65 entries or more than 2*nface - 1 nodes taken give {CRTHIP_QUERY_TREE, 0, 0, 0}, and the box's slice is then unspecified within its
 *   face_capacity words; no access leaves the arrays and no loop is unbounded.
 * Chosen, not tuned: one thread a box, one wave of 64 a workgroup, the cast's depth-major stack in LDS, plain 4-byte stores into the thread's
 *   own slice.
 * Left out: frustum or plane-set queries (few large queries: they want a wave or a workgroup a query); the closest face (crthip_bvh_closest);
 *   one-query-many-lanes traversal; a shortcut for nodes wholly inside the box; lists in face-id order; a per-face bitmask output; a top
 *   level over blobs; the pool, the facade and the veneers. */
#define CRTHIP_QUERY_COUNT  1u  /* counts only: no list is written, faces may be NULL, face_capacity is ignored */
#define CRTHIP_QUERY_BOXES  2u  /* the face's own box stands for the face (conservative broad phase) */
#define CRTHIP_QUERY_INSIDE 4u  /* only faces whose three corners all lie in the closed box */
enum { CRTHIP_QUERY_OK = 0, CRTHIP_QUERY_CLIPPED = 1, CRTHIP_QUERY_RANGE = 2, CRTHIP_QUERY_TREE = 3 };
typedef struct crthip_box { int32_t min[3]; uint32_t user0; int32_t max[3]; uint32_t user1; } crthip_box;   /* 32 bytes: the bytes of a crthip_bvh_node are a valid box; the user words never reach a result */
typedef struct crthip_query_result { uint32_t status, count, written, reserved; } crthip_query_result;     /* 16 bytes */
typedef struct crthip_bvh_query_set {
	const crthip_bvh_node *nodes; const void *position; const void *index; const crthip_quant_transform *transform;   /* as in crthip_bvh_cast_set */
	const crthip_box *boxes;               /* DEVICE, 16-byte aligned, nbox records */
	crthip_query_result *results;          /* DEVICE, 16-byte aligned, nbox records */
	uint32_t *faces;                       /* DEVICE, 4-byte aligned, nbox*face_capacity words: box i owns words [i*face_capacity, (i+1)*face_capacity) */
	int32_t base[3]; uint32_t pos_stride;  /* 0 or 6: packed; else even and >= 6 */
	uint32_t nvert, nface, index_format, nbox;
	uint32_t face_capacity, flags, reserved[2];
} crthip_bvh_query_set;
/* Queries every set - many blobs, any number of boxes each - in ONE launch, asynchronously, on the context's main stream, with
 * crthip_bvh_cast's stream order (a decode followed by a query with a `transform` needs no host wait in between); crthip_ctx_sync waits for
 * it.  `sets` is read before the call returns.  nsets == 0 and sets with nbox == 0 write nothing.  Every error comes from this call, before
 * anything is enqueued, in this order:
 * CRTHIP_E_ARGUMENT: ctx NULL; sets NULL with nsets > 0; then per set, in set order: with nbox > 0, nodes, position or index NULL or
 * misaligned, transform misaligned, boxes or results NULL or misaligned, or - without CRTHIP_QUERY_COUNT and with face_capacity > 0 -
 * faces NULL or not 4-byte aligned (face_capacity == 0 without CRTHIP_QUERY_COUNT is legal: every match is clipped; under
 * CRTHIP_QUERY_COUNT or with face_capacity == 0 faces is not looked at); nface == 0 or beyond
 * 2^31 - 1; index_format neither CRTHIP_FMT_UINT32 nor CRTHIP_FMT_UINT16; pos_stride neither 0 nor even and >= 6; flags beyond the three,
 * or CRTHIP_QUERY_BOXES together with CRTHIP_QUERY_INSIDE; reserved != 0; then, with nbox > 0, an array that is not device memory of the
 * context's device with its whole extent inside one allocation (nodes, position, index and transform as in crthip_bvh_cast, boxes nbox*32
 * bytes, results nbox*16 bytes, and without CRTHIP_QUERY_COUNT and with face_capacity > 0, faces nbox*face_capacity*4 bytes).
 * CRTHIP_E_LIMIT: more than 2^31 - 1 workgroups of 64 boxes in all.  crthip_last_error() names the set and the field. */
int crthip_bvh_query(crthip_ctx *ctx, uint32_t nsets, const crthip_bvh_query_set *sets);

/* CLOSEST-FACE QUERIES against a blob's BVH: for a point, the face nearest to it, the squared distance as an exact fraction and the part of
 * the face - corner, edge, interior - that holds the closest point: snapping, proximity and clearance tests, collision response, distance
 * fields, mesh-to-mesh error (kernel bvh_closest; csrc/bvh_closest.h has the source the kernel and the hook share).  A stand-alone call like
 * crthip_bvh_cast, on the same device pointers and in the same frame, no part of a batch's plan: a batch that never asks launches what it
 * launched before.  Everything is an integer in grid units, so every byte below is defined exactly, for any traversal order.
 * Frame: crthip_bvh_cast's.  With `transform`, base is transform->base, read on the DEVICE, and transform->written == 0 gives every point of
 *   the set CRTHIP_CLOSEST_RANGE.
 * Range: a point is in range iff -2^19 <= p[c] - base[c] < 2^19 for every c (in 64 bits).  Otherwise its record is
 *   {CRTHIP_CLOSEST_RANGE, CRTHIP_NO_FACE, 0, 0, 0, 0, 0, 0} and nothing is tested.
 * Distance to one face: a face with a corner >= nvert is absent (the corner is compared, never an address).  For a present face with corners
 *   a, b, c let A_0 = a - P, A_1 = b - P, A_2 = c - P (|A[c]| < 2^20) and e_0 = A_1 - A_0, e_1 = A_2 - A_1, e_2 = A_0 - A_2.  The squared
 *   distance is that of the closest point of the CLOSED triangle (unique: a triangle is convex); a face with equal or collinear corners is
 *   the segment or the point that it is.  It is reported as num/den, NOT reduced, by the feature that holds the closest point, and `feature`
 *   is the least code whose closed feature holds it:
 *     0, 1, 2  the corners a, b, c    {|A_k|^2, 1}                           always a candidate
 *     3, 4, 5  the edges ab, bc, ca   {|A_i x e_i|^2, |e_i|^2}               iff |e_i|^2 > 0 and 0 <= -A_i . e_i <= |e_i|^2
 *     6        the interior           {(n . A_0)^2, |n|^2}, n = e_0 x e_1    iff |n|^2 > 0 and (A_i x e_i) . n >= 0 for all three i
 *   The candidates are met in the order 0 to 6 and one is taken only if it is STRICTLY less than the best so far; that gives the least code.
 *   Widths: n[c] below 2^33, |n|^2 below 2^68, n . A below 2^55, an interior num below 2^110, a side test (A_i x e_i) . n below 2^72 (a signed
 *   128-bit sum), an edge's num below 2^76 and its den below 2^34; num1*den2 against num2*den1 is below 2^178 and is compared in 256 bits.
 * Answer: the minimum over the present faces under the total order (num/den, f): at equal distance the least face id.  Its record is
 *   {CRTHIP_CLOSEST_HIT, f, feature, 0, num, den}, num and den as two 64-bit halves each.  No present face:
 *   {CRTHIP_CLOSEST_MISS, CRTHIP_NO_FACE, 0, 0, 0, 0, 0, 0}.
 * CRTHIP_CLOSEST_WITHIN: only faces with num/den <= r^2 count - inclusive -, r = min(point.radius, 2^21); every present face lies closer than
 *   2^21 to any in-range point, so a larger radius is no limit.  No face within the radius: the MISS record.  Without the flag `radius` is a
 *   user word and never reaches a result.
 * CRTHIP_CLOSEST_ANY (only together with CRTHIP_CLOSEST_WITHIN): {CRTHIP_CLOSEST_HIT, CRTHIP_NO_FACE, 0, 0, 0, 0, 0, 0} if some face is
 *   within the radius, else the MISS record (which face is found first changes with the schedule, so none is reported).
 * Tree: only a way to skip faces - a node is skipped iff the squared distance from P to its box (minus base, in 64 bits, each axis clamped at
 *   2^21) times den exceeds num of the best so far, strictly.  With the nodes crthip_batch_bind_bvh wrote for this index and these positions
 *   no answer depends on them, nor on the order in which children are visited.  ANY bytes in `nodes` are survived under crthip_bvh_cast's
 *   four bounds: a child id >= 2*nface - 1, a leaf whose face id is >= nface, a traversal stack deeper than 65 entries or more than
 *   2*nface - 1 nodes taken give {CRTHIP_CLOSEST_TREE, CRTHIP_NO_FACE, 0, 0, 0, 0, 0, 0}; no access leaves the arrays and no loop is unbounded.
 * Chosen, not tuned: one thread a point, one wave of 64 a workgroup, the cast's depth-major stack in LDS, every comparison of two distances
 *   through 256-bit products.  The nearer child is visited first (profiles/bvh_closest.md has the counts behind that).
 * Left out: the closest point's coordinates or barycentrics as outputs; k nearest faces and all-within-radius lists; signed distance or
 *   inside-outside; float points; a query over welded or LOD sources; a top level over blobs; several lanes a point; the pool, the facade
 *   and the veneers. */
#define CRTHIP_CLOSEST_WITHIN 1u  /* only faces within point.radius (inclusive) */
#define CRTHIP_CLOSEST_ANY    2u  /* with CRTHIP_CLOSEST_WITHIN: whether some face is within the radius, not which */
enum { CRTHIP_CLOSEST_MISS = 0, CRTHIP_CLOSEST_HIT = 1, CRTHIP_CLOSEST_RANGE = 2, CRTHIP_CLOSEST_TREE = 3 };
typedef struct crthip_point { int32_t p[3]; uint32_t radius; } crthip_point;   /* 16 bytes; without CRTHIP_CLOSEST_WITHIN radius is a user word */
typedef struct crthip_closest_hit { uint32_t status, face, feature, reserved; uint64_t num_lo, num_hi, den_lo, den_hi; } crthip_closest_hit;   /* 48 bytes, 16-byte units */
typedef struct crthip_bvh_closest_set {
	const crthip_bvh_node *nodes; const void *position; const void *index; const crthip_quant_transform *transform;   /* as in crthip_bvh_cast_set */
	const crthip_point *points;            /* DEVICE, 16-byte aligned, npoint records */
	crthip_closest_hit *hits;              /* DEVICE, 16-byte aligned, npoint records; nothing else is written */
	int32_t base[3]; uint32_t pos_stride;  /* 0 or 6: packed; else even and >= 6 */
	uint32_t nvert, nface, index_format, npoint;
	uint32_t flags, reserved;
} crthip_bvh_closest_set;
/* Answers every set - many blobs, any number of points each - in ONE launch, asynchronously, on the context's main stream, with
 * crthip_bvh_cast's stream order (a decode followed by this call with a `transform` needs no host wait in between); crthip_ctx_sync waits for
 * it.  `sets` is read before the call returns.  nsets == 0 and sets with npoint == 0 write nothing.  Every error comes from this call, before
 * anything is enqueued, in crthip_bvh_cast's order:
 * CRTHIP_E_ARGUMENT: ctx NULL; sets NULL with nsets > 0; then per set, in set order: with npoint > 0, nodes, position, index, points or hits
 * NULL or misaligned, or transform misaligned; nface == 0 or beyond 2^31 - 1; index_format neither CRTHIP_FMT_UINT32 nor CRTHIP_FMT_UINT16;
 * pos_stride neither 0 nor even and >= 6; flags beyond the two, or CRTHIP_CLOSEST_ANY without CRTHIP_CLOSEST_WITHIN; reserved != 0; then,
 * with npoint > 0, an array that is not device memory of the context's device with its whole extent inside one allocation (nodes, position,
 * index and transform as in crthip_bvh_cast, points npoint*16 bytes, hits npoint*48 bytes).  CRTHIP_E_LIMIT: more than 2^31 - 1 workgroups of
 * 64 points in all.  crthip_last_error() names the set and the field. */
int crthip_bvh_closest(crthip_ctx *ctx, uint32_t nsets, const crthip_bvh_closest_set *sets);

/* The record of attribute `attr` of blob i, bound with CRTHIP_BIND_QUANTIZED.  Valid after crthip_batch_sync of a decode: the kernels write
 * the records into the batch's pinned status block, beside the status words.  CRTHIP_E_ARGUMENT if that attribute was not bound
 * quantised in that decode, or the batch has not been decoded and synced. */
int crthip_batch_quant_transform(const crthip_batch *b, uint32_t i, uint32_t attr, crthip_quant_transform *out);
/* Optional: a DEVICE copy of the records for GPU-driven consumers.  device_records: room for sum(nattr) records, 16-byte aligned (else
 * CRTHIP_E_ARGUMENT); the record of blob i, attribute k is at index sum(nattr of blobs < i) + k - crthip_batch_bind_all's order.  Entries
 * of attributes not bound quantised are not touched.  NULL removes it; crthip_batch_reset* drops it. */
int crthip_batch_bind_quant_transforms(crthip_batch *b, void *device_records);

/* Enqueue the whole decode of the batch on the context's stream (asynchronous). */
int crthip_batch_decode(crthip_batch *b);
/* A lane that decodes a STREAM of batches on one context, pipelined over two of them: the decode of a batch has an entropy stage (the
 * Tunstall dictionaries and streams: reads the blobs, writes only the batch's own scratch) and a mesh stage (everything that writes the
 * bound outputs and the status), and this call enqueues the mesh stage of `cur` together with the entropy stage of `next` - where both
 * batches allow it INSIDE cur's kernels' grids, which leave most of the GPU empty, so that it costs the stream no time of its own (a pool's
 * contexts share a few hardware queues, and a queue runs one kernel at a time).  `next` is planned here like any decode (create / reset and
 * bind it first); `cur` must have been `next` of the call before.  next == NULL: cur's mesh stage alone (the last batch; crthip_batch_decode(cur)
 * does the same); cur == NULL: next's entropy stage alone (the first).  crthip_batch_sync / _done (cur) cover everything the call enqueued.
 * Two batch objects are alive on the context, so they must not share its per-call blocks: give one of them parity 1 (crthip_batch_set_parity,
 * once, before it is filled: create it with no blobs, set, then crthip_batch_reset).  Outputs, statuses and statistics are those of
 * crthip_batch_decode; what a context learns from a batch's flags (LDS slots of the automaton, the 32-bit delta layout) reaches the batch after
 * the next one.  $CORTO_CARRY=0: the entropy stage is enqueued as launches of its own. */
int crthip_batch_decode_with_next(crthip_batch *cur, crthip_batch *next);
/* Which of the context's two sets of per-call blocks (arena image, descriptors, scratch, status) the object uses: 0 (default) or 1. */
int crthip_batch_set_parity(crthip_batch *b, uint32_t parity);
/* Wait for completion and collect per-blob status: status[i] = CRTHIP_OK or CRTHIP_E_* (may be NULL).
 * Returns CRTHIP_OK if every blob decoded, else the first failing blob's code. */
int crthip_batch_sync(crthip_batch *b, int32_t *status);
/* Without waiting: 1 if crthip_batch_sync would return at once (the decode has finished, or none is in flight), 0 if it is still
 * running, <0 on error.  For callers that keep several batches in flight and refill whichever finishes first (crthip_pool). */
int crthip_batch_done(crthip_batch *b);

/* One-blob convenience with HOST output buffers: probe + plan + device decode + copy back.
 * This is what the crt::Decoder facade (include/corto/decoder.h of this repo) calls.
 * attrs == NULL: no attribute is bound (an index-only decode, like a Decoder nobody called set*() on).  Host buffers have
 * upstream's tightly packed layouts: a binding with a non-zero stride is refused with CRTHIP_E_ARGUMENT (strides are for
 * DEVICE vertex buffers, crthip_batch_bind). */
int crthip_decode_host(crthip_ctx *ctx, const uint8_t *blob, size_t len, const crthip_attr_binding *attrs,
                       void *index, uint32_t index_format);

/* Where the decoded arrays of a list of blobs lie in ONE output block: the layout crthip_pool_decode writes, and the one the pool's own lanes
 * use.  Host-only, needs no device: it reads the headers (crthip_probe) and returns the first failing blob's code, "(blob i)" in
 * crthip_last_error().  The rule:
 *   - every array starts on the next 256-byte multiple, blob after blob, a blob's attributes in info.attr order and its index behind them;
 *   - generic attributes (position, uv, radius, ...) are FLOAT, nvert*N*4 bytes; normals FLOAT, nvert*12 bytes - INT16, nvert*6 bytes,
 *     under CRTHIP_LAYOUT_RENDER; colour is UINT8 x 4, nvert*4 bytes;
 *   - the index is UINT32, nface*12 bytes - UINT16, nface*6 bytes, under CRTHIP_LAYOUT_RENDER where nvert < 65536; a cloud has none;
 *   - *total is the end of the last array rounded up to 256 (0 for no blobs).
 * attr: NULL, or sum(nattr) entries, blob after blob; index: NULL, or nblobs entries (bytes == 0 for a cloud).  out_components is what a
 * vertex holds in the array (N, 3 for a normal, 4 for colour; 3 for the index).  Any flag bit but CRTHIP_LAYOUT_RENDER: CRTHIP_E_ARGUMENT.
 * (No reference counterpart: upstream's callers size one buffer per attribute from nvert / nface, src/main.cpp:266-300.) */
#define CRTHIP_LAYOUT_RENDER 1u   /* crthip_pool_set_render_layouts' formats */
typedef struct { uint64_t offset, bytes; uint32_t format, out_components; } crthip_out_array;
int crthip_output_layout(uint32_t nblobs, const uint8_t *const *blobs, const uint32_t *lens, uint32_t flags,
                         crthip_out_array *attr, crthip_out_array *index, uint64_t *total);

/* ---- multi-GPU decode pool ------------------------------------------------------------------------
 * Upstream decodes one blob on one thread; its Decoder objects are independent (src/decoder.cpp:126-196 touches nothing
 * shared), so a list of blobs shards by blob with NO collective.  The pool is that, for the GPUs of one node: `ndevices`
 * devices, `depth` batches in flight per host thread and `threads_per_device` host threads per device, every batch on its
 * own context (crthip_ctx: own HIP streams, scratch, descriptors) with its own output block in that device's HBM.  All
 * threads of all devices pull tickets from ONE queue - an atomic counter - so a faster or less loaded GPU simply takes more steps:
 * no RCCL, no peer traffic.  Which item a ticket decodes is home-shard-first: pool device d prefers the items j with
 * j % ndevices == d (the shard resident in ITS HBM: give device_arena[d] for those and NULL elsewhere), and a device without a home
 * item takes the others' (and uploads them, since they are not resident there).  Worker threads are pinned to the CPUs of their GPU's
 * NUMA node when sysfs names one.
 * Groups.  A hardware queue runs one kernel at a time, and a decode's kernels last as long as their slowest blob's chain of dependent steps,
 * hardly longer for 512 blobs than for 256.  Where the pool's lanes outnumber the queues (single-stream, pipelined lanes) the rate is
 * queues / (a launch set's kernel time), so the pool pays that time once per GROUP: a lane call draws up to G tickets and decodes their items
 * as ONE batch object - the blob lists joined, first ticket first, every item's outputs bound into a block of its own (the lane's block holds G
 * of them; crthip_pool_decode: the item's destination).  G is 2 on such lanes and 1 elsewhere; $CORTO_POOL_GROUP = 1 .. 4, read by
 * crthip_pool_create, overrides it.  Every member remains a step of its own: one completion and one completion time (the group's members share
 * the instant), its own statuses, its own `done` call, its own device-to-host copy.  Extra tickets are drawn only while at least 2 x lanes x G
 * tickets are undrawn, so the end of a crthip_pool_run - the steps crthip_pool_lane_read shows - and a short crthip_pool_decode run one item a
 * call on all lanes.  A group's members are all resident on the lane's device (their device arenas may be separate allocations) or all
 * uploaded IN PLACE (crthip_pool_set_packed_host_blobs on and the members' blobs in at most 8 runs together: a copy a run,
 * crthip_ctx_set_packed_host_blobs); items whose blobs have to be gathered on the worker thread - scattered host blobs, or the switch off -
 * are decoded one a call as before.  A ticket that does not fit the group it was drawn for waits for the thread's next call.  A group that planning refuses for a blob's own fault is planned again one item a call, so that the bad item alone carries the code.
 * A lane whose groups turn out not to pipeline where its single items did (two items' dictionaries can exceed what a grid carries) returns to
 * one item a call for the rest of the run.  Nothing is deduplicated: two tickets that name the same item are uploaded and decoded twice.
 * Memory: every lane's output block holds G strides of the call's largest item block (plus an eighth), whether or not the call ever forms a
 * group - a short crthip_pool_decode and a lane back at one item a call keep the larger block - and with crthip_pool_set_outputs_to_host or
 * pageable host destinations the lane's pinned mirror is as large: for C4 items (32 MB a block) 72 MB of HBM a lane at G = 2 against 36 at
 * G = 1, and as much pinned host memory again where there is a mirror.  $CORTO_POOL_GROUP=1 gives the smaller blocks back.
 * devices == NULL: devices 0 .. ndevices-1.  A device id may repeat (several pool "devices" on one GPU: how the N > 1 path
 * is exercised on a one-GPU box). */
typedef struct crthip_pool crthip_pool;
int crthip_pool_create(uint32_t ndevices, const int *devices, uint32_t threads_per_device, uint32_t depth, crthip_pool **out);
void crthip_pool_destroy(crthip_pool *pool);
uint32_t crthip_pool_lanes(const crthip_pool *pool);     /* ndevices * threads_per_device * depth contexts */
/* "" or what crthip_pool_create found wrong with the hardware queues (also printed to stderr once): every context needs a queue of
 * its own, ROCm hands out $GPU_MAX_HW_QUEUES (default 4) per process and reads it when HIP initialises - a pool of 16 contexts on
 * the default runs at a fraction of its rate.  Contexts are counted per physical GPU (a device id may repeat). */
const char *crthip_pool_warning(const crthip_pool *pool);
/* The host CPUs of pool device `device_slot`'s NUMA node (what the pool pins that device's worker threads to): up to cap ids into
 * cpus, returns how many there are (0: sysfs names no node).  A caller that allocates the pinned input buffers of that device's shard
 * on one of these CPUs gets them on the memory next to the GPU's PCIe root (bench.py does). */
int64_t crthip_pool_device_cpus(const crthip_pool *pool, uint32_t device_slot, int32_t *cpus, size_t cap);
/* crthip_ctx_set_packed_host_blobs for every context of the pool (items handed to crthip_pool_run without device arenas). */
int crthip_pool_set_packed_host_blobs(crthip_pool *pool, int on);
/* SURVEY 8d's secondary region: every step of crthip_pool_run ends with ONE device-to-host copy of its decoded outputs into a pinned host block
 * of the lane (queued on the context's stream behind the kernels; a step is complete when the copy is), and crthip_pool_lane_read returns what
 * that copy delivered.  What a host-side consumer of the outputs sees - the reference's own region, decode() into host buffers
 * (src/main.cpp:266-300).  Off by default: outputs stay in HBM. */
int crthip_pool_set_outputs_to_host(crthip_pool *pool, int on);
/* SURVEY 8f3's render layouts for every lane's outputs: normals as int16 (upstream's NormalAttr INT16 output, src/normal_attribute.cpp:203-208,
 * 317-323) and the index as uint16 where a blob has fewer than 65 536 vertices (Decoder::setIndex(uint16_t *), include/corto/decoder.h:61) - 22 % fewer
 * output bytes for a C4 blob, which is what the secondary region's D2H copy moves.  crthip_pool_lane_read returns those bytes. */
int crthip_pool_set_render_layouts(crthip_pool *pool, int on);

/* One work item = one batch of blobs (HOST pointers, borrowed for the duration of crthip_pool_run / crthip_pool_decode).
 * device_arena: NULL -> every execution uploads the blobs (pageable or pinned host memory -> HBM) inside the step (SURVEY.md 8d's primary
 *                       region): one DMA copy at the head of the context's own stream, as crthip_batch_create does;
 *               else ndevices DEVICE pointers, entry d = the item's blobs already resident on pool device d in
 *               crthip_arena_layout order (an entry may be NULL: that device uploads). */
typedef struct {
	uint32_t nblobs;
	const uint8_t *const *blobs;
	const uint32_t *lens;
	const void *const *device_arena;
} crthip_pool_item;

typedef struct {
	double elapsed_s;            /* wall time from the completion of the last warm-up step to the completion of the last timed step:
	                                the pipeline is full at both ends (extra steps are queued behind the timed ones and drained untimed) */
	uint64_t steps;              /* timed steps completed (= the `steps` asked for) */
	uint64_t triangles, vertices;/* decoded by the timed steps: the steps whose TICKET number lies in [warmup, warmup + steps), whichever order they completed in
	                                (steps_per_device likewise).  elapsed_s is taken between COMPLETIONS number warmup and warmup + steps.  With equal items the
	                                two windows hold the same work; with items that differ, triangles / elapsed_s mixes them by the few steps that completed
	                                out of ticket order at either end (at most the batches in flight).  This holds at every group size, 1 included */
	uint64_t failed_blobs;       /* blobs (over all executed steps) whose status was not CRTHIP_OK */
	int32_t first_error;         /* first failing status seen, or CRTHIP_OK */
	uint32_t devices_used;       /* pool devices that completed at least one timed step */
	uint64_t steps_per_device[16];
	uint64_t topology_fallbacks;
	uint32_t poisoned_lanes;     /* contexts whose LAST executed step started from an output block the pool had just filled with 0xA5 on the
	                                context's stream: the last round of timed steps and the tail behind them are run that way, so what
	                                crthip_pool_lane_read returns afterwards was written by those steps and by nothing earlier */
	uint32_t pinned_devices;     /* pool devices whose worker threads were pinned to the CPUs of the GPU's NUMA node */
	float host_us_per_step;      /* host time per step and thread: plan (walk + bind) + enqueue, averaged over every executed step (a group's time is shared
	                                by its members: the host_*_us figures stay per step) */
	float host_plan_max_us;      /* the LONGEST single plan call (walk + the upload's enqueue + bind) of the run ... */
	float host_wait_us, host_finish_us, host_plan_us;   /* of a worker thread's time per step: waiting for one of its contexts to finish; harvesting it
	                                (sync, status); the walk + bind part of host_us_per_step */
	float host_launch_max_us;    /* ... and the longest single crthip_batch_decode call: a host thread that blocks inside the runtime shows here */
	uint64_t grouped_steps;      /* steps (over all executed ones, warm-up and tail included) that a lane decoded together with another step, as members of
	                                one batch object ("Groups" above); 0 when every call decoded one item */
} crthip_pool_report;

/* Decode every item exactly ONCE into memory the caller owns: the pool as a service.  No warm-up, no tail, no poisoning; the call blocks
 * until every item's outputs are complete and visible in dests[j].out (a host destination: the copy included) and the per-blob codes are
 * in `status`.  An item's block is laid out as crthip_output_layout says for its blobs, under CRTHIP_LAYOUT_RENDER when
 * crthip_pool_set_render_layouts is on (crthip_pool_set_outputs_to_host has no bearing: the destination decides).
 *   device destination (device_slot >= 0): `out` is device memory of pool device device_slot's GPU and only lanes of that slot draw the
 *     item.  The kernels write straight into it and nothing outside the arrays' extents: the gaps between arrays and [total, cap) keep
 *     the caller's bytes.  The caller's own work on the block has completed before the call ("Device buffers" above).
 *   host destination (CRTHIP_POOL_DEST_HOST): the item is drawn home-first (pool device j % ndevices), then by whichever device is free;
 *     it decodes into the lane's device block and ONE device-to-host copy of [0, total) follows the kernels on the context's stream -
 *     straight into `out` where that is pinned memory (hipPointerGetAttributes decides), else into the lane's pinned mirror and from there
 *     with a memcpy on the worker thread.  Bytes of [0, total) outside the arrays are unspecified; [total, cap) is untouched.
 *   items[j].device_arena[slot] is used as in crthip_pool_run when the decoding slot has one.
 * Scheduling is crthip_pool_run's: the same worker threads and pinning, groups of items a lane call where the list is long enough ("Groups"
 * above: a call of fewer than 2 x lanes x G items runs one item a call), lanes pipelined two batches a call where they are there
 * ($CORTO_CARRY=0 honoured); a worker takes its slot's device-destination items first, then its home host items, then the other slots'.
 * Before the first launch every destination is checked - CRTHIP_E_ARGUMENT for the call, the item named in crthip_last_error(), nothing
 * written: a NULL `out` with total > 0, `out` not 256-byte aligned, cap < total, a device_slot that is neither a pool device nor
 * CRTHIP_POOL_DEST_HOST, reserved != 0, a device destination that is not device memory of that slot's GPU or whose [out, out + total)
 * leaves its allocation (the runtime's pointer queries), a host destination that is device memory.  Overlapping destinations are the
 * caller's business.
 * Failures of one item do not stop the call: an item whose layout or planning fails (a blob the host walk refuses: magic, truncation,
 * alignment) gets that code in every one of its status entries and its destination is not written; a blob that fails on the device gets
 * its own code.  The call returns CRTHIP_OK in both cases; only CRTHIP_E_DEVICE, CRTHIP_E_NOMEM and the checks above fail it.
 *   status: NULL, or sum(nblobs) codes, item after item.
 *   done:   NULL, or called on a worker thread once per item - one that failed to plan included - after the item's outputs and statuses
 *           are final, with the slot that handled it and the item's nblobs codes.  Calls from different threads may overlap; it must
 *           not call into the pool.
 *   report: NULL, or the struct of crthip_pool_run: steps = nitems, elapsed_s the wall time from the first plan to the last completion,
 *           triangles / vertices of the items decoded, poisoned_lanes 0, the other fields as there.
 * Afterwards crthip_pool_lane_item returns -1 and crthip_pool_lane_read CRTHIP_E_ARGUMENT until the next crthip_pool_run; the two calls
 * may alternate freely on one pool. */
#define CRTHIP_POOL_DEST_HOST (-1)
typedef struct {
	void *out;                   /* the item's output block, laid out as crthip_output_layout says */
	uint64_t cap;                /* >= that layout's total */
	int32_t device_slot;         /* >= 0: `out` is device memory of pool device `device_slot`, and a lane of that slot decodes the item;
	                                CRTHIP_POOL_DEST_HOST: `out` is host memory (pinned or not), any device may decode the item */
	uint32_t reserved;           /* 0 */
} crthip_pool_dest;
typedef void (*crthip_pool_done_fn)(void *user, uint32_t item, uint32_t device_slot, const int32_t *status /* the item's nblobs codes */);
int crthip_pool_decode(crthip_pool *pool, uint32_t nitems, const crthip_pool_item *items, const crthip_pool_dest *dests,
                       int32_t *status, crthip_pool_done_fn done, void *user, crthip_pool_report *report);

/* The measuring loop (bench.py): decode warmup + steps batches drawn cyclically from the items (each device from its home items, see above; + a few more steps to
 * keep every context busy until the last timed completion), outputs into the contexts' own device blocks: every attribute bound in its natural format
 * (generic FLOAT, normal FLOAT, colour UINT8 x 4, index UINT32).  completion_s: NULL, or `steps` doubles that receive the
 * completion time of every timed step in seconds since the start of the timed region, in completion order.
 * Blocks until everything has drained.  Returns CRTHIP_OK or the first HIP / planning error (per-blob decode failures are
 * counted in the report, not returned). */
int crthip_pool_run(crthip_pool *pool, uint32_t nitems, const crthip_pool_item *items, uint64_t steps, uint64_t warmup,
                    crthip_pool_report *report, double *completion_s);

/* After a run every lane (context) still holds the outputs of the last step it executed: which item that was, on which pool
 * device, and a copy of one output array of one of its blobs to the host ("position", "normal", "color", "uv", ... or "index").
 * ("#tail": the last 256 bytes of the context's output block, behind every array - 0xA5 after a run, see poisoned_lanes.)
 * Returns bytes written / the item index, or <0.  This is how bench.py and the tests check what every GPU decoded. */
int64_t crthip_pool_lane_item(const crthip_pool *pool, uint32_t lane, uint32_t *device_slot);
int64_t crthip_pool_lane_read(crthip_pool *pool, uint32_t lane, uint32_t blob, const char *what, void *host_out, size_t cap);

/* ---- .crt writer (host only) -------------------------------------------------------------
 * Byte-identical to upstream's crt::Encoder (src/encoder.cpp:207-722) for positions, normals (all three predictions),
 * rgb/rgba colours, uvs, one generic "radius" attribute, groups, exif, entropy NONE/TUNSTALL, meshes and point clouds; more generic
 * attributes through crthip_encode_attrs below.
 * Lets tests and bench.py synthesise inputs without the reference library. */
typedef struct {
	uint32_t nvert, nface;
	const float *position;        /* nvert*3, required */
	const uint32_t *index;        /* nface*3, NULL for point clouds */
	int32_t position_bits;        /* >0: step = max extent / 2^bits (Encoder::addPositionsBits); else position_q */
	float position_q;
	const float *normal;          /* nvert*3 or NULL */
	int32_t normal_bits;
	int32_t normal_prediction;    /* 0 DIFF, 1 ESTIMATED, 2 BORDER */
	const uint8_t *color;         /* nvert*color_components or NULL */
	int32_t color_components;     /* 3 or 4 */
	int32_t color_bits[4];
	const float *uv;              /* nvert*2 or NULL */
	float uv_q;
	const float *radius;          /* nvert or NULL */
	float radius_q;
	const uint32_t *group_end;    /* ngroups end-face markers or NULL */
	uint32_t ngroups;
	int32_t entropy;              /* CRTHIP_ENTROPY_* */
	const char *exif;             /* "k\0v\0..." nexif pairs or NULL */
	uint32_t nexif;
	/* Group::properties (Encoder::addGroup(end, props), include/corto/encoder.h:75): group g has group_nprops[g] pairs, all pairs
	 * of all groups flat in group_props as "k\0v\0...".  Written sorted by key like upstream's std::map.  NULL: no properties. */
	const uint32_t *group_nprops;
	const char *group_props;
} crthip_mesh;
/* returns the blob size (also when out == NULL or cap is too small), or <0 */
int64_t crthip_encode(const crthip_mesh *mesh, uint8_t *out, size_t cap, uint32_t *out_nvert, uint32_t *out_nface);

/* Generic vertex attributes beyond crthip_mesh's fixed slots (additions within ABI 6): upstream's
 * Encoder::addAttribute(name, buffer, format, components, q, strategy) (include/corto/encoder.h:70, src/encoder.cpp:187-197).
 * Each one is written as a GENERIC attribute with the caller's N, q, strategy and, as its format byte, the input format.
 * Quantisation is upstream's `(int)(buffer[i]/q)` as compiled for x86-64 (include/corto/vertex_attribute.h:79-104):
 *   FLOAT                 (int)(x/q)                   float division, truncation; INT_MIN for NaN / out of range (cvttss2si)
 *   INT32, INT16, INT8    (int)((float)x/q)            the int -> float conversion rounds to nearest even above 2^24
 *   DOUBLE                (int)(x/(double)q)           double division, truncation; INT_MIN for NaN / out of range (cvttsd2si)
 * Checks upstream does not make (it throws "Unsupported format." or silently drops a duplicate name):
 *   CRTHIP_E_FORMAT    a UINT32 / UINT16 / UINT8 format (or any other value)
 *   CRTHIP_E_ARGUMENT  a name the mesh already produces (position, and normal / color / uv / radius where the mesh has them) or one
 *                      repeated in the list; q not finite and > 0; strategy bits other than CRTHIP_PARALLEL | CRTHIP_CORRELATED;
 *                      values == NULL with nvert > 0
 *   CRTHIP_E_LIMIT     a name of 0 or >= CRTHIP_NAME_MAX bytes; components 0 or > 16; more than CRTHIP_MAX_ATTRS attributes in all;
 *                      nvert*components >= 2^32; in the device encoders nvert*components > 2^26 (the value coder's bound)
 * A residual of exactly INT_MIN in a stream without CORRELATED (NaN / infinite / out-of-range inputs beside zeros) is undefined
 * upstream (encodeValues writes a 64-bit field, include/corto/cstream.h:128-133): no bytes are promised for it. */
typedef struct {
	const char *name;             /* NUL-terminated, 1..63 bytes */
	const void *values;           /* HOST (crthip_encode_batch_resident: DEVICE), nvert*components elements of `format`, packed (vertex-major) */
	uint32_t format;              /* CRTHIP_FMT_FLOAT, _DOUBLE, _INT32, _INT16 or _INT8 */
	uint32_t components;          /* 1..16 */
	float q;                      /* quantisation step */
	uint32_t strategy;            /* 0, CRTHIP_PARALLEL, CRTHIP_CORRELATED or both */
} crthip_generic_attr;
typedef struct {
	uint32_t nattr;
	const crthip_generic_attr *attr;
} crthip_attr_list;
/* crthip_encode plus the attributes of `extra`: extra == NULL or extra->nattr == 0 is crthip_encode, byte for byte */
int64_t crthip_encode_attrs(const crthip_mesh *mesh, const crthip_attr_list *extra, uint8_t *out, size_t cap,
                            uint32_t *out_nvert, uint32_t *out_nface);

/* ---- measurement / test hooks (not needed by integrators) ---- */
typedef struct {
	uint64_t arena_bytes;       /* compressed input resident in HBM */
	uint64_t output_bytes;      /* bytes of all bound outputs */
	uint64_t tunstall_in;       /* compressed bytes through the Tunstall kernel */
	uint64_t tunstall_out;      /* decoded symbol bytes out of it */
	uint64_t tunstall_tables;   /* probability-table header bytes (1 + 2*nsym + 8 per stream) */
	uint32_t tunstall_streams;
	uint64_t total_nvert, total_nface;
	uint64_t scratch_bytes;
	uint64_t clers_symbols;     /* decoded CLERS symbols over all mesh blobs */
	uint64_t split_bytes;       /* bytes of the split / vertex-id bit blocks */
	uint64_t topology_fallbacks;/* after crthip_batch_sync: mesh blobs whose CLERS automaton outgrew its LDS edge slots and was
	                               redone with the front in HBM (same results, slower) */
	float host_plan_us;         /* host time of the last crthip_batch_decode: job planning (descriptor build) ... */
	float host_stage_us;        /* ... pointer fix-up + staging of the descriptors ... */
	float host_launch_us;       /* ... and issuing the copies / kernel launches (asynchronous; no device wait) */
	float host_create_us;       /* host time of crthip_batch_create: header parse + bounds-checked walk of every blob */
	uint32_t topology_scale;    /* factor on the LDS edge slots this decode was planned with (1, 2, 4 ...): the context raises it
	                               after a batch with fallbacks, so that meshes with long fronts (handles, many boundary loops)
	                               stay in LDS from the next batch on, and lowers it again after a long run without any */
	uint32_t tunstall_dictionaries; /* Tunstall dictionaries the last decode BUILT: streams of a batch that carry the same probability table
	                               share one (the dictionary is a function of the table alone, src/tunstall.cpp:125-256), so this is
	                               <= tunstall_streams; $CORTO_TUN_SHARE=0 builds one per stream */
	uint32_t delta_redone;      /* after crthip_batch_sync: blobs with an attribute whose values, relative to vertex 0, left int16 (K-DELTA's LDS
	                               layout) and were redone on the 32-bit values in HBM (same results, slower); the context plans its next
	                               batches with 32-bit values in LDS when that happens */
	uint32_t delta_walked;      /* after crthip_batch_sync: blobs of which K-DELTA finished an attribute with its ROUND LOOP (a scan of affine maps: parents one or
	                               two vertices back) rather than its window of prefix sums: irregular connectivity (k_delta.hip; the name is rounds 3-4's, when the
	                               fallback was a walk along the stretches of the prediction graph) */
	uint32_t delta_wide;        /* 1: this decode was planned with 32-bit values in K-DELTA's LDS (the context had met such blobs, or $CORTO_DELTA_WIDE=1) */
	uint32_t descriptor_bytes;  /* the job descriptors of the last decode: one host -> HBM copy beside the blobs' own bytes (it shares their PCIe link) */
	uint32_t int16_streams;     /* log streams of the last decode whose values K-BIT handed on as int16 instead of int32: the stream's probability table holds no
	                               width above 16 bits (15 for per-component streams), and the reader is the LDS-resident K-DELTA / K-NRM ($CORTO_VALUES_I32=1: none) */
	uint32_t upload_copies;     /* host -> HBM copies crthip_batch_create / _reset enqueued for the blobs' bytes: 0 for resident blobs, 1 for gathered ones, the
	                               number of runs for packed host blobs (crthip_ctx_set_packed_host_blobs) */
	uint64_t upload_gathered_bytes; /* ... and the bytes it gathered into the context's pinned image first (0: every copy read the caller's memory in place) */
} crthip_batch_stats;
int crthip_batch_get_stats(const crthip_batch *b, crthip_batch_stats *s);

/* Per-kernel device time of the LAST crthip_batch_decode of this batch, measured with HIP events on the
 * context's stream.  Enable before decode with crthip_ctx_set_profiling(ctx, 1).  names[i] static strings. */
#define CRTHIP_MAX_KERNELS 32
typedef struct {
	uint32_t count;
	const char *name[CRTHIP_MAX_KERNELS];
	float ms[CRTHIP_MAX_KERNELS];
	uint32_t launches[CRTHIP_MAX_KERNELS];
} crthip_kernel_times;
int crthip_ctx_set_profiling(crthip_ctx *ctx, int enable);
int crthip_batch_kernel_times(crthip_batch *b, crthip_kernel_times *t);
/* The prediction triples of blob i of the last decode (upstream's index.prediction, include/corto/index_attribute.h:34-38,76: one Face
 * {a, b, c} per vertex in decode order - what VertexAttribute::deltaDecode takes as its context): nvert*3 uint32 copied to HOST memory;
 * returns the bytes written (0 for a point cloud), < 0 on error.  Valid until the context's next decode. */
int64_t crthip_batch_read_prediction(crthip_batch *b, uint32_t i, void *host_out, size_t cap);

/* Copy an internal intermediate of blob i to a HOST buffer (tests compare these with the oracle):
 * what = "clers" (u8 symbols), "prediction" (nvert*3 u32). Returns bytes written or <0. */
int64_t crthip_batch_debug_read(crthip_batch *b, uint32_t i, const char *what, void *host_out, size_t cap);

/* Stand-alone Tunstall run on DEVICE-resident blocks, used for the HBM-roofline measurement of the
 * Tunstall kernels: n blocks, each "u8 nsym | nsym*(sym,prob) | u32 size | u32 csize | payload"
 * exactly as in the .crt stream (src/cstream.cpp:89-109), block_offset[i] bytes into device_blocks;
 * out_offset[i] bytes into device_out.  host_blocks is the same memory on the host (for framing). */
int crthip_tunstall_decode_blocks(crthip_ctx *ctx, uint32_t n, const uint8_t *host_blocks, const void *device_blocks,
                                  const uint64_t *block_offset, void *device_out, const uint64_t *out_offset,
                                  crthip_kernel_times *times);
int crthip_ctx_sync(crthip_ctx *ctx);

/* GPU encoder stage: the entropy coder of crt::Encoder for a batch of n byte streams, i.e.
 * OutStream::tunstall_compress (src/cstream.cpp:89-109) n times: byte histogram and greedy Tunstall parse
 * (Tunstall::getProbabilities / compress, src/tunstall.cpp:83-115, 384-428) run on the device, one wave per stream;
 * the 256-word dictionary and its trie (src/tunstall.cpp:125-256, 335-382) are built on the host in between.
 * src[i] / sizes[i]: HOST symbol arrays (<= 2^23 symbols each).  Writes the n blocks back to back into out
 * ("u8 nsym | nsym*(sym,prob) | i32 size | i32 csize | codewords", byte-identical to the reference's), their
 * starts into block_offset[0..n] (n+1 entries), and returns the total size, or <0.  out == NULL sizes only.
 * No CPU fallback: CRTHIP_E_DEVICE without a HIP device. */
int64_t crthip_tunstall_encode_blocks(crthip_ctx *ctx, uint32_t n, const uint8_t *const *src, const uint32_t *sizes,
                                      uint8_t *out, size_t cap, uint64_t *block_offset, crthip_kernel_times *times);

/* GPU encoder stage: the value coders of crt::Encoder for a batch of integer arrays - OutStream::encodeArray<int>
 * (one bit width per element, include/corto/cstream.h:143-164), OutStream::encodeValues<int|char> (component-major, one
 * width per value, sign folded, :115-141) and plain symbol streams.  Bit widths and bit packing (src/bitstream.cpp:86-101)
 * run on the device; the width arrays go through the Tunstall coder above without leaving HBM (entropy 1), or are
 * written raw (entropy 0, src/cstream.cpp:43-64).
 * Stream i is written as  "u32 nwords | nwords x u32 | block(s)"  (symbol streams: the block alone).  The reference pads
 * with zeros to a 4-byte stream position between nwords and the words (OutStream::write(BitStream&), cstream.h:79-89);
 * that depends on where the caller puts the stream, so it is the caller's to insert.  Returns the total size or <0. */
#define CRTHIP_ENC_SYMBOLS 0u       /* count bytes */
#define CRTHIP_ENC_ARRAY 1u         /* count x components int32, encodeArray */
#define CRTHIP_ENC_VALUES_I32 2u    /* count x components int32, encodeValues<int> */
#define CRTHIP_ENC_VALUES_I8 3u     /* count x components int8, encodeValues<char> (colours) */
typedef struct crthip_enc_stream {
	uint32_t kind, count, components, reserved;
	const void *values;             /* HOST pointer */
} crthip_enc_stream;
int64_t crthip_encode_values(crthip_ctx *ctx, uint32_t entropy, uint32_t n, const crthip_enc_stream *streams,
                             uint8_t *out, size_t cap, uint64_t *stream_offset, crthip_kernel_times *times);

/* crthip_encode with the value coding and the entropy coder on the device (the topology pass, quantisation and the
 * container stay on the host): same arguments plus the context, byte-identical output. */
int64_t crthip_encode_gpu(crthip_ctx *ctx, const crthip_mesh *mesh, uint8_t *out, size_t cap, uint32_t *out_nvert, uint32_t *out_nface);
/* crthip_encode_gpu with generic attributes (crthip_encode_attrs; ABI 6 addition); the quantisation runs on the device too */
int64_t crthip_encode_gpu_attrs(crthip_ctx *ctx, const crthip_mesh *mesh, const crthip_attr_list *extra, uint8_t *out, size_t cap,
                                uint32_t *out_nvert, uint32_t *out_nface);

/* A batch of meshes and point clouds in, one .crt per item out, every blob byte-identical to crthip_encode of that item.
 * The CLERS topology pass runs on `host_threads` host threads (0: min(16, CPUs of the process's affinity mask)) while the
 * device quantises (or on the device, where the context says so: crthip_ctx_set_encode_topology below); estimated normals, residuals, the point clouds' Morton sort and the value / Tunstall coders run on the
 * device, all meshes in one set of launches (each point cloud sorted by launches of its own).  Blob i is
 * out[blob_offset[i] .. blob_offset[i+1]) (n+1 offsets); the call returns the total size, writes only when cap suffices,
 * and out == NULL sizes only.
 * Per mesh: crthip_encode's argument checks, a Tunstall stream over 2^23 symbols (CRTHIP_E_LIMIT), or more than 2^26 / 3
 * vertices (CRTHIP_E_LIMIT: the device value coder's bound on an array; crthip_encode has none) put that CRTHIP_E_* in
 * status[i] (may be NULL) and give the mesh an empty range; the others are still encoded.  < 0 for the call: null context, no
 * device, a mesh too big for the device (CRTHIP_E_LIMIT).  No CPU fallback.
 * Equal Morton keys (duplicate quantised points, coordinates beyond 21 bits): std::sort leaves those in an order no device
 * sort reproduces, so such a cloud is ordered by the host's std::sort (clouds_host_sorted). */
typedef struct {
	float wall_ms;                 /* the whole call */
	float host_topology_ms;        /* wall time of the host topology passes (they overlap the device work) */
	float host_frame_ms;           /* headers, groups, CLERS / split splicing, zero padding */
	uint32_t clouds_device_sorted; /* point clouds whose Morton order came from the device sort */
	uint32_t clouds_host_sorted;   /* ... from the host std::sort (equal keys) */
	uint32_t value_streams;        /* streams through the value coder / Tunstall coder in this call */
	uint64_t bytes_to_device, bytes_from_device;
	float host_check_ms;           /* argument checks, position steps and attribute tables, before any device work */
	float host_stage_ms;           /* host copies into the upload buffers (raw attributes, faces, quads, CLERS) */
	float sync_wait_ms;            /* blocked on the device in the batch's own stages (uploads, sorts, residuals, read-backs) */
	float value_coder_ms;          /* wall time of the value + Tunstall coders, their copies included */
	float upload_ms;               /* in the uploads of raw attributes, faces and quads (a copy from pageable memory returns when staged) */
	float alloc_ms;                /* allocating the device image */
	float topology_wait_ms;        /* waiting for topology passes that had not finished when the device stages needed them */
	uint32_t topology_device;      /* meshes whose topology pass ran on the device in this call (crthip_ctx_set_encode_topology) */
	uint32_t topology_lds;         /* ... those of them whose walk state was LDS-resident */
	float device_topology_ms;      /* wall time from the first topology launch to the arrival of the meshes' counts on the host */
} crthip_encode_batch_stats;
int64_t crthip_encode_batch(crthip_ctx *ctx, uint32_t n, const crthip_mesh *meshes, uint32_t host_threads,
                            uint8_t *out, size_t cap, uint64_t *blob_offset, uint32_t *out_nvert, uint32_t *out_nface,
                            int32_t *status, crthip_encode_batch_stats *stats, crthip_kernel_times *times);
/* crthip_encode_batch with generic attributes (ABI 6 addition): extra holds n lists, mesh i gets extra[i] (NULL: none at all);
 * blob i is byte-identical to crthip_encode_attrs(&meshes[i], &extra[i]).  A mesh whose list breaks a rule of crthip_encode_attrs
 * gets that code in status[i] and an empty range; the others are still encoded. */
int64_t crthip_encode_batch_attrs(crthip_ctx *ctx, uint32_t n, const crthip_mesh *meshes, const crthip_attr_list *extra, uint32_t host_threads,
                                  uint8_t *out, size_t cap, uint64_t *blob_offset, uint32_t *out_nvert, uint32_t *out_nface,
                                  int32_t *status, crthip_encode_batch_stats *stats, crthip_kernel_times *times);

/* crthip_encode_batch_attrs for meshes that live in DEVICE memory (ABI 6 addition): a simulation's or a reconstruction's output, a
 * decoded batch being re-quantised.  Arguments and results are those of crthip_encode_batch_attrs (extra: n lists or NULL), and blob i is
 * byte-identical to crthip_encode_attrs of the same arrays held in host memory.  What differs: the DATA arrays are device pointers on the
 * context's device - position, index, normal, color, uv, radius and every crthip_generic_attr.values.  The metadata stays in host memory:
 * group_end, group_nprops, group_props, exif, the names and the structs themselves; out, blob_offset, out_nvert, out_nface and status
 * are host memory as before.  Nothing of the arrays is staged or copied up: the quantiser and the device topology pass read them where
 * they are, and what the host encoder reads from them before it quantises - the index range check, the bounding box or the mean first-edge
 * length behind the position step - is computed on the device (kernels enc_input_check, enc_input_reduce in crthip_kernel_times; upstream's
 * arithmetic in upstream's order, NaN, infinities and the sign of a zero included) and comes back as one record per item.  Meshes whose
 * topology pass runs on the host pool (crthip_ctx_set_encode_topology: all of them by default, under SPLIT those beyond LDS) have their index
 * copied back for it (bytes_from_device); attributes never come back.  The three modes give the same bytes.
 * The caller's rules:
 *   - every array is aligned to its element size: 4 bytes for float / uint32 / int32, 8 for double, 2 for int16 (colours and int8: none),
 *     else CRTHIP_E_ARGUMENT in status[i];
 *   - every non-empty array is device memory of the context's device (pinned or managed host memory is refused: host arrays belong to
 *     crthip_encode_batch) and its whole extent lies inside one allocation, else CRTHIP_E_ARGUMENT in status[i]: both are checked with
 *     the runtime's pointer queries before the first launch (their cost, about five queries a mesh, is part of host_check_ms, as is the
 *     input pass), so a wrong pointer is an error code and never a device fault;
 *   - the caller's writes to the arrays have completed before the call ("Device buffers" above); the call returns with everything it
 *     queued drained, as crthip_encode_batch does;
 *   - the library never writes to the caller's arrays;
 *   - with nvert == 0 the position pointer only has to be non-NULL and is never dereferenced: the step of position_bits > 0 is then 0.0f,
 *     which is what the host computes from any finite position[0].
 * Per-mesh errors keep their codes: a face index >= nvert, now found on the device, is CRTHIP_E_ARGUMENT with an empty range, and the
 * neighbouring meshes are still encoded.  The blobs are spliced on the host and returned in host memory (crthip_encode_batch_to_device
 * below leaves them in device memory). */
int64_t crthip_encode_batch_resident(crthip_ctx *ctx, uint32_t n, const crthip_mesh *meshes, const crthip_attr_list *extra /* n lists or NULL */,
                                     uint32_t host_threads, uint8_t *out, size_t cap, uint64_t *blob_offset, uint32_t *out_nvert,
                                     uint32_t *out_nface, int32_t *status, crthip_encode_batch_stats *stats, crthip_kernel_times *times);

/* crthip_encode_batch_attrs / crthip_encode_batch_resident with the blobs left in DEVICE memory (ABI 6 addition): the containers are
 * spliced on the GPU (kernel enc_splice in crthip_kernel_times) from where the coders made their payload, so a producer on the GPU can hand
 * its blobs to crthip_batch_create_resident without a copy back and a copy up.  Only what the host needs to lay the containers out comes
 * back (the streams' word and codeword counts, the Tunstall tables' records); what the host makes itself - frames, word counts, padding,
 * split words, block headers - goes up once, as one literal buffer beside the job table.
 *   flags       0: the data arrays of meshes / extra are HOST arrays, as in crthip_encode_batch_attrs;
 *               CRTHIP_ENCODE_INPUTS_RESIDENT: they are DEVICE arrays - the rules, checks and per-mesh errors of crthip_encode_batch_resident;
 *               any other bit: CRTHIP_E_ARGUMENT
 *   device_out  16-byte aligned device memory of the context's device, [device_out, device_out + cap) inside one allocation: checked with
 *               the runtime's pointer queries before the first launch, else CRTHIP_E_ARGUMENT for the call and never a fault.  NULL sizes only.
 *   blob_offset, blob_len   n entries each, HOST memory: blob i is the blob_len[i] bytes at device_out + blob_offset[i], byte-identical to
 *               crthip_encode_attrs of that item.  The offsets are crthip_arena_layout(n, blob_len, ...): every blob starts on a 16-byte multiple,
 *               and the bytes from a blob's end to the next multiple are written as zeros - crthip_batch_create_resident(ctx, n, device_out,
 *               blob_offset, blob_len, ...) takes the three arrays as they are.
 * Returns the arena's total (what crthip_arena_layout returns).  When it exceeds cap nothing is written to device_out and the total is still
 * returned, as crthip_encode_batch does.  A failed mesh gets its code in status[i] and blob_len[i] = 0; its neighbours are still encoded.
 * The three topology modes give the same bytes.  The call returns with everything it queued drained.  out_nvert, out_nface, status,
 * stats and times are crthip_encode_batch's (host_frame_ms: the plan; bytes_to_device includes the literal buffer, literal_bytes, and the
 * job table: 24 bytes a piece and 4 a tile start, pieces + 1 of them - nothing else goes up for the splice).
 * When not to use it: a caller who wants the blobs in host memory anyway (a file, a socket) - crthip_encode_batch copies back once;
 * this call followed by a copy back moves the same bytes and adds a launch. */
#define CRTHIP_ENCODE_INPUTS_RESIDENT 1u   /* the data arrays are DEVICE pointers: the rules of crthip_encode_batch_resident */
int64_t crthip_encode_batch_to_device(crthip_ctx *ctx, uint32_t n, const crthip_mesh *meshes, const crthip_attr_list *extra /* n lists or NULL */,
                                      uint32_t host_threads, uint32_t flags, void *device_out, size_t cap,
                                      uint64_t *blob_offset /* n */, uint32_t *blob_len /* n */, uint32_t *out_nvert, uint32_t *out_nface,
                                      int32_t *status, crthip_encode_batch_stats *stats, crthip_kernel_times *times);
/* Bytes that the arena total of crthip_encode_batch_to_device with the same arguments can never exceed, from the descriptors alone (host
 * only, no device; with resident inputs the data arrays are not read): allocate once instead of encoding twice.  Per item: the container
 * without its streams (header, attribute table, groups with their properties, exif) + CRTHIP_TOPOLOGY_CLERS_CAP(nface) symbols +
 * CRTHIP_TOPOLOGY_SPLIT_CAP(nface) words + per value stream count*N + 1 bit words (the value coder's own check) + per Tunstall block
 * 9 + 2*256 + size + 1 bytes (the Tunstall coder's own check; 4 + size under entropy NONE) + 15 bytes of padding.  A mesh the checks of
 * crthip_encode_batch would refuse from its descriptor contributes 0.
 * The bound of crthip_encode_batch_layout is this one: a crthip_mesh_layout changes neither nvert nor nface nor any attribute's
 * component count, and nothing else enters the sum. */
uint64_t crthip_encode_batch_bound(uint32_t n, const crthip_mesh *meshes, const crthip_attr_list *extra);

/* ---- render-ready inputs (additions within ABI 6) ------------------------------------------------------------------
 * How the DATA arrays of a crthip_mesh are read, for callers who keep their meshes in the form the decoder writes through
 * crthip_attr_binding.stride: one interleaved vertex buffer (position f32x3, normal i16x3, uv f32x2, rgba8), a uint16 index.  The
 * conversions are upstream's own, each ONE IEEE float operation:
 *   CRTHIP_IN_INDEX_UINT16   Encoder::addPositions(buffer, const uint16_t *index, q, o), src/encoder.cpp:114-119: every entry widened to
 *                            uint32.  The range check stays `entry >= nvert`; nvert may exceed 65536.  The array is 2-byte aligned.
 *   CRTHIP_IN_NORMAL_INT16   Encoder::addNormals(const int16_t *, bits, prediction), src/encoder.cpp:151-158: each component becomes
 *                            (float)v / 32767.0f, then the float path runs; the header's format byte stays FLOAT.  2-byte aligned.
 *   origin                   the `o` of every addPositions overload, src/encoder.cpp:77-81: coords[i] = input[i] - o per component, in
 *                            float, before quantisation.  A cloud's position_q == 0 recipe (the bounding box, :83-91) runs on input - o;
 *                            a mesh's (the first edges, :101-111) on the raw positions.  Upstream's addPositionsBits has no origin:
 *                            position_bits > 0 with a non-zero origin is CRTHIP_E_ARGUMENT, as is an origin that is not finite.
 *   strides                  (no upstream counterpart: the mirror of crthip_attr_binding.stride) element i of an array lies at
 *                            base + i*stride.  A stride is a multiple of the element's alignment - 4 for float / int32, 8 for double, 2 for
 *                            int16, 1 for colours and int8 - and at least one vertex's bytes of that array (12 for a float position, 6 for
 *                            an int16 normal, components * element size for a generic attribute), else CRTHIP_E_ARGUMENT.
 * A blob is byte-identical to crthip_encode_attrs of the same data converted as above into packed arrays.  An all-zero layout (or a NULL
 * one) is exactly what crthip_mesh means today. */
#define CRTHIP_IN_INDEX_UINT16  1u   /* crthip_mesh.index points at nface*3 uint16_t */
#define CRTHIP_IN_NORMAL_INT16  2u   /* crthip_mesh.normal points at int16_t triples */
typedef struct {
	uint32_t flags;                  /* the two bits above; any other bit: CRTHIP_E_ARGUMENT */
	uint32_t position_stride, normal_stride, color_stride, uv_stride, radius_stride;
	                                 /* bytes from one vertex to the next, 0 = packed */
	const uint32_t *attr_stride;     /* NULL, or one stride per entry of the mesh's crthip_attr_list */
	float origin[3];                 /* upstream's `o`: coords[i] = input[i] - o, per component, in float */
} crthip_mesh_layout;
/* crthip_encode_attrs on HOST arrays read through `layout` (NULL or all zero: crthip_encode_attrs' bytes).  A refused layout returns its code
 * and writes nothing. */
int64_t crthip_encode_layout(const crthip_mesh *mesh, const crthip_attr_list *extra, const crthip_mesh_layout *layout, uint8_t *out, size_t cap,
                             uint32_t *out_nvert, uint32_t *out_nface);
/* The batch encoder on arrays read through layouts[i] (layouts: n entries, or NULL for none).
 *   flags   CRTHIP_ENCODE_INPUTS_RESIDENT: the data arrays are DEVICE arrays (the rules of crthip_encode_batch_resident), read WHERE THEY LIE:
 *             nothing is de-interleaved, widened or staged on the device - enc_quantize_batch reads through the stride, subtracts the
 *             origin and converts int16 normals; enc_input_check compares uint16 entries (16-byte groups of eight behind a scalar head and
 *             tail), folds the box over strided positions minus the origin and gathers first edges through either index width;
 *             enc_topo_compact reads either width.  The runtime's pointer queries cover the strided extent
 *             [ptr, ptr + (nvert-1)*stride + one vertex's bytes) inside one allocation of the context's device, else CRTHIP_E_ARGUMENT in
 *             status[i] and nothing is launched on that mesh.  A mesh whose topology pass runs on the host pool has its uint16 index
 *             copied back as it is and widened there.
 *             Clear: HOST arrays, packed by the staging copies; int16 normals and uint16 indices go up as they are and are converted by
 *             the same kernels.
 *           CRTHIP_ENCODE_OUTPUT_DEVICE: `out` is device memory and the blobs are spliced on the GPU, with the rules of
 *             crthip_encode_batch_to_device's device_out.  Clear: `out` is HOST memory.
 *           Any other bit: CRTHIP_E_ARGUMENT.
 * Either way the result is laid out as crthip_encode_batch_to_device lays it out: blob i is the blob_len[i] bytes at out + blob_offset[i]
 * (n entries each), the offsets are crthip_arena_layout's, the bytes up to the next 16-byte multiple are zeros, and the total is returned
 * even when it exceeds cap (nothing is written then).  Per-mesh failures - crthip_encode_batch's, a refused layout, an index entry >= nvert -
 * go into status[i] with blob_len[i] = 0; the neighbouring meshes are still encoded.  The three topology modes give the same bytes.
 * When not to use it: INTEGRATION.md 3c. */
#define CRTHIP_ENCODE_OUTPUT_DEVICE 2u
int64_t crthip_encode_batch_layout(crthip_ctx *ctx, uint32_t n, const crthip_mesh *meshes, const crthip_attr_list *extra /* n lists or NULL */,
                                   const crthip_mesh_layout *layouts /* n or NULL */, uint32_t host_threads, uint32_t flags, void *out, size_t cap,
                                   uint64_t *blob_offset /* n */, uint32_t *blob_len /* n */, uint32_t *out_nvert, uint32_t *out_nface,
                                   int32_t *status, crthip_encode_batch_stats *stats, crthip_kernel_times *times);
/* The splice of the last crthip_encode_batch_to_device on the context (all of its chunks). */
typedef struct {
	uint32_t pieces;             /* stretches of the arena with one source: a run of host-made bytes, or one payload on the device */
	uint32_t jobs;               /* the pieces after tiling: waves of enc_splice */
	uint64_t literal_bytes;      /* host-made bytes: the literal buffer, uploaded once and packed (this is its size on the link) */
	uint64_t device_bytes;       /* bytes moved from device sources */
	uint64_t arena_bytes;        /* literal_bytes + device_bytes = the call's return value */
	float splice_kernel_us;      /* device time of enc_splice */
	uint32_t launches;           /* launches of enc_splice: one a chunk */
} crthip_splice_stats;
int crthip_ctx_encode_splice_stats(const crthip_ctx *ctx, crthip_splice_stats *s);

/* Where crthip_encode_batch / crthip_encode_batch_attrs / crthip_encode_batch_resident on this context run a mesh's CLERS topology pass (degenerate faces, half-edge
 * pairing, the walk that writes the CLERS symbols, split bits, vertex numbering and prediction quads).  Same bytes in every mode.
 *   CRTHIP_TOPOLOGY_HOST    (default) on the host_threads pool, overlapping the device's quantisation
 *   CRTHIP_TOPOLOGY_DEVICE  every mesh on the device (kernels enc_topo_compact, enc_topo_pair, enc_topo_walk): no host thread is started,
 *                           host_threads is ignored, the compacted faces, quads and CLERS symbols never leave the device
 *   CRTHIP_TOPOLOGY_SPLIT   meshes whose walk state fits LDS (crthip_encode_topology_fits_lds) on the device, the others on the pool,
 *                           at the same time
 * Any other value: CRTHIP_E_ARGUMENT.  A mesh's connectivity never decides where it runs: non-manifold input is byte-identical too. */
#define CRTHIP_TOPOLOGY_HOST 0
#define CRTHIP_TOPOLOGY_DEVICE 1
#define CRTHIP_TOPOLOGY_SPLIT 2
int crthip_ctx_set_encode_topology(crthip_ctx *ctx, int where);

/* (test hooks, no device needed)  1 when the device pass keeps this mesh's walk state in LDS, else 0: a function of nvert and nface as
 * given, the one the batch planner uses. */
int crthip_encode_topology_fits_lds(const crthip_mesh *m);
/* The topology pass of one mesh on the host: which = 0 the host encoder's own pass (what crthip_encode runs), which = 1 the source the
 * device kernels run (csrc/enc_topology.h), compiled for the host, with 16- or 32-bit walk state as the device would pick.  The caller
 * gives the buffers: faces mesh->nface*3 words, group_end max(mesh->ngroups, 1), quads mesh->nvert*4, clers CRTHIP_TOPOLOGY_CLERS_CAP
 * bytes, split_words CRTHIP_TOPOLOGY_SPLIT_CAP words (the pass's own bounds); the counts come back in the struct.  CRTHIP_E_ARGUMENT for
 * another `which`, a point cloud, or a mesh crthip_encode would refuse. */
#define CRTHIP_TOPOLOGY_CLERS_CAP(nface) (7ull*(nface) + 64)
#define CRTHIP_TOPOLOGY_SPLIT_CAP(nface) (4ull*(nface) + 4)
typedef struct {
	uint32_t *faces;            /* out: compacted faces, nface*3 */
	uint32_t *group_end;        /* out: ngroups new ends */
	uint32_t *quads;            /* out: nvert x (t, a, b, c) */
	uint8_t *clers;             /* out: nclers symbols */
	uint32_t *split_words;      /* out: nsplit_words words, MSB-first, the last one zero-padded */
	uint32_t nvert, nface;      /* out: what the container says */
	uint32_t ngroups, max_front, nclers, split_bits, nsplit_words;
	uint32_t lds;               /* out: which = 1 walked with the 16-bit (LDS) state */
} crthip_topology_result;
int crthip_encode_topology_model(const crthip_mesh *m, int which, crthip_topology_result *r);


/* (test hook, no device needed)  What the encoder reads from a mesh's HOST arrays before it quantises: which = 0 the host encoder's own
 * loops (what crthip_encode runs), which = 1 the source the kernels of crthip_encode_batch_resident run (csrc/enc_input_check.h),
 * compiled for the host and walked in the kernels' partition (the same runs, tiles, merge order and sequential sum).  recipe says how the
 * position step is derived: 0 position_q as given, 1 the bounding box seeded from vertex 0 (position_bits > 0), 2 the mean length of the
 * faces' first edges, 3 the bounding box seeded from +-FLT_MAX (a cloud); mn / mx / sum are what that recipe's loop leaves (0 where it has
 * none) and step the resulting q.  Neither model gathers through an index entry >= nvert or reads position[0] of an empty mesh: with
 * index_out_of_range set, sum and step are reported as 0.  CRTHIP_E_ARGUMENT for another `which` or a mesh crthip_encode would refuse for
 * anything but its index entries. */
typedef struct {
	uint32_t index_out_of_range;  /* 1: an index entry >= nvert */
	uint32_t recipe;
	float mn[3], mx[3];
	double sum;
	float step;
	uint32_t reserved;
} crthip_encode_input_result;
int crthip_encode_input_model(const crthip_mesh *m, int which, crthip_encode_input_result *r);
/* (test hooks, no device needed)  The two models above with the mesh's HOST arrays read through a crthip_mesh_layout (NULL: as above):
 * which = 0 the host loops, which = 1 the kernels' source in the kernels' partition - for a uint16 index the head, the 16-byte groups of
 * eight and the tail of enc_input_check's range pass, and enc_topo_compact reading 16-bit entries.  A refused layout: CRTHIP_E_ARGUMENT,
 * nothing written. */
int crthip_encode_input_model_layout(const crthip_mesh *m, const crthip_mesh_layout *layout, int which, crthip_encode_input_result *r);
int crthip_encode_topology_model_layout(const crthip_mesh *m, const crthip_mesh_layout *layout, int which, crthip_topology_result *r);

/* (test hooks, no device needed)  The splice of crthip_encode_batch_to_device on the host.  crthip_encode_splice_model runs the host encoder
 * in its deferred mode, codes each recorded stream with the host encoder's own writers, then runs the plan and the mover of csrc/enc_splice.h
 * in the kernel's partition - the same tiles, lanes walked in a loop, tiles in a shuffled order - with the payload in buffers of its own
 * and the arena at an address that is dst_misalign (0..15) bytes off a 16-byte boundary.  Writes the blob and the zeros to the next
 * 16-byte multiple to out (cap >= that) and returns the blob's length, which must equal crthip_encode_attrs byte for byte; < 0 on error.
 * crthip_splice_copy_model moves `bytes` bytes from src to dst with the mover alone, tiles shuffled; it reads up to 3 bytes on either
 * side of the source (enc_splice.h: SOURCES).
 * crthip_encode_splice_plan_model plans n items in chunks of chunk_items (0: one chunk), each chunk a plan of its own that continues
 * the arena where the one before it ended, as a batch beyond one device image does: blob_offset / blob_len as
 * crthip_encode_batch_to_device gives them, the statistics summed over the chunks, and up to piece_cap pieces as (arena offset, bytes,
 * 1 literal | 0 device) triples; returns the pieces' count. */
int64_t crthip_encode_splice_model(const crthip_mesh *mesh, const crthip_attr_list *extra, uint32_t dst_misalign, uint8_t *out, size_t cap);
int crthip_splice_copy_model(const uint8_t *src, uint8_t *dst, uint64_t bytes, uint32_t seed);
int64_t crthip_encode_splice_plan_model(uint32_t n, const crthip_mesh *meshes, const crthip_attr_list *extra, uint64_t *blob_offset, uint32_t *blob_len,
                                        crthip_splice_stats *stats, uint64_t *pieces /* 3 per piece */, size_t piece_cap, uint32_t chunk_items);

/* (test hook, no device needed)  The two passes of CRTHIP_BIND_QUANTIZED (csrc/quant_out.h) on the host, in the kernels' partition, lanes walked
 * in a loop from the last to the first.  values: nvert*N int32, packed; out: the destination as a binding's buffer would be (2-byte aligned;
 * stride as in the binding, 0 = packed); transform->q on entry is the attribute's step, the whole record on return.  which 0: the
 * one-workgroup partition of k_quant_out_blob; which 1: the blocks of k_quant_range / k_quant_store, each pass visiting its blocks in an
 * order shuffled by `seed`.  1 <= N <= 4, else CRTHIP_E_ARGUMENT. */
int crthip_quant_out_model(const int32_t *values, uint32_t nvert, uint32_t N, uint32_t stride, void *out, crthip_quant_transform *transform,
                           int which, uint32_t seed);

/* (test hook, no device needed)  The value of crthip_batch_bind_computed_tangents (csrc/tangent.h) on the host, in the kernels' partition.
 * position: nvert*3 int32, uv: nvert*2 int32, packed; index: nface*3 uint32, or uint16 with index_u16; normal: the normals as a binding of
 * normal_format (FLOAT / INT16) and normal_stride (0 = packed) leaves them; out, format, stride: as in the binding.  which 0: the
 * one-workgroup partition of tangent_blob (nvert <= 2 304, else CRTHIP_E_ARGUMENT); which 1: the blocks of tangent_faces /
 * tangent_vertex.  Blocks and lanes are visited in an order shuffled by `seed`. */
int crthip_tangent_model(const int32_t *position, const int32_t *uv, const void *index, uint32_t index_u16, uint32_t nvert, uint32_t nface,
                         const void *normal, uint32_t normal_format, uint32_t normal_stride, void *out, uint32_t format, uint32_t stride,
                         int which, uint32_t seed);

/* (test hook, no device needed)  crthip_batch_bind_meshlets on the host: csrc/meshlet.h, the kernels' source, in their partition.  index:
 * nface*3 uint32, or uint16 with index_u16; group_end / ngroups: the group table; the three arrays and their capacities as in the binding
 * (host memory); counts: the blob's record.  which 0: meshlet_blob (one workgroup, a wave a segment, a blob of one segment written in
 * place; any number of segments is taken here); which 1: meshlet_segments / meshlet_place.  Segments, workgroups and the lanes of every
 * step are visited in an order shuffled by `seed`.  The errors of the bind call and of crthip_meshlet_bound apply. */
int crthip_meshlet_model(const void *index, uint32_t index_u16, uint32_t nface, uint32_t ngroups, const uint32_t *group_end,
                         const crthip_meshlet_binding *m, crthip_meshlet_counts *counts, int which, uint32_t seed);

/* (test hook, no device needed)  crthip_batch_bind_meshlet_bounds on the host: csrc/meshlet_bounds.h, the kernel's source, in its partition.
 * position: nvert*3 delta-decoded integers (may be NULL when nvert is 0); meshlets, vertices, triangles, counts: the host arrays of a
 * finished meshlet build (crthip_meshlet_model's), in which vertex ids may be >= nvert; bounds: host memory, 16-byte aligned, room for
 * `capacity` records, of which counts->meshlets are written.  The grid is sized by `capacity` as the kernel's is by the bound; workgroups,
 * their waves and the lanes of every step are visited in an order shuffled by `seed`.  CRTHIP_E_ARGUMENT: a NULL or misaligned array,
 * capacity below counts->meshlets, a meshlet of more than 255 vertices or 512 triangles or one that reaches outside the counts, or a local
 * id that is not below its meshlet's vertex_count. */
int crthip_meshlet_bounds_model(const int32_t *position, uint32_t nvert, const crthip_meshlet *meshlets, const uint32_t *vertices,
                                const uint8_t *triangles, const crthip_meshlet_counts *counts, crthip_meshlet_bounds *bounds, uint32_t capacity,
                                uint32_t seed);

/* (test hook, no device needed)  crthip_batch_bind_adjacency on the host: csrc/adjacency.h, the kernels' source, in their partition.  index:
 * nface*3 uint32, or uint16 with index_u16 (may be NULL when nface is 0); twin: host memory, 3*nface words; counts: the record, or NULL.
 * which 0: adjacency_blob, one workgroup with 16-bit list entries (a blob beyond its limit - 3*nface > 65 536 or more than 64 KiB of lists -
 * is CRTHIP_E_LIMIT here; the decode sends such a blob down the other path); which 1: adjacency_count, adjacency_offsets, adjacency_fill,
 * adjacency_twin.  Workgroups, waves and lanes, and so the order of every atomic, are shuffled by `seed`.  CRTHIP_E_ARGUMENT: an unknown
 * partition, a NULL or misaligned twin (4 bytes) with nface > 0, 3*nface beyond 32 bits.  nface == 0 writes the all-zero record. */
int crthip_adjacency_model(const void *index, uint32_t index_u16, uint32_t nface, uint32_t nvert, uint32_t *twin, crthip_adjacency_counts *counts,
                           int which, uint32_t seed);

/* (test hook, no device needed)  crthip_batch_bind_weld on the host: csrc/weld.h, the kernels' source, in their partition.  position: nvert*3
 * int32 (may be NULL when nvert is 0); index: nface*3 uint32, or uint16 with index_u16 (may be NULL when nface is 0); remap: host memory,
 * nvert words; windex: host memory, 3*nface words, or NULL (no welded index: degenerate is 0); counts: the record, or NULL; stats: two words,
 * or NULL - the slots all insert walks visited and the longest walk's.
 * which 0: weld_blob, one workgroup with its table where the kernel has LDS (a blob beyond its limit - more than 8 192 vertices - is
 * CRTHIP_E_LIMIT here; the decode sends such a blob down the other path); which 1: weld_insert, weld_lookup, weld_index.  Workgroups and
 * threads, and so the order of every atomic, are shuffled by `seed`.  CRTHIP_E_ARGUMENT: an unknown partition, a NULL position, index or
 * remap where there is something to read or write, a misaligned remap or windex (4 bytes), 3*nface beyond 32 bits. */
int crthip_weld_model(const int32_t *position, const void *index, uint32_t index_u16, uint32_t nface, uint32_t nvert, uint32_t *remap, uint32_t *windex,
                      crthip_weld_counts *counts, uint64_t *stats, int which, uint32_t seed);

/* (test hook, no device needed)  ONE level of crthip_batch_bind_lod on the host: csrc/lod.h, the kernels' source, in their partition.  position:
 * nvert*3 int32; index: nface*3 ids, uint16 if index_u16 else uint32 (ids >= nvert are allowed); remap: host memory, nvert words; lod_index:
 * host memory, 3*nface words of which 3*faces are written; counts: the record, or NULL; stats: four words, the slots all vertex insert walks
 * visited and the longest of them, then the same for the face inserts; or NULL.
 * which 0: lod_blob, one workgroup with its table where the kernel has LDS (a job beyond its limit - more than 8 192 vertices or faces - is
 * CRTHIP_E_LIMIT here; the decode sends such a job down the other path); which 1: lod_insert, lod_lookup, lod_faces, lod_keep, lod_offsets,
 * lod_scatter.  Workgroups and threads, and with them every atomic, are walked in an order shuffled by seed: the bytes do not depend on it. */
int crthip_lod_model(const int32_t *position, const void *index, uint32_t index_u16, uint32_t nface, uint32_t nvert, uint32_t shift, uint32_t *remap,
                     uint32_t *lod_index, crthip_lod_counts *counts, uint64_t *stats, int which, uint32_t seed);

/* (test hook, no device needed)  ONE level of crthip_batch_bind_cloud_lod on the host: csrc/cloud_lod.h, the kernels' source, in their
 * partition.  position: nvert*3 int32, nvert >= 1; chunk_points: K, or 0 with chunks NULL; remap, points: host memory, nvert words, of points
 * `cells` are written; weight: nvert words of which `cells` are written, or NULL; chunks: ceil(nvert / K) records of which ceil(cells / K) are
 * written, or NULL; counts: the record, or NULL; stats: two words, the slots all insert walks visited and the longest walk's, or NULL.
 * which 0: cloud_lod_blob, one workgroup with its table where the kernel has LDS (a job beyond its limit - more than 8 192 vertices - is
 * CRTHIP_E_LIMIT here; the decode sends such a job down the other path); which 1: cloud_lod_insert, cloud_lod_lookup, cloud_lod_offsets,
 * cloud_lod_scatter, cloud_lod_chunks.  Workgroups and threads, and with them every atomic, are walked in an order shuffled by seed: the bytes
 * do not depend on it.  CRTHIP_E_ARGUMENT: an unknown partition, a NULL position, and whatever crthip_batch_bind_cloud_lod refuses of a binding
 * of this one level at capacities of exactly nvert and ceil(nvert / K), in its order. */
int crthip_cloud_lod_model(const int32_t *position, uint32_t nvert, uint32_t shift, uint32_t chunk_points, uint32_t *remap, uint32_t *points,
                           uint32_t *weight, crthip_cloud_chunk *chunks, crthip_cloud_lod_counts *counts, uint64_t *stats, int which, uint32_t seed);

/* (test hook, no device needed)  ONE set of crthip_batch_bind_compact on the host: csrc/compact.h, the kernels' source, in their partition.
 * src: the id list, 3*nface words (uint16 if src_u16), of which the first 3*faces are read - nface is the bound the grids are sized from,
 * faces <= nface what the kernels read from the source's record (a LOD level's `faces`; nface itself for the other sources).  newid: nvert
 * words or NULL; order: vertex_capacity words or NULL; index: index_capacity words or NULL; counts: the record, or NULL.  gathers: ngather
 * records of host pointers - E bytes of vertex v at src + v*src_stride go to dst + j*dst_stride (a stride of 0: packed); the copy unit is
 * chosen from them as the planner chooses it.  which 0: compact_blob, one workgroup with its mask where the kernel has LDS (nvert or nface
 * beyond 8 192 is CRTHIP_E_LIMIT here; the decode sends such a set down the other path); which 1: compact_mark, compact_count,
 * compact_offsets, compact_place, compact_index; both end with compact_gather.  which 2: a cloud set - src is the level's points (nface words
 * of capacity, `faces` of them kept: used), newid, order and index NULL, compact_gather alone.  Workgroups and threads, and with them every
 * atomic, are walked in an order shuffled by seed: the bytes do not depend on it.  CRTHIP_E_ARGUMENT: an unknown partition, a NULL src with
 * nface > 0, faces > nface, ngather > CRTHIP_COMPACT_MAX_GATHERS, a gather with a NULL pointer, E == 0 or a stride below E. */
typedef struct crthip_compact_model_gather { const void *src; void *dst; uint32_t E, src_stride, dst_stride, reserved; } crthip_compact_model_gather;
int crthip_compact_model(const void *src, uint32_t src_u16, uint32_t nface, uint32_t faces, uint32_t nvert, uint32_t *newid, uint32_t *order,
                         uint32_t *index, uint32_t vertex_capacity, uint32_t index_capacity, crthip_compact_counts *counts,
                         const crthip_compact_model_gather *gathers, uint32_t ngather, int which, uint32_t seed);

/* (test hook, no device needed)  crthip_batch_bind_bvh on the host: csrc/bvh.h, the kernels' source, in their partition.  position: nvert*3
 * int32, the delta-decoded integers; index: 3*nface ids (uint16 if index_u16), an id >= nvert makes its face absent; nodes: host memory,
 * 2*nface - 1 records, 16-byte aligned; parent: 2*nface - 1 words or NULL; order: nface words or NULL; counts: the record, or NULL.
 * which 0: bvh_blob, one workgroup with its arrays where the kernel has LDS (a blob beyond its limit - more than 4 096 faces - is
 * CRTHIP_E_LIMIT here; the decode sends such a blob down the other path); which 1: bvh_boxes, bvh_keys, four passes of bvh_sort_count,
 * bvh_sort_offsets and bvh_sort_scatter, bvh_tree, bvh_refit.  Workgroups and threads, and with them every atomic and every arrival, are
 * walked in an order shuffled by seed: the bytes do not depend on it.  CRTHIP_E_ARGUMENT: an unknown partition, nface == 0, a NULL position
 * with nvert > 0, a NULL index, nodes NULL or not 16-byte aligned. */
int crthip_bvh_model(const int32_t *position, uint32_t nvert, const void *index, uint32_t index_u16, uint32_t nface, crthip_bvh_node *nodes,
                     uint32_t *parent, uint32_t *order, crthip_bvh_counts *counts, int which, uint32_t seed);

/* (test hook, no device needed)  crthip_bvh_cast of ONE set on the host: csrc/bvh_cast.h, the kernel's source, one workgroup of 64 segments
 * after another, each with a stack block of the kernel's size.  Every pointer of the set is HOST memory, `transform` included; hits: nseg
 * records.  The set's own checks are crthip_bvh_cast's, in its order (set or hits NULL: CRTHIP_E_ARGUMENT); where the memory is cannot be
 * checked.  Any bytes in `nodes` end as the contract says.  stats (or NULL): two words, the nodes taken from the stacks and the faces tested,
 * summed over the segments. */
int crthip_bvh_cast_model(const crthip_bvh_cast_set *set, crthip_cast_hit *hits);
int crthip_bvh_cast_model_stats(const crthip_bvh_cast_set *set, crthip_cast_hit *hits, uint64_t *stats);

/* (test hook, no device needed)  crthip_bvh_query of ONE set on the host: csrc/bvh_query.h, the kernel's source, one workgroup of 64 boxes
 * after another, each with a stack block of the kernel's size.  Every pointer of the set is HOST memory, `transform` included; results: nbox
 * records; faces: nbox*face_capacity words (or NULL where the call allows it).  The set's own checks are crthip_bvh_query's, in its order
 * (set or results NULL: CRTHIP_E_ARGUMENT); where the memory is cannot be checked.  Any bytes in `nodes` end as the contract says.  stats (or
 * NULL): two words, the nodes taken from the stacks and the faces tested, summed over the boxes. */
int crthip_bvh_query_model(const crthip_bvh_query_set *set, crthip_query_result *results, uint32_t *faces);
int crthip_bvh_query_model_stats(const crthip_bvh_query_set *set, crthip_query_result *results, uint32_t *faces, uint64_t *stats);

/* (test hook, no device needed)  crthip_bvh_closest of ONE set on the host: csrc/bvh_closest.h, the kernel's source, one workgroup of 64
 * points after another, each with a stack block of the kernel's size.  Every pointer of the set is HOST memory, `transform` included; hits:
 * npoint records.  The set's own checks are crthip_bvh_closest's, in its order (set or hits NULL: CRTHIP_E_ARGUMENT); where the memory is
 * cannot be checked.  Any bytes in `nodes` end as the contract says.  stats (or NULL): two words, the nodes taken from the stacks and the
 * faces tested, summed over the points.  order: 0 visits the nearer child first, as the kernel does; 1 the children in the nodes' own order
 * (the same bytes, other counts); anything else: CRTHIP_E_ARGUMENT. */
int crthip_bvh_closest_model(const crthip_bvh_closest_set *set, crthip_closest_hit *hits);
int crthip_bvh_closest_model_stats(const crthip_bvh_closest_set *set, crthip_closest_hit *hits, uint64_t *stats, uint32_t order);

#ifdef __cplusplus
}
#endif
#endif /* CORTO_HIP_H */
