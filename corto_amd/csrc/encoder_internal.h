// encoder_internal.h — pieces of the host encoder (encoder.cpp) and of the context (batch.cpp) that the GPU encoder
// stages (encode_gpu.cpp, k_encode.hip) and the batch encoder (encode_batch.cpp) use, and the device helpers those two share: the
// try macro, DevMem, EventTimer, quant_job, Carver, and the one form a coded stream has between the coders and the container writer
// (Coded; the writer is enc_splice.h's write_container).  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/corto_hip.h"
#include "device_plan.h"
#include "enc_input_check.h"

namespace corto_hip {

int ctx_fail(int code, const char *msg);

// ---- device helpers of the encoder's host side (encode_gpu.cpp, encode_batch.cpp) ----
#define ENC_TRY(expr) do { hipError_t e_ = (expr); if(e_ != hipSuccess) return corto_hip::ctx_fail(CRTHIP_E_DEVICE, (std::string(#expr ": ") + hipGetErrorString(e_)).c_str()); } while(0)

struct DevMem { void *p = nullptr; ~DevMem() { if(p) (void)hipFree(p); } uint8_t *u8() const { return (uint8_t *)p; } };   // freed on every way out

// a pair of events around a stage's launches, made on first use and destroyed on every way out
struct EventTimer {
	hipEvent_t a = nullptr, b = nullptr; bool used = false;
	~EventTimer() { if(a) (void)hipEventDestroy(a); if(b) (void)hipEventDestroy(b); }
	int begin(hipStream_t st) { if(!a) { ENC_TRY(hipEventCreate(&a)); ENC_TRY(hipEventCreate(&b)); } used = true; ENC_TRY(hipEventRecord(a, st)); return 0; }
	int end(hipStream_t st) { ENC_TRY(hipEventRecord(b, st)); return 0; }
	// after the stream has passed end(): adds the stage's milliseconds to `sum`; false if the timer never ran or the events give no time
	bool add_to(float &sum) { float m = 0; if(!used || hipEventElapsedTime(&m, a, b) != hipSuccess) return false; sum += m; return true; }
};

struct Carver {                         // bump allocator over one device block (offsets only): the decode planner's scratch, the batch encoder's image
	uint64_t off = 0;
	uint64_t take(uint64_t bytes, uint64_t align = 256) { off = (off + align - 1) & ~(align - 1); const uint64_t r = off; off += bytes; return r; }
};

// What Tunstall::compress walks (src/tunstall.cpp:384-428), made from a byte histogram exactly as
// getProbabilities + createDecodingTables2 + createEncodingTables make it (src/tunstall.cpp:83-115, 125-256, 335-382).
struct TunEncoderTables {
	uint32_t nsym = 0;
	uint8_t probs[512];                 // nsym x (symbol, probability), sorted as the reference sorts them
	uint8_t remap[256];                 // symbol -> index in probs
	uint16_t lengths[256];              // word lengths by codeword
	std::vector<int32_t> offsets;       // the 2-symbol-step trie: >= 0 codeword, < 0 minus the offset of the next level
};
void tun_encoder_tables(const uint32_t counts[256], uint32_t size, TunEncoderTables &out);

// What the value coders and the entropy coder make of a batch of streams, in the one form every container writer takes
// (enc_splice.h: write_container).  A stream is its bit words (a symbol stream has none: words is null) and its blocks: the entropy-coded
// log arrays (1 for ARRAY, components for VALUES) or the symbol block.  A block is its header, which the host makes (Tunstall: u8 nsym |
// nsym x (sym, prob) | i32 size | i32 csize; entropy NONE: i32 size), and its payload (codewords; raw logs / symbols under NONE) by address
// and length; an empty payload has no address.  on_device says where EVERY words / payload pointer of the object points: into device
// memory, where the coders left it (crthip_encode_batch_to_device), or into the host buffers it was brought back to.  The object owns
// what they point into and must outlive whoever reads them; each device allocation has a 256-byte aligned base and 16 bytes behind its
// last region (enc_splice.h: SOURCES).
struct CodedBlock { std::vector<uint8_t> head; const uint8_t *payload = nullptr; uint32_t bytes = 0; };
struct CodedStream { uint32_t nwords = 0; const uint8_t *words = nullptr; std::vector<CodedBlock> blocks; };
struct Coded {
	std::vector<CodedStream> streams;
	bool on_device = false;
	DevMem image, tun_image, clers;                 // the value coder's image, the Tunstall coder's, the batch's host-mode CLERS block (encode_batch.cpp)
	std::vector<uint8_t> h_back, h_codes;           // brought back: words and raw logs / symbols compacted, the Tunstall coder's codeword region
	std::vector<std::vector<uint8_t>> h_made;       // made on the host (encoder.cpp: encode_host_coded): a buffer per stream
};

// value arrays for the device stages (encode_gpu.cpp); values are HOST pointers: they go up in one copy, the payload comes back
struct EncValueStream { uint32_t kind = 0, count = 0, components = 1; const void *values = nullptr; };   // kind: CRTHIP_ENC_*
int encode_value_streams(crthip_ctx *ctx, uint32_t entropy, const std::vector<EncValueStream> &in, Coded &out, crthip_kernel_times *times);

// quantisation on the device (encode_gpu.cpp: k_enc_quantize): HOST arrays in, HOST arrays out, one upload / download for all of them.
// kind: QK_FLOAT, QK_NORMAL, QK_COLOR, QK_INT (format: CRTHIP_FMT_INT32 / INT16 / INT8), QK_DOUBLE - device_plan.h
// stride / comps / flags / origin: how `in` is read through a crthip_mesh_layout (QuantJob's fields of the same names)
struct QuantRequest { uint32_t kind = 0, count = 0, N = 1, format = CRTHIP_FMT_FLOAT; const void *in = nullptr; void *out = nullptr; float q = 0; int32_t unit = 0; uint32_t qc[4] = {1, 1, 1, 1};
                      uint32_t stride = 0, comps = 1, flags = 0; float origin[3] = {0, 0, 0}; };
uint64_t quant_in_bytes(const QuantRequest &r);      // the raw input's bytes when packed (format-aware)
uint64_t quant_vertex_bytes(const QuantRequest &r);  // one vertex's bytes of the raw input
uint64_t quant_out_bytes(const QuantRequest &r);     // the quantised values' bytes
int quantize_device(crthip_ctx *ctx, const std::vector<QuantRequest> &reqs);
// the kernels' job (k_enc_quantize, k_enc_quantize_batch) of a request; packed: `in` is a packed copy of the request's array (a staged
// upload), else the caller's array with the request's stride
inline QuantJob quant_job(const QuantRequest &r, const void *in, void *out, bool packed = true) {
	QuantJob J{};
	J.in = in; J.out = out; J.count = r.count; J.kind = r.kind; J.N = r.N; J.q = r.q; J.unit = r.unit; J.format = r.format;
	for(int c = 0; c < 4; c++) J.qc[c] = r.qc[c] ? r.qc[c] : 1u;
	J.stride = packed || r.stride == quant_vertex_bytes(r) ? 0u : r.stride; J.comps = r.comps; J.flags = r.flags;
	for(int c = 0; c < 3; c++) J.origin[c] = r.origin[c];
	return J;
}

// the value coders + entropy coder over DEVICE-resident arrays (encode_gpu.cpp); each stream carries its mesh's entropy
struct DevValueStream { uint32_t kind = 0, count = 0, components = 1, entropy = 0; const void *values = nullptr; };
struct EncStageTimes { float hist = 0, parse = 0, pack = 0, tables = 0, trie = 0; bool any_hist = false, any_parse = false, any_pack = false, any_tables = false;
                       uint32_t host_table_streams = 0; uint64_t bytes_to_device = 0, bytes_from_device = 0; };
// fetch: the payload comes back (one gather launch, one copy of words and raw logs, one of codewords) and the pointers are host pointers;
// else only the word counts, the codeword counts and what the host-made tables need come back: no k_enc_gather, no copy of words, logs
// or codewords.  Ends with the stream synchronised.
int encode_value_streams_device(crthip_ctx *ctx, const std::vector<DevValueStream> &in, bool fetch, Coded &out, EncStageTimes &tm);
void enc_report_times(crthip_kernel_times *times, const EncStageTimes &tm);   // appends the stages' entries behind times->count

// ---- crthip_mesh_layout (encoder.cpp) ----
// A layout resolved against its mesh: how every data array is read.  Strides are bytes and never 0 (a packed array's is one vertex's bytes).
struct MeshRead {
	bool plain = true;                                    // nothing differs from what crthip_mesh means by itself
	bool index16 = false, normal16 = false, has_origin = false;
	uint32_t position = 12, normal = 12, color = 0, uv = 8, radius = 4;
	std::vector<uint32_t> attr;                           // one per entry of the mesh's crthip_attr_list
	float origin[3] = {0, 0, 0};
};
uint32_t generic_esize(uint32_t format);                  // bytes of one element of a crthip_generic_attr
// the rules of crthip_mesh_layout (sets the last error); m and extra have passed encode_check / encode_check_attrs
int layout_resolve(const crthip_mesh *m, const crthip_attr_list *extra, const crthip_mesh_layout *layout, MeshRead &rd);
// the index range check over HOST entries of either width
int index_range_host(const crthip_mesh *m, const MeshRead &rd);
EncInputJob enc_input_job(const crthip_mesh *m, const MeshRead *rd);   // position, index, sizes, recipe and the layout's fields; kind, partials, rec unset

// ---- crthip_encode_batch (encoder.cpp: checks, topology pass and container; encode_batch.cpp: the device half) ----
// encode_checked's argument checks (sets the last error); index_on_host == false: m->index is a DEVICE pointer, its entries are not read
int encode_check(const crthip_mesh *m, bool index_on_host = true);
// the position step's loops over the mesh's HOST arrays as setup runs them (recipe: enc_in_recipe), and the formulas over what they leave
void input_stats_host(const crthip_mesh *m, uint32_t recipe, EncInputRecord &r, const MeshRead *rd = nullptr);   // rd: the arrays are read through it
float position_step(const crthip_mesh *m, uint32_t recipe, const EncInputRecord &r);
// the rules of crthip_encode_attrs's extra list (sets the last error); device: also the value coder's bound on nvert*components
int encode_check_attrs(const crthip_mesh *m, const crthip_attr_list *extra, bool device);
constexpr uint32_t BATCH_BITS = 0xFFu;                // a stream that is the CLERS split bits, already packed
struct BatchAttr { uint32_t codec = 0, N = 0, prediction = 0, strategy = 0; QuantRequest quant; };
struct BatchStream { size_t at = 0; uint32_t kind = 0, count = 0, N = 1; int32_t attr = 0; };   // attr: index in attrs, -1 CLERS symbols, -2 split bits
struct BatchItem {
	int32_t status = CRTHIP_OK;
	uint32_t entropy = 0, nvert_in = 0, nface_in = 0;    // as given (nface_in 0: a point cloud)
	uint32_t nvert = 0, nface = 0;                        // what the container says (after the topology pass)
	std::vector<BatchAttr> attrs;                         // the container's order; quant.out unset
	uint32_t pos = 0;                                     // which of them is the position
	std::vector<uint32_t> faces;                          // meshes: degenerate faces dropped, original vertex ids
	std::vector<uint32_t> quads;                          // meshes: the prediction, (t, a, b, c) per encoded vertex
	std::vector<uint8_t> clers;
	uint32_t nclers = 0;                                  // CLERS symbols (clers.size(), or the device pass's count: its symbols stay on the device)
	bool topo_device = false, topo_lds = false;           // meshes: the topology pass runs on the device / with its walk state in LDS
	bool topo_image = false;                              // meshes: the CLERS symbols have their place in the chunk's device image (every mode but HOST)
	uint32_t topo_groups = 1;                             // groups the device pass walks (a mesh given without groups: one)
	bool index16 = false;                                 // meshes: the caller's index entries are uint16 (crthip_mesh_layout)
	std::vector<uint32_t> split_words;
	std::vector<uint8_t> frame;                           // the container without its streams
	std::vector<BatchStream> streams;                     // where they belong in it, in order (a BORDER normal's count: 0 until the device has it)
};
// extra: the mesh's generic attributes (or null), checked by encode_check_attrs
// position step + attribute table (after encode_check); step: the position step where the caller has it (crthip_encode_batch_resident:
// from the device's record) - m's data arrays are then not read
// rd: the mesh's resolved layout (or null): the requests carry its strides, origin and int16 flag, and a step computed here reads through it
void batch_setup(const crthip_mesh *m, const crthip_attr_list *extra, BatchItem &it, const float *step = nullptr, const MeshRead *rd = nullptr);
void batch_topology(const crthip_mesh *m, const crthip_attr_list *extra, BatchItem &it);   // topology pass (meshes) + frame; reads the index alone
// a mesh's frame from what the device topology pass reports (its record, the new group ends, the packed split words): header, counts,
// groups, max_front and the stream slots, without running the pass
struct EncTopoRecord;
void batch_frame(const crthip_mesh *m, const crthip_attr_list *extra, BatchItem &it, const EncTopoRecord &rec, const uint32_t *group_end,
                 const uint32_t *split_words);
// One item through the host encoder in its deferred mode, each recorded stream then coded by the host encoder's own writers
// (crthip_encode_splice_model): the frame, the slots, a coded stream per slot but the split bits (host pointers into coded.h_made), the
// split words.  Runs encode_check / encode_check_attrs first; returns their code.
struct HostCodedItem { std::vector<uint8_t> frame; std::vector<BatchStream> slots; Coded coded; std::vector<uint32_t> split_words;
                       uint32_t entropy = 0, nvert = 0, nface = 0; };
int encode_host_coded(const crthip_mesh *m, const crthip_attr_list *extra, HostCodedItem &out);

// the host encoder's topology pass alone (crthip_encode_topology_model, which = 0); split_bits before the final flush
struct TopologyModel { std::vector<uint32_t> faces, group_end, quads, split_words; std::vector<uint8_t> clers; uint32_t nvert = 0, nface = 0, max_front = 0; uint64_t split_bits = 0; };
void topology_host_model(const crthip_mesh *m, TopologyModel &out);   // (m->index: uint32)
void morton_order_host(const int32_t *coords, uint32_t nvert, std::vector<uint32_t> &order);   // encode_cloud's std::sort of the Morton records

// several blobs with HOST output buffers in one batch (batch.cpp): what crthip_decode_host is one of, and what the crt::Decoder facade's
// combiner hands over when several threads call decode() at once.  copy_out: copy every output into the caller's buffer before
// returning; else leave them in the context's pinned landing zone and say where (out_src -> out_dst, out_bytes): valid until the next
// call on this context - the facade lets every waiting thread copy its own.
struct HostDecodeReq {
	const uint8_t *blob; size_t len;
	const crthip_attr_binding *attrs;       // info.nattr entries in attribute order, or null: nothing bound
	void *index; uint32_t index_format;
	void *prediction;                       // host, nvert*3 uint32 or null: upstream's index.prediction (the context of a caller-supplied codec's deltaDecode)
	int32_t status;                         // out: CRTHIP_OK or this blob's CRTHIP_E_*
	uint32_t nout;                          // out (copy_out == false): pieces to copy
	const uint8_t *out_src[CRTHIP_MAX_ATTRS + 2]; void *out_dst[CRTHIP_MAX_ATTRS + 2]; size_t out_bytes[CRTHIP_MAX_ATTRS + 2];
};
int decode_host_many(crthip_ctx *ctx, uint32_t n, HostDecodeReq *reqs, bool copy_out);

// context plumbing (batch.cpp); ctx_fail is declared at the top
int ctx_device(crthip_ctx *ctx);
crthip_splice_stats &ctx_splice_stats(crthip_ctx *ctx);   // of the last crthip_encode_batch_to_device on the context
uint64_t ctx_encode_image_budget(crthip_ctx *ctx);   // $CORTO_ENCODE_IMAGE_BUDGET (debug_config.h), 0: none
int ctx_encode_topology(crthip_ctx *ctx);   // CRTHIP_TOPOLOGY_* of crthip_ctx_set_encode_topology
hipStream_t ctx_stream(crthip_ctx *ctx);
int ctx_quiesce(crthip_ctx *ctx);       // wait for whatever batch is in flight on the context
// (what the pool uses of the context and of a batch: pool_internal.h)

} // namespace corto_hip
