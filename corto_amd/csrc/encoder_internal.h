// encoder_internal.h — pieces of the host encoder (encoder.cpp) and of the context (batch.cpp) that the GPU encoder
// stages (encode_gpu.cpp, k_encode.hip) use.  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "../../include/corto_hip.h"

namespace corto_hip {

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

// value arrays for the device stages (encode_gpu.cpp); values are HOST pointers
struct EncValueStream { uint32_t kind = 0, count = 0, components = 1; const void *values = nullptr; };   // kind: CRTHIP_ENC_*
struct EncValueResult {
	std::vector<uint32_t> words;                    // the bit stream (empty for a symbol stream); the writer pads to 4 bytes before it
	std::vector<std::vector<uint8_t>> blocks;       // entropy-coded log arrays (1 for ARRAY, components for VALUES) or the symbol block
};
int encode_value_streams(crthip_ctx *ctx, uint32_t entropy, const std::vector<EncValueStream> &in, std::vector<EncValueResult> &res,
                         crthip_kernel_times *times);

// quantisation on the device (encode_gpu.cpp: k_enc_quantize): HOST arrays in, HOST arrays out, one upload / download for all of them.
// kind: QK_FLOAT, QK_NORMAL, QK_COLOR, QK_INT (format: CRTHIP_FMT_INT32 / INT16 / INT8), QK_DOUBLE - device_plan.h
struct QuantRequest { uint32_t kind = 0, count = 0, N = 1, format = CRTHIP_FMT_FLOAT; const void *in = nullptr; void *out = nullptr; float q = 0; int32_t unit = 0; uint32_t qc[4] = {1, 1, 1, 1}; };
uint64_t quant_in_bytes(const QuantRequest &r);      // the raw input's bytes (format-aware)
uint64_t quant_out_bytes(const QuantRequest &r);     // the quantised values' bytes
int quantize_device(crthip_ctx *ctx, const std::vector<QuantRequest> &reqs);

// the value coders + entropy coder over DEVICE-resident arrays (encode_gpu.cpp); each stream carries its mesh's entropy
struct DevValueStream { uint32_t kind = 0, count = 0, components = 1, entropy = 0; const void *values = nullptr; };
struct EncStageTimes { float hist = 0, parse = 0, pack = 0, tables = 0, trie = 0; bool any_hist = false, any_parse = false, any_pack = false, any_tables = false;
                       uint32_t host_table_streams = 0; uint64_t bytes_to_device = 0, bytes_from_device = 0; };
int encode_value_streams_device(crthip_ctx *ctx, const std::vector<DevValueStream> &in, std::vector<EncValueResult> &res, EncStageTimes &tm);
void enc_report_times(crthip_kernel_times *times, const EncStageTimes &tm);   // appends the stages' entries behind times->count

// ---- crthip_encode_batch (encoder.cpp: checks, topology pass and container; encode_batch.cpp: the device half) ----
int encode_check(const crthip_mesh *m);              // encode_checked's argument checks (sets the last error)
// the rules of crthip_encode_attrs's extra list (sets the last error); device: also the value coder's bound on nvert*components
int encode_check_attrs(const crthip_mesh *m, const crthip_attr_list *extra, bool device);
constexpr uint32_t BATCH_BITS = 0xFFu;                // a stream that is the CLERS split bits, already packed
struct BatchAttr { uint32_t codec = 0, N = 0, prediction = 0, strategy = 0; bool position = false; QuantRequest quant; };
struct BatchStream { size_t at = 0; uint32_t kind = 0, count = 0, N = 1; int32_t attr = 0; };   // attr: index in attrs, -1 CLERS symbols, -2 split bits
struct BatchItem {
	int32_t status = CRTHIP_OK;
	uint32_t entropy = 0, nvert_in = 0, nface_in = 0;    // as given (nface_in 0: a point cloud)
	uint32_t nvert = 0, nface = 0;                        // what the container says (after the topology pass)
	std::vector<BatchAttr> attrs;                         // the container's order; quant.out unset
	std::vector<uint32_t> faces;                          // meshes: degenerate faces dropped, original vertex ids
	std::vector<uint32_t> quads;                          // meshes: the prediction, (t, a, b, c) per encoded vertex
	std::vector<uint8_t> clers;
	uint32_t nclers = 0;                                  // CLERS symbols (clers.size(), or the device pass's count: its symbols stay on the device)
	bool topo_device = false, topo_lds = false;           // meshes: the topology pass runs on the device / with its walk state in LDS
	bool topo_image = false;                              // meshes: the CLERS symbols have their place in the chunk's device image (every mode but HOST)
	uint32_t topo_groups = 1;                             // groups the device pass walks (a mesh given without groups: one)
	std::vector<uint32_t> split_words;
	std::vector<uint8_t> frame;                           // the container without its streams
	std::vector<BatchStream> streams;                     // where they belong in it, in order (a BORDER normal's count: 0 until the device has it)
};
// extra: the mesh's generic attributes (or null), checked by encode_check_attrs
void batch_setup(const crthip_mesh *m, const crthip_attr_list *extra, BatchItem &it);      // position step + attribute table (after encode_check)
void batch_topology(const crthip_mesh *m, const crthip_attr_list *extra, BatchItem &it);   // topology pass (meshes) + frame; reads the index alone
// a mesh's frame from what the device topology pass reports (its record, the new group ends, the packed split words): header, counts,
// groups, max_front and the stream slots, without running the pass
struct EncTopoRecord;
void batch_frame(const crthip_mesh *m, const crthip_attr_list *extra, BatchItem &it, const EncTopoRecord &rec, const uint32_t *group_end,
                 const uint32_t *split_words);
// the host encoder's topology pass alone (crthip_encode_topology_model, which = 0); split_bits before the final flush
struct TopologyModel { std::vector<uint32_t> faces, group_end, quads, split_words; std::vector<uint8_t> clers; uint32_t nvert = 0, nface = 0, max_front = 0; uint64_t split_bits = 0; };
void topology_host_model(const crthip_mesh *m, TopologyModel &out);
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

// context plumbing (batch.cpp)
int ctx_fail(int code, const char *msg);
int ctx_device(crthip_ctx *ctx);
int ctx_encode_topology(crthip_ctx *ctx);   // CRTHIP_TOPOLOGY_* of crthip_ctx_set_encode_topology
hipStream_t ctx_stream(crthip_ctx *ctx);
int ctx_quiesce(crthip_ctx *ctx);       // wait for whatever batch is in flight on the context
int ctx_fill_async(crthip_ctx *ctx, void *dst, size_t bytes, int value);   // k_fill_block on the context's main stream
int ctx_copy_to_host_async(crthip_ctx *ctx, void *host_dst, const void *dev_src, size_t bytes);   // D2H behind the decode in flight; sync / done then cover the copy

} // namespace corto_hip
