// host_probe.cpp — the entry points that read a blob's header and nothing else, and the thread's last error: crthip_probe,
// crthip_output_layout, crthip_strerror / crthip_last_error.  Host only: no HIP call, no device code, so a stand-alone program can be
// built from this file and crt_format.cpp alone (tests/cpp/output_layout_check.cpp).
//
// Reference anchor: crt::Decoder::Decoder reads the header (src/decoder.cpp:41-89); its callers size their own buffers from nvert / nface
// (src/main.cpp:266-300).
#include <cstring>
#include <string>

#include "../../include/corto_hip.h"
#include "crt_format.h"
#include "output_layout.h"

using namespace corto_hip;

// errors: the thread's last message (crthip_last_error) and the code handed back (batch_internal.h)
static thread_local std::string g_error;
int fail(int code, const std::string &msg) { g_error = msg; return code; }

extern "C" const char *crthip_strerror(int code) {
	switch(code) {
	case CRTHIP_OK: return "ok";
	case CRTHIP_E_ALIGN: return "Memory must be alignegned on 4 bytes.";
	case CRTHIP_E_MAGIC: return "Not a crt file.";
	case CRTHIP_E_TRUNCATED: return "Truncated or inconsistent crt stream.";
	case CRTHIP_E_ENTROPY: return "Unknown entropy";
	case CRTHIP_E_TOPOLOGY: return "Decoding topology failed";
	case CRTHIP_E_NORMAL_NEEDS_POSITION: return "No position attribute found. Use DIFF normal strategy instead.";
	case CRTHIP_E_FORMAT: return "Format not supported for this attribute on the device path";
	case CRTHIP_E_ARGUMENT: return "Invalid argument";
	case CRTHIP_E_DEVICE: return "No usable HIP device (the MI355X path has no CPU fallback)";
	case CRTHIP_E_NOMEM: return "Out of memory";
	case CRTHIP_E_LIMIT: return "Too many attributes or components for this build";
	}
	return "unknown error";
}
int fail(int code) { return fail(code, crthip_strerror(code)); }
// context plumbing for the encoder stages (encoder_internal.h)
namespace corto_hip { int ctx_fail(int code, const char *msg) { return fail(code, msg ? std::string(msg) :
	std::string(crthip_strerror(code))); } }
extern "C" const char *crthip_last_error(void) { return g_error.c_str(); }

// ------------------------------------------------------------------------------------------------
// host-only probes
void fill_info(const BlobHeader &h, crthip_blob_info *info) {
	memset(info, 0, sizeof(*info));
	info->version = h.version; info->entropy = h.entropy; info->nvert = h.nvert; info->nface = h.nface;
	info->nattr = (uint32_t)h.attrs.size(); info->nexif = (uint32_t)h.exif.size(); info->body_offset = h.body_offset;
	for(size_t i = 0; i < h.attrs.size(); i++) {
		crthip_attr_info &a = info->attr[i];
		strncpy(a.name, h.attrs[i].name.c_str(), CRTHIP_NAME_MAX - 1);
		a.codec = h.attrs[i].codec; a.q = h.attrs[i].q; a.components = h.attrs[i].N;
		a.format = h.attrs[i].format; a.strategy = h.attrs[i].strategy;
	}
}

extern "C" int crthip_probe(const uint8_t *blob, size_t len, crthip_blob_info *info) {
	if(!blob || !info) return fail(CRTHIP_E_ARGUMENT);
	BlobHeader h;
	int err = parse_header(blob, len, h);
	if(err) return fail(err);
	fill_info(h, info);
	return CRTHIP_OK;
}

// ------------------------------------------------------------------------------------------------
// Where a decoded item's arrays lie in its output block.  Every array starts on the next 256-byte multiple; the formats are the natural
// ones (generic FLOAT, normal FLOAT, colour UINT8 x 4, index UINT32) or, under CRTHIP_LAYOUT_RENDER, SURVEY 8f3's (normal INT16, index
// UINT16 where the blob's vertex ids fit).
namespace corto_hip {
void layout_blob(const crthip_blob_info &info, uint32_t flags, uint64_t &off, crthip_out_array *attr, crthip_out_array *index) {
	const bool render = (flags & CRTHIP_LAYOUT_RENDER) != 0;
	auto take = [&off](uint64_t n) { off = (off + 255) & ~(uint64_t)255; const uint64_t r = off; off += n; return r; };
	for(uint32_t k = 0; k < info.nattr; k++) {
		const crthip_attr_info &a = info.attr[k];
		crthip_out_array o; o.format = CRTHIP_FMT_FLOAT; o.out_components = a.components;
		if(a.codec == CRTHIP_CODEC_NORMAL) { o.out_components = 3; o.bytes = (uint64_t)info.nvert*(render ? 6 : 12); if(render) o.format = CRTHIP_FMT_INT16; }
		else if(a.codec == CRTHIP_CODEC_COLOR) { o.format = CRTHIP_FMT_UINT8; o.out_components = 4; o.bytes = (uint64_t)info.nvert*4; }
		else o.bytes = (uint64_t)info.nvert*a.components*4;
		o.offset = take(o.bytes);
		if(attr) attr[k] = o;
	}
	crthip_out_array o; o.offset = 0; o.bytes = 0; o.format = CRTHIP_FMT_UINT32; o.out_components = 3;
	if(info.nface) {
		const bool u16 = render && info.nvert < 65536;
		if(u16) o.format = CRTHIP_FMT_UINT16;
		o.bytes = (uint64_t)info.nface*(u16 ? 6 : 12);
		o.offset = take(o.bytes);
	}
	if(index) *index = o;
}
}

extern "C" int crthip_output_layout(uint32_t nblobs, const uint8_t *const *blobs, const uint32_t *lens, uint32_t flags,
                                    crthip_out_array *attr, crthip_out_array *index, uint64_t *total) {
	if(flags & ~CRTHIP_LAYOUT_RENDER) return fail(CRTHIP_E_ARGUMENT, "crthip_output_layout: unknown flag bits");
	if(!total || (nblobs && (!blobs || !lens))) return fail(CRTHIP_E_ARGUMENT, "crthip_output_layout: null argument");
	uint64_t off = 0;
	crthip_blob_info info;
	for(uint32_t i = 0; i < nblobs; i++) {
		const int err = crthip_probe(blobs[i], lens[i], &info);
		if(err) return fail(err, std::string(crthip_strerror(err)) + " (blob " + std::to_string(i) + ")");
		layout_blob(info, flags, off, attr, index ? index + i : nullptr);
		if(attr) attr += info.nattr;
	}
	*total = layout_total(off);
	return CRTHIP_OK;
}
