// pool_internal.h — what the pool (pool.cpp) uses of the library beside the public C ABI: a little context and batch plumbing
// (batch.cpp), the packed-host-blob run rule it shares with crthip_batch_reset, and the device-range check it shares with the resident
// encoder (encode_batch.cpp).  Needs nothing from the encoder or the planner; tests/cpp/pool_fake_backend.cpp implements exactly this
// header (and the public calls the pool makes), so that the pool's schedule runs without a GPU.  Not part of the C ABI.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/corto_hip.h"

namespace corto_hip {

int ctx_fail(int code, const char *msg);   // sets the thread's last error (host_probe.cpp) and returns `code`

// context and batch plumbing (batch.cpp)
bool ctx_pipelines(crthip_ctx *ctx);    // a single-stream context without $CORTO_CARRY=0: crthip_batch_decode_with_next can carry a batch's entropy stage in another's grids
bool batch_carriable(const crthip_batch *b);      // its last decode could have been carried by a batch like itself, and could have carried one
bool batch_entropy_done(const crthip_batch *b);   // planned as `next` of crthip_batch_decode_with_next, and that call enqueued (carried) its entropy stage
int batch_reset_at(crthip_batch *b, uint32_t nblobs, const uint8_t *const *blobs, const uint32_t *lens, const void *device_base, const uint64_t *dev_off);   // crthip_batch_reset, blob i resident at device_base + dev_off[i]
int ctx_fill_async(crthip_ctx *ctx, void *dst, size_t bytes, int value);   // k_fill_block on the context's main stream
int ctx_copy_to_host_async(crthip_ctx *ctx, void *host_dst, const void *dev_src, size_t bytes);   // D2H behind the decode in flight; sync / done then cover the copy

// Packed host blobs (crthip_ctx_set_packed_host_blobs): a run is a stretch of blobs that follow one another in host memory as they do in
// arena layout (16-byte aligned, in list order), and goes up with one copy.  In more runs than PACKED_RUNS_MAX the blobs are gathered on the
// calling thread as if the switch were off (batch.cpp: batch_fill); the pool counts an item's runs to keep such items out of groups
constexpr uint32_t PACKED_RUNS_MAX = 8;
inline bool packed_run_starts(const uint8_t *const *blobs, const uint32_t *lens, uint32_t i) {
	return i == 0 || blobs[i] != blobs[i - 1] + (((size_t)lens[i - 1] + 15) & ~(size_t)15);
}

// [p, p + bytes) is `align`-aligned device memory of `device`, inside one allocation, by the runtime's pointer queries (encode_batch.cpp);
// bytes == 0: true
bool resident_array_ok(const void *p, uint64_t bytes, uint32_t align, int device);

} // namespace corto_hip
