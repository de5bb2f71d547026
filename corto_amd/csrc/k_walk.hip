// k_walk.hip — the .crt blob walk on the device, for blobs that live only in device memory (crthip_batch_create_resident).
// One wave per blob runs crt_walk.h's walker, wave-uniform: every lane reads the same bytes and takes the same branches.  Bytes come out of
// a 1 KiB window in LDS that the 64 lanes refill with one 16-byte load each, aligned to 16 and never past the blob's 16-byte-rounded
// extent, so each hop of the cursor through the stream framing is one dependent round trip to memory, not one per field.  The record is
// built in LDS and leaves with one 16-byte store per lane.
#include "crt_walk.h"
#include "kernels.h"

namespace corto_hip {

constexpr uint32_t WALK_WINDOW = 1024;          // 64 lanes x 16 bytes

struct WindowReader {
	const uint8_t *p;                           // the blob: 16-byte aligned
	uint64_t ext;                               // its length rounded up to 16: no load reaches past it
	uint8_t *win;                               // LDS, WALK_WINDOW bytes
	uint32_t lo, hi;                            // the window holds [lo, hi)
	__device__ uint32_t byte(uint32_t pos) {
		if(pos < lo || pos >= hi) refill(pos);
		return win[pos - lo];
	}
	__device__ void refill(uint32_t pos) {
		__syncthreads();                        // every lane is done with the old window
		lo = pos & ~15u; hi = lo + WALK_WINDOW;
		const uint64_t o = (uint64_t)lo + threadIdx.x*16;
		uint4 v = make_uint4(0, 0, 0, 0);
		if(o < ext) v = *(const uint4 *)(p + o);
		*(uint4 *)(win + threadIdx.x*16) = v;
		__syncthreads();
	}
	__device__ void copy(uint8_t *dst, uint32_t n) {         // blob bytes [0, round16(n)) to dst (LDS, 16-byte aligned)
		const uint32_t n16 = (n + 15) & ~15u;
		for(uint32_t o = threadIdx.x*16; o < n16; o += WALK_WINDOW) *(uint4 *)(dst + o) = *(const uint4 *)(p + o);
	}
};

__global__ __launch_bounds__(64) void k_walk_blobs(const uint8_t *base, const WalkJob *jobs, uint32_t nblobs, uint8_t *records, uint32_t rec_cap) {
	__shared__ __attribute__((aligned(16))) uint8_t win[WALK_WINDOW];
	__shared__ __attribute__((aligned(16))) uint8_t rec[WALK_RECORD_BYTES];
	__shared__ WalkWork work;
	const uint32_t i = blockIdx.x;
	if(i >= nblobs) return;
	const WalkJob j = jobs[i];
	WindowReader r{base + j.off, ((uint64_t)j.len + 15u) & ~15ull, win, 1u, 0u};
	walk_record(r, j.len, rec, rec_cap, work);
	__syncthreads();
	uint8_t *dst = records + (uint64_t)i*rec_cap;
	for(uint32_t o = threadIdx.x*16; o < rec_cap; o += WALK_WINDOW) *(uint4 *)(dst + o) = *(const uint4 *)(rec + o);
}

} // namespace corto_hip
