// k_encode_splice.hip — K-ENC-SPLICE: the pieces of a chunk's .crt containers from where the coders left them to their place in the
// caller's device arena (crthip_encode_batch_to_device), for gfx950.  enc_splice.h has the plan, the mover and the rules that make
// the tiles independent; this file is the launch shape alone.
//
//   k_enc_splice    one wave per tile of ESP_TILE destination bytes, four tiles a workgroup, tiles in destination order: neighbouring
//                   waves write neighbouring lines.  The tile's piece is found in tile_start (enc_job_of, as the batch's other kernels
//                   find a workgroup's job); the wave's number is made uniform first, so the search and the job's fields are scalar
//                   loads.  Plain vector loads and stores: no LDS, no atomics, no destination byte is read.
// Nothing is written outside [dst, dst + bytes) of a job, and nothing is read further than 3 bytes outside [src, src + bytes): the
// host has checked the arena's extent before the launch, and every source is a library allocation with slack (enc_splice.h: SOURCES).
#include "kernels_common.h"
#include "kernels.h"
#include "enc_splice.h"

namespace corto_hip {

__global__ __launch_bounds__(256) void k_enc_splice(const SpliceJob *__restrict__ jobs, const uint32_t *__restrict__ tile_start, uint32_t njobs) {
	const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x*(ESP_THREADS/ESP_LANES) + wave_id()));
	if(w >= tile_start[njobs]) return;
	const uint32_t j = enc_job_of(tile_start, njobs, w);
	const SpliceJob J = jobs[j];
	esp_copy_lane(J, w - tile_start[j], lane_id());
}

} // namespace corto_hip
