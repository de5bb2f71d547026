// debug_config.h — every environment switch of the decode path (and the batch encoders' one) in one struct, filled when a context is made
// (crthip_ctx_create) and never consulted anywhere else: no getenv in the planner, no function-local statics.
//
// These are deployment settings and test hooks (documented in INTEGRATION.md); none changes results, only which kernels produce them.
// Rounds 2-3 also carried some fifteen experiment switches (alternative kernel paths kept for A/B measurements: a two-pass and a
// single-pass long-stream decode, three decode launches, K-DELTA without LDS / as pointer jumping / walk-only, LDS pad knobs, K-BIT
// twice ...).  Each was measured level or slower (profiles/r03_what_bounds_the_pipeline.txt has the numbers) and they were
// REMOVED in round 4, kernels included: the library has one kernel per stage and size class.
// Besides these: decoder_facade.cpp reads $CORTO_HIP_CONTEXTS / $CORTO_HIP_DEVICE / $CORTO_HIP_COMBINE_US / $CORTO_HIP_LEADERS once, pool.cpp reads
// ROCm's own $GPU_MAX_HW_QUEUES to size itself.
#pragma once
#include <cstdint>
#include <cstdlib>

#include "device_plan.h"

namespace corto_hip {

struct DebugConfig {
	int tun_share = -1;             // $CORTO_TUN_SHARE: unset: launches of 64+ streams make every DISTINCT probability table's dictionary once (K-TAB) and decode
	                                // the streams in groups of one dictionary; 2: the same two kernels but one dictionary PER STREAM, whatever repeats (what a
	                                // batch of unrelated meshes looks like: bench.py's `without_dictionary_sharing`); 0: dictionary and decode by one wave per
	                                // stream (what a launch of fewer than 64 streams takes anyway); 1: two kernels always
	int delta_wide = 0;             // $CORTO_DELTA_WIDE=1: K-DELTA keeps 32-bit values in LDS from the start (a context otherwise learns it from its first overflowing batch)
	bool check_pinned = false;      // $CORTO_HIP_CHECK_PINNED=1: a buffer handed over as a packed pinned arena (crthip_ctx_set_packed_host_blobs) is verified to be pinned host memory
	bool delta_rounds = false;      // $CORTO_DELTA_ROUNDS=1 (test hook): K-DELTA's round loop from vertex 1 for every attribute - int16, 32-bit and byte records, with and
	                                // without parallelogram prediction - instead of after 24 slow window passes (tests/test_gpu_parity.py runs every fixture through it)
	bool values_i32 = false;        // $CORTO_VALUES_I32=1 (A/B and test hook): K-BIT always hands 32-bit values on (otherwise int16 where an attribute's tables prove every
	                                // width <= 16 bits and the consumer is k_delta_lds16 / k_normal_blob: plan_jobs.cpp)
	bool unpack_chunked = false;    // $CORTO_UNPACK_CHUNKED=1 (test hook): every bit block through the chunked K-BIT with its look-back - the kernel of big meshes -
	                                // however small (tests/test_gpu_parity.py runs ragged sizes through both)
	bool front_off = false;         // $CORTO_FRONT=0 (A/B and test hook): a single-stream context launches the automata and K-BIT as two kernels, one after the
	                                // other, instead of k_front's one grid (plan_launch.cpp)
	bool carry_off = false;         // $CORTO_CARRY=0 (A/B and test hook): crthip_batch_decode_with_next enqueues the next batch's entropy stage as launches of its
	                                // own behind this batch's kernels instead of inside k_front's / k_delta_lds16's grids, and the pool runs one batch per
	                                // lane and call as it did before it pipelined its lanes (plan_launch.cpp, pool.cpp)
	uint32_t qout_blob_max = 0;     // $CORTO_QOUT_BLOB_MAX=<vertices> (A/B hook, tools/quant_out_rate.py): the largest quantised attribute k_quant_out_blob takes, in place
	                                // of QOUT_BLOB_MAX (kernels.h); beyond it k_quant_range / k_quant_store.  Either kernel takes any size: the same bytes
	uint64_t encode_image_budget = 0; // $CORTO_ENCODE_IMAGE_BUDGET=<bytes> (test hook): the batch encoders cut a batch into chunks whose device image stays within
	                                // this many bytes instead of within half the free device memory - a batch of small meshes then runs in several chunks, the
	                                // path a batch beyond one device image takes (tests/test_encode_device_out_gpu.py); never above that half
};

inline DebugConfig debug_config_from_env() {
	DebugConfig c;
	auto on = [](const char *name) { const char *e = getenv(name); return e && e[0] == '1'; };
	if(const char *e = getenv("CORTO_TUN_SHARE")) if(e[0] >= '0' && e[0] <= '2') c.tun_share = e[0] - '0';
	c.delta_wide = on("CORTO_DELTA_WIDE");
	c.check_pinned = on("CORTO_HIP_CHECK_PINNED");
	c.unpack_chunked = on("CORTO_UNPACK_CHUNKED");
	c.delta_rounds = on("CORTO_DELTA_ROUNDS");
	c.values_i32 = on("CORTO_VALUES_I32");
	{ const char *e = getenv("CORTO_FRONT"); c.front_off = e && e[0] == '0'; }
	{ const char *e = getenv("CORTO_CARRY"); c.carry_off = e && e[0] == '0'; }
	if(const char *e = getenv("CORTO_QOUT_BLOB_MAX")) c.qout_blob_max = (uint32_t)strtoul(e, nullptr, 10);
	if(const char *e = getenv("CORTO_ENCODE_IMAGE_BUDGET")) c.encode_image_budget = strtoull(e, nullptr, 10);
	return c;
}

} // namespace corto_hip
