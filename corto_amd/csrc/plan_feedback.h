// plan_feedback.h — what a context learns from the flags of the batches it has decoded: K-DELTA's narrow / wide LDS layout and the LDS edge
// slots of the CLERS automaton, each with its back-off.  Arithmetic on a few integers and the status words, no HIP call: harvest (batch.cpp)
// feeds them, the planner reads them, tests/cpp/plan_feedback_check.cpp pins their trajectories on the host.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "kernels.h"

namespace corto_hip {

// K-DELTA keeps values in LDS as int16 relative to vertex 0 and redoes an attribute that does not fit in HBM (slow, exact): a context
// that meets such blobs (positions quantised beyond 15 bits) plans its next batches with 32-bit values; a long run of batches later it
// tries the narrow layout again, with growing patience if that turns out wrong
struct DeltaFeedback {
	bool wide = false;                  // 32-bit values in LDS: $CORTO_DELTA_WIDE=1, or learnt from a batch whose 16-bit relative values overflowed
	uint32_t calm = 0, patience = 256;
	bool just_narrowed = false;         // the narrow layout is on trial again after a wide spell (an overflow now doubles the patience)
	// planned_wide: the layout the batch was planned with; redone_blobs: its blobs with an attribute that left int16; forced_wide: the environment switch
	void update(bool planned_wide, uint64_t redone_blobs, bool forced_wide) {
		if(!planned_wide) {
			if(redone_blobs) {
				wide = true;
				// overflowed right after narrowing again (never on a context's first overflow)
				if(just_narrowed && patience < (1u << 20)) patience *= 2;
				calm = 0;
			}
			just_narrowed = false;                                              // (narrow and fine, or wide from here on)
		} else if(!forced_wide && ++calm >= patience) { wide = false; calm = 0; just_narrowed = true; }
	}
};

// what a blob of a harvested batch tells K-TOPO's feedback: flags is its StatusWords::topo_flags word (bit 0: redone on the HBM front; above it
// the ring slots, 15 bits, and from bit 16 the pool slots it would have needed), status its CRTHIP_* code
struct TopoBlob { uint32_t nface, nclers, flags; int32_t status; };

// The LDS edge slots of the CLERS automaton: ring x scale (a power of two), pool x pool_q8 / 8, the pool not beyond pool_cap (0: none) -
// topo_lds_geometry's arguments.  Raised after a batch with fallbacks, lowered after a long calm run.
struct TopoFeedback {
	uint32_t scale = 1, pool_q8 = 8, pool_cap = 0, calm = 0, patience = 64;
	// blob(i) -> TopoBlob, for i < n
	template <class F> void update(size_t n, F blob) {
		uint64_t fallbacks = 0;
		for(size_t i = 0; i < n; i++) fallbacks += blob(i).flags & 1u;
		// more than one blob in twenty redone on the HBM front (5x slower): more edge slots from the next batch on - as many as the redone blobs
		// say they would have needed (k_topology_lds' redo reports ring and pool slots above bit 0 of the flags word; round 4 went up four-fold
		// whatever was missing, and a batch of Delaunay discs that needed 600 pool slots of its 512 got 2 048 + 2 048: 72 KB of LDS a blob, two
		// automata a CU, the pipeline at a third of its rate); a long run without any: try less again, and be more patient the next time that
		// turns out to be too little
		if(fallbacks*20 > n) {
			uint32_t ring_m = 1, q8 = 8;
			const uint32_t cap_before = pool_cap;
			uint32_t learnable = 0;
			for(size_t i = 0; i < n; i++) {
				const TopoBlob B = blob(i);
				if(!(B.flags & 1u)) continue;
				// a redo that ended in an error (an untrusted stream runs its pool dry before it fails) teaches nothing, and a front beyond the LDS
				// form's 4 096 + 4 096 records is on the HBM path by design: neither may scale every OTHER blob's request up
				if(B.status) continue;
				const uint32_t need_ring = (B.flags >> 1) & 0x7FFFu, need_pool = B.flags >> 16;
				if(need_ring > TOPO_SLOTS_MAX || need_pool > TOPO_SLOTS_MAX) continue;
				learnable++;
				uint32_t ring, pool, symwin;
				topo_lds_geometry(B.nface, B.nclers, TOPO_SLOTS_MAX, 1, 8, topo_slots((uint32_t)n), ring, pool, symwin);
				uint32_t m = 1;
				while(ring*m < need_ring && m < 16) m <<= 1;
				ring_m = std::max(ring_m, m);
				q8 = std::max(q8, std::min(128u, (need_pool*8 + pool - 1)/pool + 1u));      // (an eighth on top)
				pool_cap = std::max(pool_cap, need_pool + need_pool/8);
			}
			const bool grew = ring_m > scale || q8 > pool_q8 || pool_cap > cap_before;
			scale = std::max(scale, ring_m); pool_q8 = std::max(pool_q8, q8);
			// (they fell back with what they asked for: capacity, or a need the redo cannot see)
			if(!grew && learnable) { scale = std::min(16u, scale*2); pool_q8 = std::min(128u, pool_q8*2); pool_cap *= 2; }
			pool_cap = std::min(pool_cap, TOPO_SLOTS_MAX + TOPO_SLOTS_MAX/8);      // (a uint32 that doubled without a bound wrapped to 0 = "no cap")
			if(calm == 0 && patience < (1u << 20)) patience *= 2;                  // fell back right after scaling down
			calm = 0;
		} else if(fallbacks == 0 && (scale > 1 || pool_q8 > 8) && ++calm >= patience) {
			scale = std::max(1u, scale/2); pool_q8 = std::max(8u, pool_q8*3/4); pool_cap = pool_cap*3/4; calm = 0;
		}
	}
};

}
