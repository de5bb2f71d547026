// output_layout.h — the one rule that places a decoded item's output arrays in one block (crthip_output_layout, include/corto_hip.h):
// host_probe.cpp states it, the pool's lanes (pool.cpp) lay their blocks out through it.  No HIP.  Not part of the C ABI.
#pragma once
#include <cstdint>

#include "../../include/corto_hip.h"

namespace corto_hip {

// the arrays of ONE blob behind `off` (the end of the arrays laid out so far; moved to the end of this blob's last array): attr receives
// info.nattr entries in info.attr order, index one entry (bytes == 0 for a cloud); either may be null
void layout_blob(const crthip_blob_info &info, uint32_t flags, uint64_t &off, crthip_out_array *attr, crthip_out_array *index);
// the block's size: the end of the last array rounded up to 256
inline uint64_t layout_total(uint64_t off) { return (off + 255) & ~(uint64_t)255; }

} // namespace corto_hip
