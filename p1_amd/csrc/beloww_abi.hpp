// beloww_abi.hpp -- what the host runtime (p1hip.hip, p1hip_scan_below_batch_wide)
// and the fifth code object (p1hip_beloww_kernels.hip) agree on.  The kernel is
// loaded by name from the embedded object (p1hip_beloww_blob.S), so this header
// IS its ABI.  tools/batch_emu (`beloww`) replays the same tables with the same
// per-thread function.
//
// The sparse slices of many target searches share k_scan launches as the wide
// requests of p1hip_scan_batch_wide do (wide_plan.hpp): every tile leaves its
// 16-byte partial, the tile's minimum, in the device's partial array, and a
// request owns a list of ranges of it.  A tile can hold a hit only if its
// partial is at or below the request's target:
//   k_beloww_filter   one workgroup per request walks that request's ranges and
//                     writes the partial-array indices of its first `slots`
//                     such tiles, in table order, and the number of all of them
#pragma once
#include "batch_abi.hpp"

namespace p1 {

// Thread `t` of the chunk that starts at tile `c0` of range R: its tile's index
// in the partial array goes to *tile; is that tile inside the range with a
// partial at or below the target?  (A tile without a valid thread wrote the
// identity key, which passes under target UINT64_MAX: the host, which knows the
// tile map, drops it -- below_plan.hpp below_candidate.)  k_beloww_filter and
// the host replay share it.
P1_HD bool beloww_thread(const Key* part, WideRange R, uint32_t c0, uint32_t t, uint64_t target, uint32_t* tile) {
  const uint32_t i = c0 + t;
  *tile = R.tile0 + i;
  return i < R.ntiles && part[R.tile0 + i].h <= target;
}

// Kernel entry point (extern "C" name in the beloww code object):
//   k_beloww_filter(const Key* part, const WideRange* ranges, const uint32_t* req_range0,
//                   const uint64_t* targets, const uint32_t* req_slot0, uint32_t* cand, uint32_t* count)
//                                     grid: requests x kBlock; request r owns
//                                     ranges[req_range0[r] .. req_range0[r + 1])
//                                     and slots [req_slot0[r], req_slot0[r + 1]);
//                                     it writes the first min(count[r], slots)
//                                     of its slots, count[r] = every tile of its
//                                     ranges with part.h <= targets[r]
}  // namespace p1
