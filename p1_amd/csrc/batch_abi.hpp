// batch_abi.hpp -- what the host runtime (p1hip.hip, p1hip_scan_batch) and the
// batch code object (p1hip_batch_kernels.hip) agree on: the segment table of
// one coalesced launch pair and the lookup every workgroup runs on it.  The
// kernels are loaded by name from the second embedded code object
// (p1hip_batch_blob.S), so this header IS their ABI.  tools/batch_emu replays
// the same table with the same lookup on the host.
//
// One launch pair answers many small requests (each at most kBatchMaxNonces
// nonces, possibly of different messages):
//   k_batch_scan    one workgroup per tile of kBlock nonces; the tiles of all
//                   requests lie back to back, request after request, decade
//                   piece after decade piece; one partial Key per tile
//   k_batch_reduce  one workgroup per request folds that request's partials
#pragma once
#include "scan_abi.hpp"

namespace p1 {

// One decade piece of one request: GenArgs is self-contained (the message's
// chaining value and tail template travel with it), so pieces of different
// messages share one table.
struct BatchSeg {
  GenArgs ga;
  uint32_t block0;  // first tile of the piece within the launch, strictly increasing
  uint32_t req;     // request (within the launch) the piece belongs to
};

// A request is coalesced when it has at most this many nonces: the range of
// the one-launch small path, so it has at most kSmallMaxBlocks tiles.
constexpr uint64_t kBatchMaxNonces = kSmallMaxNonces;
// Tiles per launch pair: 2^20 partials of 16 bytes = 16 MB per launch.
constexpr uint32_t kBatchMaxTiles = 1u << 20;

// The segment of tile b: the last i with segs[i].block0 <= b (segs[0].block0
// is 0).  Binary search: a launch holds up to kBatchMaxTiles segments.  b is
// the workgroup's tile, so on the device every load here is wave-uniform.
P1_HD uint32_t batch_find_seg(const BatchSeg* segs, uint32_t nseg, uint32_t b) {
  uint32_t lo = 0, hi = nseg;  // invariant: segs[lo].block0 <= b, and segs[hi].block0 > b where hi < nseg
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (segs[mid].block0 <= b) lo = mid;
    else hi = mid;
  }
  return lo;
}

// p1hip_scan_batch_wide: the mid-size requests of a call share k_scan launches
// (the scan code object's kernel, unchanged), whose pieces are ordered
// longest-running first across all requests, so a request's partials are not
// contiguous.  One range = a run of tiles of one request in the device's
// partial array (one k_scan segment, or the request's generic tiles).
struct WideRange {
  uint32_t tile0, ntiles;
};

// What thread `tid` of `nthreads` folds for a request whose ranges are
// ranges[r0 .. r1): the restatement of k_wide_reduce's loop that
// tools/batch_emu replays (the kernel then takes the workgroup's minimum).
P1_HD Key wide_fold_thread(const Key* part, const WideRange* ranges, uint32_t r0, uint32_t r1, uint32_t tid,
                           uint32_t nthreads) {
  Key m = {~0ull, ~0ull};
  for (uint32_t j = r0; j < r1; ++j) {
    const WideRange R = ranges[j];
    for (uint32_t i = tid; i < R.ntiles; i += nthreads)
      if (key_lt(part[R.tile0 + i], m)) m = part[R.tile0 + i];
  }
  return m;
}

// Kernel entry points (extern "C" names in the batch code object):
//   k_batch_scan(const BatchSeg* segs, uint32_t nseg, Key* part)       grid: tiles x kBlock
//   k_batch_reduce(const Key* part, const uint32_t* req_tile0, Key* out)
//                                     grid: requests x kBlock; request r owns
//                                     part[req_tile0[r] .. req_tile0[r + 1])
//   k_wide_reduce(const Key* part, const WideRange* ranges, const uint32_t* req_range0, Key* out)
//                                     grid: requests x kBlock; request r owns
//                                     ranges[req_range0[r] .. req_range0[r + 1])
}  // namespace p1
