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

// Kernel entry points (extern "C" names in the batch code object):
//   k_batch_scan(const BatchSeg* segs, uint32_t nseg, Key* part)       grid: tiles x kBlock
//   k_batch_reduce(const Key* part, const uint32_t* req_tile0, Key* out)
//                                     grid: requests x kBlock; request r owns
//                                     part[req_tile0[r] .. req_tile0[r + 1])
}  // namespace p1
