// below_abi.hpp -- what the host runtime (p1hip.hip, p1hip_scan_below) and the
// third code object (p1hip_below_kernels.hip) agree on.  The kernel is loaded
// by name from the embedded object (p1hip_below_blob.S), so this header IS its
// ABI.  tools/p1emu replays the same table with the same per-thread function.
//
// k_below_mark answers, for every nonce of a table of generic pieces
// (batch_abi.hpp BatchSeg: one nonce per thread, kBlock per tile), whether
// bitcoin.Hash(msg, nonce) <= target: one bit per nonce, one 64-bit word per
// wave, kBelowWordsPerTile words per tile.
#pragma once
#include "batch_abi.hpp"

namespace p1 {

constexpr uint32_t kBelowWordsPerTile = kBlock / 64;  // one ballot per wave

// The longest slice of one p1hip_scan_below step.  Sparse (k_scan filters, the
// survivors are marked): 2^34 nonces bound the work done after the answer is
// already known to about a third of a second.  Dense (every nonce is marked):
// 2^28 nonces are one mark launch of kBatchMaxTiles tiles.
constexpr uint64_t kBelowMaxSliceSparse = 1ull << 34;
constexpr uint64_t kBelowMaxSliceDense = (uint64_t)kBatchMaxTiles * kBlock;
constexpr uint64_t kBelowMinSlice = 1ull << 16;
// At or above this target a slice skips the filter: about one expected hit
// per 2^18-nonce tile, so most tiles would survive it anyway.
constexpr uint64_t kBelowDenseTarget = 1ull << 46;

// Thread `gid` of the piece `A`: is it a nonce of the piece whose hash is at
// or below the target?  Validity comes from `count`, never from the identity
// key: nonce 2^64-1 is a legal nonce and UINT64_MAX a legal target.
P1_HD bool below_thread(const GenArgs& A, uint64_t gid, uint64_t target) {
  const Key k = generic_thread(A, gid);
  return gid < A.count && k.h <= target;
}

// Kernel entry point (extern "C" name in the below code object):
//   k_below_mark(const BatchSeg* segs, uint32_t nseg, uint64_t target, uint64_t* marks)
//                                     grid: tiles x kBlock; wave w of tile b
//                                     writes marks[kBelowWordsPerTile * b + w],
//                                     bit l = lane l's below_thread; every word
//                                     of the launch's tiles is written
}  // namespace p1
