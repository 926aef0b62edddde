// belowb_abi.hpp -- what the host runtime (p1hip.hip, p1hip_scan_below_batch)
// and the fourth code object (p1hip_belowb_kernels.hip) agree on.  The kernels
// are loaded by name from the embedded object (p1hip_belowb_blob.S), so this
// header IS their ABI.  tools/batch_emu (`below`) replays the same tables with
// the same per-thread and per-word functions.
//
// One launch pair answers the current slice of many target searches (each
// slice dense and of at most kBelowBatchMaxNonces nonces, of any messages and
// any targets):
//   k_belowb_mark     k_below_mark with a target per request: one workgroup
//                     per tile of kBlock nonces, the tiles of all requests
//                     back to back (batch_abi.hpp BatchSeg), one ballot word
//                     per wave; the marks stay on the device
//   k_belowb_collect  one workgroup per request turns that request's mark
//                     words into the thread indices of its first `slots` set
//                     bits, in order, and their number
#pragma once
#include "below_abi.hpp"

namespace p1 {

// A request is coalesced when its first slice is dense and has at most this
// many nonces.  Derived, not measured: the slice rule asks for
// 2 * want * 2^64 / (target + 1) nonces, so every cap = 1 request at a dense
// target (>= 2^46) has a slice of at most 2 * 2^64 / 2^46 = 2^19 nonces, and
// cap = 2 at the switch target itself one of 2^20.
constexpr uint64_t kBelowBatchMaxNonces = 1ull << 20;
// Hit slots per launch pair: 2^22 indices of 4 bytes = 16 MB per launch pair.
constexpr uint64_t kBelowBatchMaxSlots = 1ull << 22;

// The set bits of mark word number `widx` of a launch, lowest first, as
// in-launch thread indices (64 * widx + bit; below 2^28, a launch has at most
// kBatchMaxTiles * kBelowWordsPerTile words): the first `room` of them go to
// out[0 ..).  Returns how many were written.  k_belowb_collect and the host
// replay share it.
P1_HD uint32_t belowb_expand_word(uint64_t word, uint32_t widx, uint32_t room, uint32_t* out) {
  uint32_t k = 0;
  while (word != 0 && k < room) {
    out[k++] = widx * 64u + (uint32_t)__builtin_ctzll(word);
    word &= word - 1;
  }
  return k;
}

// Kernel entry points (extern "C" names in the belowb code object):
//   k_belowb_mark(const BatchSeg* segs, uint32_t nseg, const uint64_t* targets, uint64_t* marks)
//                                     grid: tiles x kBlock; wave w of tile b
//                                     writes marks[kBelowWordsPerTile * b + w],
//                                     bit l = lane l's below_thread against
//                                     targets[segs[..].req]; every word of the
//                                     launch's tiles is written exactly once
//   k_belowb_collect(const uint64_t* marks, const uint32_t* req_tile0, const uint32_t* req_hit0,
//                    uint32_t* idx, uint32_t* count)
//                                     grid: requests x kBlock; request r owns
//                                     words [4 * req_tile0[r], 4 * req_tile0[r + 1])
//                                     and slots [req_hit0[r], req_hit0[r + 1]);
//                                     it writes the first count[r] =
//                                     min(set bits, slots) of its slots
}  // namespace p1
