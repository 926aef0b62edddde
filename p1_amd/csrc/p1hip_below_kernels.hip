// p1hip_below_kernels.hip -- the third gfx950 code object of libp1hip.so: the
// mark kernel of p1hip_scan_below (every nonce whose hash is at or below a
// target).
//
// Only the generic per-thread path (scan_core.hpp generic_thread), so it
// compiles in seconds and needs no tools/isa_post.py pass; it is built
// device-only, linked into build/p1hip_below.hsaco and embedded by
// p1hip_below_blob.S after the other two objects, which stay as they are.
// The ABI with the host runtime is below_abi.hpp.
#include <hip/hip_runtime.h>

#include "below_abi.hpp"

using namespace p1;

// One tile per workgroup, as k_batch_scan: the workgroup finds its piece by
// binary search on block0 (uniform: scalar loads) and runs one nonce per
// thread.  Instead of a minimum it keeps one bit per nonce: the wave's ballot
// of "valid and at or below the target", stored by lane 0 with an ordinary
// vector store.  Every word of the launch's tiles is written by exactly one
// wave, so there is no memset, no atomic and nothing that waits.
extern "C" __global__ __launch_bounds__(kBlock) void k_below_mark(const BatchSeg* __restrict__ segs, uint32_t nseg,
                                                                  uint64_t target, uint64_t* __restrict__ marks) {
  const uint32_t b = blockIdx.x;
  // The target waits in a VGPR pair: the piece's 48 uniform words fill the
  // SGPR file, and with two more live scalars the allocator parks two SGPRs
  // in VGPR lanes ("SGPRs Spill: 2"; with this, 0).
  uint64_t t = target;
  asm volatile("" : "+v"(t));
  const BatchSeg& S = segs[batch_find_seg(segs, nseg, b)];
  const bool hit = below_thread(S.ga, (uint64_t)(b - S.block0) * kBlock + threadIdx.x, t);
  const uint64_t word = __ballot(hit);
  if ((threadIdx.x & 63u) == 0) marks[(uint64_t)b * kBelowWordsPerTile + (threadIdx.x >> 6)] = word;
}
