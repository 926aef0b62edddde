// scan_replay.hpp -- TEST TOOLS: one tile of k_scan replayed on the host, for
// tools/p1emu (a scan's launches) and tools/batch_emu (the shared launches of
// a wide call).  Never part of libp1hip.so.
#pragma once
#include "../p1_amd/csrc/scan_abi.hpp"

// One tile of k_scan: the workgroup's kBlock threads and their minimum.  The
// segment walk is the tools' own copy of the two lines in p1hip_kernels.hip
// scan_tile (the kernel source is not shared with the host).
static inline p1::Key replay_scan_tile(const p1::Segment* segs, uint32_t nseg, uint32_t b) {
  using namespace p1;
  uint32_t si = 0;
  while (si + 1 < nseg && segs[si + 1].block0 <= b) ++si;
  const Segment& S = segs[si];
  Key m = {~0ull, ~0ull};
  for (uint32_t t = 0; t < (uint32_t)kBlock; ++t) {
    const uint32_t local = (b - S.block0) * kBlock + t;
    Key k;
    switch (S.kind) {
#define P1_CASE(FV, NV, TR)                   \
  case variant_id(FV, NV, TR):                \
    k = fast_thread<FV, NV, TR>(S.fa, local); \
    break;
#include "../p1_amd/csrc/fast_variants.inc"
#undef P1_CASE
      default:
        k = generic_thread(S.ga, local);
        break;
    }
    if (key_lt(k, m)) m = k;
  }
  return m;
}
