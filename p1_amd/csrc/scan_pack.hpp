// scan_pack.hpp -- the HIP-free part of a scan launch: how a plan's pieces
// are ordered and cut into k_scan launches, the segment table of each launch,
// and the argument block of k_scan_small.  Host only, no HIP call: p1hip.hip
// runs what this header lays out, and tools/p1emu replays it tile by tile on
// the CPU (the way batch_plan.hpp is shared with tools/batch_emu).
#pragma once
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "planner.hpp"
#include "scan_abi.hpp"

namespace p1 {

constexpr uint32_t kMaxSegs = 64;              // segments per launch
// Workgroups per launch: 2^22 x 256 threads stays below HIP's 2^32-thread
// grid limit and keeps configs[3] on one GPU (2^38 nonces, ~1.07M
// workgroups) in one launch, i.e. one grid drain per scan.
constexpr uint32_t kMaxLaunchBlocks = 1u << 22;

inline bool has_variant(int fv, int mode, bool trail) {
#define P1_CASE(FV, MODE, TR) \
  if (fv == FV && mode == MODE && trail == TR) return true;
#include "fast_variants.inc"
#undef P1_CASE
  return false;
}

// Per-scan accounting of one device (what p1hip_get_stats sums up).
struct ScanCounters {
  uint64_t fast_launches = 0, fast_nonces = 0, fast_ops = 0, gen_launches = 0, gen_nonces = 0;
  uint64_t scan_launches = 0, scan_nonces = 0, scan_ops = 0;
  double scan_ms = 0.0;
  ScanCounters& operator+=(const ScanCounters& o) {
    fast_launches += o.fast_launches; fast_nonces += o.fast_nonces; fast_ops += o.fast_ops;
    gen_launches += o.gen_launches; gen_nonces += o.gen_nonces;
    scan_launches += o.scan_launches; scan_nonces += o.scan_nonces; scan_ops += o.scan_ops;
    scan_ms += o.scan_ms;
    return *this;
  }
};

// One k_scan launch: pieces order[first .. first + count) of the plan.
struct ScanBatch {
  size_t first, count;
  uint32_t blocks;
};

struct ScanPack {
  std::vector<size_t> order;       // plan.launches indices, longest-running first
  std::vector<ScanBatch> batches;  // the launches, in order
  uint32_t total_blocks = 0;
};

// Order a plan's pieces and cut them into launches of at most `max_segs`
// segments and `max_blocks` workgroups (a piece larger than `max_blocks`
// gets a launch of its own).  `max_segs` is a parameter only so that a test
// can lower it: the library always packs with kMaxSegs.
inline ScanPack pack_scan(const Plan& plan, uint64_t max_blocks, uint32_t max_segs = kMaxSegs) {
  ScanPack P;
  // Longest-running workgroups first: fast pieces by lo-loop length (10^k),
  // then generic pieces, so short work fills the grid's drain.
  P.order.resize(plan.launches.size());
  for (size_t i = 0; i < P.order.size(); ++i) P.order[i] = i;
  auto weight = [&](size_t i) -> uint64_t {
    const Launch& L = plan.launches[i];
    return L.fast ? (uint64_t)(L.fa.kpow / L.fa.nsub) * (uint64_t)L.btail : (uint64_t)L.btail - 1;
  };
  std::stable_sort(P.order.begin(), P.order.end(), [&](size_t a, size_t b) { return weight(a) > weight(b); });
  // When a scan needs several launches (e.g. configs[3]'s 2^38 nonces on one
  // GPU), balance them: each batch closes once it reaches total/launches
  // workgroups, so the launches are near-equal rather than one full and one
  // small one (equal drains, and a per-launch average that means something).
  uint64_t all_blocks = 0;
  for (const Launch& L : plan.launches) all_blocks += L.blocks;
  const uint64_t nlaunch = (all_blocks + max_blocks - 1) / max_blocks;
  const uint64_t target = nlaunch > 1 ? (all_blocks + nlaunch - 1) / nlaunch : max_blocks;
  for (size_t r = 0; r < P.order.size(); ++r) {
    const Launch& L = plan.launches[P.order[r]];
    const uint64_t cur = P.batches.empty() ? 0 : P.batches.back().blocks;
    if (P.batches.empty() || P.batches.back().count == max_segs || cur + (uint64_t)L.blocks > max_blocks ||
        (cur > 0 && cur + L.blocks / 2 > target && P.batches.size() < nlaunch))  // fits the next batch better
      P.batches.push_back({r, 0, 0});
    P.batches.back().count++;
    P.batches.back().blocks += L.blocks;
    P.total_blocks += L.blocks;
  }
  return P;
}

// The segment table of launch `B` into segs[0 .. B.count): what k_scan walks
// to find a tile's piece.  tabptr[i] is the K+W table of plan.launches[i]
// (MODE 5 / 7 pieces; indexed by plan index, not by position in the order).
// Adds the launch to `c`.  Returns "" or an error.
inline std::string fill_segments(const Plan& plan, const ScanPack& P, const ScanBatch& B, const uint64_t* tabptr,
                                 Segment* segs, ScanCounters& c) {
  uint32_t block0 = 0;
  for (size_t j = 0; j < B.count; ++j) {
    const size_t i = P.order[B.first + j];
    const Launch& L = plan.launches[i];
    Segment& S = segs[j];
    memset(&S, 0, sizeof S);
    S.block0 = block0;
    block0 += L.blocks;
    if (L.fast) {
      if (!has_variant(L.fv, L.mode, L.trail)) return "no fast kernel variant";
      S.kind = variant_id(L.fv, L.mode, L.trail);
      S.fa = L.fa;
      if (L.mode == 5 || L.mode == 7) S.fa.kwtab = tabptr[i];
      c.fast_launches++;
      c.fast_nonces += L.nonces;
      c.fast_ops += L.nonces * kAlgOpsPerCompression * (uint64_t)L.btail;
    } else {
      S.kind = kGenericKind;
      S.ga = L.ga;
      c.gen_launches++;
      c.gen_nonces += L.nonces;
    }
    c.scan_nonces += L.nonces;
    c.scan_ops += L.nonces * kAlgOpsPerCompression * (uint64_t)L.btail;
  }
  c.scan_launches++;
  return "";
}

// k_scan_small's argument block for a generic-only plan: pieces, first
// workgroups, counts.  The four pointers are the caller's to set.  Adds the
// launch to `c`.  Returns "" or an error.
inline std::string fill_small(const Plan& plan, SmallArgs& a, ScanCounters& c) {
  if (plan.launches.size() > kSmallMaxSegs || plan.total_blocks > kSmallMaxBlocks)
    return "internal: small plan exceeds its argument block";
  memset(&a, 0, sizeof a);
  uint32_t block0 = 0;
  for (size_t i = 0; i < plan.launches.size(); ++i) {
    const Launch& L = plan.launches[i];
    a.ga[i] = L.ga;
    a.block0[i] = block0;
    block0 += L.blocks;
    c.gen_launches++;
    c.gen_nonces += L.nonces;
    c.scan_ops += L.nonces * kAlgOpsPerCompression * (uint64_t)L.btail;
  }
  a.nseg = (uint32_t)plan.launches.size();
  a.nblocks = block0;
  c.scan_launches++;
  c.scan_nonces += plan.total_nonces;
  return "";
}

}  // namespace p1
