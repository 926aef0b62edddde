// tile_map.hpp -- TEST SUPPORT, host only, no HIP call: which nonces each tile
// of a scan covers.  For a Plan and its ScanPack (scan_pack.hpp) it lists the
// tiles in partial-array order -- launch by launch, and inside a launch
// segment by segment as fill_segments lays them out -- with the exact nonce
// set of each, so that a test can compare every 16-byte partial k_scan (or
// k_scan_small) wrote with the oracle's minimum over that set.  p1hip.hip
// returns it from p1hip_scan_tiles for the plan it launched, tools/p1emu
// prints it next to the partials it replays (`tiles`).
//
// The sets are derived from the Launch fields alone (threads per hi value,
// fa.hi_first / nthreads / kpow / nsub, ga.lo / count) and the pack order;
// nothing here calls the per-thread code of scan_core.hpp.
#pragma once
#include <vector>

#include "scan_pack.hpp"

namespace p1 {

// `count` runs of `run_len` consecutive nonces: run i starts at
// first + i * stride (stride 0 when count == 1).
struct TileRun {
  uint64_t first, stride;
  uint32_t run_len, count;
};

constexpr uint32_t kTileMaxRuns = kBlock / 64;  // one per wave

struct TileInfo {
  uint32_t launch;  // k_scan launch of the scan, from 0
  uint32_t tile;    // tile (workgroup-sized piece of work) within that launch
  uint32_t kind;    // the segment's: variant_id(...) or kGenericKind
  uint32_t k;       // lo digits per thread (fast), 0 (generic)
  uint32_t nruns;   // 0: no valid thread, the partial is (2^64-1, 2^64-1)
  TileRun runs[kTileMaxRuns];
};

// Tile `t` (from 0) of piece L.
inline void tile_runs(const Launch& L, uint32_t t, TileInfo& T) {
  T.nruns = 0;
  memset(T.runs, 0, sizeof T.runs);
  const uint64_t tid0 = (uint64_t)t * kBlock;  // the tile's first thread within the piece
  if (!L.fast) {
    T.kind = kGenericKind;
    T.k = 0;
    if (tid0 >= L.ga.count) return;
    const uint64_t left = L.ga.count - tid0;
    T.runs[T.nruns++] = {L.ga.lo + tid0, 0, (uint32_t)(left < kBlock ? left : kBlock), 1};
    return;
  }
  T.kind = variant_id(L.fv, L.mode, L.trail);
  T.k = (uint32_t)L.Y.k;
  const FastArgs& A = L.fa;
  if (A.nsub <= 1) {
    // one thread per hi value, 10^k consecutive nonces each: threads tid0 ..
    // of the valid ones together hold one contiguous run
    if (tid0 >= A.nthreads) return;
    const uint64_t left = A.nthreads - tid0;
    const uint32_t cnt = (uint32_t)(left < kBlock ? left : kBlock);
    T.runs[T.nruns++] = {(A.hi_first + tid0) * A.kpow, 0, cnt * A.kpow, 1};
    return;
  }
  // MODE 5 with k = 4..7: wave w of the piece takes rows [sub * per, sub * per
  // + per) of the hi values (w / nsub) * 64 + lane, sub = w % nsub
  const uint32_t per = A.kpow / A.nsub;
  for (uint32_t wl = 0; wl < kTileMaxRuns; ++wl) {
    const uint64_t w = tid0 / 64 + wl;
    const uint64_t sub = w % A.nsub, hid0 = w / A.nsub * 64;
    if (hid0 >= A.nthreads) continue;
    const uint64_t left = A.nthreads - hid0;
    T.runs[T.nruns++] = {(A.hi_first + hid0) * A.kpow + sub * per, A.kpow, per, (uint32_t)(left < 64 ? left : 64)};
  }
}

// Every tile of a packed scan, in the order of its partial array (the launches
// write consecutive slices of it: p1hip.hip run_range's part_off).
inline std::vector<TileInfo> tile_map(const Plan& plan, const ScanPack& P) {
  std::vector<TileInfo> out;
  out.reserve(P.total_blocks);
  for (size_t bi = 0; bi < P.batches.size(); ++bi) {
    const ScanBatch& B = P.batches[bi];
    uint32_t tile = 0;
    for (size_t j = 0; j < B.count; ++j) {
      const Launch& L = plan.launches[P.order[B.first + j]];
      for (uint32_t t = 0; t < L.blocks; ++t) {
        TileInfo T;
        T.launch = (uint32_t)bi;
        T.tile = tile++;
        tile_runs(L, t, T);
        out.push_back(T);
      }
    }
  }
  return out;
}

// The tiles of k_scan_small's one launch (fill_small: pieces in plan order).
inline std::vector<TileInfo> tile_map_small(const Plan& plan) {
  std::vector<TileInfo> out;
  out.reserve(plan.total_blocks);
  uint32_t tile = 0;
  for (const Launch& L : plan.launches)
    for (uint32_t t = 0; t < L.blocks; ++t) {
      TileInfo T;
      T.launch = 0;
      T.tile = tile++;
      tile_runs(L, t, T);
      out.push_back(T);
    }
  return out;
}

}  // namespace p1
