// wide_plan.hpp -- host side of p1hip_scan_batch_wide that needs no device:
// the route of every request, the split of the wide requests over devices,
// their plans, the packing of all their fast pieces into shared k_scan
// launches, the one k_batch_scan table of their generic pieces and the range
// table k_wide_reduce folds by.  p1hip.hip (p1hip_scan_batch_wide,
// p1hip_wide_layout) and tools/batch_emu share it, so the host replay runs
// the library's own tables.
//
// A request of 10^5..10^7 nonces does not fill the device: run alone it is a
// handful of segments and a few dozen tiles on a device that holds ~1024
// workgroups.  A Segment of k_scan is self-contained (FastArgs / GenArgs carry
// the message's chaining value and tail template), so the fast pieces of many
// requests -- of any messages -- go into one segment table, at most kMaxSegs
// per launch, and one k_scan launch runs them all.
//
// The partial array of a device, in tiles:
//   [k_scan launch 0][k_scan launch 1] ... [generic tiles (k_batch_scan)]
// Inside a launch the pieces keep pack_scan's order, longest-running first
// across all requests, so a request's partials are not contiguous: each
// request owns a list of ranges (one per fast piece, one for its generic
// tiles, which lie request after request).
#pragma once
#include <algorithm>
#include <string>
#include <vector>

#include "batch_plan.hpp"
#include "scan_pack.hpp"

namespace p1 {

// A request above kBatchMaxNonces and of at most this many nonces is wide.
constexpr uint64_t kWideMaxNonces = 1ull << 24;
// Tiles of one device's partial array in one call (2^24 partials of 16 bytes
// = 256 MB).  A wide request that would pass it runs individually instead.
constexpr uint64_t kWideMaxTiles = 1ull << 24;

// p1hip_wide_layout's route[i]
enum : int32_t { kWideRouteEmpty = 0, kWideRouteSmall = 1, kWideRouteWide = 2, kWideRouteIndividual = 3 };

// The occupancy floor the wide requests of one device are planned with.
// make_plan lowers k (10^k nonces per thread) until a decade has at least
// `min_fast_threads` threads; its default, kMinFastThreads = 2^18, is what
// fills the device from ONE request.  Here the device is filled by the sum of
// the threads that share a k_scan launch, and at most `max_segs` requests
// share one (each has at least one fast segment), so each request only has to
// bring its share: 2^18 / min(requests on the device, max_segs), rounded up.
// Few requests keep the per-request floor (k drops as for a lone scan, which
// shortens the tiles and with them the drain); many requests keep k = 3, the
// cheapest code per nonce.
inline uint64_t wide_min_fast_threads(size_t wide_on_device, uint32_t max_segs) {
  const uint64_t sharers = std::max<uint64_t>(1, std::min<uint64_t>(wide_on_device, max_segs));
  return std::max<uint64_t>(1, (kMinFastThreads + sharers - 1) / sharers);
}

// One fast piece in a device's packing order.
struct WideFast {
  uint32_t req;    // index into WideDevice::reqs
  uint32_t piece;  // index into that request's plan.launches
};

// One k_scan launch: pieces fast[first .. first + count).
struct WideLaunch {
  size_t first, count;
  uint32_t tile0;  // first tile of the launch in the device's partial array
  uint32_t tiles;
};

struct WideDevice {
  std::vector<size_t> reqs;          // the call's request indices answered here, in order
  std::vector<Plan> plans;           // one per request
  uint64_t min_fast_threads = 0;     // what they were planned with
  std::vector<WideFast> fast;        // every fast piece, longest-running first
  std::vector<WideLaunch> launches;  // k_scan launches, in order
  std::vector<BatchSeg> gsegs;       // k_batch_scan's table (block0 from 0), request after request
  uint32_t gen_tile0 = 0, gen_tiles = 0;  // the generic tiles' place in the partial array
  // k_wide_reduce's tables: request r owns ranges[req_range0[r] .. req_range0[r + 1])
  std::vector<WideRange> ranges;
  std::vector<int32_t> range_launch;  // k_scan launch of the range; -1: the generic tiles
  std::vector<uint32_t> req_range0;
  uint32_t total_tiles = 0;
  uint64_t nonces = 0;
};

struct WideLayout {
  // per request of the call
  std::vector<int32_t> route, device;  // device: of a wide request, else -1
  std::vector<uint32_t> segs, tiles;   // wide: its k_scan segments and all its tiles, else 0
  std::vector<WideDevice> devs;        // one per device
  uint64_t empty = 0, small = 0, wide = 0, individual = 0;
};

// Predicted cost of [lower, upper] (lower <= upper): nonces x nonce_cycles per decade.
inline double wide_cost(const uint8_t* msg, size_t len, uint64_t lower, uint64_t upper) {
  Prefix P;
  make_prefix(msg, len, P);
  double c = 0.0;
  for (int d = 1; d <= 20; ++d) {
    const uint64_t dlo = (d == 1) ? 0u : pow10u(d - 1);
    const uint64_t dhi = (d == 20) ? ~0ull : pow10u(d) - 1u;
    const uint64_t s = lower > dlo ? lower : dlo;
    const uint64_t e = upper < dhi ? upper : dhi;
    if (s <= e) c += ((double)(e - s) + 1.0) * nonce_cycles(P, d);
  }
  return c;
}

// The k_scan segment of fast piece L at first tile `block0` of its launch
// (fill_segments' fast branch; a wide plan has no MODE 5 / 7 piece, so no table).
inline std::string wide_fill_segment(const Launch& L, uint32_t block0, Segment& S) {
  if (!L.fast || L.mode == 5 || L.mode == 7) return "internal: wide piece is not a table-free fast piece";
  if (!has_variant(L.fv, L.mode, L.trail)) return "no fast kernel variant";
  memset(&S, 0, sizeof S);
  S.kind = variant_id(L.fv, L.mode, L.trail);
  S.block0 = block0;
  S.fa = L.fa;
  S.fa.part_off = 0;
  return "";
}

// The segment table of k_scan launch `W` of device `D` into segs[0 .. W.count).
inline std::string wide_fill_launch(const WideDevice& D, const WideLaunch& W, Segment* segs) {
  uint32_t block0 = 0;
  for (size_t j = 0; j < W.count; ++j) {
    const WideFast& f = D.fast[W.first + j];
    const Launch& L = D.plans[f.req].launches[f.piece];
    const std::string err = wide_fill_segment(L, block0, segs[j]);
    if (!err.empty()) return "request " + std::to_string(D.reqs[f.req]) + ": " + err;
    block0 += L.blocks;
  }
  if (block0 != W.tiles) return "internal: wide launch tile count";
  return "";
}

// Route `n` requests and lay the wide ones out over `ndev` devices.
//   small_max  a non-empty request of at most this many nonces is `small`
//              (p1hip_scan_batch's coalesced launch pair)
//   wide_max   above that and at most this many: wide
//   max_segs   segments per k_scan launch (kMaxSegs; tests cut launches small)
//   fast_floor 0: wide_min_fast_threads per device; else the floor itself
//   max_tiles  tiles of one device's partial array (kWideMaxTiles; tests cut it
//              small so that requests are turned away for lack of room)
// The wide requests are cut, in request order, into `ndev` contiguous groups
// of near-equal predicted cost (a request goes to the device in whose share
// of the cost its middle falls).  Returns "" or an error naming the request.
inline std::string wide_layout(const BatchReq* reqs, size_t n, int ndev, uint64_t small_max, uint64_t wide_max,
                               uint32_t max_segs, uint64_t fast_floor, bool split, WideLayout& Y,
                               uint64_t max_tiles = kWideMaxTiles) {
  Y = WideLayout();
  Y.route.assign(n, kWideRouteEmpty);
  Y.device.assign(n, -1);
  Y.segs.assign(n, 0);
  Y.tiles.assign(n, 0);
  Y.devs.resize((size_t)ndev);
  if (small_max > kBatchMaxNonces) small_max = kBatchMaxNonces;
  if (max_segs == 0 || max_segs > kMaxSegs) max_segs = kMaxSegs;
  std::vector<double> cost(n, 0.0);
  double total = 0.0;
  for (size_t i = 0; i < n; ++i) {
    const BatchReq& q = reqs[i];
    if (q.lower > q.upper) {
      Y.empty++;
    } else if (q.upper - q.lower < small_max) {
      Y.route[i] = kWideRouteSmall;
      Y.small++;
    } else if (q.upper - q.lower < wide_max) {
      Y.route[i] = kWideRouteWide;
      cost[i] = wide_cost(q.msg, q.len, q.lower, q.upper);
      total += cost[i];
    } else {
      Y.route[i] = kWideRouteIndividual;
    }
  }
  double before = 0.0;
  for (size_t i = 0; i < n; ++i) {
    if (Y.route[i] != kWideRouteWide) continue;
    int dev = total > 0.0 ? (int)((before + cost[i] / 2) * ndev / total) : 0;
    dev = std::min(std::max(dev, 0), ndev - 1);
    before += cost[i];
    Y.device[i] = dev;
    Y.devs[(size_t)dev].reqs.push_back(i);
  }
  for (int dv = 0; dv < ndev; ++dv) {
    WideDevice& D = Y.devs[(size_t)dv];
    D.min_fast_threads = fast_floor ? fast_floor : wide_min_fast_threads(D.reqs.size(), max_segs);
    // plan; a request whose tiles would pass the device's partial array runs individually
    std::vector<size_t> kept;
    uint64_t tiles = 0;
    for (size_t i : D.reqs) {
      const BatchReq& q = reqs[i];
      Plan plan;
      const std::string err = make_plan(q.msg, q.len, q.lower, q.upper, plan, true, D.min_fast_threads, split, false);
      if (!err.empty()) return "request " + std::to_string(i) + ": planner: " + err;
      if (tiles + plan.total_blocks > max_tiles) {
        Y.route[i] = kWideRouteIndividual;
        Y.device[i] = -1;
        continue;
      }
      tiles += plan.total_blocks;
      Y.tiles[i] = plan.total_blocks;
      D.nonces += plan.total_nonces;
      kept.push_back(i);
      D.plans.push_back(std::move(plan));
    }
    D.reqs.swap(kept);
    D.total_tiles = (uint32_t)tiles;
    // every fast piece of the device, longest-running workgroups first
    // (pack_scan's weight: lo-loop length x tail blocks); ties stay in request order
    std::vector<uint64_t> weight;
    for (size_t r = 0; r < D.reqs.size(); ++r)
      for (size_t p = 0; p < D.plans[r].launches.size(); ++p) {
        const Launch& L = D.plans[r].launches[p];
        if (!L.fast) continue;
        D.fast.push_back({(uint32_t)r, (uint32_t)p});
        weight.push_back((uint64_t)(L.fa.kpow / L.fa.nsub) * (uint64_t)L.btail);
      }
    std::vector<size_t> order(D.fast.size());
    for (size_t j = 0; j < order.size(); ++j) order[j] = j;
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return weight[a] > weight[b]; });
    std::vector<WideFast> sorted(D.fast.size());
    for (size_t j = 0; j < order.size(); ++j) sorted[j] = D.fast[order[j]];
    D.fast.swap(sorted);
    // cut into launches of at most max_segs segments and kMaxLaunchBlocks tiles;
    // a request's ranges are gathered per request first, then flattened
    std::vector<std::vector<std::pair<WideRange, int32_t>>> per(D.reqs.size());
    uint32_t tile = 0;
    for (size_t j = 0; j < D.fast.size(); ++j) {
      const WideFast& f = D.fast[j];
      const Launch& L = D.plans[f.req].launches[f.piece];
      if (D.launches.empty() || D.launches.back().count == max_segs ||
          (uint64_t)D.launches.back().tiles + L.blocks > kMaxLaunchBlocks)
        D.launches.push_back({j, 0, tile, 0});
      WideLaunch& W = D.launches.back();
      per[f.req].push_back({WideRange{tile, L.blocks}, (int32_t)D.launches.size() - 1});
      W.count++;
      W.tiles += L.blocks;
      tile += L.blocks;
      Y.segs[D.reqs[f.req]]++;
    }
    // the generic pieces: one k_batch_scan table, request after request
    D.gen_tile0 = tile;
    for (size_t r = 0; r < D.reqs.size(); ++r) {
      const uint32_t first = D.gen_tiles;
      for (const Launch& L : D.plans[r].launches) {
        if (L.fast) continue;
        BatchSeg S;
        memset(&S, 0, sizeof S);
        S.ga = L.ga;
        S.ga.part_off = 0;
        S.block0 = D.gen_tiles;
        S.req = (uint32_t)r;
        D.gsegs.push_back(S);
        D.gen_tiles += L.blocks;
      }
      if (D.gen_tiles > first) per[r].push_back({WideRange{D.gen_tile0 + first, D.gen_tiles - first}, -1});
    }
    if ((uint64_t)tile + D.gen_tiles != tiles) return "internal: wide layout tile count";
    for (size_t r = 0; r < D.reqs.size(); ++r) {
      D.req_range0.push_back((uint32_t)D.ranges.size());
      for (const auto& rg : per[r]) {
        D.ranges.push_back(rg.first);
        D.range_launch.push_back(rg.second);
      }
    }
    D.req_range0.push_back((uint32_t)D.ranges.size());
    Y.wide += D.reqs.size();
  }
  for (size_t i = 0; i < n; ++i) Y.individual += Y.route[i] == kWideRouteIndividual;
  return "";
}

}  // namespace p1
