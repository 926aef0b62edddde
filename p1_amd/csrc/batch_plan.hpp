// batch_plan.hpp -- host side of p1hip_scan_batch that needs no device: which
// requests are coalesced, how the coalesced ones are laid out over devices
// and launch pairs, and the segment table of one launch pair.  p1hip.hip
// (p1hip_scan_batch, p1hip_batch_layout) and tools/batch_emu share it, so the
// host replay builds its tables with the library's own code.
#pragma once
#include <string>
#include <vector>

#include "batch_abi.hpp"
#include "planner.hpp"

namespace p1 {

struct BatchReq {
  const uint8_t* msg;
  size_t len;
  uint64_t lower, upper;  // inclusive; lower > upper: empty
};

// Tiles (workgroups of kBlock nonces) of a non-empty request run on the
// generic path: every decade piece starts a tile of its own, as in
// make_plan(..., fast_ok = false).
inline uint64_t batch_req_tiles(uint64_t lower, uint64_t upper) {
  uint64_t tiles = 0;
  for (int d = 1; d <= 20; ++d) {
    const uint64_t dlo = (d == 1) ? 0u : pow10u(d - 1);
    const uint64_t dhi = (d == 20) ? ~0ull : pow10u(d) - 1u;
    const uint64_t s = lower > dlo ? lower : dlo;
    const uint64_t e = upper < dhi ? upper : dhi;
    if (s > e) continue;
    tiles += (e - s) / kBlock + 1;  // ceil((e - s + 1) / kBlock) without overflow
  }
  return tiles;
}

// One launch pair: the requests (indices into the call's array, in order) it
// answers on one device.
struct BatchLaunch {
  int device;  // index into the open devices
  int launch;  // launch pair of that device, from 0
  std::vector<size_t> reqs;
  uint32_t tiles = 0;
};

struct BatchLayout {
  // per request: tiles (0: empty range, or run individually), device and
  // launch of its coalesced launch pair (-1: empty or individual)
  std::vector<uint32_t> tiles;
  std::vector<int32_t> device, launch;
  std::vector<BatchLaunch> launches;  // by device, then by launch
  uint64_t coalesced = 0, individual = 0, empty = 0;
};

// Lay `n` requests out over `ndev` devices.  A non-empty request of at most
// `max_nonces` nonces is coalesced.  The coalesced requests are cut, in
// request order, into `ndev` contiguous groups of near-equal tile count (a
// request goes to the device in whose share of the tiles its middle falls),
// one group per device; a device's group is cut into launch pairs that close
// when the next request's tiles would pass `max_tiles` (raised to the largest
// single request, so a request is never split).
inline BatchLayout batch_layout(const BatchReq* reqs, size_t n, int ndev, uint64_t max_nonces, uint64_t max_tiles) {
  BatchLayout Y;
  Y.tiles.assign(n, 0);
  Y.device.assign(n, -1);
  Y.launch.assign(n, -1);
  if (max_nonces > kBatchMaxNonces) max_nonces = kBatchMaxNonces;
  if (max_tiles == 0 || max_tiles > kBatchMaxTiles) max_tiles = kBatchMaxTiles;
  uint64_t total = 0;
  for (size_t i = 0; i < n; ++i) {
    const BatchReq& q = reqs[i];
    if (q.lower > q.upper) {
      Y.empty++;
    } else if (q.upper - q.lower >= max_nonces) {  // more than max_nonces nonces (or max_nonces == 0)
      Y.individual++;
    } else {
      Y.tiles[i] = (uint32_t)batch_req_tiles(q.lower, q.upper);
      total += Y.tiles[i];
      if (Y.tiles[i] > max_tiles) max_tiles = Y.tiles[i];
      Y.coalesced++;
    }
  }
  uint64_t before = 0;
  for (size_t i = 0; i < n; ++i) {
    const uint64_t t = Y.tiles[i];
    if (t == 0) continue;
    // middle of the request in units of half tiles: (2 * before + t) / (2 * total) of the way
    uint64_t dev = (uint64_t)((unsigned __int128)(2 * before + t) * (uint64_t)ndev / (2 * total));
    if (dev >= (uint64_t)ndev) dev = (uint64_t)ndev - 1;
    before += t;
    if (Y.launches.empty() || Y.launches.back().device != (int)dev) {
      BatchLaunch L;
      L.device = (int)dev;
      L.launch = 0;
      Y.launches.push_back(L);
    } else if ((uint64_t)Y.launches.back().tiles + t > max_tiles) {
      BatchLaunch L;
      L.device = (int)dev;
      L.launch = Y.launches.back().launch + 1;
      Y.launches.push_back(L);
    }
    BatchLaunch& L = Y.launches.back();
    L.reqs.push_back(i);
    L.tiles += (uint32_t)t;
    Y.device[i] = L.device;
    Y.launch[i] = L.launch;
  }
  return Y;
}

// The tables of one launch pair.
struct BatchTable {
  std::vector<BatchSeg> segs;       // k_batch_scan's table, block0 strictly increasing
  std::vector<uint32_t> req_tile0;  // k_batch_reduce's: request r owns tiles [req_tile0[r], req_tile0[r + 1])
  uint64_t nonces = 0;
};

// Build the tables of launch pair L; "" or the planner's error.
inline std::string batch_build_table(const BatchReq* reqs, const BatchLaunch& L, BatchTable& T) {
  T.segs.clear();
  T.req_tile0.clear();
  T.nonces = 0;
  uint32_t tile = 0;
  Plan plan;
  for (size_t r = 0; r < L.reqs.size(); ++r) {
    const BatchReq& q = reqs[L.reqs[r]];
    std::string err = make_plan(q.msg, q.len, q.lower, q.upper, plan, false);
    if (!err.empty()) return "request " + std::to_string(L.reqs[r]) + ": planner: " + err;
    T.req_tile0.push_back(tile);
    for (const Launch& P : plan.launches) {
      BatchSeg S;
      memset(&S, 0, sizeof S);
      S.ga = P.ga;
      S.ga.part_off = 0;
      S.block0 = tile;
      S.req = (uint32_t)r;
      T.segs.push_back(S);
      tile += P.blocks;
    }
    T.nonces += plan.total_nonces;
  }
  T.req_tile0.push_back(tile);
  if (tile != L.tiles) return "internal: batch table has " + std::to_string(tile) + " tiles, layout " + std::to_string(L.tiles);
  return std::string();
}

}  // namespace p1
