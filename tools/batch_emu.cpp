// batch_emu -- TEST TOOL: replays a p1hip_scan_batch, p1hip_scan_batch_wide or
// p1hip_scan_below_batch call on the host.
//
// It lays the requests out with the library's own batch_layout, builds every
// launch pair's tables with the library's own batch_build_table
// (p1_amd/csrc/batch_plan.hpp), then replays k_batch_scan tile by tile (the
// shared lookup batch_find_seg, generic_thread per simulated thread, one
// partial per tile) and k_batch_reduce (the per-request fold of the
// partials).  So the table layout, the lookup and the fold can be
// parity-tested against the oracle in the CPU-only suite.  It is never part
// of libp1hip.so and never used to produce a product result.
//
// usage: batch_emu [ndev [max_tiles]] < requests
//   stdin: one request per line, "<msg-hex|-> <lower> <upper>"
//   stdout: "<hash> <nonce>" per request, in request order
//   stderr: "launches=<n> tiles=<n> segs=<n>"
//   a non-empty request of more than 2^16 nonces (which the library runs on
//   its own through p1hip_scan) is refused: exit status 1
//
// usage: batch_emu wide [ndev [max_segs [F]]] < requests
//   replays p1hip_scan_batch_wide with the library's own wide_layout
//   (p1_amd/csrc/wide_plan.hpp; max_segs segments per k_scan launch, 0 = the
//   library's 64; F = the occupancy floor, 0 = the library's rule): per
//   device the partial array, k_batch_scan over the generic table into its
//   place in it, every k_scan launch tile by tile from the launch's segment
//   table (scan_replay.hpp, shared with tools/p1emu), then k_wide_reduce's
//   fold of each request's ranges (batch_abi.hpp wide_fold_thread).  Small
//   requests go through the batch replay above.  Every tile must be written
//   exactly once and every range must lie inside the array.
//   stderr: "launches=<k_scan launches> tiles=<n> segs=<k_scan segments> gsegs=<n> ranges=<n> small=<n> wide=<n>"
//   a request above 2^24 nonces is refused: exit status 1
//
// usage: batch_emu below <ndev> [maxslice=N] [corrupt=K] < requests
//   replays p1hip_scan_below_batch with the library's own belowb_plan.hpp:
//   routes, rounds, the layout of every round with its tile and slot caps and
//   the tables; per launch pair k_belowb_mark (below_thread per simulated
//   thread against the request's own target, one word per wave),
//   k_belowb_collect (belowb_collect_replay: the shared word expansion) and
//   the library's decoder.  maxslice=N is P1HIP_BELOW_MAX_SLICE.  corrupt=K
//   adds 1 to the K-th index the first launch pair returns before it is
//   decoded (the decoder must refuse it: exit status 1).
//   stdin: one request per line, "<msg-hex|-> <lower> <upper> <target> <cap>"
//   stdout: per request one line, "<found>" and then " <hash>:<nonce>" per hit
//   stderr: "rounds=<n> launches=<n> tiles=<n> slots=<n> coalesced=<n> empty=<n>"
//   a request on the individual route is refused: exit status 1
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <string>
#include <thread>
#include <vector>

#include "../p1_amd/csrc/belowb_plan.hpp"
#include "../p1_amd/csrc/wide_plan.hpp"
#include "scan_replay.hpp"

using namespace p1;

static std::vector<uint8_t> unhex(const char* s) {
  std::vector<uint8_t> v;
  size_t n = strlen(s);
  for (size_t i = 0; i + 1 < n; i += 2) {
    unsigned b;
    sscanf(s + i, "%2x", &b);
    v.push_back((uint8_t)b);
  }
  return v;
}

// fn(b) for every tile b of a grid, on a few host threads (a wide call is
// tens of millions of hashes); tiles are independent, as on the device
template <typename Fn>
static void for_tiles(uint32_t tiles, Fn&& fn) {
  unsigned nt = std::thread::hardware_concurrency();
  nt = nt < 1 ? 1 : nt > 16 ? 16 : nt;
  if (tiles < 64) nt = 1;
  std::atomic<uint32_t> next{0};
  auto work = [&]() {
    for (uint32_t b; (b = next.fetch_add(1, std::memory_order_relaxed)) < tiles;) fn(b);
  };
  std::vector<std::thread> th;
  for (unsigned i = 1; i < nt; ++i) th.emplace_back(work);
  work();
  for (std::thread& t : th) t.join();
}

struct BatchInfo {
  uint64_t launches = 0, tiles = 0, segs = 0;
};

// The p1hip_scan_batch replay of `reqs` (all of at most 2^16 nonces, or empty).
static int replay_batch(const std::vector<BatchReq>& reqs, int ndev, uint64_t max_tiles, std::vector<Key>& out,
                        BatchInfo& info) {
  const size_t n = reqs.size();
  const BatchLayout Y = batch_layout(reqs.data(), n, ndev, kBatchMaxNonces, max_tiles);
  if (Y.individual) {
    fprintf(stderr, "%" PRIu64 " request(s) above 2^16 nonces: not a batch replay\n", Y.individual);
    return 1;
  }
  out.assign(n, Key{~0ull, 0});  // empty ranges keep the identity
  BatchTable T;
  for (const BatchLaunch& L : Y.launches) {
    std::string err = batch_build_table(reqs.data(), L, T);
    if (!err.empty()) {
      fprintf(stderr, "table error: %s\n", err.c_str());
      return 1;
    }
    // k_batch_scan: grid = L.tiles workgroups of kBlock threads
    std::vector<Key> part(L.tiles);
    for (uint32_t blk = 0; blk < L.tiles; ++blk) {
      const BatchSeg& S = T.segs[batch_find_seg(T.segs.data(), (uint32_t)T.segs.size(), blk)];
      Key m = {~0ull, ~0ull};
      for (uint32_t t = 0; t < (uint32_t)kBlock; ++t) {
        const Key k = generic_thread(S.ga, (uint64_t)(blk - S.block0) * kBlock + t);
        if (key_lt(k, m)) m = k;
      }
      part[blk] = m;
    }
    // k_batch_reduce: grid = requests of the launch
    for (size_t r = 0; r < L.reqs.size(); ++r) {
      Key m = {~0ull, ~0ull};
      for (uint32_t i = T.req_tile0[r]; i < T.req_tile0[r + 1]; ++i)
        if (key_lt(part[i], m)) m = part[i];
      if (m.h == ~0ull) m.n = 0;  // identity of miner.go:56
      out[L.reqs[r]] = m;
    }
    info.tiles += L.tiles;
    info.segs += T.segs.size();
  }
  info.launches += Y.launches.size();
  return 0;
}

// The p1hip_scan_batch_wide replay.
static int replay_wide(const std::vector<BatchReq>& reqs, int ndev, uint32_t max_segs, uint64_t floor,
                       std::vector<Key>& out) {
  const size_t n = reqs.size();
  WideLayout Y;
  const std::string lerr = wide_layout(reqs.data(), n, ndev, kBatchMaxNonces, kWideMaxNonces, max_segs, floor, true, Y);
  if (!lerr.empty()) {
    fprintf(stderr, "layout error: %s\n", lerr.c_str());
    return 1;
  }
  if (Y.individual) {
    fprintf(stderr, "%" PRIu64 " request(s) above 2^24 nonces: not a wide replay\n", Y.individual);
    return 1;
  }
  out.assign(n, Key{~0ull, 0});
  // small route
  std::vector<BatchReq> sq;
  std::vector<size_t> sidx;
  for (size_t i = 0; i < n; ++i)
    if (Y.route[i] == kWideRouteSmall) {
      sq.push_back(reqs[i]);
      sidx.push_back(i);
    }
  if (!sq.empty()) {
    std::vector<Key> so;
    BatchInfo bi;
    if (int rc = replay_batch(sq, ndev, kBatchMaxTiles, so, bi)) return rc;
    for (size_t j = 0; j < sidx.size(); ++j) out[sidx[j]] = so[j];
  }
  uint64_t launches = 0, tiles = 0, segs = 0, gsegs = 0, ranges = 0;
  const Key unwritten = {0x756e7772697474ull, 0x656eull};  // every tile must be overwritten
  for (const WideDevice& D : Y.devs) {
    if (D.reqs.empty()) continue;
    std::vector<Key> part(D.total_tiles, unwritten);
    std::vector<uint8_t> written(D.total_tiles, 0);
    // k_batch_scan: grid = D.gen_tiles, part + D.gen_tile0
    if (D.gen_tiles) {
      if ((uint64_t)D.gen_tile0 + D.gen_tiles > D.total_tiles) {
        fprintf(stderr, "generic tiles outside the partial array\n");
        return 1;
      }
      for_tiles(D.gen_tiles, [&](uint32_t blk) {
        const BatchSeg& S = D.gsegs[batch_find_seg(D.gsegs.data(), (uint32_t)D.gsegs.size(), blk)];
        Key m = {~0ull, ~0ull};
        for (uint32_t t = 0; t < (uint32_t)kBlock; ++t) {
          const Key k = generic_thread(S.ga, (uint64_t)(blk - S.block0) * kBlock + t);
          if (key_lt(k, m)) m = k;
        }
        part[D.gen_tile0 + blk] = m;
        written[D.gen_tile0 + blk]++;
      });
    }
    // k_scan launches: ntiles = W.tiles, part + W.tile0
    std::vector<Segment> tab;
    for (const WideLaunch& W : D.launches) {
      if (W.count > max_segs || (uint64_t)W.tile0 + W.tiles > D.total_tiles) {
        fprintf(stderr, "launch of %zu segments / tiles outside the partial array\n", W.count);
        return 1;
      }
      tab.assign(W.count, Segment());
      const std::string err = wide_fill_launch(D, W, tab.data());
      if (!err.empty()) {
        fprintf(stderr, "segment error: %s\n", err.c_str());
        return 1;
      }
      for_tiles(W.tiles, [&](uint32_t b) {
        part[W.tile0 + b] = replay_scan_tile(tab.data(), (uint32_t)W.count, b);
        written[W.tile0 + b]++;
      });
      segs += W.count;
    }
    for (uint32_t t = 0; t < D.total_tiles; ++t)
      if (written[t] != 1) {
        fprintf(stderr, "tile %u written %u times\n", t, (unsigned)written[t]);
        return 1;
      }
    // k_wide_reduce: grid = requests of the device; every range inside the
    // array, every tile in exactly one range
    std::vector<uint8_t> owned(D.total_tiles, 0);
    for (size_t r = 0; r < D.reqs.size(); ++r) {
      for (uint32_t j = D.req_range0[r]; j < D.req_range0[r + 1]; ++j) {
        const WideRange R = D.ranges[j];
        if ((uint64_t)R.tile0 + R.ntiles > D.total_tiles || R.ntiles == 0) {
          fprintf(stderr, "range %u outside the partial array\n", j);
          return 1;
        }
        for (uint32_t t = 0; t < R.ntiles; ++t) owned[R.tile0 + t]++;
      }
      Key m = {~0ull, ~0ull};
      for (uint32_t t = 0; t < (uint32_t)kBlock; ++t) {
        const Key k = wide_fold_thread(part.data(), D.ranges.data(), D.req_range0[r], D.req_range0[r + 1], t, kBlock);
        if (key_lt(k, m)) m = k;
      }
      if (m.h == ~0ull) m.n = 0;  // identity of miner.go:56
      out[D.reqs[r]] = m;
    }
    for (uint32_t t = 0; t < D.total_tiles; ++t)
      if (owned[t] != 1) {
        fprintf(stderr, "tile %u in %u ranges\n", t, (unsigned)owned[t]);
        return 1;
      }
    launches += D.launches.size();
    tiles += D.total_tiles;
    gsegs += D.gsegs.size();
    ranges += D.ranges.size();
  }
  fprintf(stderr,
          "launches=%" PRIu64 " tiles=%" PRIu64 " segs=%" PRIu64 " gsegs=%" PRIu64 " ranges=%" PRIu64 " small=%" PRIu64
          " wide=%" PRIu64 "\n",
          launches, tiles, segs, gsegs, ranges, Y.small, Y.wide);
  return 0;
}

// The p1hip_scan_below_batch replay.
static int replay_below(const std::vector<BelowBReq>& reqs, int ndev, uint64_t max_slice, long corrupt) {
  const size_t n = reqs.size();
  std::vector<size_t> coalesced;
  uint64_t empty = 0;
  for (size_t i = 0; i < n; ++i) {
    const int route = belowb_route(reqs[i], kBelowAuto, max_slice);
    if (route == kBelowBIndividual) {
      fprintf(stderr, "request %zu takes the individual route: not a below batch replay\n", i);
      return 1;
    }
    if (route == kBelowBCoalesced) coalesced.push_back(i);
    else empty++;
  }
  std::vector<std::vector<Key>> res(n);
  std::vector<BelowBState> st(coalesced.size());
  for (size_t j = 0; j < coalesced.size(); ++j) st[j] = {reqs[coalesced[j]].lower, 0, false};
  uint64_t rounds = 0, nlaunch = 0, tiles = 0, slots = 0;
  std::vector<BelowBItem> items;
  BelowBTable B;
  std::vector<std::vector<Key>> got;
  const uint64_t unwritten = 0x756e7772697474ull;  // every word must be overwritten
  for (size_t left = coalesced.size(); left > 0; ++rounds) {
    std::string err = belowb_round_items(reqs.data(), coalesced, st, kBelowAuto, max_slice, items);
    if (!err.empty()) {
      fprintf(stderr, "round error: %s\n", err.c_str());
      return 1;
    }
    for (const BelowBLaunch& L : belowb_layout(items, ndev)) {
      err = belowb_build_table(reqs.data(), coalesced, items, L, B);
      if (!err.empty()) {
        fprintf(stderr, "table error: %s\n", err.c_str());
        return 1;
      }
      if (L.tiles > kBatchMaxTiles || L.slots > kBelowBatchMaxSlots) {
        fprintf(stderr, "launch pair of %u tiles, %llu slots\n", L.tiles, (unsigned long long)L.slots);
        return 1;
      }
      const size_t nreq = L.items.size();
      // k_belowb_mark: grid = L.tiles workgroups of kBlock threads, one word per wave
      std::vector<uint64_t> marks((size_t)L.tiles * kBelowWordsPerTile, unwritten);
      for_tiles(L.tiles, [&](uint32_t b) {
        const BatchSeg& S = B.T.segs[batch_find_seg(B.T.segs.data(), (uint32_t)B.T.segs.size(), b)];
        const uint64_t target = B.targets[S.req];
        for (uint32_t w = 0; w < kBelowWordsPerTile; ++w) {
          uint64_t word = 0;
          for (uint32_t l = 0; l < 64; ++l)
            if (below_thread(S.ga, (uint64_t)(b - S.block0) * kBlock + w * 64u + l, target)) word |= 1ull << l;
          marks[(size_t)b * kBelowWordsPerTile + w] = word;
        }
      });
      // k_belowb_collect: grid = requests of the launch pair
      std::vector<uint32_t> idx((size_t)L.slots + 1, ~0u), count(nreq, ~0u);
      for (uint32_t r = 0; r < (uint32_t)nreq; ++r)
        belowb_collect_replay(marks.data(), B.T.req_tile0.data(), B.req_hit0.data(), r, idx.data(), count.data());
      if (idx[L.slots] != ~0u) {
        fprintf(stderr, "an index past the launch pair's slots was written\n");
        return 1;
      }
      if (corrupt >= 0 && nlaunch == 0 && (uint64_t)corrupt < L.slots) idx[(size_t)corrupt] += 1;
      err = belowb_decode(B, idx.data(), count.data(), got);
      if (!err.empty()) {
        fprintf(stderr, "decode error: %s\n", err.c_str());
        return 1;
      }
      for (size_t r = 0; r < nreq; ++r) {
        const BelowBItem& it = items[L.items[r]];
        BelowBState& S = st[it.req];
        const size_t i = coalesced[it.req];
        for (const Key& k : got[r]) res[i].push_back(k);
        S.found += got[r].size();
        if (S.found == reqs[i].cap || it.hi == reqs[i].upper) {
          S.done = true;
          --left;
        } else {
          S.lo = it.hi + 1;
        }
      }
      nlaunch++;
      tiles += L.tiles;
      slots += L.slots;
    }
  }
  for (size_t i = 0; i < n; ++i) {
    printf("%zu", res[i].size());
    for (const Key& k : res[i]) printf(" %" PRIu64 ":%" PRIu64, k.h, k.n);
    printf("\n");
  }
  fprintf(stderr, "rounds=%" PRIu64 " launches=%" PRIu64 " tiles=%" PRIu64 " slots=%" PRIu64 " coalesced=%zu empty=%" PRIu64 "\n",
          rounds, nlaunch, tiles, slots, coalesced.size(), empty);
  return 0;
}

static int main_below(int argc, char** argv) {
  const int ndev = argc > 2 ? atoi(argv[2]) : 0;
  uint64_t max_slice = 0;
  long corrupt = -1;
  bool bad = ndev < 1;
  for (int i = 3; i < argc; ++i) {
    if (!strncmp(argv[i], "maxslice=", 9)) max_slice = strtoull(argv[i] + 9, nullptr, 10);
    else if (!strncmp(argv[i], "corrupt=", 8)) corrupt = atol(argv[i] + 8);
    else bad = true;
  }
  if (bad) {
    fprintf(stderr, "usage: %s below <ndev> [maxslice=N] [corrupt=K] < requests\n", argv[0]);
    return 2;
  }
  std::vector<std::vector<uint8_t>> msgs;
  std::vector<BelowBReq> reqs;
  char hex[4096];
  uint64_t a, b, t, c;
  while (scanf("%4095s %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, hex, &a, &b, &t, &c) == 5) {
    msgs.push_back(strcmp(hex, "-") == 0 ? std::vector<uint8_t>() : unhex(hex));
    reqs.push_back({nullptr, 0, a, b, t, c});
  }
  for (size_t i = 0; i < reqs.size(); ++i) {
    reqs[i].msg = msgs[i].data();
    reqs[i].len = msgs[i].size();
  }
  return replay_below(reqs, ndev, max_slice, corrupt);
}

int main(int argc, char** argv) {
  if (argc > 1 && strcmp(argv[1], "below") == 0) return main_below(argc, argv);
  const bool wide = argc > 1 && strcmp(argv[1], "wide") == 0;
  const int a0 = wide ? 2 : 1;
  const int ndev = argc > a0 ? atoi(argv[a0]) : 1;
  const uint64_t arg2 = argc > a0 + 1 ? strtoull(argv[a0 + 1], nullptr, 10) : 0;
  const uint64_t floor = argc > a0 + 2 ? strtoull(argv[a0 + 2], nullptr, 10) : 0;
  if (ndev < 1) {
    fprintf(stderr, "usage: %s [ndev [max_tiles]] < requests\n       %s wide [ndev [max_segs [F]]] < requests\n", argv[0],
            argv[0]);
    return 2;
  }
  std::vector<std::vector<uint8_t>> msgs;
  std::vector<uint64_t> lo, hi;
  char hex[4096];
  uint64_t a, b;
  while (scanf("%4095s %" SCNu64 " %" SCNu64, hex, &a, &b) == 3) {
    msgs.push_back(strcmp(hex, "-") == 0 ? std::vector<uint8_t>() : unhex(hex));
    lo.push_back(a);
    hi.push_back(b);
  }
  const size_t n = msgs.size();
  std::vector<BatchReq> reqs(n);
  for (size_t i = 0; i < n; ++i) reqs[i] = {msgs[i].data(), msgs[i].size(), lo[i], hi[i]};
  std::vector<Key> out;
  if (wide) {
    const uint32_t max_segs = arg2 > 0 && arg2 < kMaxSegs ? (uint32_t)arg2 : kMaxSegs;
    if (int rc = replay_wide(reqs, ndev, max_segs, floor, out)) return rc;
  } else {
    BatchInfo info;
    if (int rc = replay_batch(reqs, ndev, argc > 2 ? arg2 : kBatchMaxTiles, out, info)) return rc;
    fprintf(stderr, "launches=%" PRIu64 " tiles=%" PRIu64 " segs=%" PRIu64 "\n", info.launches, info.tiles, info.segs);
  }
  for (size_t i = 0; i < n; ++i) printf("%" PRIu64 " %" PRIu64 "\n", out[i].h, out[i].n);
  return 0;
}
