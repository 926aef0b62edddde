// batch_emu -- TEST TOOL: replays a p1hip_scan_batch, p1hip_scan_batch_wide,
// p1hip_scan_below_batch or p1hip_scan_below_batch_wide call on the host.
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
//
// usage: batch_emu beloww <ndev> [maxslice=N] [path=P] [corrupt=K|mK] [maxsegs=N] [floor=F] [maxslots=N] [maxtiles=N]
//   replays p1hip_scan_below_batch_wide with the library's own beloww_plan.hpp:
//   routes, rounds, the dense items through the launch-pair replay above, the
//   sparse items group by group: wide_layout's partial array filled by
//   k_batch_scan and k_scan tile by tile as in `wide`, k_beloww_filter
//   (beloww_filter_replay: the shared per-thread function), the host filter
//   where a request's slots overflow, the candidates' pieces, k_belowb_mark
//   over them (below_thread per simulated thread against the piece's own
//   target), the library's decoder and its tile check.  maxslice=N and path=P
//   are P1HIP_BELOW_MAX_SLICE and P1HIP_BELOW_PATH, maxsegs=N and floor=F
//   P1HIP_WIDE_MAX_SEGS and P1HIP_WIDE_MIN_FAST_THREADS, maxslots=N
//   P1HIP_BELOW_WIDE_MAX_SLOTS; maxtiles=N is the tile limit of a device's
//   partial array (the library's is 2^24), so that slices are deferred to a
//   further group.  corrupt=K adds 1 to the K-th candidate slot of the first
//   filter launch, corrupt=mK flips bit K of the first mark launch's marks (the
//   kept checks must refuse either: exit status 1).
//   stdin, stdout: as for `below`
//   stderr: "rounds=<n> groups=<n> launches=<k_scan launches> tiles=<n> slots=<n> candidates=<n> overflows=<n>
//            marks=<mark launches> pairs=<dense launch pairs> dense_rounds=<n> scan_nonces=<n> filtered=<n>
//            coalesced=<n> empty=<n>"
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
#include "../p1_amd/csrc/beloww_plan.hpp"
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

// One launch pair of p1hip_scan_below_batch: k_belowb_mark, k_belowb_collect and
// the library's decoder.  corrupt >= 0 adds 1 to that index before it is decoded.
static int replay_below_pair(const BelowBLaunch& L, const BelowBTable& B, long corrupt, std::vector<std::vector<Key>>& got) {
  const uint64_t unwritten = 0x756e7772697474ull;  // every word must be overwritten
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
  if (corrupt >= 0 && (uint64_t)corrupt < L.slots) idx[(size_t)corrupt] += 1;
  const std::string err = belowb_decode(B, idx.data(), count.data(), got);
  if (!err.empty()) {
    fprintf(stderr, "decode error: %s\n", err.c_str());
    return 1;
  }
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
      if (int rc = replay_below_pair(L, B, nlaunch == 0 ? corrupt : -1, got)) return rc;
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

// What `batch_emu beloww` takes from its command line.
struct BelowWOpts {
  int ndev = 0, path = kBelowAuto;
  uint64_t max_slice = 0, floor = 0, max_slots = 0, max_tiles = kWideMaxTiles;
  uint32_t max_segs = kMaxSegs;
  long corrupt_cand = -1, corrupt_mark = -1;
};

// The p1hip_scan_below_batch_wide replay.
static int replay_beloww(const std::vector<BelowBReq>& reqs, const BelowWOpts& O) {
  const size_t n = reqs.size();
  std::vector<size_t> live;
  std::vector<BelowWState> st;
  uint64_t empty = 0, coalesced = 0, filtered = 0;
  for (size_t i = 0; i < n; ++i) {
    const int route = beloww_route(reqs[i], O.path, O.max_slice);
    if (route == kBelowWIndividual) {
      fprintf(stderr, "request %zu takes the individual route: not a below wide replay\n", i);
      return 1;
    }
    if (route == kBelowWEmpty) {
      empty++;
      continue;
    }
    (route == kBelowWCoalesced ? coalesced : filtered)++;
    live.push_back(i);
    st.push_back(beloww_state(reqs[i], route, O.path, O.max_slice));
  }
  std::vector<std::vector<Key>> res(n);
  size_t left = live.size();
  auto take = [&](size_t j, uint64_t hi, const Key* got, size_t ngot) -> int {
    const size_t i = live[j];
    for (size_t k = 0; k < ngot; ++k) {
      if (!res[i].empty() && got[k].n <= res[i].back().n) {
        fprintf(stderr, "collect check: request %zu has nonces out of order\n", i);
        return 1;
      }
      res[i].push_back(got[k]);
    }
    st[j].found += ngot;
    if (st[j].found == reqs[i].cap || hi == reqs[i].upper) {
      st[j].done = true;
      --left;
    } else {
      st[j].lo = hi + 1;
    }
    return 0;
  };
  uint64_t rounds = 0, groups = 0, launches = 0, tiles = 0, slots = 0, candidates = 0, overflows = 0, pairs = 0,
           marks_launched = 0, scan_nonces = 0, dense_rounds = 0;
  std::vector<BelowBItem> dense;
  std::vector<BelowWItem> sparse;
  BelowBTable DB;
  std::vector<std::vector<Key>> dgot, got(n);
  const Key unwritten = {0x756e7772697474ull, 0x656eull};  // every tile must be overwritten
  bool first_filter = true, first_mark = true;
  for (; left > 0; ++rounds) {
    std::string err = beloww_round_items(reqs.data(), live, st, O.path, O.max_slice, dense, sparse);
    if (!err.empty()) {
      fprintf(stderr, "round error: %s\n", err.c_str());
      return 1;
    }
    // the sparse slices, group after group
    std::vector<size_t> pending(sparse.size());
    for (size_t s = 0; s < sparse.size(); ++s) pending[s] = s;
    BelowWGroup G;
    while (!pending.empty()) {
      err = beloww_next_group(reqs.data(), live, sparse, pending, O.ndev, O.max_segs, O.floor, true, O.max_tiles, G);
      if (!err.empty()) {
        fprintf(stderr, "group error: %s\n", err.c_str());
        return 1;
      }
      groups++;
      for (size_t dv = 0; dv < G.Y.devs.size(); ++dv) {
        const WideDevice& D = G.Y.devs[dv];
        if (D.reqs.empty()) continue;
        const size_t nreq = D.reqs.size();
        BelowWFilter F;
        err = beloww_filter_tables(reqs.data(), live, sparse, G, dv, O.max_slots, F);
        if (!err.empty()) {
          fprintf(stderr, "filter table error: %s\n", err.c_str());
          return 1;
        }
        // phase A: k_batch_scan and the k_scan launches into the partial array
        std::vector<Key> part(D.total_tiles, unwritten);
        std::vector<uint8_t> written(D.total_tiles, 0);
        if (D.gen_tiles)
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
        std::vector<Segment> tab;
        for (const WideLaunch& W : D.launches) {
          if (W.count > O.max_segs || (uint64_t)W.tile0 + W.tiles > D.total_tiles) {
            fprintf(stderr, "launch of %zu segments / tiles outside the partial array\n", W.count);
            return 1;
          }
          tab.assign(W.count, Segment());
          err = wide_fill_launch(D, W, tab.data());
          if (!err.empty()) {
            fprintf(stderr, "segment error: %s\n", err.c_str());
            return 1;
          }
          for_tiles(W.tiles, [&](uint32_t b) {
            part[W.tile0 + b] = replay_scan_tile(tab.data(), (uint32_t)W.count, b);
            written[W.tile0 + b]++;
          });
        }
        for (uint32_t t = 0; t < D.total_tiles; ++t)
          if (written[t] != 1) {
            fprintf(stderr, "tile %u written %u times\n", t, (unsigned)written[t]);
            return 1;
          }
        launches += D.launches.size();
        tiles += D.total_tiles;
        scan_nonces += D.nonces;
        // k_beloww_filter: grid = requests of the device
        const uint32_t nslot = F.req_slot0[nreq];
        std::vector<uint32_t> cand((size_t)nslot + 1, ~0u), count(nreq, ~0u);
        for (uint32_t r = 0; r < (uint32_t)nreq; ++r) beloww_filter_replay(part.data(), D, F, r, cand.data(), count.data());
        if (cand[nslot] != ~0u) {
          fprintf(stderr, "an index past the device's slots was written\n");
          return 1;
        }
        slots += nslot;
        if (first_filter && O.corrupt_cand >= 0 && (uint64_t)O.corrupt_cand < nslot) cand[(size_t)O.corrupt_cand] += 1;
        first_filter = false;
        // the host: candidates (the host filter where the slots overflowed), pieces
        BelowWRefine X;
        std::vector<uint32_t> idx;
        for (uint32_t r = 0; r < (uint32_t)nreq; ++r) {
          const size_t i = live[sparse[G.members[D.reqs[r]]].req];
          const uint32_t s0 = F.req_slot0[r], room = F.req_slot0[r + 1] - s0;
          if (count[r] <= room) {
            err = beloww_add_candidates(D, F, r, i, cand.data() + s0, count[r], X);
          } else {
            overflows++;
            idx.clear();
            for (uint32_t j = D.req_range0[r]; j < D.req_range0[r + 1]; ++j)
              for (uint32_t t = 0; t < D.ranges[j].ntiles; ++t) {
                uint32_t tile;
                if (beloww_thread(part.data(), D.ranges[j], 0, t, F.targets[r], &tile)) idx.push_back(tile);
              }
            if (idx.size() != count[r]) {
              fprintf(stderr, "filter check: request %zu reports %u candidates, its partials hold %zu\n", i, count[r],
                      idx.size());
              return 1;
            }
            err = beloww_add_candidates(D, F, r, i, idx.data(), (uint32_t)idx.size(), X);
          }
          if (!err.empty()) {
            fprintf(stderr, "candidate error: %s\n", err.c_str());
            return 1;
          }
        }
        for (size_t c = 0; c < X.cand_req.size(); ++c) X.cand_part[c] = part[X.cand_tile[c]];
        candidates += X.cand_req.size();
        err = beloww_check_parts(reqs.data(), X);
        if (!err.empty()) {
          fprintf(stderr, "candidate error: %s\n", err.c_str());
          return 1;
        }
        // phase B: k_belowb_mark over the candidates' pieces, table after table
        std::vector<BelowHit> hits;
        BelowTable B;
        std::vector<uint64_t> targets;
        for (size_t first = 0; first < X.pieces.size(); first += B.count) {
          err = beloww_build_table(reqs.data(), X, first, B, targets);
          if (!err.empty() || B.count == 0) {
            fprintf(stderr, "refine table error: %s\n", err.c_str());
            return 1;
          }
          std::vector<uint64_t> marks((size_t)B.tiles * kBelowWordsPerTile, unwritten.h);
          for_tiles(B.tiles, [&](uint32_t b) {
            const BatchSeg& S = B.T.segs[batch_find_seg(B.T.segs.data(), (uint32_t)B.T.segs.size(), b)];
            for (uint32_t w = 0; w < kBelowWordsPerTile; ++w) {
              uint64_t word = 0;
              for (uint32_t l = 0; l < 64; ++l)
                if (below_thread(S.ga, (uint64_t)(b - S.block0) * kBlock + w * 64u + l, targets[S.req])) word |= 1ull << l;
              marks[(size_t)b * kBelowWordsPerTile + w] = word;
            }
          });
          if (first_mark && O.corrupt_mark >= 0 && (uint64_t)O.corrupt_mark < marks.size() * 64)
            marks[(size_t)O.corrupt_mark / 64] ^= 1ull << (O.corrupt_mark % 64);
          first_mark = false;
          err = beloww_decode(B, X, marks.data(), targets, hits);
          if (!err.empty()) {
            fprintf(stderr, "decode error: %s\n", err.c_str());
            return 1;
          }
          marks_launched++;
        }
        err = beloww_finish(X, hits);
        if (!err.empty()) {
          fprintf(stderr, "decode error: %s\n", err.c_str());
          return 1;
        }
        for (const BelowHit& h : hits) got[X.cand_req[h.cand]].push_back(h.key);
        for (size_t r = 0; r < nreq; ++r) {
          const BelowWItem& it = sparse[G.members[D.reqs[r]]];
          std::vector<Key>& mine = got[live[it.req]];
          if (int rc = take(it.req, it.hi, mine.data(), (size_t)std::min<uint64_t>(it.want, mine.size()))) return rc;
          mine.clear();
        }
      }
    }
    // the dense slices: p1hip_scan_below_batch's launch pairs
    dense_rounds += !dense.empty();
    for (const BelowBLaunch& L : belowb_layout(dense, O.ndev)) {
      err = belowb_build_table(reqs.data(), live, dense, L, DB);
      if (!err.empty()) {
        fprintf(stderr, "table error: %s\n", err.c_str());
        return 1;
      }
      if (int rc = replay_below_pair(L, DB, -1, dgot)) return rc;
      for (size_t r = 0; r < L.items.size(); ++r) {
        const BelowBItem& it = dense[L.items[r]];
        if (int rc = take(it.req, it.hi, dgot[r].data(), dgot[r].size())) return rc;
      }
      pairs++;
    }
  }
  for (size_t i = 0; i < n; ++i) {
    printf("%zu", res[i].size());
    for (const Key& k : res[i]) printf(" %" PRIu64 ":%" PRIu64, k.h, k.n);
    printf("\n");
  }
  fprintf(stderr,
          "rounds=%" PRIu64 " groups=%" PRIu64 " launches=%" PRIu64 " tiles=%" PRIu64 " slots=%" PRIu64
          " candidates=%" PRIu64 " overflows=%" PRIu64 " marks=%" PRIu64 " pairs=%" PRIu64 " dense_rounds=%" PRIu64
          " scan_nonces=%" PRIu64 " filtered=%" PRIu64 " coalesced=%" PRIu64 " empty=%" PRIu64 "\n",
          rounds, groups, launches, tiles, slots, candidates, overflows, marks_launched, pairs, dense_rounds, scan_nonces,
          filtered, coalesced, empty);
  return 0;
}

static int main_beloww(int argc, char** argv) {
  BelowWOpts O;
  O.ndev = argc > 2 ? atoi(argv[2]) : 0;
  bool bad = O.ndev < 1;
  for (int i = 3; i < argc; ++i) {
    if (!strncmp(argv[i], "maxslice=", 9)) O.max_slice = strtoull(argv[i] + 9, nullptr, 10);
    else if (!strncmp(argv[i], "path=", 5)) O.path = atoi(argv[i] + 5);
    else if (!strncmp(argv[i], "corrupt=m", 9)) O.corrupt_mark = atol(argv[i] + 9);
    else if (!strncmp(argv[i], "corrupt=", 8)) O.corrupt_cand = atol(argv[i] + 8);
    else if (!strncmp(argv[i], "maxsegs=", 8)) O.max_segs = (uint32_t)strtoul(argv[i] + 8, nullptr, 10);
    else if (!strncmp(argv[i], "floor=", 6)) O.floor = strtoull(argv[i] + 6, nullptr, 10);
    else if (!strncmp(argv[i], "maxslots=", 9)) O.max_slots = strtoull(argv[i] + 9, nullptr, 10);
    else if (!strncmp(argv[i], "maxtiles=", 9)) O.max_tiles = strtoull(argv[i] + 9, nullptr, 10);
    else bad = true;
  }
  if (O.max_segs == 0 || O.max_segs > kMaxSegs) O.max_segs = kMaxSegs;
  if (bad || O.path < kBelowAuto || O.path > kBelowDense) {
    fprintf(stderr,
            "usage: %s beloww <ndev> [maxslice=N] [path=P] [corrupt=K|mK] [maxsegs=N] [floor=F] [maxslots=N] "
            "[maxtiles=N] < requests\n",
            argv[0]);
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
  return replay_beloww(reqs, O);
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
  if (argc > 1 && strcmp(argv[1], "beloww") == 0) return main_beloww(argc, argv);
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
