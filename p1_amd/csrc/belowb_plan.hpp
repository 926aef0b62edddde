// belowb_plan.hpp -- host side of p1hip_scan_below_batch that needs no device:
// the route of a request, the layout of one round over devices and launch
// pairs (with the slot cap), the tables of a launch pair, the replay of
// k_belowb_collect and the decoder of what it returns.  p1hip.hip
// (p1hip_scan_below_batch, p1hip_below_batch_layout) and tools/batch_emu
// (`below`) share it, so the host replay lays a call out with the library's
// own code.
//
// A call answers many (message, range, target, cap) searches.  The coalesced
// ones advance in rounds: a round takes the next slice (below_plan.hpp
// below_next_slice) of every unfinished request, lays the slices' tiles back
// to back in launch pairs, and each launch pair marks them (k_belowb_mark) and
// turns every request's marks into at most `slots` thread indices
// (k_belowb_collect).
#pragma once
#include <string>
#include <vector>

#include "below_plan.hpp"
#include "belowb_abi.hpp"

namespace p1 {

struct BelowBReq {
  const uint8_t* msg;
  size_t len;
  uint64_t lower, upper, target;  // inclusive range
  uint64_t cap;
};

enum BelowBRoute { kBelowBEmpty = 0, kBelowBCoalesced = 1, kBelowBIndividual = 2 };

// The route of a request, fixed from its first slice: coalesced when that
// slice is dense and has at most kBelowBatchMaxNonces nonces.  `path` and
// `max_slice` are below_next_slice's test knobs.
inline int belowb_route(const BelowBReq& q, int path, uint64_t max_slice) {
  if (q.lower > q.upper || q.cap == 0) return kBelowBEmpty;
  const BelowSlice S0 = below_next_slice(q.lower, q.upper, q.target, q.cap, path, max_slice);
  return S0.dense && S0.hi - S0.lo < kBelowBatchMaxNonces ? kBelowBCoalesced : kBelowBIndividual;
}

// One coalesced request's part of a round: its slice and what it may return.
struct BelowBItem {
  size_t req;       // index into the call's array
  uint64_t lo, hi;  // the slice, inclusive
  uint32_t tiles;
  uint32_t slots;   // min(hits still wanted, nonces of the slice)
};

// Where a coalesced request stands between rounds.
struct BelowBState {
  uint64_t lo;     // first nonce not yet examined
  uint64_t found;  // hits so far
  bool done;
};

// The next round's items: the next slice of every unfinished coalesced
// request, in request order.  Invariant: a later slice of a coalesced request
// is never longer than its first, because `want` only falls and the slice
// length is monotone in it (below_slice_pow2), and it stays dense, because
// density comes from the target or from a length that only falls; so the route
// cannot change mid-request.  Checked here: "" or an internal error.
inline std::string belowb_round_items(const BelowBReq* reqs, const std::vector<size_t>& coalesced,
                                      const std::vector<BelowBState>& st, int path, uint64_t max_slice,
                                      std::vector<BelowBItem>& items) {
  items.clear();
  for (size_t j = 0; j < coalesced.size(); ++j) {
    if (st[j].done) continue;
    const BelowBReq& q = reqs[coalesced[j]];
    const uint64_t want = q.cap - st[j].found;
    const BelowSlice S = below_next_slice(st[j].lo, q.upper, q.target, want, path, max_slice);
    const uint64_t len1 = S.hi - S.lo;  // nonces - 1
    if (!S.dense || len1 >= kBelowBatchMaxNonces)
      return "internal: request " + std::to_string(coalesced[j]) + " left the coalesced route mid-request";
    items.push_back({j, S.lo, S.hi, (uint32_t)batch_req_tiles(S.lo, S.hi), (uint32_t)(want <= len1 ? want : len1 + 1)});
  }
  return std::string();
}

// One launch pair of a round: items (indices into the round's) on one device.
struct BelowBLaunch {
  int device;  // index into the open devices
  int launch;  // launch pair of that device within the round, from 0
  std::vector<size_t> items;
  uint32_t tiles = 0;
  uint64_t slots = 0;
};

// Lay a round's items out over `ndev` devices by batch_layout's rule: cut, in
// order, into `ndev` contiguous groups of near-equal tile count (an item goes
// to the device in whose share of the tiles its middle falls, wholly), a
// device's group cut into launch pairs that close when the next item's tiles
// would pass `max_tiles` or its slots `max_slots` (a single item fits both: it
// has at most kBelowBatchMaxNonces nonces).
inline std::vector<BelowBLaunch> belowb_layout(const std::vector<BelowBItem>& items, int ndev,
                                               uint64_t max_tiles = kBatchMaxTiles,
                                               uint64_t max_slots = kBelowBatchMaxSlots) {
  std::vector<BelowBLaunch> launches;
  uint64_t total = 0, before = 0;
  for (const BelowBItem& it : items) total += it.tiles;
  for (size_t i = 0; i < items.size(); ++i) {
    const uint64_t t = items[i].tiles, s = items[i].slots;
    uint64_t dev = (uint64_t)((unsigned __int128)(2 * before + t) * (uint64_t)ndev / (2 * total));
    if (dev >= (uint64_t)ndev) dev = (uint64_t)ndev - 1;
    before += t;
    if (launches.empty() || launches.back().device != (int)dev) {
      BelowBLaunch L;
      L.device = (int)dev;
      L.launch = 0;
      launches.push_back(L);
    } else if ((uint64_t)launches.back().tiles + t > max_tiles || launches.back().slots + s > max_slots) {
      BelowBLaunch L;
      L.device = (int)dev;
      L.launch = launches.back().launch + 1;
      launches.push_back(L);
    }
    BelowBLaunch& L = launches.back();
    L.items.push_back(i);
    L.tiles += (uint32_t)t;
    L.slots += s;
  }
  return launches;
}

// The tables of one launch pair.  T.segs[..].req and every per-request table
// are indexed by the item's place in the launch.
struct BelowBTable {
  BatchTable T;                     // k_belowb_mark's segments; req_tile0 is k_belowb_collect's
  std::vector<uint64_t> targets;    // per request
  std::vector<uint32_t> req_hit0;   // request r owns slots [req_hit0[r], req_hit0[r + 1])
};

// Built by batch_build_table as a p1hip_scan_batch launch pair's are, every
// slice a request.  "" or an error.
inline std::string belowb_build_table(const BelowBReq* reqs, const std::vector<size_t>& coalesced,
                                      const std::vector<BelowBItem>& items, const BelowBLaunch& L, BelowBTable& B) {
  std::vector<BatchReq> q;
  BatchLaunch bl;
  bl.device = L.device;
  bl.launch = L.launch;
  bl.tiles = L.tiles;
  B.targets.clear();
  B.req_hit0.clear();
  uint32_t slot = 0;
  for (size_t r = 0; r < L.items.size(); ++r) {
    const BelowBItem& it = items[L.items[r]];
    const BelowBReq& src = reqs[coalesced[it.req]];
    q.push_back({src.msg, src.len, it.lo, it.hi});
    bl.reqs.push_back(r);
    B.targets.push_back(src.target);
    B.req_hit0.push_back(slot);
    slot += it.slots;
  }
  B.req_hit0.push_back(slot);
  if (slot != L.slots) return "internal: below batch table has " + std::to_string(slot) + " slots, layout " + std::to_string(L.slots);
  return batch_build_table(q.data(), bl, B.T);
}

// Host replay of k_belowb_collect for request r of a launch: the same chunks
// of kBlock words, the same exclusive prefix per word, the same expansion
// function, the same early end.
inline void belowb_collect_replay(const uint64_t* marks, const uint32_t* req_tile0, const uint32_t* req_hit0, uint32_t r,
                                  uint32_t* idx, uint32_t* count) {
  const uint32_t w0 = req_tile0[r] * kBelowWordsPerTile, w1 = req_tile0[r + 1] * kBelowWordsPerTile;
  const uint32_t s0 = req_hit0[r], slots = req_hit0[r + 1] - s0;
  uint32_t base = 0;
  for (uint32_t c0 = w0; c0 < w1 && base < slots; c0 += kBlock) {
    uint32_t excl = base;
    for (uint32_t t = 0; t < (uint32_t)kBlock && c0 + t < w1; ++t) {
      const uint64_t word = marks[c0 + t];
      if (word != 0 && excl < slots) belowb_expand_word(word, c0 + t, slots - excl, idx + s0 + excl);
      excl += (uint32_t)__builtin_popcountll(word);
    }
    base = excl;
  }
  count[r] = base < slots ? base : slots;
}

// Decode what one launch pair returned: count[r] indices of request r from
// idx[req_hit0[r]] on, appended to hits[r] as (hash, nonce).  Checked, an
// error otherwise: count[r] is at most the request's slots; every index is a
// thread of a tile of the request and of its piece (gid < count); its hash,
// recomputed with the kernel's own per-thread function, is at or below the
// request's target; the request's nonces are strictly increasing.
inline std::string belowb_decode(const BelowBTable& B, const uint32_t* idx, const uint32_t* count,
                                 std::vector<std::vector<Key>>& hits) {
  const std::vector<BatchSeg>& segs = B.T.segs;
  const size_t nreq = B.targets.size();
  hits.assign(nreq, std::vector<Key>());
  for (size_t r = 0; r < nreq; ++r) {
    const uint32_t slots = B.req_hit0[r + 1] - B.req_hit0[r];
    const uint32_t t0 = B.T.req_tile0[r], t1 = B.T.req_tile0[r + 1];
    if (count[r] > slots)
      return "collect check: request " + std::to_string(r) + " reports " + std::to_string(count[r]) + " hits in " +
             std::to_string(slots) + " slots";
    for (uint32_t j = 0; j < count[r]; ++j) {
      const uint32_t t = idx[B.req_hit0[r] + j];
      const uint32_t b = t / (uint32_t)kBlock;
      if (b < t0 || b >= t1) return "collect check: request " + std::to_string(r) + " has an index outside its tiles";
      const BatchSeg& S = segs[batch_find_seg(segs.data(), (uint32_t)segs.size(), b)];
      const uint64_t gid = (uint64_t)(b - S.block0) * kBlock + t % (uint32_t)kBlock;
      if (S.req != r || gid >= S.ga.count) return "collect check: a thread past its piece's last nonce is returned";
      const Key k = generic_thread(S.ga, gid);
      if (k.h > B.targets[r])
        return "collect check: nonce " + std::to_string(k.n) + " is returned, its hash is above the target";
      if (!hits[r].empty() && k.n <= hits[r].back().n)
        return "collect check: request " + std::to_string(r) + " has nonces out of order";
      hits[r].push_back(k);
    }
  }
  return std::string();
}

}  // namespace p1
