// beloww_plan.hpp -- host side of p1hip_scan_below_batch_wide that needs no
// device: the route of a request, the items of a round (dense slices for
// p1hip_scan_below_batch's launch pairs, sparse slices for shared k_scan
// launches), the groups a round's sparse slices run in, the slot rule, the
// tables and the replay of k_beloww_filter, the way from a candidate index back
// to its tile's nonces, and the table and decoder of the refinement.  p1hip.hip
// (p1hip_scan_below_batch_wide, p1hip_below_wide_layout) and tools/batch_emu
// (`beloww`) share it, so the host replay lays a call out with the library's
// own code.
//
// A sparse slice is answered in two phases.  Phase A: the slices of a group are
// laid out by wide_layout (wide_plan.hpp) as wide requests are, k_scan and
// k_batch_scan leave one partial per tile on the device, and k_beloww_filter
// turns each request's partials into at most `slots` candidate tile indices and
// the number of all its candidates.  Phase B: the host turns every candidate
// into the pieces of its tile (tile_map.hpp, below_plan.hpp), k_belowb_mark
// marks them against each request's own target, and the marks are decoded and
// checked against the candidates' partials.
#pragma once
#include <algorithm>
#include <string>
#include <vector>

#include "belowb_plan.hpp"
#include "beloww_abi.hpp"
#include "wide_plan.hpp"

namespace p1 {

enum BelowWRoute { kBelowWEmpty = 0, kBelowWCoalesced = 1, kBelowWIndividual = 2, kBelowWFiltered = 3 };

// The route of a request, fixed from its first slice: coalesced exactly as
// belowb_route has it (dense, at most kBelowBatchMaxNonces nonces); filtered
// when that slice is sparse and has at most kWideMaxNonces nonces.  `path` and
// `max_slice` are below_next_slice's test knobs.
inline int beloww_route(const BelowBReq& q, int path, uint64_t max_slice) {
  if (q.lower > q.upper || q.cap == 0) return kBelowWEmpty;
  const BelowSlice S0 = below_next_slice(q.lower, q.upper, q.target, q.cap, path, max_slice);
  const uint64_t len1 = S0.hi - S0.lo;  // nonces - 1
  if (S0.dense) return len1 < kBelowBatchMaxNonces ? kBelowWCoalesced : kBelowWIndividual;
  return len1 < kWideMaxNonces ? kBelowWFiltered : kBelowWIndividual;
}

// Candidate slots of a sparse slice of `len` nonces in `tiles` tiles:
// min(tiles, 16 + 4 * ceil(len * (target + 1) / 2^64)).  Derived, not measured:
// len * (target + 1) / 2^64 is the expected number of hits of the slice, and a
// candidate tile holds at least one hit, so it bounds the expected candidates;
// under the auto path it is at most 2^24 * 2^46 / 2^64 = 64, and a Poisson
// count above 16 + 4 * mean is negligible for every mean up to 64.  len <=
// 2^24 and target + 1 <= 2^64: the product is below 2^88.  `max_slots`
// (a test knob; 0: none) caps the result, so that tests reach the overflow
// path, which the rule itself all but rules out.
inline uint32_t beloww_slots(uint64_t len, uint64_t target, uint32_t tiles, uint64_t max_slots = 0) {
  const unsigned __int128 prod = (unsigned __int128)len * ((unsigned __int128)target + 1);
  const unsigned __int128 mean = (prod + (((unsigned __int128)1 << 64) - 1)) >> 64;
  unsigned __int128 s = 16 + 4 * mean;
  if (s > tiles) s = tiles;
  if (max_slots && s > max_slots) s = max_slots;
  return (uint32_t)s;
}

// Where a coalesced or filtered request stands between rounds.
struct BelowWState {
  uint64_t lo;          // first nonce not yet examined
  uint64_t found;       // hits so far
  bool done;
  int route;            // kBelowWCoalesced or kBelowWFiltered
  uint64_t first_len1;  // nonces - 1 of its first slice
};

inline BelowWState beloww_state(const BelowBReq& q, int route, int path, uint64_t max_slice) {
  const BelowSlice S0 = below_next_slice(q.lower, q.upper, q.target, q.cap, path, max_slice);
  return {q.lower, 0, false, route, S0.hi - S0.lo};
}

// One filtered request's sparse slice of a round.
struct BelowWItem {
  size_t req;       // index into the call's live list
  uint64_t lo, hi;  // the slice, inclusive
  uint64_t want;    // hits still wanted
};

// The next round's items: the next slice of every unfinished request of the
// live list (the coalesced and the filtered ones, in request order); the dense
// slices as belowb_round_items gives them (BelowBItem::req indexes `live`),
// the sparse ones for the shared k_scan launches.
// Route invariant: a later slice is never longer than the first, because
// `want` only falls and the slice length is monotone in it (below_slice_pow2).
// A filtered request's later slice is either sparse, and then of at most
// kWideMaxNonces nonces as its first was, or it has fallen to at most
// kBelowMinSlice nonces and become dense, and then it goes through the dense
// launch pair of the same round.  A coalesced request never turns sparse:
// density comes from the target or from a length that only falls.  Checked
// here every round: "" or an internal error.
inline std::string beloww_round_items(const BelowBReq* reqs, const std::vector<size_t>& live,
                                      const std::vector<BelowWState>& st, int path, uint64_t max_slice,
                                      std::vector<BelowBItem>& dense, std::vector<BelowWItem>& sparse) {
  dense.clear();
  sparse.clear();
  for (size_t j = 0; j < live.size(); ++j) {
    if (st[j].done) continue;
    const BelowBReq& q = reqs[live[j]];
    const uint64_t want = q.cap - st[j].found;
    const BelowSlice S = below_next_slice(st[j].lo, q.upper, q.target, want, path, max_slice);
    const uint64_t len1 = S.hi - S.lo;  // nonces - 1
    const std::string who = "internal: request " + std::to_string(live[j]);
    if (len1 > st[j].first_len1) return who + " has a slice longer than its first";
    if (st[j].route == kBelowWCoalesced) {
      if (!S.dense || len1 >= kBelowBatchMaxNonces) return who + " left the coalesced route mid-request";
    } else if (S.dense ? len1 >= kBelowMinSlice : len1 >= kWideMaxNonces) {
      return who + " left the filtered route mid-request";
    }
    if (S.dense)
      dense.push_back({j, S.lo, S.hi, (uint32_t)batch_req_tiles(S.lo, S.hi), (uint32_t)(want <= len1 ? want : len1 + 1)});
    else
      sparse.push_back({j, S.lo, S.hi, want});
  }
  return std::string();
}

// One group of a round's sparse slices: what one wide_layout call placed.
struct BelowWGroup {
  std::vector<size_t> members;  // Y's request i is the round's sparse item members[i]
  WideLayout Y;                 // table-free plans, small_max = 0
};

// Lay the sparse items `pending` (indices into `sparse`) out over `ndev`
// devices; the items wide_layout turns away for lack of room in a device's
// partial array (`max_tiles`) are left in `pending` for a further group of the
// same round, the others leave it.  A single item always fits alone under
// kWideMaxTiles (it has at most kWideMaxNonces nonces); a group that places
// nothing is an error.  `max_segs`, `floor`: wide_layout's.
inline std::string beloww_next_group(const BelowBReq* reqs, const std::vector<size_t>& live,
                                     const std::vector<BelowWItem>& sparse, std::vector<size_t>& pending, int ndev,
                                     uint32_t max_segs, uint64_t floor, bool split, uint64_t max_tiles, BelowWGroup& G) {
  std::vector<BatchReq> q;
  for (size_t s : pending) {
    const BelowBReq& src = reqs[live[sparse[s].req]];
    q.push_back({src.msg, src.len, sparse[s].lo, sparse[s].hi});
  }
  G.members = pending;
  const std::string err = wide_layout(q.data(), q.size(), ndev, 0, kWideMaxNonces, max_segs, floor, split, G.Y, max_tiles);
  if (!err.empty()) return err;
  std::vector<size_t> later;
  for (size_t i = 0; i < pending.size(); ++i) {
    if (G.Y.route[i] == kWideRouteIndividual) later.push_back(pending[i]);
    else if (G.Y.route[i] != kWideRouteWide) return "internal: a sparse slice is not laid out as a wide request";
  }
  if (later.size() == pending.size()) return "internal: a sparse slice does not fit a device's partial array";
  pending.swap(later);
  return std::string();
}

// k_beloww_filter's tables of one device of a group, next to the device's
// range table (WideDevice::ranges, req_range0), and the way back from a range
// to the piece that wrote it.
struct BelowWFilter {
  std::vector<uint64_t> targets;     // per request of the device
  std::vector<uint32_t> req_slot0;   // request r owns slots [req_slot0[r], req_slot0[r + 1])
  std::vector<int32_t> range_piece;  // per range: its fast piece in the request's plan; -1: the generic tiles
};

inline std::string beloww_filter_tables(const BelowBReq* reqs, const std::vector<size_t>& live,
                                        const std::vector<BelowWItem>& sparse, const BelowWGroup& G, size_t dv,
                                        uint64_t max_slots, BelowWFilter& F) {
  const WideDevice& D = G.Y.devs[dv];
  F.targets.clear();
  F.req_slot0.clear();
  F.range_piece.assign(D.ranges.size(), -1);
  uint64_t slot = 0;
  for (size_t r = 0; r < D.reqs.size(); ++r) {
    const BelowWItem& it = sparse[G.members[D.reqs[r]]];
    const uint64_t target = reqs[live[it.req]].target;
    F.targets.push_back(target);
    F.req_slot0.push_back((uint32_t)slot);
    slot += beloww_slots(it.hi - it.lo + 1, target, G.Y.tiles[D.reqs[r]], max_slots);
  }
  if (slot > kWideMaxTiles) return "internal: more candidate slots than tiles";
  F.req_slot0.push_back((uint32_t)slot);
  // wide_layout appends a request's fast ranges in the device's packing order
  // and its generic range last
  std::vector<uint32_t> next(D.reqs.size(), 0);
  for (const WideFast& f : D.fast) {
    const uint32_t j = D.req_range0[f.req] + next[f.req]++;
    if (j >= D.req_range0[f.req + 1] || D.range_launch[j] < 0 || D.ranges[j].ntiles != D.plans[f.req].launches[f.piece].blocks)
      return "internal: a fast piece without its range";
    F.range_piece[j] = (int32_t)f.piece;
  }
  return std::string();
}

// Host replay of k_beloww_filter for request r of a device: the same ranges in
// the same order, the same chunks of kBlock tiles, the same per-thread
// function, the total not clamped.
inline void beloww_filter_replay(const Key* part, const WideDevice& D, const BelowWFilter& F, uint32_t r, uint32_t* cand,
                                 uint32_t* count) {
  const uint32_t s0 = F.req_slot0[r], slots = F.req_slot0[r + 1] - s0;
  uint32_t base = 0;
  for (uint32_t j = D.req_range0[r]; j < D.req_range0[r + 1]; ++j) {
    const WideRange R = D.ranges[j];
    for (uint32_t c0 = 0; c0 < R.ntiles; c0 += kBlock)
      for (uint32_t t = 0; t < (uint32_t)kBlock; ++t) {
        uint32_t tile;
        if (!beloww_thread(part, R, c0, t, F.targets[r], &tile)) continue;
        if (base < slots) cand[s0 + base] = tile;
        ++base;
      }
  }
  count[r] = base;
}

// The tile at index `idx` of the device's partial array, which request r of the
// device reports as a candidate: its nonce set into T and its place in the
// request's table order into *pos.  An index outside the request's ranges is an
// error.
inline std::string beloww_tile_info(const WideDevice& D, const BelowWFilter& F, uint32_t r, uint32_t idx, TileInfo& T,
                                    uint64_t* pos) {
  uint64_t before = 0;
  for (uint32_t j = D.req_range0[r]; j < D.req_range0[r + 1]; ++j) {
    const WideRange R = D.ranges[j];
    if (idx < R.tile0 || idx - R.tile0 >= R.ntiles) {
      before += R.ntiles;
      continue;
    }
    uint32_t t = idx - R.tile0;
    *pos = before + t;
    T.launch = (uint32_t)(D.range_launch[j] < 0 ? D.launches.size() : (size_t)D.range_launch[j]);
    T.tile = idx;
    if (F.range_piece[j] >= 0) {
      tile_runs(D.plans[r].launches[(size_t)F.range_piece[j]], t, T);
      return std::string();
    }
    for (const Launch& L : D.plans[r].launches) {
      if (L.fast) continue;
      if (t < L.blocks) {
        tile_runs(L, t, T);
        return std::string();
      }
      t -= L.blocks;
    }
    return "internal: a generic range longer than its pieces";
  }
  return "filter check: request " + std::to_string(D.reqs[r]) + " of the group has a candidate outside its ranges";
}

// Everything one device refines in phase B.
struct BelowWRefine {
  std::vector<BelowPiece> pieces;   // cand: index into the three vectors below
  std::vector<size_t> cand_req;     // the call's request the candidate tile belongs to
  std::vector<uint32_t> cand_tile;  // its index in the device's partial array
  std::vector<Key> cand_part;       // its partial (filled by whoever has the partials)
  void clear() {
    pieces.clear();
    cand_req.clear();
    cand_tile.clear();
    cand_part.clear();
  }
};

// Add the `n` candidate indices idx[0 .. n) of request r of the device (call
// request `req`).  Checked: every index lies in the request's ranges and they
// come in table order, strictly.  A tile without a valid thread is dropped
// (its identity key is not a hash: below_candidate's rule); the others become
// pieces (below_tile_pieces).
inline std::string beloww_add_candidates(const WideDevice& D, const BelowWFilter& F, uint32_t r, size_t req,
                                         const uint32_t* idx, uint32_t n, BelowWRefine& X) {
  uint64_t last = 0;
  TileInfo T;
  for (uint32_t c = 0; c < n; ++c) {
    uint64_t pos = 0;
    const std::string err = beloww_tile_info(D, F, r, idx[c], T, &pos);
    if (!err.empty()) return err;
    if (c && pos <= last) return "filter check: request " + std::to_string(req) + " has candidates out of table order";
    last = pos;
    if (T.nruns == 0) continue;
    below_tile_pieces(T, (uint32_t)X.cand_req.size(), X.pieces);
    X.cand_req.push_back(req);
    X.cand_tile.push_back(idx[c]);
    X.cand_part.push_back(Key{~0ull, ~0ull});
  }
  return std::string();
}

// Once cand_part is filled: every candidate's partial is at or below its
// request's target (the filter's own claim).
inline std::string beloww_check_parts(const BelowBReq* reqs, const BelowWRefine& X) {
  for (size_t c = 0; c < X.cand_req.size(); ++c)
    if (X.cand_part[c].h > reqs[X.cand_req[c]].target)
      return "filter check: tile " + std::to_string(X.cand_tile[c]) + " is a candidate of request " +
             std::to_string(X.cand_req[c]) + ", its partial is above the target";
  return std::string();
}

// The k_belowb_mark table that starts at piece `first` of X, bounded as
// below_build_table bounds it (kBatchMaxTiles tiles, kBelowMaxPieces pieces, a
// single piece never split); every piece is a request of its own message, and
// targets[i] is the target of piece first + i.  "" or an error.
inline std::string beloww_build_table(const BelowBReq* reqs, const BelowWRefine& X, size_t first, BelowTable& B,
                                      std::vector<uint64_t>& targets) {
  B.first = first;
  B.count = 0;
  B.tiles = 0;
  targets.clear();
  std::vector<BatchReq> q;
  BatchLaunch L;
  L.device = 0;
  L.launch = 0;
  for (size_t i = first; i < X.pieces.size() && B.count < kBelowMaxPieces; ++i) {
    const uint64_t t = batch_req_tiles(X.pieces[i].lo, X.pieces[i].hi);
    if (t > 0xffffffffull) return "internal: a refine piece of more than 2^32 tiles";
    if (B.count && (uint64_t)B.tiles + t > kBatchMaxTiles) break;
    const BelowBReq& src = reqs[X.cand_req[X.pieces[i].cand]];
    q.push_back({src.msg, src.len, X.pieces[i].lo, X.pieces[i].hi});
    targets.push_back(src.target);
    L.reqs.push_back(B.count);
    B.tiles += (uint32_t)t;
    B.count++;
  }
  L.tiles = B.tiles;
  return batch_build_table(q.data(), L, B.T);
}

// Decode the marks of one such launch as below_decode does, every piece
// against its own target: every marked thread must be a nonce of its piece and
// its hash, recomputed here with the kernel's own per-thread function, at or
// below that target ("" otherwise).
inline std::string beloww_decode(const BelowTable& B, const BelowWRefine& X, const uint64_t* marks,
                                 const std::vector<uint64_t>& targets, std::vector<BelowHit>& hits) {
  const std::vector<BatchSeg>& segs = B.T.segs;
  for (size_t si = 0; si < segs.size(); ++si) {
    const BatchSeg& S = segs[si];
    const uint32_t b1 = si + 1 < segs.size() ? segs[si + 1].block0 : B.tiles;
    const uint32_t cand = X.pieces[B.first + S.req].cand;
    for (uint32_t b = S.block0; b < b1; ++b)
      for (uint32_t w = 0; w < kBelowWordsPerTile; ++w) {
        uint64_t word = marks[(size_t)b * kBelowWordsPerTile + w];
        while (word) {
          const uint32_t lane = (uint32_t)__builtin_ctzll(word);
          word &= word - 1;
          const uint64_t gid = (uint64_t)(b - S.block0) * kBlock + w * 64u + lane;
          if (gid >= S.ga.count) return "mark check: a thread past its piece's last nonce is marked";
          const Key k = generic_thread(S.ga, gid);
          if (k.h > targets[S.req])
            return "mark check: nonce " + std::to_string(k.n) + " is marked, its hash is above the target";
          hits.push_back({k, cand});
        }
      }
  }
  return std::string();
}

// After every table of the device is decoded: the tile check
// (below_check_candidates: each candidate tile's refinement has exactly the
// tile's partial as its minimum), then the hits request by request, in
// increasing nonce (below_sort_hits within a request).
inline std::string beloww_finish(const BelowWRefine& X, std::vector<BelowHit>& hits) {
  const std::string err = below_check_candidates(X.cand_part, hits);
  if (!err.empty()) return err;
  below_sort_hits(hits);
  std::stable_sort(hits.begin(), hits.end(),
                   [&](const BelowHit& a, const BelowHit& b) { return X.cand_req[a.cand] < X.cand_req[b.cand]; });
  return std::string();
}

}  // namespace p1
