// below_plan.hpp -- host side of p1hip_scan_below that needs no device: the
// slice rule, the route choice, the candidate filter over k_scan's partials,
// the refine tables of the mark kernel and the decoder of its marks.
// p1hip.hip (p1hip_scan_below) and tools/p1emu (`below=`) share it, so the
// host replay lays a call out with the library's own code.
//
// The call answers "every nonce n of [lower, upper] with Hash(msg, n) <=
// target, in increasing n, the first `cap` of them" slice by slice:
//   sparse slice  k_scan runs as in p1hip_scan; a tile can hold a hit only if
//                 its 16-byte partial (the tile's minimum) is at or below the
//                 target; every run element of such a candidate tile
//                 (tile_map.hpp) becomes a generic piece and k_below_mark
//                 answers one bit per nonce of the pieces
//   dense slice   the slice's decade pieces go straight to k_below_mark
#pragma once
#include <algorithm>
#include <string>
#include <vector>

#include "batch_plan.hpp"
#include "below_abi.hpp"
#include "tile_map.hpp"

namespace p1 {

enum BelowPath { kBelowAuto = 0, kBelowSparse = 1, kBelowDense = 2 };

// Pieces per refine table: bounds the table's memory (a BatchSeg is 200
// bytes) whatever the pieces' sizes; the tiles are bounded by kBatchMaxTiles.
constexpr size_t kBelowMaxPieces = 1u << 16;

// The smallest power of two P in [kBelowMinSlice, max_len] with
// P >= 2 * want * 2^64 / (target + 1), twice the nonces expected to hold
// `want` hits (max_len if there is none; max_len is a power of two of at most
// 2^34).  P * (target + 1) < 2^99 and, for want < 2^34, want * 2^65 < 2^99:
// no 128-bit overflow for any target and any want.
inline uint64_t below_slice_pow2(uint64_t target, uint64_t want, uint64_t max_len) {
  if (max_len <= kBelowMinSlice) return kBelowMinSlice;
  if (want >= (1ull << 34)) return max_len;
  const unsigned __int128 t1 = (unsigned __int128)target + 1;
  const unsigned __int128 need = (unsigned __int128)want << 65;
  uint64_t P = kBelowMinSlice;
  while (P < max_len && (unsigned __int128)P * t1 < need) P <<= 1;
  return P;
}

struct BelowSlice {
  uint64_t lo, hi;  // inclusive, lo <= hi
  bool dense;
};

// The slice that starts at `lo` (lo <= upper) when `want` >= 1 hits are still
// missing.  `path`: kBelowAuto, or a forced route; `max_slice`: 0, or a cap on
// the slice length below the route's own (both are test knobs).
inline BelowSlice below_next_slice(uint64_t lo, uint64_t upper, uint64_t target, uint64_t want, int path,
                                   uint64_t max_slice) {
  bool dense = path == kBelowDense || (path == kBelowAuto && target >= kBelowDenseTarget);
  uint64_t len = below_slice_pow2(target, want, dense ? kBelowMaxSliceDense : kBelowMaxSliceSparse);
  if (max_slice && len > max_slice) len = max_slice;
  const uint64_t left = upper - lo;  // nonces left - 1
  if (len - 1 > left) len = left + 1;  // left + 1 <= len here: no overflow
  // k_scan_small's territory: nothing for a filter to reject at a profit
  if (path == kBelowAuto && len <= kBelowMinSlice) dense = true;
  return {lo, lo + (len - 1), dense};
}

// A tile can hold a hit only if its partial, the tile's minimum, is at or
// below the target.  A tile without a valid thread wrote the identity key,
// which is not a hash: nruns decides, so that target UINT64_MAX stays exact.
inline bool below_candidate(const TileInfo& T, const Key& part, uint64_t target) {
  return T.nruns > 0 && part.h <= target;
}

// One contiguous run of nonces the mark kernel looks at, one nonce per
// thread.  `cand`: the candidate tile it refines (sparse), 0 (dense).
struct BelowPiece {
  uint64_t lo, hi;  // inclusive
  uint32_t cand;
};

// Every run element of a candidate tile.
inline void below_tile_pieces(const TileInfo& T, uint32_t cand, std::vector<BelowPiece>& out) {
  for (uint32_t r = 0; r < T.nruns; ++r) {
    const TileRun& R = T.runs[r];
    for (uint32_t j = 0; j < R.count; ++j) {
      const uint64_t first = R.first + (uint64_t)j * R.stride;
      out.push_back({first, first + (R.run_len - 1), cand});
    }
  }
}

// A dense slice's pieces: the slice cut at the decade boundaries, in order.
inline void below_dense_pieces(uint64_t lo, uint64_t hi, std::vector<BelowPiece>& out) {
  for (int d = 1; d <= 20; ++d) {
    const uint64_t dlo = (d == 1) ? 0u : pow10u(d - 1);
    const uint64_t dhi = (d == 20) ? ~0ull : pow10u(d) - 1u;
    const uint64_t s = lo > dlo ? lo : dlo;
    const uint64_t e = hi < dhi ? hi : dhi;
    if (s <= e) out.push_back({s, e, 0});
  }
}

// One launch of k_below_mark: pieces [first, first + count) of the slice.
struct BelowTable {
  size_t first = 0, count = 0;
  uint32_t tiles = 0;
  BatchTable T;  // segs[i].req is the piece, relative to `first`
};

// The table that starts at piece `first` (< pieces.size()): it takes pieces
// while their tiles fit kBatchMaxTiles and their number kBelowMaxPieces; a
// single piece is never split.  Built by batch_build_table as a launch pair's
// is, every piece a request of the same message.  "" or an error.
inline std::string below_build_table(const uint8_t* msg, size_t len, const std::vector<BelowPiece>& pieces,
                                     size_t first, BelowTable& B) {
  B.first = first;
  B.count = 0;
  B.tiles = 0;
  std::vector<BatchReq> reqs;
  BatchLaunch L;
  L.device = 0;
  L.launch = 0;
  for (size_t i = first; i < pieces.size() && B.count < kBelowMaxPieces; ++i) {
    const uint64_t t = batch_req_tiles(pieces[i].lo, pieces[i].hi);
    if (t > 0xffffffffull) return "internal: a refine piece of more than 2^32 tiles";
    if (B.count && (uint64_t)B.tiles + t > kBatchMaxTiles) break;
    reqs.push_back({msg, len, pieces[i].lo, pieces[i].hi});
    L.reqs.push_back(B.count);
    B.tiles += (uint32_t)t;
    B.count++;
  }
  L.tiles = B.tiles;
  return batch_build_table(reqs.data(), L, B.T);
}

struct BelowHit {
  Key key;        // (hash, nonce), the hash recomputed on the host
  uint32_t cand;  // the piece's candidate tile
};

// Decode the marks of one launch, kBelowWordsPerTile words per tile, in table
// order (for a dense slice that is nonce order), appending at most `limit`
// hits.  Every marked thread must be a nonce of its piece and its hash,
// recomputed here with the kernel's own per-thread function, at or below the
// target: anything else is an error ("" otherwise).
inline std::string below_decode(const BelowTable& B, const std::vector<BelowPiece>& pieces, const uint64_t* marks,
                                uint64_t target, size_t limit, std::vector<BelowHit>& hits) {
  const std::vector<BatchSeg>& segs = B.T.segs;
  size_t added = 0;
  for (size_t si = 0; si < segs.size(); ++si) {
    const BatchSeg& S = segs[si];
    const uint32_t b1 = si + 1 < segs.size() ? segs[si + 1].block0 : B.tiles;
    const uint32_t cand = pieces[B.first + S.req].cand;
    for (uint32_t b = S.block0; b < b1; ++b)
      for (uint32_t w = 0; w < kBelowWordsPerTile; ++w) {
        uint64_t word = marks[(size_t)b * kBelowWordsPerTile + w];
        while (word) {
          const uint32_t lane = (uint32_t)__builtin_ctzll(word);
          word &= word - 1;
          const uint64_t gid = (uint64_t)(b - S.block0) * kBlock + w * 64u + lane;
          if (gid >= S.ga.count) return "mark check: a thread past its piece's last nonce is marked";
          const Key k = generic_thread(S.ga, gid);
          if (k.h > target) return "mark check: nonce " + std::to_string(k.n) + " is marked, its hash is above the target";
          if (added == limit) return std::string();
          hits.push_back({k, cand});
          ++added;
        }
      }
  }
  return std::string();
}

// Sparse slice, after all its tables are decoded: the hits of candidate tile c
// must have exactly the tile's partial as their lexicographic minimum (the
// partial is the tile's minimum and at or below the target, so it is a hit).
inline std::string below_check_candidates(const std::vector<Key>& cand_part, const std::vector<BelowHit>& hits) {
  std::vector<Key> best(cand_part.size(), Key{~0ull, ~0ull});
  std::vector<char> any(cand_part.size(), 0);
  for (const BelowHit& h : hits) {
    if (!any[h.cand] || key_lt(h.key, best[h.cand])) best[h.cand] = h.key;
    any[h.cand] = 1;
  }
  for (size_t c = 0; c < cand_part.size(); ++c)
    if (!any[c] || best[c].h != cand_part[c].h || best[c].n != cand_part[c].n)
      return "tile check: candidate tile " + std::to_string(c) + " has partial (" + std::to_string(cand_part[c].h) +
             ", " + std::to_string(cand_part[c].n) + "), its refinement " +
             (any[c] ? "(" + std::to_string(best[c].h) + ", " + std::to_string(best[c].n) + ")" : std::string("nothing"));
  return std::string();
}

// A slice's hits in increasing nonce (the pieces of a sparse slice come in
// pack order, a MODE 5 tile's in strided runs).
inline void below_sort_hits(std::vector<BelowHit>& hits) {
  std::sort(hits.begin(), hits.end(), [](const BelowHit& a, const BelowHit& b) { return a.key.n < b.key.n; });
}

}  // namespace p1
