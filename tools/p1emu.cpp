// p1emu -- TEST TOOL: replays the scan plan and the kernels' per-thread code
// (fast_thread / generic_thread from p1_amd/csrc/scan_core.hpp) on the host,
// one simulated GPU thread at a time, and prints the (hash, nonce) result.
//
// It exists so the layout logic (decade split, digit placement, lo-digit
// deltas, PRE/TRAIL blocks) and the launch packing (piece order, launch cuts,
// segment tables, block0) can be parity-tested against the oracle in the
// CPU-only test suite.  It is never part of libp1hip.so and never used to
// produce a product result.
//
// usage: p1emu <msg-hex> <lower> <upper> [generic | minthreads=N] [nosplit] [notable]
//              [packed=MAXBLOCKS[,MAXSEGS] | small] [tiles]
//   minthreads=N sets the planner's occupancy floor (1 keeps k = 3 on small
//   ranges, so every k = 3 variant is replayed); nosplit uses mode 2 for
//   straddling lo digits (p1emu is built with -DP1_NV2_PLAIN); notable keeps
//   layouts whose tail block 1 holds only lo digits off MODE 5
//   prints "<hash> <nonce> <fast_launches> <generic_launches> <variants>"
//   where <variants> lists the fast variants run as FV:MODE:TRAIL,... ("-"
//   when none)
//
//   Without packed= or small the plan's pieces are replayed one at a time.
//   packed=MAXBLOCKS[,MAXSEGS] replays the scan the way the device runs it:
//   the library's own packing (p1_amd/csrc/scan_pack.hpp pack_scan, at most
//   MAXBLOCKS workgroups and MAXSEGS segments per launch; 0 or nothing = the
//   library's limits) and segment tables (fill_segments), then k_scan tile by
//   tile: the kernel's segment walk, the variant chosen from the segment's
//   kind, kBlock threads, one partial per tile, all partials folded.
//   small replays k_scan_small from the library's argument block (fill_small;
//   generic pieces, at most 2^16 nonces).  Both also print
//   "launches=<n> tiles=<n> segs=<n>" on stderr.
//   tiles (with packed= or small) adds the per-tile witness of
//   tests/test_tiles.py: the partial vector starts out poisoned (every byte
//   0xA5, as p1hip_scan_tiles poisons the device's), and after the result
//   line comes one line per entry of it, in order:
//     tile <launch> <tile> <kind> <k> <hash> <nonce> <nruns> {<first> <run_len> <stride> <count>}
//   the replayed partial and the tile's nonce set from p1_amd/csrc/tile_map.hpp
//
// usage: p1emu <msg-hex> <lower> <upper> below=<target> [cap=N] [path=sparse|dense] [maxslice=N]
//              [minthreads=N] [notable] [nosplit]
//   replays a whole p1hip_scan_below call on one device: the library's slices,
//   routes, candidate filter, refine tables and mark decoder
//   (p1_amd/csrc/below_plan.hpp), the packed-plan replay above for a sparse
//   slice's partials, and k_below_mark's per-thread function for the marks.
//   path= and maxslice= stand for P1HIP_BELOW_PATH and P1HIP_BELOW_MAX_SLICE.
//   prints one "hit <hash> <nonce>" line per hit, then
//   "below found=<n> slices=<n> sparse=<n> dense=<n> examined=<n> scan_nonces=<n> mark_nonces=<n>
//    candidate_tiles=<n> mark_launches=<n>"
// usage: p1emu - <lo> <upper> belowslice=<target>,<want>[,<path>[,<maxslice>]]
//   the slice rule alone: prints "slice <lo> <hi> <dense>" for the slice that
//   starts at <lo>
// usage: p1emu <msg-hex> <lower> <upper> belowdecode=<target>,<thread>
//   the decoder alone: the true marks of [lower, upper] as one dense table,
//   with the mark of thread <thread> of the launch inverted; prints
//   "decoded <hits>" or "error <text>"
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../p1_amd/csrc/below_plan.hpp"
#include "../p1_amd/csrc/scan_pack.hpp"
#include "../p1_amd/csrc/tile_map.hpp"
#include "scan_replay.hpp"

using namespace p1;

template <int FV, int MODE, bool TR>
static Key run_fast(const FastArgs& A, uint64_t threads) {
  Key best = {~0ull, ~0ull};
  for (uint64_t t = 0; t < threads; ++t) {
    Key k = fast_thread<FV, MODE, TR>(A, (uint32_t)t);
    if (key_lt(k, best)) best = k;
  }
  return best;
}

static Key dispatch_fast(const Launch& L0) {
  Launch L = L0;
  std::vector<uint32_t> tab;  // MODE 5: the K+W table, here in host memory
  if (L.mode == 5 || L.mode == 7) {
    tab = build_kwtable(L);
    L.fa.kwtab = (uint64_t)(uintptr_t)tab.data();
  }
#define P1_CASE(FV, MODE, TR) \
  if (L.fv == FV && L.mode == MODE && L.trail == TR) return run_fast<FV, MODE, TR>(L.fa, L.threads);
#include "../p1_amd/csrc/fast_variants.inc"
#undef P1_CASE
  fprintf(stderr, "no fast variant fv=%d mode=%d trail=%d\n", L.fv, L.mode, (int)L.trail);
  exit(3);
}

// One tile of k_scan (scan_replay.hpp, shared with tools/batch_emu).
static Key scan_tile(const Segment* segs, uint32_t nseg, uint32_t b) { return replay_scan_tile(segs, nseg, b); }

// what a partial holds before any tile wrote it (`tiles`): p1hip.h P1HIP_TILE_POISON
static const Key kPoison = {0xA5A5A5A5A5A5A5A5ull, 0xA5A5A5A5A5A5A5A5ull};

static void print_tiles(const std::vector<TileInfo>& map, const std::vector<Key>& part) {
  for (size_t i = 0; i < map.size(); ++i) {
    const TileInfo& T = map[i];
    printf("tile %u %u %u %u %" PRIu64 " %" PRIu64 " %u", T.launch, T.tile, T.kind, T.k, part[i].h, part[i].n, T.nruns);
    for (uint32_t r = 0; r < T.nruns; ++r)
      printf(" %" PRIu64 " %u %" PRIu64 " %u", T.runs[r].first, T.runs[r].run_len, T.runs[r].stride, T.runs[r].count);
    printf("\n");
  }
}

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

// ---------------------------------------------------------------------------
// below=: a p1hip_scan_below call on one device
// ---------------------------------------------------------------------------
struct BelowOpts {
  uint64_t target = 0, cap = 1, max_slice = 0, min_threads = kMinFastThreads;
  int path = kBelowAuto;
  bool split = true, tabulate = true;
};

// k_below_mark on the host: kBelowWordsPerTile ballots per tile.
static std::vector<uint64_t> mark_table(const BelowTable& B, uint64_t target) {
  std::vector<uint64_t> marks((size_t)B.tiles * kBelowWordsPerTile, 0);
  const std::vector<BatchSeg>& segs = B.T.segs;
  for (uint32_t b = 0; b < B.tiles; ++b) {
    const BatchSeg& S = segs[batch_find_seg(segs.data(), (uint32_t)segs.size(), b)];
    for (uint32_t t = 0; t < (uint32_t)kBlock; ++t)
      if (below_thread(S.ga, (uint64_t)(b - S.block0) * kBlock + t, target))
        marks[(size_t)b * kBelowWordsPerTile + t / 64] |= 1ull << (t % 64);
  }
  return marks;
}

// A sparse slice's pass 1 as run_range runs it: plan, tables, pack, k_scan
// tile by tile; the tile map and the partials.  "" or an error.
static std::string below_pass1(const std::vector<uint8_t>& msg, uint64_t lo, uint64_t hi, const BelowOpts& o,
                               std::vector<TileInfo>& map, std::vector<Key>& part, uint64_t& nonces) {
  Plan plan;
  std::string err = make_plan(msg.data(), msg.size(), lo, hi, plan, true, o.min_threads, o.split, o.tabulate);
  if (!err.empty()) return "plan error: " + err;
  std::vector<std::vector<uint32_t>> tabs(plan.launches.size());
  std::vector<uint64_t> tabptr(plan.launches.size(), 0);
  for (size_t i = 0; i < plan.launches.size(); ++i) {
    const Launch& L = plan.launches[i];
    if (!L.fast || (L.mode != 5 && L.mode != 7)) continue;
    tabs[i] = build_kwtable(L);
    tabptr[i] = (uint64_t)(uintptr_t)tabs[i].data();
  }
  const ScanPack P = pack_scan(plan, kMaxLaunchBlocks);
  std::vector<Segment> segs(kMaxSegs);
  part.assign(P.total_blocks, kPoison);
  ScanCounters ctr;
  uint32_t part_off = 0;
  for (const ScanBatch& B : P.batches) {
    err = fill_segments(plan, P, B, tabptr.data(), segs.data(), ctr);
    if (!err.empty()) return "segment error: " + err;
    for (uint32_t b = 0; b < B.blocks; ++b) part[part_off + b] = scan_tile(segs.data(), (uint32_t)B.count, b);
    part_off += B.blocks;
  }
  map = tile_map(plan, P);
  nonces = ctr.scan_nonces;
  return map.size() == part.size() ? std::string() : std::string("packing error: map and partials differ in size");
}

static int run_below(const std::vector<uint8_t>& msg, uint64_t lower, uint64_t upper, const BelowOpts& o) {
  std::vector<Key> res;
  uint64_t slices = 0, sparse = 0, dense = 0, examined = 0, scan_nonces = 0, mark_nonces = 0, cands = 0, launches = 0;
  if (lower <= upper && o.cap > 0) {
    std::vector<BelowPiece> pieces;
    std::vector<Key> cand_part;
    std::vector<BelowHit> got;
    BelowTable B;
    for (uint64_t lo = lower;;) {
      const uint64_t want = o.cap - res.size();
      const BelowSlice S = below_next_slice(lo, upper, o.target, want, o.path, o.max_slice);
      pieces.clear();
      cand_part.clear();
      got.clear();
      std::string err;
      if (S.dense) {
        below_dense_pieces(S.lo, S.hi, pieces);
        ++dense;
      } else {
        std::vector<TileInfo> map;
        std::vector<Key> part;
        uint64_t n = 0;
        err = below_pass1(msg, S.lo, S.hi, o, map, part, n);
        if (!err.empty()) {
          fprintf(stderr, "%s\n", err.c_str());
          return 1;
        }
        scan_nonces += n;
        for (size_t t = 0; t < map.size(); ++t)
          if (below_candidate(map[t], part[t], o.target)) {
            below_tile_pieces(map[t], (uint32_t)cand_part.size(), pieces);
            cand_part.push_back(part[t]);
          }
        ++sparse;
        cands += cand_part.size();
      }
      for (size_t first = 0; first < pieces.size() && (!S.dense || got.size() < want); first += B.count) {
        err = below_build_table(msg.data(), msg.size(), pieces, first, B);
        if (err.empty() && (B.count == 0 || B.tiles == 0)) err = "internal: empty refine table";
        if (err.empty()) {
          const std::vector<uint64_t> marks = mark_table(B, o.target);
          ++launches;
          mark_nonces += B.T.nonces;
          err = below_decode(B, pieces, marks.data(), o.target, S.dense ? (size_t)(want - got.size()) : ~(size_t)0, got);
        }
        if (!err.empty()) {
          fprintf(stderr, "%s\n", err.c_str());
          return 1;
        }
      }
      if (!S.dense) {
        err = below_check_candidates(cand_part, got);
        if (!err.empty()) {
          fprintf(stderr, "%s\n", err.c_str());
          return 1;
        }
        below_sort_hits(got);
      }
      for (size_t i = 0; i < got.size() && res.size() < o.cap; ++i) res.push_back(got[i].key);
      ++slices;
      examined += S.hi - S.lo + 1;
      if (res.size() == o.cap || S.hi == upper) break;
      lo = S.hi + 1;
    }
  }
  for (const Key& k : res) printf("hit %" PRIu64 " %" PRIu64 "\n", k.h, k.n);
  printf("below found=%zu slices=%" PRIu64 " sparse=%" PRIu64 " dense=%" PRIu64 " examined=%" PRIu64
         " scan_nonces=%" PRIu64 " mark_nonces=%" PRIu64 " candidate_tiles=%" PRIu64 " mark_launches=%" PRIu64 "\n",
         res.size(), slices, sparse, dense, examined, scan_nonces, mark_nonces, cands, launches);
  return 0;
}

static int run_below_decode(const std::vector<uint8_t>& msg, uint64_t lower, uint64_t upper, uint64_t target,
                            uint64_t thread) {
  std::vector<BelowPiece> pieces;
  below_dense_pieces(lower, upper, pieces);
  BelowTable B;
  std::string err = below_build_table(msg.data(), msg.size(), pieces, 0, B);
  if (!err.empty() || B.count != pieces.size() || thread >= (uint64_t)B.tiles * kBlock) {
    fprintf(stderr, "belowdecode: %s\n", err.empty() ? "range or thread out of one table" : err.c_str());
    return 2;
  }
  std::vector<uint64_t> marks = mark_table(B, target);
  marks[thread / 64] ^= 1ull << (thread % 64);
  std::vector<BelowHit> got;
  err = below_decode(B, pieces, marks.data(), target, ~(size_t)0, got);
  if (!err.empty()) printf("error %s\n", err.c_str());
  else printf("decoded %zu\n", got.size());
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 4) {
    fprintf(stderr,
            "usage: %s <msg-hex|-> <lower> <upper> [generic|minthreads=N] [nosplit] [notable] "
            "[packed=MAXBLOCKS[,MAXSEGS]|small] [tiles]\n"
            "       %s <msg-hex|-> <lower> <upper> below=<target> [cap=N] [path=sparse|dense] [maxslice=N] "
            "[minthreads=N] [notable] [nosplit]\n",
            argv[0], argv[0]);
    return 2;
  }
  std::vector<uint8_t> msg = strcmp(argv[1], "-") == 0 ? std::vector<uint8_t>() : unhex(argv[1]);
  const uint64_t lower = strtoull(argv[2], nullptr, 10);
  const uint64_t upper = strtoull(argv[3], nullptr, 10);
  bool generic_only = argc > 4 && strcmp(argv[4], "generic") == 0;
  uint64_t min_threads = kMinFastThreads;
  bool split = true, tabulate = true, packed = false, small = false, tiles_out = false;
  uint64_t max_blocks = kMaxLaunchBlocks;
  uint32_t max_segs = kMaxSegs;
  for (int i = 4; i < argc; ++i) {
    if (strncmp(argv[i], "minthreads=", 11) == 0) min_threads = strtoull(argv[i] + 11, nullptr, 10);
    if (strcmp(argv[i], "nosplit") == 0) split = false;
    if (strcmp(argv[i], "notable") == 0) tabulate = false;
    if (strcmp(argv[i], "tiles") == 0) tiles_out = true;
    if (strcmp(argv[i], "small") == 0) small = generic_only = true;  // as run_small plans
    if (strncmp(argv[i], "packed=", 7) == 0) {
      packed = true;
      char* end = nullptr;
      const uint64_t mb = strtoull(argv[i] + 7, &end, 10);
      const uint64_t ms = *end == ',' ? strtoull(end + 1, nullptr, 10) : 0;
      if (mb > 0 && mb < kMaxLaunchBlocks) max_blocks = mb;
      if (ms > 0 && ms < kMaxSegs) max_segs = (uint32_t)ms;
    }
  }
  for (int i = 4; i < argc; ++i) {
    if (strncmp(argv[i], "belowslice=", 11) == 0) {
      uint64_t v[4] = {0, 1, kBelowAuto, 0};
      const char* c = argv[i] + 11;
      for (int j = 0; j < 4 && *c; ++j) {
        char* end = nullptr;
        v[j] = strtoull(c, &end, 10);
        c = *end == ',' ? end + 1 : end;
      }
      if (lower > upper || v[1] == 0) return 2;
      const BelowSlice S = below_next_slice(lower, upper, v[0], v[1], (int)v[2], v[3]);
      printf("slice %" PRIu64 " %" PRIu64 " %d\n", S.lo, S.hi, (int)S.dense);
      return 0;
    }
    if (strncmp(argv[i], "belowdecode=", 12) == 0) {
      char* end = nullptr;
      const uint64_t target = strtoull(argv[i] + 12, &end, 10);
      if (*end != ',' || lower > upper) return 2;
      return run_below_decode(msg, lower, upper, target, strtoull(end + 1, nullptr, 10));
    }
  }
  for (int i = 4; i < argc; ++i)
    if (strncmp(argv[i], "below=", 6) == 0) {
      BelowOpts o;
      o.target = strtoull(argv[i] + 6, nullptr, 10);
      o.min_threads = min_threads;
      o.split = split;
      o.tabulate = tabulate;
      for (int j = 4; j < argc; ++j) {
        if (strncmp(argv[j], "cap=", 4) == 0) o.cap = strtoull(argv[j] + 4, nullptr, 10);
        if (strncmp(argv[j], "maxslice=", 9) == 0) o.max_slice = strtoull(argv[j] + 9, nullptr, 10);
        if (strcmp(argv[j], "path=sparse") == 0) o.path = kBelowSparse;
        if (strcmp(argv[j], "path=dense") == 0) o.path = kBelowDense;
      }
      return run_below(msg, lower, upper, o);
    }
  if (tiles_out && !packed && !small) {
    fprintf(stderr, "tiles needs packed= or small\n");
    return 2;
  }
  Key best = {~0ull, ~0ull};
  std::vector<TileInfo> tmap;  // `tiles`: the map and the partial vector it describes
  std::vector<Key> tpart;
  int nf = 0, ng = 0;
  std::string vars;
  size_t launches = 0;
  uint64_t tiles = 0, nsegs = 0;
  if (lower <= upper) {
    Plan plan;
    std::string err = make_plan(msg.data(), msg.size(), lower, upper, plan, !generic_only, min_threads, split, tabulate);
    if (!err.empty()) {
      fprintf(stderr, "plan error: %s\n", err.c_str());
      return 1;
    }
    for (const Launch& L : plan.launches) {
      if (L.fast) {
        ++nf;
        char v[32];
        snprintf(v, sizeof v, "%s%d:%d:%d", vars.empty() ? "" : ",", L.fv, L.mode, (int)L.trail);
        vars += v;
      } else {
        ++ng;
      }
    }
    ScanCounters ctr;
    if (small) {
      // k_scan_small: grid = a.nblocks workgroups, pieces found by the walk
      // over a.block0 (p1emu's copy of the kernel's), the last workgroup's
      // fold of the partials
      SmallArgs a;
      err = fill_small(plan, a, ctr);
      if (!err.empty()) {
        fprintf(stderr, "small error: %s\n", err.c_str());
        return 1;
      }
      std::vector<Key> part(a.nblocks, kPoison);
      for (uint32_t b = 0; b < a.nblocks; ++b) {
        uint32_t si = 0;
        while (si + 1 < a.nseg && a.block0[si + 1] <= b) ++si;
        Key m = {~0ull, ~0ull};
        for (uint32_t t = 0; t < (uint32_t)kBlock; ++t) {
          const Key k = generic_thread(a.ga[si], (uint64_t)(b - a.block0[si]) * kBlock + t);
          if (key_lt(k, m)) m = k;
        }
        part[b] = m;
      }
      for (const Key& p : part)
        if (key_lt(p, best)) best = p;
      launches = 1;
      tiles = a.nblocks;
      nsegs = a.nseg;
      if (tiles_out) {
        tmap = tile_map_small(plan);
        tpart = part;
      }
    } else if (packed) {
      // K+W tables in host memory, one per MODE 5 / 7 piece, by plan index
      std::vector<std::vector<uint32_t>> tabs(plan.launches.size());
      std::vector<uint64_t> tabptr(plan.launches.size(), 0);
      for (size_t i = 0; i < plan.launches.size(); ++i) {
        const Launch& L = plan.launches[i];
        if (!L.fast || (L.mode != 5 && L.mode != 7)) continue;
        tabs[i] = build_kwtable(L);
        tabptr[i] = (uint64_t)(uintptr_t)tabs[i].data();
      }
      const ScanPack P = pack_scan(plan, max_blocks, max_segs);
      std::vector<Segment> segs(max_segs);
      // one partial per tile, all launches (k_reduce folds them); each launch
      // writes its own slice, from part_off (p1hip.hip run_range)
      std::vector<Key> part(P.total_blocks, kPoison);
      uint32_t part_off = 0;
      for (const ScanBatch& B : P.batches) {
        err = fill_segments(plan, P, B, tabptr.data(), segs.data(), ctr);
        if (!err.empty()) {
          fprintf(stderr, "segment error: %s\n", err.c_str());
          return 1;
        }
        if ((uint64_t)part_off + B.blocks > part.size()) {
          fprintf(stderr, "packing error: launch past the %zu packed tiles\n", part.size());
          return 1;
        }
        for (uint32_t b = 0; b < B.blocks; ++b) part[part_off + b] = scan_tile(segs.data(), (uint32_t)B.count, b);
        part_off += B.blocks;
        nsegs += B.count;
      }
      if (part_off != plan.total_blocks || P.total_blocks != plan.total_blocks) {
        fprintf(stderr, "packing error: %u tiles replayed, %u packed, %u planned\n", part_off, P.total_blocks,
                plan.total_blocks);
        return 1;
      }
      for (const Key& p : part)
        if (key_lt(p, best)) best = p;
      launches = P.batches.size();
      tiles = part.size();
      if (tiles_out) {
        tmap = tile_map(plan, P);
        tpart = part;
      }
    } else {
      for (const Launch& L : plan.launches) {
        Key k;
        if (L.fast) {
          k = dispatch_fast(L);
        } else {
          k = {~0ull, ~0ull};
          for (uint64_t g = 0; g < L.threads; ++g) {
            Key t = generic_thread(L.ga, g);
            if (key_lt(t, k)) k = t;
          }
        }
        if (key_lt(k, best)) best = k;
      }
    }
  }
  if (best.h == ~0ull) best.n = 0;  // identity of miner.go:56
  printf("%" PRIu64 " %" PRIu64 " %d %d %s\n", best.h, best.n, nf, ng, vars.empty() ? "-" : vars.c_str());
  print_tiles(tmap, tpart);
  if (packed || small) fprintf(stderr, "launches=%zu tiles=%" PRIu64 " segs=%" PRIu64 "\n", launches, tiles, nsegs);
  return 0;
}
