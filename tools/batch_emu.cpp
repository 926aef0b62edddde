// batch_emu -- TEST TOOL: replays a p1hip_scan_batch call on the host.
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
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../p1_amd/csrc/batch_plan.hpp"

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

int main(int argc, char** argv) {
  const int ndev = argc > 1 ? atoi(argv[1]) : 1;
  const uint64_t max_tiles = argc > 2 ? strtoull(argv[2], nullptr, 10) : kBatchMaxTiles;
  if (ndev < 1) {
    fprintf(stderr, "usage: %s [ndev [max_tiles]] < requests\n", argv[0]);
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
  const BatchLayout Y = batch_layout(reqs.data(), n, ndev, kBatchMaxNonces, max_tiles);
  if (Y.individual) {
    fprintf(stderr, "%" PRIu64 " request(s) above 2^16 nonces: not a batch replay\n", Y.individual);
    return 1;
  }
  std::vector<Key> out(n, Key{~0ull, 0});  // empty ranges keep the identity
  uint64_t tiles = 0, nsegs = 0;
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
    tiles += L.tiles;
    nsegs += T.segs.size();
  }
  for (size_t i = 0; i < n; ++i) printf("%" PRIu64 " %" PRIu64 "\n", out[i].h, out[i].n);
  fprintf(stderr, "launches=%zu tiles=%" PRIu64 " segs=%" PRIu64 "\n", Y.launches.size(), tiles, nsegs);
  return 0;
}
