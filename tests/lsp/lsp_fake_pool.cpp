// lsp_fake_pool -- TEST DOUBLE for the multi-connection miner's CPU tests:
// the very miner::RunPool that `p1miner lsp --conns C` runs
// (p1_amd/host/miner_pool.hpp), with a backend that answers every piece with
// the oracle (oracle/libp1oracle.so, the CPU checker) instead of the GPU.
//
//   lsp_fake_pool <host:port> --conns C [--chunk C] [--linger-us U] [--round-log FILE] [--stats]
//                 [--epoch-limit K] [--epoch-millis M] [--window W] [--copies K] [--connect-copies K]
// FAKE_ROUND_SLEEP_MS=n: sleep n ms inside every backend call, so that a long
// job stays in flight long enough for a test to send another one.
// P1LSP_* env vars inject loss (lspnet.hpp).
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <string>
#include <thread>
#include <vector>

#include "../../p1_amd/host/bitcoin.hpp"
#include "../../p1_amd/host/lsp.hpp"
#include "../../p1_amd/host/lspnet.hpp"
#include "../../p1_amd/host/miner_pool.hpp"

extern "C" int p1o_scan(const uint8_t* msg, size_t len, uint64_t lower, uint64_t upper, uint64_t* out_hash,
                        uint64_t* out_nonce);

static bool parse_u64(const char* s, uint64_t* v) {
  char* end = nullptr;
  if (!s || !*s || *s == '-') return false;
  errno = 0;
  unsigned long long r = strtoull(s, &end, 10);
  if (errno || *end) return false;
  *v = r;
  return true;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  lspnet::ConfigureFromEnv();
  lsp::Params prm = lsp::NewParams();
  prm.Copies = lsp::DefaultAppCopies;  // like p1miner
  uint64_t conns = 0, chunk = miner::kDefaultChunk, linger_us = 0;
  bool want_stats = false;
  std::string round_log;
  for (int i = 2; i < argc; ++i) {
    if (!strcmp(argv[i], "--epoch-limit") && i + 1 < argc) prm.EpochLimit = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--epoch-millis") && i + 1 < argc) prm.EpochMillis = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--window") && i + 1 < argc) prm.WindowSize = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--copies") && i + 1 < argc) prm.Copies = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--connect-copies") && i + 1 < argc) prm.ConnectCopies = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--conns") && i + 1 < argc) { if (!parse_u64(argv[++i], &conns) || conns < 1 || conns > 256) return 2; }
    else if (!strcmp(argv[i], "--chunk") && i + 1 < argc) { if (!parse_u64(argv[++i], &chunk)) return 2; }
    else if (!strcmp(argv[i], "--linger-us") && i + 1 < argc) { if (!parse_u64(argv[++i], &linger_us) || linger_us > 60000000) return 2; }
    else if (!strcmp(argv[i], "--round-log") && i + 1 < argc) round_log = argv[++i];
    else if (!strcmp(argv[i], "--stats")) want_stats = true;
    else return 2;
  }
  if (conns == 0) return 2;
  const char* sl = getenv("FAKE_ROUND_SLEEP_MS");
  const long sleep_ms = sl && *sl ? atol(sl) : 0;
  miner::PoolStats st;
  std::string err;
  const int rc = miner::RunPool(
      argv[1], prm, (int)conns, chunk, (long)linger_us,
      [sleep_ms](const std::vector<miner::Piece>& pieces, std::vector<miner::PieceResult>* out) {
        if (sleep_ms > 0) std::this_thread::sleep_for(std::chrono::milliseconds(sleep_ms));
        for (size_t i = 0; i < pieces.size(); ++i) {
          const miner::Piece& p = pieces[i];
          uint64_t h = UINT64_MAX, n = 0;
          if (p.lower <= p.upper) p1o_scan((const uint8_t*)p.msg.data(), p.msg.size(), p.lower, p.upper, &h, &n);
          (*out)[i].hash = h;
          (*out)[i].nonce = n;
        }
      },
      round_log, &st, &err);
  if (rc != 0) {
    printf("Failed to join with server: %s\n", err.c_str());
    return 1;
  }
  if (want_stats) {
    printf("{%s}\n", miner::StatsJsonFields(st).c_str());
    fflush(stdout);
  }
  return 0;
}
