// p1gpuserver -- `p1server lsp` that also scans on its own GPU: the server's
// LSP loop (server_lsp.hpp) plus S local slots (local_slots.hpp) answered
// through libp1hip.so's asynchronous batch calls.
//
//   p1gpuserver [p1server's lsp options] [--device D] [--slots S] [--local-chunk C] [--inflight N]
//               [--linger-us U] [--stats] lsp <port>
//
// Every client's job is visible to the server at once, so a round holds one
// chunk of every waiting job (up to --slots, default 64, 1..256) instead of
// what a multi-connection miner happens to hold after the server's round trip,
// and a job costs the server one Request in and one Result out, not a second
// pair with a miner.  A local slot gets chunks of at most --local-chunk nonces
// (default 2^24, the most that shares k_scan launches in
// p1hip_scan_batch_wide); every round is one p1hip_batch_submit(..., wide = 1)
// and up to --inflight rounds (default 2, 1..P1HIP_MAX_INFLIGHT) are
// outstanding, collected by p1hip_batch_wait on a second thread
// (miner::SubmitPieces / CollectPieces, the pool's backend functions).
// --linger-us U: wait up to U us for more jobs before a round is cut while
// nothing is outstanding (default 0).  Remote miners may still Join (`p1miner
// lsp host:port`); they get chunks of --chunk nonces as from p1server.
//
// If the GPU fails (bitcoin::HipError from a submit or a wait) one line goes
// to stderr, the local slots are lost like any miner -- their chunks go back
// to their requests -- and the server goes on with its remote miners; the
// device is not re-initialised.  --exit-after N and SIGTERM / SIGINT collect
// every outstanding round, write its Results, close the server and exit 0.
// --stats: one JSON line on stderr at exit: slots, inflight, local_chunk,
// rounds, pieces, max_round (most pieces in one round), max_outstanding (most
// rounds out at once), failures, and the library's p1hip_get_batch_stats /
// _wide_stats / _async_stats as "batch" / "wide" / "async".
// P1LSP_* env vars inject loss (lspnet.hpp).
#include <inttypes.h>
#include <signal.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/p1hip.h"
#include "bitcoin.hpp"
#include "lspnet.hpp"
#include "miner_pool.hpp"
#include "server_lsp.hpp"

static int usage() {
  fprintf(stderr,
          "usage: p1gpuserver [--chunk C] [--epoch-limit K] [--epoch-millis M] [--window W] [--copies K] "
          "[--exit-after N] [--device D] [--slots S] [--local-chunk C] [--inflight N] [--linger-us U] [--stats] "
          "lsp <port>\n");
  return 2;
}

int main(int argc, char** argv) {
  signal(SIGPIPE, SIG_IGN);
  lspnet::ConfigureFromEnv();
  server::LspServerArgs args;
  server::LocalOptions lo;
  lo.name = "p1gpuserver";
  bool want_stats = false;
  int port = 0, dev = 0;
  const bool ok = server::ParseLocalServerArgs(
      argc, argv, P1HIP_MAX_INFLIGHT, &args, &lo, &want_stats, &port, [&](int ac, char** av, int* i) {
        if (strcmp(av[*i], "--device") || *i + 1 >= ac) return 0;
        uint64_t v = 0;
        if (!server::ParseU64(av[++*i], &v) || v > 1023) return -1;
        dev = (int)v;
        return 1;
      });
  if (!ok) return usage();
  // the flags are checked; open the GPU before listening, so the first request does not pay for it
  if (p1hip_init_devices(&dev, 1) != P1HIP_OK) {
    fprintf(stderr, "p1hip init: %s\n", p1hip_last_error());
    return 1;
  }
  lo.backend.Submit = [](const std::vector<miner::Piece>& pieces) { return miner::SubmitPieces(pieces, true); };
  lo.backend.Collect = [](uint64_t h, std::vector<miner::PieceResult>* out) { miner::CollectPieces(h, out); };
  server::LocalStats st;
  const int rc = server::RunLsp(port, args.prm, args.chunk, args.exit_after, &lo, &st);
  if (want_stats) {
    p1hip_batch_stats_t b = {};
    p1hip_wide_stats_t w = {};
    p1hip_async_stats_t a = {};
    p1hip_get_batch_stats(&b);
    p1hip_get_wide_stats(&w);
    p1hip_get_async_stats(&a);
    fprintf(stderr,
            "{%s, \"batch\": {\"calls\": %" PRIu64 ", \"requests\": %" PRIu64 ", \"coalesced\": %" PRIu64
            ", \"individual\": %" PRIu64 ", \"empty\": %" PRIu64 ", \"launches\": %" PRIu64 ", \"tiles\": %" PRIu64
            ", \"nonces\": %" PRIu64 ", \"wall_ms\": %.3f}, \"wide\": {\"calls\": %" PRIu64 ", \"requests\": %" PRIu64
            ", \"empty\": %" PRIu64 ", \"small\": %" PRIu64 ", \"wide\": %" PRIu64 ", \"individual\": %" PRIu64
            ", \"scan_launches\": %" PRIu64 ", \"scan_segments\": %" PRIu64 ", \"generic_launches\": %" PRIu64
            ", \"generic_segments\": %" PRIu64 ", \"tiles\": %" PRIu64 ", \"nonces\": %" PRIu64
            ", \"wall_ms\": %.3f}, \"async\": {\"submits\": %" PRIu64 ", \"waits\": %" PRIu64 ", \"busy\": %" PRIu64
            ", \"max_inflight\": %" PRIu64 ", \"submit_ms\": %.3f, \"wait_ms\": %.3f}}\n",
            server::StatsJsonFields(st).c_str(), b.calls, b.requests, b.coalesced, b.individual, b.empty, b.launches,
            b.tiles, b.nonces, b.wall_ms, w.calls, w.requests, w.empty, w.small, w.wide, w.individual, w.scan_launches,
            w.scan_segments, w.generic_launches, w.generic_segments, w.tiles, w.nonces, w.wall_ms, a.submits, a.waits,
            a.busy, a.max_inflight, a.submit_ms, a.wait_ms);
    fflush(stderr);
  }
  p1hip_shutdown();
  return rc;
}
