// server_lsp.hpp -- the bitcoin server's LSP loop (server.go:83-168), shared
// by `p1server lsp` and the servers that also scan themselves (p1gpuserver,
// tools/lsp_fake_server_local): Read -> Join / Request / Result into the
// scheduler -> Dispatch() to the miners -> TakeDone() to the clients.
//
// Without `local` this is p1server's loop, statement for statement: one
// thread, no signal handling, --exit-after closes the server from that thread.
//
// With `local` (local_slots.hpp) S local slots are miners of the same
// scheduler.  Assignments for positive ids go to srv->Write as before, those
// for local ids to the slots' queue; the collector thread feeds results back
// and runs the same pump.  lsp::Server::Write never blocks and the endpoint
// keeps its state under its own mutex (lsp.hpp, "Threading"), so writing from
// the collector while this thread sits in Read is legal; what needs a mutex
// here is the Scheduler, taken by this loop and by the slots' threads and
// never held across a backend call.  Shutdown -- --exit-after N reached,
// SIGTERM / SIGINT -- runs on a thread of its own, because the thread that
// notices may be the collector: stop cutting, collect every outstanding round
// (their Results are written), only then srv->Close(), which blocks until the
// Results are acknowledged and makes Read return; exit status 0.
#pragma once
#include <errno.h>
#include <signal.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/eventfd.h>
#include <unistd.h>

#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>

#include "bitcoin.hpp"
#include "gojson.hpp"
#include "local_slots.hpp"
#include "lsp.hpp"
#include "scheduler.hpp"

namespace server {

// What a self-scanning server adds to the loop.
struct LocalOptions {
  int slots = 64;                                   // --slots (1..256, as --conns)
  uint64_t chunk = LocalSlots::kDefaultChunk;       // --local-chunk
  int inflight = 2;                                 // --inflight (1..P1HIP_MAX_INFLIGHT)
  long linger_us = 0;                               // --linger-us
  miner::AsyncBackend backend;
  std::string name = "server";                      // for the failure line on stderr
};

inline int RunLsp(int port, const lsp::Params& prm, uint64_t chunk, long exit_after,
                  const LocalOptions* local = nullptr, LocalStats* local_stats = nullptr) {
  std::string err;
  std::unique_ptr<lsp::Server> srv = lsp::NewServer(port, prm, &err);
  if (!srv) {
    printf("%s\n", err.c_str());
    return 1;
  }
  sched::Scheduler S(chunk);
  long answered = 0;
  std::mutex mu;  // S, answered, the local slots (uncontended without them)

  std::unique_ptr<LocalSlots> slots;
  std::unique_ptr<LocalRunner> runner;
  int efd = -1;
  bool finishing = false, closer_quit = false;  // mu
  std::thread closer;
  struct sigaction old_term = {}, old_int = {};
  auto request_finish = [&] { miner::pool_detail::on_signal(0); };  // wakes the closer

  // Dispatch() and TakeDone(), with mu held.  true once --exit-after Results are written.
  std::function<bool()> pump = [&]() -> bool {
    bool queued = false;
    for (const sched::Assignment& a : S.Dispatch()) {
      if (slots && LocalSlots::IsLocal(a.miner)) {
        slots->Queue(a);
        queued = true;
      } else if (!srv->Write(a.miner, bitcoin::Marshal(bitcoin::NewRequest(a.data, a.lo, a.hi)))) {
        S.Unassign(a.miner);
      }
    }
    if (queued) runner->Notify();
    for (const sched::Done& d : S.TakeDone()) {
      srv->Write((int)d.client, bitcoin::Marshal(bitcoin::NewResult(d.hash, d.nonce)));  // client may be gone
      if (exit_after > 0 && ++answered >= exit_after) return true;
    }
    return false;
  };

  if (local) {
    slots.reset(new LocalSlots(local->slots, local->chunk, (size_t)local->inflight));
    slots->Join(S);
    runner.reset(new LocalRunner(mu, S, *slots, local->backend, local->linger_us,
                                 [&] { if (pump()) request_finish(); }, local->name));
    efd = eventfd(0, EFD_CLOEXEC);
    if (efd < 0) {
      printf("eventfd failed\n");
      return 1;
    }
    miner::pool_detail::signal_fd() = efd;
    struct sigaction sa = {};
    sa.sa_handler = miner::pool_detail::on_signal;
    sigemptyset(&sa.sa_mask);
    sa.sa_flags = SA_RESTART;
    sigaction(SIGTERM, &sa, &old_term);
    sigaction(SIGINT, &sa, &old_int);
    runner->Start();
    closer = std::thread([&] {
      uint64_t v = 0;
      while (read(efd, &v, sizeof v) < 0 && errno == EINTR) {}
      {
        std::lock_guard<std::mutex> g(mu);
        if (closer_quit) return;
        finishing = true;
      }
      runner->Stop();  // every outstanding round is collected and its Results written
      srv->Close();    // blocks until the results are acknowledged; Read returns
    });
  }

  // once the signal handlers stand: who reads this line may send SIGTERM at once
  printf("Server listening on port %d\n", srv->Port());
  fflush(stdout);
  int rc = 1;
  for (;;) {
    int id = 0;
    std::string payload;
    const bool ok = srv->Read(&id, &payload, &err);
    if (!ok && id == 0) break;  // server closed
    std::lock_guard<std::mutex> g(mu);
    if (!ok) {
      // a lost connection: a miner's chunk is re-queued, a client's request dropped
      if (S.IsMiner(id)) S.LoseMiner(id);
      else S.CancelClient(id);
    } else {
      // server.go:117 ignores Unmarshal's error and switches on whatever was
      // decoded: a type error (say a negative Lower) still yields the rest of
      // the message.  Unlike the reference, a payload that is not JSON at all
      // is dropped rather than read as a zero Message (a Join).
      bitcoin::Message m;
      if (bitcoin::UnmarshalStatus(payload, &m) != gojson::kSyntaxError) {
        switch (m.Type) {
          case bitcoin::Join: S.AddMiner(id); break;
          case bitcoin::Request: S.Submit(id, m.Data, m.Lower, m.Upper); break;
          case bitcoin::Result: S.Result(id, m.Hash, m.Nonce); break;
        }
      }
    }
    if (pump()) {
      if (!local) {
        srv->Close();  // blocks until the results are acknowledged
        return 0;
      }
      request_finish();
    }
  }

  if (local) {
    {
      std::lock_guard<std::mutex> g(mu);
      closer_quit = true;
      if (finishing) rc = 0;
    }
    request_finish();  // lets the closer out if it still waits
    closer.join();
    runner->Stop();
    sigaction(SIGTERM, &old_term, nullptr);
    sigaction(SIGINT, &old_int, nullptr);
    miner::pool_detail::signal_fd() = -1;
    close(efd);
    if (local_stats) *local_stats = slots->Stats();
  }
  return rc;
}

// The lsp options every server takes (p1server's): --chunk C --epoch-limit K
// --epoch-millis M --window W --copies K --exit-after N.
struct LspServerArgs {
  lsp::Params prm;
  uint64_t chunk = 1ull << 32;
  long exit_after = 0;
};

inline bool ParseU64(const char* s, uint64_t* v) {
  char* end = nullptr;
  if (!s || !*s || *s == '-') return false;
  errno = 0;
  unsigned long long r = strtoull(s, &end, 10);
  if (errno || *end) return false;
  *v = r;
  return true;
}

// Command line of a self-scanning server:
//   [lsp options] [--slots S] [--local-chunk C] [--inflight N] [--linger-us U] [--stats] [extra] lsp <port>
// `extra(argc, argv, &i)`: the program's own flags (1 taken, 0 not its flag,
// -1 bad value).  false: a usage error.
inline bool ParseLocalServerArgs(int argc, char** argv, int max_inflight, LspServerArgs* a, LocalOptions* lo,
                                 bool* want_stats, int* port, const std::function<int(int, char**, int*)>& extra) {
  a->prm = lsp::NewParams();
  a->prm.Copies = lsp::DefaultAppCopies;
  int i = 1;
  for (; i < argc; ++i) {
    uint64_t v = 0;
    const bool has = i + 1 < argc;
    if (!strcmp(argv[i], "--chunk") && has) { if (!ParseU64(argv[++i], &a->chunk) || a->chunk == 0) return false; }
    else if (!strcmp(argv[i], "--epoch-limit") && has) a->prm.EpochLimit = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--epoch-millis") && has) a->prm.EpochMillis = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--window") && has) a->prm.WindowSize = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--copies") && has) a->prm.Copies = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--exit-after") && has) a->exit_after = atol(argv[++i]);
    else if (!strcmp(argv[i], "--slots") && has) { if (!ParseU64(argv[++i], &v) || v < 1 || v > 256) return false; lo->slots = (int)v; }
    else if (!strcmp(argv[i], "--local-chunk") && has) { if (!ParseU64(argv[++i], &lo->chunk) || lo->chunk == 0) return false; }
    else if (!strcmp(argv[i], "--inflight") && has) { if (!ParseU64(argv[++i], &v) || v < 1 || v > (uint64_t)max_inflight) return false; lo->inflight = (int)v; }
    else if (!strcmp(argv[i], "--linger-us") && has) { if (!ParseU64(argv[++i], &v) || v > 60000000) return false; lo->linger_us = (long)v; }
    else if (!strcmp(argv[i], "--stats")) *want_stats = true;
    else {
      const int r = extra ? extra(argc, argv, &i) : 0;
      if (r < 0) return false;
      if (r == 0) break;
    }
  }
  if (a->prm.EpochLimit < 1 || a->prm.EpochMillis < 1 || a->prm.WindowSize < 1) return false;
  if (i + 2 != argc || strcmp(argv[i], "lsp")) return false;
  char* end = nullptr;
  const long p = strtol(argv[i + 1], &end, 10);
  if (!argv[i + 1][0] || *end || p < 0 || p > 65535) return false;
  *port = (int)p;
  return true;
}

}  // namespace server
