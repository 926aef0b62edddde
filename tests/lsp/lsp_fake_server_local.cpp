// lsp_fake_server_local -- TEST DOUBLE for p1gpuserver's CPU tests: the very
// server::RunLsp loop and local slots that p1gpuserver runs
// (p1_amd/host/server_lsp.hpp, local_slots.hpp), over a backend that answers
// every piece with the oracle (oracle/libp1oracle.so, the CPU checker) instead
// of the GPU.  Like the GPU, the backend works while the server goes on:
// Submit only queues the round for a worker thread, which answers the rounds
// in order; Collect blocks until its round is done.
//
//   lsp_fake_server_local [p1server's lsp options] [--slots S] [--local-chunk C] [--inflight N] [--linger-us U]
//                         [--stats] [--fail-submit K] lsp <port>
// --fail-submit K (the double only): the K-th Submit (from 1) throws, as the
// GPU backend does when the device fails.
// FAKE_ROUND_SLEEP_MS=n: the worker sleeps n ms per round, so that rounds stay
// outstanding long enough for a test to send more jobs, or to end the server.
// P1LSP_* env vars inject loss (lspnet.hpp).
#include <signal.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <condition_variable>
#include <deque>
#include <map>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../../p1_amd/host/bitcoin.hpp"
#include "../../p1_amd/host/lspnet.hpp"
#include "../../p1_amd/host/miner_pool.hpp"
#include "../../p1_amd/host/server_lsp.hpp"

extern "C" int p1o_scan(const uint8_t* msg, size_t len, uint64_t lower, uint64_t upper, uint64_t* out_hash,
                        uint64_t* out_nonce);

static void answer(const std::vector<miner::Piece>& pieces, std::vector<miner::PieceResult>* out) {
  out->assign(pieces.size(), miner::PieceResult());
  for (size_t i = 0; i < pieces.size(); ++i) {
    const miner::Piece& p = pieces[i];
    if (p.lower <= p.upper)
      p1o_scan((const uint8_t*)p.msg.data(), p.msg.size(), p.lower, p.upper, &(*out)[i].hash, &(*out)[i].nonce);
  }
}

// One worker thread answering the submitted rounds in order.
class Worker {
 public:
  Worker(long sleep_ms, uint64_t fail_submit) : sleep_ms_(sleep_ms), fail_submit_(fail_submit), th_([this] { run(); }) {}
  ~Worker() {
    {
      std::lock_guard<std::mutex> g(mu_);
      quit_ = true;
    }
    cv_.notify_all();
    th_.join();
  }
  uint64_t Submit(const std::vector<miner::Piece>& pieces) {
    std::lock_guard<std::mutex> g(mu_);
    if (++submits_ == fail_submit_) throw std::runtime_error("fake device failure in Submit " + std::to_string(submits_));
    todo_.push_back({++handle_, pieces});
    cv_.notify_all();
    return handle_;
  }
  void Collect(uint64_t handle, std::vector<miner::PieceResult>* out) {
    std::unique_lock<std::mutex> lk(mu_);
    cv_.wait(lk, [&] { return done_.count(handle) > 0; });
    *out = std::move(done_[handle]);
    done_.erase(handle);
  }

 private:
  void run() {
    std::unique_lock<std::mutex> lk(mu_);
    for (;;) {
      cv_.wait(lk, [&] { return quit_ || !todo_.empty(); });
      if (todo_.empty()) return;  // quit, and nothing left to answer
      std::pair<uint64_t, std::vector<miner::Piece>> job = std::move(todo_.front());
      todo_.pop_front();
      lk.unlock();
      if (sleep_ms_ > 0) std::this_thread::sleep_for(std::chrono::milliseconds(sleep_ms_));
      std::vector<miner::PieceResult> res;
      answer(job.second, &res);
      lk.lock();
      done_[job.first] = std::move(res);
      cv_.notify_all();
    }
  }
  const long sleep_ms_;
  const uint64_t fail_submit_;
  std::mutex mu_;
  std::condition_variable cv_;
  std::deque<std::pair<uint64_t, std::vector<miner::Piece>>> todo_;
  std::map<uint64_t, std::vector<miner::PieceResult>> done_;
  uint64_t handle_ = 0, submits_ = 0;
  bool quit_ = false;
  std::thread th_;  // last: started when everything above exists
};

int main(int argc, char** argv) {
  signal(SIGPIPE, SIG_IGN);
  lspnet::ConfigureFromEnv();
  server::LspServerArgs args;
  server::LocalOptions lo;
  lo.name = "lsp_fake_server_local";
  bool want_stats = false;
  int port = 0;
  uint64_t fail_submit = 0;
  const bool ok = server::ParseLocalServerArgs(argc, argv, 4, &args, &lo, &want_stats, &port,
                                               [&](int ac, char** av, int* i) {
                                                 if (strcmp(av[*i], "--fail-submit") || *i + 1 >= ac) return 0;
                                                 return server::ParseU64(av[++*i], &fail_submit) ? 1 : -1;
                                               });
  if (!ok) {
    fprintf(stderr, "usage: lsp_fake_server_local [lsp options] [--slots S] [--local-chunk C] [--inflight N] "
                    "[--linger-us U] [--stats] [--fail-submit K] lsp <port>\n");
    return 2;
  }
  const char* sl = getenv("FAKE_ROUND_SLEEP_MS");
  int rc;
  server::LocalStats st;
  {
    Worker worker(sl && *sl ? atol(sl) : 0, fail_submit);
    lo.backend.Submit = [&](const std::vector<miner::Piece>& pieces) { return worker.Submit(pieces); };
    lo.backend.Collect = [&](uint64_t h, std::vector<miner::PieceResult>* out) { worker.Collect(h, out); };
    rc = server::RunLsp(port, args.prm, args.chunk, args.exit_after, &lo, &st);
  }
  if (want_stats) {
    fprintf(stderr, "{%s}\n", server::StatsJsonFields(st).c_str());
    fflush(stderr);
  }
  return rc;
}
