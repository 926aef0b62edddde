// lsp_fake_pool_async -- TEST DOUBLE for the pipelined pool's CPU tests: the
// very miner::RunPool that `p1miner lsp --conns C --inflight N` runs
// (p1_amd/host/miner_pool.hpp), over a backend that answers every piece with
// the oracle (oracle/libp1oracle.so, the CPU checker) instead of the GPU.
// Like the GPU, the backend works while the round loop goes on: Submit only
// queues the round for a worker thread, which answers the rounds in order;
// Collect blocks until its round is done.
//
//   lsp_fake_pool_async <host:port> --conns C [--inflight N] [--chunk C] [--linger-us U] [--round-log FILE]
//                 [--stats] [--epoch-limit K] [--epoch-millis M] [--window W] [--copies K] [--connect-copies K]
// FAKE_ROUND_SLEEP_MS=n: the worker sleeps n ms per round, so that rounds stay
// outstanding long enough for a test to send more jobs, or to end the pool.
// P1LSP_* env vars inject loss (lspnet.hpp).
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <condition_variable>
#include <deque>
#include <map>
#include <mutex>
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
  explicit Worker(long sleep_ms) : sleep_ms_(sleep_ms), th_([this] { run(); }) {}
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
  std::mutex mu_;
  std::condition_variable cv_;
  std::deque<std::pair<uint64_t, std::vector<miner::Piece>>> todo_;
  std::map<uint64_t, std::vector<miner::PieceResult>> done_;
  uint64_t handle_ = 0;
  bool quit_ = false;
  std::thread th_;  // last: started when everything above exists
};

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  lspnet::ConfigureFromEnv();
  lsp::Params prm = lsp::NewParams();
  prm.Copies = lsp::DefaultAppCopies;  // like p1miner
  uint64_t conns = 0, chunk = miner::kDefaultChunk, linger_us = 0, inflight = 1;
  bool want_stats = false;
  std::string round_log;
  for (int i = 2; i < argc; ++i) {
    if (!strcmp(argv[i], "--epoch-limit") && i + 1 < argc) prm.EpochLimit = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--epoch-millis") && i + 1 < argc) prm.EpochMillis = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--window") && i + 1 < argc) prm.WindowSize = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--copies") && i + 1 < argc) prm.Copies = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--connect-copies") && i + 1 < argc) prm.ConnectCopies = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--conns") && i + 1 < argc) { if (!parse_u64(argv[++i], &conns) || conns < 1 || conns > 256) return 2; }
    else if (!strcmp(argv[i], "--inflight") && i + 1 < argc) { if (!parse_u64(argv[++i], &inflight) || inflight < 1 || inflight > 4) return 2; }
    else if (!strcmp(argv[i], "--chunk") && i + 1 < argc) { if (!parse_u64(argv[++i], &chunk)) return 2; }
    else if (!strcmp(argv[i], "--linger-us") && i + 1 < argc) { if (!parse_u64(argv[++i], &linger_us) || linger_us > 60000000) return 2; }
    else if (!strcmp(argv[i], "--round-log") && i + 1 < argc) round_log = argv[++i];
    else if (!strcmp(argv[i], "--stats")) want_stats = true;
    else return 2;
  }
  if (conns == 0) return 2;
  const char* sl = getenv("FAKE_ROUND_SLEEP_MS");
  const long sleep_ms = sl && *sl ? atol(sl) : 0;
  Worker worker(sleep_ms);
  miner::AsyncBackend async;
  async.Submit = [&](const std::vector<miner::Piece>& pieces) { return worker.Submit(pieces); };
  async.Collect = [&](uint64_t h, std::vector<miner::PieceResult>* out) { worker.Collect(h, out); };
  miner::PoolStats st;
  std::string err;
  const int rc = miner::RunPool(
      argv[1], prm, (int)conns, chunk, (long)linger_us,
      [sleep_ms](const std::vector<miner::Piece>& pieces, std::vector<miner::PieceResult>* out) {
        if (sleep_ms > 0) std::this_thread::sleep_for(std::chrono::milliseconds(sleep_ms));
        answer(pieces, out);
      },
      async, (int)inflight, round_log, &st, &err);
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
