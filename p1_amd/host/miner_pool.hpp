// miner_pool.hpp -- a miner that holds several LSP connections and answers
// their jobs in rounds: one piece of every connection's current job per
// backend call, so that the jobs of many connections reach the GPU together
// (p1hip_scan_batch / p1hip_scan_batch_wide) although the protocol hands a
// connection one job at a time (miner.go:49-67, scheduler.hpp).  To the
// server every connection is simply a miner.
//
// Two parts, so that the logic is testable without a network or a device:
//   miner::Rounds   no threads, no I/O: the jobs of the connections, cut into
//                   rounds and folded back (tests/pool_test.cpp)
//   miner::RunPool  the connections, one reader thread each, the round loop,
//                   shutdown and the statistics (tests/lsp/lsp_fake_pool.cpp
//                   runs it over the CPU oracle, p1miner lsp --conns on the GPU)
// HIP-free: the backend is a std::function; the GPU one is
// miner::AnswerPieces (miner_gpu.cpp).
#pragma once
#include <errno.h>
#include <signal.h>
#include <stdint.h>
#include <stdio.h>
#include <sys/eventfd.h>
#include <unistd.h>

#include <chrono>
#include <condition_variable>
#include <deque>
#include <exception>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "bitcoin.hpp"
#include "lsp.hpp"

namespace miner {

// One piece of one connection's current job: scan [lower, upper] of msg.
struct Piece {
  int conn = 0;
  uint64_t job = 0;  // serial of the job it was cut from (a result for a forgotten job is ignored)
  std::string msg;
  uint64_t lower = 0, upper = 0;
};
struct PieceResult {
  uint64_t hash = UINT64_MAX, nonce = 0;
};
// A finished job: the Result (hash, nonce) to write on connection `conn`.
struct Done {
  int conn = 0;
  uint64_t hash = UINT64_MAX, nonce = 0;
};

// The bookkeeping of jobs cut into rounds.  Every connection has a FIFO of
// decoded Requests; the front one is its active job, a cursor as in
// ScanChunked (msg, next, upper; best, best_n, found).  A round takes one
// piece of at most `chunk` nonces from every active job, so every connection
// with a job advances by one piece per round and a short job waits at most
// one round behind a long one on another connection (what scheduler.hpp
// keeps on the server side).  Contract: every job's Result is bit for bit
// what miner::HandleRequest(req, chunk) returns -- its pieces are folded in
// increasing nonce order with a strict '<', so the first minimum wins, and a
// job that never saw a hash below MaxUint64 answers nonce 0.
class Rounds {
 public:
  // A decoded Request arrived on `conn`.  Scanned whatever its Type, like
  // miner.go:55-63.  A job with Lower > Upper is finished as (MaxUint64, 0)
  // the moment it becomes its connection's active job and yields no piece.
  void Push(int conn, const bitcoin::Message& req) {
    Conn& c = conns_[conn];
    Job j;
    j.serial = ++serial_;
    j.msg = req.Data;
    j.next = req.Lower;
    j.upper = req.Upper;
    j.empty = req.Lower > req.Upper;
    c.q.push_back(std::move(j));
    settle(conn, c);
  }

  // The next round: for every connection whose active job has no piece in
  // flight, [next, min(upper, next + chunk - 1)], without wrapping at
  // upper == 2^64-1.  In increasing connection order.
  std::vector<Piece> Next(uint64_t chunk) {
    if (chunk == 0) chunk = kDefaultChunk;
    std::vector<Piece> out;
    for (auto& kv : conns_) {
      if (kv.second.q.empty()) continue;
      Job& j = kv.second.q.front();
      if (j.inflight) continue;
      Piece p;
      p.conn = kv.first;
      p.job = j.serial;
      p.msg = j.msg;
      p.lower = j.next;
      p.upper = (j.upper - j.next >= chunk) ? j.next + (chunk - 1) : j.upper;
      j.inflight = true;
      out.push_back(std::move(p));
    }
    return out;
  }

  // Folds results[i] into the job of pieces[i], as ScanChunked does, and
  // returns the jobs this finished (followed by any empty job that became
  // active behind them), in the order of `pieces`.  A piece whose job is gone
  // (Drop) is ignored.
  std::vector<Done> Finish(const std::vector<Piece>& pieces, const std::vector<PieceResult>& results) {
    for (size_t i = 0; i < pieces.size() && i < results.size(); ++i) {
      const Piece& p = pieces[i];
      auto it = conns_.find(p.conn);
      if (it == conns_.end() || it->second.q.empty()) continue;
      Job& j = it->second.q.front();
      if (j.serial != p.job || !j.inflight) continue;
      j.inflight = false;
      if (results[i].hash < j.best) {
        j.best = results[i].hash;
        j.best_n = results[i].nonce;
        j.found = true;
      }
      if (p.upper == j.upper) {
        done_.push_back({p.conn, j.best, j.found ? j.best_n : 0});
        it->second.q.pop_front();
        settle(p.conn, it->second);
      } else {
        j.next = p.upper + 1;
      }
    }
    return TakeDone();
  }

  // Jobs finished without a piece (empty ranges) since the last call.
  std::vector<Done> TakeDone() {
    std::vector<Done> d;
    d.swap(done_);
    return d;
  }

  // Forgets a lost connection's jobs, the unanswered empty ones included;
  // results for its pieces still in flight are ignored by Finish.
  void Drop(int conn) {
    conns_.erase(conn);
    std::vector<Done> keep;
    for (const Done& d : done_)
      if (d.conn != conn) keep.push_back(d);
    done_.swap(keep);
  }

  // Connections that have an active job.
  size_t Active() const {
    size_t n = 0;
    for (const auto& kv : conns_) n += !kv.second.q.empty();
    return n;
  }
  bool HasDone() const { return !done_.empty(); }

 private:
  struct Job {
    uint64_t serial = 0;
    std::string msg;
    uint64_t next = 0, upper = 0;
    uint64_t best = UINT64_MAX, best_n = 0;
    bool found = false, empty = false, inflight = false;
  };
  struct Conn {
    std::deque<Job> q;
  };

  // answer the empty jobs at the front of a connection's queue
  void settle(int conn, Conn& c) {
    while (!c.q.empty() && c.q.front().empty) {
      done_.push_back({conn, UINT64_MAX, 0});
      c.q.pop_front();
    }
  }

  std::map<int, Conn> conns_;
  std::vector<Done> done_;
  uint64_t serial_ = 0;
};

struct PoolStats {
  uint64_t conns_wanted = 0;  // --conns
  uint64_t conns_open = 0;    // ... that joined the server
  uint64_t requests = 0;      // jobs answered
  uint64_t pieces = 0;        // pieces handed to the backend
  uint64_t rounds = 0;        // backend calls
  uint64_t max_round = 0;     // most pieces in one round
  uint64_t lost_conns = 0;    // connections whose Read or Write failed
};

// "conns_wanted": .., ... "lost_conns": ..  -- the members of a JSON object,
// without its braces (p1miner adds the library's statistics after them).
inline std::string StatsJsonFields(const PoolStats& s) {
  char b[320];
  snprintf(b, sizeof b,
           "\"conns_wanted\": %llu, \"conns_open\": %llu, \"requests\": %llu, \"pieces\": %llu, \"rounds\": %llu, "
           "\"max_round\": %llu, \"lost_conns\": %llu",
           (unsigned long long)s.conns_wanted, (unsigned long long)s.conns_open, (unsigned long long)s.requests,
           (unsigned long long)s.pieces, (unsigned long long)s.rounds, (unsigned long long)s.max_round,
           (unsigned long long)s.lost_conns);
  return b;
}

// Fills one (hash, nonce) per piece: what scanning [lower, upper] of msg gives.
using PoolBackend = std::function<void(const std::vector<Piece>&, std::vector<PieceResult>*)>;

// The GPU backend (miner_gpu.cpp): one piece through p1hip_scan, two or more
// through one p1hip_scan_batch call, or one p1hip_scan_batch_wide call with
// `wide`.  Throws bitcoin::HipError.
void AnswerPieces(const std::vector<Piece>& pieces, bool wide, std::vector<PieceResult>* out);

namespace pool_detail {
// SIGTERM / SIGINT end the pool: the handler only writes to an eventfd, a
// watcher thread turns that into the pool's stop flag.
inline int& signal_fd() {
  static int fd = -1;
  return fd;
}
inline void on_signal(int) {
  const int fd = signal_fd();
  const uint64_t one = 1;
  if (fd >= 0) {
    ssize_t r = write(fd, &one, sizeof one);
    (void)r;
  }
}
}  // namespace pool_detail

// Opens `conns` LSP connections to hostport, one after another, each sending
// its Join (miner.go:13-31), and answers their Requests in rounds until every
// connection is gone or SIGTERM / SIGINT arrives; then the round in flight is
// finished, every client is closed and 0 is returned.  1 (with *err) if no
// connection could be opened; with only some, the pool runs on those.
// Threads: one reader per connection (Read -> Unmarshal, the error ignored as
// at miner.go:54-55 -> Rounds::Push) and the round loop on the calling
// thread, which waits for an active job, lingers at most linger_us while
// fewer jobs are active than connections alive (0: takes what is there),
// forms the round, calls the backend once, folds and writes every finished
// Result on its own connection.  A connection whose Read or Write fails is
// dropped.  One mutex guards the pool's state and is never held across a
// call into an lsp::Client, whose own mutex is the only other lock.
// round_log (if not empty): one appended text line per round, the round's
// index and then conn:lower:upper for each of its pieces.
// An exception of the backend ends the pool the same way and is rethrown.
inline int RunPool(const std::string& hostport, const lsp::Params& params, int conns, uint64_t chunk, long linger_us,
                   const PoolBackend& backend, const std::string& round_log, PoolStats* stats,
                   std::string* err = nullptr) {
  PoolStats st;
  st.conns_wanted = (uint64_t)(conns > 0 ? conns : 0);
  std::vector<std::unique_ptr<lsp::Client>> clis;
  std::string first_err;
  for (int i = 0; i < conns; ++i) {
    std::string e;
    std::unique_ptr<lsp::Client> c = lsp::NewClient(hostport, params, &e);
    if (c && !c->Write(bitcoin::Marshal(bitcoin::NewJoin()), &e)) {
      c->Close();
      c.reset();
    }
    if (c) clis.push_back(std::move(c));
    else if (first_err.empty()) first_err = e;
  }
  st.conns_open = clis.size();
  if (clis.empty()) {
    if (err) *err = first_err;
    if (stats) *stats = st;
    return 1;
  }

  std::mutex mu;
  std::condition_variable cv;
  Rounds rounds;
  std::vector<char> lost(clis.size(), 0);
  size_t alive = clis.size();
  bool stop = false;

  auto lose = [&](int conn) {  // with mu held
    if (lost[conn]) return;
    lost[conn] = 1;
    rounds.Drop(conn);
    --alive;
    ++st.lost_conns;
  };

  const int efd = eventfd(0, EFD_CLOEXEC);
  if (efd < 0) {
    for (auto& c : clis) c->Close();
    if (err) *err = "eventfd failed";
    if (stats) *stats = st;
    return 1;
  }
  pool_detail::signal_fd() = efd;
  struct sigaction sa = {}, old_term = {}, old_int = {};
  sa.sa_handler = pool_detail::on_signal;
  sigemptyset(&sa.sa_mask);
  sa.sa_flags = SA_RESTART;
  sigaction(SIGTERM, &sa, &old_term);
  sigaction(SIGINT, &sa, &old_int);
  bool watcher_quit = false;
  std::thread watcher([&] {
    uint64_t v = 0;
    while (read(efd, &v, sizeof v) < 0 && errno == EINTR) {}
    std::lock_guard<std::mutex> g(mu);
    if (!watcher_quit) stop = true;
    cv.notify_all();
  });

  std::vector<std::thread> readers;
  for (size_t i = 0; i < clis.size(); ++i) {
    readers.emplace_back([&, i] {
      lsp::Client* cli = clis[i].get();
      for (;;) {
        std::string buf;
        if (!cli->Read(&buf)) break;
        bitcoin::Message req;
        bitcoin::Unmarshal(buf, &req);  // miner.go:54-55: a fresh Message, the error ignored
        std::lock_guard<std::mutex> g(mu);
        if (lost[i]) break;
        rounds.Push((int)i, req);
        cv.notify_all();
      }
      std::lock_guard<std::mutex> g(mu);
      if (!stop) lose((int)i);  // a Read that fails after Close is not a loss
      cv.notify_all();
    });
  }

  FILE* logf = round_log.empty() ? nullptr : fopen(round_log.c_str(), "a");
  auto answer = [&](const std::vector<Done>& done) {  // without mu
    for (const Done& d : done) {
      if (clis[d.conn]->Write(bitcoin::Marshal(bitcoin::NewResult(d.hash, d.nonce)))) continue;
      std::lock_guard<std::mutex> g(mu);
      if (!stop) lose(d.conn);
    }
  };

  std::exception_ptr failure;
  try {
    std::unique_lock<std::mutex> lk(mu);
    for (;;) {
      cv.wait(lk, [&] { return stop || alive == 0 || rounds.Active() > 0 || rounds.HasDone(); });
      if (stop || alive == 0) break;
      if (linger_us > 0 && rounds.Active() < alive)
        cv.wait_for(lk, std::chrono::microseconds(linger_us),
                    [&] { return stop || alive == 0 || rounds.Active() >= alive; });
      std::vector<Done> done = rounds.TakeDone();
      const std::vector<Piece> pieces = rounds.Next(chunk);
      st.requests += done.size();
      lk.unlock();
      answer(done);
      if (!pieces.empty()) {
        if (logf) {
          fprintf(logf, "%llu", (unsigned long long)st.rounds);
          for (const Piece& p : pieces)
            fprintf(logf, " %d:%llu:%llu", p.conn, (unsigned long long)p.lower, (unsigned long long)p.upper);
          fputc('\n', logf);
          fflush(logf);
        }
        std::vector<PieceResult> res(pieces.size());
        backend(pieces, &res);
        lk.lock();
        done = rounds.Finish(pieces, res);
        ++st.rounds;
        st.pieces += pieces.size();
        if (pieces.size() > st.max_round) st.max_round = pieces.size();
        st.requests += done.size();
        lk.unlock();
        answer(done);
      }
      lk.lock();
    }
  } catch (...) {
    failure = std::current_exception();
  }

  {
    std::lock_guard<std::mutex> g(mu);
    stop = true;  // from here on a failing Read is the Close below, not a loss
  }
  for (auto& c : clis) c->Close();  // unblocks its reader
  for (auto& t : readers) t.join();
  {
    std::lock_guard<std::mutex> g(mu);
    watcher_quit = true;
  }
  pool_detail::on_signal(0);  // wakes the watcher
  watcher.join();
  sigaction(SIGTERM, &old_term, nullptr);
  sigaction(SIGINT, &old_int, nullptr);
  pool_detail::signal_fd() = -1;
  close(efd);
  if (logf) fclose(logf);
  if (stats) *stats = st;
  if (failure) std::rethrow_exception(failure);
  return 0;
}

}  // namespace miner
