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
  // Connections whose active job has no piece in flight: what Next would cut.
  size_t Free() const {
    size_t n = 0;
    for (const auto& kv : conns_) n += !kv.second.q.empty() && !kv.second.q.front().inflight;
    return n;
  }

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

// Rounds in flight.  A backend that can take a round and answer it later
// (AsyncBackend: Submit now, Collect when it is needed) lets the pool cut and
// submit round k + 1 while round k runs.  Pipeline holds the rounds that are
// out, oldest first, and the one decision of the round loop: with fewer than
// `depth` rounds out and Rounds::Next non-empty, cut and submit another;
// otherwise collect the oldest, fold it (Rounds::Finish) and hand back the
// finished jobs.  Rounds needs no change for this: Next skips a job whose
// piece is in flight, so a job has at most one piece outstanding over all the
// rounds that are out, and its pieces still fold in increasing nonce order.
// No threads, no I/O (tests/pool_pipeline_test.cpp); RunPool calls the parts
// with its own locking, single-threaded users call Step.
class Pipeline {
 public:
  struct Round {
    uint64_t index = 0;  // rounds submitted before this one
    std::vector<Piece> pieces;
    uint64_t handle = 0;  // the backend's
  };

  explicit Pipeline(size_t depth) : depth_(depth ? depth : 1) {}

  size_t Depth() const { return depth_; }
  size_t Outstanding() const { return out_.size(); }
  size_t MaxOutstanding() const { return max_out_; }
  uint64_t Submitted() const { return submitted_; }
  const Round& Oldest() const { return out_.front(); }

  // The next round's pieces, or none: `depth` rounds are out already, or no
  // active job is free (Rounds::Next).  A non-empty result must be submitted
  // and reported with Sent (its jobs are marked in flight).
  std::vector<Piece> Cut(Rounds& rounds, uint64_t chunk) {
    if (out_.size() >= depth_) return {};
    return rounds.Next(chunk);
  }

  // The pieces of Cut went to the backend, which knows them as `handle`.
  const Round& Sent(std::vector<Piece> pieces, uint64_t handle) {
    Round r;
    r.index = submitted_++;
    r.pieces = std::move(pieces);
    r.handle = handle;
    out_.push_back(std::move(r));
    if (out_.size() > max_out_) max_out_ = out_.size();
    return out_.back();
  }

  // The backend answered the oldest round: fold it and return the jobs this finished.
  std::vector<Done> Collected(Rounds& rounds, const std::vector<PieceResult>& results) {
    std::vector<Done> d = rounds.Finish(out_.front().pieces, results);
    out_.pop_front();
    return d;
  }

  // Forget the oldest round without folding it (a backend that failed; shutdown).
  void Abandon() { out_.pop_front(); }

  // The decision, for a caller without locks: kSubmitted (another round went
  // out), kCollected (the oldest came back; *done: the jobs it finished) or
  // kIdle (nothing out and nothing to cut).  B has
  //   uint64_t Submit(const std::vector<Piece>&)
  //   void Collect(uint64_t handle, std::vector<PieceResult>* results)   (sized to the round)
  enum Action { kIdle, kSubmitted, kCollected };
  template <typename B>
  Action Step(Rounds& rounds, B& backend, uint64_t chunk, std::vector<Done>* done) {
    std::vector<Piece> pieces = Cut(rounds, chunk);
    if (!pieces.empty()) {
      const uint64_t h = backend.Submit(pieces);
      Sent(std::move(pieces), h);
      return kSubmitted;
    }
    if (out_.empty()) return kIdle;
    std::vector<PieceResult> res(out_.front().pieces.size());
    backend.Collect(out_.front().handle, &res);
    std::vector<Done> d = Collected(rounds, res);
    if (done) done->insert(done->end(), d.begin(), d.end());
    return kCollected;
  }

 private:
  size_t depth_;
  std::deque<Round> out_;
  size_t max_out_ = 0;
  uint64_t submitted_ = 0;
};

struct PoolStats {
  uint64_t conns_wanted = 0;  // --conns
  uint64_t conns_open = 0;    // ... that joined the server
  uint64_t requests = 0;      // jobs answered
  uint64_t pieces = 0;        // pieces handed to the backend
  uint64_t rounds = 0;        // backend calls
  uint64_t max_round = 0;     // most pieces in one round
  uint64_t lost_conns = 0;    // connections whose Read or Write failed
  uint64_t inflight = 1;      // --inflight: rounds that may be outstanding at once
  uint64_t max_outstanding = 0;  // most rounds outstanding at once
};

// "conns_wanted": .., ... "lost_conns": ..  -- the members of a JSON object,
// without its braces (p1miner adds the library's statistics after them).
inline std::string StatsJsonFields(const PoolStats& s) {
  char b[480];
  snprintf(b, sizeof b,
           "\"conns_wanted\": %llu, \"conns_open\": %llu, \"requests\": %llu, \"pieces\": %llu, \"rounds\": %llu, "
           "\"max_round\": %llu, \"lost_conns\": %llu, \"inflight\": %llu, \"max_outstanding\": %llu",
           (unsigned long long)s.conns_wanted, (unsigned long long)s.conns_open, (unsigned long long)s.requests,
           (unsigned long long)s.pieces, (unsigned long long)s.rounds, (unsigned long long)s.max_round,
           (unsigned long long)s.lost_conns, (unsigned long long)s.inflight, (unsigned long long)s.max_outstanding);
  return b;
}

// Fills one (hash, nonce) per piece: what scanning [lower, upper] of msg gives.
using PoolBackend = std::function<void(const std::vector<Piece>&, std::vector<PieceResult>*)>;

// The GPU backend (miner_gpu.cpp): one piece through p1hip_scan, two or more
// through one p1hip_scan_batch call, or one p1hip_scan_batch_wide call with
// `wide`.  Throws bitcoin::HipError.
void AnswerPieces(const std::vector<Piece>& pieces, bool wide, std::vector<PieceResult>* out);

// The second backend shape, for --inflight N >= 2: Submit hands a round over
// and returns at once with a handle; Collect blocks until that round is done
// and fills one result per piece (`results` comes sized to the round).
// Submit is called from the round loop's thread, Collect from one other
// thread (the collector), in Submit's order.
struct AsyncBackend {
  std::function<uint64_t(const std::vector<Piece>&)> Submit;
  std::function<void(uint64_t, std::vector<PieceResult>*)> Collect;
};

// The GPU one (miner_gpu.cpp): p1hip_batch_submit(..., wide) and
// p1hip_batch_wait; the handle is the ticket.  They copy nothing more than
// AnswerPieces does.  Throw bitcoin::HipError.
uint64_t SubmitPieces(const std::vector<Piece>& pieces, bool wide);
void CollectPieces(uint64_t handle, std::vector<PieceResult>* out);

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
//
// With `async` and inflight >= 2 the loop keeps up to `inflight` rounds
// outstanding (Pipeline): it cuts and submits a round whenever fewer are out
// and a job is free, and answers finished jobs and writes the round log while
// the backend works; it never blocks in the backend.  One more thread, the
// collector, blocks in Collect for the oldest round and folds it.  A round's
// log line is written when it is submitted.  --linger-us applies before a
// round is cut while nothing is outstanding.  On shutdown, when every
// connection is lost and after a backend exception every outstanding round is
// collected (its results ignored) before the clients are closed.  With inflight <= 1 `backend` is used and the loop
// is the synchronous one, call for call.
namespace pool_detail {
inline int RunPoolImpl(const std::string& hostport, const lsp::Params& params, int conns, uint64_t chunk,
                       long linger_us, const PoolBackend* backend_p, const AsyncBackend* async, int inflight,
                       const std::string& round_log, PoolStats* stats, std::string* err) {
  PoolStats st;
  const bool pipelined = async && inflight >= 2;
  st.inflight = pipelined ? (uint64_t)inflight : 1;
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
  Pipeline pipe(pipelined ? (size_t)inflight : 1);
  // Pipelined: the round loop never blocks in the backend.  A collector
  // thread waits for the oldest round (Collect), folds it under `mu` and
  // leaves the finished jobs in `carry`; the round loop cuts and submits a
  // round whenever fewer than `inflight` are out and a job is free
  // (Rounds::Free), and writes Results meanwhile.
  std::vector<Done> carry;      // finished by the collector, not yet written (mu)
  bool collector_quit = false;  // mu
  std::exception_ptr collect_failure;  // mu
  std::thread collector;
  if (pipelined) collector = std::thread([&] {
    std::unique_lock<std::mutex> lk(mu);
    for (;;) {
      cv.wait(lk, [&] { return collector_quit || pipe.Outstanding() > 0; });
      if (pipe.Outstanding() == 0) return;  // quit, and nothing left out
      const uint64_t handle = pipe.Oldest().handle;
      std::vector<PieceResult> res(pipe.Oldest().pieces.size());
      lk.unlock();
      std::exception_ptr ex;
      try {
        async->Collect(handle, &res);
      } catch (...) {
        ex = std::current_exception();
      }
      lk.lock();
      if (ex) {  // the round is abandoned; the round loop ends the pool
        if (!collect_failure) collect_failure = ex;
        pipe.Abandon();
      } else {
        std::vector<Done> d = pipe.Collected(rounds, res);
        st.requests += d.size();
        carry.insert(carry.end(), d.begin(), d.end());
      }
      cv.notify_all();
    }
  });
  if (pipelined) try {
    std::unique_lock<std::mutex> lk(mu);
    for (;;) {
      cv.wait(lk, [&] {
        return stop || alive == 0 || collect_failure || !carry.empty() || rounds.HasDone() ||
               (pipe.Outstanding() < pipe.Depth() && rounds.Free() > 0);
      });
      if (stop || alive == 0 || collect_failure) {
        std::vector<Done> last;
        last.swap(carry);
        lk.unlock();
        answer(last);
        lk.lock();
        break;
      }
      if (linger_us > 0 && pipe.Outstanding() == 0 && rounds.Active() < alive)
        cv.wait_for(lk, std::chrono::microseconds(linger_us),
                    [&] { return stop || alive == 0 || rounds.Active() >= alive; });
      std::vector<Done> done = rounds.TakeDone();
      st.requests += done.size();
      done.insert(done.end(), carry.begin(), carry.end());
      carry.clear();
      std::vector<Piece> pieces = pipe.Cut(rounds, chunk);
      lk.unlock();
      if (!pieces.empty()) {
        if (logf) {
          fprintf(logf, "%llu", (unsigned long long)st.rounds);
          for (const Piece& p : pieces)
            fprintf(logf, " %d:%llu:%llu", p.conn, (unsigned long long)p.lower, (unsigned long long)p.upper);
          fputc('\n', logf);
          fflush(logf);
        }
        ++st.rounds;
        st.pieces += pieces.size();
        if (pieces.size() > st.max_round) st.max_round = pieces.size();
        const uint64_t h = async->Submit(pieces);
        lk.lock();
        pipe.Sent(std::move(pieces), h);
        st.max_outstanding = pipe.MaxOutstanding();
        cv.notify_all();  // the collector
        lk.unlock();
      }
      answer(done);  // while the backend works
      lk.lock();
    }
  } catch (...) {
    failure = std::current_exception();
  }
  if (pipelined) {
    // nothing stays outstanding behind the pool: the collector takes what is
    // out (a Submit that threw left its pieces marked in flight, nothing out)
    {
      std::lock_guard<std::mutex> g(mu);
      collector_quit = true;
    }
    cv.notify_all();
    collector.join();
    if (!failure) failure = collect_failure;
  }
  else try {
    const PoolBackend& backend = *backend_p;
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
        st.max_outstanding = 1;
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
}  // namespace pool_detail

inline int RunPool(const std::string& hostport, const lsp::Params& params, int conns, uint64_t chunk, long linger_us,
                   const PoolBackend& backend, const std::string& round_log, PoolStats* stats,
                   std::string* err = nullptr) {
  return pool_detail::RunPoolImpl(hostport, params, conns, chunk, linger_us, &backend, nullptr, 1, round_log, stats,
                                  err);
}

// RunPool with up to `inflight` rounds outstanding (1: the loop above, through `backend`).
inline int RunPool(const std::string& hostport, const lsp::Params& params, int conns, uint64_t chunk, long linger_us,
                   const PoolBackend& backend, const AsyncBackend& async, int inflight, const std::string& round_log,
                   PoolStats* stats, std::string* err = nullptr) {
  return pool_detail::RunPoolImpl(hostport, params, conns, chunk, linger_us, &backend, &async, inflight, round_log,
                                  stats, err);
}

}  // namespace miner
