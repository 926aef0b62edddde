// local_slots.hpp -- a server that scans on its own device: S virtual miners
// ("local slots") registered with the scheduler next to the remote ones, whose
// chunks are answered in rounds by an asynchronous backend (p1gpuserver: the
// GPU through p1hip_batch_submit / p1hip_batch_wait; tools/lsp_fake_server_local:
// the CPU oracle on a worker thread).  The server sees every client's job at
// once, so a round holds one chunk of every waiting job, up to S, where the
// multi-connection miner (miner_pool.hpp) sees one job per connection and only
// after the server's round trip.  To the scheduler a local slot is just
// another miner: fairness, the fold of a request's chunks (identity
// (MaxUint64, 0), strict '<') and the re-queue of a lost miner's chunk are
// scheduler.hpp's, unchanged, so an answer is bit for bit what one miner
// scanning the whole range returns.  LSP connection ids are positive; the
// local slots are the miners -1 .. -S.
//
// Two parts, as in miner_pool.hpp:
//   server::LocalSlots    no threads, no I/O: the assignments waiting for a
//                         round, when a round is cut and what goes in it, the
//                         rounds that are out and how their results map back
//                         to slots (tests/local_slots_test.cpp)
//   server::LocalRunner   the round thread and the collector thread around it
// HIP-free: the backend is miner::AsyncBackend (miner_pool.hpp); the pieces
// and the GPU backend functions are the pool's own.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <chrono>
#include <condition_variable>
#include <deque>
#include <exception>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "miner_pool.hpp"
#include "scheduler.hpp"

namespace server {

struct LocalStats {
  uint64_t slots = 0;            // --slots
  uint64_t inflight = 1;         // --inflight: rounds that may be outstanding at once
  uint64_t local_chunk = 0;      // --local-chunk
  uint64_t rounds = 0;           // rounds handed to the backend
  uint64_t pieces = 0;           // pieces in them
  uint64_t max_round = 0;        // most pieces in one round
  uint64_t max_outstanding = 0;  // most rounds outstanding at once
  uint64_t failures = 0;         // 1 once the backend failed and the slots were lost
};

// "slots": .., ... "failures": ..  -- the members of a JSON object, without its braces.
inline std::string StatsJsonFields(const LocalStats& s) {
  char b[400];
  snprintf(b, sizeof b,
           "\"slots\": %llu, \"inflight\": %llu, \"local_chunk\": %llu, \"rounds\": %llu, \"pieces\": %llu, "
           "\"max_round\": %llu, \"max_outstanding\": %llu, \"failures\": %llu",
           (unsigned long long)s.slots, (unsigned long long)s.inflight, (unsigned long long)s.local_chunk,
           (unsigned long long)s.rounds, (unsigned long long)s.pieces, (unsigned long long)s.max_round,
           (unsigned long long)s.max_outstanding, (unsigned long long)s.failures);
  return b;
}

// The decisions.  The caller owns the Scheduler and calls Dispatch() itself;
// an Assignment whose miner IsLocal goes to Queue.  A round is cut when
// Ready(): something is queued and fewer than `inflight` rounds are out.  It
// takes everything queued -- at most one piece per slot, the scheduler hands a
// busy miner nothing -- as miner::Piece{conn = slot id, job = request id, msg,
// lower, upper}, in queue order.  Cut() must be followed by Sent(handle) (the
// backend took it) or Fail.  Collected feeds the oldest round's results to
// Scheduler::Result, slot by slot; a slot whose client went away meanwhile is
// simply idle again (the scheduler ignores its result).  Fail abandons every
// round and calls LoseMiner on every slot, so their chunks -- queued, being
// submitted or out -- go back to the front of their requests for whatever
// remote miners there are; nothing is cut afterwards.
//
// A slot's piece holds at most `chunk` nonces, except one that a lost remote
// miner handed back: the scheduler re-deals it with its own bounds
// (scheduler.hpp), and a piece above the backend's coalescing limit simply
// takes the backend's individual route.
class LocalSlots {
 public:
  struct Round {
    uint64_t index = 0;  // rounds sent before this one
    std::vector<miner::Piece> pieces;
    uint64_t handle = 0;  // the backend's
  };

  LocalSlots(int slots, uint64_t chunk, size_t inflight)
      : slots_(slots > 0 ? slots : 1), chunk_(chunk ? chunk : kDefaultChunk), inflight_(inflight ? inflight : 1) {
    st_.slots = (uint64_t)slots_;
    st_.inflight = inflight_;
    st_.local_chunk = chunk_;
  }

  // 2^24 nonces, p1hip_scan_batch_wide's limit for a request that shares
  // launches: above it a piece takes the individual route, which
  // p1hip_batch_wait runs synchronously.
  static constexpr uint64_t kDefaultChunk = 1ull << 24;

  static bool IsLocal(int miner) { return miner < 0; }
  int Slots() const { return slots_; }
  uint64_t Chunk() const { return chunk_; }
  size_t Inflight() const { return inflight_; }

  // Registers the slots as idle miners -1 .. -S with their own chunk size.
  void Join(sched::Scheduler& S) {
    for (int k = 1; k <= slots_; ++k) S.AddMiner(-k, chunk_);
  }

  // An assignment Dispatch() made for a local slot.
  void Queue(const sched::Assignment& a) {
    miner::Piece p;
    p.conn = a.miner;
    p.job = a.req;
    p.msg = a.data;
    p.lower = a.lo;
    p.upper = a.hi;
    queue_.push_back(std::move(p));
  }

  size_t Queued() const { return queue_.size(); }
  size_t Outstanding() const { return out_.size(); }
  bool Submitting() const { return !pending_.empty(); }
  bool Failed() const { return failed_; }
  bool HasOut() const { return !out_.empty(); }
  const Round& Oldest() const { return out_.front(); }
  const LocalStats& Stats() const { return st_; }

  // A round may be cut now.
  bool Ready() const {
    return !failed_ && pending_.empty() && !queue_.empty() && out_.size() < inflight_;
  }
  // --linger-us applies: nothing is out, and slots are still free to take
  // assignments that have not arrived yet (as in the pool: while a round is
  // out, more gather anyway).
  bool Linger() const { return Ready() && out_.empty() && queue_.size() < (size_t)slots_; }

  // Everything queued becomes the next round.  The pieces stay here until Sent.
  const std::vector<miner::Piece>& Cut() {
    pending_.swap(queue_);
    queue_.clear();
    return pending_;
  }

  // The backend took the round Cut() returned and knows it as `handle`.
  void Sent(uint64_t handle) {
    Round r;
    r.index = sent_++;
    r.pieces.swap(pending_);
    r.handle = handle;
    ++st_.rounds;
    st_.pieces += r.pieces.size();
    if (r.pieces.size() > st_.max_round) st_.max_round = r.pieces.size();
    out_.push_back(std::move(r));
    if (out_.size() > st_.max_outstanding) st_.max_outstanding = out_.size();
  }

  // The backend answered round `index` (Oldest().index when it was asked):
  // one Scheduler::Result per piece.  false, and nothing done, if that round
  // was abandoned meanwhile (Fail).
  bool Collected(sched::Scheduler& S, uint64_t index, const std::vector<miner::PieceResult>& results) {
    if (failed_ || out_.empty() || out_.front().index != index) return false;
    const Round& r = out_.front();
    for (size_t i = 0; i < r.pieces.size() && i < results.size(); ++i)
      S.Result(r.pieces[i].conn, results[i].hash, results[i].nonce);
    out_.pop_front();
    return true;
  }

  // The backend failed: every round is abandoned and every slot lost.
  void Fail(sched::Scheduler& S) {
    if (failed_) return;
    failed_ = true;
    st_.failures = 1;
    queue_.clear();
    pending_.clear();
    out_.clear();
    for (int k = 1; k <= slots_; ++k) S.LoseMiner(-k);
  }

 private:
  const int slots_;
  const uint64_t chunk_;
  const size_t inflight_;
  std::vector<miner::Piece> queue_;    // assigned, not in a round yet
  std::vector<miner::Piece> pending_;  // the round being submitted
  std::deque<Round> out_;              // oldest first
  uint64_t sent_ = 0;
  bool failed_ = false;
  LocalStats st_;
};

// The threads.  `mu` is the server's mutex: it guards the Scheduler, the
// LocalSlots and whatever `pump` touches, and is never held across a backend
// call.  pump() is called with `mu` held after results were fed to the
// scheduler (and after a failure): the server's Dispatch() -- remote writes,
// local queueing -- and TakeDone() -- Result writes to clients.
//   round thread   waits until LocalSlots::Ready(), lingers at most linger_us
//                  while Linger(), cuts the round and calls Submit
//   collector      Collect on the oldest round, Scheduler::Result per piece
//                  (LocalSlots::Collected), pump()
// Submit or Collect may throw (the GPU backend: bitcoin::HipError): one line
// on stderr, LocalSlots::Fail, pump(), and both threads end; the device is not
// re-initialised and nothing is retried.  The server goes on with its remote
// miners.  Stop() (without `mu`): no further round is cut, every outstanding
// round is collected and pumped, both threads are joined.
class LocalRunner {
 public:
  LocalRunner(std::mutex& mu, sched::Scheduler& S, LocalSlots& core, miner::AsyncBackend backend, long linger_us,
              std::function<void()> pump, std::string name)
      : mu_(mu), S_(S), core_(core), backend_(std::move(backend)), linger_us_(linger_us), pump_(std::move(pump)),
        name_(std::move(name)) {}
  ~LocalRunner() { Stop(); }

  void Start() {
    round_ = std::thread([this] { round_loop(); });
    collector_ = std::thread([this] { collect_loop(); });
  }

  // With `mu` held: the queue changed.
  void Notify() { cv_.notify_all(); }

  void Stop() {
    {
      std::lock_guard<std::mutex> g(mu_);
      stop_ = true;
    }
    cv_.notify_all();
    if (round_.joinable()) round_.join();
    {
      std::lock_guard<std::mutex> g(mu_);
      quit_ = true;  // nothing is being submitted any more: the collector takes what is out
    }
    cv_.notify_all();
    if (collector_.joinable()) collector_.join();
  }

 private:
  void fail(const std::string& what) {  // with mu_ held
    if (!core_.Failed())
      fprintf(stderr, "%s: the local backend failed (%s): %d local slots lost\n", name_.c_str(), what.c_str(),
              core_.Slots());
    core_.Fail(S_);
    pump_();
    cv_.notify_all();
  }

  void round_loop() {
    std::unique_lock<std::mutex> lk(mu_);
    for (;;) {
      cv_.wait(lk, [&] { return stop_ || core_.Failed() || core_.Ready(); });
      if (stop_ || core_.Failed()) return;
      if (linger_us_ > 0 && core_.Linger()) {
        cv_.wait_for(lk, std::chrono::microseconds(linger_us_),
                     [&] { return stop_ || core_.Failed() || !core_.Linger(); });
        if (stop_ || core_.Failed()) return;
      }
      const std::vector<miner::Piece> pieces = core_.Cut();
      lk.unlock();
      uint64_t handle = 0;
      std::string what;
      bool ok = true;
      try {
        handle = backend_.Submit(pieces);
      } catch (const std::exception& e) {
        ok = false;
        what = e.what();
      } catch (...) {
        ok = false;
        what = "unknown exception";
      }
      lk.lock();
      if (!ok) {
        fail(what);
        return;
      }
      core_.Sent(handle);
      cv_.notify_all();  // the collector
    }
  }

  void collect_loop() {
    std::unique_lock<std::mutex> lk(mu_);
    for (;;) {
      cv_.wait(lk, [&] { return core_.Failed() || core_.HasOut() || quit_; });
      if (core_.Failed() || !core_.HasOut()) return;  // abandoned; or quit and nothing left out
      const uint64_t index = core_.Oldest().index, handle = core_.Oldest().handle;
      std::vector<miner::PieceResult> res(core_.Oldest().pieces.size());
      lk.unlock();
      std::string what;
      bool ok = true;
      try {
        backend_.Collect(handle, &res);
      } catch (const std::exception& e) {
        ok = false;
        what = e.what();
      } catch (...) {
        ok = false;
        what = "unknown exception";
      }
      lk.lock();
      if (core_.Failed()) return;  // the round was abandoned while it ran
      if (!ok) {
        fail(what);
        return;
      }
      core_.Collected(S_, index, res);
      pump_();
      cv_.notify_all();  // the round thread: a round fewer is out
    }
  }

  std::mutex& mu_;
  sched::Scheduler& S_;
  LocalSlots& core_;
  miner::AsyncBackend backend_;
  const long linger_us_;
  std::function<void()> pump_;
  const std::string name_;
  std::condition_variable cv_;
  bool stop_ = false, quit_ = false;
  std::thread round_, collector_;
};

}  // namespace server
