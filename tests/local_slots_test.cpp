// Model-based test of the server's local slots (p1_amd/host/local_slots.hpp:
// server::LocalSlots, the thread-free core) over a real sched::Scheduler, with
// every piece answered by the CPU oracle.  No network, no threads.
//
//   local_slots_test [seed]
//
// One scenario = (--local-chunk in {1, 1000, 2^16}) x (slots in {1, 3, 64}) x
// (inflight in {1, 2, 4}) x (no failure | Submit of round k throws | Collect of
// round k throws).  In every scenario random events drive the server's pump by
// hand: clients submit ranges (lower > upper, 1 nonce, below one chunk, one
// chunk and a ragged rest, many chunks, ranges ending at 2^64-1; up to 3*10^5
// nonces), a round is cut when LocalSlots::Ready(), the oldest round is
// collected, clients go away -- by preference one whose piece is in a round
// that is out --, remote miners (positive ids, the scheduler's own, larger
// chunk) join, answer and vanish holding a chunk, which is then re-dealt with
// its own bounds, to a local slot too.  Checked on every step:
//   - a request completes at most once, never after its client left, and its
//     answer equals p1o_scan of its whole range (identity (MaxUint64, 0));
//   - no nonce of a request is out with two takers, and the backend never sees
//     a piece twice unless it was handed back;
//   - a slot never has two pieces out (queued, being submitted or in a round);
//   - a slot's piece holds at most --local-chunk nonces unless a lost remote
//     miner handed that very chunk back;
//   - a round holds at most one piece per slot and at most `inflight` are out;
//   - after a backend failure nothing is cut, every local chunk is back with
//     its request, and with a remote miner every live request still completes.
// Prints "local_slots_test: ok ..." and "all passed", or exits 1.
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>

#include <map>
#include <random>
#include <set>
#include <string>
#include <tuple>
#include <vector>

#include "../p1_amd/host/local_slots.hpp"
#include "../p1_amd/host/scheduler.hpp"

extern "C" int p1o_scan(const uint8_t* msg, size_t len, uint64_t lower, uint64_t upper, uint64_t* out_hash,
                        uint64_t* out_nonce);
extern "C" int p1o_scan_mt(const uint8_t* msg, size_t len, uint64_t lower, uint64_t upper, int nthreads,
                           uint64_t* out_hash, uint64_t* out_nonce);

namespace {

#define FAIL(...)                                 \
  do {                                            \
    fprintf(stderr, "local_slots_test: %s: ", g_what.c_str()); \
    fprintf(stderr, __VA_ARGS__);                 \
    fprintf(stderr, "\n");                        \
    exit(1);                                      \
  } while (0)

std::string g_what;

struct ReqInfo {
  int64_t client;
  std::string data;
  uint64_t lo, hi;
  bool done = false;
};
struct Chunk {
  uint64_t req, lo, hi;
  bool operator<(const Chunk& o) const { return std::tie(req, lo, hi) < std::tie(o.req, o.lo, o.hi); }
};

struct Totals {
  long scenarios = 0, requests = 0, rounds = 0, pieces = 0, handed_back = 0, failures = 0, cancelled_out = 0,
       big_local = 0, max_round = 0;
};

enum FailAt { kNoFail, kFailSubmit, kFailCollect };

void scenario(uint64_t seed, uint64_t chunk, int slots, size_t inflight, FailAt fail_at, uint64_t fail_round,
              bool remotes, Totals* tot) {
  char what[160];
  snprintf(what, sizeof what, "seed %" PRIu64 " chunk %" PRIu64 " slots %d inflight %zu fail %d@%" PRIu64 " remotes %d",
           seed, chunk, slots, inflight, (int)fail_at, fail_round, (int)remotes);
  g_what = what;
  std::mt19937_64 g(seed);
  auto rnd = [&](uint64_t n) { return (uint64_t)(g() % n); };

  const uint64_t remote_chunk = 4 * chunk + 7;  // a handed-back remote chunk exceeds a slot's
  sched::Scheduler S(remote_chunk);
  server::LocalSlots core(slots, chunk, inflight);
  core.Join(S);

  std::map<uint64_t, ReqInfo> reqs;
  std::set<int64_t> gone;
  std::map<Chunk, int> out_with;        // chunks out, and with whom
  std::map<int, Chunk> held;            // by taker (local slot < 0, remote miner > 0)
  std::multiset<Chunk> handed_back;     // given up by a lost taker, not re-dealt yet
  std::set<Chunk> backend_seen;
  std::set<int> remote_alive;
  // the backend: rounds by handle, answered at Collect
  std::map<uint64_t, std::vector<miner::Piece>> backend;
  uint64_t submits = 0, collects = 0, next_handle = 0;
  int next_remote = 1;
  int64_t next_client = 1000;
  int64_t budget = 150000;  // nonces the random requests may ask for (every one is hashed twice)
  bool cut_after_failure = false;

  auto give_back = [&](int taker) {
    auto it = held.find(taker);
    if (it == held.end()) return;
    out_with.erase(it->second);
    if (reqs.count(it->second.req) && !gone.count(reqs[it->second.req].client)) {
      handed_back.insert(it->second);
      ++tot->handed_back;
    }
    held.erase(it);
  };
  auto fail_backend = [&] {
    core.Fail(S);
    for (int k = 1; k <= slots; ++k) {
      give_back(-k);
      if (S.IsMiner(-k)) FAIL("slot %d still a miner after the failure", -k);
    }
    backend.clear();
    ++tot->failures;
  };
  auto pump = [&] {
    for (const sched::Assignment& a : S.Dispatch()) {
      auto it = reqs.find(a.req);
      if (it == reqs.end()) FAIL("assignment for an unknown request");
      const ReqInfo& r = it->second;
      if (a.lo > a.hi || a.lo < r.lo || a.hi > r.hi || a.data != r.data) FAIL("assignment outside its request");
      const Chunk c{a.req, a.lo, a.hi};
      for (const auto& kv : out_with)
        if (kv.first.req == a.req && !(a.hi < kv.first.lo || kv.first.hi < a.lo))
          FAIL("request %" PRIu64 ": [%" PRIu64 ", %" PRIu64 "] is out twice", a.req, a.lo, a.hi);
      if (held.count(a.miner)) FAIL("taker %d given a second chunk", a.miner);
      auto hb = handed_back.find(c);
      const bool was_back = hb != handed_back.end();
      if (was_back) handed_back.erase(hb);
      const uint64_t limit = server::LocalSlots::IsLocal(a.miner) ? chunk : remote_chunk;
      if (a.hi - a.lo >= limit && !was_back)
        FAIL("taker %d: [%" PRIu64 ", %" PRIu64 "] exceeds its chunk %" PRIu64, a.miner, a.lo, a.hi, limit);
      out_with[c] = a.miner;
      held[a.miner] = c;
      if (server::LocalSlots::IsLocal(a.miner)) {
        if (core.Failed()) FAIL("a lost slot was dealt a chunk");
        if (a.miner < -slots) FAIL("slot id %d out of range", a.miner);
        if (a.hi - a.lo >= chunk) ++tot->big_local;
        core.Queue(a);
      }
    }
    for (const sched::Done& d : S.TakeDone()) {
      auto it = reqs.find(d.req);
      if (it == reqs.end()) FAIL("unknown request completed");
      ReqInfo& r = it->second;
      if (r.done) FAIL("request %" PRIu64 " completed twice", d.req);
      if (gone.count(r.client)) FAIL("request %" PRIu64 " completed after its client left", d.req);
      if (d.client != r.client) FAIL("request %" PRIu64 " answered to the wrong client", d.req);
      uint64_t h = UINT64_MAX, n = 0;
      if (r.lo <= r.hi) p1o_scan_mt((const uint8_t*)r.data.data(), r.data.size(), r.lo, r.hi, 4, &h, &n);
      if (d.hash != h || d.nonce != n)
        FAIL("request %" PRIu64 " [%" PRIu64 ", %" PRIu64 "]: got (%" PRIu64 ", %" PRIu64 ") want (%" PRIu64
             ", %" PRIu64 ")", d.req, r.lo, r.hi, d.hash, d.nonce, h, n);
      r.done = true;
      ++tot->requests;
    }
    if (core.Outstanding() > inflight) FAIL("%zu rounds out", core.Outstanding());
  };
  auto cut = [&] {
    if (core.Failed()) cut_after_failure = cut_after_failure || core.Ready();
    if (!core.Ready()) return;
    const std::vector<miner::Piece> pieces = core.Cut();  // a copy, as the round thread takes
    if (pieces.empty() || pieces.size() > (size_t)slots) FAIL("a round of %zu pieces", pieces.size());
    if (core.Ready()) FAIL("Ready while a round is being submitted");
    std::set<int> in_round;
    for (const miner::Piece& p : pieces) {
      if (!in_round.insert(p.conn).second) FAIL("slot %d twice in a round", p.conn);
      auto h = held.find(p.conn);
      if (h == held.end() || h->second.lo != p.lower || h->second.hi != p.upper || h->second.req != p.job)
        FAIL("slot %d: the piece is not its chunk", p.conn);
      if (reqs[p.job].data != p.msg) FAIL("slot %d: wrong message", p.conn);
      if (!backend_seen.insert({p.job, p.lower, p.upper}).second) FAIL("the backend sees a piece twice");
    }
    ++submits;
    if (fail_at == kFailSubmit && submits == fail_round) {
      fail_backend();
      return;
    }
    backend[++next_handle] = pieces;
    core.Sent(next_handle);
    ++tot->rounds;
    tot->pieces += (long)pieces.size();
    if ((long)pieces.size() > tot->max_round) tot->max_round = (long)pieces.size();
  };
  auto collect = [&] {
    if (!core.HasOut()) return;
    const uint64_t index = core.Oldest().index, handle = core.Oldest().handle;
    ++collects;
    if (fail_at == kFailCollect && collects == fail_round) {
      fail_backend();
      return;
    }
    const std::vector<miner::Piece>& pieces = backend[handle];
    if (pieces.size() != core.Oldest().pieces.size()) FAIL("round %" PRIu64 " is not what was submitted", index);
    std::vector<miner::PieceResult> res(pieces.size());
    for (size_t i = 0; i < pieces.size(); ++i) {
      const miner::Piece& p = pieces[i];
      p1o_scan((const uint8_t*)p.msg.data(), p.msg.size(), p.lower, p.upper, &res[i].hash, &res[i].nonce);
      auto h = held.find(p.conn);
      if (h == held.end()) FAIL("slot %d answers a piece it does not hold", p.conn);
      out_with.erase(h->second);
      held.erase(h);
    }
    if (!core.Collected(S, index, res)) FAIL("round %" PRIu64 " refused", index);
    backend.erase(handle);
  };
  auto remote_report = [&](int m) {
    auto h = held.find(m);
    if (h == held.end()) return;
    const Chunk c = h->second;
    uint64_t hash = UINT64_MAX, nonce = 0;
    const std::string& d = reqs[c.req].data;
    p1o_scan_mt((const uint8_t*)d.data(), d.size(), c.lo, c.hi, 4, &hash, &nonce);
    out_with.erase(c);
    held.erase(h);
    if (!S.Result(m, hash, nonce)) FAIL("a remote miner's Result refused");
  };
  auto submit = [&] {
    ReqInfo r;
    r.client = rnd(4) == 0 && !reqs.empty() ? reqs.rbegin()->second.client : next_client++;
    if (gone.count(r.client)) r.client = next_client++;
    static const size_t lens[] = {0, 1, 8, 54, 55, 63, 64, 119, 120};
    r.data = std::string(lens[rnd(9)], (char)('a' + rnd(26)));
    for (char& ch : r.data) ch = (char)('a' + rnd(26));
    const uint64_t many = chunk * 300 < 300000 ? chunk * 300 : 300000;
    uint64_t span;  // nonces - 1
    const uint64_t kind = rnd(12);
    if (kind == 0) {  // lower > upper
      r.lo = 100 + rnd(1000);
      r.hi = r.lo - 1 - rnd(50);
      reqs[S.Submit(r.client, r.data, r.lo, r.hi)] = r;
      return;
    }
    if (kind == 1) span = 0;                               // one nonce
    else if (kind <= 4) span = rnd(chunk);                 // one piece
    else if (kind <= 7) span = chunk + rnd(chunk);         // two pieces, the last ragged or whole
    else span = rnd(many);                                 // many pieces
    if ((int64_t)span + 1 > budget) span = budget > 0 ? (uint64_t)budget - 1 : 0;
    budget -= (int64_t)span + 1;
    if (rnd(8) == 0) { r.hi = UINT64_MAX; r.lo = UINT64_MAX - span; }  // the u64 top
    else { r.lo = rnd(1ull << 40); r.hi = r.lo + span; }
    reqs[S.Submit(r.client, r.data, r.lo, r.hi)] = r;
  };
  auto cancel = [&] {
    // a client whose piece is in a round that is out, if there is one
    int64_t c = -1;
    bool in_out_round = false;
    for (const auto& kv : backend)
      for (const miner::Piece& p : kv.second)
        if (c < 0 && reqs.count(p.job) && !reqs[p.job].done && !gone.count(reqs[p.job].client)) {
          c = reqs[p.job].client;
          in_out_round = true;
        }
    if (c < 0 || rnd(3) == 0) {
      in_out_round = false;
      if (reqs.empty()) return;
      auto it = reqs.begin();
      std::advance(it, rnd(reqs.size()));
      if (it->second.done || gone.count(it->second.client)) return;
      c = it->second.client;
    }
    S.CancelClient(c);
    gone.insert(c);
    if (in_out_round) ++tot->cancelled_out;
    for (auto it = handed_back.begin(); it != handed_back.end();)
      it = gone.count(reqs[it->req].client) ? handed_back.erase(it) : std::next(it);
  };

  // the largest request first in some scenarios, so that 3*10^5 nonces are really asked for
  if (chunk >= 1000 && seed % 7 == 0) {
    ReqInfo r;
    r.client = next_client++;
    r.data = "bradfitz";
    r.lo = 0;
    r.hi = 299999;
    reqs[S.Submit(r.client, r.data, r.lo, r.hi)] = r;
  }
  const int steps = 400;
  for (int step = 0; step < steps; ++step) {
    const uint64_t ev = rnd(100);
    if (ev < 22) submit();
    else if (ev < 50) cut();
    else if (ev < 80) collect();
    else if (ev < 84) cancel();
    else if (ev < 89) {
      if (remotes && remote_alive.size() < 2) {
        const int m = next_remote++;
        S.AddMiner(m);
        remote_alive.insert(m);
      }
    } else if (ev < 96) {
      if (!remote_alive.empty()) {
        auto it = remote_alive.begin();
        std::advance(it, rnd(remote_alive.size()));
        remote_report(*it);
      }
    } else if (!remote_alive.empty()) {  // a remote miner vanishes, maybe holding a chunk
      auto it = remote_alive.begin();
      std::advance(it, rnd(remote_alive.size()));
      const int m = *it;
      S.LoseMiner(m);
      give_back(m);
      remote_alive.erase(it);
    }
    pump();
  }
  // drain: the local slots if they live, and one remote miner that never fails
  // if they do not (or if the scenario has remote miners anyway)
  if (core.Failed() || remotes) {
    const int m = next_remote++;
    S.AddMiner(m);
    remote_alive.insert(m);
  }
  for (int guard = 0; !S.Idle(); ++guard) {
    if (guard > 2000000) FAIL("the drain does not end");
    pump();
    cut();
    pump();
    collect();
    pump();
    for (int m : std::set<int>(remote_alive)) remote_report(m);
    pump();
  }
  while (core.HasOut()) collect();  // rounds of departed clients only
  pump();
  if (cut_after_failure) FAIL("Ready() after the failure");
  for (const auto& kv : reqs)
    if (!kv.second.done && !gone.count(kv.second.client))
      FAIL("request %" PRIu64 " never completed", kv.first);
  if (!handed_back.empty()) FAIL("%zu handed-back chunks never re-dealt", handed_back.size());
  const server::LocalStats& st = core.Stats();
  if (st.max_outstanding > inflight || st.max_round > (uint64_t)slots) FAIL("stats out of bounds");
  if (fail_at != kNoFail && !core.Failed() && st.rounds >= fail_round + inflight) FAIL("the failure never happened");
  ++tot->scenarios;
}

}  // namespace

int main(int argc, char** argv) {
  const uint64_t seed0 = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
  Totals tot;
  uint64_t seed = seed0;
  const uint64_t chunks[] = {1, 1000, 1ull << 16};
  const int slots[] = {1, 3, 64};
  const size_t inflights[] = {1, 2, 4};
  for (uint64_t chunk : chunks)
    for (int s : slots)
      for (size_t n : inflights) {
        scenario(seed, chunk, s, n, kNoFail, 0, false, &tot);
        scenario(seed + 1, chunk, s, n, kNoFail, 0, true, &tot);
        scenario(seed + 2, chunk, s, n, kFailSubmit, 1 + seed % 5, true, &tot);
        scenario(seed + 3, chunk, s, n, kFailCollect, 1 + seed % 5, true, &tot);
        scenario(seed + 4, chunk, s, n, seed % 2 ? kFailSubmit : kFailCollect, 2, false, &tot);
        seed += 5;
      }
  printf("local_slots_test: ok scenarios %ld requests %ld rounds %ld pieces %ld max_round %ld handed_back %ld "
         "failures %ld cancelled_in_an_out_round %ld pieces_above_the_local_chunk %ld\n",
         tot.scenarios, tot.requests, tot.rounds, tot.pieces, tot.max_round, tot.handed_back, tot.failures,
         tot.cancelled_out, tot.big_local);
  if (tot.requests < 1000 || tot.failures < 20 || tot.handed_back < 20 || tot.cancelled_out < 10 ||
      tot.big_local < 1 || tot.max_round < 8) {
    fprintf(stderr, "local_slots_test: the scenarios did not reach what they are there for\n");
    return 1;
  }
  printf("all passed\n");
  return 0;
}
