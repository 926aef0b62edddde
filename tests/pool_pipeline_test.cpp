// pool_pipeline_test.cpp -- unit tests of miner::Pipeline over miner::Rounds
// (p1_amd/host/miner_pool.hpp: up to `depth` rounds outstanding), run by
// tests/test_pool_pipeline_host.py::test_pipeline_unit.  No LSP, no GPU, no
// threads: the backend keeps every submitted round until the pipeline collects
// it -- the test decides what arrives, and what is dropped, between a round's
// Submit and its Collect -- and answers it with the CPU oracle
// (oracle/libp1oracle.so).  Every job's Result must equal the oracle's direct
// scan of its whole range (what miner::HandleRequest computes,
// miner.go:56-63).  Exit status 0 = all passed.
#include <stdio.h>
#include <stdlib.h>

#include <deque>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "../p1_amd/host/miner_pool.hpp"

extern "C" int p1o_scan(const uint8_t* msg, size_t len, uint64_t lower, uint64_t upper, uint64_t* out_hash,
                        uint64_t* out_nonce);

#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c); \
      exit(1);                                                     \
    }                                                              \
  } while (0)

// miner.go:56-63 over [lower, upper] by the oracle: (MaxUint64, 0) for an empty range
static miner::PieceResult direct(const std::string& msg, uint64_t lower, uint64_t upper) {
  miner::PieceResult r;
  if (lower <= upper) CHECK(p1o_scan((const uint8_t*)msg.data(), msg.size(), lower, upper, &r.hash, &r.nonce) == 0);
  return r;
}

// Keeps a round from Submit to Collect.  Collect must come in Submit's order.
struct GatedBackend {
  std::deque<std::pair<uint64_t, std::vector<miner::Piece>>> out;
  uint64_t next_handle = 100;
  std::vector<std::vector<miner::Piece>> log;  // every round, in submit order
  size_t max_out = 0;
  uint64_t Submit(const std::vector<miner::Piece>& pieces) {
    CHECK(!pieces.empty());
    // no job ever has two pieces outstanding
    for (const auto& o : out)
      for (const miner::Piece& a : o.second)
        for (const miner::Piece& b : pieces) CHECK(a.job != b.job);
    out.push_back({next_handle, pieces});
    log.push_back(pieces);
    if (out.size() > max_out) max_out = out.size();
    return next_handle++;
  }
  void Collect(uint64_t handle, std::vector<miner::PieceResult>* res) {
    CHECK(!out.empty() && out.front().first == handle);
    CHECK(res->size() == out.front().second.size());
    for (size_t i = 0; i < res->size(); ++i) {
      const miner::Piece& p = out.front().second[i];
      (*res)[i] = direct(p.msg, p.lower, p.upper);
    }
    out.pop_front();
  }
};

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return rng_state * 2685821657736338717ull;
}
static uint64_t below(uint64_t n) { return rnd() % n; }

struct Req {
  std::string msg;
  uint64_t lower, upper;
};

static bitcoin::Message request(const Req& r) {
  bitcoin::Message m;
  m.Type = bitcoin::Request;
  m.Data = r.msg;
  m.Lower = r.lower;
  m.Upper = r.upper;
  return m;
}

static Req random_req(uint64_t chunk) {
  Req r;
  const uint64_t span = below(4) == 0 ? below(chunk < 300 ? 3 * chunk + 2 : 900) : below(200);
  switch (below(8)) {
    case 0: r.upper = UINT64_MAX; r.lower = UINT64_MAX - span; break;            // ends at 2^64-1
    case 1: r.lower = 5 + below(100); r.upper = r.lower - 1 - below(5); break;  // lower > upper
    default: r.lower = below(1000000); r.upper = r.lower + span; break;
  }
  // a few messages only, so that equal jobs (ties between connections) occur
  r.msg = "pipeline " + std::to_string(below(3));
  return r;
}

// One random scenario at `depth`: connections with 1..3 Requests each arriving
// at random between steps (queued behind an active job, or while its piece is
// out); one connection may be dropped while it has a piece out -- at depth >=
// 2 when two rounds are out.  Every Done is checked against the oracle.
static void scenario(uint64_t chunk, int nconn, size_t depth) {
  miner::Rounds R;
  miner::Pipeline P(depth);
  GatedBackend B;
  std::vector<std::vector<Req>> plan(nconn);
  std::vector<size_t> pushed(nconn, 0), answered(nconn, 0);
  std::vector<bool> dropped(nconn, false);
  size_t to_push = 0;
  for (int c = 0; c < nconn; ++c) {
    const int n = 1 + (int)below(3);
    for (int k = 0; k < n; ++k) plan[c].push_back(random_req(chunk));
    to_push += n;
  }
  int drop_conn = below(3) == 0 ? (int)below(nconn) : -1;
  auto take = [&](const std::vector<miner::Done>& done) {
    for (const miner::Done& d : done) {
      CHECK(d.conn >= 0 && d.conn < nconn && !dropped[d.conn]);
      CHECK(answered[d.conn] < pushed[d.conn]);  // in order: the oldest unanswered Request
      const Req& q = plan[d.conn][answered[d.conn]];
      const miner::PieceResult want = direct(q.msg, q.lower, q.upper);
      CHECK(d.hash == want.hash && d.nonce == want.nonce);
      ++answered[d.conn];
    }
  };
  for (uint64_t step = 0;; ++step) {
    for (uint64_t k = below(nconn + 1); k > 0 && to_push > 0; --k) {
      const int c = (int)below(nconn);
      if (dropped[c] || pushed[c] == plan[c].size()) continue;
      R.Push(c, request(plan[c][pushed[c]++]));
      --to_push;
    }
    take(R.TakeDone());
    if (drop_conn >= 0 && !dropped[drop_conn] && B.out.size() >= (depth >= 2 ? 2u : 1u)) {
      bool has_piece = false;
      for (const auto& o : B.out)
        for (const miner::Piece& p : o.second) has_piece = has_piece || p.conn == drop_conn;
      if (has_piece) {  // its piece is out: the result must be ignored
        R.Drop(drop_conn);
        dropped[drop_conn] = true;
        to_push -= plan[drop_conn].size() - pushed[drop_conn];
      }
    }
    std::vector<miner::Done> done;
    const size_t out_before = P.Outstanding();
    const miner::Pipeline::Action a = P.Step(R, B, chunk, &done);
    CHECK(P.Outstanding() == B.out.size() && P.Outstanding() <= depth);
    if (a == miner::Pipeline::kSubmitted) {
      CHECK(out_before < depth && P.Outstanding() == out_before + 1);
      for (const miner::Piece& p : B.log.back()) {
        CHECK(p.lower <= p.upper && p.upper - p.lower <= chunk - 1);  // no wrap at 2^64-1
        CHECK(!dropped[p.conn]);
      }
    } else if (a == miner::Pipeline::kCollected) {
      CHECK(P.Outstanding() + 1 == out_before);
      take(done);
    } else {
      CHECK(out_before == 0 && done.empty());
    }
    bool open = to_push > 0 || P.Outstanding() > 0;
    for (int c = 0; c < nconn; ++c) open = open || (!dropped[c] && answered[c] < pushed[c]);
    if (!open) break;
    CHECK(step < 10000000);
  }
  CHECK(R.Active() == 0 && R.Next(chunk).empty() && R.TakeDone().empty() && B.out.empty());
  CHECK(P.MaxOutstanding() == B.max_out && P.Submitted() == B.log.size());
  for (int c = 0; c < nconn; ++c) CHECK(dropped[c] || answered[c] == plan[c].size());
}

static void random_scenarios() {
  const uint64_t chunks[] = {1, 2, 7, 64, 100, 1000, 1ull << 36};
  for (int i = 0; i < 1500; ++i) scenario(chunks[below(7)], 1 + (int)below(8), 1 + (size_t)below(4));
}

// Depth 1 is the synchronous loop: for the same arrivals, the rounds (piece
// for piece) and the finished jobs are those of Rounds::Next / Finish alone,
// which tests/pool_test.cpp pins down.
static void depth_one_is_the_synchronous_loop() {
  for (int i = 0; i < 300; ++i) {
    const uint64_t chunk = 1 + below(300);
    const int nconn = 1 + (int)below(8);
    std::vector<std::vector<std::pair<int, Req>>> arrivals;  // per round
    for (int r = 0, n = 2 + (int)below(6); r < n; ++r) {
      arrivals.emplace_back();
      for (uint64_t k = below(nconn + 1); k > 0; --k) arrivals.back().push_back({(int)below(nconn), random_req(chunk)});
    }
    auto run = [&](bool piped, std::vector<std::vector<miner::Piece>>* rounds, std::vector<miner::Done>* dones) {
      miner::Rounds R;
      miner::Pipeline P(1);
      GatedBackend B;
      for (size_t r = 0; r < arrivals.size() || R.Active() > 0; ++r) {
        if (r < arrivals.size())
          for (const auto& a : arrivals[r]) R.Push(a.first, request(a.second));
        std::vector<miner::Done> d = R.TakeDone();
        if (piped) {
          const miner::Pipeline::Action a = P.Step(R, B, chunk, &d);
          if (a == miner::Pipeline::kSubmitted) {
            CHECK(P.Outstanding() == 1);
            CHECK(P.Step(R, B, chunk, &d) == miner::Pipeline::kCollected);  // at depth: never a second submit
          } else {
            CHECK(a == miner::Pipeline::kIdle);
          }
        } else {
          const std::vector<miner::Piece> pieces = R.Next(chunk);
          if (!pieces.empty()) {
            std::vector<miner::PieceResult> res(pieces.size());
            B.Submit(pieces);
            B.Collect(B.out.front().first, &res);
            const std::vector<miner::Done> f = R.Finish(pieces, res);
            d.insert(d.end(), f.begin(), f.end());
          }
        }
        dones->insert(dones->end(), d.begin(), d.end());
        CHECK(r < 100000);
      }
      *rounds = B.log;
    };
    std::vector<std::vector<miner::Piece>> ra, rb;
    std::vector<miner::Done> da, db;
    run(false, &ra, &da);
    run(true, &rb, &db);
    CHECK(ra.size() == rb.size() && da.size() == db.size());
    for (size_t r = 0; r < ra.size(); ++r) {
      CHECK(ra[r].size() == rb[r].size());
      for (size_t j = 0; j < ra[r].size(); ++j)
        CHECK(ra[r][j].conn == rb[r][j].conn && ra[r][j].job == rb[r][j].job && ra[r][j].msg == rb[r][j].msg &&
              ra[r][j].lower == rb[r][j].lower && ra[r][j].upper == rb[r][j].upper);
    }
    for (size_t j = 0; j < da.size(); ++j)
      CHECK(da[j].conn == db[j].conn && da[j].hash == db[j].hash && da[j].nonce == db[j].nonce);
  }
}

// At depth 2 a second round goes out before the first comes back when
// another connection has a job; the job whose piece is out is not in it.
static void second_round_is_submitted_before_the_first_is_collected() {
  miner::Rounds R;
  miner::Pipeline P(2);
  GatedBackend B;
  std::vector<miner::Done> d;
  R.Push(0, request({"long", 0, 299}));  // 3 pieces of 100
  CHECK(P.Step(R, B, 100, &d) == miner::Pipeline::kSubmitted && P.Outstanding() == 1);
  R.Push(1, request({"short", 1000, 1049}));
  CHECK(P.Step(R, B, 100, &d) == miner::Pipeline::kSubmitted && P.Outstanding() == 2 && B.out.size() == 2);
  CHECK(B.log[1].size() == 1 && B.log[1][0].conn == 1);  // conn 0's piece is out: no second one
  R.Push(2, request({"third", 5, 9}));
  CHECK(P.Step(R, B, 100, &d) == miner::Pipeline::kCollected && d.empty());  // at depth: the oldest comes back
  // round 2: conn 0's next piece and conn 2 (conn 1's piece is still out)
  CHECK(P.Step(R, B, 100, &d) == miner::Pipeline::kSubmitted);
  CHECK(B.log[2].size() == 2 && B.log[2][0].conn == 0 && B.log[2][0].lower == 100 && B.log[2][1].conn == 2);
  CHECK(P.Step(R, B, 100, &d) == miner::Pipeline::kCollected);
  const miner::PieceResult s = direct("short", 1000, 1049);
  CHECK(d.size() == 1 && d[0].conn == 1 && d[0].hash == s.hash && d[0].nonce == s.nonce);
  while (P.Step(R, B, 100, &d) != miner::Pipeline::kIdle) {}
  const miner::PieceResult l = direct("long", 0, 299), t = direct("third", 5, 9);
  CHECK(d.size() == 3 && d[1].conn == 2 && d[1].hash == t.hash && d[1].nonce == t.nonce);
  CHECK(d[2].conn == 0 && d[2].hash == l.hash && d[2].nonce == l.nonce);
  CHECK(P.MaxOutstanding() == 2 && P.Submitted() == 4);
}

// Drop with the connection's pieces out in two rounds' time: both results are ignored.
static void drop_with_two_rounds_out() {
  miner::Rounds R;
  miner::Pipeline P(2);
  GatedBackend B;
  std::vector<miner::Done> d;
  R.Push(0, request({"a", 0, 99}));
  CHECK(P.Step(R, B, 50, &d) == miner::Pipeline::kSubmitted);
  R.Push(1, request({"b", 0, 99}));
  R.Push(1, request({"b", 9, 3}));  // queued behind it
  CHECK(P.Step(R, B, 50, &d) == miner::Pipeline::kSubmitted && P.Outstanding() == 2);
  R.Drop(0);
  R.Drop(1);
  R.Push(1, request({"c", 10, 19}));  // the same connection number again: not confused with the old piece
  CHECK(P.Step(R, B, 50, &d) == miner::Pipeline::kCollected && d.empty());
  CHECK(P.Step(R, B, 50, &d) == miner::Pipeline::kSubmitted && B.log[2].size() == 1 && B.log[2][0].msg == "c");
  CHECK(P.Step(R, B, 50, &d) == miner::Pipeline::kCollected && d.empty());
  CHECK(P.Step(R, B, 50, &d) == miner::Pipeline::kCollected);
  const miner::PieceResult c = direct("c", 10, 19);
  CHECK(d.size() == 1 && d[0].conn == 1 && d[0].hash == c.hash && d[0].nonce == c.nonce);
  CHECK(P.Step(R, B, 50, &d) == miner::Pipeline::kIdle);
  // Abandon forgets a round without folding it
  R.Push(4, request({"d", 0, 9}));
  CHECK(P.Step(R, B, 50, &d) == miner::Pipeline::kSubmitted);
  P.Abandon();
  CHECK(P.Outstanding() == 0);
}

int main() {
  second_round_is_submitted_before_the_first_is_collected();
  drop_with_two_rounds_out();
  depth_one_is_the_synchronous_loop();
  random_scenarios();
  printf("pool_pipeline_test: all passed\n");
  return 0;
}
