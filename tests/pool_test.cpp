// pool_test.cpp -- unit tests of miner::Rounds (p1_amd/host/miner_pool.hpp:
// the multi-connection miner's jobs cut into rounds and folded back), run by
// tests/test_pool_host.py::test_rounds_unit.  No LSP, no oracle, no GPU: the
// backends are small deterministic functions of the nonce, and every job's
// Result must equal the direct left-to-right scan of its range (what
// miner::HandleRequest computes, miner.go:56-63).  Exit status 0 = all passed.
#include <stdio.h>
#include <stdlib.h>

#include <map>
#include <set>
#include <string>
#include <vector>

#include "../p1_amd/host/miner_pool.hpp"

#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c); \
      exit(1);                                                     \
    }                                                              \
  } while (0)

// The hash functions, chosen by the job's message:
//   "ties"     (n * 2654435761) % 7: many equal minima, the first must win
//   "max"      MaxUint64 everywhere: the job answers nonce 0
//   "edge:E"   a unique minimum at nonce E (the tests put E on a piece edge)
static uint64_t hash_of(const std::string& msg, uint64_t n) {
  if (msg == "max") return UINT64_MAX;
  if (msg.compare(0, 5, "edge:") == 0) return n == strtoull(msg.c_str() + 5, nullptr, 10) ? 1 : 1000 + n % 13;
  return (n * 2654435761ull) % 7;
}

// miner.go:56-63 over [lower, upper], the way p1hip_scan answers it: the
// first minimum; nonce 0 if no hash is below MaxUint64; no wrap at 2^64-1.
static miner::PieceResult direct(const std::string& msg, uint64_t lower, uint64_t upper) {
  miner::PieceResult r;
  bool found = false;
  if (lower > upper) return r;
  for (uint64_t n = lower;; ++n) {
    const uint64_t h = hash_of(msg, n);
    if (h < r.hash) { r.hash = h; r.nonce = n; found = true; }
    if (n == upper) break;
  }
  if (!found) r.nonce = 0;
  return r;
}

static std::vector<miner::PieceResult> backend(const std::vector<miner::Piece>& pieces) {
  std::vector<miner::PieceResult> out;
  for (const miner::Piece& p : pieces) out.push_back(direct(p.msg, p.lower, p.upper));
  return out;
}

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
  // nonces - 1: mostly a few pieces' worth, capped so that the direct scan stays cheap
  const uint64_t span = below(4) == 0 ? below(chunk < 600 ? 3 * chunk + 2 : 2000) : below(400);
  switch (below(8)) {
    case 0: r.upper = UINT64_MAX; r.lower = UINT64_MAX - span; break;  // ends at 2^64-1
    case 1: r.lower = 5 + below(100); r.upper = r.lower - 1 - below(5); break;  // lower > upper
    default: r.lower = below(1000000); r.upper = r.lower + span; break;
  }
  switch (below(4)) {
    case 0: r.msg = "max"; break;
    case 1: {  // the unique minimum on a piece edge: the last nonce of a piece or the first of the next
      uint64_t e = r.lower;
      if (r.lower <= r.upper) {
        const uint64_t pieces = (r.upper - r.lower) / chunk + 1;
        e = r.lower + below(pieces) * chunk;  // a piece's first nonce
        if (below(2) && e > r.lower) --e;     // or the last one of the piece before
      }
      r.msg = "edge:" + std::to_string(e);
      break;
    }
    default: r.msg = "ties"; break;
  }
  return r;
}

// One random scenario: `nconn` connections with 1..3 Requests each, arriving
// in random order between rounds (a second Request may arrive while the
// first is active: it is queued and answered in order); one connection may be
// dropped in mid-job.  Checks every round's shape and every Result.
static void scenario(uint64_t chunk, int nconn) {
  miner::Rounds R;
  std::vector<std::vector<Req>> plan(nconn);
  std::vector<size_t> pushed(nconn, 0), answered(nconn, 0);
  std::vector<bool> dropped(nconn, false);
  std::map<int, uint64_t> expect_lower;  // the next piece of a connection's active job starts here
  size_t to_push = 0;
  for (int c = 0; c < nconn; ++c) {
    const int n = 1 + (int)below(3);
    for (int k = 0; k < n; ++k) plan[c].push_back(random_req(chunk));
    to_push += n;
  }
  const int drop_conn = below(3) == 0 ? (int)below(nconn) : -1;
  const uint64_t drop_round = below(4);

  auto take = [&](const std::vector<miner::Done>& done) {
    for (const miner::Done& d : done) {
      CHECK(d.conn >= 0 && d.conn < nconn && !dropped[d.conn]);
      CHECK(answered[d.conn] < pushed[d.conn]);  // in order: the oldest unanswered Request
      const Req& q = plan[d.conn][answered[d.conn]];
      const miner::PieceResult want = direct(q.msg, q.lower, q.upper);
      CHECK(d.hash == want.hash && d.nonce == want.nonce);
      ++answered[d.conn];
      expect_lower.erase(d.conn);
    }
  };

  uint64_t round = 0;
  for (;;) {
    // arrivals: a random number of Requests on random connections
    for (uint64_t k = below(nconn + 1); k > 0 && to_push > 0; --k) {
      const int c = (int)below(nconn);
      if (dropped[c] || pushed[c] == plan[c].size()) continue;
      R.Push(c, request(plan[c][pushed[c]++]));
      --to_push;
      take(R.TakeDone());  // an empty job on an idle connection is finished at once
    }
    std::vector<miner::Piece> pieces = R.Next(chunk);
    // exactly one piece for each connection with an active job, none else
    std::set<int> seen;
    for (const miner::Piece& p : pieces) {
      CHECK(seen.insert(p.conn).second);
      CHECK(!dropped[p.conn] && answered[p.conn] < pushed[p.conn]);
      const Req& q = plan[p.conn][answered[p.conn]];
      CHECK(p.msg == q.msg);
      const uint64_t lo = expect_lower.count(p.conn) ? expect_lower[p.conn] : q.lower;
      CHECK(p.lower == lo && p.lower <= p.upper && p.upper <= q.upper);  // in nonce order, no wrap
      CHECK(p.upper - p.lower <= chunk - 1);
      CHECK(p.upper == q.upper || p.upper - p.lower == chunk - 1);  // only a job's last piece is short
      if (p.upper != q.upper) expect_lower[p.conn] = p.upper + 1;
    }
    size_t active = 0;
    for (int c = 0; c < nconn; ++c) active += !dropped[c] && answered[c] < pushed[c];
    CHECK(pieces.size() == active && R.Active() == active);
    if (drop_conn >= 0 && !dropped[drop_conn] && round >= drop_round && seen.count(drop_conn)) {
      R.Drop(drop_conn);  // its piece is in flight: the result must be ignored
      dropped[drop_conn] = true;
      to_push -= plan[drop_conn].size() - pushed[drop_conn];
      expect_lower.erase(drop_conn);
    }
    take(R.Finish(pieces, backend(pieces)));
    ++round;
    bool open = to_push > 0;
    for (int c = 0; c < nconn; ++c) open = open || (!dropped[c] && answered[c] < pushed[c]);
    if (!open) break;
    CHECK(round < 1000000);
  }
  CHECK(R.Active() == 0 && R.Next(chunk).empty() && R.TakeDone().empty());
  for (int c = 0; c < nconn; ++c) CHECK(dropped[c] || answered[c] == plan[c].size());
}

static void random_scenarios() {
  const uint64_t chunks[] = {1, 2, 7, 64, 100, 1000, 1ull << 36};
  for (int i = 0; i < 4000; ++i) scenario(chunks[below(7)], 1 + (int)below(8));
}

static void full_range_end_does_not_wrap() {
  miner::Rounds R;
  R.Push(3, request({"ties", UINT64_MAX - 9, UINT64_MAX}));
  std::vector<miner::Piece> p = R.Next(4);
  CHECK(p.size() == 1 && p[0].conn == 3 && p[0].lower == UINT64_MAX - 9 && p[0].upper == UINT64_MAX - 6);
  CHECK(R.Finish(p, backend(p)).empty());
  p = R.Next(4);
  CHECK(p.size() == 1 && p[0].lower == UINT64_MAX - 5 && p[0].upper == UINT64_MAX - 2);
  CHECK(R.Finish(p, backend(p)).empty());
  p = R.Next(4);
  CHECK(p.size() == 1 && p[0].lower == UINT64_MAX - 1 && p[0].upper == UINT64_MAX);
  std::vector<miner::Done> d = R.Finish(p, backend(p));
  const miner::PieceResult want = direct("ties", UINT64_MAX - 9, UINT64_MAX);
  CHECK(d.size() == 1 && d[0].conn == 3 && d[0].hash == want.hash && d[0].nonce == want.nonce);
  CHECK(R.Next(4).empty());
  // the whole of uint64 in one piece; chunk 0 means the default chunk
  R.Push(1, request({"max", 0, UINT64_MAX}));
  p = R.Next(0);
  CHECK(p.size() == 1 && p[0].lower == 0 && p[0].upper == miner::kDefaultChunk - 1);
}

static void empty_and_queued_jobs_are_answered_in_order() {
  miner::Rounds R;
  R.Push(0, request({"ties", 9, 3}));  // lower > upper: at once, no piece
  std::vector<miner::Done> d = R.TakeDone();
  CHECK(d.size() == 1 && d[0].conn == 0 && d[0].hash == UINT64_MAX && d[0].nonce == 0);
  CHECK(R.Next(10).empty() && R.Active() == 0);
  R.Push(0, request({"ties", 0, 14}));  // active
  R.Push(0, request({"ties", 9, 3}));   // queued behind it: not answered before it
  R.Push(0, request({"max", 20, 22}));  // queued third
  CHECK(!R.HasDone() && R.Active() == 1);
  std::vector<miner::Piece> p = R.Next(10);
  CHECK(p.size() == 1 && p[0].lower == 0 && p[0].upper == 9);
  CHECK(R.Next(10).empty());  // its piece is in flight: no second one
  CHECK(R.Finish(p, backend(p)).empty());
  p = R.Next(10);
  CHECK(p.size() == 1 && p[0].lower == 10 && p[0].upper == 14);
  d = R.Finish(p, backend(p));
  const miner::PieceResult want = direct("ties", 0, 14);
  CHECK(d.size() == 2 && d[0].hash == want.hash && d[0].nonce == want.nonce);
  CHECK(d[1].conn == 0 && d[1].hash == UINT64_MAX && d[1].nonce == 0);
  p = R.Next(10);
  CHECK(p.size() == 1 && p[0].msg == "max" && p[0].lower == 20 && p[0].upper == 22);
  d = R.Finish(p, backend(p));
  CHECK(d.size() == 1 && d[0].hash == UINT64_MAX && d[0].nonce == 0);  // never below MaxUint64: nonce 0
}

static void first_minimum_wins_across_pieces() {
  miner::Rounds R;
  R.Push(5, request({"x", 0, 29}));
  const uint64_t hashes[3] = {70, 40, 40}, nonces[3] = {3, 17, 22};
  std::vector<miner::Done> d;
  for (int i = 0; i < 3; ++i) {
    std::vector<miner::Piece> p = R.Next(10);
    CHECK(p.size() == 1);
    miner::PieceResult r;
    r.hash = hashes[i];
    r.nonce = nonces[i];
    d = R.Finish(p, {r});
  }
  CHECK(d.size() == 1 && d[0].conn == 5 && d[0].hash == 40 && d[0].nonce == 17);
}

static void short_job_waits_one_round_behind_a_long_one() {
  miner::Rounds R;
  R.Push(0, request({"ties", 0, 49999}));  // 50 pieces of 1000
  for (int i = 0; i < 3; ++i) {
    std::vector<miner::Piece> p = R.Next(1000);
    CHECK(p.size() == 1 && p[0].conn == 0);
    CHECK(R.Finish(p, backend(p)).empty());
  }
  R.Push(1, request({"ties", 0, 999}));
  std::vector<miner::Piece> p = R.Next(1000);  // the very next round holds both
  CHECK(p.size() == 2 && p[0].conn == 0 && p[0].lower == 3000 && p[1].conn == 1 && p[1].upper == 999);
  std::vector<miner::Done> d = R.Finish(p, backend(p));
  const miner::PieceResult want = direct("ties", 0, 999);
  CHECK(d.size() == 1 && d[0].conn == 1 && d[0].hash == want.hash && d[0].nonce == want.nonce);
  int rounds = 4;
  for (;; ++rounds) {
    p = R.Next(1000);
    CHECK(p.size() == 1);
    d = R.Finish(p, backend(p));
    if (!d.empty()) break;
  }
  CHECK(rounds + 1 == 50);
  const miner::PieceResult all = direct("ties", 0, 49999);
  CHECK(d.size() == 1 && d[0].conn == 0 && d[0].hash == all.hash && d[0].nonce == all.nonce);
}

static void drop_in_mid_job() {
  miner::Rounds R;
  R.Push(0, request({"ties", 0, 99}));
  R.Push(1, request({"ties", 0, 99}));
  R.Push(1, request({"ties", 7, 2}));  // queued on the connection that goes
  std::vector<miner::Piece> p = R.Next(50);
  CHECK(p.size() == 2);
  R.Drop(1);
  CHECK(R.Active() == 1);
  CHECK(R.Finish(p, backend(p)).empty());  // conn 1's result is ignored, conn 0 is half way
  p = R.Next(50);
  CHECK(p.size() == 1 && p[0].conn == 0 && p[0].lower == 50);
  // a new job on the same connection number is not confused with the old piece
  R.Push(1, request({"max", 0, 9}));
  std::vector<miner::Piece> stale(1);
  stale[0].conn = 1;
  stale[0].job = 2;
  stale[0].upper = 9;
  CHECK(R.Finish(stale, backend(stale)).empty());
  std::vector<miner::Done> d = R.Finish(p, backend(p));
  CHECK(d.size() == 1 && d[0].conn == 0);
  p = R.Next(50);
  CHECK(p.size() == 1 && p[0].conn == 1 && p[0].msg == "max");
  // an empty job waiting to be written is forgotten with its connection
  R.Push(2, request({"ties", 7, 2}));
  CHECK(R.HasDone());
  R.Drop(2);
  CHECK(!R.HasDone());
}

int main() {
  full_range_end_does_not_wrap();
  empty_and_queued_jobs_are_answered_in_order();
  first_minimum_wins_across_pieces();
  short_job_waits_one_round_behind_a_long_one();
  drop_in_mid_job();
  random_scenarios();
  printf("pool_test: all passed\n");
  return 0;
}
