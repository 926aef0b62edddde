// async_slots_test.cpp -- p1::AsyncSlotsT (p1_amd/csrc/async_slots.hpp, the
// ticket bookkeeping of p1hip_batch_submit / p1hip_batch_wait) against a
// model: random sequences of allocate, claim, release and cancel-all.
//   - a ticket is never 0 and never equal to any ticket issued before it
//     (so never reused while live)
//   - Alloc gives 0 exactly when kSlots tickets are outstanding, and then
//     changes nothing
//   - stale tickets (released, cancelled, never issued) are refused by Holds,
//     Claim and Release; a second Claim and a second Release are refused
//   - two outstanding tickets never share a slot
// Usage: async_slots_test [seed [steps]]; prints "ok ..." and exits 0, or the
// first mismatch and exits 1.
#include <stdio.h>
#include <stdlib.h>

#include <map>
#include <random>
#include <set>
#include <vector>

#include "../p1_amd/csrc/async_slots.hpp"

namespace {

int g_fail = 0;
#define EXPECT(cond)                                             \
  do {                                                           \
    if (!(cond)) {                                               \
      if (!g_fail) fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
      g_fail = 1;                                                \
    }                                                            \
  } while (0)

template <int N>
void run(uint64_t seed, int steps) {
  p1::AsyncSlotsT<N> S;
  std::mt19937_64 rnd(seed);
  enum { kLive, kClaimed };
  std::map<uint64_t, int> model;  // outstanding ticket -> state
  std::set<uint64_t> ever;        // every ticket ever issued
  std::vector<uint64_t> stale;    // tickets that must be refused
  auto pick = [&](const std::vector<uint64_t>& v) { return v[rnd() % v.size()]; };
  auto outstanding = [&] {
    std::vector<uint64_t> v;
    for (auto& kv : model) v.push_back(kv.first);
    return v;
  };
  for (int step = 0; step < steps && !g_fail; ++step) {
    const int op = (int)(rnd() % 100);
    if (op < 40) {  // allocate
      const uint64_t t = S.Alloc();
      if ((int)model.size() == N) {
        EXPECT(t == 0);
      } else {
        EXPECT(t != 0);
        EXPECT(!ever.count(t));
        ever.insert(t);
        const int s = S.Holds(t);
        EXPECT(s >= 0 && s < N);
        for (auto& kv : model) EXPECT(S.Holds(kv.first) != s);
        model[t] = kLive;
      }
    } else if (op < 60 && !model.empty()) {  // claim
      const uint64_t t = pick(outstanding());
      const int s = S.Claim(t);
      if (model[t] == kLive) {
        EXPECT(s >= 0 && s == S.Holds(t));
        model[t] = kClaimed;
      } else {
        EXPECT(s == -1);  // claimed twice
      }
    } else if (op < 85 && !model.empty()) {  // release (live or claimed)
      const uint64_t t = pick(outstanding());
      EXPECT(S.Release(t));
      EXPECT(!S.Release(t));  // double release
      model.erase(t);
      stale.push_back(t);
    } else if (op < 88) {  // cancel all
      EXPECT(S.CancelAll() == (int)model.size());
      for (auto& kv : model) stale.push_back(kv.first);
      model.clear();
    } else if (!stale.empty()) {  // a stale or made-up ticket
      uint64_t t = pick(stale);
      if (op == 99) t = rnd();  // most likely never issued
      if (op == 98) t = 0;
      if (!model.count(t)) {
        EXPECT(S.Holds(t) == -1);
        EXPECT(S.Claim(t) == -1);
        EXPECT(!S.Release(t));
      }
    }
    EXPECT(S.Outstanding() == (int)model.size());
    for (auto& kv : model) EXPECT(S.Holds(kv.first) >= 0);
  }
}

}  // namespace

int main(int argc, char** argv) {
  const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
  const int steps = argc > 2 ? atoi(argv[2]) : 200000;
  run<1>(seed, steps / 4);
  run<2>(seed + 1, steps / 4);
  run<4>(seed + 2, steps);
  run<255>(seed + 3, steps / 16);
  if (g_fail) return 1;
  printf("ok async_slots seed=%llu steps=%d\n", (unsigned long long)seed, steps);
  return 0;
}
