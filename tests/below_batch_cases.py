"""Request lists and the oracle side of the p1hip_scan_below_batch tests, shared
by the CPU replay (tests/test_below_batch_host.py, through `batch_emu below`)
and the GPU tests (tests/test_gpu_below_batch.py, through
p1_amd.scan_below_batch), the way below_cases.py is shared.

A request is (msg, lower, upper, target, cap); its expected answer is the
reference loop, brute force by the oracle (below_cases.Expect), cut at cap."""
import batch_cases
from below_cases import U64_MAX, Expect

_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def matrix(oracle, n=150, seed=29):
    """-> (requests, expected): batch_cases.random_requests (message lengths
    0..129, every digit count, decade straddles, the top of u64, [0, 0] of the
    empty message, an empty range); request i's target is taken from its own
    data (the 1st, 3rd or 8th smallest hash of its range), or is 0 or
    UINT64_MAX; its cap is 0, 1, 3, exactly its hit count, or above it.  Every
    target kind meets every cap kind."""
    def make():
        reqs, want = [], []
        for i, (m, lo, hi) in enumerate(batch_cases.random_requests(n, seed)):
            if lo > hi:
                reqs.append((m, lo, hi, U64_MAX, 3))
                want.append([])
                continue
            E = Expect(oracle, m, lo, hi)
            target = (E.nth(0), E.nth(2), E.nth(7), 0, U64_MAX)[i % 5]
            hits = E.below(target)
            cap = (0, 1, 3, len(hits), len(hits) + 2)[(i // 5) % 5]
            reqs.append((m, lo, hi, target, cap))
            want.append(hits[:cap])
        return reqs, want
    return _once(("matrix", n, seed), make)


def rounds(oracle, n=24, seed=31):
    """-> (requests, expected): requests of up to 5000 nonces, to be run with a
    slice cap of 1000 so that they finish in different rounds: some ask for
    every hit at or below their 41st smallest hash, some for the first 3 at or
    below the 8th."""
    def make():
        reqs, want = [], []
        for i, (m, lo, hi) in enumerate(batch_cases.random_requests(n, seed, max_nonces=5000)):
            if lo > hi:
                reqs.append((m, lo, hi, U64_MAX, 3))
                want.append([])
                continue
            E = Expect(oracle, m, lo, hi)
            target, cap = ((E.nth(40), 100), (E.nth(7), 3))[i % 2]
            reqs.append((m, lo, hi, target, cap))
            want.append(E.below(target, cap=cap))
        return reqs, want
    return _once(("rounds", n, seed), make)
