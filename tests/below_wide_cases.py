"""Request lists and the oracle side of the p1hip_scan_below_batch_wide tests,
shared by the CPU replay (tests/test_below_wide_host.py, through `batch_emu
beloww`) and the GPU tests (tests/test_gpu_below_wide.py, through
p1_amd.scan_below_batch_wide), the way below_batch_cases.py is shared.

A request is (msg, lower, upper, target, cap); its expected answer is the
reference loop, brute force by the oracle (below_cases.Expect), cut at cap.
Targets are taken from the data (Expect.nth), so hit counts are known."""
import below_cases
from below_cases import U64_MAX, Expect

DENSE_TARGET = 1 << 46
_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def cells(oracle):
    """The oracle's hashes of every below_cases.K3_QS cell (564000 nonces each,
    one k = 3 variant per cell under the floor below_cases.FLOOR), once."""
    return _once("cells", lambda: [Expect(oracle, *c) for c in below_cases.k3_selection()])


def small(oracle):
    return _once("small", lambda: Expect(oracle, b"one tile", 77, 200))


def mixed(oracle, forced_sparse):
    """-> (requests, expected, number of filtered ones).  Every K3_QS cell,
    between them dense one-tile requests and empty ones.

    Auto path (`forced_sparse` off): a cell's target is the largest of its
    four smallest hashes that is still below 2^46 (the sparse side of the
    switch), so its one slice of 564000 nonces is filtered; a cell without
    one asks for its first hit at its smallest hash and is coalesced; the
    one-tile requests are dense and share the round's launch pairs.
    Forced sparse: a cell's target is its 8th smallest hash, whatever that is,
    and the one-tile requests are filtered too."""
    def make():
        reqs, want, filtered = [], [], 0
        S = small(oracle)
        for i, E in enumerate(cells(oracle)):
            if forced_sparse:
                j = 7
            else:
                j = max([k for k in range(4) if E.nth(k) < DENSE_TARGET], default=None)
            if j is None:  # even its smallest hash is on the dense side: cap = 1 keeps it coalesced, in several rounds
                target, cap = E.nth(0), 1
            else:
                target, cap = E.nth(j), (1, j + 1, j + 3, 100, 2, j + 1)[i]
                filtered += 1
            reqs.append((E.msg, E.lo, E.hi, target, cap))
            want.append(E.below(target, cap=cap))
            t = S.nth(i)
            reqs.append((S.msg, S.lo, S.hi, t, 10))
            want.append(S.below(t))
            filtered += forced_sparse
            if i % 2:
                reqs.append((E.msg, E.hi, E.lo, U64_MAX, 3) if i % 4 == 1 else (E.msg, E.lo, E.hi, U64_MAX, 0))
                want.append([])
        return reqs, want, filtered
    return _once(("mixed", forced_sparse), make)
