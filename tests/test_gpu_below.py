"""GPU tests of p1hip_scan_below: every nonce of a range whose hash is at or
below a target, in increasing nonce, the first `cap` of them.

The expected list is always the reference loop, brute force by the oracle
(below_cases.Expect), and equality is exact.  Both routes of a slice run on
every shape: sparse (the shipped k_scan filters, k_below_mark looks at the
surviving tiles) and dense (k_below_mark looks at every nonce); the shapes are
those of the CPU replay in tests/test_below_host.py."""
import pytest

import below_cases
import tile_cases
from below_cases import U64_MAX, Expect, increasing, resume_chain

pytestmark = pytest.mark.gpu

SCAN_CODEOBJ = "da205152f146ea639f2cb01d4e2dcb4fae1b0325fc87a52e875623d86b11db41"
BATCH_CODEOBJ = "b79543a94ef1c35ca696d644d9aea4595ca7862ae9ece505fc64376007ebc8af"
SPARSE, DENSE = "1", "2"
_STATE = {"floor": None}


@pytest.fixture
def dev(gpu, monkeypatch):
    """-> go(floor): device 0 opened with that occupancy floor (None: the
    library's own), re-initialised only when the floor changes.  The per-call
    knobs of this module are cleared before and after."""
    def clear():
        for k in ("P1HIP_BELOW_PATH", "P1HIP_BELOW_MAX_SLICE"):
            monkeypatch.delenv(k, raising=False)

    def go(floor=None):
        if _STATE["floor"] != floor or gpu.device_count() != 1:
            if floor is None:
                monkeypatch.delenv("P1HIP_MIN_FAST_THREADS", raising=False)
            else:
                monkeypatch.setenv("P1HIP_MIN_FAST_THREADS", str(floor))
            gpu.shutdown()
            gpu.init_devices([0])
            monkeypatch.delenv("P1HIP_MIN_FAST_THREADS", raising=False)
            _STATE["floor"] = floor
        gpu.reset_stats()
        return gpu

    clear()
    yield go
    clear()


@pytest.fixture(scope="module", autouse=True)
def default_device_afterwards(gpu):
    gpu.shutdown()  # whatever floor an earlier module left the device with
    gpu.init_devices([0])
    _STATE["floor"] = None
    yield
    gpu.shutdown()
    gpu.init_devices([0])
    _STATE["floor"] = None


def routed(g, monkeypatch, path, *args, max_slice=None, **kw):
    """scan_below under a forced route (None: the library's choice)."""
    if path is None:
        monkeypatch.delenv("P1HIP_BELOW_PATH", raising=False)
    else:
        monkeypatch.setenv("P1HIP_BELOW_PATH", path)
    if max_slice is None:
        monkeypatch.delenv("P1HIP_BELOW_MAX_SLICE", raising=False)
    else:
        monkeypatch.setenv("P1HIP_BELOW_MAX_SLICE", str(max_slice))
    return g.scan_below(*args, **kw)


# ---------------------------------------------------------------------------
# Known answers
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("msg,target,want,route", [
    # the handout answer is the minimum of [0, 9999], hence the first nonce at or below it; a dense target
    (b"bradfitz", 1419516646206828, (1419516646206828, 9898), "dense_slices"),
    # the golden pin of configs[1]: sparse, one slice of 2^33
    (b"bradfitz", 5256245051, (5256245051, 1626825724), "sparse_slices"),
    # the pin of configs[2]: sparse, MODE 5 with its real table, one slice
    (b"cmu440-p1-" * 12, 1902263685, (1902263685, 2962726851), "sparse_slices"),
])
def test_below_kats(dev, msg, target, want, route):
    g = dev()
    assert g.test_knobs().get("P1HIP_BELOW_PATH") is None
    assert g.scan_below(msg, 0, 2 ** 40, target) == [want]
    s = g.get_below_stats()
    print(s)
    assert s["calls"] == 1 and s["slices"] == 1 and s[route] == 1 and s["hits"] == 1
    assert want[1] < s["examined"] <= g.BELOW_MAX_SLICE
    if route == "sparse_slices":
        assert s["scan_nonces"] == s["examined"] and s["candidate_tiles"] >= 1
        assert s["mark_nonces"] <= 256000 * s["candidate_tiles"]


# ---------------------------------------------------------------------------
# Parity matrix
# ---------------------------------------------------------------------------
_EXPECT = {}


def expect(oracle, case):
    if case not in _EXPECT:
        _EXPECT[case] = Expect(oracle, *case)
    return _EXPECT[case]


def matrix(g, monkeypatch, E):
    msg, lo, hi = E.msg, E.lo, E.hi
    target = E.nth(7)
    want = E.below(target)
    assert len(want) >= min(8, hi - lo + 1)
    # both routes and the library's choice
    sparse = routed(g, monkeypatch, SPARSE, msg, lo, hi, target, cap=100)
    dense = routed(g, monkeypatch, DENSE, msg, lo, hi, target, cap=100)
    auto = routed(g, monkeypatch, None, msg, lo, hi, target, cap=100)
    assert sparse == want and dense == want and auto == want and increasing(want)
    # several slices, not a power of two, hits next to slice edges
    for path in (SPARSE, DENSE):
        g.reset_stats()
        assert routed(g, monkeypatch, path, msg, lo, hi, target, cap=100, max_slice=100000) == want
        assert g.get_below_stats()["slices"] == (hi - lo) // 100000 + 1
    for path in (SPARSE, DENSE, None):
        # truncation: the first three, found == cap
        assert routed(g, monkeypatch, path, msg, lo, hi, target, cap=3) == want[:3]
        # the cap = 1 resume chain reproduces the list
        assert resume_chain(lambda a: routed(g, monkeypatch, path, msg, a, hi, target, cap=1), lo, hi) == want
        # <=: a hash equal to the target is a hit, one above it is not
        h = want[len(want) // 2][0]
        assert routed(g, monkeypatch, path, msg, lo, hi, h, cap=100) == E.below(h)
        assert routed(g, monkeypatch, path, msg, lo, hi, h - 1, cap=100) == E.below(h - 1)
        assert want[len(want) // 2] in E.below(h) and want[len(want) // 2] not in E.below(h - 1)
        # nothing below the range's minimum
        assert routed(g, monkeypatch, path, msg, lo, hi, E.nth(0) - 1, cap=100) == []
        # every nonce is at or below 2^64 - 1
        assert routed(g, monkeypatch, path, msg, lo, hi, U64_MAX, cap=5) == E.first(5)


@pytest.mark.parametrize("i", range(len(below_cases.K3_QS)))
def test_below_matrix_k3_cells(dev, oracle_mod, monkeypatch, i):
    """One tail block, TRAIL, MODE 7, MODE 5 at k = 2 and 3, a PRE cell: k = 3
    tiles of 256000 nonces, ragged generic tiles at both ends."""
    matrix(dev(below_cases.FLOOR), monkeypatch, expect(oracle_mod, below_cases.k3_selection()[i]))


@pytest.mark.parametrize("i", range(2))
def test_below_matrix_mode5_strided_tiles(dev, oracle_mod, monkeypatch, i):
    """MODE 5 with k = 4 and 5: a candidate tile is 4 x 64 strided runs of 1000 nonces."""
    g = dev(1)
    E = expect(oracle_mod, below_cases.mode5_k45()[i])
    matrix(g, monkeypatch, E)
    g.reset_stats()
    assert routed(g, monkeypatch, SPARSE, E.msg, E.lo, E.hi, E.nth(7), cap=100) == E.below(E.nth(7))
    s = g.get_below_stats()
    assert s["candidate_tiles"] >= 1 and s["mark_nonces"] < s["scan_nonces"]


def test_below_last_nonce_of_u64(dev, oracle_mod, monkeypatch):
    """upper == 2^64 - 1 is scanned inclusively, and nonce 2^64 - 1 can be a hit."""
    g = dev(below_cases.FLOOR)
    E = expect(oracle_mod, (b"edge of u64", U64_MAX - 299_999, U64_MAX))
    target = E.nth(7)
    want = E.below(target)
    last = E.last(1)[0][0]  # the last nonce is a hit of the range's last 1000 nonces at its own hash
    tail = E.below(last, lower=U64_MAX - 999)
    assert tail[-1][1] == U64_MAX
    for path in (SPARSE, DENSE, None):
        assert routed(g, monkeypatch, path, E.msg, E.lo, E.hi, target, cap=100) == want
        assert routed(g, monkeypatch, path, E.msg, E.lo, E.hi, target, cap=100, max_slice=100000) == want
        assert routed(g, monkeypatch, path, E.msg, U64_MAX - 999, U64_MAX, last, cap=2000) == tail
        assert routed(g, monkeypatch, path, E.msg, U64_MAX - 2, U64_MAX, U64_MAX, cap=5) == E.last(3)
        assert routed(g, monkeypatch, path, E.msg, U64_MAX, U64_MAX, last, cap=1) == E.last(1)
        assert routed(g, monkeypatch, path, E.msg, U64_MAX, U64_MAX, last - 1, cap=1) == []


def test_below_slice_of_2_16_and_one_more(dev, oracle_mod):
    """At most 2^16 nonces are marked directly whatever the target; one more
    and a hard target goes through the filter.  The hit is the range's last nonce."""
    g = dev()
    msg, target = b"bradfitz", g.BELOW_DENSE_TARGET - 1
    (h0, n0), = g.scan_below(msg, 10 ** 9, 2 ** 40, target)
    for n, route in ((1 << 16, "dense_slices"), ((1 << 16) + 1, "sparse_slices")):
        E = Expect(oracle_mod, msg, n0 - n + 1, n0)
        g.reset_stats()
        assert g.scan_below(msg, E.lo, E.hi, target, cap=10) == E.below(target)
        assert (h0, n0) in E.below(target)
        s = g.get_below_stats()
        assert s["slices"] == 1 and s[route] == 1 and s["examined"] == n


# ---------------------------------------------------------------------------
# Statistics, devices, neighbours, code objects
# ---------------------------------------------------------------------------
def test_below_sparse_refines_only_its_candidates(dev, oracle_mod, monkeypatch):
    g = dev(below_cases.FLOOR)
    E = expect(oracle_mod, below_cases.k3_selection()[0])
    target = E.nth(7)
    _, tiles, _ = g.scan_tiles(E.msg, E.lo, E.hi)
    cands = [t for t in tiles if t[5] and t[4][0] <= target]
    assert 1 <= len(cands) < len(tiles)
    g.reset_stats()
    assert routed(g, monkeypatch, SPARSE, E.msg, E.lo, E.hi, target, cap=100) == E.below(target)
    s = g.get_below_stats()
    assert s["candidate_tiles"] == len(cands)
    assert s["mark_nonces"] == sum(rl * c for t in cands for _, rl, _, c in t[5])
    assert s["scan_nonces"] == s["examined"] == E.hi - E.lo + 1 and s["sparse_slices"] == 1 and s["dense_slices"] == 0
    assert s["hits"] == len(E.below(target)) and s["mark_launches"] == 1


def test_below_two_logical_devices(dev, oracle_mod, monkeypatch):
    """GPU 0 listed twice (P1HIP_NO_RCCL): a sparse slice is cut across both,
    each enqueued on its own stream; the list is the one-device list."""
    g = dev(below_cases.FLOOR)
    E = expect(oracle_mod, below_cases.k3_selection()[1])
    target = E.nth(7)
    monkeypatch.setenv("P1HIP_NO_RCCL", "1")
    monkeypatch.setenv("P1HIP_MIN_FAST_THREADS", str(below_cases.FLOOR))
    g.shutdown()
    g.init_devices([0, 0])
    try:
        g.reset_stats()
        for path in (SPARSE, DENSE, None):
            assert routed(g, monkeypatch, path, E.msg, E.lo, E.hi, target, cap=100) == E.below(target)
            assert routed(g, monkeypatch, path, E.msg, E.lo, E.hi, target, cap=100, max_slice=100000) == E.below(target)
        d0, d1 = g.get_device_stats(0), g.get_device_stats(1)
        assert d0["scan_nonces"] > 0 and d1["scan_nonces"] > 0
        assert d0["scan_nonces"] + d1["scan_nonces"] == g.get_below_stats()["scan_nonces"]
    finally:
        monkeypatch.delenv("P1HIP_NO_RCCL")
        monkeypatch.delenv("P1HIP_MIN_FAST_THREADS")
        g.shutdown()
        g.init_devices([0])
        _STATE["floor"] = None


def test_below_leaves_its_neighbours_alone(dev, oracle_mod, monkeypatch):
    """A scan, a scan_batch_wide and an outstanding batch_submit ticket around
    a scan_below: all four answers are what they are alone."""
    g = dev()
    small = [(b"ticket %d" % i, 10 ** 6 + 1000 * i, 10 ** 6 + 1000 * i + 999) for i in range(40)]
    wide = [(b"wide %d" % i, 10 ** 9 + i, 10 ** 9 + i + 200_000) for i in range(3)]
    a, lo, hi = tile_cases.QUEUE_RANGES[1]
    E = Expect(oracle_mod, a, lo, hi)
    target = E.nth(7)
    ticket = g.batch_submit(small)
    first = g.scan(a, lo, hi)
    sparse = routed(g, monkeypatch, SPARSE, a, lo, hi, target, cap=100)
    got_wide = g.scan_batch_wide(wide)
    dense = routed(g, monkeypatch, DENSE, a, lo, hi, target, cap=100)
    second = g.scan(a, lo, hi)
    got_small = g.batch_wait(ticket)
    assert sparse == dense == E.below(target)
    assert first == second == E.minimum
    assert got_wide == [oracle_mod.scan(m, x, y, threads=8) for m, x, y in wide]
    assert got_small == [oracle_mod.scan(m, x, y) for m, x, y in small]


def test_below_code_objects(gpu):
    assert gpu.codeobj_sha256() == SCAN_CODEOBJ
    assert gpu.batch_codeobj_sha256() == BATCH_CODEOBJ
    new = gpu.below_codeobj_sha256()
    assert len(new) == 64 and int(new, 16) >= 0 and new not in (SCAN_CODEOBJ, BATCH_CODEOBJ)
