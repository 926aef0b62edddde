"""GPU parity of p1hip_scan_batch_wide: the requests of a call above 2^16 and
of at most 2^24 nonces, of any messages, share k_scan launches (up to 64
segments each, pieces ordered longest-running first across all requests),
their generic pieces share one k_batch_scan launch, and k_wide_reduce folds
one result per request from the request's ranges of the device's partial
array.  Every result must be exactly what p1hip_scan / the oracle gives for
that request, in request order, whatever shares the launches: other
messages, the same request twice, many launches back to back on one ticket,
requests whose pieces land in different launches, two devices, earlier
calls' buffers (shared with p1hip_scan and p1hip_scan_batch).

Reference: miner.go:56-63 (each request's answer is that loop's)."""
import random
import time

import pytest

from wide_cases import SMALL, U64_MAX, mid_requests

pytestmark = pytest.mark.gpu


@pytest.fixture
def wide(gpu):
    gpu.reset_stats()
    return gpu


def oracle_all(oracle_mod, reqs):
    return [oracle_mod.scan(m if isinstance(m, bytes) else m.encode(), lo, hi, threads=8) for m, lo, hi in reqs]


@pytest.fixture(scope="module")
def mid40():
    return mid_requests(40, seed=82)


@pytest.fixture(scope="module")
def want40(mid40, oracle_mod):
    return oracle_all(oracle_mod, mid40)


def test_wide_mixed_kats(wide, oracle_mod, monkeypatch):
    monkeypatch.setenv("P1HIP_WIDE_MAX_NONCES", "300000")
    reqs = [("bradfitz", 0, 99999), ("bradfitz", 0, 9999), ("msg", 5, 4), ("bradfitz", 10 ** 9, 10 ** 9 + 300000)]
    got = wide.scan_batch_wide(reqs)
    assert got == oracle_all(oracle_mod, reqs)
    assert got[1] == (1419516646206828, 9898) and got[2] == (U64_MAX, 0)
    s = wide.get_wide_stats()
    assert (s["calls"], s["requests"]) == (1, 4)
    assert (s["empty"], s["small"], s["wide"], s["individual"]) == (1, 1, 1, 1)
    assert s["scan_launches"] == 1 and s["nonces"] == 100000
    lay, dev_tiles = wide.wide_layout(reqs, 1)
    assert [x["route"] for x in lay] == ["wide", "small", "empty", "individual"]
    assert (s["scan_segments"], s["tiles"]) == (lay[0]["segs"], lay[0]["tiles"]) and dev_tiles == [lay[0]["tiles"]]
    # the other accounts move only by what the small and the individual route do
    b = wide.get_batch_stats()
    assert (b["calls"], b["requests"], b["coalesced"], b["individual"], b["empty"], b["launches"]) == (1, 1, 1, 0, 0, 1)
    assert b["nonces"] == 10000
    st = wide.get_stats()
    assert st["scans"] == 1 and st["scan_nonces"] == 300001
    wide.reset_stats()
    assert wide.get_wide_stats()["calls"] == 0


def test_wide_random_against_oracle(wide, mid40, want40, monkeypatch):
    got = wide.scan_batch_wide(mid40)
    assert got == want40
    assert wide.scan_batch_wide(mid40[::-1]) == want40[::-1]
    s = wide.get_wide_stats()
    assert s["wide"] == 80 and s["small"] == s["individual"] == 0 and s["scan_launches"] >= 2
    free_tiles = s["tiles"]
    # the floor that keeps k = 3: other variants, fewer and longer tiles
    wide.reset_stats()
    monkeypatch.setenv("P1HIP_WIDE_MIN_FAST_THREADS", "1")
    assert wide.scan_batch_wide(mid40) == want40
    assert wide.scan_batch_wide(mid40[::-1]) == want40[::-1]
    assert wide.get_wide_stats()["tiles"] < free_tiles


def test_wide_small_launches(wide, mid40, want40, monkeypatch):
    """Launches of at most 4 segments: many k_scan launches back to back on
    one ticket, and requests whose pieces land in different launches."""
    free = wide.scan_batch_wide(mid40)
    wide.reset_stats()
    monkeypatch.setenv("P1HIP_WIDE_MAX_SEGS", "4")
    capped = wide.scan_batch_wide(mid40)
    s = wide.get_wide_stats()
    assert s["scan_launches"] >= len(mid40) / 4 and s["scan_launches"] >= s["scan_segments"] / 4
    assert capped == free == want40
    lay, _ = wide.wide_layout(mid40, 1)
    assert any(len({ln for _, _, ln in x["ranges"] if ln >= 0}) > 1 for x in lay)


def test_wide_adjacent_ranges(wide, oracle_mod):
    a = 10 ** 8 - 90000
    reqs = [("adjacent", a, a + 99999), ("adjacent", a + 100000, a + 100000 + 149999), ("adjacent", a, a + 249999)]
    got = wide.scan_batch_wide(reqs)
    assert min(got[0], got[1]) == got[2]
    assert got == oracle_all(oracle_mod, reqs)
    assert wide.get_wide_stats()["wide"] == 3


def test_wide_golden(wide, golden):
    """The three golden mtest vectors above 2^16 nonces (10^7-nonce jobs) in one call."""
    vs = [v for v in golden["scan"] if "mtest" in v["source"] and v["upper"] - v["lower"] >= SMALL]
    assert len(vs) == 3
    got = wide.scan_batch_wide([(bytes.fromhex(v["msg_hex"]), v["lower"], v["upper"]) for v in vs])
    assert got == [(v["hash"], v["nonce"]) for v in vs]
    s = wide.get_wide_stats()
    assert s["wide"] == 3 and s["nonces"] == sum(v["upper"] - v["lower"] + 1 for v in vs)


def test_wide_calls_interleaved_with_scans_and_batches(wide, oracle_mod, mid40, want40):
    """Buffer reuse and growth, and the ticket: d_part, the segment table and
    the ticket are p1hip_scan's, the generic table and the result array
    p1hip_scan_batch's."""
    rnd = random.Random(83)
    small = [(b"small %d" % i, max(0, 10 ** (i % 12) - 40), 10 ** (i % 12) + rnd.randrange(1, 500)) for i in range(24)]
    small_want = oracle_all(oracle_mod, small)
    for call in range(20):
        idx = [rnd.randrange(len(mid40)) for _ in range(rnd.randrange(1, 13))]
        assert wide.scan_batch_wide([mid40[i] for i in idx]) == [want40[i] for i in idx], call
        lo = rnd.randrange(10 ** 9)
        m = b"between %d" % call
        assert wide.scan(m, lo, lo + 70000) == oracle_mod.scan(m, lo, lo + 70000, threads=8), call
        j = rnd.randrange(len(small) - 6)
        assert wide.scan_batch(small[j:j + 6]) == small_want[j:j + 6], call
    s = wide.get_wide_stats()
    assert s["calls"] == 20 and wide.get_stats()["scans"] == 20 and wide.get_batch_stats()["calls"] == 20


def test_wide_two_logical_devices(wide, mid40, want40, monkeypatch):
    """GPU 0 listed twice (P1HIP_NO_RCCL: no communicator): the wide requests
    are cut into one contiguous group per device, each enqueued on its
    device's stream before either is synchronised."""
    monkeypatch.setenv("P1HIP_NO_RCCL", "1")
    wide.shutdown()
    wide.init_devices([0, 0])
    try:
        wide.reset_stats()
        assert wide.scan_batch_wide(mid40) == want40
        lay, dev_tiles = wide.wide_layout(mid40, 2)
        assert {x["device"] for x in lay} == {0, 1} and all(dev_tiles)
        s = wide.get_wide_stats()
        assert s["tiles"] == sum(dev_tiles) and s["scan_launches"] >= 2 and s["generic_launches"] == 2
    finally:
        monkeypatch.delenv("P1HIP_NO_RCCL")
        wide.shutdown()
        wide.init_devices([0])


def test_wide_beats_the_scan_loop(wide, capsys):
    """256 x `bradfitz [10^9, 10^9 + 10^5 - 1]`: one scan_batch_wide call
    against 256 p1hip_scan calls (the parent's behaviour for this size), best
    of 5 each after warm-up, both timed from Python in this process.  Only
    wide <= loop is asserted; the figures are printed.

    Measured on the MI355X: scan_batch_wide 999 us (876 us of it inside the
    library; 4 k_scan launches, 10240 tiles) against 13379 us for the loop
    (52.3 us per call), 13.4x; profiles/wide_timing_test.txt."""
    reqs = [("bradfitz", 10 ** 9, 10 ** 9 + 10 ** 5 - 1)] * 256
    for _ in range(3):  # warm-up: buffers, code objects, clocks
        wide.scan_batch_wide(reqs)
        for m, lo, hi in reqs[:32]:
            wide.scan(m, lo, hi)
    t_wide, t_loop = [], []
    wide.reset_stats()
    for _ in range(5):
        t0 = time.perf_counter()
        got = wide.scan_batch_wide(reqs)
        t_wide.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        ref = [wide.scan(m, lo, hi) for m, lo, hi in reqs]
        t_loop.append(time.perf_counter() - t0)
        assert got == ref and len(set(got)) == 1
    tw, tl = min(t_wide), min(t_loop)
    s = wide.get_wide_stats()
    with capsys.disabled():
        print(f"\n256 x 10^5 nonces: scan_batch_wide {tw * 1e6:.0f} us ({s['wall_ms'] / 5 * 1e3:.0f} us of it inside "
              f"the library, mean; {s['scan_launches'] // 5} k_scan launches, {s['tiles'] // 5} tiles), 256 scan calls "
              f"{tl * 1e6:.0f} us ({tl / 256 * 1e6:.1f} us each), ratio {tl / tw:.1f}x")
    assert s["wide"] == 5 * 256
    assert tw <= tl
