"""GPU parity of p1hip_scan_batch: many small requests, of any messages, in
one launch pair per device (k_batch_scan: one workgroup per 256 nonces, its
piece found by binary search in the segment table; k_batch_reduce: one
workgroup per request).  Every result must be exactly what p1hip_scan / the
oracle gives for that request, in request order, whatever shares the launch:
other messages, one-nonce neighbours, requests run individually, several
launch pairs, two devices, earlier calls' buffers.

The session sets P1HIP_SMALL_MAX_NONCES=0 (conftest.py); coalescing does not
depend on it.

Reference: miner.go:56-63 (each request's answer is that loop's)."""
import random
import time

import pytest

from batch_cases import U64_MAX, random_requests

pytestmark = pytest.mark.gpu
SMALL = 1 << 16


@pytest.fixture
def batch(gpu):
    gpu.reset_stats()
    return gpu


def oracle_all(oracle_mod, reqs):
    return [oracle_mod.scan(m if isinstance(m, bytes) else m.encode(), lo, hi, threads=8) for m, lo, hi in reqs]


def test_batch_kats(batch, oracle_mod):
    got = batch.scan_batch([("msg", 0, 2), ("bradfitz", 0, 9999), ("msg", 5, 4), ("", 0, 0)])
    assert got[0] == (4754799531757243342, 1)
    assert got[1] == (1419516646206828, 9898)
    assert got[2] == (U64_MAX, 0)
    assert got[3] == oracle_mod.scan(b"", 0, 0)
    s = batch.get_batch_stats()
    assert (s["calls"], s["requests"], s["coalesced"], s["empty"], s["individual"], s["launches"]) == (1, 4, 3, 1, 0, 1)
    assert s["nonces"] == 3 + 10000 + 1
    assert batch.get_stats()["scans"] == 0  # coalesced requests are not p1hip_scan calls
    batch.reset_stats()
    assert batch.get_batch_stats()["calls"] == 0


def test_batch_random_against_oracle(batch, oracle_mod):
    reqs = random_requests(200, seed=72)
    want = oracle_all(oracle_mod, reqs)
    got = batch.scan_batch(reqs)
    assert got == want
    assert batch.scan_batch(reqs[::-1]) == got[::-1]
    assert batch.get_batch_stats()["launches"] == 2


def test_batch_size_limit(batch, oracle_mod):
    b = 10 ** 9
    reqs = [("bradfitz", b, b + n - 1) for n in (1, 255, 256, 257, SMALL, SMALL + 1)]
    assert batch.scan_batch(reqs) == oracle_all(oracle_mod, reqs)
    s = batch.get_batch_stats()
    assert (s["coalesced"], s["individual"], s["launches"]) == (5, 1, 1)
    assert s["tiles"] == 1 + 1 + 1 + 2 + 256
    assert batch.get_stats()["scans"] == 1


def test_batch_mixed_with_a_large_request(batch, oracle_mod):
    reqs = [("alpha", 990, 1010), (b"cmu440-p1-" * 12, 10 ** 9 - 1000, 10 ** 9 - 1000 + (1 << 20) - 1), ("beta", 7, 6),
            ("gamma", U64_MAX - 300, U64_MAX)]
    assert batch.scan_batch(reqs) == oracle_all(oracle_mod, reqs)
    s = batch.get_batch_stats()
    assert (s["coalesced"], s["individual"], s["empty"], s["launches"]) == (2, 1, 1, 1)
    st = batch.get_stats()
    assert st["scans"] == 1 and st["scan_nonces"] == 1 << 20


def test_batch_many_one_nonce_requests(batch, golden):
    vs = [golden["hash"][i % len(golden["hash"])] for i in range(4096)]
    got = batch.scan_batch([(bytes.fromhex(v["msg_hex"]), v["nonce"], v["nonce"]) for v in vs])
    assert got == [(v["hash"], v["nonce"] if v["hash"] != U64_MAX else 0) for v in vs]
    s = batch.get_batch_stats()
    assert s["tiles"] == 4096 == s["nonces"] and s["launches"] == 1


def test_batch_small_launch_cap(batch, oracle_mod, monkeypatch):
    rnd = random.Random(73)
    reqs = []
    for i in range(40):
        lo = rnd.choice([0, 10 ** 5 - 100, rnd.randrange(10 ** 12)])
        reqs.append((bytes(rnd.randrange(256) for _ in range(rnd.randrange(0, 130))), lo, lo + rnd.randrange(1, 601) - 1))
    free = batch.scan_batch(reqs)
    assert batch.get_batch_stats()["launches"] == 1
    batch.reset_stats()
    # 40 requests of 1..600 nonces are about 70 tiles: a cap of 300 still holds
    # them in one launch pair, so the same knob at 30 is what cuts them into
    # several (test_batch_small_launch_cap_300 has requests large enough for 300)
    monkeypatch.setenv("P1HIP_BATCH_MAX_TILES", "300")
    assert batch.scan_batch(reqs) == free
    monkeypatch.setenv("P1HIP_BATCH_MAX_TILES", "30")
    capped = batch.scan_batch(reqs)
    assert batch.get_batch_stats()["launches"] >= 1 + 3
    assert capped == free == oracle_all(oracle_mod, reqs)


def test_batch_small_launch_cap_300(batch, oracle_mod, monkeypatch):
    """P1HIP_BATCH_MAX_TILES=300 with 40 requests large enough for several
    launch pairs of at most 300 tiles."""
    rnd = random.Random(74)
    reqs = []
    for i in range(40):
        lo = rnd.choice([0, 10 ** 5 - 100, rnd.randrange(10 ** 12)])
        n = rnd.randrange(1, 601) if i % 2 else rnd.randrange(1, 601) * 64  # 1..600 nonces, and 1..150 tiles
        reqs.append((b"launch cap %d" % i, lo, lo + n - 1))
    free = batch.scan_batch(reqs)
    one = batch.get_batch_stats()
    assert one["launches"] == 1 and one["tiles"] > 900
    batch.reset_stats()
    monkeypatch.setenv("P1HIP_BATCH_MAX_TILES", "300")
    capped = batch.scan_batch(reqs)
    s = batch.get_batch_stats()
    assert s["launches"] >= 4 and s["tiles"] == one["tiles"]
    assert capped == free == oracle_all(oracle_mod, reqs)


def test_batch_repeated_calls_interleaved_with_scans(batch, oracle_mod):
    """Buffer reuse and growth: 50 calls of 1..64 requests, a plain scan of
    another message between them (its buffers are not the batch's)."""
    rnd = random.Random(75)
    pool = random_requests(400, seed=76, max_nonces=600)
    want = dict(zip(range(len(pool)), oracle_all(oracle_mod, pool)))
    for call in range(50):
        idx = [rnd.randrange(len(pool)) for _ in range(rnd.randrange(1, 65))]
        assert batch.scan_batch([pool[i] for i in idx]) == [want[i] for i in idx], call
        lo = rnd.randrange(10 ** 9)
        m = b"between %d" % call
        assert batch.scan(m, lo, lo + 2000) == oracle_mod.scan(m, lo, lo + 2000), call
    s = batch.get_batch_stats()
    assert s["calls"] == 50 and batch.get_stats()["scans"] == 50


def test_batch_two_logical_devices(batch, oracle_mod, monkeypatch):
    """GPU 0 listed twice (P1HIP_NO_RCCL: no communicator): the coalesced
    requests are cut into one contiguous group per device, each launched on
    its device's stream before either is synchronised."""
    monkeypatch.setenv("P1HIP_NO_RCCL", "1")
    batch.shutdown()
    batch.init_devices([0, 0])
    try:
        batch.reset_stats()
        reqs = random_requests(30, seed=77)
        assert batch.scan_batch(reqs) == oracle_all(oracle_mod, reqs)
        lay = batch.batch_layout(reqs, 2)
        assert {x["device"] for x in lay if x["tiles"]} == {0, 1}
        s = batch.get_batch_stats()
        assert s["launches"] == 2 and s["tiles"] == sum(x["tiles"] for x in lay)
    finally:
        monkeypatch.delenv("P1HIP_NO_RCCL")
        batch.shutdown()
        batch.init_devices([0])


def test_batch_beats_the_scan_loop(batch, monkeypatch, capsys):
    """256 x configs[0] (`bradfitz [0, 9999]`): one scan_batch call against
    256 p1hip_scan calls on production's path (the one-launch small path).
    The loop is latency-bound on a device it fills to a few percent, so the
    floor asserted is a factor 2; missing it means nothing was coalesced.

    Measured on the MI355X (best of 5 each, both sides timed from Python):
    scan_batch 356 us (235 us of it inside the library) against 5528 us for
    the loop (21.6 us per call), 15.5x; profiles/batch_timing_test.txt."""
    reqs = [("bradfitz", 0, 9999)] * 256
    monkeypatch.setenv("P1HIP_SMALL_MAX_NONCES", str(SMALL))
    try:
        for _ in range(3):  # warm-up: buffers, code objects, clocks
            batch.scan_batch(reqs)
            for m, lo, hi in reqs[:32]:
                batch.scan(m, lo, hi)
        t_batch, t_loop = [], []
        batch.reset_stats()
        for _ in range(5):
            t0 = time.perf_counter()
            got = batch.scan_batch(reqs)
            t_batch.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            ref = [batch.scan(m, lo, hi) for m, lo, hi in reqs]
            t_loop.append(time.perf_counter() - t0)
            assert got == ref == [(1419516646206828, 9898)] * 256
        assert batch.get_stats()["small_scans"] >= 5 * 256
    finally:
        monkeypatch.setenv("P1HIP_SMALL_MAX_NONCES", "0")
    tb, tl = min(t_batch), min(t_loop)
    lib_us = batch.get_batch_stats()["wall_ms"] / 5 * 1e3
    with capsys.disabled():
        print(f"\n256 x configs[0]: scan_batch {tb * 1e6:.0f} us ({lib_us:.0f} us of it inside the library, mean), "
              f"256 scan calls {tl * 1e6:.0f} us ({tl / 256 * 1e6:.1f} us each), ratio {tl / tb:.1f}x")
    assert tb <= tl / 2
