"""GPU parity of p1hip_batch_submit / p1hip_batch_wait: a ticket's results
are exactly what p1hip_scan gives for each request, whatever else is
outstanding -- other tickets (each in its own slot's buffers), a synchronous
call queued behind them on the same stream, another host thread blocked in a
wait.  Expected values come from the CPU oracle or from the synchronous call,
never from another ticket.

Reference: miner.go:56-63 (each request's answer is that loop's)."""
import ctypes
import threading

import pytest

from batch_cases import random_requests
from wide_cases import SMALL, U64_MAX, WIDE_MAX, mid_requests

pytestmark = pytest.mark.gpu

TWO_BLOCK = b"t" * 50  # 50 + ' ' + 10 digits pass the 55 bytes one tail block holds


@pytest.fixture
def asy(gpu):
    gpu.reset_stats()
    return gpu


def oracle_all(oracle_mod, reqs):
    return [oracle_mod.scan(m if isinstance(m, bytes) else m.encode(), lo, hi, threads=8) for m, lo, hi in reqs]


def sized(msg, lo, n):
    return (msg, lo, lo + n - 1)


@pytest.fixture(scope="module")
def edges():
    """One call: every size at which a route or a tile count changes, two
    messages (one with a two-block tail), a decade crossing, an empty range,
    the shared random lists, and one request for the individual route."""
    a = 10 ** 9 - 300
    reqs = [sized(b"bradfitz" if i % 2 else TWO_BLOCK, a + 1000 * i, n)
            for i, n in enumerate((1, 255, 256, 257, SMALL, SMALL + 1))]
    reqs += [(b"bradfitz", 99990, 100100), (b"msg", 5, 4), (TWO_BLOCK, 99990, 100100)]
    reqs += random_requests(40, seed=91) + mid_requests(12, seed=92)
    reqs.append(sized(b"one past the wide limit", 10 ** 10 - 5000, WIDE_MAX + 1))
    return reqs


@pytest.fixture(scope="module")
def edges_want(edges, oracle_mod):
    return oracle_all(oracle_mod, edges)


@pytest.mark.parametrize("wide", [False, True])
def test_parity_at_the_edges(asy, edges, edges_want, wide):
    t = asy.batch_submit(edges, wide=wide)
    assert t != 0
    got = asy.batch_wait(t)
    assert got == edges_want
    assert got[7] == (U64_MAX, 0)
    nonempty = [r for r in edges if r[1] <= r[2]]
    if wide:
        s = asy.get_wide_stats()
        assert (s["calls"], s["requests"], s["empty"], s["individual"]) == (1, len(edges), 2, 1)
        assert s["small"] == sum(hi - lo < SMALL for _, lo, hi in nonempty)
        assert s["wide"] == sum(SMALL <= hi - lo < WIDE_MAX for _, lo, hi in nonempty) and s["wide"] == 13
        assert asy.get_stats()["scans"] == 1
    else:
        b = asy.get_batch_stats()
        assert (b["calls"], b["requests"], b["empty"]) == (1, len(edges), 2)
        assert b["individual"] == sum(hi - lo >= SMALL for _, lo, hi in nonempty) == asy.get_stats()["scans"]
    a = asy.get_async_stats()
    assert (a["submits"], a["waits"], a["busy"], a["max_inflight"]) == (1, 1, 0, 1)


def ticket_requests(k):
    """The k-th of several calls of one shape: the same request counts and
    sizes, another message and other ranges."""
    m = b"ticket %d" % k
    return ([sized(m, 10 ** 6 * (k + 1) + 5000 * i, 1 + 700 * i) for i in range(5)] +
            [sized(m + b" wide", 10 ** 8 - 40000 + 10 ** 5 * k, 70000 + 999 * i) for i in range(3)] + [(m, 9, 8)])


def test_four_tickets_reverse_order_then_busy(asy, oracle_mod):
    calls = [ticket_requests(k) for k in range(5)]
    want = [oracle_all(oracle_mod, c) for c in calls]
    ts = [asy.batch_submit(c, wide=True) for c in calls[:4]]
    assert len(set(ts)) == 4 and 0 not in ts
    with pytest.raises(asy.P1HipError) as e:
        asy.batch_submit(calls[4], wide=True)
    assert e.value.rc == asy.ERR_BUSY
    assert asy.batch_wait(ts[3]) == want[3]
    t5 = asy.batch_submit(calls[4], wide=True)  # one wait made room
    assert t5 not in ts
    for k in (2, 1, 0):
        assert asy.batch_wait(ts[k]) == want[k], k
    assert asy.batch_wait(t5) == want[4]
    a = asy.get_async_stats()
    assert (a["submits"], a["waits"], a["busy"], a["max_inflight"]) == (5, 5, 1, 4)
    s = asy.get_wide_stats()
    assert (s["calls"], s["wide"], s["small"], s["empty"]) == (5, 15, 25, 5)


@pytest.mark.parametrize("wide", [0, 1])
def test_requests_are_borrowed_only_until_submit_returns(asy, oracle_mod, wide):
    from p1_amd import _lib

    lib = asy.load()
    # 10^5 nonces: the individual route without `wide` (its message is needed again by the wait)
    reqs = [(b"borrowed one", 10 ** 7 - 300, 10 ** 7 + 400), (b"borrowed two!", 5, 70), (b"borrowed 3", 10 ** 9, 10 ** 9 + 99999)]
    want = oracle_all(oracle_mod, reqs)
    bufs = [ctypes.create_string_buffer(m, len(m)) for m, _, _ in reqs]
    arr = (_lib.Request * len(reqs))()
    for r, b, (m, lo, hi) in zip(arr, bufs, reqs):
        r.msg, r.msg_len, r.lower, r.upper = ctypes.cast(b, ctypes.c_char_p), len(m), lo, hi
    t = ctypes.c_uint64(0)
    _lib._check(lib.p1hip_batch_submit(arr, len(reqs), wide, ctypes.byref(t)))
    for b in bufs:
        ctypes.memset(b, 0x58, len(b))
    ctypes.memset(arr, 0, ctypes.sizeof(arr))
    del bufs
    out = (_lib.Result * len(reqs))()
    _lib._check(lib.p1hip_batch_wait(t.value, out))
    assert [(o.hash, o.nonce) for o in out] == want


def test_slot_reuse_with_growth(asy, oracle_mod):
    """A slot that held a 2-request call takes a 300-request call (its
    buffers grow: the slot is idle) while another ticket is outstanding."""
    two = [(b"two", 100, 4000), (b"two wide", 10 ** 6 - 7, 10 ** 6 + 80000)]
    other = mid_requests(8, seed=93) + random_requests(20, seed=94)
    big = random_requests(280, seed=95) + mid_requests(20, seed=96)
    want_two, want_other, want_big = (oracle_all(oracle_mod, r) for r in (two, other, big))
    for wide in (True, False):
        ta = asy.batch_submit(two, wide=wide)
        tb = asy.batch_submit(other, wide=wide)
        assert asy.batch_wait(ta) == want_two
        tc = asy.batch_submit(big, wide=wide)
        assert (tc & 0xff) == (ta & 0xff) != (tb & 0xff)  # async_slots.hpp: the low byte is the slot
        assert asy.batch_wait(tc) == want_big
        assert asy.batch_wait(tb) == want_other
    assert asy.get_async_stats()["max_inflight"] == 2


def counters(d):
    return {k: v for k, v in d.items() if k != "wall_ms"}


@pytest.mark.parametrize("wide", [False, True])
def test_synchronous_call_between_submit_and_wait(asy, oracle_mod, wide):
    reqs = mid_requests(10, seed=97) + random_requests(30, seed=98)
    want = oracle_all(oracle_mod, reqs)
    t = asy.batch_submit(reqs, wide=wide)
    assert asy.scan("bradfitz", 0, 9999) == (1419516646206828, 9898)  # configs[0]'s request
    assert asy.scan_batch(reqs[10:16]) == want[10:16]
    assert asy.scan_batch_wide(reqs[:3]) == want[:3]
    assert asy.batch_wait(t) == want
    # the accounts move exactly as the synchronous call's do
    asy.reset_stats()
    assert asy.batch_wait(asy.batch_submit(reqs, wide=wide)) == want
    got = counters(asy.get_wide_stats()), counters(asy.get_batch_stats()), asy.get_stats()["scans"]
    asy.reset_stats()
    assert (asy.scan_batch_wide(reqs) if wide else asy.scan_batch(reqs)) == want
    assert got == (counters(asy.get_wide_stats()), counters(asy.get_batch_stats()), asy.get_stats()["scans"])
    assert got[0 if wide else 1]["calls"] == 1


def test_ticket_lifetime(asy, oracle_mod):
    reqs = ticket_requests(7)
    want = oracle_all(oracle_mod, reqs)
    t = asy.batch_submit(reqs, wide=True)
    assert asy.batch_wait(t) == want
    from p1_amd import _lib

    out = (_lib.Result * len(reqs))()
    assert asy.load().p1hip_batch_wait(t, out) == -4  # a second wait
    assert not any(o.hash or o.nonce for o in out)
    t = asy.batch_submit(reqs, wide=True)
    try:
        asy.shutdown()  # drains the stream, cancels the ticket
        assert asy.device_count() == 0
        with pytest.raises(asy.P1HipError) as e:
            asy.batch_wait(t)
        assert e.value.rc == -4
        t2 = asy.batch_submit(reqs, wide=True)  # re-initialises, in fresh slots
        assert t2 != t and asy.device_count() >= 1
        assert asy.batch_wait(t2) == want
    finally:
        asy.shutdown()
        asy.init_devices([0])


def test_two_host_threads(asy, oracle_mod):
    """One thread blocks in the wait of a 16 x 10^6 wide ticket; the other
    submits and waits a small one meanwhile (the wait holds no lock)."""
    big = [sized(b"big %d" % i, 10 ** 9 + 10 ** 7 * i, 10 ** 6) for i in range(16)]
    small = random_requests(30, seed=99)
    want_big, want_small = asy.scan_batch_wide(big), oracle_all(oracle_mod, small)
    assert want_big[:2] == oracle_all(oracle_mod, big[:2])
    asy.reset_stats()
    t = asy.batch_submit(big, wide=True)
    got = {}

    def waiter():
        try:
            got["big"] = asy.batch_wait(t)
        except Exception as ex:  # noqa: BLE001 - reported by the assert below
            got["big"] = ex

    th = threading.Thread(target=waiter)
    th.start()
    got["small"] = asy.batch_wait(asy.batch_submit(small))
    th.join(60)
    assert not th.is_alive()
    assert got["small"] == want_small and got["big"] == want_big
    a = asy.get_async_stats()
    assert (a["submits"], a["waits"]) == (2, 2)


def test_two_logical_devices(asy, edges, edges_want, monkeypatch):
    """GPU 0 listed twice (P1HIP_NO_RCCL: no communicator), as in
    tests/test_gpu_wide.py: a ticket records one event on each device's
    stream, and its individual request is sharded over both."""
    monkeypatch.setenv("P1HIP_NO_RCCL", "1")
    asy.shutdown()
    asy.init_devices([0, 0])
    try:
        for wide in (False, True):
            asy.reset_stats()
            t1 = asy.batch_submit(edges, wide=wide)
            t2 = asy.batch_submit(edges[::-1], wide=wide)
            assert asy.batch_wait(t2) == edges_want[::-1]
            assert asy.batch_wait(t1) == edges_want
        lay, dev_tiles = asy.wide_layout(edges, 2)
        assert {x["device"] for x in lay if x["route"] == "wide"} == {0, 1} and all(dev_tiles)
        s = asy.get_wide_stats()
        assert (s["calls"], s["wide"], s["individual"]) == (2, 26, 2)
    finally:
        monkeypatch.delenv("P1HIP_NO_RCCL")
        asy.shutdown()
        asy.init_devices([0])
