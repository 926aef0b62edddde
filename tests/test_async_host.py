"""p1hip_batch_submit / p1hip_batch_wait without a GPU: the new entry points
and struct sizes, the empty call (a ticket without a device), tickets that
hold nothing, the argument checks that run before anything is enqueued, and
`tools/async_slots_test` -- the ticket bookkeeping (p1_amd/csrc/async_slots.hpp)
against a model.

Reference: miner.go:56-63 (each request's answer is that loop's; the GPU side
is tests/test_gpu_async.py)."""
import ctypes
import os
import subprocess

import pytest

from conftest import ROOT, host_bin

SLOTS_TEST = host_bin(os.path.join(ROOT, "tools", "async_slots_test"))


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(SLOTS_TEST):
        subprocess.run(["make", "-s", "-C", ROOT, "tools/async_slots_test"], check=True)


def test_symbols_constants_and_struct_sizes():
    import p1_amd
    from p1_amd import _lib

    for name in ("batch_submit", "batch_wait", "get_async_stats"):
        assert callable(getattr(p1_amd, name))
    lib = p1_amd.load()
    for sym in ("p1hip_batch_submit", "p1hip_batch_wait", "p1hip_get_async_stats"):
        assert getattr(lib, sym)
    assert p1_amd.ERR_BUSY == -5 and p1_amd.MAX_INFLIGHT == 4
    assert p1_amd.abi_version() == 6 == p1_amd.ABI_VERSION  # purely additive
    # include/p1hip.h: 4 x uint64_t + 2 x double; a ticket is a uint64_t
    assert ctypes.sizeof(_lib.AsyncStats) == 48
    assert [n for n, _ in _lib.AsyncStats._fields_] == ["submits", "waits", "busy", "max_inflight", "submit_ms",
                                                        "wait_ms"]
    assert ctypes.sizeof(_lib.Request) == 32 and ctypes.sizeof(_lib.Result) == 16
    hdr = open(os.path.join(ROOT, "include", "p1hip.h")).read()
    assert "#define P1HIP_ERR_BUSY (-5)" in hdr and "#define P1HIP_MAX_INFLIGHT 4" in hdr
    assert "#define P1HIP_ABI_VERSION 6" in hdr
    assert lib.p1hip_get_async_stats(None) == -4


def test_empty_call_takes_a_ticket_and_no_device():
    import p1_amd

    p1_amd.reset_stats()
    seen = set()
    for wide in (False, True):
        t = p1_amd.batch_submit([], wide=wide)
        assert t != 0 and t not in seen
        seen.add(t)
        assert p1_amd.batch_wait(t) == []
        with pytest.raises(p1_amd.P1HipError) as e:  # already waited
            p1_amd.batch_wait(t)
        assert e.value.rc == -4 and "ticket" in str(e.value)
    assert p1_amd.device_count() == 0
    s = p1_amd.get_async_stats()
    assert (s["submits"], s["waits"], s["busy"], s["max_inflight"]) == (2, 2, 0, 1)
    # an empty call counts in neither route's account, as the synchronous calls' n == 0 does not
    assert p1_amd.get_batch_stats()["calls"] == 0 and p1_amd.get_wide_stats()["calls"] == 0


def test_empty_calls_fill_the_slots():
    """P1HIP_MAX_INFLIGHT tickets, then P1HIP_ERR_BUSY; waited in reverse
    order; a wait frees a slot."""
    import p1_amd

    p1_amd.reset_stats()
    ts = [p1_amd.batch_submit([]) for _ in range(p1_amd.MAX_INFLIGHT)]
    assert len(set(ts)) == p1_amd.MAX_INFLIGHT and 0 not in ts
    with pytest.raises(p1_amd.P1HipError) as e:
        p1_amd.batch_submit([])
    assert e.value.rc == p1_amd.ERR_BUSY
    assert p1_amd.batch_wait(ts.pop()) == []
    ts.append(p1_amd.batch_submit([], wide=True))
    assert len(set(ts)) == p1_amd.MAX_INFLIGHT
    for t in reversed(ts):
        assert p1_amd.batch_wait(t) == []
    s = p1_amd.get_async_stats()
    assert (s["submits"], s["waits"], s["busy"], s["max_inflight"]) == (5, 5, 1, 4)
    assert p1_amd.device_count() == 0


def test_shutdown_cancels_tickets():
    import p1_amd

    t = p1_amd.batch_submit([])
    p1_amd.shutdown()
    with pytest.raises(p1_amd.P1HipError) as e:
        p1_amd.batch_wait(t)
    assert e.value.rc == -4
    # the slot is free again: a full set of tickets fits
    ts = [p1_amd.batch_submit([]) for _ in range(p1_amd.MAX_INFLIGHT)]
    assert t not in ts
    for x in ts:
        assert p1_amd.batch_wait(x) == []


@pytest.mark.parametrize("ticket", [0, 1, 5, 0x101, 0xffffffffffffffff, 0x123456789a02])
def test_bogus_ticket(ticket):
    import p1_amd
    from p1_amd import _lib

    lib = p1_amd.load()
    out = (_lib.Result * 1)()
    out[0].hash, out[0].nonce = 7, 7
    assert lib.p1hip_batch_wait(ticket, out) == -4
    assert b"ticket" in lib.p1hip_last_error()
    assert (out[0].hash, out[0].nonce) == (7, 7)
    assert p1_amd.device_count() == 0


@pytest.mark.parametrize("wide", [0, 1])
@pytest.mark.parametrize("bad", ["null_msg", "too_long"])
def test_bad_request_is_named_and_takes_no_slot(bad, wide):
    import p1_amd
    from p1_amd import _lib

    lib = p1_amd.load()
    arr = (_lib.Request * 4)()
    for r in arr:
        r.msg, r.msg_len, r.lower, r.upper = b"msg", 3, 0, 2
    if bad == "null_msg":
        arr[2].msg, arr[2].msg_len = None, 5
    else:
        arr[2].msg_len = (1 << 28) + 1  # P1HIP_MAX_MSG_LEN + 1 (checked, never read)
    t = ctypes.c_uint64(77)
    for _ in range(p1_amd.MAX_INFLIGHT + 1):  # a refused call holds no slot: never P1HIP_ERR_BUSY
        assert lib.p1hip_batch_submit(arr, 4, wide, ctypes.byref(t)) == -4
        assert b"request 2" in lib.p1hip_last_error()
    assert t.value == 77  # written only on success
    assert lib.p1hip_batch_submit(None, 4, wide, ctypes.byref(t)) == -4
    assert lib.p1hip_batch_submit(arr, 4, wide, None) == -4
    assert p1_amd.device_count() == 0


def test_slots_unit():
    r = subprocess.run([SLOTS_TEST, "7", "200000"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout + r.stderr
