"""p1hip_scan_batch_wide without a GPU: the new entry points and their
argument checks, the layout of a wide call (p1hip_wide_layout /
p1hip_wide_ranges, the function p1hip_scan_batch_wide itself lays out with)
and the host replay `tools/batch_emu wide` -- the library's own wide_plan.hpp,
k_scan tile by tile from each shared launch's segment table, k_batch_scan for
the generic pieces, the per-request range fold -- against the oracle and the
golden fixtures.

Reference: miner.go:56-63 (each request's answer is that loop's)."""
import os
import subprocess

import pytest

from conftest import ROOT, host_bin
from wide_cases import SMALL, U64_MAX, WIDE_MAX, mid_requests

EMU = host_bin(os.path.join(ROOT, "tools", "batch_emu"))


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(EMU):
        subprocess.run(["make", "-s", "-C", ROOT, "tools/batch_emu"], check=True)


def emu_wide(reqs, ndev=1, max_segs=0, floor=0):
    """[(hash, nonce)] per request and the replay's counts."""
    text = "".join(f"{m.hex() or '-'} {lo} {hi}\n" for m, lo, hi in reqs)
    r = subprocess.run([EMU, "wide", str(ndev), str(max_segs), str(floor)], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
    info = dict((k, int(v)) for k, v in (kv.split("=") for kv in r.stderr.split()))
    return out, info


@pytest.fixture(scope="module")
def mid60():
    return mid_requests(60, seed=81)


@pytest.fixture(scope="module")
def want60(mid60, oracle_mod):
    return [oracle_mod.scan(m, lo, hi, threads=8) for m, lo, hi in mid60]


def test_symbols_and_abi():
    import p1_amd

    for name in ("scan_batch_wide", "wide_layout", "get_wide_stats"):
        assert callable(getattr(p1_amd, name))
    assert p1_amd.abi_version() == 6 == p1_amd.ABI_VERSION
    assert p1_amd.scan_batch_wide([]) == []
    assert p1_amd.device_count() == 0  # an empty call opens no device
    assert p1_amd.wide_layout([], 2) == ([], [0, 0])
    s = p1_amd.get_wide_stats()
    assert s["calls"] == 0 and set(s) >= {"empty", "small", "wide", "individual", "scan_launches", "scan_segments",
                                           "tiles", "nonces", "wall_ms"}


@pytest.mark.parametrize("bad", ["null_msg", "too_long"])
def test_bad_request_is_named_before_anything_runs(bad):
    import ctypes

    import p1_amd
    from p1_amd import _lib

    lib = p1_amd.load()
    arr = (_lib.Request * 4)()
    for r in arr:
        r.msg, r.msg_len, r.lower, r.upper = b"msg", 3, 0, 99999
    if bad == "null_msg":
        arr[2].msg, arr[2].msg_len = None, 5
    else:
        arr[2].msg_len = (1 << 28) + 1  # P1HIP_MAX_MSG_LEN + 1 (checked, never read)
    out = (_lib.Result * 4)()
    for o in out:
        o.hash, o.nonce = 7, 7
    with pytest.raises(p1_amd.P1HipError) as e:
        _lib._check(lib.p1hip_scan_batch_wide(arr, 4, out))
    assert e.value.rc == -4 and "request 2" in str(e.value)
    assert all((o.hash, o.nonce) == (7, 7) for o in out)
    assert p1_amd.device_count() == 0
    route, dev = (ctypes.c_int32 * 4)(), (ctypes.c_int32 * 4)()
    segs, tiles = (ctypes.c_uint32 * 4)(), (ctypes.c_uint32 * 4)()
    assert lib.p1hip_wide_layout(arr, 4, 1, route, dev, segs, tiles) == -4
    assert b"request 2" in lib.p1hip_last_error()
    assert lib.p1hip_scan_batch_wide(None, 4, out) == -4 and lib.p1hip_scan_batch_wide(arr, 4, None) == -4


def test_routes_by_size():
    import p1_amd

    b = 10 ** 9
    sizes = [0, 1, SMALL, SMALL + 1, WIDE_MAX, WIDE_MAX + 1]
    reqs = [("m", b, b + n - 1) for n in sizes]
    lay, dev_tiles = p1_amd.wide_layout(reqs, 1)
    assert [x["route"] for x in lay] == ["empty", "small", "small", "wide", "wide", "individual"]
    assert [x["device"] for x in lay] == [-1, -1, -1, 0, 0, -1]
    for x in lay:
        assert (x["tiles"] > 0 and x["segs"] > 0 and x["ranges"]) if x["route"] == "wide" else \
            (x["tiles"] == 0 and x["segs"] == 0 and not x["ranges"])
    assert dev_tiles == [lay[3]["tiles"] + lay[4]["tiles"]]
    # the top of the u64 range is an ordinary wide request
    lay, _ = p1_amd.wide_layout([("m", U64_MAX - 100000, U64_MAX)], 1)
    assert lay[0]["route"] == "wide"


def check_layout(lay, dev_tiles, max_segs):
    """The invariants of a wide layout: per device the wide requests' ranges
    are disjoint, lie inside the partial array and cover it exactly; each
    request's ranges add up to its tiles; one range per k_scan segment, at
    most one for the generic tiles; no k_scan launch above max_segs
    segments, and the launches of a device lie back to back, the generic
    tiles last."""
    for dv, total in enumerate(dev_tiles):
        mine = [x for x in lay if x["device"] == dv]
        spans = sorted((t0, t0 + nt, ln) for x in mine for t0, nt, ln in x["ranges"])
        pos = 0
        for t0, t1, ln in spans:
            assert t0 == pos and t1 > t0, (dv, t0, t1, pos)
            pos = t1
        assert pos == total
        per_launch = {}
        for t0, t1, ln in spans:
            per_launch[ln] = per_launch.get(ln, 0) + 1
        fast = sorted(ln for ln in per_launch if ln >= 0)
        assert fast == list(range(len(fast)))
        assert all(per_launch[ln] <= max_segs for ln in fast)
        order = [ln for _, _, ln in spans]  # by tile: launch 0, 1, ..., then the generic tiles (-1)
        assert order == sorted(order, key=lambda ln: (ln < 0, ln))
        for x in mine:
            assert x["route"] == "wide"
            assert sum(nt for _, nt, _ in x["ranges"]) == x["tiles"]
            assert sum(1 for _, _, ln in x["ranges"] if ln >= 0) == x["segs"]
            assert sum(1 for _, _, ln in x["ranges"] if ln < 0) <= 1
    for x in lay:
        assert (x["device"] >= 0) == (x["route"] == "wide")


def test_layout_invariants(mid60, monkeypatch):
    import p1_amd

    mixed = mid60 + [("small", 5, 600), ("empty", 5, 4), ("bradfitz", 0, 10 ** 6), ("big", 0, WIDE_MAX)]
    lay, dev_tiles = p1_amd.wide_layout(mixed, 1)
    check_layout(lay, dev_tiles, 64)
    assert [x["route"] for x in lay[-4:]] == ["small", "empty", "wide", "individual"]
    assert sum(x["segs"] for x in lay) > 64  # more than one k_scan launch
    assert max(ln for x in lay for _, _, ln in x["ranges"]) >= 1
    # 3 devices: contiguous groups in request order, every device used
    lay3, dev3 = p1_amd.wide_layout(mixed, 3)
    check_layout(lay3, dev3, 64)
    devs = [x["device"] for x in lay3 if x["route"] == "wide"]
    assert devs == sorted(devs) and set(devs) == {0, 1, 2} and all(dev3)
    # the knobs: launches cut small; the floor that keeps k = 3 gives fewer tiles
    monkeypatch.setenv("P1HIP_TEST_KNOBS", "1")
    monkeypatch.setenv("P1HIP_WIDE_MAX_SEGS", "4")
    assert p1_amd.test_knobs()["P1HIP_WIDE_MAX_SEGS"] == "4"
    lay4, dev4 = p1_amd.wide_layout(mixed, 1)
    check_layout(lay4, dev4, 4)
    assert max(ln for x in lay4 for _, _, ln in x["ranges"]) >= sum(x["segs"] for x in lay4) // 4 - 1
    monkeypatch.delenv("P1HIP_WIDE_MAX_SEGS")
    monkeypatch.setenv("P1HIP_WIDE_MIN_FAST_THREADS", "1")
    lay1, dev1 = p1_amd.wide_layout(mixed, 1)
    check_layout(lay1, dev1, 64)
    monkeypatch.setenv("P1HIP_WIDE_MIN_FAST_THREADS", str(1 << 18))
    layf, devf = p1_amd.wide_layout(mixed, 1)
    check_layout(layf, devf, 64)
    assert dev1[0] < dev_tiles[0] <= devf[0]
    monkeypatch.delenv("P1HIP_WIDE_MIN_FAST_THREADS")
    monkeypatch.setenv("P1HIP_WIDE_MAX_NONCES", "100000")
    layw, _ = p1_amd.wide_layout([("m", 0, 99999), ("m", 0, 100000)], 1)
    assert [x["route"] for x in layw] == ["wide", "individual"]
    # without the master switch the knobs are ignored
    monkeypatch.delenv("P1HIP_TEST_KNOBS")
    assert [x["route"] for x in p1_amd.wide_layout([("m", 0, 100000)], 1)[0]] == ["wide"]


def test_floor_rule_is_visible_in_the_layout():
    """The occupancy floor is 2^18 / min(wide requests on the device, 64): a
    request of 10^6 nonces alone is planned like a lone scan (floor 2^18:
    k = 1, 10^5 threads), among 64 or more the floor is 4096 and k = 2
    (10^4 threads) is enough; a request of 10^7 nonces then keeps k = 3."""
    import p1_amd

    r = ("bradfitz", 10 ** 9, 10 ** 9 + 10 ** 6 - 1)
    tiles = {w: p1_amd.wide_layout([r] * w, 1)[0][0]["tiles"] for w in (1, 16, 64, 256)}
    assert tiles[1] == -(-10 ** 5 // 256)    # floor 2^18: k = 1
    assert tiles[16] == -(-10 ** 5 // 256)   # floor 16384 > 10^4 threads: still k = 1
    assert tiles[64] == tiles[256] == -(-10 ** 4 // 256)  # floor 4096: k = 2
    r7 = ("bradfitz", 10 ** 9, 10 ** 9 + 10 ** 7 - 1)
    assert p1_amd.wide_layout([r7], 1)[0][0]["tiles"] == -(-10 ** 6 // 256)       # k = 1
    assert p1_amd.wide_layout([r7] * 64, 1)[0][0]["tiles"] == -(-10 ** 4 // 256)  # 10^4 threads >= 4096: k = 3


def test_emu_wide_against_oracle(mid60, want60):
    got, info = emu_wide(mid60)
    assert got == want60
    assert info["wide"] == 60 and info["small"] == 0 and info["launches"] >= 2
    assert got[5 + 13] == got[5 + 26]  # the same request twice (wide_cases.py)


@pytest.mark.parametrize("setting", ["floor1", "segs4", "dev3"])
def test_emu_wide_settings_agree(mid60, want60, setting):
    """F = 1 (k = 3 everywhere), launches of at most 4 segments (many
    launches, a request's pieces in different ones) and 3 devices: other
    tables, same answers."""
    if setting == "floor1":
        got, info = emu_wide(mid60, floor=1)
    elif setting == "segs4":
        got, info = emu_wide(mid60, max_segs=4)
        assert info["launches"] >= info["segs"] / 4 and info["launches"] >= 15
    else:
        got, info = emu_wide(mid60, ndev=3)
    assert got == want60


def test_emu_wide_golden(golden):
    """The three golden mtest vectors above 2^16 nonces (10^7-nonce jobs,
    the reference's own job size) through the wide replay, in one call."""
    vs = [v for v in golden["scan"] if "mtest" in v["source"] and v["upper"] - v["lower"] >= SMALL]
    assert len(vs) == 3 and all(v["upper"] - v["lower"] < WIDE_MAX for v in vs)
    got, info = emu_wide([(bytes.fromhex(v["msg_hex"]), v["lower"], v["upper"]) for v in vs])
    assert got == [(v["hash"], v["nonce"]) for v in vs]
    assert info["wide"] == 3 and info["launches"] == 1


def test_emu_wide_mixed_routes_and_limit(oracle_mod):
    reqs = [(b"small", 990, 1010), (b"bradfitz", 0, 99999), (b"none", 7, 6)]
    got, info = emu_wide(reqs)
    assert got == [oracle_mod.scan(m, lo, hi) for m, lo, hi in reqs] and (info["small"], info["wide"]) == (1, 1)
    r = subprocess.run([EMU, "wide"], input=f"6d7367 0 {WIDE_MAX}\n", capture_output=True, text=True)
    assert r.returncode == 1 and "2^24" in r.stderr
