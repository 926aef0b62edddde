"""p1hip_scan_batch without a GPU: the new entry points and their argument
checks, the layout of a batch over devices and launch pairs
(p1hip_batch_layout, the function p1hip_scan_batch itself lays out with), and
the host replay tools/batch_emu -- the library's own table builder and
segment lookup, generic_thread per simulated thread, the per-request fold --
against the oracle and the golden fixtures.

Reference: miner.go:56-63 (each request's answer is that loop's)."""
import ctypes
import os
import subprocess

import pytest

from batch_cases import U64_MAX, random_requests
from conftest import ROOT, host_bin

EMU = host_bin(os.path.join(ROOT, "tools", "batch_emu"))
SMALL = 1 << 16


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(EMU):
        subprocess.run(["make", "-s", "-C", ROOT, "tools/batch_emu"], check=True)


def emu(reqs, ndev=1, max_tiles=None):
    """[(hash, nonce)] per request and the replay's {launches, tiles, segs}."""
    text = "".join(f"{m.hex() or '-'} {lo} {hi}\n" for m, lo, hi in reqs)
    args = [EMU, str(ndev)] + ([str(max_tiles)] if max_tiles else [])
    r = subprocess.run(args, input=text, capture_output=True, text=True, check=True)
    out = [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
    info = dict((k, int(v)) for k, v in (kv.split("=") for kv in r.stderr.split()))
    return out, info


@pytest.fixture(scope="module")
def batch150():
    return random_requests(150, seed=71)


def test_symbols_and_abi():
    import p1_amd

    for name in ("scan_batch", "batch_layout", "get_batch_stats"):
        assert callable(getattr(p1_amd, name))
    assert p1_amd.abi_version() == 6 == p1_amd.ABI_VERSION
    assert p1_amd.version() == "p1hip 0.6 gfx950"
    assert p1_amd.scan_batch([]) == []
    assert p1_amd.device_count() == 0  # an empty batch opens no device
    assert p1_amd.batch_layout([], 2) == []
    assert len(p1_amd.batch_codeobj_sha256()) == 64 and p1_amd.batch_codeobj_sha256() != p1_amd.codeobj_sha256()


@pytest.mark.parametrize("bad", ["null_msg", "too_long"])
def test_bad_request_is_named_before_anything_runs(bad):
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
    out = (_lib.Result * 4)()
    for o in out:
        o.hash, o.nonce = 7, 7
    with pytest.raises(p1_amd.P1HipError) as e:
        _lib._check(lib.p1hip_scan_batch(arr, 4, out))
    assert e.value.rc == -4 and "request 2" in str(e.value)
    assert all((o.hash, o.nonce) == (7, 7) for o in out)
    assert p1_amd.device_count() == 0
    tiles, dev, launch = (ctypes.c_uint32 * 4)(), (ctypes.c_int32 * 4)(), (ctypes.c_int32 * 4)()
    assert lib.p1hip_batch_layout(arr, 4, 1, tiles, dev, launch) == -4
    assert b"request 2" in lib.p1hip_last_error()
    # null arrays with n > 0
    assert lib.p1hip_scan_batch(None, 4, out) == -4 and lib.p1hip_scan_batch(arr, 4, None) == -4


def decade_tiles(lo, hi):
    """Sum over the decade pieces of [lo, hi] of ceil(count / 256)."""
    t = 0
    for d in range(1, 21):
        s, e = max(lo, 0 if d == 1 else 10 ** (d - 1)), min(hi, 10 ** d - 1, U64_MAX)
        if s <= e:
            t += -(-(e - s + 1) // 256)
    return t


def test_layout_tile_counts(batch150):
    import p1_amd

    b = 10 ** 6  # inside a decade
    reqs = [("m", b, b), ("m", b, b + 255), ("m", b, b + 256), ("m", b, b + SMALL - 1), ("m", 0, SMALL - 1),
            ("m", b, b + SMALL), ("m", 5, 4), ("m", U64_MAX - 500, U64_MAX)]
    lay = p1_amd.batch_layout(reqs, 1)
    assert [x["tiles"] for x in lay] == [1, 1, 2, 256, decade_tiles(0, SMALL - 1), 0, 0, 2]
    assert 256 <= lay[4]["tiles"] <= 262
    assert [(x["device"], x["launch"]) for x in lay] == [(0, 0)] * 5 + [(-1, -1)] * 2 + [(0, 0)]
    lay = p1_amd.batch_layout(batch150, 1)
    for (m, lo, hi), x in zip(batch150, lay):
        assert x["tiles"] == (decade_tiles(lo, hi) if lo <= hi else 0), (lo, hi)


def test_layout_devices_are_contiguous_and_balanced(batch150):
    import p1_amd

    lay = p1_amd.batch_layout([("bradfitz", 0, 9999)] * 10, 3)
    devs = [x["device"] for x in lay]
    assert devs == sorted(devs) and set(devs) == {0, 1, 2}
    counts = [devs.count(d) for d in range(3)]
    assert max(counts) - min(counts) <= 1
    assert all(x["launch"] == 0 for x in lay)
    # unequal requests: contiguous, in order, and no device more than one
    # request's tiles away from its share
    lay = [x for x in p1_amd.batch_layout(batch150, 4) if x["tiles"]]
    devs = [x["device"] for x in lay]
    assert devs == sorted(devs) and set(devs) == {0, 1, 2, 3}
    total = sum(x["tiles"] for x in lay)
    for d in range(4):
        got = sum(x["tiles"] for x in lay if x["device"] == d)
        assert abs(got - total / 4) <= max(x["tiles"] for x in lay)
    # more devices than requests: every request still has one device
    lay = p1_amd.batch_layout([("a", 0, 0), ("b", 1, 1)], 8)
    assert [x["device"] for x in lay] == sorted(x["device"] for x in lay) and all(0 <= x["device"] < 8 for x in lay)


def test_layout_launch_cap(batch150, monkeypatch):
    import p1_amd

    monkeypatch.setenv("P1HIP_TEST_KNOBS", "1")
    monkeypatch.setenv("P1HIP_BATCH_MAX_TILES", "300")
    assert p1_amd.test_knobs()["P1HIP_BATCH_MAX_TILES"] == "300"
    reqs = batch150 + [("bradfitz", 10 ** 6, 10 ** 6 + SMALL - 1)]  # 256 tiles in one request
    lay = p1_amd.batch_layout(reqs, 2)
    groups = {}
    for i, x in enumerate(lay):
        if x["tiles"]:
            groups.setdefault((x["device"], x["launch"]), []).append(i)
    assert len(groups) >= 4  # > 900 tiles in launch pairs of at most 300
    for idx in groups.values():
        assert sum(lay[i]["tiles"] for i in idx) <= 300
    # requests stay in order: (device, launch) never goes back, so every launch pair is a contiguous run
    seq = [(x["device"], x["launch"]) for x in lay if x["tiles"]]
    assert seq == sorted(seq)
    for dev in (0, 1):
        launches = sorted(l for d, l in groups if d == dev)
        assert launches == list(range(len(launches)))
    # a cap below one request's tiles is raised to it: the request is not split
    monkeypatch.setenv("P1HIP_BATCH_MAX_TILES", "100")
    lay = p1_amd.batch_layout(reqs, 1)
    assert lay[-1]["tiles"] == 256 and lay[-1]["launch"] >= 0
    # the coalescing limit: 0 runs everything individually; it is not P1HIP_SMALL_MAX_NONCES
    monkeypatch.setenv("P1HIP_BATCH_MAX_NONCES", "0")
    assert all(x["tiles"] == 0 and x["device"] == -1 for x in p1_amd.batch_layout(reqs, 1))
    monkeypatch.delenv("P1HIP_BATCH_MAX_NONCES")
    monkeypatch.setenv("P1HIP_SMALL_MAX_NONCES", "0")
    assert p1_amd.batch_layout(reqs, 1)[-1]["tiles"] == 256
    # without the master switch the knobs are ignored
    monkeypatch.delenv("P1HIP_TEST_KNOBS")
    assert {x["launch"] for x in p1_amd.batch_layout(reqs, 1)} <= {0, -1}


def test_emu_random_batch_against_oracle(batch150, oracle_mod):
    want = [oracle_mod.scan(m, lo, hi) for m, lo, hi in batch150]
    got, info = emu(batch150)
    assert got == want
    assert info["launches"] == 1
    assert info["tiles"] == sum(decade_tiles(lo, hi) for m, lo, hi in batch150 if lo <= hi)
    # the same requests over 3 devices and capped launch pairs: other tables, same answers
    got3, info3 = emu(batch150, ndev=3, max_tiles=40)
    assert got3 == want and info3["launches"] > 6 and info3["tiles"] == info["tiles"]
    # reversed: every request's answer is its own
    assert emu(batch150[::-1])[0] == want[::-1]


def test_emu_golden(golden):
    """The golden mtest vector that fits a coalesced request (the other three
    are above 2^16 nonces), every other golden scan that fits, and every
    golden hash as a one-nonce request, all in one batch."""
    reqs, want = [], []
    for v in golden["scan"]:
        if v["upper"] - v["lower"] < SMALL:  # also the empty ranges
            reqs.append((bytes.fromhex(v["msg_hex"]), v["lower"], v["upper"]))
            want.append((v["hash"], v["nonce"]))
    assert sum("mtest" in v["source"] and v["upper"] - v["lower"] < SMALL for v in golden["scan"]) >= 1
    for v in golden["hash"]:
        reqs.append((bytes.fromhex(v["msg_hex"]), v["nonce"], v["nonce"]))
        want.append((v["hash"], v["nonce"] if v["hash"] != U64_MAX else 0))
    got, _ = emu(reqs)
    assert got == want


def test_emu_refuses_a_request_above_the_limit():
    r = subprocess.run([EMU], input=f"6d7367 0 {SMALL}\n", capture_output=True, text=True)
    assert r.returncode == 1 and "2^16" in r.stderr
