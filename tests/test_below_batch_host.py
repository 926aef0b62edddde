"""p1hip_scan_below_batch without a GPU: the new entry points and their argument
checks, the routes (p1hip_below_batch_layout), and the host replay
`tools/batch_emu below` -- the library's own routes, rounds, round layout with
its slot cap, tables and decoder (p1_amd/csrc/belowb_plan.hpp), below_thread
per simulated thread and the word expansion k_belowb_collect shares -- against
the reference loop, brute force by the oracle.  Equality is exact;
tests/test_gpu_below_batch.py runs the same matrix on the device."""
import ctypes
import os
import subprocess

import pytest

import below_batch_cases
from below_cases import U64_MAX
from conftest import ROOT, host_bin

EMU = host_bin(os.path.join(ROOT, "tools", "batch_emu"))
ERR_ARGS = -4
BRADFITZ = b"bradfitz"


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(EMU):
        subprocess.run(["make", "-s", "-C", ROOT, "tools/batch_emu"], check=True)


def emu(reqs, ndev=1, maxslice=None, corrupt=None, check=True):
    """-> ([[(hash, nonce)]] per request, the replay's counters), or the
    failed process when `check` is off."""
    text = "".join(f"{m.hex() or '-'} {lo} {hi} {t} {cap}\n" for m, lo, hi, t, cap in reqs)
    args = [EMU, "below", str(ndev)]
    if maxslice:
        args.append(f"maxslice={maxslice}")
    if corrupt is not None:
        args.append(f"corrupt={corrupt}")
    r = subprocess.run(args, input=text, capture_output=True, text=True, timeout=600)
    if not check:
        return r
    assert r.returncode == 0, r.stderr
    out = []
    for line in r.stdout.splitlines():
        f = line.split()
        hits = [tuple(int(x) for x in h.split(":")) for h in f[1:]]
        assert int(f[0]) == len(hits)
        out.append(hits)
    info = dict((k, int(v)) for k, v in (kv.split("=") for kv in r.stderr.split()))
    return out, info


# ---------------------------------------------------------------------------
# Symbols, ABI, errors
# ---------------------------------------------------------------------------
def test_symbols_and_abi():
    import p1_amd

    for name in ("scan_below_batch", "below_batch_layout", "get_below_batch_stats", "below_collect",
                 "belowb_codeobj_sha256"):
        assert callable(getattr(p1_amd, name))
    assert p1_amd.abi_version() == 6 == p1_amd.ABI_VERSION
    assert p1_amd.version() == "p1hip 0.6 gfx950"
    before = p1_amd.device_count()  # 0 unless an earlier test of the session opened one
    assert p1_amd.scan_below_batch([]) == []
    # requests that are all empty are answered on the host as well
    assert p1_amd.scan_below_batch([(b"msg", 5, 4, U64_MAX, 3), (b"msg", 0, 9, U64_MAX, 0)]) == [[], []]
    assert p1_amd.device_count() == before  # neither call opened a device
    assert p1_amd.below_batch_layout([], 2) == []
    new = p1_amd.belowb_codeobj_sha256()
    assert len(new) == 64 and new not in (p1_amd.codeobj_sha256(), p1_amd.batch_codeobj_sha256(),
                                          p1_amd.below_codeobj_sha256())
    assert p1_amd.BELOW_BATCH_MAX_NONCES == 1 << 20 and p1_amd.BELOW_BATCH_MAX_SLOTS == 1 << 22


def raw_call(caps, hits_len, spoil=None):
    """p1hip_scan_below_batch on requests [0, 2] of b"msg" with these caps;
    -> (rc, error text, outputs untouched?).  Every case here must fail before
    anything runs: this machine has no device."""
    import p1_amd
    from p1_amd import _lib

    lib = p1_amd.load()
    arr = (_lib.BelowRequest * len(caps))()
    for r, cap in zip(arr, caps):
        r.msg, r.msg_len, r.lower, r.upper, r.target, r.cap = b"msg", 3, 0, 2, U64_MAX, cap
    if spoil:
        spoil(arr)
    nhits = 8
    hits = (_lib.Result * nhits)()
    for h in hits:
        h.hash, h.nonce = 111, 222
    found = (ctypes.c_size_t * len(caps))(*([333] * len(caps)))
    rc = lib.p1hip_scan_below_batch(arr, len(caps), hits, hits_len, found)
    untouched = all((h.hash, h.nonce) == (111, 222) for h in hits) and all(f == 333 for f in found)
    return rc, lib.p1hip_last_error().decode(), untouched


@pytest.mark.parametrize("bad", ["null_msg", "too_long"])
def test_bad_request_is_named_before_anything_runs(bad):
    def spoil(arr):
        if bad == "null_msg":
            arr[2].msg, arr[2].msg_len = None, 5
        else:
            arr[2].msg_len = (1 << 28) + 1  # P1HIP_MAX_MSG_LEN + 1 (checked, never read)

    rc, err, untouched = raw_call([1, 1, 1, 1], 8, spoil)
    assert rc == ERR_ARGS and "request 2" in err and untouched, err


def test_caps_above_hits_len():
    rc, err, untouched = raw_call([3, 3, 3], 8)
    assert rc == ERR_ARGS and "hits_len" in err and untouched, err
    # exactly hits_len is legal as far as the arguments go: the same call with an empty range everywhere
    def empty(arr):
        for r in arr:
            r.lower, r.upper = 5, 4
    rc, err, _ = raw_call([3, 3, 2], 8, empty)
    assert rc == 0, err


def test_caps_overflow():
    rc, err, untouched = raw_call([1 << 63, 1, 1 << 63], (1 << 64) - 1)
    assert rc == ERR_ARGS and "overflow" in err and untouched, err
    rc, err, untouched = raw_call([(1 << 64) - 1, 1], (1 << 64) - 1)
    assert rc == ERR_ARGS and "overflow" in err and untouched, err


def test_layout_argument_errors():
    import p1_amd

    with pytest.raises(p1_amd.P1HipError) as e:
        p1_amd.below_batch_layout([(b"m", 0, 9, 5, 1)], 0)
    assert e.value.rc == ERR_ARGS


# ---------------------------------------------------------------------------
# Routes
# ---------------------------------------------------------------------------
def test_route_boundaries():
    """The 2^20 limit admits cap = 1 at every dense target and cap = 2 at the
    switch target 2^46; a sparse first slice is never coalesced; at most 2^16
    nonces are dense whatever the target."""
    import p1_amd

    lo, hi, T = 10 ** 9, 10 ** 9 + (1 << 23) - 1, 1 << 46
    reqs = [
        (BRADFITZ, lo, hi, T, 1), (BRADFITZ, lo, hi, T, 2), (BRADFITZ, lo, hi, T, 3), (BRADFITZ, lo, hi, T - 1, 1),
        (BRADFITZ, lo, lo + (1 << 16) - 1, 1 << 40, 1), (BRADFITZ, lo, lo + (1 << 16), 1 << 40, 1),
        (BRADFITZ, 9, 3, T, 1), (BRADFITZ, lo, hi, T, 0),
    ]
    lay = p1_amd.below_batch_layout(reqs, 1)
    assert [x["route"] for x in lay] == ["coalesced", "coalesced", "individual", "individual", "coalesced",
                                         "individual", "empty", "empty"]
    # the first slices: 2^19 and 2^20 nonces from 10^9 on (one decade), 2^16
    assert [x["tiles"] for x in lay] == [1 << 11, 1 << 12, 0, 0, 1 << 8, 0, 0, 0]
    assert [x["device"] for x in lay] == [0, 0, -1, -1, 0, -1, -1, -1]
    # contiguous groups by tile count, a request wholly on one device
    lay = p1_amd.below_batch_layout([(b"w%d" % i, 0, 2 ** 32, 1 << 56, 1) for i in range(12)], 3)
    assert [x["device"] for x in lay] == [0] * 4 + [1] * 4 + [2] * 4
    # the first slice is [0, 2^16): five decade pieces, each starting a tile of its own
    pieces = [(0, 9), (10, 99), (100, 999), (1000, 9999), (10000, 65535)]
    assert all(x["route"] == "coalesced" and x["tiles"] == sum((b - a) // 256 + 1 for a, b in pieces) for x in lay)


def test_slot_cap_closes_a_launch_pair():
    """Five requests of 2^20 slots each: four fill the 2^22 slots of a launch
    pair, the fifth opens the next (their tiles are far below the tile cap)."""
    n = 1 << 20
    reqs = [(b"slots %d" % i, 10 ** 9, 10 ** 9 + n - 1, 1 << 46, n) for i in range(5)]
    out, info = emu(reqs)
    assert info["launches"] == 2 and info["rounds"] == 1 and info["slots"] == 5 * n and info["tiles"] == 5 * 4096
    assert all(len(h) < 8 for h in out)  # 2^20 nonces at 2^-18 per nonce
    out4, info4 = emu(reqs[:4])
    assert info4["launches"] == 1 and out4 == out[:4]


# ---------------------------------------------------------------------------
# Parity
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("ndev", [1, 3])
def test_matrix(oracle_mod, ndev):
    reqs, want = below_batch_cases.matrix(oracle_mod)
    assert len(reqs) == 150
    # every target kind met every cap kind, and the fixed edge cases are in
    assert {c for *_, c in reqs} >= {0, 1, 3} and {t for *_, t, _ in reqs} >= {0, U64_MAX}
    assert any(lo > hi for _, lo, hi, _, _ in reqs) and any(hi == U64_MAX for _, _, hi, _, _ in reqs)
    assert any(len(w) == c > 3 for w, (*_, c) in zip(want, reqs)) and any(3 < len(w) < c for w, (*_, c) in zip(want, reqs))
    out, info = emu(reqs, ndev)
    assert out == want
    assert info["rounds"] == 1 and info["launches"] == ndev
    assert info["coalesced"] + info["empty"] == 150 and info["empty"] == sum(lo > hi or c == 0 for _, lo, hi, _, c in reqs)


def rounds_needed(req, want):
    """Slices of 1000 nonces until the request has its cap or its range ends."""
    _, lo, hi, _, cap = req
    if lo > hi or cap == 0:
        return 0, 0
    tiles = 0
    for r in range(1, 100):
        end = min(lo + 1000 * r - 1, hi)
        tiles += slice_tiles(lo + 1000 * (r - 1), end)
        if end == hi or sum(n <= end for _, n in want) == cap:
            return r, tiles


def slice_tiles(lo, hi):
    """Every decade piece of [lo, hi] starts a tile of its own."""
    pieces = [(max(lo, 10 ** (d - 1) if d > 1 else 0), min(hi, 10 ** d - 1)) for d in range(1, 21)]
    return sum((b - a) // 256 + 1 for a, b in pieces if a <= b)


def test_rounds(oracle_mod):
    """A slice cap of 1000 on requests of up to 5000 nonces: requests finish in
    different rounds, and a finished request leaves the later rounds."""
    reqs, want = below_batch_cases.rounds(oracle_mod)
    out, info = emu(reqs, 2, maxslice=1000)
    assert out == want
    need = [rounds_needed(q, w) for q, w in zip(reqs, want)]
    assert info["rounds"] == max(r for r, _ in need) == 5 and len({r for r, _ in need}) >= 4
    # every request takes part in exactly the rounds it needs
    assert info["tiles"] == sum(t for _, t in need) and info["launches"] > info["rounds"]
    one, info1 = emu(reqs, 1)
    assert one == want and info1["rounds"] == 1


def test_decoder_refuses_a_corrupted_index():
    reqs = [(BRADFITZ, 0, 99999, 300000000000000, 5), (b"msg", 0, 4, U64_MAX, 5)]
    out, _ = emu(reqs)
    assert out[0] == [(158752571039048, 91989), (85364550342847, 98985)] and [n for _, n in out[1]] == [0, 1, 2, 3, 4]
    # slot 0: bradfitz's first hit moved to the next nonce, whose hash is above the target
    r = emu(reqs, corrupt=0, check=False)
    assert r.returncode == 1 and "its hash is above the target" in r.stderr
    # slot 5: the other request's nonce 0 becomes nonce 1, and nonce 1 follows: not increasing
    r = emu(reqs, corrupt=5, check=False)
    assert r.returncode == 1 and "out of order" in r.stderr
    # slot 9: its nonce 4 becomes thread 5 of a piece of 5 nonces
    r = emu(reqs, corrupt=9, check=False)
    assert r.returncode == 1 and "past its piece" in r.stderr
