"""p1hip_scan_below_batch_wide without a GPU: the new entry points and their
argument checks, the routes and the slot rule (p1hip_below_wide_layout), and
the host replay `tools/batch_emu beloww` -- the library's own routes, round
items, groups, slot rule, filter tables, candidate mapping, refine tables and
decoder (p1_amd/csrc/beloww_plan.hpp), k_scan tile by tile, the per-thread
function k_beloww_filter shares, below_thread per simulated thread -- against
the reference loop, brute force by the oracle.  Equality is exact;
tests/test_gpu_below_wide.py runs the same lists on the device."""
import ctypes
import os
import re
import subprocess

import pytest

import below_wide_cases
from below_cases import FLOOR, U64_MAX
from conftest import ROOT, host_bin

EMU = host_bin(os.path.join(ROOT, "tools", "batch_emu"))
ERR_ARGS = -4
BRADFITZ = b"bradfitz"


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(EMU):
        subprocess.run(["make", "-s", "-C", ROOT, "tools/batch_emu"], check=True)


def emu(reqs, ndev=1, check=True, **opts):
    """-> ([[(hash, nonce)]] per request, the replay's counters), or the
    failed process when `check` is off.  opts: batch_emu beloww's name=value."""
    text = "".join(f"{m.hex() or '-'} {lo} {hi} {t} {cap}\n" for m, lo, hi, t, cap in reqs)
    args = [EMU, "beloww", str(ndev)] + [f"{k}={v}" for k, v in opts.items()]
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


@pytest.fixture
def knobs(monkeypatch):
    """The library's test knobs are honoured, and the ones this file sets are clear."""
    monkeypatch.setenv("P1HIP_TEST_KNOBS", "1")
    for k in ("P1HIP_BELOW_PATH", "P1HIP_BELOW_MAX_SLICE", "P1HIP_BELOW_WIDE_MAX_SLOTS", "P1HIP_WIDE_MIN_FAST_THREADS",
              "P1HIP_WIDE_MAX_SEGS"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


# ---------------------------------------------------------------------------
# Symbols, ABI, errors
# ---------------------------------------------------------------------------
def test_symbols_and_abi():
    import p1_amd
    from p1_amd import _lib

    for name in ("scan_below_batch_wide", "below_wide_layout", "get_below_wide_stats", "below_filter",
                 "beloww_codeobj_sha256"):
        assert callable(getattr(p1_amd, name))
    assert p1_amd.abi_version() == 6 == p1_amd.ABI_VERSION
    assert p1_amd.version() == "p1hip 0.6 gfx950"
    before = p1_amd.device_count()  # 0 unless an earlier test of the session opened one
    assert p1_amd.scan_below_batch_wide([]) == []
    # requests that are all empty are answered on the host as well
    assert p1_amd.scan_below_batch_wide([(b"msg", 5, 4, U64_MAX, 3), (b"msg", 0, 9, U64_MAX, 0)]) == [[], []]
    assert p1_amd.device_count() == before  # neither call opened a device
    assert p1_amd.below_wide_layout([], 2) == []
    new = p1_amd.beloww_codeobj_sha256()
    assert len(new) == 64 and new not in (p1_amd.codeobj_sha256(), p1_amd.batch_codeobj_sha256(),
                                          p1_amd.below_codeobj_sha256(), p1_amd.belowb_codeobj_sha256())
    assert p1_amd.BELOW_WIDE_MAX_NONCES == 1 << 24 and p1_amd.BELOW_WIDE_ROUTES[3] == "filtered"
    # the struct as the header declares it: 20 counters and the wall time
    with open(os.path.join(ROOT, "include", "p1hip.h")) as f:
        body = re.search(r"typedef struct \{([^}]*)\} p1hip_below_wide_stats_t;", f.read()).group(1)
    fields = re.findall(r"^\s*(?:uint64_t|double) (\w+);", body, re.M)
    assert fields == [k for k, _ in _lib.BelowWideStats._fields_] and len(fields) == 21
    assert ctypes.sizeof(_lib.BelowWideStats) == 21 * 8
    s = p1_amd.get_below_wide_stats()
    assert set(s) == set(fields)


def raw_call(caps, hits_len, spoil=None):
    """p1hip_scan_below_batch_wide on requests [0, 2] of b"msg" with these caps;
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
    rc = lib.p1hip_scan_below_batch_wide(arr, len(caps), hits, hits_len, found)
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


def test_caps_above_hits_len_and_caps_overflow():
    rc, err, untouched = raw_call([3, 3, 3], 8)
    assert rc == ERR_ARGS and "hits_len" in err and untouched, err
    # exactly hits_len is legal as far as the arguments go: the same call with an empty range everywhere
    def empty(arr):
        for r in arr:
            r.lower, r.upper = 5, 4
    rc, err, _ = raw_call([3, 3, 2], 8, empty)
    assert rc == 0, err
    rc, err, untouched = raw_call([1 << 63, 1, 1 << 63], (1 << 64) - 1)
    assert rc == ERR_ARGS and "overflow" in err and untouched, err


def test_layout_argument_errors():
    import p1_amd

    with pytest.raises(p1_amd.P1HipError) as e:
        p1_amd.below_wide_layout([(b"m", 0, 9, 5, 1)], 0)
    assert e.value.rc == ERR_ARGS


# ---------------------------------------------------------------------------
# Routes and the slot rule
# ---------------------------------------------------------------------------
def test_route_boundaries_and_slots(knobs):
    """cap = 1 over [0, 2^40]: the slice rule asks for 2 * 2^64 / (target + 1)
    nonces, so target 2^41 - 1 gives the longest filtered slice (2^24), 2^40 one
    of 2^25 (individual), 2^46 - 1 the shortest sparse one (2^19) and 2^46 the
    dense one p1hip_scan_below_batch coalesces.  A hard target is clamped by its
    range: 2^24 nonces are filtered, one more is individual.
    Slots: 16 + 4 * ceil(len * (target + 1) / 2^64), at most the tile count."""
    import p1_amd

    hi = 1 << 40
    lo24 = 10 ** 9
    reqs = [
        (BRADFITZ, 0, hi, (1 << 41) - 1, 1), (BRADFITZ, 0, hi, 1 << 40, 1), (BRADFITZ, 0, hi, (1 << 46) - 1, 1),
        (BRADFITZ, 0, hi, 1 << 46, 1), (BRADFITZ, lo24, lo24 + (1 << 24) - 1, 1 << 32, 1),
        (BRADFITZ, lo24, lo24 + (1 << 24), 1 << 32, 1), (BRADFITZ, 9, 3, 1 << 32, 1), (BRADFITZ, 0, hi, 1 << 32, 0),
        (BRADFITZ, lo24, lo24 + (1 << 16), 1 << 40, 1), (BRADFITZ, lo24, lo24 + (1 << 16) - 1, 1 << 40, 1),
    ]
    lay = p1_amd.below_wide_layout(reqs, 1)
    assert [x["route"] for x in lay] == ["filtered", "individual", "filtered", "coalesced", "filtered", "individual",
                                         "empty", "empty", "filtered", "coalesced"]
    # the same requests as p1hip_scan_below_batch routes them: filtered ones are individual there
    old = p1_amd.below_batch_layout(reqs, 1)
    assert [x["route"] for x in old] == ["individual", "individual", "individual", "coalesced", "individual",
                                         "individual", "empty", "empty", "individual", "coalesced"]
    assert [x["tiles"] for x in lay][3] == old[3]["tiles"] and lay[3]["slots"] == 1 and lay[9]["slots"] == 1
    # expected hits 2, 2, 2^-8, 2^-8 (rounded up to 1): 24, 24, 20, 20 slots
    assert [lay[i]["slots"] for i in (0, 2, 4, 8)] == [24, 24, 20, 20]
    assert all(lay[i]["tiles"] > lay[i]["slots"] and lay[i]["device"] == 0 for i in (0, 2, 4, 8))
    assert all(lay[i]["device"] == -1 and lay[i]["tiles"] == 0 == lay[i]["slots"] for i in (1, 5, 6, 7))
    # several devices: contiguous groups, a request wholly on one device
    lay = p1_amd.below_wide_layout([(b"w%d" % i, 0, 2 ** 32, 1 << 44, 1) for i in range(12)], 3)
    assert [x["device"] for x in lay] == [0] * 4 + [1] * 4 + [2] * 4
    # 2^21 nonces at (2^44 + 1) / 2^64 per nonce: a little above 2 expected hits, rounded up to 3
    assert all(x["route"] == "filtered" and x["slots"] == 16 + 4 * 3 for x in lay)


def test_slots_are_clamped_by_the_tile_count(knobs):
    """Forced sparse, shorter slices are filtered too: 3000 nonces at target
    UINT64_MAX expect 3000 hits, 12016 slots by the rule, and have far fewer
    tiles; the test knob caps the slots below that."""
    import p1_amd

    knobs.setenv("P1HIP_BELOW_PATH", "1")
    req = [(BRADFITZ, 10 ** 6, 10 ** 6 + 2999, U64_MAX, 5000)]
    lay = p1_amd.below_wide_layout(req, 1)[0]
    assert lay["route"] == "filtered" and 1 < lay["tiles"] <= 13 and lay["slots"] == lay["tiles"]
    knobs.setenv("P1HIP_BELOW_WIDE_MAX_SLOTS", "1")
    assert p1_amd.below_wide_layout(req, 1)[0]["slots"] == 1
    knobs.delenv("P1HIP_BELOW_PATH")
    assert p1_amd.below_wide_layout(req, 1)[0]["route"] == "coalesced"  # at most 2^16 nonces are dense


# ---------------------------------------------------------------------------
# Parity
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("forced", [False, True])
@pytest.mark.parametrize("ndev", [1, 3])
def test_mixed(oracle_mod, ndev, forced):
    reqs, want, filtered = below_wide_cases.mixed(oracle_mod, forced)
    assert filtered >= 4 and sum(lo > hi or cap == 0 for _, lo, hi, _, cap in reqs) == 3
    opts = dict(floor=FLOOR, path=1) if forced else dict(floor=FLOOR)
    out, info = emu(reqs, ndev, **opts)
    assert out == want
    assert info["filtered"] == filtered and info["empty"] == 3 and info["coalesced"] == len(reqs) - 3 - filtered
    assert info["groups"] == 1 and info["launches"] == ndev and info["overflows"] == 0
    assert info["candidates"] >= filtered and info["marks"] == ndev
    sparse = [(lo, hi) for _, lo, hi, t, cap in reqs if lo <= hi and cap and (forced or (t < 1 << 46 and hi - lo >= 1 << 16))]
    assert len(sparse) == filtered
    if forced:
        # easier targets: a request that asks for few hits has a first slice shorter than its range
        assert info["rounds"] == 1 and info["pairs"] == 0 and info["scan_nonces"] < sum(hi - lo + 1 for lo, hi in sparse)
    else:
        # every filtered request's one slice is its whole range
        assert info["scan_nonces"] == sum(hi - lo + 1 for lo, hi in sparse)
        assert info["pairs"] >= 1 and info["dense_rounds"] == info["rounds"]


def test_mixed_ranges_span_several_launches(oracle_mod):
    """Two segments per k_scan launch: a request's pieces land in different launches."""
    reqs, want, _ = below_wide_cases.mixed(oracle_mod, True)
    out, info = emu(reqs, 1, floor=FLOOR, path=1, maxsegs=2)
    one, info1 = emu(reqs, 1, floor=FLOOR, path=1)
    assert out == want == one
    assert info["launches"] > 4 * info1["launches"] and info["tiles"] == info1["tiles"] and info["slots"] == info1["slots"]


@pytest.mark.parametrize("forced", [False, True])
def test_rounds(oracle_mod, forced):
    """A slice cap of 200000 on requests of 564000 nonces: three rounds, a group in
    each, requests that have their cap leave early."""
    reqs, want, filtered = below_wide_cases.mixed(oracle_mod, forced)
    opts = dict(floor=FLOOR, path=1) if forced else dict(floor=FLOOR)
    out, info = emu(reqs, 2, maxslice=200000, **opts)
    assert out == want
    assert info["rounds"] == 3 == info["groups"] and info["filtered"] == filtered


def test_last_slice_turns_dense(oracle_mod):
    """Slices of 250000, 250000 and 64000 nonces of a filtered request: the third
    has fallen to at most 2^16 and goes through the dense launch pair."""
    E = next(E for E in below_wide_cases.cells(oracle_mod) if E.nth(1) < 1 << 46)
    req = [(E.msg, E.lo, E.hi, E.nth(1), 100)]
    out, info = emu(req, 1, floor=FLOOR, maxslice=250000)
    assert out == [E.below(E.nth(1))] and len(out[0]) == 2
    assert info["filtered"] == 1 and info["coalesced"] == 0
    assert info["rounds"] == 3 and info["groups"] == 2 and info["pairs"] == 1 and info["dense_rounds"] == 1
    assert info["scan_nonces"] == 500000


def test_every_tile_a_candidate_and_the_overflow_fallback(oracle_mod):
    """Forced sparse at target UINT64_MAX: every tile is a candidate and every
    nonce a hit.  The slot rule gives such a request a slot per tile (expected
    hits = nonces), so nothing overflows; under a slot cap of 1 the filter
    reports more candidates than slots and the host filter answers."""
    E = below_wide_cases.small(oracle_mod)
    reqs = [(BRADFITZ, 10 ** 6 - 1500, 10 ** 6 + 1499, U64_MAX, 5000), (E.msg, E.lo, E.hi, E.nth(3), 10)]
    want = [[(int(h), 10 ** 6 - 1500 + i) for i, h in enumerate(oracle_mod.hashes(BRADFITZ, 10 ** 6 - 1500, 3000))],
            E.below(E.nth(3))]
    out, info = emu(reqs, 1, path=1)
    assert out == want and len(out[0]) == 3000
    assert info["overflows"] == 0 and info["slots"] >= info["candidates"] >= 3
    out, info1 = emu(reqs, 1, path=1, maxslots=1)
    assert out == want
    assert info1["overflows"] == 1 and info1["slots"] == 2 and info1["candidates"] == info["candidates"]


def test_deferral_into_further_groups(oracle_mod):
    """A device's partial array of 230 tiles: of the twelve slices (301 tiles) of
    the forced-sparse list the one of 223 tiles finds no room behind its
    predecessors and runs in a second group of the same round."""
    reqs, want, filtered = below_wide_cases.mixed(oracle_mod, True)
    out, info = emu(reqs, 1, floor=FLOOR, path=1, maxtiles=230)
    assert out == want
    assert info["rounds"] == 1 and info["groups"] == 2 and info["tiles"] == 301 and info["filtered"] == filtered
    # a slice that fits no group is an error, not a loop
    r = emu(reqs, 1, check=False, floor=FLOOR, path=1, maxtiles=100)
    assert r.returncode == 1 and "does not fit" in r.stderr


def test_kept_checks_refuse_corrupted_values(oracle_mod):
    E = below_wide_cases.cells(oracle_mod)[0]
    target = E.nth(7)
    req = [(E.msg, E.lo, E.hi, target, 100)]
    out, info = emu(req, 1, floor=FLOOR, path=1)
    assert out == [E.below(target)] and info["candidates"] >= 2
    # candidate slot 0 names the next tile: its partial is above the target (were it a candidate, it would be slot 1)
    r = emu(req, 1, check=False, floor=FLOOR, path=1, corrupt=0)
    assert r.returncode == 1 and ("its partial is above the target" in r.stderr or "out of table order" in r.stderr), r.stderr
    # the last candidate slot moved past the request's last range
    r = emu(req, 1, check=False, floor=FLOOR, path=1, corrupt=info["candidates"] - 1)
    assert r.returncode == 1 and "check" in r.stderr, r.stderr
    # mark bit 0: the first nonce of the first candidate tile is marked (its hash is above the target), or, if it
    # was the tile's hit, unmarked (the refinement no longer has the tile's partial as its minimum)
    r = emu(req, 1, check=False, floor=FLOOR, path=1, corrupt="m0")
    assert r.returncode == 1 and ("mark check" in r.stderr or "tile check" in r.stderr), r.stderr
