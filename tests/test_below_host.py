"""p1hip_scan_below replayed on the host: `p1emu ... below=` runs the whole
call with the library's own slices, routes, candidate filter, refine tables
and mark decoder (p1_amd/csrc/below_plan.hpp), the packed-plan replay of
k_scan for a sparse slice's partials and k_below_mark's per-thread function
for the marks.  The expected list is the reference loop, brute force by the
oracle, and equality is exact; tests/test_gpu_below.py runs the same matrix on
the device."""
import concurrent.futures as cf
import os
import subprocess

import pytest

import below_cases
import tile_cases
from below_cases import U64_MAX, Expect, increasing, resume_chain
from conftest import ROOT, host_bin

EMU = host_bin(os.path.join(ROOT, "tools", "p1emu"))
SIZE_MAX = U64_MAX


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(EMU):
        subprocess.run(["make", "-s", "-C", ROOT, "tools/p1emu"], check=True)


def emu_below(msg, lo, hi, target, cap=1, path=None, maxslice=None, floor=None, flags=()):
    """-> ([(hash, nonce)], stats) of one replayed call."""
    args = [EMU, msg.hex() or "-", str(lo), str(hi), f"below={target}", f"cap={cap}"]
    if path:
        args.append(f"path={path}")
    if maxslice:
        args.append(f"maxslice={maxslice}")
    if floor is not None:
        args.append(f"minthreads={floor}")
    r = subprocess.run(args + list(flags), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (args[2:], r.stderr)
    lines = r.stdout.splitlines()
    assert lines and lines[-1].startswith("below "), r.stdout
    stats = {k: int(v) for k, v in (kv.split("=") for kv in lines[-1].split()[1:])}
    hits = [tuple(int(x) for x in ln.split()[1:]) for ln in lines[:-1]]
    assert all(ln.startswith("hit ") for ln in lines[:-1]) and stats["found"] == len(hits)
    return hits, stats


def matrix(E, floor, routes=("sparse", "dense", None)):
    """Every property on one shape; the replays run side by side.  The full
    list always runs through both routes and the library's choice; `routes`
    are those the other properties run through (all three, or for the shapes
    of millions of nonces the library's choice alone)."""
    msg, lo, hi = E.msg, E.lo, E.hi
    n = hi - lo + 1
    target = E.nth(7)
    want = E.below(target)
    assert len(want) >= min(8, n) and increasing(want)
    mid = want[len(want) // 2]
    jobs = {}  # name -> (callable, expected)

    def one(name, expected, *a, **kw):
        jobs[name] = (lambda: emu_below(msg, *a, floor=floor, **kw)[0], expected)

    for path in ("sparse", "dense", None):
        one(f"{path} all", want, lo, hi, target, cap=100, path=path)
    for path in routes:
        one(f"{path} cap 3", want[:3], lo, hi, target, cap=3, path=path)
        jobs[f"{path} chain"] = (
            lambda path=path: resume_chain(lambda a: emu_below(msg, a, hi, target, cap=1, path=path, floor=floor)[0],
                                           lo, hi), want)
        one(f"{path} at the target", E.below(mid[0]), lo, hi, mid[0], cap=100, path=path)
        one(f"{path} one below it", E.below(mid[0] - 1), lo, hi, mid[0] - 1, cap=100, path=path)
        one(f"{path} below the minimum", [], lo, hi, E.nth(0) - 1, cap=100, path=path)
        one(f"{path} every nonce", E.first(5), lo, hi, U64_MAX, cap=5, path=path)
    for path in ("sparse", "dense"):
        jobs[f"{path} maxslice"] = (lambda path=path: emu_below(msg, lo, hi, target, cap=100, path=path,
                                                                maxslice=100000, floor=floor), None)
    with cf.ThreadPoolExecutor(8) as ex:
        got = dict(zip(jobs, ex.map(lambda j: j[0](), jobs.values())))
    assert mid in E.below(mid[0]) and mid not in E.below(mid[0] - 1)
    assert len(E.below(target, cap=3)) == min(3, len(want))
    for name, (_, expected) in jobs.items():
        if expected is not None:
            assert got[name] == expected, name
    for path in ("sparse", "dense"):
        hits, stats = got[f"{path} maxslice"]
        assert hits == want, path
        assert stats["slices"] == (n - 1) // 100000 + 1 and stats[path] == stats["slices"] and stats["examined"] == n


_EXPECT = {}


def expect(oracle, case):
    if case not in _EXPECT:
        _EXPECT[case] = Expect(oracle, *case)
    return _EXPECT[case]


@pytest.mark.parametrize("i", range(len(below_cases.K3_QS)))
def test_below_matrix_k3_cells(oracle_mod, i):
    """One tail block, TRAIL, MODE 7, MODE 5 at k = 2 and 3, a PRE cell."""
    matrix(expect(oracle_mod, below_cases.k3_selection()[i]), below_cases.FLOOR)


@pytest.mark.parametrize("i", range(len(below_cases.mode5_k45_all())))
def test_below_matrix_mode5_strided_tiles(oracle_mod, i):
    """MODE 5 with k = 4 and 5: tiles of several strided runs."""
    case = below_cases.mode5_k45_all()[i]
    matrix(expect(oracle_mod, case), 1, routes=("sparse", "dense", None) if case[2] - case[1] < 10 ** 6 else (None,))
    E = expect(oracle_mod, case)
    _, stats = emu_below(*case, E.nth(7), cap=100, path="sparse", floor=1)
    assert stats["candidate_tiles"] >= 1 and stats["mark_nonces"] < stats["scan_nonces"]
    assert stats["mark_nonces"] % 1000 == 0  # whole runs of 1000 nonces, not the ragged generic tiles


@pytest.mark.parametrize("i", range(len(tile_cases.SMALL_RANGES)))
def test_below_matrix_small_ranges(oracle_mod, i):
    """1, 256, 257 and 2^16 nonces, and a range that straddles a decade."""
    matrix(expect(oracle_mod, tile_cases.SMALL_RANGES[i]), None)


def test_below_matrix_queue_range(oracle_mod):
    """The library's own occupancy floor: k = 1 tiles of 2560 nonces."""
    matrix(expect(oracle_mod, tile_cases.QUEUE_RANGES[0]), None)


def test_below_candidates_are_the_tiles_at_or_below_the_target(oracle_mod):
    """A sparse slice refines only its candidates: k = 3 tiles of 256000
    nonces, so 8 hits mark at most 8 tiles of them and the generic edges."""
    E = expect(oracle_mod, below_cases.k3_selection()[0])
    hits, stats = emu_below(E.msg, E.lo, E.hi, E.nth(7), cap=100, path="sparse", floor=below_cases.FLOOR)
    assert hits == E.below(E.nth(7))
    assert 1 <= stats["candidate_tiles"] <= 8 and stats["mark_launches"] == 1
    assert stats["scan_nonces"] == stats["examined"] == E.hi - E.lo + 1
    _, stats = emu_below(E.msg, E.lo, E.hi, E.nth(0) - 1, cap=100, path="sparse", floor=below_cases.FLOOR)
    assert stats["candidate_tiles"] == 0 and stats["mark_launches"] == 0 and stats["mark_nonces"] == 0


def test_below_last_nonce_of_u64(oracle_mod):
    """upper == 2^64 - 1 is scanned inclusively, and nonce 2^64 - 1 can be a hit."""
    E = expect(oracle_mod, (b"edge of u64", U64_MAX - 299_999, U64_MAX))
    matrix(E, below_cases.FLOOR)
    last = E.last(1)[0][0]
    tail = E.below(last, lower=U64_MAX - 999)
    assert tail[-1][1] == U64_MAX
    for path in ("sparse", "dense", None):
        kw = dict(path=path, floor=below_cases.FLOOR)
        assert emu_below(E.msg, U64_MAX - 999, U64_MAX, last, cap=2000, **kw)[0] == tail
        assert emu_below(E.msg, U64_MAX - 2, U64_MAX, U64_MAX, cap=5, **kw)[0] == E.last(3)
        assert emu_below(E.msg, U64_MAX, U64_MAX, last, cap=1, **kw)[0] == E.last(1)
        assert emu_below(E.msg, U64_MAX, U64_MAX, last - 1, cap=1, **kw)[0] == []


def test_below_across_a_decade(oracle_mod):
    """A range straddling 10^6 -> 10^6 + 1 digits: both decades' fast tiles
    and the generic pieces between them, in nonce order."""
    E = expect(oracle_mod, (b"straddle", 10 ** 6 - 300_000, 10 ** 6 + 300_000))
    matrix(E, below_cases.FLOOR)
    want = E.below(E.nth(19))
    assert any(n < 10 ** 6 for _, n in want) and any(n >= 10 ** 6 for _, n in want)
    for path in ("sparse", "dense"):
        assert emu_below(E.msg, E.lo, E.hi, E.nth(19), cap=100, path=path, floor=below_cases.FLOOR)[0] == want


def test_below_empty_calls():
    assert emu_below(b"x", 5, 4, U64_MAX, cap=9) == ([], dict(found=0, slices=0, sparse=0, dense=0, examined=0,
                                                              scan_nonces=0, mark_nonces=0, candidate_tiles=0,
                                                              mark_launches=0))
    assert emu_below(b"x", 0, 100, U64_MAX, cap=0)[1]["slices"] == 0


def test_below_planner_flags_reach_the_filter(oracle_mod):
    """notable / nosplit change which variants the sparse slice runs, never the list."""
    E = expect(oracle_mod, below_cases.k3_selection()[4])  # MODE 5 at k = 3 by default
    want = E.below(E.nth(7))
    for flags in (("notable",), ("nosplit",), ("notable", "nosplit")):
        assert emu_below(E.msg, E.lo, E.hi, E.nth(7), cap=100, path="sparse", floor=below_cases.FLOOR,
                         flags=flags)[0] == want


# ---------------------------------------------------------------------------
# The slice rule and the decoder, directly
# ---------------------------------------------------------------------------
def slice_of(lo, upper, target, want, path=0, maxslice=0):
    r = subprocess.run([EMU, "-", str(lo), str(upper), f"belowslice={target},{want},{path},{maxslice}"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    tag, a, b, dense = r.stdout.split()
    assert tag == "slice" and int(a) == lo
    return int(b) - int(a) + 1, bool(int(dense))


def rule(target, want, dense):
    """2 * want * 2^64 / (target + 1) rounded up to a power of two, clamped."""
    need = -(-(2 * want << 64) // (target + 1))
    p = 1 << 16
    while p < need and p < (1 << 28 if dense else 1 << 34):
        p <<= 1
    return p


@pytest.mark.parametrize("target", [0, 1, 12345, (1 << 30) - 1, 1 << 30, (1 << 30) + 1, (1 << 46) - 1, 1 << 46,
                                    3 << 50, (1 << 63) - 1, 1 << 63, U64_MAX - 1, U64_MAX])
def test_slice_rule(target):
    """Against the rule restated in Python integers, cap (want) up to SIZE_MAX."""
    dense = target >= 1 << 46
    ranges = ((0, U64_MAX), (U64_MAX - (1 << 40), U64_MAX), (10 ** 9, 10 ** 9 + (1 << 36)))
    wants = (1, 2, 3, 1000, (1 << 34) - 1, 1 << 34, (1 << 63) - 1, 1 << 63, SIZE_MAX)
    for i, want in enumerate(wants):
        lo, upper = ranges[i % 3]
        assert slice_of(lo, upper, target, want) == (rule(target, want, dense), dense)
        assert slice_of(lo, upper, target, want, path=1) == (rule(target, want, False), False)
        assert slice_of(lo, upper, target, want, path=2) == (rule(target, want, True), True)
        assert slice_of(lo, upper, target, want, maxslice=100000) == (min(rule(target, want, dense), 100000), dense)


def test_slice_rule_at_the_ends_of_a_range():
    # what is left of the range caps the slice; at most 2^16 nonces are always marked directly
    assert slice_of(U64_MAX - 9, U64_MAX, 0, SIZE_MAX) == (10, True)
    assert slice_of(U64_MAX, U64_MAX, U64_MAX, SIZE_MAX) == (1, True)
    assert slice_of(0, (1 << 16) - 1, 5, 1) == (1 << 16, True)
    assert slice_of(0, 1 << 16, 5, 1) == ((1 << 16) + 1, False)
    assert slice_of(0, 1 << 16, 5, 1, path=1) == ((1 << 16) + 1, False)
    assert slice_of(0, 99, 5, 1, path=1) == (100, False)
    assert slice_of(0, U64_MAX, 0, SIZE_MAX) == (1 << 34, False)
    assert slice_of(0, U64_MAX, U64_MAX, 1) == (1 << 16, True)
    assert slice_of(0, U64_MAX, U64_MAX, SIZE_MAX) == (1 << 28, True)
    # the hand-out's shape: one expected hit per 2^32 nonces, twice that per slice
    assert slice_of(0, 1 << 40, (1 << 32) - 1, 1) == (1 << 33, False)


def decode(msg, lo, hi, target, thread):
    r = subprocess.run([EMU, msg.hex(), str(lo), str(hi), f"belowdecode={target},{thread}"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    return r.stdout.strip()


def test_mark_decoder_checks_every_mark(oracle_mod):
    """[0, 999] is three pieces (1, 2, 3 digits) in 1 + 1 + 4 tiles.  The true
    marks with one mark inverted: a thread past its piece, a nonce above the
    target, and a hit taken away (which only the tile check of a sparse slice
    can see: the decoder reports one hit fewer)."""
    E = Expect(oracle_mod, b"bradfitz", 0, 999)
    for target in (0, E.nth(7), U64_MAX):
        hits = E.below(target)
        miss = next(n for h, n in E.first(1000) if h > target) if target != U64_MAX else None
        assert "past its piece" in decode(E.msg, 0, 999, target, 10)            # tile 0 holds 10 nonces
        assert "past its piece" in decode(E.msg, 0, 999, target, 256 + 90)      # tile 1 holds 90
        assert "past its piece" in decode(E.msg, 0, 999, target, 5 * 256 + 132)  # 900 = 3 * 256 + 132
        if miss is not None:
            thread = miss if miss < 10 else 256 + miss - 10 if miss < 100 else 512 + miss - 100
            assert f"nonce {miss} is marked, its hash is above the target" in decode(E.msg, 0, 999, target, thread)
        if hits:
            n = hits[0][1]
            thread = n if n < 10 else 256 + n - 10 if n < 100 else 512 + n - 100
            assert decode(E.msg, 0, 999, target, thread) == f"decoded {len(hits) - 1}"


def test_python_binding_answers_empty_calls_without_a_device():
    """lower > upper and cap == 0 give nothing with rc 0 and open no device."""
    import p1_amd

    before = p1_amd.device_count()  # 0 unless an earlier test of the session opened one
    assert p1_amd.scan_below(b"x", 5, 4, U64_MAX, cap=3) == []
    assert p1_amd.scan_below(b"x", 0, 100, U64_MAX, cap=0) == []
    assert p1_amd.device_count() == before
    assert p1_amd.BELOW_MAX_SLICE == 1 << 34 and p1_amd.BELOW_MAX_SLICE_DENSE == 1 << 28
    assert p1_amd.BELOW_DENSE_TARGET == 1 << 46
    assert len(p1_amd.below_codeobj_sha256()) == 64
    assert p1_amd.below_codeobj_sha256() not in (p1_amd.codeobj_sha256(), p1_amd.batch_codeobj_sha256())
    import ctypes

    lib = p1_amd.load()
    found = ctypes.c_size_t(77)
    assert lib.p1hip_scan_below(None, 3, 0, 9, 5, 1, (p1_amd._lib.Result * 1)(), ctypes.byref(found)) == -4
    assert lib.p1hip_scan_below(b"x", 1, 0, 9, 5, 1, None, ctypes.byref(found)) == -4
    assert lib.p1hip_scan_below(b"x", 1, 0, 9, 5, 1, (p1_amd._lib.Result * 1)(), None) == -4
    assert found.value == 77  # written only on success
    assert lib.p1hip_get_below_stats(None) == -4
