"""CPU tests of the per-tile witness (tests/tile_check.py): the checker's own
self-test on synthetic data, and the case lists of tests/tile_cases.py
replayed by `p1emu ... packed=... tiles` -- the library's plan, packing,
segment tables and tile map (p1_amd/csrc/tile_map.hpp), the kernels'
per-thread code, one partial per tile from a poisoned vector -- with every
partial checked against the oracle.  tests/test_gpu_tiles.py runs the same
lists on the device; here the tile map and the checker are validated without
one."""
import concurrent.futures as cf
import os
import subprocess

import numpy as np
import pytest

import tile_cases
from conftest import ROOT, host_bin
from tile_check import (GENERIC_KIND, POISON, U64_MAX, TileError, check_tiles, parse_emu_tiles, shipped_variants,
                        valid_threads)

EMU = host_bin(os.path.join(ROOT, "tools", "p1emu"))


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(EMU):
        subprocess.run(["make", "-s", "-C", ROOT, "tools/p1emu"], check=True)


# ----------------------------------------------------------------------------
# the checker on synthetic data
# ----------------------------------------------------------------------------
class FakeOracle:
    """hashes()/scan() over a made-up hash array for nonces lo .. lo + n - 1."""

    def __init__(self, lo, H):
        self.lo, self.H = lo, np.asarray(H, dtype=np.uint64)

    def hashes(self, msg, first, count, threads=1):
        return self.H[first - self.lo: first - self.lo + count].copy()

    def scan(self, msg, lower, upper, threads=1):
        seg = self.H[lower - self.lo: upper - self.lo + 1]
        j = int(seg.argmin())
        return int(seg[j]), lower + j


def _synthetic():
    """[1000, 1000 + 2999]: a generic tile of 256 + one of 44 (300 nonces), a
    fast k = 1 segment of 260 hi values (one full tile, one of 4 threads), a
    strided tile (2 interleaved runs, each 25 of every 50 nonces, twice) and
    an empty one.  Hashes are distinct except for the planted tie."""
    lo, hi = 1000, 3999
    rng = np.random.default_rng(5)
    H = rng.permutation(np.arange(10_000, 13_000, dtype=np.uint64))
    H[10] = H[200] = 7          # generic tile 0: the minimum twice, nonces 1010 and 1200
    tiles_runs = [(0, 0, GENERIC_KIND, 0, [(1000, 256, 0, 1)]),
                  (0, 1, GENERIC_KIND, 0, [(1256, 44, 0, 1)]),
                  (0, 2, 4, 1, [(1300, 2560, 0, 1)]),
                  (0, 3, 4, 1, [(3860, 40, 0, 1)]),
                  (1, 0, 128, 5, [(3900, 25, 50, 2), (3925, 25, 50, 2)]),
                  (1, 1, 128, 5, [])]
    orc = FakeOracle(lo, H)
    tiles = []
    for launch, t, kind, k, runs in tiles_runs:
        best = (U64_MAX, U64_MAX)
        for first, rl, st, c in runs:
            for j in range(c):
                a = first + j * st
                best = min(best, min((int(orc.H[n - lo]), n) for n in range(a, a + rl)))
        tiles.append((launch, t, kind, k, best, runs))
    return orc, lo, hi, tiles


def test_checker_accepts_the_exact_witness_and_rejects_each_fault():
    orc, lo, hi, tiles = _synthetic()
    result = orc.scan(b"m", lo, hi)
    assert result == (7, 1010)
    assert check_tiles(orc, b"m", lo, hi, tiles, result) == {GENERIC_KIND, 4}

    def broken(i, **kw):
        t = list(tiles[i])
        for name, v in kw.items():
            t[{"key": 4, "runs": 5}[name]] = v
        return tiles[:i] + [tuple(t)] + tiles[i + 1:]

    # one key left at poison: named, and said to be poison
    with pytest.raises(TileError, match=r"launch 0 tile 3 kind 4 k 1.*poison"):
        check_tiles(orc, b"m", lo, hi, broken(3, key=(POISON, POISON)), result)
    # the tile's second-smallest hash
    second = sorted((int(orc.H[n - lo]), n) for n in range(1300, 3860))[1]
    with pytest.raises(TileError, match=r"launch 0 tile 2 kind 4 k 1: partial"):
        check_tiles(orc, b"m", lo, hi, broken(2, key=second), result)
    # the right hash with the higher tied nonce
    with pytest.raises(TileError, match=r"launch 0 tile 0 kind 255 k 0: partial \(7, 1200\)"):
        check_tiles(orc, b"m", lo, hi, broken(0, key=(7, 1200)), result)
    # an empty tile must hold the identity, not poison and not a hash
    with pytest.raises(TileError, match=r"launch 1 tile 1 kind 128 k 5"):
        check_tiles(orc, b"m", lo, hi, broken(5, key=(POISON, POISON)), result)
    # a map that omits one nonce (the tile's key recomputed for the shorter set, so only the map is wrong)
    short = [(1256, 43, 0, 1)]
    key = min((int(orc.H[n - lo]), n) for n in range(1256, 1299))
    with pytest.raises(TileError, match=r"no partition: 1 nonces in no tile, first 1299"):
        check_tiles(orc, b"m", lo, hi, broken(1, runs=short, key=key), result)
    # a map that repeats one nonce
    longer = [(1256, 45, 0, 1)]
    key = min((int(orc.H[n - lo]), n) for n in range(1256, 1301))
    with pytest.raises(TileError, match=r"no partition: 1 nonces in more than one tile, first 1300"):
        check_tiles(orc, b"m", lo, hi, broken(1, runs=longer, key=key), result)
    # a tile that reaches outside the range
    with pytest.raises(TileError, match=r"launch 0 tile 0 .* reaches outside"):
        check_tiles(orc, b"m", lo, hi, broken(0, runs=[(999, 257, 0, 1)]), result)
    # a finished result that is not the minimum of the partials / not oracle.scan
    with pytest.raises(TileError, match=r"result \(7, 1200\)"):
        check_tiles(orc, b"m", lo, hi, tiles, (7, 1200))
    assert [valid_threads(t) for t in tiles] == [256, 44, 256, 4, 4, 0]


# ----------------------------------------------------------------------------
# the case lists through the CPU replay
# ----------------------------------------------------------------------------
def emu_tiles(case, mode="packed=0", floor=None, notable=False, nosplit=False):
    """-> (tiles, finished result, launches) of one `p1emu ... tiles` run."""
    msg, lo, hi = case
    args = [EMU, msg.hex() if msg else "-", str(lo), str(hi)]
    if floor is not None:
        args.append(f"minthreads={floor}")
    args += (["notable"] if notable else []) + (["nosplit"] if nosplit else []) + [mode, "tiles"]
    r = subprocess.run(args, capture_output=True, text=True, check=True)
    head = r.stdout.split("\n", 1)[0].split()
    tiles = parse_emu_tiles(r.stdout)
    return tiles, (int(head[0]), int(head[1])), len({t[0] for t in tiles})


_GROUPS = {}


def run_group(oracle, name, cases, **flags):
    """Replay and check every case of a group (once per session); -> per case
    the kinds seen in full tiles and the kinds seen at all."""
    if name not in _GROUPS:
        def one(case):
            tiles, result, _ = emu_tiles(case, **flags)
            full = check_tiles(oracle, case[0], case[1], case[2], tiles, result, threads=2)
            return full, {t[2] for t in tiles}

        with cf.ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:
            _GROUPS[name] = list(ex.map(one, cases))
    return _GROUPS[name]


def _k3(oracle):
    return run_group(oracle, "k3", tile_cases.k3_cells(), floor=tile_cases.FLOOR)


def _modes(kinds, variants):
    return {variants[k][1] for k in kinds if k in variants}


@pytest.mark.parametrize("k", [1, 2])
def test_emu_tiles_every_tail_layout_small_k(oracle_mod, k):
    """The whole (r, d) grid at k = 1 (with and without a midstate block) and
    k = 2 (alternating): every tile of every cell exact."""
    res = run_group(oracle_mod, f"k{k}", tile_cases.grid(k, both_midstates=k == 1), floor=tile_cases.FLOOR)
    assert all(GENERIC_KIND in seen for _, seen in res)  # ragged edges everywhere
    assert sum(1 for full, _ in res if full - {GENERIC_KIND}) > 0.9 * len(res)  # full fast tiles nearly everywhere


def test_emu_tiles_k3_cells(oracle_mod):
    res = _k3(oracle_mod)
    assert all(full - {GENERIC_KIND} for full, _ in res)  # every cell has a full fast tile


def test_emu_tiles_k3_cells_without_table_and_split(oracle_mod):
    """The k = 3 cells whose variant P1HIP_NO_TABLE (MODE 5 / 7 cells) or
    P1HIP_NO_SPLIT (mode 3 / 4 cells: mode 2, which only p1emu is built with)
    changes, under that setting."""
    variants = shipped_variants(True)
    cells = tile_cases.k3_cells()
    base = _k3(oracle_mod)
    tabled = [c for c, (_, seen) in zip(cells, base) if _modes(seen, variants) & {5, 7}]
    splits = [c for c, (_, seen) in zip(cells, base) if _modes(seen, variants) & {3, 4}]
    assert len(tabled) == 3 and len(splits) >= 28
    res = run_group(oracle_mod, "k3_notable", tabled, floor=tile_cases.FLOOR, notable=True)
    assert all(not _modes(seen, variants) & {5, 7} for _, seen in res)
    res = run_group(oracle_mod, "k3_nosplit", splits, floor=tile_cases.FLOOR, nosplit=True)
    assert all(_modes(full, variants) == {2} for full, _ in res)


def test_emu_tiles_mode5_blocks(oracle_mod):
    """MODE 5 with 1..6 digits in tail block 1 (k = 7 is left to the GPU test:
    its table is 2.56 GB of host memory and its two blocks 2 x 10^7 nonces of
    one host thread).  With k >= 4 the wave-to-run mapping and its padded
    waves are witnessed: strided runs, some with fewer than 64 hi values."""
    cases = [(k, c) for k, c in tile_cases.mode5_blocks() if k <= 6]
    res = run_group(oracle_mod, "mode5", [c for _, c in cases], floor=1)
    for (k, case), (_, seen) in zip(cases, res):
        # MODE 5 ran (one digit in block 1 at 1000 nonces per thread is MODE 7, the two-level MODE 5)
        assert (207 if k == 1 else 128) in seen, (k, case[1])
    tiles, _, _ = emu_tiles(cases[-1][1], floor=1)
    strided = [r for t in tiles if t[2] == 128 for r in t[5]]
    assert strided and all(st == 10 ** 6 and rl == 1000 and c == 3 for _, rl, st, c in strided)


def test_emu_tiles_variant_coverage(oracle_mod):
    """Full tiles (256 valid threads) of the k = 1, 2 grids, the k = 3 cells
    (with and without the table) and the MODE 5 blocks together reach every
    variant the library ships.  <0,6> runs only without the table: its layout
    (lo digits from byte 0 of tail block 1) is MODE 5's otherwise."""
    variants = shipped_variants(False)
    cells = tile_cases.k3_cells()
    base = _k3(oracle_mod)
    tabled = [c for c, (_, seen) in zip(cells, base) if _modes(seen, variants) & {5, 7}]
    full = set()
    for name, cases, flags in [("k1", tile_cases.grid(1, True), {}), ("k2", tile_cases.grid(2, False), {}),
                               ("k3", cells, {}), ("k3_notable", tabled, {"notable": True})]:
        for f, _ in run_group(oracle_mod, name, cases, floor=tile_cases.FLOOR, **flags):
            full |= f
    assert full - {GENERIC_KIND} == set(variants), sorted(variants[k] for k in set(variants) ^ (full - {GENERIC_KIND}))
    assert GENERIC_KIND in full


@pytest.mark.parametrize("mode,launches", [("packed=0", 1), ("packed=1", 3), ("packed=5", 2), ("packed=1500", 1)])
def test_emu_tiles_queue_ranges_across_launches(oracle_mod, mode, launches):
    """The work-queue ranges of the GPU test cut into launches: each launch
    writes its own slice of the partial vector (part_off).  A range is a fast
    piece between two one-tile generic edges: a launch each at 1 workgroup per
    launch, the edges together at 5."""
    for case, ntiles in zip(tile_cases.QUEUE_RANGES, (30, 300)):
        tiles, result, nl = emu_tiles(case, mode=mode)
        check_tiles(oracle_mod, *case, tiles, result)
        assert nl == launches and abs(len(tiles) - ntiles) <= 3, (len(tiles), nl)


def test_emu_tiles_small_route(oracle_mod):
    for case in tile_cases.SMALL_RANGES:
        tiles, result, nl = emu_tiles(case, mode="small")
        full = check_tiles(oracle_mod, *case, tiles, result)
        assert nl == 1 and {t[2] for t in tiles} == {GENERIC_KIND}
        assert len(tiles) >= (case[2] - case[1]) // 256 + 1 and (full or case[2] - case[1] < 255)


def test_emu_tiles_replan_cases_have_no_table_kind(oracle_mod):
    """The forced re-plan of the GPU test plans without MODE 5 / 7 (p1emu:
    notable); by default the same cases do run them."""
    variants = shipped_variants(True)
    default = [emu_tiles(c, floor=tile_cases.FLOOR)[0] for c in tile_cases.REPLAN_CASES]
    assert all(_modes({t[2] for t in tiles}, variants) & {5, 7} for tiles in default)
    for case in tile_cases.REPLAN_CASES:
        tiles, result, _ = emu_tiles(case, floor=tile_cases.FLOOR, notable=True)
        check_tiles(oracle_mod, *case, tiles, result)
        assert not _modes({t[2] for t in tiles}, variants) & {5, 7}
