"""GPU tests of the per-tile witness: the shipped k_scan / k_scan_small run
unchanged, and every workgroup partial they write is compared with the
oracle's minimum over exactly that tile's nonces.

The other GPU modules compare one (hash, nonce) per scan, which sees a fault
in one tile of n with probability about 2/n, and a stale partial from an
earlier identical scan not at all.  Here p1_amd.scan_tiles (p1hip_scan_tiles,
a test hook) poisons the scan's slice of the partial array, runs the scan
through the code p1hip_scan runs, and returns the raw partials with the tile
map of the plan it launched; tests/tile_check.py proves the map a partition of
the range and every partial exact, and names the launch, tile, kind and k of
one that is not (and whether it is still poison: a tile the work queue never
handed out).  The case lists (tests/tile_cases.py) are those the CPU replay
checks in tests/test_tiles.py.

P1HIP_NO_SPLIT cells run on the CPU replay only: they plan mode 2, which the
shipped code object is not built with."""
import concurrent.futures as cf
import time

import pytest

import tile_cases
from tile_check import GENERIC_KIND, check_tiles, shipped_variants

pytestmark = pytest.mark.gpu

INIT_KNOBS = ("P1HIP_MIN_FAST_THREADS", "P1HIP_NO_TABLE")
SCAN_KNOBS = ("P1HIP_SCAN_GRID", "P1HIP_MAX_LAUNCH_BLOCKS", "P1HIP_KWTAB_MAX_BYTES")


@pytest.fixture
def reinit(gpu, monkeypatch):
    """Set env knobs, re-initialise on device 0; restore after."""
    def go(**env):
        for k in INIT_KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, str(v))
        gpu.shutdown()
        gpu.init_devices([0])
        return gpu

    yield go
    for k in INIT_KNOBS + SCAN_KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("P1HIP_SMALL_MAX_NONCES", "0")
    monkeypatch.setenv("P1HIP_TEST_KNOBS", "1")
    gpu.shutdown()
    gpu.init_devices([0])


def check_all(oracle, runs):
    """runs: [(case, route, tiles, result)] -> per run (kinds in full tiles,
    kinds seen); the oracle's hashing spread over the host threads."""
    def one(run):
        (msg, lo, hi), _, tiles, result = run
        threads = 2 if hi - lo < 2_000_000 else 16  # the few long ranges are hashed wide
        return check_tiles(oracle, msg, lo, hi, tiles, result, threads=threads), {t[2] for t in tiles}

    with cf.ThreadPoolExecutor(8) as ex:
        return list(ex.map(one, runs))


_GROUPS = {}


def run_group(reinit, oracle, name, cases, **env):
    """Scan and check every case of a group (once per session)."""
    if name not in _GROUPS:
        g = reinit(**env)
        t0 = time.time()
        runs = [(c,) + g.scan_tiles(*c) for c in cases]
        t1 = time.time()
        assert all(route == "scan" for _, route, _, _ in runs)
        _GROUPS[name] = check_all(oracle, runs)
        print(f"{name}: {len(cases)} scans, {sum(len(r[2]) for r in runs)} tiles, device {t1 - t0:.2f} s, "
              f"checking {time.time() - t1:.2f} s")
    return _GROUPS[name]


def _k3(reinit, oracle):
    return run_group(reinit, oracle, "k3", tile_cases.k3_cells(), P1HIP_MIN_FAST_THREADS=tile_cases.FLOOR)


def _modes(kinds, variants):
    return {variants[k][1] for k in kinds if k in variants}


def _tabled(reinit, oracle, variants):
    cells = tile_cases.k3_cells()
    return [c for c, (_, seen) in zip(cells, _k3(reinit, oracle)) if _modes(seen, variants) & {5, 7}]


def test_tiles_every_tail_layout_k1(reinit, oracle_mod):
    """Every (r, d) cell, with and without a midstate block, at k = 1."""
    res = run_group(reinit, oracle_mod, "k1", tile_cases.grid(1, True), P1HIP_MIN_FAST_THREADS=tile_cases.FLOOR)
    assert all(GENERIC_KIND in seen for _, seen in res)
    assert sum(1 for full, _ in res if full - {GENERIC_KIND}) > 0.9 * len(res)


def test_tiles_every_tail_layout_k2(reinit, oracle_mod):
    """Every (r, d) cell at k = 2, the midstate block alternating."""
    res = run_group(reinit, oracle_mod, "k2", tile_cases.grid(2, False), P1HIP_MIN_FAST_THREADS=tile_cases.FLOOR)
    assert all(GENERIC_KIND in seen for _, seen in res)
    assert sum(1 for full, _ in res if full - {GENERIC_KIND}) > 0.9 * len(res)


def test_tiles_k3_cells(reinit, oracle_mod):
    """One cell per variant the planner selects at k = 3, and the PRE layouts."""
    assert all(full - {GENERIC_KIND} for full, _ in _k3(reinit, oracle_mod))


def test_tiles_k3_cells_without_table(reinit, oracle_mod):
    """The MODE 5 / 7 cells of the k = 3 list under P1HIP_NO_TABLE=1."""
    variants = shipped_variants()
    tabled = _tabled(reinit, oracle_mod, variants)
    assert len(tabled) == 3
    res = run_group(reinit, oracle_mod, "k3_notable", tabled, P1HIP_MIN_FAST_THREADS=tile_cases.FLOOR,
                    P1HIP_NO_TABLE=1)
    assert all(not _modes(seen, variants) & {5, 7} for _, seen in res)


def test_tiles_mode5_blocks(reinit, oracle_mod):
    """MODE 5 with k = 1..7 digits in tail block 1 (k = 1: MODE 7), whole
    blocks plus ragged edges; with k >= 4 the wave-to-run mapping and its
    padded waves."""
    cases = tile_cases.mode5_blocks()
    g = reinit(P1HIP_MIN_FAST_THREADS=1)
    runs = [(c,) + g.scan_tiles(*c) for _, c in cases]
    for (k, case), (_, seen) in zip(cases, check_all(oracle_mod, runs)):
        assert (207 if k == 1 else 128) in seen, (k, case[1])
    strided = [r for t in runs[-1][2] if t[2] == 128 for r in t[5]]
    assert strided and all(st == 10 ** 7 and rl == 1000 and c == 2 for _, rl, st, c in strided)


def test_tiles_variant_coverage(reinit, oracle_mod):
    """Full tiles (256 valid threads) of the k = 1, 2 grids and the k = 3
    cells, with and without the table, reach every variant the library ships
    (<0,6> only without the table: its layout is MODE 5's otherwise)."""
    variants = shipped_variants()
    full = set()
    for name, cases, env in [("k1", tile_cases.grid(1, True), {}), ("k2", tile_cases.grid(2, False), {}),
                             ("k3", tile_cases.k3_cells(), {}),
                             ("k3_notable", _tabled(reinit, oracle_mod, variants), {"P1HIP_NO_TABLE": 1})]:
        for f, _ in run_group(reinit, oracle_mod, name, cases, P1HIP_MIN_FAST_THREADS=tile_cases.FLOOR, **env):
            full |= f
    assert full - {GENERIC_KIND} == set(variants), sorted(variants[k] for k in set(variants) ^ (full - {GENERIC_KIND}))
    assert GENERIC_KIND in full


def _alternate(g, oracle):
    a, b = tile_cases.QUEUE_RANGES
    runs = [(c,) + g.scan_tiles(*c) for c in (a, b, a, b)]
    check_all(oracle, runs)
    return runs


@pytest.mark.parametrize("grid", [1, 3, 7])
def test_tiles_work_queue_small_grids(reinit, oracle_mod, monkeypatch, grid):
    """k_scan on 1, 3 and 7 workgroups: every tile past those comes from the
    ticket.  Ranges of about 30 and 300 tiles and different messages
    alternate on the stream; poison fills the partial array only as far as
    each scan's own tiles, so the longer scan's partials lie behind the
    shorter one's."""
    g = reinit()
    monkeypatch.setenv("P1HIP_SCAN_GRID", str(grid))
    runs = _alternate(g, oracle_mod)
    assert [len({t[0] for t in r[2]}) for r in runs] == [1, 1, 1, 1]
    assert 25 <= len(runs[0][2]) <= 35 and 290 <= len(runs[1][2]) <= 310


@pytest.mark.parametrize("blocks,launches", [(1, 3), (5, 2), (1500, 1)])
def test_tiles_work_queue_across_launches(reinit, oracle_mod, monkeypatch, blocks, launches):
    """The same alternation cut into launches of at most 1, 5 and 1500
    workgroups: part_off across launches, the ticket reset between them."""
    g = reinit()
    monkeypatch.setenv("P1HIP_SCAN_GRID", "3")
    monkeypatch.setenv("P1HIP_MAX_LAUNCH_BLOCKS", str(blocks))
    runs = _alternate(g, oracle_mod)
    assert [len({t[0] for t in r[2]}) for r in runs] == [launches] * 4


def test_tiles_small_route(reinit, oracle_mod, monkeypatch):
    """k_scan_small's partials (P1HIP_SMALL_MAX_NONCES=65536), a queued scan
    in between."""
    g = reinit()
    monkeypatch.setenv("P1HIP_SMALL_MAX_NONCES", "65536")
    runs = []
    for c in tile_cases.SMALL_RANGES:
        runs.append((c,) + g.scan_tiles(*c))
        runs.append((tile_cases.QUEUE_RANGES[0],) + g.scan_tiles(*tile_cases.QUEUE_RANGES[0]))
    check_all(oracle_mod, runs)
    assert [r[1] for r in runs] == ["small", "scan"] * len(tile_cases.SMALL_RANGES)
    for (_, lo, hi), _, tiles, _ in runs[0::2]:
        assert {t[2] for t in tiles} == {GENERIC_KIND} and len(tiles) >= (hi - lo) // 256 + 1


def test_tiles_after_forced_replan(reinit, oracle_mod, monkeypatch):
    """A table that cannot be had (P1HIP_KWTAB_MAX_BYTES=1000) re-plans the
    share: every tile still exact, none of a MODE 5 / 7 kind; without the cap
    the same cases do run them."""
    variants = shipped_variants()
    g = reinit(P1HIP_MIN_FAST_THREADS=tile_cases.FLOOR)  # a fresh device: no cached table
    monkeypatch.setenv("P1HIP_KWTAB_MAX_BYTES", "1000")
    runs = [(c,) + g.scan_tiles(*c) for c in tile_cases.REPLAN_CASES]
    monkeypatch.delenv("P1HIP_KWTAB_MAX_BYTES")
    for _, seen in check_all(oracle_mod, runs):
        assert not _modes(seen, variants) & {5, 7}
    runs = [(c,) + g.scan_tiles(*c) for c in tile_cases.REPLAN_CASES]
    for _, seen in check_all(oracle_mod, runs):
        assert _modes(seen, variants) & {5, 7}


def test_scan_tiles_refuses_empty_and_oversized_ranges(gpu):
    for lo, hi in [(5, 4), (0, 1 << 32), (7, 7 + (1 << 32))]:
        with pytest.raises(gpu.P1HipError) as e:
            gpu.scan_tiles(b"bradfitz", lo, hi)
        assert e.value.rc == -4
