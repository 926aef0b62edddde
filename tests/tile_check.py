"""The per-tile witness: every workgroup partial of one scan against the
oracle's minimum over exactly the nonces that tile covers.

A scan's correctness tests elsewhere compare one (hash, nonce) per scan; a
fault that touches one tile in n shows there with probability ~2/n.  Here a
scan of [lo, hi] comes with its raw partial array and its tile map -- from the
device (p1_amd.scan_tiles, partials poisoned first) or from the CPU replay
(`p1emu ... tiles`), both listing p1_amd/csrc/tile_map.hpp's map of the plan
they ran -- and check_tiles() proves

  (a) the map is a partition: every nonce of [lo, hi] lies in exactly one
      tile, and no tile reaches outside the range;
  (b) every tile's partial is the oracle's (min hash, lowest nonce) over the
      tile's own nonce set; a tile without a valid thread holds
      (2^64-1, 2^64-1);
  (c) the finished result is the lexicographic minimum of the partials and
      equals oracle.scan;

and on failure names the launch, tile, kind and k, and says whether the
partial is still the poison pattern (the tile never ran).

Plain Python and numpy; tests/test_tiles.py holds its self-test."""
import os
import re

import numpy as np

from conftest import ROOT

U64_MAX = (1 << 64) - 1
POISON = int.from_bytes(b"\xa5" * 8, "little")  # include/p1hip.h P1HIP_TILE_POISON, 8 bytes of it
GENERIC_KIND = 255                                # scan_abi.hpp kGenericKind
TILE_THREADS = 256                                # scan_core.hpp kBlock


class TileError(AssertionError):
    pass


def variant_id(fv, mode, trail):
    """scan_abi.hpp variant_id."""
    if mode == 5:
        return 128 + fv
    if mode == 7:
        return 192 + fv
    if mode == 6:
        return 160 + (16 if trail else 0) + fv
    return (64 if trail else 0) + fv * 4 + (mode - 1)


def shipped_variants(plain_mode2=False):
    """{kind: (FV, MODE, TRAIL)} of every P1_CASE of fast_variants.inc; the
    mode-2 block only with `plain_mode2` (p1emu is built with it, the library
    is not)."""
    with open(os.path.join(ROOT, "p1_amd", "csrc", "fast_variants.inc")) as f:
        text = f.read()
    if not plain_mode2:
        text = text.split("#ifdef P1_NV2_PLAIN")[0]
    out = {}
    for a, b, c in re.findall(r"P1_CASE\((\d+), (\d+), (true|false)\)", text):
        v = (int(a), int(b), c == "true")
        out[variant_id(*v)] = v
    return out


def parse_emu_tiles(stdout):
    """The `tile ...` lines of `p1emu ... tiles` -> the tuples scan_tiles gives:
    (launch, tile, kind, k, (hash, nonce), [(first, run_len, stride, count)])."""
    tiles = []
    for ln in stdout.splitlines():
        if not ln.startswith("tile "):
            continue
        f = [int(x) for x in ln.split()[1:]]
        runs = [tuple(f[7 + 4 * i: 11 + 4 * i]) for i in range(f[6])]
        assert len(f) == 7 + 4 * f[6], ln
        tiles.append((f[0], f[1], f[2], f[3], (f[4], f[5]), runs))
    return tiles


def valid_threads(tile):
    """Threads of the tile that hold a nonce (256: a full tile)."""
    _, _, kind, k, _, runs = tile
    if kind == GENERIC_KIND:
        return sum(rl * c for _, rl, _, c in runs)
    if all(c == 1 for _, _, _, c in runs):  # one thread per hi value, 10^k nonces each
        return sum(rl for _, rl, _, _ in runs) // 10 ** k
    return sum(c for _, _, _, c in runs)    # MODE 5, k > 3: one lane per hi value and run


def _name(tile):
    launch, t, kind, k, _, _ = tile
    return f"launch {launch} tile {t} kind {kind} k {k}"


def check_tiles(oracle, msg, lo, hi, tiles, result, threads=16, max_report=5):
    """Raise TileError unless (a), (b) and (c) of the module docstring hold.
    `tiles` in partial-array order, `result` the finished (hash, nonce).
    Returns the set of kinds seen in tiles with 256 valid threads."""
    n = hi - lo + 1
    H = oracle.hashes(msg, lo, n, threads)
    cover = np.zeros(n, dtype=np.uint8)
    bad = []
    full_kinds = set()
    best = (U64_MAX, U64_MAX)
    for tile in tiles:
        key, runs = tile[4], tile[5]
        want = (U64_MAX, U64_MAX)  # no valid thread
        inside = True
        for first, run_len, stride, count in runs:
            last = first + (count - 1) * stride + run_len - 1
            if count < 1 or run_len < 1 or first < lo or last > hi or (count > 1 and stride < run_len):
                bad.append(f"{_name(tile)}: run ({first}, {run_len}, {stride}, {count}) reaches outside "
                           f"[{lo}, {hi}] or overlaps itself")
                inside = False
                continue
            off = first - lo
            if count == 1:
                seg = H[off:off + run_len]
                cover[off:off + run_len] += 1
                j = int(seg.argmin())  # first occurrence: the lowest nonce of the minimum
                cand = (int(seg[j]), first + j)
            else:
                view = np.lib.stride_tricks.as_strided(H[off:], shape=(count, run_len), strides=(8 * stride, 8),
                                                       writeable=False)
                cv = np.lib.stride_tricks.as_strided(cover[off:], shape=(count, run_len), strides=(stride, 1))
                cv += 1
                j = int(view.argmin())  # row-major = ascending nonce
                row, col = divmod(j, run_len)
                cand = (int(view[row, col]), first + row * stride + col)
            want = min(want, cand)
        if inside and key != want:
            why = " (still the poison pattern: this tile was never written)" if key == (POISON, POISON) else ""
            bad.append(f"{_name(tile)}: partial {key}, the oracle's minimum over its nonces is {want}{why}")
        best = min(best, key)
        if valid_threads(tile) == TILE_THREADS:
            full_kinds.add(tile[2])
    if not (cover == 1).all():
        miss = np.flatnonzero(cover == 0)
        twice = np.flatnonzero(cover > 1)
        if len(miss):
            bad.append(f"the map is no partition: {len(miss)} nonces in no tile, first {lo + int(miss[0])}")
        if len(twice):
            bad.append(f"the map is no partition: {len(twice)} nonces in more than one tile, first "
                       f"{lo + int(twice[0])}")
    fin = (best[0], 0 if best[0] == U64_MAX else best[1])  # identity (MaxUint64, 0) of miner.go:56
    want_res = oracle.scan(msg, lo, hi, threads=threads)
    if tuple(result) != fin:
        bad.append(f"result {tuple(result)} is not the minimum of the partials {fin}")
    if tuple(result) != want_res:
        bad.append(f"result {tuple(result)}, oracle.scan gives {want_res}")
    if bad:
        more = f" (+{len(bad) - max_report} more)" if len(bad) > max_report else ""
        raise TileError(f"{len(msg)}-byte message, [{lo}, {hi}], {len(tiles)} tiles: " + "; ".join(bad[:max_report]) + more)
    return full_kinds
