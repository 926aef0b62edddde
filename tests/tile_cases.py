"""Case lists of the per-tile witness, shared by the CPU replay tests
(tests/test_tiles.py, through `p1emu ... packed=0 tiles`) and the GPU tests
(tests/test_gpu_tiles.py, through p1_amd.scan_tiles), the way batch_cases.py
and wide_cases.py are shared.

A case is (msg, lo, hi).  A group is a list of cases that run under one
planner setting: `floor` (the occupancy floor: P1HIP_MIN_FAST_THREADS on the
device, minthreads= in p1emu), `notable` (P1HIP_NO_TABLE / notable) and
`nosplit` (P1HIP_NO_SPLIT / nosplit).

Shapes: a span of about 2.2 x 256 x 10^k nonces under a floor of 200 makes the
planner settle on k lo digits per thread (it lowers k while the decade has
fewer than 200 threads: 56 at k + 1, 563 at k), which is 563 threads: two
full tiles and a ragged one per fast segment, so all four waves, all 64
lanes, the second tile's block0 arithmetic and the last tile's nthreads edge
are witnessed; the ragged ends of the range add generic tiles."""
import random

U64_MAX = (1 << 64) - 1
FLOOR = 200


def span_for(k):
    return 564 * 10 ** k  # 2.2 x 256 x 10^k, rounded up to a whole number of threads


def _msg(rnd, r, mid):
    """A message with (L + 1) % 64 == r, with (`mid`) or without a midstate block."""
    return bytes(rnd.randrange(32, 127) for _ in range((r - 1) % 64 + (64 if mid else 0)))


def _cell(rnd, r, d, span, mid):
    dlo, dhi = 10 ** (d - 1), min(10 ** d - 1, U64_MAX)
    room = dhi - dlo + 1 - span  # stay inside the decade where it is large enough
    lo = dlo + (rnd.randrange(0, min(room, 10 ** 5)) if room > 0 else 0)
    lo = lo // 10 * 10 + 7  # off every 10^k boundary: ragged (generic) tiles at both ends
    return _msg(rnd, r, mid), lo, min(lo + span - 1, U64_MAX)


def grid(k, both_midstates):
    """Every tail layout: (L + 1) % 64 = r in 0..63 x digit count d in 4..20,
    with and without a midstate block (`both_midstates`) or alternating."""
    rnd = random.Random(50 + k)
    out = []
    for r in range(64):
        for d in range(4, 21):
            for mid in ((False, True) if both_midstates else ((r + d) % 2 == 1,)):
                out.append(_cell(rnd, r, d, span_for(k), mid))
    return out


def k3_cells():
    """At k = 3 the variant depends on q = r + d - 1 alone (the tail byte of
    the last digit): one cell per q in 5..66 reaches every (FV, MODE, TRAIL)
    the default planner selects at k = 3 (q <= 54 one tail block, 55..63
    TRAIL, 64 MODE 7, 65 / 66 MODE 5 at k = 2 / 3), and q in 71..82 runs the
    digit variants again behind a per-thread PRE block.  The digit count
    varies from cell to cell."""
    rnd = random.Random(53)
    out = []
    for q in list(range(5, 67)) + list(range(71, 83)):
        d = 6 + (q * 7) % 15
        if not 0 <= q - d + 1 <= 63:
            d = min(q + 1, 20)
        out.append(_cell(rnd, q - d + 1, d, span_for(3), q % 2 == 1))
    return out


def mode5_blocks():
    """MODE 5 with k = 1..7 digits in tail block 1 (the (k, r) list of
    test_gpu_paths.py test_mode5_whole_blocks_vs_oracle), floor 1 so that k is
    never lowered: whole 10^k blocks plus ragged edges.  70 blocks up to
    k = 5 (with k = 4, 5: one full wave group of 64 hi values and a padded
    one of 6, so full tiles and padded waves both appear), 3 and 2 blocks at
    k = 6, 7 (every wave padded).  -> [(k, case)]"""
    rnd = random.Random(55)
    out = []
    for k in (1, 2, 3, 4, 5, 6, 7):
        for r in (57, 50):
            d = k + 64 - r
            if d > 20:
                continue
            L = r - 1 + (64 if r == 57 else 0)
            m = b"cmu440-p1-" * 12 if L == 120 else bytes(rnd.randrange(32, 127) for _ in range(L))
            blk = 10 ** k
            nblk = {6: 3, 7: 2}.get(k, 70)
            base = 10 ** (d - 1) + rnd.randrange(1, 50) * blk
            out.append((k, (m, base - 777, base + nblk * blk + 555)))
    return out


# Work queue: ranges whose tile counts differ by about 10x and whose messages
# differ, alternated on one stream (default floor: k = 1, 10 nonces per
# thread, 2560 per tile): 30 tiles, then 300.
QUEUE_RANGES = [(b"bradfitz", 10 ** 9 + 12345, 10 ** 9 + 12345 + 76_000),
                (b"cmu440-p1-" * 12, 10 ** 10 + 777, 10 ** 10 + 777 + 760_000)]

# Small route (k_scan_small, P1HIP_SMALL_MAX_NONCES=65536): 1, 256, 257 and
# 2^16 nonces, and a range that straddles a decade.
SMALL_RANGES = [(b"bradfitz", 1000, 1000), (b"bradfitz", 1000, 1255), (b"bradfitz", 1000, 1256),
                (b"bradfitz", 0, 65535), (b"x" * 70, 10 ** 9 - 3000, 10 ** 9 + 3000)]

# Forced re-plan (P1HIP_KWTAB_MAX_BYTES=1000): layouts that plan MODE 7 (q =
# 64) and MODE 5 (q = 65) by default, at spans that keep them so under the floor
def _replan_cases():
    rnd = random.Random(57)
    return [_cell(rnd, 64 - d + 1, d, span_for(3), False) for d in (9, 12)] + \
           [_cell(rnd, 65 - d + 1, d, span_for(3), True) for d in (10, 20)]


REPLAN_CASES = _replan_cases()
