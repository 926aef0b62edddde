"""Case lists and the oracle side of the p1hip_scan_below tests, shared by the
CPU replay (tests/test_below_host.py, through `p1emu ... below=`) and the GPU
tests (tests/test_gpu_below.py, through p1_amd.scan_below), the way
tile_cases.py is shared.

The expected answer is the reference loop itself, brute force over the range:
    for i := lower; i <= upper; i++ { if bitcoin.Hash(data, i) <= target { hits = append(hits, i) } }
Targets are chosen from the data: sorted(hashes)[7] gives exactly the hits at
or below it."""
import tile_cases

U64_MAX = (1 << 64) - 1
FLOOR = tile_cases.FLOOR

# tile_cases.k3_cells() is one cell per q = tail byte of the last digit:
# one tail block (q <= 54), TRAIL (55..63), MODE 7 (64), MODE 5 at k = 2 and
# k = 3 (65, 66), and a PRE cell (q >= 71)
K3_QS = (20, 58, 64, 65, 66, 75)


def k3_selection():
    qs = list(range(5, 67)) + list(range(71, 83))
    cells = dict(zip(qs, tile_cases.k3_cells()))
    return [cells[q] for q in K3_QS]


def mode5_k45():
    """MODE 5 with k = 4 and 5 digits in tail block 1, the 120-byte message
    (a midstate block): tiles of several strided runs.  Floor 1."""
    return [case for k, case in tile_cases.mode5_blocks() if k in (4, 5) and len(case[0]) == 120]


def mode5_k45_all():
    return [case for k, case in tile_cases.mode5_blocks() if k in (4, 5)]


class Expect:
    """The oracle's hashes of one range, once, and the lists derived from them."""

    def __init__(self, oracle, msg, lo, hi):
        import numpy as np

        self.msg, self.lo, self.hi = msg, lo, hi
        self.hs = oracle.hashes(msg, lo, hi - lo + 1, threads=8)
        self.sorted = np.sort(self.hs)

    def _pairs(self, idx):
        return [(int(self.hs[i]), self.lo + int(i)) for i in idx]

    @property
    def minimum(self):
        """What the min scan returns: the lowest hash, at its lowest nonce."""
        return self._pairs([int(self.hs.argmin())])[0]

    def first(self, n):
        return self._pairs(range(min(n, len(self.hs))))

    def last(self, n):
        return self._pairs(range(max(len(self.hs) - n, 0), len(self.hs)))

    def nth(self, n):
        """The (n + 1)-th smallest hash of the range (the last if it has fewer)."""
        return int(self.sorted[min(n, len(self.sorted) - 1)])

    def below(self, target, cap=None, lower=None):
        import numpy as np

        idx = np.nonzero(self.hs <= np.uint64(target))[0] if target >= 0 else []
        out = [p for p in self._pairs(idx) if lower is None or p[1] >= lower]
        return out if cap is None else out[:cap]


def increasing(hits):
    return all(a[1] < b[1] for a, b in zip(hits, hits[1:]))


def resume_chain(scan_one, lo, hi):
    """The cap = 1 resume chain: scan_one(lower) -> [] or [(hash, nonce)]."""
    out = []
    while lo <= hi:
        got = scan_one(lo)
        assert len(got) <= 1
        if not got:
            break
        out += got
        if got[0][1] == U64_MAX:
            break
        lo = got[0][1] + 1
    return out
