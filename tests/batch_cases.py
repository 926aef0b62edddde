"""Request lists shared by the batch tests (tests/test_batch_host.py replays
them on the host through tools/batch_emu, tests/test_gpu_batch.py runs them
on the GPU through p1_amd.scan_batch)."""
import random

U64_MAX = (1 << 64) - 1


def random_requests(n, seed, max_nonces=2000):
    """n requests (msg bytes, lower, upper) for one batch: message lengths
    0..129 (each once when n >= 130, arbitrary bytes), digit counts 1..20 with
    most ranges straddling a decade, 1 to max_nonces nonces each, one-tile
    requests next to multi-tile ones, plus the fixed edge cases: the top of
    the u64 range, [0, 0] of the empty message, an empty range and a single
    nonce at U64_MAX."""
    rnd = random.Random(seed)
    reqs = []
    for i in range(n):
        L = i % 130 if i < 130 else rnd.randrange(130)
        if i % 2:
            m = bytes(rnd.randrange(256) for _ in range(L))
        else:
            m = bytes(rnd.randrange(32, 127) for _ in range(L))
        d = 1 + i % 20
        lo = max(0, 10 ** (d - 1) - rnd.randrange(0, 300))
        if i % 3 == 0:
            size = rnd.randrange(1, min(256, max_nonces) + 1)   # one tile (two across a decade)
        else:
            size = rnd.randrange(min(257, max_nonces), max_nonces + 1)
        reqs.append((m, lo, min(lo + size - 1, U64_MAX)))
    fixed = [(b"top of range", U64_MAX - 500, U64_MAX), (b"", 0, 0), (b"msg", 5, 4), (b"last", U64_MAX, U64_MAX)]
    for j, f in enumerate(fixed[:n]):
        reqs[(j * 37 + 11) % n] = f
    return reqs
