"""Request lists shared by the wide-batch tests (tests/test_wide_host.py
replays them on the host through `tools/batch_emu wide`,
tests/test_gpu_wide.py runs them on the GPU through p1_amd.scan_batch_wide)."""
import random

U64_MAX = (1 << 64) - 1
SMALL = 1 << 16
WIDE_MAX = 1 << 24


def mid_requests(n, seed, max_nonces=200_000):
    """n wide requests (msg bytes, lower, upper): message lengths 0..129
    (arbitrary bytes and printable alternate), 65,537 to max_nonces nonces,
    starts 10^(d-1) - r for d = 1..20 so that most ranges straddle a decade,
    plus the fixed edges: the top of the u64 range, a request of exactly
    2^16 + 1 nonces, and that same request a second time."""
    rnd = random.Random(seed)
    reqs = []
    for i in range(n):
        L = (i * 7) % 130
        if i % 2:
            m = bytes(rnd.randrange(256) for _ in range(L))
        else:
            m = bytes(rnd.randrange(32, 127) for _ in range(L))
        d = 1 + i % 20
        size = rnd.randrange(SMALL + 1, max_nonces + 1)
        lo = max(0, 10 ** (d - 1) - rnd.randrange(0, size))
        reqs.append((m, lo, min(lo + size - 1, U64_MAX)))
    edge = (b"exactly one past the small limit", 10 ** 7 - 1234, 10 ** 7 - 1234 + SMALL)
    fixed = [(b"top of range", U64_MAX - 100000, U64_MAX), edge, edge]
    for j, f in enumerate(fixed[:n]):
        reqs[(j * 13 + 5) % n] = f
    return reqs
