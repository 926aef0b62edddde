"""GPU tests of p1hip_scan_below_batch: many (message, range, target, cap)
searches in one call, each answered exactly as p1hip_scan_below answers it.

Every expected list is the reference loop, brute force by the oracle
(below_cases.Expect), and equality is exact.  The request lists are those of
the CPU replay in tests/test_below_batch_host.py (below_batch_cases.py)."""
import pytest

import below_batch_cases
import tile_cases
from below_cases import U64_MAX, Expect

pytestmark = pytest.mark.gpu

BELOW_CODEOBJ = "3b0943b0c749d0ad2099d6e5114f287dbe3b67f13ae015be6c145e7ba4acbfae"  # profiles/below_bench.json
UNWRITTEN = (1 << 32) - 1


@pytest.fixture
def dev(gpu, monkeypatch):
    """Device 0 alone, the per-call knobs of p1hip_scan_below cleared, fresh statistics."""
    for k in ("P1HIP_BELOW_PATH", "P1HIP_BELOW_MAX_SLICE"):
        monkeypatch.delenv(k, raising=False)
    if gpu.device_count() != 1:
        gpu.shutdown()
        gpu.init_devices([0])
    gpu.reset_stats()
    return gpu


# ---------------------------------------------------------------------------
# (a), (b): the matrix, in one round and in several
# ---------------------------------------------------------------------------
def test_below_batch_matrix(dev, oracle_mod):
    reqs, want = below_batch_cases.matrix(oracle_mod)
    assert dev.scan_below_batch(reqs) == want
    s = dev.get_below_batch_stats()
    print(s)
    empty = sum(lo > hi or cap == 0 for _, lo, hi, _, cap in reqs)
    assert s["calls"] == 1 and s["requests"] == 150 and s["empty"] == empty and s["coalesced"] == 150 - empty
    assert s["individual"] == 0 and s["rounds"] == 1 and s["launches"] == 1
    assert s["mark_nonces"] == sum(hi - lo + 1 for _, lo, hi, _, cap in reqs if lo <= hi and cap)
    assert s["hits"] == sum(len(w) for w in want)
    # the one copy back: a count per request and 4 bytes per hit slot
    slots = sum(min(cap, hi - lo + 1) for _, lo, hi, _, cap in reqs if lo <= hi)
    assert s["bytes_back"] == 4 * (150 - empty + slots)


def test_below_batch_rounds(dev, oracle_mod, monkeypatch):
    """P1HIP_BELOW_MAX_SLICE=1000: five rounds on the 5000-nonce list, and more on the matrix."""
    monkeypatch.setenv("P1HIP_BELOW_MAX_SLICE", "1000")
    reqs, want = below_batch_cases.rounds(oracle_mod)
    assert dev.scan_below_batch(reqs) == want
    s = dev.get_below_batch_stats()
    print(s)
    assert s["rounds"] == 5 and s["launches"] == 5 and s["individual"] == 0
    reqs, want = below_batch_cases.matrix(oracle_mod)
    assert dev.scan_below_batch(reqs) == want
    assert dev.get_below_batch_stats()["rounds"] == 5 + 2


# ---------------------------------------------------------------------------
# (c): a full-size request next to one-tile requests
# ---------------------------------------------------------------------------
def test_below_batch_every_nonce_and_none(dev, oracle_mod):
    lo, hi = 99990, 99990 + 65535  # 257 tiles: ten nonces before the decade boundary
    E = Expect(oracle_mod, b"full size", lo, hi)
    small = Expect(oracle_mod, b"one tile", 77, 200)
    t = small.nth(3)
    got = dev.scan_below_batch([
        (b"one tile", 77, 200, t, 10), (b"full size", lo, hi, U64_MAX, 65536), (b"one tile", 77, 200, U64_MAX, 200),
        (b"full size", lo, hi, 0, 65536), (b"one tile", 77, 200, t, 2),
    ])
    assert len(got[1]) == 65536 and got[1] == E.first(65536)
    assert got[3] == E.below(0) == []
    assert got[0] == small.below(t) and len(got[0]) == 4 and got[2] == small.first(124) and got[4] == small.below(t, cap=2)
    s = dev.get_below_batch_stats()
    assert s["rounds"] == 1 and s["tiles"] == 2 * 257 + 3 * 2 and s["coalesced"] == 5


# ---------------------------------------------------------------------------
# (d), (e): the pool's question at library defaults; the 2^20 class over two rounds
# ---------------------------------------------------------------------------
def test_below_batch_pool_workers(dev, oracle_mod):
    assert dev.test_knobs().get("P1HIP_BELOW_MAX_SLICE") is None and dev.test_knobs().get("P1HIP_BELOW_PATH") is None
    reqs = [(b"worker %d" % i, 0, 2 ** 32 - 1, 1 << 56, 1) for i in range(64)]
    want = [Expect(oracle_mod, m, 0, 65535).below(1 << 56, cap=1) for m, *_ in reqs]
    assert all(len(w) == 1 for w in want)
    assert dev.scan_below_batch(reqs) == want
    s = dev.get_below_batch_stats()
    print(s)
    assert s["rounds"] == 1 and s["launches"] == 1 and s["coalesced"] == 64 and s["mark_nonces"] == 64 << 16
    assert s["bytes_back"] == 64 * 8


def test_below_batch_two_rounds_of_2_20(dev, oracle_mod):
    lo, hi = 10 ** 9 + 400000, 10 ** 9 + 2 ** 21 - 1
    E = Expect(oracle_mod, b"bradfitz", lo, hi)
    want = E.below(1 << 46, cap=2)
    assert [n for _, n in want] == [10 ** 9 + 1927140]  # in the second slice of 2^20
    assert dev.below_batch_layout([(b"bradfitz", lo, hi, 1 << 46, 2)], 1) == [{"route": "coalesced", "device": 0, "tiles": 4096}]
    assert dev.scan_below_batch([(b"bradfitz", lo, hi, 1 << 46, 2)]) == [want]
    s = dev.get_below_batch_stats()
    assert s["rounds"] == 2 and s["coalesced"] == 1 and s["mark_nonces"] == hi - lo + 1
    # a request one cap above the class runs through p1hip_scan_below's own path
    dev.reset_stats()
    assert dev.scan_below_batch([(b"bradfitz", lo, hi, 1 << 46, 3), (b"msg", 0, 9, U64_MAX, 2)]) == \
        [E.below(1 << 46, cap=3), [(dev.hash(b"msg", 0), 0), (dev.hash(b"msg", 1), 1)]]
    s = dev.get_below_batch_stats()
    assert s["individual"] == 1 and s["coalesced"] == 1 and dev.get_below_stats()["calls"] == 1


# ---------------------------------------------------------------------------
# (f): k_belowb_collect alone on crafted words
# ---------------------------------------------------------------------------
def collect_model(words, tile0, hit0):
    """(idx, count) by integer arithmetic: per request the indices 64 * word +
    bit of its first set bits, in word and bit order, as many as it has slots."""
    idx, count = [UNWRITTEN] * hit0[-1], []
    for r in range(len(tile0) - 1):
        slots, keep = hit0[r + 1] - hit0[r], []
        for w in range(4 * tile0[r], 4 * tile0[r + 1]):
            if len(keep) >= slots:
                break
            x = words[w]
            if x == FULL:
                keep.extend(range(64 * w, 64 * w + 64))
            while x and x != FULL:
                keep.append(64 * w + (x & -x).bit_length() - 1)
                x &= x - 1
        keep = keep[:slots]
        idx[hit0[r]:hit0[r] + len(keep)] = keep
        count.append(len(keep))
    return idx, count


FULL = (1 << 64) - 1
# words per request: one tile; 259 tiles, whose last chunk of 256 words is ragged; more than 64 chunks
SIZES = (4, 1036, 16388)


def patterns(n):
    yield [0] * n
    yield [FULL] * n
    for w, b in ((0, 0), (0, 63), (n - 1, 0), (n - 1, 63)):  # a single bit: lane 0 and lane 63 of the first and the last word
        words = [0] * n
        words[w] = 1 << b
        yield words
    yield [(0x9E3779B97F4A7C15 * (i + 1)) & FULL if i % 3 else 0 for i in range(n)]


@pytest.mark.parametrize("n", SIZES)
def test_below_collect_crafted_words(dev, n):
    """Every pattern as a request of n words meets every slot count: zero, one, one that
    ends inside a word, one that ends with a chunk of 256 full words, exactly every bit, and
    more.  The requests of a launch are neighbours with different slot counts; a launch is
    closed before its slots pass the library's limit."""
    slot_kinds = (0, 1, 100, 64 * 256, 64 * n, 64 * n + 7)
    launches = [([], [0], [0])]
    for pat in patterns(n):
        for slots in slot_kinds:
            if launches[-1][2][-1] + slots > dev.BELOW_BATCH_MAX_SLOTS:
                launches.append(([], [0], [0]))
            words, tile0, hit0 = launches[-1]
            words += pat
            tile0.append(tile0[-1] + n // 4)
            hit0.append(hit0[-1] + slots)
    assert (len(launches) > 1) == (n == 16388) and all(h[-1] <= dev.BELOW_BATCH_MAX_SLOTS for _, _, h in launches)
    for words, tile0, hit0 in launches:
        idx, count = dev.below_collect(words, tile0, hit0)
        want_idx, want_count = collect_model(words, tile0, hit0)
        assert count == want_count
        assert idx == want_idx
    assert dev.get_below_batch_stats()["calls"] == 0  # the hook counts in no statistics


def test_below_collect_neighbours_of_all_sizes(dev):
    """The three sizes in one launch, an empty request between them, slot counts that end
    inside a word and exactly at the end of a chunk of 256 full words."""
    words = [FULL] * 4 + [FULL] * 1036 + [(1 << 63) | 1] * 16388
    tile0 = [0, 1, 1, 260, 4357]
    hit0 = [0, 70, 75, 75 + 64 * 256, 75 + 64 * 256 + 2 * 256 + 1]
    idx, count = dev.below_collect(words, tile0, hit0)
    assert (idx, count) == collect_model(words, tile0, hit0)
    assert count == [70, 0, 64 * 256, 513] and UNWRITTEN in idx[70:75] and idx[-1] == 64 * (1040 + 256)


# ---------------------------------------------------------------------------
# (g), (h), (i): devices, neighbours, code objects
# ---------------------------------------------------------------------------
def test_below_batch_two_logical_devices(dev, oracle_mod, monkeypatch):
    """GPU 0 listed twice (P1HIP_NO_RCCL): the round is cut across both, each
    enqueued on its own stream; the lists are the one-device lists."""
    reqs, want = below_batch_cases.matrix(oracle_mod)
    rreqs, rwant = below_batch_cases.rounds(oracle_mod)
    monkeypatch.setenv("P1HIP_NO_RCCL", "1")
    dev.shutdown()
    dev.init_devices([0, 0])
    try:
        dev.reset_stats()
        lay = dev.below_batch_layout(reqs, 2)
        assert {x["device"] for x in lay} == {-1, 0, 1}
        assert dev.scan_below_batch(reqs) == want
        s = dev.get_below_batch_stats()
        assert s["rounds"] == 1 and s["launches"] == 2
        monkeypatch.setenv("P1HIP_BELOW_MAX_SLICE", "1000")
        assert dev.scan_below_batch(rreqs) == rwant
        assert dev.get_below_batch_stats()["rounds"] == 1 + 5
    finally:
        monkeypatch.delenv("P1HIP_NO_RCCL")
        dev.shutdown()
        dev.init_devices([0])


def test_below_batch_leaves_its_neighbours_alone(dev, oracle_mod):
    """An outstanding batch_submit ticket, a scan and a scan_below around the
    call: all four answers are what they are alone."""
    small = [(b"ticket %d" % i, 10 ** 6 + 1000 * i, 10 ** 6 + 1000 * i + 999) for i in range(40)]
    a, lo, hi = tile_cases.QUEUE_RANGES[1]
    E = Expect(oracle_mod, a, lo, hi)
    target = E.nth(7)
    reqs, want = below_batch_cases.rounds(oracle_mod)
    ticket = dev.batch_submit(small)
    first = dev.scan(a, lo, hi)
    below1 = dev.scan_below(a, lo, hi, target, cap=100)
    got = dev.scan_below_batch(reqs)
    below2 = dev.scan_below(a, lo, hi, target, cap=100)
    second = dev.scan(a, lo, hi)
    again = dev.scan_below_batch(reqs)
    got_small = dev.batch_wait(ticket)
    assert got == want and again == want
    assert below1 == below2 == E.below(target)
    assert first == second == E.minimum
    assert got_small == [oracle_mod.scan(m, x, y) for m, x, y in small]


def test_below_batch_code_objects(gpu):
    import test_gpu_below

    assert gpu.codeobj_sha256() == test_gpu_below.SCAN_CODEOBJ
    assert gpu.batch_codeobj_sha256() == test_gpu_below.BATCH_CODEOBJ
    assert gpu.below_codeobj_sha256() == BELOW_CODEOBJ
    new = gpu.belowb_codeobj_sha256()
    assert len(new) == 64 and new not in (test_gpu_below.SCAN_CODEOBJ, test_gpu_below.BATCH_CODEOBJ, BELOW_CODEOBJ)
