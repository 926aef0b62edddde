"""GPU tests of p1hip_scan_below_batch_wide: many (message, range, target, cap)
searches in one call, the hard-target ones sharing k_scan launches and the
filter kernel, each answered exactly as p1hip_scan_below answers it.

Every expected list is the reference loop, brute force by the oracle
(below_cases.Expect), and equality is exact.  The request lists are those of
the CPU replay in tests/test_below_wide_host.py (below_wide_cases.py)."""
import pytest

import below_batch_cases
import below_wide_cases
import tile_cases
from below_cases import FLOOR, U64_MAX, Expect, increasing, resume_chain

pytestmark = pytest.mark.gpu

BELOWB_CODEOBJ = "28e6870b7069761e266140f1848adc299fae9055590582d4c071ff8d4556cf51"  # profiles/below_batch_bench.json
UNWRITTEN = (1 << 32) - 1
KNOBS = ("P1HIP_BELOW_PATH", "P1HIP_BELOW_MAX_SLICE", "P1HIP_BELOW_WIDE_MAX_SLOTS", "P1HIP_WIDE_MIN_FAST_THREADS",
         "P1HIP_WIDE_MAX_SEGS")


@pytest.fixture
def dev(gpu, monkeypatch):
    """Device 0 alone, the per-call knobs of the call cleared, fresh statistics."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    if gpu.device_count() != 1:
        gpu.shutdown()
        gpu.init_devices([0])
    gpu.reset_stats()
    return gpu


def sparse_slices(reqs, forced):
    return [(lo, hi) for _, lo, hi, t, cap in reqs if lo <= hi and cap and (forced or (t < 1 << 46 and hi - lo >= 1 << 16))]


# ---------------------------------------------------------------------------
# The mixed list, in one round and in several
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("forced", [False, True])
def test_below_wide_mixed(dev, oracle_mod, monkeypatch, forced):
    reqs, want, filtered = below_wide_cases.mixed(oracle_mod, forced)
    monkeypatch.setenv("P1HIP_WIDE_MIN_FAST_THREADS", str(FLOOR))
    if forced:
        monkeypatch.setenv("P1HIP_BELOW_PATH", "1")
    assert dev.scan_below_batch_wide(reqs) == want
    s = dev.get_below_wide_stats()
    print(s)
    assert s["calls"] == 1 and s["requests"] == len(reqs) and s["empty"] == 3 and s["filtered"] == filtered
    assert s["coalesced"] == len(reqs) - 3 - filtered and s["individual"] == 0
    assert s["groups"] == s["filter_launches"] == 1 and s["slot_overflows"] == 0
    assert s["rounds"] == (1 if forced else 2)  # the coalesced cell needs a second dense slice
    assert s["candidate_tiles"] >= filtered and s["hits"] == sum(len(w) for w in want)
    if not forced:  # every filtered request's one slice is its whole range
        assert s["scan_nonces"] == sum(hi - lo + 1 for lo, hi in sparse_slices(reqs, forced))
    # the same requests through p1hip_scan_below_batch, which runs the filtered ones one by one
    assert dev.scan_below_batch(reqs) == want
    assert dev.get_below_batch_stats()["individual"] == filtered


def test_below_wide_rounds_and_launches(dev, oracle_mod, monkeypatch):
    """A slice cap of 200000 and two segments per k_scan launch: three rounds, a
    request's ranges in several launches."""
    reqs, want, filtered = below_wide_cases.mixed(oracle_mod, False)
    monkeypatch.setenv("P1HIP_WIDE_MIN_FAST_THREADS", str(FLOOR))
    monkeypatch.setenv("P1HIP_BELOW_MAX_SLICE", "200000")
    monkeypatch.setenv("P1HIP_WIDE_MAX_SEGS", "2")
    assert dev.scan_below_batch_wide(reqs) == want
    s = dev.get_below_wide_stats()
    print(s)
    assert s["rounds"] == 3 == s["groups"] and s["filtered"] == filtered and s["scan_launches"] > s["groups"]
    assert s["scan_segments"] > s["scan_launches"]


def test_below_wide_last_slice_turns_dense(dev, oracle_mod, monkeypatch):
    E = next(E for E in below_wide_cases.cells(oracle_mod) if E.nth(1) < 1 << 46)
    monkeypatch.setenv("P1HIP_WIDE_MIN_FAST_THREADS", str(FLOOR))
    monkeypatch.setenv("P1HIP_BELOW_MAX_SLICE", "250000")
    assert dev.scan_below_batch_wide([(E.msg, E.lo, E.hi, E.nth(1), 100)]) == [E.below(E.nth(1))]
    s = dev.get_below_wide_stats()
    assert s["filtered"] == 1 and s["coalesced"] == 0 and s["rounds"] == 3 and s["groups"] == 2
    assert s["scan_nonces"] == 500000 and s["mark_launches"] >= 2  # two slices filtered, the third marked whole


# ---------------------------------------------------------------------------
# Library defaults: the pool's hard share target
# ---------------------------------------------------------------------------
WORKERS = (0, 1, 2, 3, 4, 5, 13, 21)
# the first nonce of [0, 2^32) at or below 2^44, by the oracle; workers 13 and 21 have none in [0, 2^21)
WORKER_HITS = [(13943714821149, 1648573), (4695866226357, 593281), (4760903520533, 862764), (8124437029075, 1869531),
               (3619863100506, 126327), (3830426266274, 863278), (9269484857478, 4058822), (10680350058760, 2387275)]


def test_below_wide_pool_workers_at_defaults(dev, oracle_mod):
    assert not any(dev.test_knobs().get(k) for k in KNOBS)
    target = 1 << 44
    reqs = [(b"worker %d" % i, 0, 2 ** 32 - 1, target, 1) for i in WORKERS]
    # the pinned list is the oracle's: the whole prefix for a worker of each kind, the hit's hash for all
    for j in (4, 7):
        E = Expect(oracle_mod, reqs[j][0], 0, WORKER_HITS[j][1])
        assert E.below(target) == [WORKER_HITS[j]]
    assert all(oracle_mod.hashes(q[0], n, 1)[0] == h <= target for q, (h, n) in zip(reqs, WORKER_HITS))
    lay = dev.below_wide_layout(reqs, 1)
    assert all(x["route"] == "filtered" and x["slots"] == 28 and x["device"] == 0 for x in lay)
    assert dev.scan_below_batch_wide(reqs) == [[w] for w in WORKER_HITS]
    s = dev.get_below_wide_stats()
    print(s)
    assert s["filtered"] == 8 and s["coalesced"] == 0 == s["individual"] and s["rounds"] == 2 == s["groups"]
    assert s["scan_nonces"] == 10 << 21 and s["slot_overflows"] == 0 and s["hits"] == 8
    # what comes back: per round a count per request and its 28 slots, 16 bytes per candidate tile, and the
    # candidates' marks, 4 words per mark tile -- against 16 bytes per k_scan tile
    assert s["bytes_back"] == 4 * (10 + 10 * 28) + 16 * s["candidate_tiles"] + 32 * s["mark_tiles"]
    assert 8 * s["bytes_back"] < 16 * sum(x["tiles"] for x in lay)
    # p1hip_scan_below_batch runs every one of them individually
    dev.reset_stats()
    assert dev.scan_below_batch(reqs[:2]) == [[w] for w in WORKER_HITS[:2]]
    assert dev.get_below_batch_stats()["individual"] == 2


# ---------------------------------------------------------------------------
# cap > 1: candidate tiles of different pieces, table order against nonce order
# ---------------------------------------------------------------------------
def test_below_wide_hits_in_different_pieces(dev, oracle_mod, monkeypatch):
    """A range that straddles 10^6 has a fast piece per decade, laid out
    longest-running first and not in nonce order, and ragged generic pieces
    behind them in the range table: two hits on either side of the boundary."""
    E = Expect(oracle_mod, b"straddle 2", 10 ** 6 - 300000, 10 ** 6 + 299999)
    target = E.nth(3)
    want = E.below(target)
    assert [n for _, n in want] == [718108, 853984, 1143884, 1172457]
    monkeypatch.setenv("P1HIP_WIDE_MIN_FAST_THREADS", str(FLOOR))
    monkeypatch.setenv("P1HIP_BELOW_PATH", "1")
    wide = dev.scan_below_batch_wide
    got = wide([(E.msg, E.lo, E.hi, target, 9), (E.msg, E.lo, E.hi, target, 3), (E.msg, E.lo, E.hi, target, 4)])
    assert got == [want, want[:3], want] and increasing(got[0])
    s = dev.get_below_wide_stats()
    assert s["candidate_tiles"] >= 3 * 2 and s["filtered"] == 3
    # found == cap: there may be more, the caller resumes behind the last nonce
    assert resume_chain(lambda lo: wide([(E.msg, lo, E.hi, target, 1)])[0], E.lo, E.hi) == want


# ---------------------------------------------------------------------------
# The overflow fallback on the device
# ---------------------------------------------------------------------------
def test_below_wide_every_nonce_and_the_overflow_fallback(dev, oracle_mod, monkeypatch):
    lo = 10 ** 6 - 1500
    E = Expect(oracle_mod, b"bradfitz", lo, lo + 2999)
    S = below_wide_cases.small(oracle_mod)
    reqs = [(E.msg, E.lo, E.hi, U64_MAX, 5000), (S.msg, S.lo, S.hi, S.nth(3), 10)]
    want = [E.first(3000), S.below(S.nth(3))]
    monkeypatch.setenv("P1HIP_BELOW_PATH", "1")
    # the slot rule gives a slot per tile at this target: every tile is a candidate, nothing overflows
    assert dev.scan_below_batch_wide(reqs) == want
    s = dev.get_below_wide_stats()
    assert s["slot_overflows"] == 0 and s["filtered"] == 2 and s["candidate_tiles"] >= 3
    # one slot per request: the filter reports more candidates than slots, the host filter answers
    monkeypatch.setenv("P1HIP_BELOW_WIDE_MAX_SLOTS", "1")
    dev.reset_stats()
    assert dev.scan_below_batch_wide(reqs) == want
    s1 = dev.get_below_wide_stats()
    assert s1["slot_overflows"] == 1 and s1["candidate_tiles"] == s["candidate_tiles"]
    assert s1["mark_nonces"] == s["mark_nonces"]


# ---------------------------------------------------------------------------
# k_beloww_filter alone on crafted partials
# ---------------------------------------------------------------------------
IDENTITY = (U64_MAX, U64_MAX)
SIZES = (1, 255, 256, 257, 513, 16388)  # 16388: more than 64 chunks of 256 tiles
PATTERNS = ("none", "all", "first", "last", "third")


def flagged(pattern, t, n):
    return {"none": False, "all": True, "first": t == 0, "last": t == n - 1,
            "third": (0x9E3779B97F4A7C15 * (t + 1) >> 40) % 3 == 0}[pattern]


def filter_model(part, ranges, range0, targets, slot0):
    """(cand, count) by integer arithmetic: per request the indices of its tiles
    with hash <= target, range after range, as many as it has slots; the count
    of all of them."""
    cand, count = [UNWRITTEN] * slot0[-1], []
    for r in range(len(range0) - 1):
        keep = [t for a, n in ranges[range0[r]:range0[r + 1]] for t in range(a, a + n) if part[t][0] <= targets[r]]
        count.append(len(keep))
        keep = keep[:slot0[r + 1] - slot0[r]]
        cand[slot0[r]:slot0[r] + len(keep)] = keep
    return cand, count


def crafted_launch():
    """One launch: every size meets every pattern; request k has 1 + k % 3 ranges
    (the size's, then one of 257 and one of 1 tile), never adjacent in the array
    (a gap of 3 tiles that would all pass lies between any two); a candidate's
    hash is the target itself or below it, another tile's is target + 1 or far
    above; the slot count is 0, 1, one that ends inside a chunk, exactly the
    total, or more, and changes from neighbour to neighbour; identity keys under a
    small target and under UINT64_MAX; an empty request between the others."""
    part, ranges, range0, targets, slot0 = [], [], [0], [], [0]
    k = 0

    def add(sizes, pattern, target, slot_kind, identity=False):
        total = 0
        for n in sizes:
            part.extend([(0, 7)] * 3)  # the gap
            ranges.append((len(part), n))
            for t in range(n):
                if identity:
                    part.append(IDENTITY)
                elif flagged(pattern, t, n):
                    part.append((target if t % 2 else target - 1 - t, t))
                    total += 1
                else:
                    part.append((target + 1 if t % 2 else target + 10 ** 6 + t, t))
        if identity:
            total = sum(sizes) if target == U64_MAX else 0
        range0.append(len(ranges))
        targets.append(target)
        slot0.append(slot0[-1] + (0, 1, 100, total, total + 5)[slot_kind])

    for size in SIZES:
        for p, pattern in enumerate(PATTERNS):
            add(([size, 257, 1])[:1 + k % 3], pattern, 10 ** 15 + k, (k // 5 + p) % 5)
            k += 1
            if k % 7 == 0:  # an empty request: no range, and slots it must not touch
                range0.append(len(ranges))
                targets.append(U64_MAX)
                slot0.append(slot0[-1] + 2)
    add([300, 2], "all", 12345, 3, identity=True)
    add([300, 2], "all", U64_MAX, 2, identity=True)
    add([300], "all", U64_MAX, 4, identity=True)
    part.extend([(0, 7)] * 3)
    return part, ranges, range0, targets, slot0


def test_below_filter_crafted_partials(dev):
    part, ranges, range0, targets, slot0 = crafted_launch()
    assert len(targets) == 30 + 4 + 3 and max(range0[r + 1] - range0[r] for r in range(len(targets))) == 3
    cand, count = dev.below_filter(part, ranges, range0, targets, slot0)
    want_cand, want_count = filter_model(part, ranges, range0, targets, slot0)
    assert count == want_count
    assert cand == want_cand
    slots = [slot0[r + 1] - slot0[r] for r in range(len(targets))]
    # with fewer slots than candidates the count is the total and nothing past the slots is written
    assert any(c > s > 0 for c, s in zip(count, slots)) and any(c > s == 0 for c, s in zip(count, slots))
    assert any(0 < c == s for c, s in zip(count, slots)) and any(0 < c < s for c, s in zip(count, slots))
    assert UNWRITTEN in cand and count[-3:] == [0, 302, 300]
    assert dev.get_below_wide_stats()["calls"] == 0  # the hook counts in no statistics


# ---------------------------------------------------------------------------
# Devices, neighbours, code objects
# ---------------------------------------------------------------------------
def test_below_wide_two_logical_devices(dev, oracle_mod, monkeypatch):
    """GPU 0 listed twice (P1HIP_NO_RCCL): a group is cut across both, each
    enqueued on its own stream and refined on its own device; the lists are the
    one-device lists."""
    reqs, want, filtered = below_wide_cases.mixed(oracle_mod, False)
    monkeypatch.setenv("P1HIP_NO_RCCL", "1")
    monkeypatch.setenv("P1HIP_WIDE_MIN_FAST_THREADS", str(FLOOR))
    dev.shutdown()
    dev.init_devices([0, 0])
    try:
        dev.reset_stats()
        lay = dev.below_wide_layout(reqs, 2)
        assert {x["device"] for x in lay if x["route"] == "filtered"} == {0, 1}
        assert dev.scan_below_batch_wide(reqs) == want
        s = dev.get_below_wide_stats()
        assert s["groups"] == 1 and s["filter_launches"] == 2 and s["filtered"] == filtered
        monkeypatch.setenv("P1HIP_BELOW_MAX_SLICE", "200000")
        assert dev.scan_below_batch_wide(reqs) == want
        assert dev.get_below_wide_stats()["rounds"] == 2 + 3
    finally:
        monkeypatch.delenv("P1HIP_NO_RCCL")
        dev.shutdown()
        dev.init_devices([0])


def test_below_wide_leaves_its_neighbours_alone(dev, oracle_mod, monkeypatch):
    """An outstanding batch_submit ticket, a scan, a scan_below and a
    scan_below_batch around the call: all answers are what they are alone."""
    small = [(b"ticket %d" % i, 10 ** 6 + 1000 * i, 10 ** 6 + 1000 * i + 999) for i in range(40)]
    a, lo, hi = tile_cases.QUEUE_RANGES[1]
    E = Expect(oracle_mod, a, lo, hi)
    target = E.nth(7)
    breqs, bwant = below_batch_cases.rounds(oracle_mod)
    reqs, want, _ = below_wide_cases.mixed(oracle_mod, False)
    monkeypatch.setenv("P1HIP_WIDE_MIN_FAST_THREADS", str(FLOOR))
    ticket = dev.batch_submit(small)
    first = dev.scan(a, lo, hi)
    below1 = dev.scan_below(a, lo, hi, target, cap=100)
    batch1 = dev.scan_below_batch(breqs)
    got = dev.scan_below_batch_wide(reqs)
    batch2 = dev.scan_below_batch(breqs)
    below2 = dev.scan_below(a, lo, hi, target, cap=100)
    second = dev.scan(a, lo, hi)
    again = dev.scan_below_batch_wide(reqs)
    got_small = dev.batch_wait(ticket)
    assert got == want and again == want
    assert batch1 == batch2 == bwant
    assert below1 == below2 == E.below(target)
    assert first == second == E.minimum
    assert got_small == [oracle_mod.scan(m, x, y) for m, x, y in small]


def test_below_wide_code_objects(gpu):
    import test_gpu_below
    import test_gpu_below_batch

    pinned = (test_gpu_below.SCAN_CODEOBJ, test_gpu_below.BATCH_CODEOBJ, test_gpu_below_batch.BELOW_CODEOBJ, BELOWB_CODEOBJ)
    assert (gpu.codeobj_sha256(), gpu.batch_codeobj_sha256(), gpu.below_codeobj_sha256(),
            gpu.belowb_codeobj_sha256()) == pinned
    new = gpu.beloww_codeobj_sha256()
    assert len(new) == 64 and int(new, 16) >= 0 and new not in pinned
