"""k_scan as a work queue (round 6): the grid is the device's workgroup slots
and the tiles beyond it are handed out through a counter that the last
workgroup of every launch zeroes for the next one (p1hip_kernels.hip
k_scan).  A counter left non-zero would make the next launch skip tiles
without any error, so these scans are built to fail if that ever happens:
the minimum of each range lies in a tile far past the first grid's worth,
and ranges of very different tile counts alternate on the same stream, in
one launch and split into many launches (P1HIP_MAX_LAUNCH_BLOCKS).
That samples one planted tile of a 2^32-nonce grid; tests/test_gpu_tiles.py
is the whole-grid form of the same property: every tile's partial of a scan,
read back from a poisoned partial array, against the oracle's minimum over
that tile's nonces.

Answers: the survey's hashlib pin of configs[1] ([0, 2^32) of "bradfitz":
(5256245051, 1626825724)) and the CPU oracle.
Reference: miner.go:56-63."""
import pytest

pytestmark = pytest.mark.gpu

C2 = (b"bradfitz", 0, (1 << 32) - 1)
C2_MIN = (5256245051, 1626825724)


def test_alternating_ranges_keep_every_tile(gpu, large):
    assert large[C2] == C2_MIN
    # [0, 1626825724]: the min is the range's last nonce, in the last tile of
    # the d = 10 piece (~2,400 tiles of 256 threads x 1000 nonces), far past
    # the first 1,024 the grid starts with
    short = (b"bradfitz", 0, C2_MIN[1])
    mid = (b"bradfitz", 10**9, C2_MIN[1])  # the same min, a different tile count and layout
    for i in range(6):
        assert gpu.scan(*C2) == C2_MIN, i
        assert gpu.scan(*short) == C2_MIN, i
        assert gpu.scan(*mid) == C2_MIN, i


def test_many_launches_per_scan_keep_every_tile(gpu, monkeypatch):
    """The same scans split into launches of at most 1,500 tiles: every
    launch past the first starts from the counter the previous one zeroed."""
    monkeypatch.setenv("P1HIP_MAX_LAUNCH_BLOCKS", "1500")
    try:
        gpu.reset_stats()
        assert gpu.scan(*C2) == C2_MIN
        assert gpu.get_stats()["scan_launches"] >= 4
        assert gpu.scan(b"bradfitz", 10**9, C2_MIN[1]) == C2_MIN
        assert gpu.scan(*C2) == C2_MIN
    finally:
        monkeypatch.delenv("P1HIP_MAX_LAUNCH_BLOCKS")
    assert gpu.scan(*C2) == C2_MIN


def test_segment_tables_regrow_and_are_kept(gpu, oracle_mod, monkeypatch):
    """One workgroup per launch: "bradfitz" [1, 200000] needs more launch
    slots than the segment tables' first allocation of 4, so they are freed
    and regrown before the first launch; the next scan runs one launch on the
    kept, larger buffers, and a scan of configs[0]'s range follows."""
    want = oracle_mod.scan(b"bradfitz", 1, 200000, threads=8)
    monkeypatch.setenv("P1HIP_MAX_LAUNCH_BLOCKS", "1")
    try:
        gpu.reset_stats()
        assert gpu.scan(b"bradfitz", 1, 200000) == want
        assert gpu.get_stats()["scan_launches"] >= 5
    finally:
        monkeypatch.delenv("P1HIP_MAX_LAUNCH_BLOCKS")
    gpu.reset_stats()
    assert gpu.scan(b"bradfitz", 1, 200000) == want
    assert gpu.get_stats()["scan_launches"] == 1
    monkeypatch.setenv("P1HIP_SMALL_MAX_NONCES", str(1 << 16))  # the session runs with the small path off
    try:
        assert gpu.scan(b"bradfitz", 0, 9999) == (1419516646206828, 9898)
        assert gpu.get_stats()["small_scans"] == 1
    finally:
        monkeypatch.setenv("P1HIP_SMALL_MAX_NONCES", "0")


def test_small_and_queued_scans_interleave(gpu, oracle_mod):
    """Scans below one grid (no queue: one tile per workgroup) between
    queued ones, checked against the oracle."""
    for lo in (10**9 + 7, 3 * 10**9 + 11, 4 * 10**9 + 5):
        small = gpu.scan(b"cmu440", lo, lo + 300_000)
        assert small == oracle_mod.scan(b"cmu440", lo, lo + 300_000, threads=8), lo
        assert gpu.scan(*C2) == C2_MIN
