"""The pipelined miner pool on the GPU: one `p1miner lsp --device 0 --conns 8
--wide --inflight 2` process behind a real `p1server lsp`, with real
`p1client`s.  Every round goes through p1hip_batch_submit / p1hip_batch_wait
(miner::SubmitPieces / CollectPieces), up to two rounds outstanding; every
Result must equal the oracle's, over every route of the wide call, with a
long job cut into pieces while short jobs arrive on other connections, and
with 5% of every write lost.

At most two processes have the GPU open: the miner and this one."""

import pytest

from test_gpu_pool import System, answer, read_log, stop

pytestmark = pytest.mark.gpu


@pytest.fixture
def system():
    made = []

    def make(*a, **k):
        s = System(*a, **k)
        made.append(s)
        return s

    yield make
    for s in made:
        s.close()


def check_stats(st):
    assert st["inflight"] == 2 and 1 <= st["max_outstanding"] <= 2, st
    assert st["lost_conns"] == 0, st


def test_every_route_with_two_rounds_in_flight(system, oracle_mod, tmp_path):
    """The jobs of tests/test_gpu_pool.py::test_every_route_in_one_pool: one
    size per route or edge of p1hip_scan_batch_wide (the individual ones run
    in p1hip_batch_wait)."""
    log = tmp_path / "rounds.txt"
    s = system(["--chunk", str(1 << 40)])
    miner = s.miner(["--conns", "8", "--wide", "--inflight", "2", "--linger-us", "50000", "--round-log", str(log),
                     "--stats"])
    jobs = [("bradfitz", 9999), ("edge-a", 65535), ("edge-b", 65536), ("w1", 10**5), ("w2", 3 * 10**5),
            ("w3", 10**6), ("edge-c", (1 << 24) - 1), ("edge-d", 1 << 24), ("big", 2 * 10**7),
            ("two-block-tail-" + "y" * 55, 10**5), ("r1", 10**5), ("r2", 10**5)]
    procs = [s.start_client(m, mx) for m, mx in jobs]
    got = [answer(p) for p in procs]
    assert got[0] == "Result 1419516646206828 9898"
    for (m, mx), g in zip(jobs, got):
        h, n = oracle_mod.scan(m, 0, mx, threads=8)
        assert g == f"Result {h} {n}", (m, mx)
    st = stop(miner)
    print(f"pool stats: {st}")
    check_stats(st)
    assert st["conns_open"] == 8 and st["requests"] == 12 and st["pieces"] == 12, st
    # every round is one wide call, whatever its size (no p1hip_scan shortcut for a round of one)
    assert st["wide"]["calls"] == st["rounds"] and st["wide"]["requests"] == 12, st
    assert st["wide"]["small"] == 2 and st["wide"]["individual"] == 2 and st["wide"]["wide"] == 8, st
    rounds = read_log(log)
    assert [r for r, _ in rounds] == list(range(st["rounds"])) and sum(len(p) for _, p in rounds) == 12


def test_long_job_is_cut_while_short_jobs_arrive(system, oracle_mod, gpu, tmp_path):
    """A: [0, 2^30) in 64 pieces of 2^24 (the wide route's largest); meanwhile
    10^4-nonce jobs arrive on the other connections, one after another.  A's
    pieces fold in nonce order; every short job is answered while A runs."""
    log = tmp_path / "rounds.txt"
    chunk, hi = 1 << 24, (1 << 30) - 1
    s = system(["--chunk", str(1 << 40)])
    miner = s.miner(["--conns", "8", "--wide", "--inflight", "2", "--chunk", str(chunk), "--round-log", str(log),
                     "--stats"])
    warm = s.start_client("warm", 0)  # once answered, the miner has opened the GPU and joined
    h0, n0 = oracle_mod.scan("warm", 0, 0)
    assert answer(warm) == f"Result {h0} {n0}"
    a = s.start_client("bradfitz", hi)
    shorts = []
    for i in range(6):
        p = s.start_client(f"short-{i}", 9999)
        shorts.append((f"short-{i}", p))
    for m, p in shorts:
        h, n = oracle_mod.scan(m, 0, 9999)
        assert answer(p) == f"Result {h} {n}", m
    word, h, n = answer(a).split()
    h, n = int(h), int(n)
    assert word == "Result" and oracle_mod.hash("bradfitz", n) == h
    assert (h, n) == gpu.scan("bradfitz", 0, hi)  # the synchronous call, in this process
    st = stop(miner)
    print(f"pool stats: {st}")
    check_stats(st)
    assert st["requests"] == 8 and st["pieces"] == 64 + 7, st
    rounds = read_log(log)
    a_pieces = [(lo, up) for _, p in rounds for _, lo, up in p if up - lo == chunk - 1]
    assert a_pieces == [(k * chunk, (k + 1) * chunk - 1) for k in range(64)]


def test_write_drop_with_two_rounds_in_flight(system, oracle_mod):
    """5% of every write lost in every process, as in tests/test_gpu_pool.py."""
    env = {"P1LSP_WRITE_DROP": "5"}
    prm = ["--window", "8", "--epoch-millis", "200"]
    s = system(["--chunk", "125000"] + prm, env=env)
    miner = s.miner(["--conns", "8", "--wide", "--inflight", "2", "--stats"] + prm)
    jobs = [(f"drop-{i}", 10**6 - 1) for i in range(4)]
    procs = [s.start_client(m, mx, args=prm) for m, mx in jobs]
    for (m, mx), p in zip(jobs, procs):
        h, n = oracle_mod.scan(m, 0, mx, threads=8)
        assert answer(p) == f"Result {h} {n}", m
    st = stop(miner)
    print(f"pool stats: {st}")
    assert st["inflight"] == 2 and 1 <= st["max_outstanding"] <= 2 and st["requests"] >= 32, st
