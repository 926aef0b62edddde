"""The pipelined miner pool without a GPU.

`tools/pool_pipeline_test` checks miner::Pipeline (up to `depth` rounds
outstanding over miner::Rounds) against the oracle's direct scans.
`tools/lsp_fake_pool_async` is the real miner::RunPool with --inflight N over
a backend that answers with the CPU oracle on a worker thread -- like the GPU,
it works while the round loop goes on -- behind the real `p1server lsp`:
concurrent clients, 20% loss, the server dying and SIGTERM with rounds
outstanding.

Reference: miner.go:49-67 (every connection is a miner to the server; every
Result is that loop's)."""
import json
import os
import subprocess
import time

import pytest

import test_pool_host as tph
from conftest import ROOT, host_bin

POOL = host_bin(os.path.join(ROOT, "tools", "lsp_fake_pool_async"))
PIPELINE_TEST = host_bin(os.path.join(ROOT, "tools", "pool_pipeline_test"))


@pytest.fixture(scope="module", autouse=True)
def built():
    for t in (POOL, PIPELINE_TEST):
        if not os.path.exists(t):
            subprocess.run(["make", "-s", "-C", ROOT, os.path.relpath(t, ROOT)], check=True)


class System(tph.System):
    def pool(self, args, env=None):
        p = subprocess.Popen([POOL, self.hostport] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                             text=True, env=dict(self.env, **(env or {})))
        self.procs.append(p)
        return p


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


def test_pipeline_unit():
    r = subprocess.run([PIPELINE_TEST], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "all passed" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("inflight", [1, 2, 4])
def test_concurrent_clients(system, oracle_mod, tmp_path, inflight):
    log = tmp_path / "rounds.txt"
    s = system(["--chunk", "500"])
    pool = s.pool(["--conns", "6", "--inflight", str(inflight), "--round-log", str(log), "--stats"],
                  env={"FAKE_ROUND_SLEEP_MS": "3"})
    jobs = [("a", 7000), ("bb", 3000), ("bradfitz", 9999), ("x" * 70, 5000)]
    procs = [s.start_client(m, mx) for m, mx in jobs]
    for (m, mx), p in zip(jobs, procs):
        assert tph.answer(p) == tph.want(oracle_mod, m, mx), m
    rc, st, err = tph.stop(pool)
    assert rc == 0, err
    assert st["conns_open"] == 6 and st["lost_conns"] == 0, st
    assert st["inflight"] == inflight and 1 <= st["max_outstanding"] <= inflight, st
    rounds = tph.read_log(log)  # a line per round, written at submit, counting up from 0
    assert len(rounds) == st["rounds"] and sum(len(p) for _, p in rounds) == st["pieces"], st
    assert st["requests"] == 15 + 7 + 20 + 11 and st["pieces"] == st["requests"], st


def test_long_job_overlaps_short_ones(system, oracle_mod, tmp_path):
    """The pool cuts a long job itself (--chunk 1000, 25 ms a round); short
    jobs on other connections go out in rounds of their own while the long
    job's piece is outstanding, and a job never has two pieces out."""
    log = tmp_path / "rounds.txt"
    s = system(["--chunk", str(1 << 40)])  # the server does not split
    pool = s.pool(["--conns", "3", "--inflight", "2", "--chunk", "1000", "--round-log", str(log), "--stats"],
                  env={"FAKE_ROUND_SLEEP_MS": "25"})
    a = s.start_client("bradfitz", 29999)  # 30 pieces
    time.sleep(0.2)
    b = s.start_client("bradfitz", 999)
    c = s.start_client("msg", 1500)
    assert tph.answer(b) == tph.want(oracle_mod, "bradfitz", 999)
    assert tph.answer(c) == tph.want(oracle_mod, "msg", 1500)
    assert tph.answer(a) == tph.want(oracle_mod, "bradfitz", 29999)
    rc, st, err = tph.stop(pool)
    assert rc == 0, err
    assert st["inflight"] == 2 and st["max_outstanding"] == 2 and st["requests"] == 3, st
    assert st["pieces"] == 30 + 1 + 2, st
    rounds = tph.read_log(log)
    # every connection's pieces are contiguous and in nonce order over the rounds
    last = {}
    for _, pieces in rounds:
        for conn, lo, up in pieces:
            assert (lo == 0 or lo == last[conn] + 1) and up - lo < 1000, (conn, lo, up)  # lo == 0: a new job
            last[conn] = up
    assert {999, 1500, 29999} <= {up for _, pieces in rounds for _, _, up in pieces}


def test_write_drop_everywhere(system, oracle_mod):
    env = {"P1LSP_WRITE_DROP": "20"}
    prm = ["--epoch-millis", "50", "--epoch-limit", "20", "--window", "4"]
    s = system(["--chunk", "3000"] + prm, env=env)
    pool = s.pool(["--conns", "3", "--inflight", "2", "--stats"] + prm, env={"FAKE_ROUND_SLEEP_MS": "2"})
    c = s.start_client("bradfitz", 49999, args=prm)
    assert tph.answer(c, timeout=120) == tph.want(oracle_mod, "bradfitz", 49999)
    rc, st, err = tph.stop(pool, timeout=60)
    assert rc == 0, err
    assert 1 <= st["conns_open"] <= 3 and st["requests"] >= 17 and st["max_outstanding"] <= 2, st


def test_server_dies_with_rounds_outstanding(system):
    prm = ["--epoch-millis", "100", "--epoch-limit", "5"]
    s = system(["--chunk", str(1 << 40)] + prm)
    pool = s.pool(["--conns", "2", "--inflight", "2", "--chunk", "1000", "--stats"] + prm,
                  env={"FAKE_ROUND_SLEEP_MS": "50"})
    s.start_client("bradfitz", 10 ** 6, args=prm)  # 1000 rounds of 50 ms: never finishes here
    time.sleep(0.2)  # the second job arrives while the first one's piece is out: a round of its own
    s.start_client("msg", 10 ** 6, args=prm)
    time.sleep(0.4)
    s.server.kill()
    s.server.wait(timeout=30)
    out, err = pool.communicate(timeout=20)  # every connection is lost after 5 epochs of 100 ms
    assert pool.returncode == 0, err
    st = json.loads([x for x in out.splitlines() if x.startswith("{")][-1])
    assert st["conns_open"] == 2 and st["lost_conns"] == 2 and st["rounds"] >= 2, st
    assert st["max_outstanding"] == 2, st


def test_sigterm_with_rounds_outstanding(system):
    s = system(["--chunk", str(1 << 40)])
    pool = s.pool(["--conns", "2", "--inflight", "2", "--chunk", "1000", "--stats"],
                  env={"FAKE_ROUND_SLEEP_MS": "50"})
    s.start_client("bradfitz", 10 ** 6)
    time.sleep(0.2)  # as above
    s.start_client("msg", 10 ** 6)
    time.sleep(0.4)
    rc, st, err = tph.stop(pool, timeout=20)  # the outstanding rounds are collected, then the clients closed
    assert rc == 0, err
    assert st["max_outstanding"] == 2 and st["rounds"] >= 2 and st["requests"] == 0, st


def test_inflight_is_checked_before_the_gpu_is_opened():
    miner = os.path.join(ROOT, "p1_amd", "p1miner")
    for bad in (["--conns", "2", "--inflight", "0"], ["--conns", "2", "--inflight", "5"], ["--inflight", "2"]):
        r = subprocess.run([miner, "lsp", "127.0.0.1:9"] + bad, capture_output=True, text=True, timeout=30)
        assert r.returncode == 2 and "usage" in r.stderr, (bad, r.stdout, r.stderr)
