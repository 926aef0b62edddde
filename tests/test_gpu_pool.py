"""The multi-connection miner on the GPU: one `p1miner lsp --device 0 --conns C`
process behind a real `p1server lsp`, with real `p1client`s.  No new device
code runs here: what is covered is the existing kernels of p1hip_scan,
p1hip_scan_batch and p1hip_scan_batch_wide driven through LSP rounds
(miner::AnswerPieces), the fold of a job's pieces across those routes, and
the teardown of a process that holds the GPU and C connections.

At most two processes have the GPU open: the miner and this one."""
import json
import os
import signal
import subprocess
import time

import pytest

from conftest import ROOT, host_bin

SERVER = host_bin(os.path.join(ROOT, "p1_amd", "p1server"))
CLIENT = host_bin(os.path.join(ROOT, "p1_amd", "p1client"))
MINER = host_bin(os.path.join(ROOT, "p1_amd", "p1miner"))

pytestmark = pytest.mark.gpu


class System:
    """One server + one miner + clients; every process is ours and is killed
    by PID.  The children do not inherit the library's test knobs that the
    `gpu` fixture sets for this process: the miner runs as in production."""

    def __init__(self, args=(), env=None):
        base = {k: v for k, v in os.environ.items() if not k.startswith("P1HIP_")}
        self.env = dict(base, **(env or {}))
        self.procs = []
        self.server = subprocess.Popen([SERVER] + list(args) + ["lsp", "0"], stdout=subprocess.PIPE, text=True,
                                       env=self.env)
        self.procs.append(self.server)
        line = self.server.stdout.readline()  # server.go:79
        assert line.startswith("Server listening on port"), line
        self.port = int(line.split()[-1])
        self.hostport = f"127.0.0.1:{self.port}"

    def miner(self, args):
        p = subprocess.Popen([MINER, "lsp", self.hostport, "--device", "0"] + list(args), stdout=subprocess.PIPE,
                             stderr=subprocess.PIPE, text=True, env=self.env)
        self.procs.append(p)
        return p

    def start_client(self, msg, max_nonce, args=()):
        p = subprocess.Popen([CLIENT, self.hostport, msg, str(max_nonce)] + list(args), stdout=subprocess.PIPE,
                             text=True, env=self.env)
        self.procs.append(p)
        return p

    def close(self):
        for p in self.procs:
            if p.poll() is None:
                p.kill()
            try:
                p.communicate(timeout=30)
            except (subprocess.TimeoutExpired, ValueError):
                p.wait(timeout=30)


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


def answer(p, timeout=120):
    out, _ = p.communicate(timeout=timeout)
    return out.strip()


def stop(miner, timeout=60):
    """SIGTERM -> the miner's --stats object; it must exit 0."""
    miner.send_signal(signal.SIGTERM)
    out, err = miner.communicate(timeout=timeout)
    assert miner.returncode == 0, (miner.returncode, out, err)
    return json.loads([x for x in out.splitlines() if x.startswith("{")][-1])


def read_log(path):
    """[(round, [(conn, lower, upper), ...]), ...]; at most one piece per
    connection in a round."""
    rounds = []
    with open(path) as f:
        for line in f:
            parts = line.split()
            pieces = [tuple(int(x) for x in p.split(":")) for p in parts[1:]]
            conns = [c for c, _, _ in pieces]
            assert pieces and len(conns) == len(set(conns)), line
            rounds.append((int(parts[0]), pieces))
    return rounds


def test_every_route_in_one_pool(system, oracle_mod, tmp_path):
    """12 concurrent clients on 8 connections; the server does not split, so a
    client's job is one miner job and (default --chunk 2^36) one piece.  One
    size per route or edge of p1hip_scan_batch_wide: small (<= 2^16 nonces),
    wide (<= 2^24), individual."""
    log = tmp_path / "rounds.txt"
    s = system(["--chunk", str(1 << 40)])
    miner = s.miner(["--conns", "8", "--wide", "--linger-us", "50000", "--round-log", str(log), "--stats"])
    jobs = [("bradfitz", 9999),                      # small; the handout's known answer
            ("edge-a", 65535), ("edge-b", 65536),    # 2^16 nonces: small; 2^16 + 1: wide
            ("w1", 10**5), ("w2", 3 * 10**5), ("w3", 10**6),
            ("edge-c", (1 << 24) - 1), ("edge-d", 1 << 24),  # 2^24 nonces: wide; 2^24 + 1: individual
            ("big", 2 * 10**7),                      # individual
            ("two-block-tail-" + "y" * 55, 10**5),   # 70 bytes: the tail spans two SHA-256 blocks
            ("r1", 10**5), ("r2", 10**5)]
    assert len(jobs) == 12 and len({m for m, _ in jobs}) == 12 and any(len(m) >= 64 for m, _ in jobs)
    procs = [s.start_client(m, mx) for m, mx in jobs]
    got = [answer(p) for p in procs]
    assert got[0] == "Result 1419516646206828 9898"
    for (m, mx), g in zip(jobs, got):
        h, n = oracle_mod.scan(m, 0, mx, threads=8)
        assert g == f"Result {h} {n}", (m, mx)
    st = stop(miner)
    print(f"pool stats: {st}")
    assert st["conns_open"] == 8 and st["lost_conns"] == 0, st
    assert st["requests"] == 12 and st["pieces"] == 12, st
    assert st["max_round"] >= 2, st
    assert st["wide"]["calls"] >= 1 and st["wide"]["wide"] >= 1, st
    assert st["wide"]["small"] + st["batch"]["coalesced"] >= 1, st
    rounds = read_log(log)
    assert sum(len(p) for _, p in rounds) == 12 and max(len(p) for _, p in rounds) == st["max_round"]


def test_long_job_does_not_starve_a_short_one(system, oracle_mod, gpu, tmp_path):
    """A: [0, 2^34) in 64 pieces of 2^28; B, 100 ms later on the other
    connection: configs[0]'s request.  B rides in one of A's rounds.  No
    wall-clock assertion."""
    log = tmp_path / "rounds.txt"
    chunk, hi = 1 << 28, (1 << 34) - 1
    s = system(["--chunk", str(1 << 40)])
    miner = s.miner(["--conns", "2", "--wide", "--chunk", str(chunk), "--round-log", str(log), "--stats"])
    # a one-nonce job first: once it is answered the miner has opened the GPU
    # and joined, so A is under way when B arrives
    warm = s.start_client("warm", 0)
    h0, n0 = oracle_mod.scan("warm", 0, 0)
    assert answer(warm) == f"Result {h0} {n0}"
    a = s.start_client("bradfitz", hi)
    time.sleep(0.1)
    b = s.start_client("bradfitz", 9999)
    assert answer(b) == "Result 1419516646206828 9898"
    word, h, n = answer(a).split()
    h, n = int(h), int(n)
    assert word == "Result" and oracle_mod.hash("bradfitz", n) == h
    assert (h, n) == gpu.scan("bradfitz", 0, hi)
    st = stop(miner)
    print(f"pool stats: {st}")
    rounds = read_log(log)
    b_at = [r for r, p in rounds for c, lo, up in p if (lo, up) == (0, 9999)]
    assert len(b_at) == 1, b_at
    a_pieces = [(r, lo, up) for r, p in rounds for c, lo, up in p if up - lo == chunk - 1]
    assert [(lo, up) for _, lo, up in a_pieces] == [(k * chunk, (k + 1) * chunk - 1) for k in range(64)]
    assert b_at[0] < a_pieces[-1][0], (b_at, a_pieces[-1])
    print(f"B's piece in round {b_at[0]}; A's pieces in rounds {a_pieces[0][0]}..{a_pieces[-1][0]}")
    assert st["requests"] == 3 and st["pieces"] == 66, st


def test_write_drop_with_a_gpu_pool(system, oracle_mod):
    """5% of every write lost in every process, window 8, 200 ms epochs: four
    concurrent clients of 10^6 nonces, cut by the server into 32 jobs for the
    8 connections of one miner."""
    env = {"P1LSP_WRITE_DROP": "5"}
    prm = ["--window", "8", "--epoch-millis", "200"]
    s = system(["--chunk", "125000"] + prm, env=env)
    miner = s.miner(["--conns", "8", "--wide", "--stats"] + prm)
    jobs = [(f"drop-{i}", 10**6 - 1) for i in range(4)]
    procs = [s.start_client(m, mx, args=prm) for m, mx in jobs]
    for (m, mx), p in zip(jobs, procs):
        h, n = oracle_mod.scan(m, 0, mx, threads=8)
        assert answer(p) == f"Result {h} {n}", m
    st = stop(miner)
    print(f"pool stats: {st}")
    assert st["requests"] >= 32, st
