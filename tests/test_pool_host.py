"""The multi-connection miner's pool (p1_amd/host/miner_pool.hpp) on the CPU:
`tools/pool_test` checks miner::Rounds (jobs cut into rounds and folded back)
against direct scans; `tools/lsp_fake_pool` is the very miner::RunPool that
`p1miner lsp --conns C` runs, with the CPU oracle as its backend (a test
double), behind a real `p1server lsp` with real `p1client`s.

A round-log line is "<round> <conn>:<lower>:<upper> ..."; the stats line is
the JSON object the pool prints at exit with --stats."""
import json
import os
import signal
import subprocess
import time

import pytest

from conftest import ROOT, host_bin

SERVER = host_bin(os.path.join(ROOT, "p1_amd", "p1server"))
CLIENT = host_bin(os.path.join(ROOT, "p1_amd", "p1client"))
POOL = host_bin(os.path.join(ROOT, "tools", "lsp_fake_pool"))
POOL_TEST = host_bin(os.path.join(ROOT, "tools", "pool_test"))


class System:
    """One server + pools + clients; every process is ours and is killed by PID."""

    def __init__(self, args=(), env=None):
        self.env = dict(os.environ, **(env or {}))
        self.procs = []
        self.server = subprocess.Popen([SERVER] + list(args) + ["lsp", "0"], stdout=subprocess.PIPE, text=True,
                                       env=self.env)
        self.procs.append(self.server)
        line = self.server.stdout.readline()  # server.go:79
        assert line.startswith("Server listening on port"), line
        self.port = int(line.split()[-1])
        self.hostport = f"127.0.0.1:{self.port}"

    def pool(self, args, env=None):
        """A pool process; its stdout (the stats line) and stderr are kept."""
        p = subprocess.Popen([POOL, self.hostport] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                             text=True, env=dict(self.env, **(env or {})))
        self.procs.append(p)
        return p

    def start_client(self, msg, max_nonce, args=(), env=None):
        p = subprocess.Popen([CLIENT, self.hostport, msg, str(max_nonce)] + list(args), stdout=subprocess.PIPE,
                             text=True, env=dict(self.env, **(env or {})))
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


def answer(p, timeout=60):
    out, _ = p.communicate(timeout=timeout)
    return out.strip()


def want(oracle_mod, msg, mx):
    h, n = oracle_mod.scan(msg, 0, mx, threads=4)
    return f"Result {h} {n}"


def stop(pool, timeout=30):
    """SIGTERM -> (exit status, stats, stderr)."""
    pool.send_signal(signal.SIGTERM)
    out, err = pool.communicate(timeout=timeout)
    assert "ThreadSanitizer" not in err and "AddressSanitizer" not in err and "runtime error" not in err, err
    lines = [x for x in out.splitlines() if x.startswith("{")]
    return pool.returncode, (json.loads(lines[-1]) if lines else None), err


def read_log(path):
    """[(round, [(conn, lower, upper), ...]), ...]; every line holds at most
    one piece per connection and the rounds count up from 0."""
    rounds = []
    with open(path) as f:
        for line in f:
            parts = line.split()
            pieces = [tuple(int(x) for x in p.split(":")) for p in parts[1:]]
            assert pieces and int(parts[0]) == len(rounds), line
            conns = [c for c, _, _ in pieces]
            assert len(conns) == len(set(conns)), line
            rounds.append((int(parts[0]), pieces))
    return rounds


def test_rounds_unit():
    r = subprocess.run([POOL_TEST], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr


def test_concurrent_clients_share_rounds(system, oracle_mod, tmp_path):
    log = tmp_path / "rounds.txt"
    s = system(["--chunk", "500"])
    pool = s.pool(["--conns", "6", "--linger-us", "50000", "--round-log", str(log), "--stats"])
    jobs = [("a", 7000), ("bb", 3000), ("bradfitz", 9999), ("x" * 70, 5000)]
    procs = [s.start_client(m, mx) for m, mx in jobs]
    for (m, mx), p in zip(jobs, procs):
        assert answer(p) == want(oracle_mod, m, mx), m
    rc, st, err = stop(pool)
    assert rc == 0, err
    assert st["conns_wanted"] == 6 and st["conns_open"] == 6 and st["lost_conns"] == 0, st
    assert st["max_round"] >= 2, st
    rounds = read_log(log)
    assert len(rounds) == st["rounds"] and sum(len(p) for _, p in rounds) == st["pieces"], st
    assert max(len(p) for _, p in rounds) == st["max_round"], st
    # the server's chunks of at most 500 nonces, each one job of one piece here:
    # ceil(7001 / 500) + ceil(3001 / 500) + ceil(10000 / 500) + ceil(5001 / 500)
    assert st["requests"] == 15 + 7 + 20 + 11 and st["pieces"] == st["requests"], st
    assert all(0 <= c < 6 and up - lo < 500 for _, p in rounds for c, lo, up in p)


def test_short_job_is_not_starved_by_a_long_one(system, oracle_mod, tmp_path):
    log = tmp_path / "rounds.txt"
    s = system(["--chunk", str(1 << 40)])  # the server does not split
    pool = s.pool(["--conns", "2", "--chunk", "1000", "--round-log", str(log), "--stats"],
                  env={"FAKE_ROUND_SLEEP_MS": "20"})
    a = s.start_client("bradfitz", 49999)  # 50 pieces, 20 ms each
    time.sleep(0.2)
    b = s.start_client("bradfitz", 999)
    assert answer(b) == want(oracle_mod, "bradfitz", 999)
    assert answer(a) == want(oracle_mod, "bradfitz", 49999)
    rc, st, err = stop(pool)
    assert rc == 0, err
    rounds = read_log(log)
    a_rounds = [r for r, p in rounds for _, lo, up in p if up - lo == 999 and (lo, up) != (0, 999)]
    first = [(r, c) for r, p in rounds for c, lo, up in p if (lo, up) == (0, 999)]
    assert len(first) == 2 and first[0][1] != first[1][1], first  # A's first piece and B's only one
    a_conn = first[0][1]
    a_pieces = [(r, lo, up) for r, p in rounds for c, lo, up in p if c == a_conn]
    assert [(lo, up) for _, lo, up in a_pieces] == [(k * 1000, k * 1000 + 999) for k in range(50)]
    b_round = first[1][0]
    assert b_round < a_pieces[-1][0], (b_round, a_pieces[-1])
    assert len(a_rounds) == 49
    assert st["requests"] == 2 and st["pieces"] == 51 and st["max_round"] == 2, st


def test_write_drop_everywhere_small_epochs(system, oracle_mod):
    # 20% of every write lost in every process, window 4: one pool of 3 connections
    env = {"P1LSP_WRITE_DROP": "20"}
    prm = ["--epoch-millis", "50", "--epoch-limit", "20", "--window", "4"]
    s = system(["--chunk", "3000"] + prm, env=env)
    pool = s.pool(["--conns", "3", "--stats"] + prm)
    c = s.start_client("bradfitz", 49999, args=prm)
    assert answer(c, timeout=120) == want(oracle_mod, "bradfitz", 49999)
    rc, st, err = stop(pool, timeout=60)
    assert rc == 0, err
    assert 1 <= st["conns_open"] <= 3 and st["requests"] >= 17, st


def test_pool_ends_when_the_server_dies(system):
    prm = ["--epoch-millis", "100", "--epoch-limit", "5"]
    s = system(prm)
    pool = s.pool(["--conns", "3", "--stats"] + prm)
    time.sleep(0.5)  # joined and idle
    s.server.kill()
    s.server.wait(timeout=30)
    out, err = pool.communicate(timeout=10)  # every connection is lost after 5 epochs of 100 ms
    assert pool.returncode == 0, err
    st = json.loads([x for x in out.splitlines() if x.startswith("{")][-1])
    assert st["conns_open"] == 3 and st["lost_conns"] == st["conns_open"], st


def test_no_server_fails_to_join():
    r = subprocess.run([POOL, "127.0.0.1:9", "--conns", "2", "--epoch-millis", "50", "--epoch-limit", "3"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stdout.startswith("Failed to join with server"), r.stdout + r.stderr


def test_miner_flags_are_checked_before_the_gpu_is_opened():
    miner = os.path.join(ROOT, "p1_amd", "p1miner")
    for args in (["--conns", "0"], ["--conns", "257"], ["--conns", "x"], ["--conns"],
                 ["--wide"], ["--stats"], ["--linger-us", "5"], ["--round-log", "f"]):  # the last four need --conns
        r = subprocess.run([miner, "lsp", "127.0.0.1:9"] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "--conns C [--wide] [--linger-us U] [--round-log FILE] [--stats]" in r.stderr, args


def test_server_split_lands_on_one_pool(system, oracle_mod):
    # what four miner processes did in test_split_over_miners_matches_oracle, one process does
    s = system(["--chunk", "1777"])
    pool = s.pool(["--conns", "4", "--stats"])
    c = s.start_client("bradfitz", 99999)
    assert answer(c) == want(oracle_mod, "bradfitz", 99999)
    rc, st, err = stop(pool)
    assert rc == 0, err
    assert st["conns_open"] == 4 and st["requests"] >= 57, st  # ceil(100000 / 1777)
