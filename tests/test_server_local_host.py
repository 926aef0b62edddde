"""A server that scans itself, without a GPU.

`tools/lsp_fake_server_local` is the very loop and local slots that
`p1gpuserver` runs (p1_amd/host/server_lsp.hpp, local_slots.hpp: the round
thread, the collector thread, the shutdown) over a backend that answers with
the CPU oracle on a worker thread -- like the GPU, it works while the server
goes on.  Real clients talk to it over LSP on loopback: `p1client`, and
`tools/lsp_jobs` (one connection, several Requests with any Lower / Upper).

The stats line is the JSON object the server prints on stderr at exit with
--stats.  Also here: `p1server`, which shares the loop, is unchanged.

Reference: server.go:83-168 (every Result is what one miner scanning the whole
range returns, miner.go:56-63)."""
import json
import os
import signal
import subprocess
import time

import pytest

from conftest import ROOT, host_bin

SERVER = host_bin(os.path.join(ROOT, "tools", "lsp_fake_server_local"))
CLIENT = host_bin(os.path.join(ROOT, "p1_amd", "p1client"))
JOBS = host_bin(os.path.join(ROOT, "tools", "lsp_jobs"))
FAKE_MINER = host_bin(os.path.join(ROOT, "tools", "lsp_fake_miner"))
P1SERVER = os.path.join(ROOT, "p1_amd", "p1server")
P1CLIENT = os.path.join(ROOT, "p1_amd", "p1client")
GPUSERVER = os.path.join(ROOT, "p1_amd", "p1gpuserver")

# every block boundary of the message + nonce tail (SHA-256 blocks of 64 bytes)
MSG_LENS = [0, 8, 54, 55, 63, 119, 120]


@pytest.fixture(scope="module", autouse=True)
def built():
    for t in (SERVER, JOBS, FAKE_MINER, GPUSERVER):
        if not os.path.exists(t):
            subprocess.run(["make", "-s", "-C", ROOT, os.path.relpath(t, ROOT)], check=True)


class System:
    """One self-scanning server + clients (+ remote fake miners); every
    process is ours and is killed by PID."""

    def __init__(self, args=(), env=None):
        self.env = dict(os.environ, **(env or {}))
        self.procs = []
        self.server = subprocess.Popen([SERVER] + list(args) + ["--stats", "lsp", "0"], stdout=subprocess.PIPE,
                                       stderr=subprocess.PIPE, text=True, env=self.env)
        self.procs.append(self.server)
        line = self.server.stdout.readline()  # server.go:79
        assert line.startswith("Server listening on port"), line
        self.hostport = f"127.0.0.1:{int(line.split()[-1])}"

    def _start(self, argv, env=None, **kw):
        p = subprocess.Popen(argv, stdout=subprocess.PIPE, text=True, env=dict(self.env, **(env or {})), **kw)
        self.procs.append(p)
        return p

    def client(self, msg, max_nonce, args=(), env=None):
        return self._start([CLIENT, self.hostport, msg, str(max_nonce)] + list(args), env)

    def jobs(self, jobs, args=(), env=None):
        """One connection, the jobs [(msg, lower, upper), ...] one after another."""
        flat = [str(x) for j in jobs for x in j]
        return self._start([JOBS, self.hostport] + list(args) + ["--"] + flat, env)

    def miner(self, args=(), env=None):
        return self._start([FAKE_MINER, self.hostport] + list(args), env)

    def stop(self, timeout=30):
        """SIGTERM -> (exit status, stats, stderr)."""
        self.server.send_signal(signal.SIGTERM)
        return self.wait(timeout)

    def wait(self, timeout=30):
        _, err = self.server.communicate(timeout=timeout)
        assert "ThreadSanitizer" not in err and "AddressSanitizer" not in err and "runtime error" not in err, err
        lines = [x for x in err.splitlines() if x.startswith("{")]
        return self.server.returncode, (json.loads(lines[-1]) if lines else None), err

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


def want(oracle_mod, jobs):
    return "\n".join("Result %d %d" % oracle_mod.scan(m, lo, hi, threads=4) for m, lo, hi in jobs)


def client_jobs(n_clients, n_jobs, top):
    """Per client its jobs: every message length of MSG_LENS, ranges that are
    empty (lower > upper), one nonce, below / exactly / just above one local
    chunk of 50000, and up to `top` nonces."""
    sizes = [None, 1, 49999, 50000, 50001, 100001, 150000, top, 12345, 9999, 77777]
    out = []
    for c in range(n_clients):
        js = []
        for j in range(n_jobs):
            k = c * n_jobs + j
            tag = f"{c}.{j}"
            msg = (tag + "x" * 200)[:MSG_LENS[k % len(MSG_LENS)]]  # length 0: the empty message, shared
            size = sizes[k % len(sizes)]
            lo = 1000 * k
            js.append((msg, lo + 5, lo) if size is None else (msg, lo, lo + size - 1))
        out.append(js)
    return out


def test_handout_answer(system):
    s = system()
    assert answer(s.client("bradfitz", 9999)) == "Result 1419516646206828 9898"
    rc, st, err = s.stop()
    assert rc == 0, err
    assert st["slots"] == 64 and st["inflight"] == 2 and st["local_chunk"] == 1 << 24, st
    assert st["rounds"] == 1 and st["pieces"] == 1 and st["failures"] == 0, st


@pytest.mark.parametrize("drop", [0, 10])
def test_concurrent_clients(system, oracle_mod, drop):
    """32 clients with 3 jobs each; with `drop`, 10% of every client's writes lost."""
    prm = ["--epoch-millis", "50", "--epoch-limit", "40", "--window", "4"]
    s = system(["--local-chunk", "50000"] + prm)
    jobs = client_jobs(32, 3, 200000)
    assert {len(m) for js in jobs for m, _, _ in js} == set(MSG_LENS)
    env = {"P1LSP_WRITE_DROP": str(drop)} if drop else None
    procs = [s.jobs(js, args=prm, env=env) for js in jobs]
    for js, p in zip(jobs, procs):
        assert answer(p, timeout=120) == want(oracle_mod, js), js
    rc, st, err = s.stop()
    assert rc == 0, err
    # ceil(size / 50000) pieces per job; empty ranges are answered by the scheduler
    pieces = sum(-(-(hi - lo + 1) // 50000) for js in jobs for _, lo, hi in js if lo <= hi)
    assert st["pieces"] == pieces and st["failures"] == 0 and st["max_outstanding"] <= 2, st
    assert 1 <= st["max_round"] <= 64, st


def test_linger_fills_a_round(system, oracle_mod):
    s = system(["--linger-us", "20000", "--inflight", "1"], env={"FAKE_ROUND_SLEEP_MS": "40"})
    jobs = client_jobs(12, 2, 60000)
    procs = [s.jobs(js) for js in jobs]
    for js, p in zip(jobs, procs):
        assert answer(p) == want(oracle_mod, js), js
    rc, st, err = s.stop()
    assert rc == 0, err
    assert st["max_round"] > 1 and st["max_outstanding"] == 1, st


def test_remote_miner_next_to_local_slots(system, oracle_mod, tmp_path):
    """4 local slots with chunks of 1000 nonces and one remote miner with the
    server's --chunk 3000: to the scheduler a slot is just another miner."""
    log = tmp_path / "miner.txt"
    s = system(["--slots", "4", "--local-chunk", "1000", "--chunk", "3000"], env={"FAKE_ROUND_SLEEP_MS": "3"})
    s.miner(env={"FAKE_LOG": str(log)})
    time.sleep(0.3)  # joined
    jobs = [[("bradfitz", 0, 99999)], [("msg", 5, 4), ("msg", 0, 60000)], [("x" * 70, 10**9, 10**9 + 45678)]]
    procs = [s.jobs(js) for js in jobs]
    for js, p in zip(jobs, procs):
        assert answer(p) == want(oracle_mod, js), js
    rc, st, err = s.stop()
    assert rc == 0, err
    remote = [tuple(int(x) for x in line.split()) for line in open(log)]
    assert remote and all(hi - lo < 3000 for lo, hi in remote), remote[:5]
    assert any(hi - lo >= 1000 for lo, hi in remote), remote[:5]  # the remote miner's own, larger chunk
    assert st["pieces"] >= 1 and st["max_round"] <= 4, st


def test_client_killed_mid_request(system, oracle_mod):
    prm = ["--epoch-millis", "100", "--epoch-limit", "5"]
    s = system(["--slots", "3", "--local-chunk", "1000"] + prm, env={"FAKE_ROUND_SLEEP_MS": "20"})
    doomed = s.jobs([("doomed", 0, 10**6)], args=prm)  # 1000 pieces of 20 ms: never finishes here
    time.sleep(0.2)
    jobs = [[("a", 0, 4999), ("b", 7, 7)], [("bradfitz", 0, 9999)]]
    procs = [s.jobs(js, args=prm) for js in jobs]
    time.sleep(0.1)
    doomed.kill()  # its piece is in a round that is out
    for js, p in zip(jobs, procs):
        assert answer(p) == want(oracle_mod, js), js
    time.sleep(1.0)  # 5 epochs of 100 ms: the server has dropped the request
    late = s.jobs([("late", 0, 2999)], args=prm)
    assert answer(late) == want(oracle_mod, [("late", 0, 2999)])
    rc, st, err = s.stop()
    assert rc == 0, err
    assert st["failures"] == 0 and st["pieces"] < 400, st  # the dropped request was not scanned on


def test_sigterm_with_rounds_outstanding(system, oracle_mod):
    """Two rounds are out when SIGTERM arrives: both are collected, their
    Results written and acknowledged, then the server exits 0."""
    s = system(["--inflight", "2"], env={"FAKE_ROUND_SLEEP_MS": "400"})
    a = s.jobs([("first", 0, 9999)])
    time.sleep(0.15)
    b = s.jobs([("second", 0, 4999)])
    time.sleep(0.15)
    rc, st, err = s.stop()
    assert rc == 0, err
    assert st["rounds"] == 2 and st["max_outstanding"] == 2 and st["pieces"] == 2, st
    assert answer(a) == want(oracle_mod, [("first", 0, 9999)])
    assert answer(b) == want(oracle_mod, [("second", 0, 4999)])


def test_exit_after(system, oracle_mod):
    s = system(["--exit-after", "3"], env={"FAKE_ROUND_SLEEP_MS": "20"})
    jobs = [("e1", 0, 999), ("e2", 3, 2), ("e3", 0, 1999)]
    p = s.jobs(jobs)
    assert answer(p) == want(oracle_mod, jobs)
    rc, st, err = s.wait()
    assert rc == 0 and st["pieces"] == 2, (rc, st, err)


def test_backend_failure_with_a_remote_miner(system, oracle_mod):
    s = system(["--slots", "4", "--local-chunk", "2000", "--fail-submit", "3"], env={"FAKE_ROUND_SLEEP_MS": "5"})
    s.miner()
    time.sleep(0.3)
    jobs = client_jobs(6, 2, 30000)
    procs = [s.jobs(js) for js in jobs]
    for js, p in zip(jobs, procs):
        assert answer(p) == want(oracle_mod, js), js
    rc, st, err = s.stop()
    assert rc == 0, err
    assert st["failures"] == 1 and st["rounds"] == 2, st
    assert err.count("the local backend failed") == 1 and "4 local slots lost" in err, err


def test_backend_failure_without_a_miner_waits_for_one(system, oracle_mod):
    s = system(["--fail-submit", "1"])
    jobs = [("stranded", 0, 9999), ("next", 0, 99)]
    p = s.jobs(jobs)
    time.sleep(0.5)
    assert p.poll() is None and s.server.poll() is None  # the request waits, the server is up
    s.miner()
    assert answer(p) == want(oracle_mod, jobs)
    rc, st, err = s.stop()
    assert rc == 0, err
    assert st["failures"] == 1 and st["rounds"] == 0 and st["pieces"] == 0, st


def test_flags_are_checked():
    for prog in (SERVER, GPUSERVER):  # p1gpuserver checks them before it opens the GPU
        for bad in (["--slots", "0"], ["--slots", "257"], ["--inflight", "0"], ["--inflight", "5"],
                    ["--local-chunk", "0"], ["--linger-us", "x"], ["--miners", "2"]):
            r = subprocess.run([prog] + bad + ["lsp", "0"], capture_output=True, text=True, timeout=30)
            assert r.returncode == 2 and "usage" in r.stderr and "--slots S" in r.stderr, (prog, bad, r.stderr)
    for args in (["lsp"], ["lsp", "x"], ["scan", "a", "0", "1"], []):
        r = subprocess.run([GPUSERVER] + args, capture_output=True, text=True, timeout=30)
        assert r.returncode == 2 and r.stderr.startswith("usage: p1gpuserver"), (args, r.stderr)


P1SERVER_USAGE = (
    "usage: p1server [--chunk C] [--epoch-limit K] [--epoch-millis M] [--window W] [--copies K] [--exit-after N] "
    "lsp <port>\n"
    "       p1server [--chunk C] [--miners N] [--devices d0,d1,..] [--miner-cmd CMD] "
    "scan <msg> <lower> <upper> | serve\n")


def needed(path):
    out = subprocess.run(["ldd", path], capture_output=True, text=True, timeout=30, check=True).stdout
    return sorted(line.split()[0] for line in out.splitlines() if line.strip())


def test_p1server_is_unchanged():
    """The loop moved to server_lsp.hpp; the program's text and what it links did not change."""
    r = subprocess.run([P1SERVER, "--help"], capture_output=True, text=True, timeout=30)
    assert r.returncode == 2 and r.stderr == P1SERVER_USAGE and r.stdout == "", (r.stdout, r.stderr)
    r = subprocess.run([P1SERVER, "--slots", "4", "lsp", "0"], capture_output=True, text=True, timeout=30)
    assert r.returncode == 2 and r.stderr == P1SERVER_USAGE and r.stdout == "", (r.stdout, r.stderr)
    libs = needed(P1SERVER)
    assert libs == needed(P1CLIENT), libs  # the client's: the C++ runtime and libc, nothing else
    assert not [x for x in libs if "p1hip" in x or "p1oracle" in x or "amdhip" in x or "rocm" in x or "rccl" in x], libs
    assert [x for x in needed(GPUSERVER) if "libp1hip" in x]


def test_p1server_exit_after_still_answers(oracle_mod):
    """`p1server lsp --exit-after` through the shared loop: one fake miner, two requests."""
    srv = subprocess.Popen([host_bin(P1SERVER), "--chunk", "3000", "--exit-after", "2", "lsp", "0"],
                           stdout=subprocess.PIPE, text=True)
    procs = [srv]
    try:
        hp = f"127.0.0.1:{int(srv.stdout.readline().split()[-1])}"
        procs.append(subprocess.Popen([FAKE_MINER, hp]))
        jobs = [("bradfitz", 0, 9999), ("none", 9, 3)]
        p = subprocess.Popen([JOBS, hp, "--"] + [str(x) for j in jobs for x in j], stdout=subprocess.PIPE, text=True)
        procs.append(p)
        assert answer(p) == want(oracle_mod, jobs)
        assert srv.wait(timeout=30) == 0
    finally:
        for q in procs:
            if q.poll() is None:
                q.kill()
            q.wait(timeout=30)
