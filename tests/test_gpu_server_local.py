"""The server that scans on its own GPU: one `p1gpuserver --device 0` process
with real clients over LSP on loopback (`p1client`; `tools/lsp_jobs`: one
connection, several Requests with any Lower / Upper).  No new device code runs
here: every round is one p1hip_batch_submit(..., wide = 1) / p1hip_batch_wait
pair (miner::SubmitPieces / CollectPieces) over k_batch_scan, k_batch_reduce,
the shared k_scan launches and k_wide_reduce, cut by server::LocalSlots from
the scheduler's chunks.  Every Result must be what one scan of the whole range
returns.

At most two processes have the GPU open (the server and this one), three in
the mixed test (a `p1miner lsp` next to the local slots).  Every subprocess
has a timeout and is killed in the fixture's teardown; nothing is retried."""
import json
import os
import signal
import subprocess
import time

import pytest

from conftest import ROOT, host_bin

GPUSERVER = host_bin(os.path.join(ROOT, "p1_amd", "p1gpuserver"))
CLIENT = host_bin(os.path.join(ROOT, "p1_amd", "p1client"))
MINER = host_bin(os.path.join(ROOT, "p1_amd", "p1miner"))
JOBS = host_bin(os.path.join(ROOT, "tools", "lsp_jobs"))

pytestmark = pytest.mark.gpu

# the code objects of the commit this feature was built on: it adds no device code
SCAN_CODEOBJ = "da205152f146ea639f2cb01d4e2dcb4fae1b0325fc87a52e875623d86b11db41"
BATCH_CODEOBJ = "b79543a94ef1c35ca696d644d9aea4595ca7862ae9ece505fc64376007ebc8af"


class System:
    """One p1gpuserver + clients; every process is ours and is killed by PID.
    The children do not inherit the library's test knobs that the `gpu`
    fixture sets for this process: the server runs as in production."""

    def __init__(self, args=()):
        self.env = {k: v for k, v in os.environ.items() if not k.startswith("P1HIP_")}
        self.procs = []
        self.server = subprocess.Popen([GPUSERVER, "--device", "0", "--stats"] + list(args) + ["lsp", "0"],
                                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=self.env)
        self.procs.append(self.server)
        line = self.server.stdout.readline()  # printed once the GPU is open
        assert line.startswith("Server listening on port"), (line, self.server.stderr.read())
        self.hostport = f"127.0.0.1:{int(line.split()[-1])}"

    def _start(self, argv):
        p = subprocess.Popen(argv, stdout=subprocess.PIPE, text=True, env=self.env)
        self.procs.append(p)
        return p

    def client(self, msg, max_nonce):
        return self._start([CLIENT, self.hostport, msg, str(max_nonce)])

    def jobs(self, jobs):
        return self._start([JOBS, self.hostport, "--"] + [str(x) for j in jobs for x in j])

    def miner(self):
        return self._start([MINER, "lsp", self.hostport, "--device", "0"])

    def stop(self, timeout=60):
        """SIGTERM -> the --stats object; the server must exit 0."""
        self.server.send_signal(signal.SIGTERM)
        _, err = self.server.communicate(timeout=timeout)
        assert self.server.returncode == 0, (self.server.returncode, err)
        return json.loads([x for x in err.splitlines() if x.startswith("{")][-1])

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


def test_code_objects_are_the_parents(gpu):
    assert gpu.codeobj_sha256() == SCAN_CODEOBJ
    assert gpu.batch_codeobj_sha256() == BATCH_CODEOBJ


def test_handout_answer(system):
    s = system()
    assert answer(s.client("bradfitz", 9999)) == "Result 1419516646206828 9898"
    st = s.stop()
    assert st["rounds"] == 1 and st["pieces"] == 1 and st["failures"] == 0, st
    assert st["async"]["submits"] == 1 and st["wide"]["calls"] == 1 and st["wide"]["small"] == 1, st


def test_every_route_and_both_sides_of_each_limit(system, oracle_mod, gpu):
    """16 concurrent clients with 4 jobs each.  Sizes: empty (lower > upper),
    1, 9999, 2^16 (the small route's most), 2^16 + 1 (wide), 10^5, 2^24 (the
    wide route's most and one whole --local-chunk), 2^24 + 1 (two pieces).
    Messages of 8, 54, 63 and 120 bytes: the nonce tail in the first block,
    across the block edge, and in a second and third block."""
    sizes = [None, 1, 9999, 1 << 16, (1 << 16) + 1, 10**5, 1 << 24, (1 << 24) + 1]
    lens = [8, 54, 63, 120]
    jobs = []
    for k in range(64):  # every size with every length, twice
        size, ln = sizes[k % 8], lens[(k // 8) % 4]
        msg = (f"job-{k:02d}-" + "z" * 120)[:ln]
        lo = 10**9 * (k % 5)
        jobs.append((msg, lo + 3, lo) if size is None else (msg, lo, lo + size - 1))
    per_client = [jobs[c::16] for c in range(16)]
    assert all(len(js) == 4 for js in per_client)
    want = {}
    for m, lo, hi in jobs:
        want[(m, lo, hi)] = oracle_mod.scan(m, lo, hi, threads=8) if hi < lo or hi - lo < 10**5 else gpu.scan(m, lo, hi)
    s = system(["--linger-us", "20000"])
    procs = [s.jobs(js) for js in per_client]
    for js, p in zip(per_client, procs):
        assert answer(p) == "\n".join("Result %d %d" % want[j] for j in js), js
    st = s.stop()
    print(f"server stats: {st}")
    assert st["slots"] == 64 and st["inflight"] == 2 and st["failures"] == 0, st
    assert st["pieces"] == 56 + 8, st  # 8 empty ranges yield no piece, 8 requests of 2^24 + 1 nonces two
    assert st["max_round"] >= 2, st
    assert st["max_outstanding"] <= 2 and st["async"]["max_inflight"] <= 2, st
    assert st["wide"]["calls"] == st["rounds"] == st["async"]["submits"] == st["async"]["waits"], st
    assert st["wide"]["requests"] == st["pieces"] and st["wide"]["individual"] == 0, st
    assert st["wide"]["small"] == 32 and st["wide"]["wide"] == 32, st


@pytest.mark.parametrize("args", [[], ["--slots", "1", "--inflight", "1"]], ids=["slots64", "slots1"])
def test_one_request_in_64_pieces(system, gpu, args):
    hi = (1 << 30) - 1
    s = system(args)
    got = answer(s.client("bradfitz", hi))
    assert got == "Result %d %d" % gpu.scan("bradfitz", 0, hi)
    st = s.stop()
    print(f"server stats: {st}")
    assert st["pieces"] == 64 and st["wide"]["wide"] == 64 and st["wide"]["individual"] == 0, st
    if args:
        assert st["rounds"] == 64 and st["max_round"] == 1 and st["max_outstanding"] == 1, st


def test_remote_gpu_miner_next_to_local_slots(system, gpu):
    """4 local slots and one real `p1miner lsp`, both with chunks of 2^24
    nonces, on one [0, 2^28) request: 16 chunks, whoever takes them."""
    hi = (1 << 28) - 1
    s = system(["--slots", "4", "--chunk", str(1 << 24)])
    s.miner()
    time.sleep(2.0)  # the miner opens the GPU, then joins; the answer is the same if it has not yet
    got = answer(s.client("bradfitz", hi))
    assert got == "Result %d %d" % gpu.scan("bradfitz", 0, hi)
    st = s.stop()
    print(f"server stats: {st} (the remote miner took {16 - st['pieces']} of 16 chunks)")
    assert 1 <= st["pieces"] <= 16 and st["max_round"] <= 4 and st["failures"] == 0, st
    assert len(s.procs) == 3  # server, miner, client: with this process at most 3 hold the GPU
