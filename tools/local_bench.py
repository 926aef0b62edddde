"""Many clients' jobs over LSP on one GPU: miners behind `p1server lsp` against
a server that scans itself (`p1gpuserver`, p1_amd/host/local_slots.hpp).
tools/pool_bench.py's workload: for every job size CLIENTS x JOBS requests
[0, size) from tools/lsp_load (all clients in one process, each sending its
next Request after the Result of the one before; every client's first job
warms the path and is not timed), answered by
  a  8 x `p1miner lsp` behind `p1server lsp`        (the yardstick: the path this feature leaves alone)
  c  1 x `p1miner lsp --conns 64 --wide --inflight 2` behind `p1server lsp`
  d  `p1gpuserver --slots 64 --inflight 2`           (no miner process at all)
all in one session on one box, one arrangement at a time, so at most 9
processes have the GPU open (8 miners and this tool's none; d: one).  Every
process that opens the GPU runs under its own `timeout -k 10 CELL_TIMEOUT`,
and the first cell that fails ends the run with a non-zero status.  The
checksum (xor of all hashes and nonces) must agree across a, c and d in every
row, or the tool exits 3.  Writes profiles/local_bench.json and prints it as
one JSON line.

env: SIZES (10000,100000,1000000,10000000), CLIENTS (64), JOBS (20),
     DEVICE (0), OUT (profiles/local_bench.json), CELL_TIMEOUT (120);
     FAKE=1 runs the CPU oracle-backed doubles (tools/lsp_fake_miner,
     tools/lsp_fake_pool_async, tools/lsp_fake_server_local: plumbing only)."""
import json
import os
import signal
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SERVER = os.path.join(ROOT, "p1_amd", "p1server")
GPUSERVER = os.path.join(ROOT, "p1_amd", "p1gpuserver")
MINER = os.path.join(ROOT, "p1_amd", "p1miner")
LOAD = os.path.join(ROOT, "tools", "lsp_load")
FAKE_MINER = os.path.join(ROOT, "tools", "lsp_fake_miner")
FAKE_POOL_ASYNC = os.path.join(ROOT, "tools", "lsp_fake_pool_async")
FAKE_SERVER_LOCAL = os.path.join(ROOT, "tools", "lsp_fake_server_local")

CELL_TIMEOUT = float(os.environ.get("CELL_TIMEOUT", "120"))
SETUPS = [("a", "8 x p1miner lsp, p1server lsp"),
          ("c", "p1miner lsp --conns 64 --wide --inflight 2, p1server lsp"),
          ("d", "p1gpuserver --slots 64 --inflight 2")]


def limited(argv):
    """A process that opens the GPU: under a time limit of its own.  `timeout`
    passes our SIGTERM on to it."""
    return ["timeout", "-k", "10", str(int(CELL_TIMEOUT) + 30)] + argv


def start(argv, **kw):
    """Every process leads a process group of its own, so that end() reaches
    the program behind `timeout` too (a SIGKILL to `timeout` alone would leave
    it running, with the GPU open, into the next cells)."""
    return subprocess.Popen(argv, text=True, start_new_session=True, **kw)


def end(p):
    try:
        os.killpg(p.pid, signal.SIGKILL)
    except ProcessLookupError:
        pass
    p.wait()


def stats_of(text):
    lines = [x for x in text.splitlines() if x.startswith("{")]
    return json.loads(lines[-1]) if lines else None


def cell(key, size, clients, jobs, fake, device):
    procs = []
    errlog = tempfile.TemporaryFile(mode="w+")
    try:
        if key == "d":
            argv = limited([FAKE_SERVER_LOCAL] if fake else [GPUSERVER, "--device", device]) + \
                   ["--slots", "64", "--inflight", "2", "--stats", "lsp", "0"]
            srv = start(argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        else:
            srv = start([SERVER, "lsp", "0"], stdout=subprocess.PIPE)
        procs.append(srv)
        line = srv.stdout.readline()  # p1gpuserver: printed once the GPU is open
        if not line.startswith("Server listening on port"):
            raise SystemExit(f"local_bench: server said {line!r}")
        hp = f"127.0.0.1:{int(line.split()[-1])}"
        miners = []
        if key == "a":
            for _ in range(8):
                argv = limited([FAKE_MINER, hp] if fake else [MINER, "lsp", hp, "--device", device])
                miners.append(start(argv, stdout=subprocess.PIPE, stderr=errlog))
        elif key == "c":
            argv = limited([FAKE_POOL_ASYNC, hp] if fake else [MINER, "lsp", hp, "--device", device, "--wide"]) + \
                   ["--conns", "64", "--inflight", "2", "--stats"]
            miners.append(start(argv, stdout=subprocess.PIPE, stderr=errlog))
        procs += miners
        if miners:
            time.sleep(0.5 if fake else 3.0)  # device open, code objects loaded, joined
        dead = [p.args for p in miners if p.poll() is not None]
        if dead:
            errlog.seek(0)
            raise SystemExit(f"local_bench: miner exited at start: {dead[0]}: {errlog.read()[-2000:]!r}")
        try:
            r = subprocess.run([LOAD, hp, str(clients), str(jobs), "job", str(size - 1), "--warm", "1"],
                               capture_output=True, text=True, timeout=CELL_TIMEOUT)
        except subprocess.TimeoutExpired:
            errlog.seek(0)
            raise SystemExit(f"local_bench: {key}, {size} nonces: lsp_load did not finish; stderr: "
                             f"{errlog.read()[-2000:]!r}")
        if r.returncode != 0:
            raise SystemExit(f"local_bench: lsp_load rc={r.returncode} out={r.stdout!r} err={r.stderr[-500:]!r}")
        timed = json.loads(r.stdout)
        dead = [p.args for p in miners + [srv] if p.poll() is not None]
        if dead:
            errlog.seek(0)
            raise SystemExit(f"local_bench: a process exited: {dead[0]}: {errlog.read()[-2000:]!r}")
        stats = None
        if key == "c":
            miners[0].send_signal(signal.SIGTERM)
            out, _ = miners[0].communicate(timeout=60)
            stats = stats_of(out)
        elif key == "d":
            srv.send_signal(signal.SIGTERM)
            _, err = srv.communicate(timeout=60)
            if srv.returncode != 0:
                raise SystemExit(f"local_bench: the server exited {srv.returncode}: {err[-2000:]!r}")
            stats = stats_of(err)
        n = timed["jobs"]
        res = {"wall_s": timed["wall_s"], "jobs": n, "jobs_per_s": n / timed["wall_s"],
               "GH_s": n * size / timed["wall_s"] / 1e9, "checksum": timed["checksum"], "stats": stats}
        if stats and stats.get("rounds"):
            res["pieces_per_round"] = stats["pieces"] / stats["rounds"]
        return res
    finally:
        for p in procs:
            end(p)
        errlog.close()


def main():
    sizes = [int(x) for x in os.environ.get("SIZES", "10000,100000,1000000,10000000").split(",")]
    clients = int(os.environ.get("CLIENTS", "64"))
    jobs = int(os.environ.get("JOBS", "20"))
    fake = os.environ.get("FAKE") == "1"
    device = os.environ.get("DEVICE", "0")
    out = os.environ.get("OUT", os.path.join(ROOT, "profiles", "local_bench.json"))
    rows, ok = [], True
    for size in sizes:
        row = {"nonces_per_job": size, "clients": clients, "jobs_per_client": jobs}
        for key, what in SETUPS:
            row[key] = dict(cell(key, size, clients, jobs, fake, device), setup=what)
            print(f"local_bench: {size} nonces, {what}: {row[key]['jobs_per_s']:.0f} jobs/s, "
                  f"{row[key]['GH_s']:.2f} GH/s", file=sys.stderr, flush=True)
        row["checksums_agree"] = row["a"]["checksum"] == row["c"]["checksum"] == row["d"]["checksum"]
        row["c_over_a"] = row["c"]["jobs_per_s"] / row["a"]["jobs_per_s"]
        row["d_over_a"] = row["d"]["jobs_per_s"] / row["a"]["jobs_per_s"]
        row["d_over_c"] = row["d"]["jobs_per_s"] / row["c"]["jobs_per_s"]
        ok = ok and row["checksums_agree"]
        rows.append(row)
    doc = {"workload": f"{clients} LSP clients x {jobs} jobs [0, size) each, messages job<client>-<job>, on loopback; "
                       f"{'CPU oracle doubles (plumbing only)' if fake else 'one MI355X, device ' + device}",
           "fake": fake, "rows": rows}
    if not fake:
        sys.path.insert(0, ROOT)
        import p1_amd  # reads the embedded code objects; opens no device

        doc["codeobj_sha256"] = p1_amd.codeobj_sha256()
        doc["batch_codeobj_sha256"] = p1_amd.batch_codeobj_sha256()
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc), flush=True)
    if not ok:
        sys.exit(3)


if __name__ == "__main__":
    main()
