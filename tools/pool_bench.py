"""Many clients' jobs over LSP on one GPU: eight single-connection miner
processes against one multi-connection miner (`p1miner lsp --conns C --wide`,
p1_amd/host/miner_pool.hpp).  For every job size, `p1server lsp` (which does
not split jobs of these sizes) gets CLIENTS x JOBS requests from
tools/lsp_load (all clients in one process, each sending its next Request
after the Result of the one before), answered by
  a  8 x `p1miner lsp`                 one process per miner slot (configs[4]'s arrangement)
  b  1 x `p1miner lsp --conns 8 --wide`
  c  1 x `p1miner lsp --conns 64 --wide`
  d  1 x `p1miner lsp --conns 64 --wide --inflight N`   (only with --inflight N, N >= 2:
     up to N rounds outstanding through p1hip_batch_submit / p1hip_batch_wait)
Every client's first job warms the miners and is not timed (lsp_load --warm 1,
on the same connections: a second lsp_load process could be handed the UDP
port, and with it the server-side connection, of a client the first one just
closed); the rest is timed inside lsp_load from the first timed Request to the
last Result.  A cell that does not finish in CELL_TIMEOUT seconds ends the
run with the miners' stderr.  The checksum (xor of all hashes and nonces)
must agree across a, b and c.  Writes profiles/pool_bench.json and prints it
as one JSON line.

env: SIZES (10000,100000,1000000,10000000), CLIENTS (64), JOBS (20),
     DEVICE (0), OUT (profiles/pool_bench.json), CELL_TIMEOUT (120);
     FAKE=1 runs the CPU oracle-backed doubles (tools/lsp_fake_miner,
     tools/lsp_fake_pool: test plumbing only, no GPU).
args: --inflight N adds column d and the ratios d_over_a, d_over_c."""
import json
import os
import signal
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SERVER = os.path.join(ROOT, "p1_amd", "p1server")
MINER = os.path.join(ROOT, "p1_amd", "p1miner")
LOAD = os.path.join(ROOT, "tools", "lsp_load")
FAKE_MINER = os.path.join(ROOT, "tools", "lsp_fake_miner")
FAKE_POOL = os.path.join(ROOT, "tools", "lsp_fake_pool")
FAKE_POOL_ASYNC = os.path.join(ROOT, "tools", "lsp_fake_pool_async")

SETUPS = [("a", "8 x p1miner lsp", 8, 0, 1), ("b", "p1miner lsp --conns 8 --wide", 1, 8, 1),
          ("c", "p1miner lsp --conns 64 --wide", 1, 64, 1)]


def load(hp, clients, jobs, prefix, max_nonce, errlog):
    try:
        r = subprocess.run([LOAD, hp, str(clients), str(jobs), prefix, str(max_nonce), "--warm", "1"],
                           capture_output=True, text=True, timeout=float(os.environ.get("CELL_TIMEOUT", "120")))
    except subprocess.TimeoutExpired:
        errlog.seek(0)
        raise SystemExit(f"pool_bench: lsp_load did not finish; miners' stderr: {errlog.read()[-2000:]!r}")
    if r.returncode != 0:
        raise SystemExit(f"pool_bench: lsp_load rc={r.returncode} out={r.stdout!r} err={r.stderr[-500:]!r}")
    return json.loads(r.stdout)


def cell(size, nproc, conns, clients, jobs, fake, device, inflight=1):
    procs = []
    errlog = tempfile.TemporaryFile(mode="w+")
    try:
        srv = subprocess.Popen([SERVER, "lsp", "0"], stdout=subprocess.PIPE, text=True)
        procs.append(srv)
        line = srv.stdout.readline()
        if not line.startswith("Server listening on port"):
            raise SystemExit(f"pool_bench: server said {line!r}")
        hp = f"127.0.0.1:{int(line.split()[-1])}"
        miners = []
        for _ in range(nproc):
            if conns:
                argv = ([FAKE_POOL_ASYNC if inflight > 1 else FAKE_POOL, hp] if fake else
                        [MINER, "lsp", hp, "--device", device, "--wide"]) + ["--conns", str(conns), "--stats"]
                if inflight > 1:
                    argv += ["--inflight", str(inflight)]
            else:
                argv = [FAKE_MINER, hp] if fake else [MINER, "lsp", hp, "--device", device]
            miners.append(subprocess.Popen(argv, stdout=subprocess.PIPE, stderr=errlog, text=True))
        procs += miners
        time.sleep(0.5 if fake else 3.0)  # device open, code objects loaded, joined
        dead = [p.args for p in miners if p.poll() is not None]
        if dead:
            raise SystemExit(f"pool_bench: miner exited at start: {dead[0]}")
        timed = load(hp, clients, jobs, "job", size - 1, errlog)
        dead = [p.args for p in miners if p.poll() is not None]
        if dead:
            errlog.seek(0)
            raise SystemExit(f"pool_bench: miner exited: {dead[0]}: {errlog.read()[-2000:]!r}")
        stats = None
        if conns:
            miners[0].send_signal(signal.SIGTERM)
            out, _ = miners[0].communicate(timeout=60)
            lines = [x for x in out.splitlines() if x.startswith("{")]
            stats = json.loads(lines[-1]) if lines else None
        n = timed["jobs"]
        return {"wall_s": timed["wall_s"], "jobs": n, "jobs_per_s": n / timed["wall_s"],
                "GH_s": n * size / timed["wall_s"] / 1e9, "checksum": timed["checksum"], "miner_stats": stats}
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
            p.wait()
        errlog.close()


def main():
    sizes = [int(x) for x in os.environ.get("SIZES", "10000,100000,1000000,10000000").split(",")]
    clients = int(os.environ.get("CLIENTS", "64"))
    jobs = int(os.environ.get("JOBS", "20"))
    fake = os.environ.get("FAKE") == "1"
    device = os.environ.get("DEVICE", "0")
    out = os.environ.get("OUT", os.path.join(ROOT, "profiles", "pool_bench.json"))
    inflight = 1
    if "--inflight" in sys.argv[1:]:
        inflight = int(sys.argv[sys.argv.index("--inflight") + 1])
    setups = list(SETUPS)
    if inflight > 1:
        setups.append(("d", f"p1miner lsp --conns 64 --wide --inflight {inflight}", 1, 64, inflight))
    rows, ok = [], True
    for size in sizes:
        row = {"nonces_per_job": size, "clients": clients, "jobs_per_client": jobs}
        for key, what, nproc, conns, depth in setups:
            row[key] = dict(cell(size, nproc, conns, clients, jobs, fake, device, depth), setup=what)
            print(f"pool_bench: {size} nonces, {what}: {row[key]['jobs_per_s']:.0f} jobs/s, "
                  f"{row[key]['GH_s']:.2f} GH/s", file=sys.stderr, flush=True)
        row["checksums_agree"] = row["a"]["checksum"] == row["b"]["checksum"] == row["c"]["checksum"]
        row["b_over_a"] = row["b"]["jobs_per_s"] / row["a"]["jobs_per_s"]
        row["c_over_a"] = row["c"]["jobs_per_s"] / row["a"]["jobs_per_s"]
        if "d" in row:
            row["checksums_agree"] = row["checksums_agree"] and row["d"]["checksum"] == row["a"]["checksum"]
            row["d_over_a"] = row["d"]["jobs_per_s"] / row["a"]["jobs_per_s"]
            row["d_over_c"] = row["d"]["jobs_per_s"] / row["c"]["jobs_per_s"]
        ok = ok and row["checksums_agree"]
        rows.append(row)
    doc = {"workload": f"{clients} LSP clients x {jobs} jobs [0, size) each, messages job<client>-<job>, through "
                       f"p1server lsp on loopback; "
                       f"{'CPU oracle doubles (plumbing only)' if fake else 'one MI355X, device ' + device}",
           "fake": fake, "rows": rows}
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc), flush=True)
    if not ok:
        sys.exit(3)


if __name__ == "__main__":
    main()
