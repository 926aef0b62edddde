"""p1hip_scan_below on one device: what the filter costs, where the two routes
cross, and how long the first hit takes.

(a) filter overhead: scan_below with a target below the range's minimum over
    `bradfitz [0, 2^36)` (every slice sparse, no candidate, nothing found)
    against p1hip_scan of the same range, alternated, best of REPS after a
    warm-up.  ratio = below / scan.
(b) the switch: targets 2^44, 2^46 and 2^48 over [0, 2^30) with a cap no call
    reaches, once through each route.  The routes are forced by the test knob
    P1HIP_BELOW_PATH, so these rows come from a separate helper process
    (`below_bench.py --forced`) that runs with P1HIP_TEST_KNOBS=1 and are
    labelled "forced"; the library's own choice is timed in this process.
(c) first hit: cap = 1 at targets 2^56, 2^48, 2^40 and 2^32 over [0, 2^40]:
    wall time, nonces examined, slices.

Refuses to run with P1HIP_TEST_KNOBS set (only the helper it starts itself
has it).  Prints one JSON line and writes it to OUT.

env: REPS (5), DEVICE (0), OUT (profiles/below_bench.json)."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MSG = b"bradfitz"
SWITCH_TARGETS = [44, 46, 48]
SWITCH_RANGE = (0, (1 << 30) - 1)
SWITCH_CAP = 1 << 20


def best_of(reps, fns, worst=None):
    """fns: {name: callable}; alternated, best wall seconds of each (`worst`,
    a dict, receives the slowest repetition of each: the run-to-run spread)."""
    best = {k: float("inf") for k in fns}
    for fn in fns.values():  # warm-up: buffers, tables, clocks
        fn()
    for _ in range(reps):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            best[k] = min(best[k], dt)
            if worst is not None:
                worst[k] = max(worst.get(k, 0.0), dt)
    return best


def forced_helper():
    """The child: both forced routes at every switch target (knobs on)."""
    import p1_amd

    reps = int(os.environ.get("REPS", "5"))
    p1_amd.init_devices([int(os.environ.get("DEVICE", "0"))])
    lo, hi = SWITCH_RANGE
    rows = []
    for e in SWITCH_TARGETS:
        target = 1 << e
        got = {}

        def run(path):
            def go():
                os.environ["P1HIP_BELOW_PATH"] = path
                got[path] = p1_amd.scan_below(MSG, lo, hi, target, cap=SWITCH_CAP)
            return go

        best = best_of(reps, {"sparse": run("1"), "dense": run("2")})
        assert got["1"] == got["2"] and len(got["1"]) < SWITCH_CAP
        rows.append({"target_log2": e, "hits": len(got["1"]), "forced_sparse_ms": round(best["sparse"] * 1e3, 3),
                     "forced_dense_ms": round(best["dense"] * 1e3, 3),
                     "faster": "sparse" if best["sparse"] < best["dense"] else "dense"})
    print(json.dumps({"knobs": p1_amd.test_knobs(), "rows": rows}), flush=True)


def main():
    if os.environ.get("P1HIP_TEST_KNOBS"):
        raise SystemExit("below_bench: P1HIP_TEST_KNOBS is set; the timed process runs without test knobs")
    reps = int(os.environ.get("REPS", "5"))
    out = os.environ.get("OUT", os.path.join(ROOT, "profiles", "below_bench.json"))
    env = dict(os.environ, P1HIP_TEST_KNOBS="1")
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--forced"], env=env, capture_output=True,
                           text=True, timeout=900)
    if child.returncode != 0:
        raise SystemExit(f"below_bench: forced helper failed: {child.stderr[-2000:]}")
    forced = json.loads(child.stdout.strip().splitlines()[-1])

    import p1_amd

    p1_amd.init_devices([int(os.environ.get("DEVICE", "0"))])
    if p1_amd.test_knobs():
        raise SystemExit(f"below_bench: test knobs in force: {p1_amd.test_knobs()}")

    # (a) filter overhead
    lo, hi = 0, (1 << 36) - 1
    low = p1_amd.scan(MSG, lo, hi)
    assert p1_amd.scan_below(MSG, lo, hi, low[0] - 1, cap=1) == [] and p1_amd.scan_below(MSG, lo, hi, low[0]) == [low]
    p1_amd.reset_stats()
    worst = {}
    best = best_of(reps, {"scan": lambda: p1_amd.scan(MSG, lo, hi),
                          "below": lambda: p1_amd.scan_below(MSG, lo, hi, low[0] - 1, cap=1)}, worst)
    s = p1_amd.get_below_stats()
    filt = {"range": "bradfitz [0, 2^36)", "scan_ms": round(best["scan"] * 1e3, 3),
            "below_ms": round(best["below"] * 1e3, 3), "ratio": round(best["below"] / best["scan"], 4),
            "scan_worst_ms": round(worst["scan"] * 1e3, 3), "below_worst_ms": round(worst["below"] * 1e3, 3),
            "slices_per_call": s["slices"] // s["calls"], "candidate_tiles": s["candidate_tiles"]}

    # (b) the switch: the library's own choice next to the forced rows
    lo, hi = SWITCH_RANGE
    switch = []
    for row in forced["rows"]:
        target = 1 << row["target_log2"]
        p1_amd.reset_stats()
        t = best_of(reps, {"auto": lambda: p1_amd.scan_below(MSG, lo, hi, target, cap=SWITCH_CAP)})
        s = p1_amd.get_below_stats()
        switch.append(dict(row, auto_ms=round(t["auto"] * 1e3, 3),
                           auto_route="dense" if s["dense_slices"] else "sparse"))

    # (c) first hit
    first = []
    for e in (56, 48, 40, 32):
        p1_amd.reset_stats()
        got = []
        t = best_of(reps, {"first": lambda: got.append(p1_amd.scan_below(MSG, 0, 1 << 40, 1 << e, cap=1))})
        s = p1_amd.get_below_stats()
        first.append({"target_log2": e, "hit": got[-1], "wall_ms": round(t["first"] * 1e3, 3),
                      "examined": s["examined"] // s["calls"], "slices": s["slices"] // s["calls"],
                      "route": "dense" if s["dense_slices"] else "sparse"})

    doc = {"what": f"p1hip_scan_below on one MI355X, best of {reps} after a warm-up, wall ms timed from Python in one "
                   f"process, sides alternated; the forced_* figures come from a helper process with "
                   f"P1HIP_TEST_KNOBS=1 (P1HIP_BELOW_PATH)",
           "version": p1_amd.version(), "codeobj_sha256": p1_amd.codeobj_sha256(),
           "batch_codeobj_sha256": p1_amd.batch_codeobj_sha256(),
           "below_codeobj_sha256": p1_amd.below_codeobj_sha256(),
           "dense_target_log2": p1_amd.BELOW_DENSE_TARGET.bit_length() - 1,
           "filter_overhead": filt, "switch": switch, "forced_helper_knobs": forced["knobs"], "first_hit": first}
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc), flush=True)


if __name__ == "__main__":
    forced_helper() if "--forced" in sys.argv[1:] else main()
