"""p1hip_scan_below_batch on one device against the loop of p1hip_scan_below
over the same requests (the unchanged path).

Workloads:
  workers  N = 1, 16, 256, 4096 requests `worker <i>` [0, 2^32), cap = 1, at
           targets 2^56 and 2^48: the pool's question, each answer one slice
  shares   256 requests of 2^16 nonces at target 2^52 with cap = 65536: every
           share of the range
Both sides are called through ctypes with their arguments marshalled and their
result buffers allocated beforehand, so a figure is the time inside the
library call(s).  One process; best of REPS after a warm-up, the sides
alternated; the slowest repetition of each side is recorded as the spread.
The two sides' answers are compared before anything is timed.  Per row the
statistics of one batch call: rounds, launch pairs, nonces marked and the
bytes copied back (4 per hit slot and request, where the loop copies one bit
per nonce marked: marks_bytes).

Refuses to run with P1HIP_TEST_KNOBS set.  Prints one JSON line and writes it
to OUT.

env: REPS (5), DEVICE (0), OUT (profiles/below_batch_bench.json)."""
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def best_of(reps, fns, worst):
    """fns: {name: callable}; alternated, best wall seconds of each; `worst`
    receives the slowest repetition of each: the run-to-run spread."""
    best = {k: float("inf") for k in fns}
    for fn in fns.values():  # warm-up: buffers, clocks
        fn()
    for _ in range(reps):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            best[k] = min(best[k], dt)
            worst[k] = max(worst.get(k, 0.0), dt)
    return best


def workload(p1_amd, reps, name, reqs):
    from p1_amd import _lib

    lib = p1_amd.load()
    n = len(reqs)
    arr, rows = _lib._below_requests(reqs)
    total = sum(r[4] for r in rows)
    hits = (_lib.Result * total)()
    found = (ctypes.c_size_t * n)()
    one_hits = (_lib.Result * max(r[4] for r in rows))()
    one_found = ctypes.c_size_t(0)
    loop_args = [(m, len(m), lo, hi, t, cap) for m, lo, hi, t, cap in rows]
    loop_got = []

    def batch():
        rc = lib.p1hip_scan_below_batch(arr, n, hits, total, found)
        assert rc == 0, lib.p1hip_last_error()

    def loop():
        loop_got.clear()
        for a in loop_args:
            rc = lib.p1hip_scan_below(*a, one_hits, ctypes.byref(one_found))
            assert rc == 0, lib.p1hip_last_error()
            loop_got.append([(one_hits[k].hash, one_hits[k].nonce) for k in range(one_found.value)])

    # the same answers, before anything is timed
    batch()
    loop()
    off, nhits = 0, 0
    for i in range(n):
        assert [(hits[off + k].hash, hits[off + k].nonce) for k in range(found[i])] == loop_got[i], (name, i)
        off += rows[i][4]
        nhits += found[i]
    p1_amd.reset_stats()
    batch()
    s = p1_amd.get_below_batch_stats()
    p1_amd.reset_stats()
    loop()
    ls = p1_amd.get_below_stats()
    worst = {}
    best = best_of(reps, {"batch": batch, "loop": loop}, worst)
    spread = max(worst["batch"] - best["batch"], worst["loop"] - best["loop"])
    return {"workload": name, "requests": n, "hits": nhits,
            "batch_ms": round(best["batch"] * 1e3, 3), "loop_ms": round(best["loop"] * 1e3, 3),
            "batch_worst_ms": round(worst["batch"] * 1e3, 3), "loop_worst_ms": round(worst["loop"] * 1e3, 3),
            "speedup": round(best["loop"] / best["batch"], 2),
            "gain_ms": round((best["loop"] - best["batch"]) * 1e3, 3), "spread_ms": round(spread * 1e3, 3),
            "faster_by_more_than_the_spread": best["loop"] - best["batch"] > spread,
            "coalesced": s["coalesced"], "individual": s["individual"], "rounds": s["rounds"],
            "launch_pairs": s["launches"], "mark_nonces": s["mark_nonces"],
            "bytes_back_per_round": s["bytes_back"] // max(s["rounds"], 1),
            "loop_marks_bytes": ls["mark_nonces"] // 8, "loop_mark_launches": ls["mark_launches"]}


def main():
    if os.environ.get("P1HIP_TEST_KNOBS"):
        raise SystemExit("below_batch_bench: P1HIP_TEST_KNOBS is set; the timed process runs without test knobs")
    reps = int(os.environ.get("REPS", "5"))
    out = os.environ.get("OUT", os.path.join(ROOT, "profiles", "below_batch_bench.json"))

    import p1_amd

    p1_amd.init_devices([int(os.environ.get("DEVICE", "0"))])
    if p1_amd.test_knobs():
        raise SystemExit(f"below_batch_bench: test knobs in force: {p1_amd.test_knobs()}")
    rows = []
    for e in (56, 48):
        for n in (1, 16, 256, 4096):
            reqs = [(b"worker %d" % i, 0, (1 << 32) - 1, 1 << e, 1) for i in range(n)]
            rows.append(workload(p1_amd, reps, f"workers N={n} target 2^{e} cap 1", reqs))
    reqs = [(b"share %d" % i, 10 ** 9, 10 ** 9 + (1 << 16) - 1, 1 << 52, 1 << 16) for i in range(256)]
    rows.append(workload(p1_amd, reps, "every share: N=256 of 2^16 nonces, target 2^52, cap 65536", reqs))
    doc = {"what": f"p1hip_scan_below_batch against the loop of p1hip_scan_below on one MI355X, best of {reps} after "
                   f"a warm-up, wall ms around the library calls (ctypes, arguments marshalled beforehand) in one "
                   f"process, sides alternated; *_worst_ms is the slowest repetition, spread_ms the larger of the two "
                   f"sides' worst - best",
           "version": p1_amd.version(), "codeobj_sha256": p1_amd.codeobj_sha256(),
           "batch_codeobj_sha256": p1_amd.batch_codeobj_sha256(),
           "below_codeobj_sha256": p1_amd.below_codeobj_sha256(),
           "belowb_codeobj_sha256": p1_amd.belowb_codeobj_sha256(), "rows": rows}
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc), flush=True)


if __name__ == "__main__":
    main()
