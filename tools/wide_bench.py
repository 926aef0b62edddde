#!/usr/bin/env python3
"""Mid-size request throughput: p1hip_scan_batch_wide against the p1hip_scan loop.

For requests of 10^5, 10^6 and 10^7 nonces (`bradfitz [10^9, 10^9 + size - 1]`)
and n = 16, 256 (and 4096 at 10^5) requests per call it times one
scan_batch_wide call of n requests and n scan calls (what p1hip_scan_batch
does with requests of that size), best of --reps each after a warm-up, and
prints one JSON line: microseconds, requests per second and GH/s of both,
their ratio, the k_scan launches, segments and tiles of the wide call, and
the sha256 of both embedded code objects.  Both sides are timed from Python,
so both include this binding's marshalling; wide_lib_us is the mean wall time
inside p1hip_scan_batch_wide itself (p1hip_get_wide_stats), what a C or cgo
caller pays.  Every answer of the wide call must equal the loop's.

    python3 tools/wide_bench.py [--device 0] [--reps 5] [--floor F] [--out FILE]

It refuses to run with the library's test knobs in force, except the one it
sets itself for --floor F: the occupancy floor the wide requests are planned
with (P1HIP_WIDE_MIN_FAST_THREADS) instead of the library's rule, recorded in
the line, to compare the rule with its alternatives (1 keeps k = 3; 262144 is
the planner's per-request floor)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import p1_amd  # noqa: E402

CASES = [(10 ** 5, 16), (10 ** 5, 256), (10 ** 5, 4096), (10 ** 6, 16), (10 ** 6, 256), (10 ** 7, 16), (10 ** 7, 256)]
BASE = 10 ** 9


def best(fn, reps):
    ts, out = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return min(ts), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--floor", type=int, default=0)
    ap.add_argument("--out", help="also append the line to this file")
    a = ap.parse_args()
    if p1_amd.load() and p1_amd.test_knobs():
        sys.exit(f"test knobs in force: {p1_amd.test_knobs()}")
    if a.floor:
        os.environ["P1HIP_TEST_KNOBS"] = "1"
        os.environ["P1HIP_WIDE_MIN_FAST_THREADS"] = str(a.floor)
    p1_amd.init_devices([a.device])
    rows = []
    for size, n in CASES:
        reqs = [("bradfitz", BASE, BASE + size - 1)] * n
        for _ in range(2):  # warm-up: buffers grown, clocks up
            p1_amd.scan_batch_wide(reqs)
            [p1_amd.scan(*reqs[0]) for _ in range(min(n, 16))]
        p1_amd.reset_stats()
        tw, got = best(lambda: p1_amd.scan_batch_wide(reqs), a.reps)
        ws = p1_amd.get_wide_stats()
        assert ws["wide"] == n * a.reps, ws
        tl, ref = best(lambda: [p1_amd.scan(*r) for r in reqs], a.reps)
        assert got == ref, (size, n, got[:2], ref[:2])
        rows.append({"nonces": size, "requests": n,
                     "wide_us": round(tw * 1e6, 1), "wide_lib_us": round(ws["wall_ms"] / ws["calls"] * 1e3, 1),
                     "wide_req_per_s": round(n / tw), "wide_ghs": round(n * size / tw / 1e9, 3),
                     "loop_us": round(tl * 1e6, 1), "loop_req_per_s": round(n / tl), "loop_ghs": round(n * size / tl / 1e9, 3),
                     "ratio": round(tl / tw, 2), "scan_launches": ws["scan_launches"] // ws["calls"],
                     "scan_segments": ws["scan_segments"] // ws["calls"], "tiles": ws["tiles"] // ws["calls"]})
    line = json.dumps({"bench": "wide_bench", "base": BASE, "reps": a.reps, "floor": a.floor or "rule", "rows": rows,
                       "device": p1_amd.device_info(0), "library": p1_amd.version(),
                       "codeobj_sha256": p1_amd.codeobj_sha256(), "batch_codeobj_sha256": p1_amd.batch_codeobj_sha256()})
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
    p1_amd.shutdown()


if __name__ == "__main__":
    main()
