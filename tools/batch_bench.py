#!/usr/bin/env python3
"""Small-request throughput: p1hip_scan_batch against the p1hip_scan loop.

For n = 1, 16, 256 and 4096 configs[0] requests (`bradfitz [0, 9999]`, 10^4
nonces each) it times one scan_batch call of n requests and n scan calls
(production's path for that size: the one-launch small path), best of --reps
each after a warm-up, and prints one JSON line: requests per second and GH/s
of both, their ratio, and the sha256 of both embedded code objects.  Both
sides are timed from Python, so both include this binding's marshalling;
batch_lib_us is the mean wall time inside p1hip_scan_batch itself
(p1hip_get_batch_stats), what a C or cgo caller pays.

    python3 tools/batch_bench.py [--device 0] [--reps 7] [--out FILE]

It refuses to run with the library's test knobs in force."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import p1_amd  # noqa: E402

REQ = ("bradfitz", 0, 9999)
WANT = (1419516646206828, 9898)
NONCES = REQ[2] - REQ[1] + 1


def best(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
        assert all(o == WANT for o in out), out[:3]
    return min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", help="also append the line to this file")
    a = ap.parse_args()
    p1_amd.init_devices([a.device])
    if p1_amd.test_knobs():
        sys.exit(f"test knobs in force: {p1_amd.test_knobs()}")
    rows = []
    for n in (1, 16, 256, 4096):
        reqs = [REQ] * n
        for _ in range(2):  # warm-up: buffers grown, clocks up
            p1_amd.scan_batch(reqs)
            [p1_amd.scan(*REQ) for _ in range(min(n, 64))]
        p1_amd.reset_stats()
        tb = best(lambda: p1_amd.scan_batch(reqs), a.reps)
        bs = p1_amd.get_batch_stats()
        tl = best(lambda: [p1_amd.scan(*r) for r in reqs], a.reps)
        rows.append({"requests": n,
                     "batch_us": round(tb * 1e6, 1), "batch_lib_us": round(bs["wall_ms"] / bs["calls"] * 1e3, 1),
                     "batch_req_per_s": round(n / tb), "batch_ghs": round(n * NONCES / tb / 1e9, 3),
                     "loop_us": round(tl * 1e6, 1), "loop_req_per_s": round(n / tl), "loop_ghs": round(n * NONCES / tl / 1e9, 3),
                     "ratio": round(tl / tb, 2)})
    line = json.dumps({"bench": "batch_bench", "request": list(REQ), "reps": a.reps, "rows": rows,
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
