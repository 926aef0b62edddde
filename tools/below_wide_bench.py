"""p1hip_scan_below_batch_wide on one device against the loop of p1hip_scan_below
over the same requests.  The loop is what the library did with these requests
before the call existed, and what p1hip_scan_below_batch still does with them:
their first slice is sparse, so it runs them one by one (asserted once per row
from its `individual` count).

Workloads:
  workers  N = 1, 16, 256 requests `worker <i>` [0, 2^32), cap = 1, at targets
           2^42, 2^44 and 2^46 - 1: a pool's hard share target, first slices of
           2^23, 2^21 and 2^19 nonces
  chunks   256 chunks of 2^24 nonces of one message at target 2^32: a server's
           "first nonce at or below T" over a job, no hit expected
Both sides are called through ctypes with their arguments marshalled and their
result buffers allocated beforehand, so a figure is the time inside the
library call(s).  One process; best of REPS after a warm-up, the sides
alternated; the slowest repetition of each side is recorded as the spread.
The two sides' answers are compared before anything is timed.  Per row the
statistics of one call: rounds, groups, candidate tiles, bytes copied back.

Refuses to run with P1HIP_TEST_KNOBS set.  Prints one JSON line and writes it
to OUT.

env: REPS (5), DEVICE (0), OUT (profiles/below_wide_bench.json)."""
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

    def wide():
        rc = lib.p1hip_scan_below_batch_wide(arr, n, hits, total, found)
        assert rc == 0, lib.p1hip_last_error()

    def loop():
        loop_got.clear()
        for a in loop_args:
            rc = lib.p1hip_scan_below(*a, one_hits, ctypes.byref(one_found))
            assert rc == 0, lib.p1hip_last_error()
            loop_got.append([(one_hits[k].hash, one_hits[k].nonce) for k in range(one_found.value)])

    # the same answers, before anything is timed
    wide()
    loop()
    off, nhits = 0, 0
    for i in range(n):
        assert [(hits[off + k].hash, hits[off + k].nonce) for k in range(found[i])] == loop_got[i], (name, i)
        off += rows[i][4]
        nhits += found[i]
    # p1hip_scan_below_batch runs every one of these requests individually: the loop is its behaviour too
    assert all(x["route"] == "individual" for x in p1_amd.below_batch_layout(reqs, 1)), name
    p1_amd.reset_stats()
    wide()
    s = p1_amd.get_below_wide_stats()
    p1_amd.reset_stats()
    loop()
    ls = p1_amd.get_below_stats()
    worst = {}
    best = best_of(reps, {"wide": wide, "loop": loop}, worst)
    spread = max(worst["wide"] - best["wide"], worst["loop"] - best["loop"])
    return {"workload": name, "requests": n, "hits": nhits,
            "wide_ms": round(best["wide"] * 1e3, 3), "loop_ms": round(best["loop"] * 1e3, 3),
            "wide_worst_ms": round(worst["wide"] * 1e3, 3), "loop_worst_ms": round(worst["loop"] * 1e3, 3),
            "speedup": round(best["loop"] / best["wide"], 2),
            "gain_ms": round((best["loop"] - best["wide"]) * 1e3, 3), "spread_ms": round(spread * 1e3, 3),
            "faster_by_more_than_the_spread": best["loop"] - best["wide"] > spread,
            "wide_ghs": round(s["scan_nonces"] / best["wide"] / 1e9, 2), "loop_ghs": round(ls["scan_nonces"] / best["loop"] / 1e9, 2),
            "filtered": s["filtered"], "coalesced": s["coalesced"], "individual": s["individual"],
            "below_batch_individual": n, "rounds": s["rounds"], "groups": s["groups"],
            "scan_launches": s["scan_launches"], "scan_nonces": s["scan_nonces"], "candidate_tiles": s["candidate_tiles"],
            "slot_overflows": s["slot_overflows"], "mark_launches": s["mark_launches"], "bytes_back": s["bytes_back"],
            "loop_slices": ls["slices"], "loop_scan_nonces": ls["scan_nonces"], "loop_candidate_tiles": ls["candidate_tiles"]}


def main():
    if os.environ.get("P1HIP_TEST_KNOBS"):
        raise SystemExit("below_wide_bench: P1HIP_TEST_KNOBS is set; the timed process runs without test knobs")
    reps = int(os.environ.get("REPS", "5"))
    out = os.environ.get("OUT", os.path.join(ROOT, "profiles", "below_wide_bench.json"))

    import p1_amd

    p1_amd.init_devices([int(os.environ.get("DEVICE", "0"))])
    if p1_amd.test_knobs():
        raise SystemExit(f"below_wide_bench: test knobs in force: {p1_amd.test_knobs()}")
    rows = []
    for label, target in (("2^42", 1 << 42), ("2^44", 1 << 44), ("2^46-1", (1 << 46) - 1)):
        for n in (1, 16, 256):
            reqs = [(b"worker %d" % i, 0, (1 << 32) - 1, target, 1) for i in range(n)]
            rows.append(workload(p1_amd, reps, f"workers N={n} target {label} cap 1", reqs))
    chunk = 1 << 24
    reqs = [(b"bradfitz", 10 ** 10 + i * chunk, 10 ** 10 + (i + 1) * chunk - 1, 1 << 32, 1) for i in range(256)]
    rows.append(workload(p1_amd, reps, "server chunks: N=256 of 2^24 nonces, target 2^32, cap 1", reqs))
    doc = {"what": f"p1hip_scan_below_batch_wide against the loop of p1hip_scan_below on one MI355X, best of {reps} "
                   f"after a warm-up, wall ms around the library calls (ctypes, arguments marshalled beforehand) in one "
                   f"process, sides alternated; *_worst_ms is the slowest repetition, spread_ms the larger of the two "
                   f"sides' worst - best; *_ghs is k_scan nonces per second of wall time",
           "version": p1_amd.version(), "codeobj_sha256": p1_amd.codeobj_sha256(),
           "batch_codeobj_sha256": p1_amd.batch_codeobj_sha256(),
           "below_codeobj_sha256": p1_amd.below_codeobj_sha256(),
           "belowb_codeobj_sha256": p1_amd.belowb_codeobj_sha256(),
           "beloww_codeobj_sha256": p1_amd.beloww_codeobj_sha256(), "rows": rows}
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc), flush=True)


if __name__ == "__main__":
    main()
