"""Back-to-back batch calls on one device: the synchronous call in a loop
against p1hip_batch_submit / p1hip_batch_wait at depth 1, 2 and 4.

For every shape, K calls of the same requests are timed three ways:
  sync     K x scan_batch / scan_batch_wide, one after the other
  depth 1  K x (submit, wait)
  depth D  every call is submitted before the oldest outstanding one is
           waited, D = 2 and 4: the host marshals call k + 1 while the device
           runs call k
Shapes: 16 x 10^6 nonces and 256 x 10^5 nonces (wide), 256 x 10^4 (small).
Each figure is the best of REPS repetitions after a warm-up, in us per call;
the results of every way are compared with the synchronous call's.  Prints
one JSON line and writes it to OUT.

env: K (32), REPS (5), DEVICE (0), OUT (profiles/async_bench.json)."""
import json
import os
import sys
import time
from collections import deque

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("16 x 10^6 wide", 16, 10 ** 6, True), ("256 x 10^5 wide", 256, 10 ** 5, True),
          ("256 x 10^4 small", 256, 10 ** 4, False)]


def main():
    import p1_amd

    k_calls = int(os.environ.get("K", "32"))
    reps = int(os.environ.get("REPS", "5"))
    out = os.environ.get("OUT", os.path.join(ROOT, "profiles", "async_bench.json"))
    p1_amd.init_devices([int(os.environ.get("DEVICE", "0"))])
    if p1_amd.test_knobs():
        raise SystemExit(f"async_bench: test knobs in force: {p1_amd.test_knobs()}")
    rows = []
    for name, n, size, wide in SHAPES:
        reqs = [(b"async bench %d" % i, 10 ** 9 + i * size, 10 ** 9 + (i + 1) * size - 1) for i in range(n)]
        sync = p1_amd.scan_batch_wide if wide else p1_amd.scan_batch
        want = sync(reqs)

        def run_sync():
            for _ in range(k_calls):
                assert sync(reqs) == want

        def run_depth(depth):
            def run():
                q = deque()
                for _ in range(k_calls):
                    if len(q) == depth:
                        assert p1_amd.batch_wait(q.popleft()) == want
                    q.append(p1_amd.batch_submit(reqs, wide=wide))
                while q:
                    assert p1_amd.batch_wait(q.popleft()) == want
            return run

        ways = [("sync", run_sync)] + [(f"depth{d}", run_depth(d)) for d in (1, 2, 4)]
        row = {"shape": name, "requests": n, "nonces_per_request": size, "wide": wide}
        best = {w: float("inf") for w, _ in ways}
        for w, fn in ways:  # warm-up: buffers of every slot, clocks
            fn()
        for _ in range(reps):  # the ways interleaved, so that drift hits all alike
            for w, fn in ways:
                t0 = time.perf_counter()
                fn()
                best[w] = min(best[w], time.perf_counter() - t0)
        for w, _ in ways:
            row[w + "_us_per_call"] = round(best[w] / k_calls * 1e6, 2)
        for d in (1, 2, 4):
            row[f"depth{d}_over_sync"] = round(best["sync"] / best[f"depth{d}"], 3)  # > 1: faster than the loop
        rows.append(row)
    doc = {"what": f"{k_calls} back-to-back calls per way, best of {reps}, us per call, timed from Python in one "
                   f"process on one MI355X; depthD_over_sync = sync time / depth-D time",
           "version": p1_amd.version(), "codeobj_sha256": p1_amd.codeobj_sha256(),
           "batch_codeobj_sha256": p1_amd.batch_codeobj_sha256(), "rows": rows}
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc), flush=True)


if __name__ == "__main__":
    main()
