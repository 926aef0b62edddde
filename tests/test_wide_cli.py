"""p1miner serve --batch B --wide: the collected request lines go through one
p1hip_scan_batch_wide call (miner::HandleBatch(reqs, chunk, wide = true)) and
are answered exactly as `p1miner serve` answers them one by one."""
import json
import os
import subprocess

import pytest

from conftest import ROOT

MINER = os.path.join(ROOT, "p1_amd", "p1miner")


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(MINER):
        subprocess.run(["make", "-s", "-C", ROOT, "p1_amd/p1miner"], check=True)


def run(args, stdin=None):
    # one visible GPU: without --device the miner opens every visible device
    env = dict(os.environ, HIP_VISIBLE_DEVICES=os.environ.get("HIP_VISIBLE_DEVICES", "0").split(",")[0])
    for k in [k for k in env if k.startswith("P1HIP_")]:
        del env[k]  # production settings, whatever the session's GPU fixture set
    return subprocess.run([MINER] + args, input=stdin, capture_output=True, text=True, timeout=120, env=env)


def req(data, lo, hi):
    return json.dumps({"Type": 1, "Data": data, "Lower": lo, "Upper": hi, "Hash": 0, "Nonce": 0}, separators=(",", ":"))


def test_wide_option_is_in_the_usage_and_parsed_before_the_device_is_opened():
    r = run([])
    assert r.returncode == 2 and "--batch B [--wide]" in r.stderr
    r = run(["serve", "--wide", "--batch", "0"])
    assert r.returncode == 2 and r.stdout == "" and "p1hip init" not in r.stderr


@pytest.mark.gpu
def test_serve_batch_wide_answers_like_serve():
    lines = [req("bradfitz", 0, 99999), req("msg", 0, 2), "this is not JSON", req("msg", 5, 4),
             req("cmu440", 10 ** 9 - 70000, 10 ** 9 + 70000), req("bradfitz", 0, 9999)]
    plain = run(["serve", "--device", "0"], "\n".join(lines) + "\n")
    assert plain.returncode == 0, plain.stderr
    want = plain.stdout.splitlines()
    assert len(want) == 6 and json.loads(want[5])["Nonce"] == 9898
    got = run(["serve", "--device", "0", "--batch", "4", "--wide"], "\n".join(lines) + "\n\n")
    assert got.returncode == 0, got.stderr
    assert got.stdout.splitlines() == want
    assert run(["serve", "--device", "0", "--wide", "--batch", "16"], "\n".join(lines) + "\n").stdout.splitlines() == want
