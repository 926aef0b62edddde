"""p1miner serve --batch B: request lines are collected and answered together
through one p1hip_scan_batch call (miner::HandleBatch), one Result line per
request line, in order -- the same lines `p1miner serve` gives one by one."""
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


def test_batch_option_is_parsed_before_the_device_is_opened():
    r = run([])
    assert r.returncode == 2 and "--batch B" in r.stderr
    for bad in ("0", "x", "-3"):
        r = run(["serve", "--batch", bad])
        assert r.returncode == 2 and r.stdout == "" and "p1hip init" not in r.stderr, bad


@pytest.mark.gpu
def test_serve_batch_answers_like_serve():
    lines = [req("bradfitz", 0, 9999), req("msg", 0, 2), "this is not JSON", req("msg", 5, 4),
             req("cmu440", 10 ** 9 - 70000, 10 ** 9 + 70000), req("", 99, 100)]
    plain = run(["serve", "--device", "0"], "\n".join(lines) + "\n")
    assert plain.returncode == 0, plain.stderr
    want = plain.stdout.splitlines()
    assert len(want) == 6
    assert json.loads(want[0])["Hash"] == 1419516646206828 and json.loads(want[0])["Nonce"] == 9898
    assert want[2] == run(["serve", "--device", "0"], req("", 0, 0) + "\n").stdout.splitlines()[0]
    # 4 + 2: the B-th line flushes, the empty line flushes the rest and is not answered
    got = run(["serve", "--device", "0", "--batch", "4"], "\n".join(lines) + "\n\n")
    assert got.returncode == 0, got.stderr
    assert got.stdout.splitlines() == want
    # EOF flushes too; --batch 1 is plain serve, which answers the empty line as a one-nonce request
    assert run(["serve", "--device", "0", "--batch", "16"], "\n".join(lines) + "\n").stdout.splitlines() == want
    one = run(["serve", "--device", "0", "--batch", "1"], "\n".join(lines) + "\n\n").stdout.splitlines()
    assert one == want + [want[2]]
