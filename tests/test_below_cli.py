"""p1miner scan <msg> <lower> <upper> --below <target> [--count N]: argument
errors and the usage text (no device: every case here ends before one is
opened); the answers themselves are tests/test_gpu_below.py's."""
import os
import subprocess

import pytest

from conftest import ROOT

MINER = os.path.join(ROOT, "p1_amd", "p1miner")


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(MINER):
        subprocess.run(["make", "-s", "-C", ROOT, "p1_amd/p1miner"], check=True)


def run(args):
    env = {k: v for k, v in os.environ.items() if not k.startswith("P1HIP_")}
    return subprocess.run([MINER] + args, capture_output=True, text=True, timeout=60, env=env)


def test_below_is_in_the_usage():
    r = run([])
    assert r.returncode == 2 and "scan <msg> <lower> <upper> [--below <target> [--count N]]" in r.stderr


@pytest.mark.parametrize("args", [
    ["--below"],                        # no target
    ["--below", "x"], ["--below", "-1"], ["--below", "1e9"], ["--below", "18446744073709551616"],
    ["--below", "5", "--count"],        # no count
    ["--below", "5", "--count", "0"], ["--below", "5", "--count", "-3"], ["--below", "5", "--count", "many"],
    ["--count", "3"],                   # --count means nothing without --below
    ["--below", "5", "--wide"], ["--above", "5"], ["5"],
])
def test_below_argument_errors(args):
    r = run(["scan", "bradfitz", "0", "9999"] + args)
    assert r.returncode == 2 and r.stdout == "" and r.stderr.startswith("usage: p1miner"), (args, r.stderr)
    assert "p1hip" not in r.stderr.replace("usage: p1miner", "")  # parsed before any device is opened


def test_below_range_errors_and_empty_ranges():
    assert run(["scan", "bradfitz", "-1", "5", "--below", "7"]).returncode == 2
    assert run(["scan", "bradfitz", "0", "x", "--below", "7"]).returncode == 2
    # lower > upper: no hit, no line, exit 0, no device
    r = run(["scan", "bradfitz", "9", "3", "--below", "18446744073709551615", "--count", "4"])
    assert (r.returncode, r.stdout, r.stderr) == (0, "", "")


@pytest.mark.gpu
def test_below_cli_answers():
    """One Result line per hit in nonce order; no line when there is none."""
    env = dict(HIP_VISIBLE_DEVICES=os.environ.get("HIP_VISIBLE_DEVICES", "0").split(",")[0])
    def go(*a):
        e = {k: v for k, v in os.environ.items() if not k.startswith("P1HIP_")}
        e.update(env)
        return subprocess.run([MINER, "scan", "bradfitz", *a], capture_output=True, text=True, timeout=120, env=e)

    r = go("0", "9999", "--below", "1419516646206828")
    assert (r.returncode, r.stdout) == (0, "Result 1419516646206828 9898\n"), r.stderr
    r = go("0", "9999", "--below", "1419516646206827")
    assert (r.returncode, r.stdout) == (0, ""), r.stderr
    r = go("0", "99999", "--below", "300000000000000", "--count", "5")
    assert (r.returncode, r.stdout) == (0, "Result 158752571039048 91989\nResult 85364550342847 98985\n"), r.stderr
    r = go("0", "99999", "--count", "1", "--below", "300000000000000")
    assert (r.returncode, r.stdout) == (0, "Result 158752571039048 91989\n"), r.stderr
    r = go("0", "4", "--below", "18446744073709551615", "--count", "3")
    assert r.returncode == 0 and [ln.split()[2] for ln in r.stdout.splitlines()] == ["0", "1", "2"], r.stderr
    # without --below the command is what it always was
    r = go("0", "9999")
    assert (r.returncode, r.stdout) == (0, "Result 1419516646206828 9898\n"), r.stderr
