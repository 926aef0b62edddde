"""p1miner below --hard: the batches go through p1hip_scan_below_batch_wide, and
every line is answered exactly as `p1miner below` answers it.  (The flag is not
spelled --wide: `p1miner below --wide` has been a usage error since the command
exists, and tests/test_below_batch_cli.py keeps it one.)"""
import os
import subprocess

import pytest

from conftest import ROOT

MINER = os.path.join(ROOT, "p1_amd", "p1miner")
U64_MAX = (1 << 64) - 1


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(MINER):
        subprocess.run(["make", "-s", "-C", ROOT, "p1_amd/p1miner"], check=True)


def run(args, text="", extra_env=None):
    env = {k: v for k, v in os.environ.items() if not k.startswith("P1HIP_")}
    env.update(extra_env or {})
    return subprocess.run([MINER, "below"] + args, input=text, capture_output=True, text=True, timeout=120, env=env)


def test_hard_flag_is_in_the_usage_and_parsed_before_any_device():
    r = subprocess.run([MINER], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "below [--device N] [--batch B] [--hard]" in r.stderr
    r = run(["--hard", "--batch"], "6d7367 0 9 5 1\n")
    assert r.returncode == 2 and r.stdout == "" and r.stderr.startswith("usage: p1miner")


def test_hard_without_a_device():
    assert (lambda r: (r.returncode, r.stdout, r.stderr))(run(["--hard"])) == (0, "", "")
    # empty requests are answered on the host, every line in order; the empty line is not answered
    r = run(["--hard", "--batch", "2"], f"6d7367 5 4 {U64_MAX} 3\n- 0 9 {U64_MAX} 0\n\n- 9 3 0 1\n")
    assert (r.returncode, r.stdout, r.stderr) == (0, "Hits 0\nHits 0\nHits 0\n", "")
    r = run(["--hard"], "6d7367 5 4 7 1\n6d7367 0 9 5\n")
    assert r.returncode == 1 and r.stdout == "Hits 0\n" and "line 2" in r.stderr


@pytest.mark.gpu
def test_hard_answers_line_for_line_as_below_does():
    env = dict(HIP_VISIBLE_DEVICES=os.environ.get("HIP_VISIBLE_DEVICES", "0").split(",")[0])
    brad = b"bradfitz".hex()
    text = (f"{brad} 0 9999 1419516646206828 1\n"
            f"{brad} 0 9999 1419516646206827 1\n"
            f"{brad} 0 99999 300000000000000 5\n"
            f"- 7 3 {U64_MAX} 2\n"
            f"{b'worker 4'.hex()} 0 4294967295 {1 << 44} 1\n"   # filtered: its first slice is 2^21 nonces, sparse
            f"{b'worker 21'.hex()} 0 4294967295 {1 << 44} 1\n"  # ... and this one needs a second round
            f"{brad} 1000000000 1016777215 4294967296 1\n"       # the server's question over 2^24 nonces: no hit
            f"{brad} 0 4 {U64_MAX} 3\n")
    plain = run(["--device", "0"], text, env)
    hard = run(["--hard", "--device", "0"], text, env)
    assert plain.returncode == 0 == hard.returncode, (plain.stderr, hard.stderr)
    assert hard.stdout == plain.stdout
    lines = hard.stdout.splitlines()
    assert lines[:2] == ["Hits 1", "Result 1419516646206828 9898"] and lines.count("Hits 0") == 3
    assert "Result 3619863100506 126327" in lines and "Result 10680350058760 2387275" in lines
    batched = run(["--hard", "--batch", "3", "--device", "0"], text, env)
    assert batched.returncode == 0 and batched.stdout == plain.stdout
