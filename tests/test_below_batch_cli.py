"""p1miner below [--device N] [--batch B]: argument errors, the usage text and
what needs no device (empty requests, a line that does not parse), then one
batch on the GPU against the answers of tests/test_below_cli.py."""
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


def test_below_command_is_in_the_usage():
    r = subprocess.run([MINER], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "below [--device N] [--batch B]" in r.stderr


@pytest.mark.parametrize("args", [
    ["--batch"], ["--batch", "0"], ["--batch", "-2"], ["--batch", "many"], ["--device"], ["--device", "x"],
    ["--device", "-1"], ["--wide"], ["7"],
])
def test_below_command_argument_errors(args):
    r = run(args, "6d7367 0 9 5 1\n")
    assert r.returncode == 2 and r.stdout == "" and r.stderr.startswith("usage: p1miner"), (args, r.stderr)
    assert "p1hip" not in r.stderr.replace("usage: p1miner", "")  # parsed before any device is opened


def test_below_command_without_a_device():
    # no line: nothing to answer
    assert (lambda r: (r.returncode, r.stdout, r.stderr))(run([])) == (0, "", "")
    # empty requests are answered on the host, every line in order; the empty line is not answered
    r = run(["--batch", "2"], f"6d7367 5 4 {U64_MAX} 3\n- 0 9 {U64_MAX} 0\n\n- 9 3 0 1\n")
    assert (r.returncode, r.stdout, r.stderr) == (0, "Hits 0\nHits 0\nHits 0\n", "")


@pytest.mark.parametrize("line", [
    "6d7367 0 9 5", "6d7367 0 9 5 1 1", "6d736 0 9 5 1", "zz 0 9 5 1", "6d7367 -1 9 5 1", "6d7367 0 9 5 x",
    "6d7367 0 18446744073709551616 5 1",
])
def test_below_command_refuses_a_bad_line_after_answering_the_ones_before(line):
    r = run([], f"6d7367 5 4 7 1\n{line}\n6d7367 5 4 7 1\n")
    assert r.returncode == 1 and r.stdout == "Hits 0\n" and "line 2" in r.stderr, r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("batch", ["2", "256"])
def test_below_command_answers(batch):
    """Every line is answered, in order, with Hits <found> and its Result lines."""
    env = dict(HIP_VISIBLE_DEVICES=os.environ.get("HIP_VISIBLE_DEVICES", "0").split(",")[0])
    brad = b"bradfitz".hex()
    text = (f"{brad} 0 9999 1419516646206828 1\n"
            f"{brad} 0 9999 1419516646206827 1\n"
            f"{brad} 0 99999 300000000000000 5\n"
            f"- 7 3 {U64_MAX} 2\n"
            f"{brad} 0 99999 300000000000000 1\n"
            f"{brad} 0 4 {U64_MAX} 3\n")
    r = run(["--batch", batch, "--device", "0"], text, env)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert lines[:7] == ["Hits 1", "Result 1419516646206828 9898", "Hits 0", "Hits 2", "Result 158752571039048 91989",
                         "Result 85364550342847 98985", "Hits 0"]
    assert lines[7:9] == ["Hits 1", "Result 158752571039048 91989"]
    assert lines[9] == "Hits 3" and [ln.split()[2] for ln in lines[10:]] == ["0", "1", "2"] and len(lines) == 13
