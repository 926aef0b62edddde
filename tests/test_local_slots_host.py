"""The server's local slots without threads, network or GPU.

`tools/local_slots_test` (tests/local_slots_test.cpp) drives
server::LocalSlots (p1_amd/host/local_slots.hpp) over a real
sched::Scheduler -- with the per-miner chunk of Scheduler::AddMiner(miner,
chunk) -- through random requests, lost clients, lost remote miners and backend
failures, every piece answered by the CPU oracle: 135 scenarios over
--local-chunk 1 / 1000 / 2^16, 1 / 3 / 64 slots and 1 / 2 / 4 rounds in flight.
What it asserts is listed at the top of the .cpp file."""
import os
import subprocess

import pytest

from conftest import ROOT, host_bin

LOCAL_SLOTS_TEST = host_bin(os.path.join(ROOT, "tools", "local_slots_test"))


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(LOCAL_SLOTS_TEST):
        subprocess.run(["make", "-s", "-C", ROOT, "tools/local_slots_test"], check=True)


def test_local_slots_model():
    r = subprocess.run([LOCAL_SLOTS_TEST], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "all passed" in r.stdout, r.stdout + r.stderr[-3000:]
    assert "scenarios 135 " in r.stdout, r.stdout


def test_local_slots_model_other_seed():
    r = subprocess.run([LOCAL_SLOTS_TEST, "977"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "all passed" in r.stdout, r.stdout + r.stderr[-3000:]
