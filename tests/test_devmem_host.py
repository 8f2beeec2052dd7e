"""The owners of the C ABI's device memory (soft-grip_amd/csrc/sg_devmem.h) on the host: tests/emu/sg_devmem_test.cpp includes the header
over counting fakes of the HIP calls and runs one sequence of allocations, uploads, a hand-over and scratch growth -- once clean, once
with each allocation and each copy failing in turn.  No block may be live once the owners are gone; the program checks the rest."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_no_block_outlives_its_owner_whatever_fails():
    emu = os.path.join(ROOT, "tests", "emu")
    subprocess.check_call(["make", "-s", "-C", emu, "sg_devmem_test"])
    res = subprocess.run([os.path.join(emu, "sg_devmem_test")], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = res.stdout.strip().splitlines()
    runs = [l for l in lines if l.startswith("run ")]
    assert lines[-1] == "PASS" and len(runs) == 1 + 8 + 3, res.stdout    # clean, 8 allocations, 3 copies
    assert all(l.endswith("live=0") for l in runs), res.stdout
