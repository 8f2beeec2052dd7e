"""The index rule of the solver's look-ahead (soft-grip_amd/csrc/sg_work.h: sg_rows_load_slot) on the host: tests/emu/sg_rows_touch_index.cpp
includes the header and checks, for every slot i and stream length nsmax in [0, SG_CAP], look-ahead distances up to 2 (what sg_rows.hip
uses) and up to 4, and 4 and 8 envs per wavefront, that every loaded slot lies in [0, nsmax - 1] -- inside the SG_CAP + 2 slots that are
allocated -- and that a pass loads slots 0 .. nsmax - 1 once each; it reads every requested word from an allocation of the library's
size.  The program is built with AddressSanitizer and UBSan and run directly: host code only (-Xarch_host), nothing of it runs on a GPU.  (The touch-ahead this file is named after was measured
as a loss and is not in the kernel: profiles/r06_rows_lookahead_ab.txt.)"""
import os
import shlex
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_look_ahead_slots_stay_inside_the_stream(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc is needed to compile the header for the host")
    exe = str(tmp_path / "sg_rows_touch_index")
    flags = "-x hip --cuda-host-only -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined -fno-omit-frame-pointer"
    subprocess.check_call([hipcc] + shlex.split(flags) + ["-o", exe, os.path.join(ROOT, "tests", "emu", "sg_rows_touch_index.cpp")])
    ds = ["2", "4"]
    res = subprocess.run([exe] + ds, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    lines = res.stdout.strip().splitlines()
    assert lines[-1] == "PASS" and len(lines) == 2 * len(ds) + 1, res.stdout
