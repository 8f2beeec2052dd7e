"""The index rules by which the phase kernel hands the equality block of a neighbour-row model to the rows solver ready-made
(soft-grip_amd/csrc/sg_rows_layout.h: sg_eq_fix_index, sg_eq_nb_index; the solver's staging trips: sg_eq_rec_*), on the host:
tests/emu/sg_rows_staging_index.cpp includes the headers and checks, for the committed two-finger models at 1, 5 and 9 envs, that every
(env, e, d) index lies inside the count sg_rows_work_each enumerates and that the indices are distinct, that the solver's lane mapping over
its record trips reaches each of an env's 4 (N + 1) rows exactly once with group N zero, and that the clamped addresses of the lanes
without a row and of the env slots past the batch stay inside the arrays; it reads every requested word from heap blocks of the library's
sizes.  The program is built with AddressSanitizer and UBSan and run directly: host code only (-Xarch_host), nothing of it runs on a GPU."""
import os
import shlex
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = ["softball", "softball_fix", "softbox", "softbox_fix", "softcylinder", "softcylinder_fix"]


def test_staging_indices_stay_inside_the_work_space(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc is needed to compile the header for the host")
    exe = str(tmp_path / "sg_rows_staging_index")
    flags = "-x hip --cuda-host-only -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined -fno-omit-frame-pointer"
    subprocess.check_call([hipcc] + shlex.split(flags) + ["-o", exe, os.path.join(ROOT, "tests", "emu", "sg_rows_staging_index.cpp"),
                                                           os.path.join(ROOT, "soft-grip_amd", "csrc", "sg_plan.cpp")])
    res = subprocess.run([exe] + [os.path.join(ROOT, "models", m + ".sgmodel") for m in MODELS], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    lines = res.stdout.strip().splitlines()
    assert lines[-1] == "PASS %d models" % len(MODELS) and len(lines) == len(MODELS) + 1, res.stdout[-3000:]
    trips = {line.split()[1].rstrip(":"): int(line.split()[-2]) for line in lines[:-1]}
    # softbox: 110 elements in the 112-row instantiation; the cylinder's 192 sit on a trip boundary (4 * 192 = 12 * 64); the ball: 218
    assert all(trips[m + ".sgmodel"] > 0 for m in ("softbox", "softcylinder", "softball")), trips
    assert all(trips[m + "_fix.sgmodel"] == 0 for m in ("softbox", "softcylinder", "softball")), trips
