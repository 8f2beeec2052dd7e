"""The host side of the rows pipeline (soft-grip_amd/csrc/sg_rows_host.h: admission, the launch shape, the solver's tables, the size of
every work-space buffer) without a GPU: tests/emu/sg_rows_host_test.cpp decodes the tables by the kernels' rules, reads every address the
kernels form from heap blocks of the enumerated sizes, and prints digests of what the header makes.  The program is built with
AddressSanitizer and UBSan and run directly: host code only (-Xarch_host), nothing of it is loaded into Python or runs on a GPU.

tests/golden/rows_host_digests.json pins the digest lines: the padded schedule, the table words and cpos of every committed two-finger
model and its work-space counts at 1, 9 and 4096 envs.  Its header says which commit's expressions produced it; the comparison is exact."""
import json
import os
import shlex
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "rows_host_digests.json")
MODELS = ["softball", "softball_fix", "softbox", "softbox_fix", "softcylinder", "softcylinder_fix"]   # softbox_fix: no neighbour rows; softbox:
# step factors in LDS, two-word table; softcylinder: streamed factors, one-word table; softball: streamed, four element rounds


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc is needed to compile the header for the host")
    exe = str(tmp_path_factory.mktemp("rows_host") / "sg_rows_host_test")
    flags = "-x hip --cuda-host-only -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined -fno-omit-frame-pointer"
    subprocess.check_call([hipcc] + shlex.split(flags) + ["-o", exe, os.path.join(ROOT, "tests", "emu", "sg_rows_host_test.cpp"),
                                                           os.path.join(ROOT, "soft-grip_amd", "csrc", "sg_plan.cpp")])
    res = subprocess.run([exe] + [os.path.join(ROOT, "models", m + ".sgmodel") for m in MODELS], capture_output=True, text=True, timeout=120)
    return res


def test_tables_and_work_space_hold_what_the_kernels_index(output):
    assert output.returncode == 0, output.stdout[-3000:] + output.stderr[-3000:]
    lines = output.stdout.strip().splitlines()
    assert lines[-1] == "PASS %d models" % len(MODELS), output.stdout[-3000:]
    assert sum(line.startswith("checked ") for line in lines) == len(MODELS)
    modes = {line.split()[1].rstrip(":"): int(line.split("mode ")[1][0]) for line in lines if line.startswith("checked ")}
    assert modes == {"softball.sgmodel": 2, "softcylinder.sgmodel": 2, "softbox.sgmodel": 1, "softball_fix.sgmodel": 0, "softbox_fix.sgmodel": 0,
                     "softcylinder_fix.sgmodel": 0}      # every table format and the models without tables are reached


def test_tables_and_counts_match_the_pinned_digests(output):
    with open(GOLDEN) as f:
        golden = json.load(f)["digests"]
    got = {}
    for line in output.stdout.splitlines():
        label, _, rest = line.partition(": ")
        if label.endswith(".sgmodel") and " " not in label:      # (not the "checked NAME: ..." lines)
            got[label] = rest
    assert sorted(got) == sorted(golden) == sorted(m + ".sgmodel" for m in MODELS)
    diff = ["%s\n  pinned: %s\n  now:    %s" % (k, golden[k], got[k]) for k in sorted(got) if got[k] != golden[k]]
    assert not diff, "\n".join(diff)
