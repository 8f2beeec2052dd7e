"""The kernel plans are pinned: tests/emu/sg_plan_dump.cpp builds the plan of every input with both builders (sg_plan_build, sg_tree_plan_build)
and prints, per builder, the refusal message or a hash of the raw bytes of each part of the plan (SgPlanHeader, elem, elem_geom, elem_dofmap,
nbtab, sched, gpairs, SgTreeDev), and per compiled .xml and composite variant a hash of the blob the native MJCF compiler wrote (`blob:`).
tests/golden/plan_digests.json holds that output; the comparison is exact.

Inputs: the committed models/*.sgmodel, every tests/data/*.xml in both composite variants, and 32 seeded random grippers of the tree class
(helpers.random_gripper_xml), every second one on a free joint.

When a plan is changed ON PURPOSE, regenerate the file with
    python tests/test_plan_digest.py --regen "<what made it: commit and reason>"
and review the diff of the golden file: only the models the change is meant to reach may move."""
import glob
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from helpers import random_gripper_xml  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "plan_digests.json")
N_RANDOM, SEED = 32, 4711


def _digests(tmpdir):
    """label -> the program's line for it, over the whole input set"""
    emu = os.path.join(ROOT, "tests", "emu")
    subprocess.check_call(["make", "-s", "-C", emu, "sg_plan_dump"])
    inputs = sorted(glob.glob(os.path.join(ROOT, "models", "*.sgmodel"))) + sorted(glob.glob(os.path.join(ROOT, "tests", "data", "*.xml")))
    rng = np.random.RandomState(SEED)
    for i in range(N_RANDOM):
        path = os.path.join(str(tmpdir), "random_gripper_%02d.xml" % i)
        with open(path, "w") as f:
            f.write(random_gripper_xml(rng, free=bool(i % 2)))
        inputs.append(path)
    res = subprocess.run([os.path.join(emu, "sg_plan_dump")] + inputs, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    out = {}
    for line in res.stdout.splitlines():
        label, _, rest = line.partition(": ")
        assert rest and label not in out, line
        out[label] = rest
    return out


def test_plans_match_the_pinned_digests(tmp_path):
    with open(GOLDEN) as f:
        golden = json.load(f)["digests"]
    got = _digests(tmp_path)
    assert len(got) >= 2 * (10 + 2 * N_RANDOM)
    refused = lambda builder: {v for k, v in golden.items() if k.endswith(builder) and v.startswith("refused")}  # noqa: E731
    accepted = lambda builder: [v for k, v in golden.items() if k.endswith(builder) and v.startswith("header=")]  # noqa: E731
    assert refused(" two") and refused(" tree") and accepted(" two") and accepted(" tree")   # the set reaches refusals and plans of both builders
    assert sorted(got) == sorted(golden), sorted(set(got) ^ set(golden))
    diff = ["%s\n  pinned: %s\n  now:    %s" % (k, golden[k], got[k]) for k in sorted(got) if got[k] != golden[k]]
    assert not diff, "%d of %d plans changed:\n%s" % (len(diff), len(got), "\n".join(diff))


if __name__ == "__main__":
    import tempfile
    assert len(sys.argv) == 3 and sys.argv[1] == "--regen", __doc__
    with tempfile.TemporaryDirectory() as tmp:
        digests = _digests(tmp)
    with open(GOLDEN, "w") as f:
        json.dump({"header": sys.argv[2], "digests": digests}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d lines -> %s" % (len(digests), GOLDEN))
