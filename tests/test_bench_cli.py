"""bench.py's command line on the CPU, over tests/fake_native.py (through tests/run_with_fake_native.py): a plain run times exactly
--steps steps and its line carries the headline only; --full adds the measurements that take runs of their own (the HIP-event pass with
the roofline block, the fix-only variant, the CPU baseline); --dump-outputs writes what the headline pass computed."""
import json
import os
import subprocess
import sys

import numpy as np

from helpers import ROOT

FAKE = os.path.join(ROOT, "tests", "run_with_fake_native.py")
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _bench(*args):
    """-> (the result line, the work the run did: tests/run_with_fake_native.py's counts of batches, resets, substeps,
    profile_enable(True) calls and CPU-oracle step_many calls)"""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run([sys.executable, FAKE, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--envs", "8"] + list(args),
                         capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    work = [ln for ln in out.stderr.splitlines() if ln.startswith("run_with_fake_native: work ")]
    assert len(work) == 1, out.stderr[-2000:]
    return json.loads(lines[0]), json.loads(work[0].split(" work ", 1)[1])


def test_plain_run_times_exactly_the_steps_asked_for_and_dumps_its_outputs(tmp_path):
    # (steps, whole episodes, episode index of the last timed step): the stratified remainder r takes the midpoints of r strata
    for steps, whole, last in ((20, 0, 195), (200, 1, 199), (300, 1, 199), (450, 2, 198)):
        d = tmp_path / str(steps)
        res, work = _bench("--steps", str(steps), "--warmup", "3", "--dump-outputs", str(d))
        assert all(k in res for k in HEADLINE) and res["steps"] == steps and res["config"]["steps_timed"] == steps
        assert abs(res["value"] - 8 / (res["ms_per_step"] * 1e-3)) < 1e-6 * res["value"]
        region = res["config"]["timed_region"]
        assert ("%d whole episode(s)" % whole in region) == (whole > 0) and ("stratified" in region) == (steps % 200 > 0), region
        assert not any(k in res for k in ("roofline", "cpu_baseline", "ms_per_step_with_hip_events")) and "fix_only_variant" not in res["config"]
        # and the work itself is only the headline's: one batch, the warm-up (a reset + 3 steps), then one reset and 200 steps per episode
        # the timed region runs -- no second pass with HIP events, no fix-only batch, no CPU oracle
        episodes = whole + (steps % 200 > 0)
        assert work == {"batches": 1, "resets": 1 + episodes, "substeps": 1 + 3 * 7 + episodes * (1 + 200 * 7), "profile_on": 0,
                        "oracle_step_many": 0}, work
        out = {f[:-4]: np.load(d / f) for f in os.listdir(d)}
        assert set(out) == {"sensors", "flags", "episode_sensors"} and all(a.dtype == np.float64 for a in out.values())
        # the fake batch's sensors count substeps: env step t of an episode from reset reads 1 + 7 (t + 1)
        assert out["sensors"].shape == (8, 12) and (out["sensors"] == 1 + 7 * (last + 1)).all()
        assert out["flags"].shape == (8,) and (out["flags"] == 0).all()
        assert out["episode_sensors"].shape == (8, 200, 12) and (out["episode_sensors"] == 1 + 7 * (np.arange(200)[None, :, None] + 1)).all()


def test_full_adds_the_other_measurements():
    res, work = _bench("--steps", "20", "--warmup", "3", "--full")
    assert work["batches"] == 2 and work["profile_on"] > 0 and work["oracle_step_many"] > 0, work    # the passes really ran
    assert res["full"] and res["config"]["steps_timed"] == 20 and all(k in res for k in HEADLINE)
    assert "ms_per_step_with_hip_events" in res and "launches_timed" in res["config"] and "avg_kernel_ms" in res["roofline"]
    assert res["config"]["fix_only_variant"]["value"] > 0 and res["cpu_baseline"]["value"] > 0 and res["cpu_baseline"]["kind"] == "port"
    res, work = _bench("--steps", "20", "--warmup", "3", "--full", "--no-cpu-baseline", "--no-fix-variant", "--no-event-pass")
    assert work["batches"] == 1 and work["profile_on"] == 0 and work["oracle_step_many"] == 0, work
    assert "roofline" in res and "cpu_baseline" not in res and "fix_only_variant" not in res["config"]
