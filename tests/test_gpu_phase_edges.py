"""The phase kernel's batched loads and its LDS gather at the shapes where they can go wrong, on the rows pipeline against the oracle on
identical inputs (comparison and tolerances of test_gpu_parity.py::test_episode_matches_oracle: sensors 1e-7 abs; ncon, nefc, sweeps and
touch bits exactly).

The kernel issues every load of a stage as ONE batch of unconditional loads -- a lane without an element reads element N - 1's words and
drops them -- reads m + armature, its inverse and the neighbour rows' summed weights from fields the host derives (sg_rows_elem_table), and
gathers the neighbour rows' warm-start forces from LDS where its block has room for them (one and two element rounds), from the work
space otherwise.  Covered:
  * 1 and 5 envs: a batch smaller than one solver wavefront (4 envs) and one that does not fill its last;
  * softbox: 110 elements -- the second element round has 46 live lanes, and there are elements without an incoming neighbour row (-1);
  * softcylinder: 192 elements, three full rounds; the LDS gather is compiled out there and the work-space path must still be right;
  * the first 50 env steps from reset: idle steps, in which the warm start loses and the slider accelerations are recomputed a second
    time from zeroed forces, then the closing fingers (first contact of the box at ~45; the cylinder touches them from the first step);
  * a masked reset in the middle (before step 25) that leaves one env out: env 2 of 5 runs on while the others restart, the only env of
    a batch of 1 runs on untouched.
Free-running for the first 20 steps, then -- as in the parity test, the neighbour-row squeeze amplifies round-off -- re-seated on the
oracle's state after every env step: what is bounded is the error the kernels add in one env step (7 substeps)."""
import os

import numpy as np
import pytest

import softgrip_amd as sg
from helpers import JOINT_IDS, TENDON_IDS, library_for, model_path
from softgrip_amd.create_dataset import episode_schedule
from test_gpu_parity import TOL_SENSOR, _bufs, _expected_touch, _touch_bit_of_geom

pytestmark = pytest.mark.gpu

STEPS = 50
FREE_RUN = 20
RESET_AT = 25
KS = [700.0, 903.6948543200572, 300.0, 1400.0, 512.25]


@pytest.mark.parametrize("scene,damper", [("softbox", None), ("softcylinder", "implicit")])
@pytest.mark.parametrize("n", [1, 5])
def test_first_steps_and_masked_reset_match_oracle(scene, damper, n):
    import torch
    from oracle import oracle as O
    from softgrip_amd import native
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    ks = KS[:n]
    m = sg.load_model(model_path(scene), damper)
    nm = native.NativeModel(m, library_for("rows"))
    b = native.NativeBatch(nm, n, 0)
    b.set_pipeline("rows")
    b.set_stiffness(np.asarray(ks, dtype=np.float64), JOINT_IDS, TENDON_IDS)
    sens, flags, touch = _bufs(b, n)
    om = O.OracleModel(m.to_blob())
    sims = [O.OracleSim(om) for _ in ks]
    threads = min(n, os.cpu_count() or 1)

    def oracle_reset(s):
        s.reset(); s.forward(); s.step()

    for s, k in zip(sims, ks):
        s._om = om
        s.jnt_stiffness[JOINT_IDS] = k
        s.tendon_stiffness[TENDON_IDS] = k
        oracle_reset(s)
    b.reset(1, sens=sens, flags=flags, touch=touch)
    np.testing.assert_allclose(sens.cpu().numpy(), np.stack([s.sensordata for s in sims]), atol=1e-12)
    bit_of = _touch_bit_of_geom(m)
    ctrl = np.zeros(2)
    keep = 2 if n > 2 else 0               # the env the masked reset leaves out
    worst, contacts_seen = 0.0, 0
    T = lambda a: torch.tensor(np.stack(a), dtype=torch.float64, device=b.device).contiguous()  # noqa: E731
    for t, c in enumerate(episode_schedule()[:STEPS]):
        if c is not None:
            ctrl[:] = c
            b.set_ctrl_broadcast(ctrl)
            for s in sims:
                s.ctrl[:] = c
        if t == RESET_AT:
            before = sens.cpu().numpy().copy()
            mask = torch.ones(n, dtype=torch.uint8, device=b.device)
            mask[keep] = 0
            b.reset(1, sens=sens, flags=flags, touch=touch, mask=mask)
            for e, s in enumerate(sims):
                if e != keep:
                    oracle_reset(s)
            got = sens.cpu().numpy()
            for e, s in enumerate(sims):    # the selected envs: the reset state's sensors; the env left out: its row untouched
                np.testing.assert_allclose(got[e], s.sensordata if e != keep else before[e], atol=1e-12 if e != keep else 0.0)
            b.set_ctrl_broadcast(ctrl)      # (a reset zeroes the selected envs' ctrl: every env goes on under the schedule's)
            for s in sims:
                s.ctrl[:] = ctrl
        b.step(7, sens=sens, flags=flags, touch=touch)
        assert O.step_many(om, sims, 7, threads) == 0, t
        got = sens.cpu().numpy()
        want_s = np.stack([s.sensordata for s in sims])
        st = b.solver_stats()
        counts = list(zip(st["ncon"].cpu().tolist(), st["nefc"].cpu().tolist(), st["iters"].cpu().tolist()))
        assert counts == [(s.ncon, s.nefc, s.solver_iter) for s in sims], (t, counts)
        worst = max(worst, float(np.abs(got - want_s).max()))
        assert worst < TOL_SENSOR, (t, worst)
        assert int(flags.abs().sum()) == 0, t
        assert touch.cpu().tolist() == [_expected_touch(m, s.contacts(), bit_of) for s in sims], t
        contacts_seen = max(contacts_seen, sims[keep].ncon)
        if t >= FREE_RUN:
            gs = b.get_state()
            for e, s in enumerate(sims):
                np.testing.assert_allclose(gs["qpos"][e].cpu().numpy(), s.qpos, atol=1e-9)
                np.testing.assert_allclose(gs["qvel"][e].cpu().numpy(), s.qvel, atol=1e-7)
            b.set_state(qpos=T([s.qpos for s in sims]), qvel=T([s.qvel for s in sims]), act=T([s.act for s in sims]),
                        qacc_warmstart=T([s.qacc_warmstart for s in sims]))
    assert contacts_seen > 0               # the env that ran the whole 50 steps did reach first contact
