"""The solver of a neighbour-row model takes its equality rows READY from the phase kernel (soft-grip_amd/csrc/sg_rows_layout.h: sg_eq_fix_index,
sg_eq_nb_index -- per row the state g = b + R f and the step factor c, element-major) and stages them, the slider words, the table and the
per-stream values in one batch of unconditional loads (sg_rows.hip: the prologue).  The runs below are chosen for what that staging has to
get right, each against the CPU oracle at tests/test_gpu_parity.py's tolerances -- qpos 1e-9, qvel 1e-7, ncon and sweeps equal:

  softbox n = 6, 7, env steps 0 .. 47     2 and 3 envs in the last wavefront of four (the other env slots read clamped addresses); contacts from step 40
  softcylinder n = 5, 6 env steps          192 elements = 3 * 64: the rows end on a trip boundary of the records; step factors streamed (NB = 2)
  softball n = 5, 6 env steps              218 elements, four element rounds in the phase kernel
  softbox n = 8, masked reset              after 44 env steps envs 1, 2 and 6 are reset by mask: a solver launch whose wavefronts hold pending and
                                           non-pending envs, the latter's rows stale.  The untouched envs' state is bit-equal across the reset
                                           call, and all eight match the oracle over four more env steps
  softbox n = 8, masked reset of env 5     the same with ONE env picked: the wavefront of envs 0 .. 3 then has no pending env at all -- it is staged
                                           like the others, has no running lane and must store nothing
  softbox n = 5, garbage warm start        a state whose qacc_warmstart is seeded noise of magnitude ~1e3, so that the warm start loses and the
                                           rows' states fall back to b; compared one and three env steps later

The oracle's runs are computed once per scene and shared."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = [700.0, 903.6948543200572, 300.0, 1400.0, 512.25, 350.0, 1000.0, 1250.0]
JOINT_IDS, TENDON_IDS = list(range(11, 64)), [0]
TOL_QPOS, TOL_QVEL = 1e-9, 1e-7     # tests/test_gpu_parity.py
DAMPER = {"softbox": None, "softcylinder": "implicit", "softball": "implicit"}


def _schedule(steps):
    from softgrip_amd.create_dataset import episode_schedule
    return episode_schedule()[:steps]


def _model(scene):
    import softgrip_amd as sg
    return sg.load_model(os.path.join(ROOT, "models", scene + ".sgmodel"), DAMPER[scene])


def _fresh_sim(om, k):
    from oracle import oracle as O
    s = O.OracleSim(om)
    s.jnt_stiffness[JOINT_IDS] = k
    s.tendon_stiffness[TENDON_IDS] = k
    s.reset(); s.forward(); s.step()
    return s


def _snap(sims):
    return dict(qpos=np.stack([s.qpos for s in sims]), qvel=np.stack([s.qvel for s in sims]), act=np.stack([s.act for s in sims]),
                warm=np.stack([s.qacc_warmstart for s in sims]), counts=np.array([(s.ncon, s.solver_iter) for s in sims]))


_ORACLE = {}


def _oracle(scene, n, steps):
    """the oracle's run of the first n envs of KS over `steps` env steps of the schedule: per event "reset", 0, 1, ... the state and the
    counts; computed once per scene (at the largest n and step count any test asks for: callers slice) and not changed afterwards"""
    if scene not in _ORACLE:
        from oracle import oracle as O
        full_n, full_steps = {"softbox": (8, 48), "softcylinder": (5, 6), "softball": (5, 6)}[scene]
        m = _model(scene)
        om = O.OracleModel(m.to_blob())
        sims = [_fresh_sim(om, k) for k in KS[:full_n]]
        out = {"om": om, "reset": _snap(sims)}
        for t, c in enumerate(_schedule(full_steps)):
            if c is not None:
                for s in sims:
                    s.ctrl[:] = c
            assert O.step_many(om, sims, 7, min(full_n, os.cpu_count() or 1)) == 0, t
            out[t] = _snap(sims)
        _ORACLE[scene] = out
    assert n <= _ORACLE[scene]["reset"]["qpos"].shape[0] and steps - 1 in _ORACLE[scene]
    return _ORACLE[scene]


def _batch(scene, n):
    import torch
    from softgrip_amd import native
    m = _model(scene)
    b = native.NativeBatch(native.NativeModel(m), n, 0)
    b.set_stiffness(np.asarray(KS[:n]), JOINT_IDS, TENDON_IDS)
    sens = torch.zeros(n, 12, dtype=torch.float64, device=b.device)
    flags = torch.zeros(n, dtype=torch.int32, device=b.device)
    return b, sens, flags


def _compare(label, b, flags, want, rows=None):
    """the batch's state and counts against an oracle snapshot (rows: which of its envs, default the first b.n); returns the deviations"""
    st, ss = b.get_state(), b.solver_stats()
    rows = list(range(b.n)) if rows is None else rows
    dq = float(np.abs(st["qpos"].cpu().numpy() - want["qpos"][rows]).max())
    dv = float(np.abs(st["qvel"].cpu().numpy() - want["qvel"][rows]).max())
    got_c = np.stack([ss["ncon"].cpu().numpy(), ss["iters"].cpu().numpy()], 1)
    print("%s: |qpos - oracle| %.2e  |qvel - oracle| %.2e  ncon max %d" % (label, dq, dv, int(got_c[:, 0].max())))
    assert int(flags.abs().sum()) == 0, label
    assert np.array_equal(got_c, want["counts"][rows]), (label, got_c.tolist(), want["counts"][rows].tolist())
    assert dq < TOL_QPOS and dv < TOL_QVEL, (label, dq, dv)
    return dq, dv


def _run(scene, n, steps):
    ref = _oracle(scene, n, steps)
    b, sens, flags = _batch(scene, n)
    b.reset(1, sens=sens, flags=flags)
    _compare("%s n %d reset" % (scene, n), b, flags, ref["reset"])
    ncon = 0
    for t, c in enumerate(_schedule(steps)):
        if c is not None:
            b.set_ctrl_broadcast(np.array([c, c]))
        b.step(7, sens=sens, flags=flags)
        _compare("%s n %d step %d" % (scene, n, t), b, flags, ref[t])
        ncon = max(ncon, int(ref[t]["counts"][:n, 0].max()))
    return ncon


@pytest.mark.gpu
@pytest.mark.parametrize("n", [6, 7])
def test_softbox_ragged_last_wavefront_matches_oracle(n):
    assert _run("softbox", n, 48) >= 1, "the run must reach the squeeze's first contacts"


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["softcylinder", "softball"])
def test_streamed_factor_models_match_oracle(scene):
    from softgrip_amd import native
    assert native.NativeModel(_model(scene)).nelem == {"softcylinder": 192, "softball": 218}[scene]
    assert _run(scene, 5, 6) >= 1, "these scenes are in contact from the reset on"


@pytest.mark.gpu
@pytest.mark.parametrize("picked", [[1, 2, 6], [5]], ids=["envs_1_2_6", "env_5"])
def test_softbox_masked_reset_leaves_the_other_envs_bits_and_matches_oracle(picked):
    import torch
    n, before, after = 8, 44, 4
    ref = _oracle("softbox", n, before + after)
    b, sens, flags = _batch("softbox", n)
    b.reset(1, sens=sens, flags=flags)
    sched = _schedule(before + after)
    for t in range(before):
        if sched[t] is not None:
            b.set_ctrl_broadcast(np.array([sched[t], sched[t]]))
        b.step(7, sens=sens, flags=flags)
    _compare("masked: step %d" % (before - 1), b, flags, ref[before - 1])
    st1 = b.get_state()
    mask = torch.zeros(n, dtype=torch.uint8, device=b.device)
    mask[picked] = 1
    b.reset(1, sens=sens, flags=flags, mask=mask)
    st2 = b.get_state()
    keep = [e for e in range(n) if e not in picked]
    for k in ("qpos", "qvel", "act", "qacc_warmstart", "ctrl"):
        assert torch.equal(st1[k][keep], st2[k][keep]), "%s of an env outside the mask changed across the masked reset" % k
    # the oracle's side: the untouched envs are the shared run's, the picked ones fresh sims (their ctrl is zero after the reset, on both sides)
    from oracle import oracle as O
    assert sched[40] == -0.2 and all(c is None for c in sched[41:before + after])
    fresh = {e: _fresh_sim(ref["om"], KS[e]) for e in picked}
    for e in picked:
        assert np.abs(st2["qpos"][e].cpu().numpy() - fresh[e].qpos).max() < TOL_QPOS and float(st2["ctrl"][e].abs().max()) == 0.0
    for t in range(before, before + after):
        b.step(7, sens=sens, flags=flags)
        assert O.step_many(ref["om"], list(fresh.values()), 7, len(picked)) == 0
        want = {k: v[:n].copy() for k, v in ref[t].items()}
        for e, s in fresh.items():
            for k, v in _snap([s]).items():
                want[k][e] = v[0]
        _compare("masked: step %d" % t, b, flags, want)


@pytest.mark.gpu
def test_softbox_garbage_warm_start_loses_and_matches_oracle():
    """The oracle offers no way to ask whether the warm start lost (it keeps no such flag); that it does is by construction: the noise is ~1e3
    times the accelerations of the state, so the warm-started forces' cost is far above zero, which is the test both sides apply."""
    import torch
    from oracle import oracle as O
    n = 5
    ref = _oracle("softbox", n, 2)
    b, sens, flags = _batch("softbox", n)
    b.reset(1, sens=sens, flags=flags)
    om = ref["om"]
    sims = [_fresh_sim(om, k) for k in KS[:n]]
    st = b.get_state()
    warm = np.random.RandomState(7).uniform(-1.0, 1.0, st["qacc_warmstart"].shape) * 1e3
    assert np.abs(warm).max() > 100 * max(1.0, float(st["qacc_warmstart"].abs().max()))
    b.set_state(qacc_warmstart=torch.tensor(warm, dtype=torch.float64, device=b.device).contiguous())
    for e, s in enumerate(sims):
        s.qacc_warmstart[:] = warm[e]
    for t in range(3):
        b.step(7, sens=sens, flags=flags)
        assert O.step_many(om, sims, 7, min(n, os.cpu_count() or 1)) == 0
        if t in (0, 2):
            _compare("garbage warm start: %d env steps later" % (t + 1), b, flags, _snap(sims))
