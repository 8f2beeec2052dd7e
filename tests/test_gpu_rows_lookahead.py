"""The look-ahead of the solver's contact pass (soft-grip_amd/csrc/sg_rows.hip: rows loaded one slot ahead,
nothing requested past the end of a wavefront's longest stream) changes WHEN memory is read, never what is computed.  So the runs below --
chosen for the stream lengths and lane patterns the look-ahead's index rule has to get right -- must give the SAME BITS as the solver
before the look-ahead was reworked: sensors, flags and (ncon, nefc, sweeps) of every env and step against tests/golden/rows_lookahead_parent.npz,
recorded once on the GPU from a library built at the parent commit (RUNS below: `python tests/test_gpu_rows_lookahead.py record <out.npz>`
under SOFTGRIP_LIB=<that library>).  To stay under 100 KB the fixture holds what the parent's runs do not repeat: an env's bits do not
depend on its place in the batch (tests/test_gpu_parity.py::test_full_size_properties), and in the parent's record the 1- and 5-env runs
ARE the first envs of the 9-env run and the masked run IS the 9-env run's first eight envs up to its masked reset, bit for bit (the
recorder asserts it) -- so those are compared against the 9-env run's rows, and only the masked run's events from the reset on are stored.
And the runs must stay within the suite's 1e-7 of the oracle (tests/test_gpu_parity.py: free-running where
the system allows it; the default box model amplifies round-off from first contact on, so from FREE_RUN_STEPS the batch is re-seated on the
oracle's state after every env step and the bound is on what one env step adds).

  softbox n = 1, 5, 9, env steps 0 .. 70   first contact near step 40; the streams then grow through odd and even lengths (the half trip at an
                                           odd nsmax; nsmax = 0, 1, 2); 5 and 9 envs leave a ragged last wavefront of four
  softbox_fix n = 9, 4 and 8 envs per wavefront   the fix-rows-only instantiations; 8 through sg_set_solver_envs_per_wavefront
  softcylinder n = 5, 10 env steps         contacts from reset on, all 30 sweeps sweep contacts, step factors streamed from memory (NB = 2)
  softbox n = 8, masked reset of envs 1 and 6 during the squeeze   every wavefront holds lanes without a pending env
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "rows_lookahead_parent.npz")
KS = [700.0, 903.6948543200572, 300.0, 1400.0, 512.25, 350.0, 1000.0, 1250.0, 640.0]
JOINT_IDS, TENDON_IDS = list(range(11, 64)), [0]
STEPS = 71            # env steps 0 .. 70
FREE_RUN_STEPS = 47   # (tests/test_gpu_parity.py)
MASK_STEP = 55        # the masked reset comes before this env step: seven steps into the squeeze's contacts
TOL_SENSOR = 1e-7
# name: (scene, envs, env steps, envs per solver wavefront to force | None, masked reset, implicit tendon damper)
RUNS = {
    "softbox_n1": ("softbox", 1, STEPS, None, False, None),
    "softbox_n5": ("softbox", 5, STEPS, None, False, None),
    "softbox_n9": ("softbox", 9, STEPS, None, False, None),
    "softbox_fix_n9_epw4": ("softbox_fix", 9, STEPS, 4, False, None),
    "softbox_fix_n9_epw8": ("softbox_fix", 9, STEPS, 8, False, None),
    "softcylinder_n5": ("softcylinder", 5, 10, None, False, "implicit"),
    "softbox_n8_masked": ("softbox", 8, STEPS, None, True, None),
}


def _schedule(steps):
    from softgrip_amd.create_dataset import episode_schedule
    return episode_schedule()[:steps]


def _gpu_run(name, reseat=None):
    """the run `name` on the GPU: per env step (and for the reset, and for a masked reset) the sensor block, the flags and the solver's
    counts.  reseat: None = free-running; else a function (label, batch) called after every recorded event that may put the batch on a
    reference state; it gets the event's sensor rows too."""
    import torch
    import softgrip_amd as sg
    from softgrip_amd import native
    scene, n, steps, epw, masked, damper = RUNS[name]
    m = sg.load_model(os.path.join(ROOT, "models", scene + ".sgmodel"), damper)
    b = native.NativeBatch(native.NativeModel(m), n, 0)
    b.set_stiffness(np.asarray(KS[:n]), JOINT_IDS, TENDON_IDS)
    if epw is not None:
        b.set_solver_envs_per_wavefront(epw)
        assert b.solver_envs_per_wavefront() == epw
    sens = torch.zeros(n, 12, dtype=torch.float64, device=b.device)
    flags = torch.zeros(n, dtype=torch.int32, device=b.device)
    rows_s, rows_f, rows_c = [], [], []

    def record(label):
        st = b.solver_stats()
        rows_s.append(sens.cpu().numpy().copy())
        rows_f.append(flags.cpu().numpy().copy())
        rows_c.append(np.stack([st["ncon"].cpu().numpy(), st["nefc"].cpu().numpy(), st["iters"].cpu().numpy()], 1))
        if reseat is not None:
            assert int(rows_f[-1].sum()) == 0, label
            reseat(label, b, rows_s[-1])

    b.reset(1, sens=sens, flags=flags)
    record(("reset", None))
    for t, c in enumerate(_schedule(steps)):
        if c is not None:
            b.set_ctrl_broadcast(np.array([c, c]))
        if masked and t == MASK_STEP:
            mask = torch.zeros(n, dtype=torch.uint8, device=b.device)
            mask[[1, 6]] = 1
            b.reset(1, sens=sens, flags=flags, mask=mask)
            record(("masked_reset", t))
        b.step(7, sens=sens, flags=flags)
        record(("step", t))
    return m, np.stack(rows_s), np.stack(rows_f), np.stack(rows_c)


_ORACLE = {}


def _oracle(scene, damper, steps):
    """the oracle's run of the nine envs of KS, computed once per scene and shared: per event "reset", 0, 1, ... the sensor rows, the counts
    and the state"""
    key = (scene, damper)
    if key not in _ORACLE:
        import softgrip_amd as sg
        from oracle import oracle as O
        m = sg.load_model(os.path.join(ROOT, "models", scene + ".sgmodel"), damper)
        om = O.OracleModel(m.to_blob())
        n = 5 if scene == "softcylinder" else len(KS)
        sims = [O.OracleSim(om) for _ in range(n)]
        for s, k in zip(sims, KS):
            s.jnt_stiffness[JOINT_IDS] = k
            s.tendon_stiffness[TENDON_IDS] = k
            s.reset(); s.forward(); s.step()
        snap = lambda: dict(sens=np.stack([s.sensordata for s in sims]), counts=np.array([(s.ncon, s.nefc, s.solver_iter) for s in sims]),  # noqa: E731
                            qpos=np.stack([s.qpos for s in sims]), qvel=np.stack([s.qvel for s in sims]), act=np.stack([s.act for s in sims]),
                            warm=np.stack([s.qacc_warmstart for s in sims]))
        out = {"reset": snap(), "om": om, "model": m}
        for t, c in enumerate(_schedule(steps)):
            if c is not None:
                for s in sims:
                    s.ctrl[:] = c
            assert O.step_many(om, sims, 7, min(n, os.cpu_count() or 1)) == 0, t
            out[t] = snap()
        _ORACLE[key] = out
    return _ORACLE[key]


def _golden_rows(golden, name, what):
    scene, n, steps, epw, masked, damper = RUNS[name]
    if name in ("softbox_n1", "softbox_n5"):
        return golden["softbox_n9." + what][:, :n]
    if masked:     # events: the reset, steps 0 .. MASK_STEP - 1 | the masked reset, steps MASK_STEP ..
        return np.concatenate([golden["softbox_n9." + what][:MASK_STEP + 1, :n], golden[name + "." + what]])
    return golden[name + "." + what]


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(RUNS))
def test_same_bits_as_before_the_look_ahead_and_oracle_parity(name, golden):
    import torch
    from oracle import oracle as O
    scene, n, steps, epw, masked, damper = RUNS[name]
    # ---- (1) free-running: the bits of the parent commit's solver
    m, sens, flags, counts = _gpu_run(name)
    assert int(np.abs(flags).sum()) == 0
    for what, got in (("sens", sens), ("flags", flags), ("counts", counts)):
        want = np.ascontiguousarray(_golden_rows(golden, name, what))
        assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
        same = got.view(np.uint8).reshape(got.shape[0], -1) == want.view(np.uint8).reshape(want.shape[0], -1)
        assert same.all(), "%s: %s differs from the parent commit's bits, first at event %d" % (name, what, int(np.flatnonzero(~same.all(1))[0]))
    if not scene.endswith("_fix") and scene != "softcylinder":
        assert counts[:, :, 0].max() >= 3 and (counts[:, :, 0] == 0).any(), "the run must go from no contact through short streams"
    # ---- (2) against the oracle
    ref = _oracle(scene, damper, steps)
    reseat_from = FREE_RUN_STEPS if scene == "softbox" else steps     # *_fix and the cylinder's first steps: free-running throughout
    fresh = {}    # masked run: the oracle's restarted envs
    worst = [0.0]

    def check(label, b, got_s):
        kind, t = label
        st = b.solver_stats()
        got_c = np.stack([st["ncon"].cpu().numpy(), st["nefc"].cpu().numpy(), st["iters"].cpu().numpy()], 1)
        if kind == "masked_reset":
            for e in (1, 6):
                s = O.OracleSim(ref["om"])
                s.jnt_stiffness[JOINT_IDS] = KS[e]
                s.tendon_stiffness[TENDON_IDS] = KS[e]
                s.reset(); s.forward(); s.step()
                fresh[e] = s
                worst[0] = max(worst[0], np.abs(got_s[e] - s.sensordata).max())
            return
        r = ref["reset"] if kind == "reset" else ref[t]
        want_s, want_c = r["sens"][:n].copy(), r["counts"][:n].copy()
        for e, s in fresh.items():      # restarted envs run on by themselves (idle phase of a new episode under the squeeze's ctrl)
            for _ in range(7):
                assert s.step() == 0
            want_s[e], want_c[e] = s.sensordata, (s.ncon, s.nefc, s.solver_iter)
        if kind == "step":
            assert np.array_equal(got_c, want_c), (name, label, got_c.tolist(), want_c.tolist())
        worst[0] = max(worst[0], np.abs(got_s - want_s).max())
        assert worst[0] < TOL_SENSOR, (name, label, worst[0])
        if kind == "step" and t >= reseat_from:
            T = lambda a: torch.tensor(a, dtype=torch.float64, device=b.device).contiguous()  # noqa: E731
            q, v, a, w = r["qpos"][:n].copy(), r["qvel"][:n].copy(), r["act"][:n].copy(), r["warm"][:n].copy()
            for e, s in fresh.items():
                q[e], v[e], a[e], w[e] = s.qpos, s.qvel, s.act, s.qacc_warmstart
            b.set_state(qpos=T(q), qvel=T(v), act=T(a), qacc_warmstart=T(w))

    # (masked run: the restarted envs' ctrl is zero after their reset, like a fresh oracle sim's, and nothing sets ctrl again before step 80)
    _gpu_run(name, reseat=check)
    assert worst[0] < TOL_SENSOR
    print("%s: same bits as the parent commit over %d events; worst |sensor - oracle| %.2e" % (name, sens.shape[0], worst[0]))


if __name__ == "__main__":   # record <out.npz>: the fixture, from whatever library SOFTGRIP_LIB names
    sys.path.insert(0, ROOT)
    assert sys.argv[1] == "record"
    full, out = {}, {}
    for name in RUNS:
        _, sn, f, c = _gpu_run(name)
        full[name + ".sens"], full[name + ".flags"], full[name + ".counts"] = sn, f, c.astype(np.int32)
        print(name, sn.shape, "ncon max", int(c[:, :, 0].max()), "flags", int(np.abs(f).sum()))
    for k, a in full.items():
        name, what = k.split(".")
        n9 = full["softbox_n9." + what]
        if name in ("softbox_n1", "softbox_n5"):
            assert a.tobytes() == np.ascontiguousarray(n9[:, :a.shape[1]]).tobytes(), k
            continue
        if name == "softbox_n8_masked":
            assert a[:MASK_STEP + 1].tobytes() == np.ascontiguousarray(n9[:MASK_STEP + 1, :8]).tobytes(), k
            a = a[MASK_STEP + 1:]
        out[k] = np.ascontiguousarray(a)
    np.savez_compressed(sys.argv[2], **out)
    print("wrote", sys.argv[2], os.path.getsize(sys.argv[2]), "bytes")
