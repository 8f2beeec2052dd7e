"""sg_get_velocities / sg_get_tendons / sg_get_energy on the GPU: the three entry points against the NumPy reference (tests/dyn_ref.py,
itself pinned to the oracle by tests/test_dyn_host.py) and straight against the oracle, over a sweep of random grippers far out of
their joint ranges (with sg_get_poses) and at the body limit, the calls' interface (env lists, NULL outputs, NaN
envs, determinism, no side effect, stream ordering against sg_set_stiffness) and ManEnv.rollout(energy_out=...)."""
import ctypes as C
import itertools

import numpy as np
import pytest

import dyn_ref as DR
from helpers import model_path

pytestmark = pytest.mark.gpu

VEL, TEN = ("ang", "lin", "com_lin"), ("length", "velocity")


def _torch():
    import torch
    return torch


def _batch(scene, ks, pipeline=None):
    from softgrip_amd import native
    m = DR.load(scene)
    _, jids, tids, nu = DR.SCENES[scene]
    nm = native.NativeModel(m)
    b = native.NativeBatch(nm, len(ks), 0)
    if pipeline:
        b.set_pipeline(pipeline)
    b.set_stiffness(np.asarray(ks, dtype=np.float64), jids, tids)
    return m, nm, b


def _squeeze(b, nu, nsteps=6):
    """sg_reset, then nsteps env steps of 7 substeps at ctrl = -0.2; no env may raise a flag"""
    torch = _torch()
    flags = torch.zeros(b.n, dtype=torch.int32, device=b.device)
    b.reset(1, flags=flags)
    assert int(flags.abs().sum()) == 0
    b.set_ctrl_broadcast(np.full(nu, -0.2))
    for _ in range(nsteps):
        b.step(7, flags=flags)
        assert int(flags.abs().sum()) == 0


def _all(b, env_ids=None):
    """the three calls' outputs as one dict of device tensors"""
    out = dict(b.velocities(env_ids))
    out.update(b.tendons(env_ids))
    out["energy"] = b.energy(env_ids)
    return out


def _host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _same_bits(a, b):
    torch = _torch()
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)))


def _against_reference(m, scene, got, qpos, qvel, ks, what, jids=None, tids=None):
    """every env of `got` against the NumPy reference at the bounds of dyn_ref; -> the worst deviation per output, the arrays' in units
    of their bound, the energy terms' relative to their scale.  jids / tids: the listed joints / tendons (None: the scene's)"""
    worst = dict.fromkeys(VEL + TEN + ("energy",), 0.0)
    for e, k in enumerate(ks):
        kj, kt = DR.stiffness(m, scene, k, jids, tids)
        ref = DR.reference(m, qpos[e], qvel[e], kj, kt)
        for name in VEL + TEN:
            dev = DR.close(got[name][e], ref[name])
            worst[name] = max(worst[name], dev)
            assert dev <= 1.0, (what, e, name, dev)
        scale = DR.energy_scale(m, ref, kj, kt, qpos[e], qvel[e], allowance=scene in DR.ALLOW_FIXED_TENDON)
        dev = np.abs(got["energy"][e] - ref["energy"]) / np.maximum(scale, 1e-300)
        plain = DR.energy_scale(m, ref, kj, kt, qpos[e], qvel[e])[2]
        print(what, "env", e, "energy", got["energy"][e], "relative deviation", dev, "tendon term against the plain scale",
              abs(got["energy"][e, 2] - ref["energy"][2]) / max(plain, 1e-300))
        worst["energy"] = max(worst["energy"], float(dev.max()))
        assert (dev <= DR.REL).all(), (what, e, dev)
        assert (got["ang"][e, 0] == 0).all() and (got["lin"][e, 0] == 0).all() and (got["com_lin"][e, 0] == 0).all()
    return worst


@pytest.mark.parametrize("scene,pipeline", [("softbox", None), ("softbox_fix", None), ("softbox_fix", "tree"), ("fourfinger_softball_fix", None),
                                            ("freeball_fix", None)])
def test_entry_points_match_the_reference(scene, pipeline):
    """3 envs of distinct stiffness, sg_reset and 6 env steps of a squeeze on the device, the state read back with sg_get_state: every
    output of the three calls against the NumPy reference at that state -- 1e-12 max(1, max |value|) per array, the energy terms 1e-11
    relative to the sum of the absolute values of their summands (dyn_ref.energy_scale).
    fourfinger_softball_fix alone takes energy_scale's allowance on the tendon-spring term (REL k |x| sum |coef q| on fixed tendons):
    its volume tendon's length is a cancelling sum of 218 terms that comes to ~1e-20 m, the term to 1e-36 .. 1e-35 J, and the kernel's
    lane-strided sum deviates from NumPy's by 3.7, 1.0 and 0.62 of the term in the three envs (measured on the MI355X); with the
    allowance the deviation is 1e-17 .. 6e-17 of the scale.  The other scenes meet the plain bound: measured <= 1.8e-14 of sum 1/2 k x^2"""
    m, nm, b = _batch(scene, DR.KS, pipeline)
    _squeeze(b, DR.SCENES[scene][3])
    st = b.get_state()
    qpos, qvel = st["qpos"].cpu().numpy(), st["qvel"].cpu().numpy()
    assert np.abs(qvel).max() > 1e-3, "the state must move"
    _against_reference(m, scene, _host(_all(b)), qpos, qvel, DR.KS, "%s/%s" % (scene, pipeline or "default"))


@pytest.mark.parametrize("scene", ["softbox_fix", "fourfinger_softball_fix", "freeball_fix"])
def test_entry_points_match_the_oracle(scene):
    """the oracle's states (dyn_ref.states) put into the batch with sg_set_state: the kinetic term against 1/2 qvel' qM qvel, ang against
    the oracle's gyro channels, length against sgo_ten_length -- each within 1e-11 of the sum of the absolute values of its terms"""
    from oracle import oracle as O
    torch = _torch()
    m, om, sts = DR.states(scene)
    _, nm, b = _batch(scene, [s["k"] for s in sts])
    T = lambda a: torch.tensor(np.stack(a), dtype=torch.float64, device=b.device).contiguous()  # noqa: E731
    b.set_state(qpos=T([s["qpos"] for s in sts]), qvel=T([s["qvel"] for s in sts]))
    got = _host(_all(b))
    sim = O.OracleSim(om)
    for e, st in enumerate(sts):
        kj, kt = DR.stiffness(m, scene, st["k"])
        DR.oracle_forward(sim, st["qpos"], st["qvel"], kj, kt)
        ke = 0.5 * st["qvel"] @ sim.qM @ st["qvel"]
        assert abs(got["energy"][e, 3] - ke) <= DR.REL * ke, (e, got["energy"][e, 3], ke)
        kin = m.kinematics(st["qpos"])
        cols = DR.dof_columns(m, kin)
        mv = DR.moved_by(m, cols[3])
        for adr, site in DR.gyro_channels(m):
            body = m.site_bodyid[site]
            scale = max(float(np.sum(np.abs(st["qvel"]) * cols[0] * mv[body])), 1e-300)
            gyro = DR.site_xmat(m, kin, site).T @ got["ang"][e, body]
            assert np.abs(gyro - sim.sensordata[adr:adr + 3]).max() <= DR.REL * scale, (e, site)
        for t in range(m.ntendon):
            scale = DR.length_scale(m, t, st["qpos"], sim.ten_length)
            assert abs(got["length"][e, t] - sim.ten_length[t]) <= DR.REL * scale, (e, t)


# ---- the sweep of dyn_ref: random grippers far out of their joint ranges, one env per state, nothing stepped ----
def _state_batch(m, qpos, qvel, ks, jids, tids):
    """a batch with one env per state: one sg_set_state(qpos, qvel), one sg_set_stiffness"""
    from softgrip_amd import native
    torch = _torch()
    b = native.NativeBatch(native.NativeModel(m), len(ks), 0)
    T = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=b.device)  # noqa: E731
    b.set_state(qpos=T(qpos), qvel=T(qvel))
    b.set_stiffness(np.asarray(ks, dtype=np.float64), jids, tids)
    return b


def _against_kinematics(m, p, qpos, what):
    """poses() of every env against Model.kinematics() / render_ref.geom_poses at tests/test_gpu_render.py's 1e-12 -> worst deviation"""
    import render_ref as R
    worst = 0.0
    for e, q in enumerate(qpos):
        kin = m.kinematics(q)
        gx, gm = R.geom_poses(m, q)
        for name, want in (("xpos", kin["xpos"]), ("xquat", kin["xquat"]), ("geom_xpos", gx), ("geom_xmat", np.reshape(gm, (-1, 9)))):
            dev = float(np.abs(p[name][e] - want).max())
            worst = max(worst, dev)
            assert dev < 1e-12, (what, e, name, dev)
    return worst


@pytest.mark.parametrize("gripper,offset", DR.SWEEP_CASES)
def test_sweep_of_random_grippers_matches_the_reference(gripper, offset, tmp_path):
    """64 states of a random gripper (dyn_ref.sweep: contacts_ref's grippers and poses, links turned up to 3 rad about up to three
    hinges per body, sliders moved, every second gripper's shell on a free joint -- every fourth of its states with the free
    quaternion scaled by 1.7 -- qvel of scale 0, 1 and 30, a stiffness per env) as 64 envs of one batch: one sg_set_state, one
    sg_set_stiffness, then poses(), velocities(), tendons() and energy() once each.  Poses against Model.kinematics() at 1e-12; the
    rest against the NumPy reference at 1e-12 max(1, max |value|) per array and 1e-11 of the PLAIN scale per energy term.  No state is
    left out.  The seventh case is gripper 3 with every hinge's anchor moved off its body's origin (dyn_ref.offset_anchors): the
    generator leaves all joints at the origin, where it does not matter in which frame a body's second hinge takes its anchor.
    What the states reach is asserted on the CPU by tests/test_dyn_host.py's test of the same name.
    sg_set_state neither refuses nor normalises a free quaternion off unit length: it stores qpos as given (sg_get_state returns the
    same bits) and every read-out normalises on the way, as Model.kinematics() does.
    Measured on the MI355X, worst over the cases: poses 1.0e-15; in units of the arrays' bound ang 9.3e-4, lin 8.7e-4,
    com_lin 9.9e-4, length 4.9e-4, velocity 3.4e-3; energy terms 2.0e-13 of their scale"""
    import contacts_ref as CR
    assert len(DR.SWEEP_CASES) == CR.SWEEP_GRIPPERS + 1
    m, qpos, qvel, ks, jids, tids = DR.sweep(gripper, tmp_path, offset)
    b = _state_batch(m, qpos, qvel, ks, jids, tids)
    p = {k: v.cpu().numpy() for k, v in b.poses().items()}
    got = _host(_all(b))
    st = b.get_state()
    assert st["qpos"].cpu().numpy().tobytes() == np.ascontiguousarray(qpos).tobytes()      # stored as given, non-unit quaternions too
    free = [int(m.jnt_qposadr[j]) for j in range(m.njnt) if m.jnt_type[j] == 0]
    assert bool(free) == bool(gripper % 2)
    for a in free:
        assert abs(np.linalg.norm(qpos[0, a + 3:a + 7]) - DR.SWEEP_QUAT_SCALE) < 1e-12
    what = "gripper %d%s" % (gripper, " with offset anchors" if offset else "")
    wp = _against_kinematics(m, p, qpos, what)
    worst = _against_reference(m, None, got, qpos, qvel, ks, what, jids, tids)
    for e in range(len(ks)):
        if not qvel[e].any():      # at rest: every velocity output is exactly zero
            assert not any(got[name][e].any() for name in VEL + ("velocity",)) and got["energy"][e, 3] == 0.0, e
    print("%s: %d bodies, %d states, poses off by at most %.2e; arrays in units of their bound, energy relative: %s"
          % (what, m.nbody, len(ks), wp, {k: "%.2e" % v for k, v in worst.items()}))
    assert len(ks) == CR.SWEEP_POSES == 64


# ---- the body limit (SGD_MAXBODY, csrc/sg_dyn.h) on the device ----
MAXBODY = 627
PAD_GRIPPER = 1      # a gripper of the sweep on a free joint


def _padded(tmp_path, nbody):
    """the sweep's gripper PAD_GRIPPER with jointless child bodies of its static body, each with one sphere of 1 cm that collides with
    nothing, up to nbody bodies: one wide level of the kernels' depth schedule"""
    import softgrip_amd as sg
    import contacts_ref as CR
    xml = CR.sweep_gripper_xmls()[PAD_GRIPPER]
    base = DR.sweep(PAD_GRIPPER, tmp_path)[0]
    roof = '<geom class="link" name="roof"'
    assert xml.count(roof) == 1
    extra = "".join('<body pos="%.2f %.2f 1.6"><geom type="sphere" size="0.01" contype="0" conaffinity="0" mass="1e-6"/></body>\n'
                    % (0.3 + 0.05 * (k % 37), -0.9 + 0.05 * (k // 37)) for k in range(nbody - base.nbody))
    path = tmp_path / ("padded_%d.xml" % nbody)
    path.write_text(xml.replace(roof, extra + roof))
    m = sg.compile_mjcf(str(path), composite_neighbors=False)
    assert m.nbody == nbody, (m.nbody, nbody)
    return m


def _padded_states(m, tmp_path):
    """two states of a padded model: a swept pose of the unpadded gripper's sweep and the rest pose, qvel of scale 1.  The padding adds
    no joint, so the unpadded gripper's qpos and qvel fit"""
    base, qpos, qvel = DR.sweep(PAD_GRIPPER, tmp_path)[:3]
    assert m.nq == base.nq and m.nv == base.nv
    q = np.stack([qpos[4], np.array(m.qpos0, dtype=np.float64)])      # (pose 4: hinges swung by up to 1.5 rad, the free quaternion times 1.7)
    v = np.stack([qvel[4], qvel[1]])
    assert abs(np.abs(v[0]).max() - 3) < 3 and abs(np.abs(v[1]).max() - 3) < 3      # (both of scale 1)
    return q, v, DR.KS[:2]


def test_body_limit_is_reached_on_the_device(tmp_path):
    """627 bodies, SGD_MAXBODY: the launch asks for 65 208 B of dynamic LDS beside the kernel's 256 B of static LDS, and the padded
    static body's ~575 children are one level of nine 64-strides (the widest level of a committed scene has four).  Two envs -- a
    swept pose and the rest pose, qvel of scale 1 -- match the reference at the sweep's bounds, and poses() matches
    Model.kinematics().  Measured on the MI355X: 576 children in the widest level, poses 3.3e-16, arrays <= 4.3e-4 of their bound,
    energy terms <= 7.1e-16"""
    m = _padded(tmp_path, MAXBODY)
    jids, tids = DR.sweep_ids(m)
    q, v, ks = _padded_states(m, tmp_path)
    b = _state_batch(m, q, v, ks, jids, tids)
    got = _host(_all(b))
    worst = _against_reference(m, None, got, q, v, ks, "%d bodies" % MAXBODY, jids, tids)
    wp = _against_kinematics(m, {k: x.cpu().numpy() for k, x in b.poses().items()}, q, "%d bodies" % MAXBODY)
    widest = int(np.bincount(np.asarray(m.body_parentid)[1:]).max())
    print("%d bodies, %d of them children of one body: poses off by at most %.2e, %s" % (m.nbody, widest, wp, {k: "%.2e" % x for k, x in worst.items()}))
    assert widest > 8 * 64


def test_one_body_beyond_the_limit_is_refused(tmp_path):
    """628 bodies: each of the three entry points returns SG_ERR_MODEL under its own name with "more than 627 bodies" and writes
    nothing (canary), and poses() of the same batch still answers correctly"""
    from softgrip_amd import native
    from softgrip_amd.native import _ptr
    torch = _torch()
    m = _padded(tmp_path, MAXBODY + 1)
    jids, tids = DR.sweep_ids(m)
    q, v, ks = _padded_states(m, tmp_path)
    b = _state_batch(m, q, v, ks, jids, tids)
    kw = dict(dtype=torch.float64, device=b.device)
    out = {n: torch.full((2, m.nbody, 3), -7.5, **kw) for n in VEL}
    out.update({n: torch.full((2, m.ntendon), -7.5, **kw) for n in TEN})
    out["energy"] = torch.full((2, 4), -7.5, **kw)
    L, s = b.L, b._stream()
    calls = (("sg_get_velocities", lambda: L.sg_get_velocities(b.ptr, None, 2, _ptr(out["ang"]), _ptr(out["lin"]), _ptr(out["com_lin"]), s)),
             ("sg_get_tendons", lambda: L.sg_get_tendons(b.ptr, None, 2, _ptr(out["length"]), _ptr(out["velocity"]), s)),
             ("sg_get_energy", lambda: L.sg_get_energy(b.ptr, None, 2, _ptr(out["energy"]), s)))
    for name, call in calls:
        assert call() == native.SG_ERR_MODEL, name
        msg = L.sg_last_error()
        assert msg.startswith(name.encode() + b":") and b"more than %d bodies" % MAXBODY in msg, (name, msg)
    torch.cuda.synchronize()
    for n, x in out.items():
        assert bool((x == -7.5).all()), n
    _against_kinematics(m, {k: x.cpu().numpy() for k, x in b.poses().items()}, q, "%d bodies" % (MAXBODY + 1))


def _raw(b, ids, n_ids, out):
    """the three entry points with any output left out (None -> NULL)"""
    from softgrip_amd.native import _ptr
    arr = None if ids is None else np.ascontiguousarray(ids, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    L, s = b.L, b._stream()
    b._check(L.sg_get_velocities(b.ptr, arr, n_ids, _ptr(out.get("ang")), _ptr(out.get("lin")), _ptr(out.get("com_lin")), s))
    b._check(L.sg_get_tendons(b.ptr, arr, n_ids, _ptr(out.get("length")), _ptr(out.get("velocity")), s))
    b._check(L.sg_get_energy(b.ptr, arr, n_ids, _ptr(out.get("energy")), s))


def test_listing_and_determinism():
    """env_ids as a subset, a permutation and with a repeated id reproduce the rows of the all-env call bit for bit; two calls give the
    same bits; outputs passed as NULL in any combination leave the others' bits as they are; an env id out of range is refused"""
    from softgrip_amd import native
    torch = _torch()
    ks = np.linspace(300, 1400, 9)
    m, nm, b = _batch("softbox_fix", ks)
    _squeeze(b, 2, nsteps=4)
    full = _all(b)
    again = _all(b)
    for name in full:
        assert _same_bits(full[name], again[name]), name
    for ids in ([4, 1], [8, 3, 0, 6, 2, 7, 1, 5, 4], [2, 2, 5], [7]):
        part = _all(b, ids)
        for name in full:
            assert _same_bits(part[name], full[name][torch.as_tensor(ids, device=b.device)]), (ids, name)
    names = VEL + TEN + ("energy",)
    for group in (VEL, TEN):
        for r in range(1, len(group)):
            for keep in itertools.combinations(group, r):
                out = {n: torch.full_like(full[n], -7.5) for n in keep}
                _raw(b, None, b.n, out)
                for n in keep:
                    assert _same_bits(out[n], full[n]), (keep, n)
    _raw(b, None, b.n, {})      # every output NULL: nothing to write, no error
    out = {n: torch.full_like(full[n], -7.5) for n in names}
    _raw(b, None, b.n, out)
    for n in names:
        assert _same_bits(out[n], full[n]), n
    bad = np.array([0, 9], np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    for fn, args in (("sg_get_velocities", (None, None, None)), ("sg_get_tendons", (None, None)), ("sg_get_energy", (None,))):
        assert getattr(b.L, fn)(b.ptr, bad, 2, *args, None) == native.SG_ERR_INVALID
        assert b.L.sg_last_error().startswith(fn.encode() + b": env id 9 out of range"), b.L.sg_last_error()
        assert getattr(b.L, fn)(b.ptr, None, 3, *args, None) == native.SG_ERR_INVALID      # (NULL ids need n_ids == n_envs)


def test_nan_envs_get_nan_and_disturb_no_other():
    """a NaN planted in env 1's qvel and in env 3's qpos (and an inf in env 4's qvel): NaN everywhere in those envs' rows, unchanged bits
    in the others'"""
    torch = _torch()
    ks = np.linspace(300, 1400, 6)
    m, nm, b = _batch("freeball_fix", ks)
    _squeeze(b, 2, nsteps=3)
    clean = _all(b)
    st = b.get_state()
    st["qvel"][1, 17] = float("nan")
    st["qpos"][3, 5] = float("nan")
    st["qvel"][4, 0] = float("inf")
    b.set_state(qpos=st["qpos"], qvel=st["qvel"])
    got = _all(b)
    for name, x in got.items():
        for e in range(6):
            if e in (1, 3, 4):
                assert bool(torch.isnan(x[e]).all()), (name, e)
            else:
                assert _same_bits(x[e], clean[name][e]), (name, e)


def test_calls_change_nothing():
    """the state is bit-identical before and after the three calls, and a twin batch that made no read-out call produces bit-identical
    sensors, flags and touch from the next sg_step"""
    torch = _torch()
    ks = np.linspace(300, 1400, 5)
    outs = []
    for read in (True, False):
        m, nm, b = _batch("softbox", ks)
        _squeeze(b, 2, nsteps=4)
        if read:
            before = b.get_state()
            _all(b)
            _all(b, [3, 0])
            after = b.get_state()
            for name in before:
                assert _same_bits(before[name], after[name]), name
        sens = torch.zeros(b.n, nm.nsensordata, dtype=torch.float64, device=b.device)
        flags = torch.zeros(b.n, dtype=torch.int32, device=b.device)
        touch = torch.zeros(b.n, dtype=torch.int32, device=b.device)
        b.step(7, sens=sens, flags=flags, touch=touch)
        outs.append((sens, flags, touch, b.get_state()))
    assert _same_bits(outs[0][0], outs[1][0])
    assert torch.equal(outs[0][1], outs[1][1]) and torch.equal(outs[0][2], outs[1][2])
    for name in outs[0][3]:
        assert _same_bits(outs[0][3][name], outs[1][3][name]), name


def test_stiffness_is_read_in_stream_order():
    """sg_set_stiffness with a DEVICE k and unchanged id sets enqueues one copy; sg_get_energy issued behind it on the same stream reports
    the spring terms of the new k (and the other two terms' bits stay)"""
    from softgrip_amd.native import _ptr
    torch = _torch()
    scene = "softbox_fix"
    k_old, k_new = np.array([640.0, 300.0, 1400.0, 512.25]), np.array([350.0, 1225.0, 777.0, 901.5])
    m, nm, b = _batch(scene, k_old)
    _, jids, tids, _ = DR.SCENES[scene]
    _squeeze(b, 2, nsteps=5)
    st = b.get_state()
    qpos, qvel = st["qpos"].cpu().numpy(), st["qvel"].cpu().numpy()
    kd = torch.tensor(k_new, dtype=torch.float64, device=b.device)
    ja, ta = (C.c_int * len(jids))(*jids), (C.c_int * len(tids))(*tids)
    e_old = b.energy()
    b._check(b.L.sg_set_stiffness(b.ptr, _ptr(kd), 0, ja, len(jids), ta, len(tids), b._stream()))
    e_new = b.energy()
    e_old, e_new = e_old.cpu().numpy(), e_new.cpu().numpy()
    for e in range(4):
        for ks, got in ((k_old, e_old), (k_new, e_new)):
            kj, kt = DR.stiffness(m, scene, ks[e])
            ref = DR.reference(m, qpos[e], qvel[e], kj, kt)
            scale = DR.energy_scale(m, ref, kj, kt, qpos[e], qvel[e])
            assert (np.abs(got[e] - ref["energy"]) <= DR.REL * scale).all(), (e, got[e], ref["energy"])
        assert e_old[e, 1] != e_new[e, 1] and e_old[e, 0] == e_new[e, 0] and e_old[e, 3] == e_new[e, 3]


def test_rollout_fills_the_energy_block():
    """ManEnv.rollout(energy_out=...) fills [n, T, 4] with get_energy() after every env step and leaves the sensors block bit-identical to
    a rollout without it.  softbox_fix at ctrl = 0, the fingers at rest: the total's change between consecutive env steps stays within the
    worst such change of the oracle's own episode (the NumPy reference on the oracle's states, same stiffness), times 1.01"""
    import softgrip_amd as sg
    from oracle import oracle as O
    torch = _torch()
    scene, T = "softbox_fix", 5
    ks = np.array([640.0, 300.0, 1400.0])
    env = sg.ManEnv(1, 7, [model_path(scene)], n_envs=3, check_scene=False, tendon_damper="explicit")
    env.set_stiffness_values(ks)
    plain, f0 = env.rollout([None] * T)
    en = torch.full((3, T, 4), -7.5, dtype=torch.float64, device=env.env.device)
    sens, f1 = env.rollout([None] * T, energy_out=en)
    assert _same_bits(plain, sens) and int(f0.abs().sum()) == 0 and int(f1.abs().sum()) == 0
    assert _same_bits(en[:, -1].contiguous(), env.get_energy())
    en = en.cpu().numpy()
    assert np.isfinite(en).all() and (en != -7.5).all()
    m = env.model
    om = O.OracleModel(m.to_blob())
    _, jids, tids, _ = DR.SCENES[scene]
    worst_oracle = 0.0
    for e, k in enumerate(ks):
        s = O.OracleSim(om)
        s.jnt_stiffness[jids] = k
        s.tendon_stiffness[tids] = k
        s.reset(); s.forward(); s.step()
        kj, kt = DR.stiffness(m, scene, k)
        tot = []
        for t in range(T):
            for _ in range(7):
                assert s.step() == 0
            tot.append(DR.reference(m, s.qpos, s.qvel, kj, kt)["energy"].sum())
        worst_oracle = max(worst_oracle, float(np.abs(np.diff(tot)).max()))
    worst = float(np.abs(np.diff(en.sum(2), axis=1)).max())
    print("largest change of the total between env steps: device %.6e, oracle %.6e" % (worst, worst_oracle))
    assert worst <= 1.01 * worst_oracle, (worst, worst_oracle)
