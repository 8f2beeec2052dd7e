"""sg_get_forces on the GPU: every state of forces_ref.all_states() against the oracle at the same bound
    |x - x_ref| <= max(TOL, 10 unit_x) max(1, max |x_ref|),    TOL = 1e-9,    x = efc_force, qacc, qfrc_constraint
(forces_ref.py: unit_x is the oracle's own largest change of x over 10 runs at qpos + 1e-14 N(0, 1); a state is left out only where
those runs disagree among themselves on (nefc, ncon, solver_iter), and the count of such states is asserted to be zero), with nefc,
ncon, the row types and ids and the sweeps against solver_iter exact; the batch's own stepping on the rows and the tree pipeline; the
call's identities without the oracle; and its interface: env lists, NULL outputs, short buffers, a NaN env, determinism, chunking,
an untouched batch, stream ordering, every error path.  Small batches: 3 or 5 envs."""
import ctypes as C

import numpy as np
import pytest

import dyn_ref as DR
import forces_ref as FR
import point_ref as PR
import solve_ref as VR
from test_gpu_smooth import SENTINEL, _T, _same_bits

pytestmark = pytest.mark.gpu
KEYS = list(FR.SCENE_STEPS) + list(FR.GRIPPERS)
NAMES = ("nefc", "iters", "efc_type", "efc_id", "efc_force", "ncon", "contact_force", "qfrc_constraint", "qacc")


def _torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return tmp_path_factory.mktemp("forces_gpu")


def _batch(key, sts, tmp):
    """a batch with one env per state, seated by one sg_set_state (qpos, qvel, act, qacc_warmstart, ctrl) and one sg_set_stiffness"""
    from softgrip_amd import native
    m, _, jids, tids = FR.model(key, tmp)
    b = native.NativeBatch(native.NativeModel(m), len(sts), 0)
    stack = lambda name: _T(b, np.stack([s[name] for s in sts]))  # noqa: E731
    b.set_state(qpos=stack("qpos"), qvel=stack("qvel"), act=stack("act"), qacc_warmstart=stack("warm"), ctrl=stack("ctrl"))
    b.set_stiffness(np.array([s["k"] for s in sts], dtype=np.float64), jids, tids)
    return m, b


def _env(out, e):
    """env e of forces()' dict on the host, in forces_ref's names"""
    n = int(out["nefc"][e])
    return dict(nefc=n, ncon=int(out["ncon"][e]), iters=int(out["iters"][e]), type=out["efc_type"][e, :max(n, 0)].cpu().numpy(),
                id=out["efc_id"][e, :max(n, 0)].cpu().numpy(), f=out["efc_force"][e, :max(n, 0)].cpu().numpy(), qacc=out["qacc"][e].cpu().numpy(),
                qfrc=out["qfrc_constraint"][e].cpu().numpy(), contact_force=out["contact_force"][e].cpu().numpy())


def _against(got, ref, what, worst):
    FR.check_discrete(got, ref, what)
    for q in ("f", "qacc", "qfrc"):
        FR.worse(worst, q, FR.dev(got[q], ref, q))


def _identities(m, b, out, what, worst):
    """without the oracle: limit and normal forces >= 0; the cone inequality; contact_force the bits of its efc_force entries;
    sg_inverse_dynamics(qacc) - actuator = qfrc_constraint within the smooth read-outs' bounds (the residual unit of M qacc plus
    dyn_ref.ARR per array)"""
    con = b.contacts(max_contacts=out["contact_force"].shape[1])
    inv, actuator, M = b.inverse_dynamics(out["qacc"]).cpu().numpy(), b.joint_forces()["actuator"].cpu().numpy(), b.mass_matrix().cpu().numpy()
    geom = con["geom"].cpu().numpy()
    for e in range(b.n):
        g = _env(out, e)
        assert g["ncon"] == int(con["ncon"][e]), what
        f, ty, ids = g["f"], g["type"], g["id"]
        assert (f[ty == 3] >= 0).all(), what
        cf, seen = g["contact_force"], np.zeros(max(g["ncon"], 1), bool)
        i = 0
        while i < g["nefc"]:
            if ty[i] in (5, 7):
                dim, c = (1, 3)[int(ty[i] == 7)], int(ids[i])
                seen[c] = True
                want = np.zeros(3)
                want[:dim] = f[i:i + dim]
                assert want.tobytes() == cf[c].tobytes() and f[i] >= 0, (what, e, c)
                if dim == 3:
                    mu = max(float(m.geom_friction[geom[e, c, 0], 0]), float(m.geom_friction[geom[e, c, 1], 0]))
                    assert np.hypot(f[i + 1], f[i + 2]) <= mu * f[i] * (1 + 1e-9) + 1e-12, (what, e, c)
                i += dim
            else:
                i += 1
        assert not cf[:g["ncon"]][~seen[:g["ncon"]]].any() if g["ncon"] else True, what
        unit = VR.residual_unit(M[e], g["qacc"], inv[e])[0] + sum(DR.ARR * max(1.0, float(np.abs(t).max())) for t in (inv[e], actuator[e], g["qfrc"]))
        FR.worse(worst, "inverse_dynamics(qacc) - actuator = qfrc_constraint", np.abs(inv[e] - actuator[e] - g["qfrc"]).max() / unit)


@pytest.mark.parametrize("key", KEYS)
def test_states_match_the_oracle(key, work):
    """every state of one scene or gripper, three envs at dyn_ref.KS, the forces() call the first call on a fresh batch; and the
    identities on the same outputs.
    Measured on the MI355X, worst over the ten cases, in units of the bound: efc_force 9.5e-5 (the four-finger scene), qacc 3.8e-6,
    qfrc_constraint 1.4e-4 (gripper 2); sg_inverse_dynamics(qacc) - actuator = qfrc_constraint 7.3e-2 of its unit (gripper 2).  The
    host build's figures: tests/test_forces_host.py; none of the 108 states is a knife edge"""
    worst, knife = {}, 0
    steps = FR.SCENE_STEPS[key] if isinstance(key, str) else FR.GRIPPER_STEPS
    for n in steps:
        sts = FR.states(key, steps, work)[n]
        m, b = _batch(key, sts, work)
        out = b.forces(max_contacts=FR.host_cap(m))
        for e in range(len(sts)):
            ref = FR.reference(key, n, e, work)
            if ref["knife"]:
                knife += 1
                continue
            _against(_env(out, e), ref, (key, n, e), worst)
        _identities(m, b, out, (key, n), worst)
    assert knife == 0, (key, knife)
    FR.report("%s" % (key,), worst)


@pytest.mark.parametrize("key,pipeline,nsteps", [("softbox", "rows", 20), (0, "tree", 10)])
def test_the_batchs_own_stepping(key, pipeline, nsteps, work):
    """sg_reset, then nsteps sg_step calls of one substep on a 3-env batch; sg_get_state, the oracle seated there, forward(), the same
    bound.  softbox on the rows pipeline, gripper 0 on the tree pipeline.  Measured on the MI355X, in units of the bound: 4.6e-7 and
    1.1e-5; neither state is a knife edge"""
    from softgrip_amd import native
    torch = _torch()
    m, _, jids, tids = FR.model(key, work)
    b = native.NativeBatch(native.NativeModel(m), len(FR.KS), 0)
    b.set_pipeline(pipeline)
    b.set_stiffness(np.asarray(FR.KS, dtype=np.float64), jids, tids)
    flags = torch.zeros(b.n, dtype=torch.int32, device=b.device)
    b.reset(1, flags=flags)
    b.set_ctrl_broadcast(np.full(m.nu, -0.2))
    for _ in range(nsteps):
        b.step(1, flags=flags)
    assert int(flags.abs().sum()) == 0
    st = {k: v.cpu().numpy() for k, v in b.get_state().items()}
    out = b.forces(max_contacts=FR.host_cap(m))
    worst, knife = {}, 0
    for e, k in enumerate(FR.KS):
        s = dict(qpos=st["qpos"][e], qvel=st["qvel"][e], act=st["act"][e], ctrl=st["ctrl"][e], warm=st["qacc_warmstart"][e], k=k)
        ref = FR.reference_at(key, s, 2000 + e, work)
        knife += int(ref["knife"])
        if not ref["knife"]:
            assert ref["nefc"] > 0
            _against(_env(out, e), ref, (key, pipeline, e), worst)
    assert knife == 0, (key, knife)
    FR.report("%s on the %s pipeline" % (key, pipeline), worst)


def test_sensors_of_the_next_step_follow_the_returned_qacc(work):
    """after sg_step(n_substeps = 1) the gyro and accelerometer channels equal sg_get_point_motion at the sensor sites at the state
    BEFORE the step with the qacc this call returned before the step, within test_gpu_parity.TOL_SENSOR (one step's sensordata).
    Measured on the MI355X: 1.0e-13"""
    from test_gpu_parity import TOL_SENSOR
    torch = _torch()
    key, n = "mini_gripper", 60
    sts = FR.states(key, FR.SCENE_STEPS[key], work)[n]
    m, b = _batch(key, sts, work)
    chans = PR.sensor_channels(m)
    assert chans
    sites = sorted({s for _, s, _ in chans})
    body = np.asarray(m.site_bodyid, np.int32)[sites]
    pos, quat = np.asarray(m.site_pos, np.float64).reshape(-1, 3)[sites], np.asarray(m.site_quat, np.float64).reshape(-1, 4)[sites]
    qacc = b.forces()["qacc"]
    pm = b.point_motion(body, pos, quat, qacc=qacc, outputs=("gyro", "accel"))
    sens = torch.zeros(b.n, m.nsensordata, dtype=torch.float64, device=b.device)
    b.step(1, sens=sens, sens_stride=m.nsensordata)
    worst = 0.0
    for adr, site, kind in chans:
        worst = max(worst, float((sens[:, adr:adr + 3] - pm[kind][:, sites.index(site)]).abs().max()))
    print("sensor channels against point motion with the returned qacc: %.3g (tolerance %.1g)" % (worst, TOL_SENSOR))
    assert worst < TOL_SENSOR


def _raw(b, ids, n_ids, max_rows, max_contacts, out):
    """sg_get_forces with any output left out (absent -> NULL)"""
    from softgrip_amd.native import _ptr
    arr = None if ids is None else np.ascontiguousarray(ids, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    return b.L.sg_get_forces(b.ptr, arr, n_ids, max_rows, max_contacts, *[_ptr(out.get(n)) for n in NAMES], b._stream())


def _five(work):
    key, n = "mini_gripper", 60
    three = FR.states(key, FR.SCENE_STEPS[key], work)[n]
    return key, [three[e % 3] for e in range(5)]


def test_listing_determinism_and_short_buffers(work):
    """mini_gripper 60 steps in (57 rows, 6 contacts), 5 envs: two calls give the same bits; env_ids as a subset, a permutation and with
    a repeated id reproduce the rows of the all-env call; every output alone (the others NULL) has the bits it has in the full call;
    max_rows < nefc and max_contacts < ncon leave the counts full, write the first rows only and leave the sentinels past them and
    the 64 guard words around every buffer intact; a work space of two envs' worth (three chunks for five envs) gives the bits of
    the unchunked call"""
    from softgrip_amd import native
    torch = _torch()
    key, sts = _five(work)
    m, b = _batch(key, sts, work)
    full, again = b.forces(max_contacts=16), b.forces(max_contacts=16)
    for name in NAMES:
        assert _same_bits(full[name].double(), again[name].double()), name
    assert int(full["nefc"].min()) == 57 and int(full["ncon"].min()) == 6
    for ids in ([4, 1], [3, 0, 2, 1, 4], [2, 2], [3]):
        part = b.forces(env_ids=ids, max_contacts=16)
        sel = torch.as_tensor(ids, device=b.device)
        for name in NAMES:
            assert _same_bits(part[name].double(), full[name][sel].double()), (ids, name)
    for name in NAMES:
        one = {name: torch.zeros_like(full[name])}
        assert _raw(b, None, 5, full["efc_force"].shape[1], 16, one) == native.SG_OK
        assert _same_bits(one[name].double(), full[name].double()), name
    # short buffers between guard words
    mr, mc = 10, 2
    shapes = dict(nefc=(5,), iters=(5,), ncon=(5,), efc_type=(5, mr), efc_id=(5, mr), efc_force=(5, mr), contact_force=(5, mc, 3), qfrc_constraint=(5, m.nv), qacc=(5, m.nv))
    bufs, views = {}, {}
    for name, shape in shapes.items():
        dt, fill = (torch.float64, SENTINEL) if full[name].dtype == torch.float64 else (torch.int32, -77)
        bufs[name] = torch.full((int(np.prod(shape)) + 128,), fill, dtype=dt, device=b.device)
        views[name] = bufs[name][64:64 + int(np.prod(shape))].view(shape)
    assert _raw(b, None, 5, mr, mc, views) == native.SG_OK
    for name, x in bufs.items():
        fill = SENTINEL if x.dtype == torch.float64 else -77
        assert bool((x[:64] == fill).all()) and bool((x[-64:] == fill).all()), name
    for name in ("nefc", "iters", "ncon", "qfrc_constraint", "qacc"):
        assert _same_bits(views[name].double(), full[name].double()), name
    for name in ("efc_type", "efc_id", "efc_force"):
        assert _same_bits(views[name].double(), full[name][:, :mr].double()), name
    assert _same_bits(views["contact_force"], full["contact_force"][:, :mc])
    # ... and a buffer LONGER than the list keeps its sentinels past the written part
    long_ = {"efc_force": torch.full((5, 80), SENTINEL, dtype=torch.float64, device=b.device), "contact_force": torch.full((5, 9, 3), SENTINEL, dtype=torch.float64, device=b.device)}
    assert _raw(b, None, 5, 80, 9, long_) == native.SG_OK
    assert bool((long_["efc_force"][:, 57:] == SENTINEL).all()) and bool((long_["contact_force"][:, 6:] == SENTINEL).all())
    assert _same_bits(long_["efc_force"][:, :57], full["efc_force"][:, :57])
    # chunking
    per_env = FR.host_env_bytes(m)
    b.set_forces_workspace(2 * per_env + 64)
    chunked = b.forces(max_contacts=16)
    for name in NAMES:
        assert _same_bits(chunked[name].double(), full[name].double()), name
    with pytest.raises(native.SoftgripError) as ei:
        b.set_forces_workspace(per_env // 2)
    assert ei.value.code == native.SG_ERR_INVALID and "one env" in str(ei.value)


def test_a_nan_env_the_untouched_batch_and_stream_order(work):
    """the batch's state is bit-identical before and after the call, and a following sg_step gives the bits of a twin batch that never
    called it; the call right behind sg_set_stiffness and sg_set_state (no synchronisation between) sees the new values; an env whose
    qpos holds a NaN reports nefc = ncon = -1 and NaN in every double output and disturbs no other env"""
    torch = _torch()
    key, sts = _five(work)
    m, b = _batch(key, sts, work)
    _, twin = _batch(key, sts, work)
    before = b.get_state()
    full = b.forces(max_contacts=16)
    after = b.get_state()
    for name in before:
        assert _same_bits(before[name], after[name]), name
    sens = [torch.zeros(5, m.nsensordata, dtype=torch.float64, device=b.device) for _ in range(2)]
    b.step(1, sens=sens[0], sens_stride=m.nsensordata)
    twin.step(1, sens=sens[1], sens_stride=m.nsensordata)
    assert _same_bits(sens[0], sens[1])
    sa, sb = b.get_state(), twin.get_state()
    for name in sa:
        assert _same_bits(sa[name], sb[name]), name
    # stream order: new stiffness and a new state, the call right behind them
    _, jids, tids = FR.model(key, work)[1:]
    swapped = [dict(sts[(e + 1) % 5]) for e in range(5)]
    m2, fresh = _batch(key, swapped, work)
    want = fresh.forces(max_contacts=16)
    stack = lambda name: _T(b, np.stack([s[name] for s in swapped]))  # noqa: E731
    b.set_state(qpos=stack("qpos"), qvel=stack("qvel"), act=stack("act"), qacc_warmstart=stack("warm"), ctrl=stack("ctrl"))
    b.set_stiffness(np.array([s["k"] for s in swapped], dtype=np.float64), jids, tids)
    got = b.forces(max_contacts=16)
    for name in NAMES:
        assert _same_bits(got[name].double(), want[name].double()), name
    assert not _same_bits(got["efc_force"], full["efc_force"])
    # a NaN env
    st = b.get_state()
    st["qpos"][1, 3] = float("nan")
    b.set_state(qpos=st["qpos"])
    bad = b.forces(max_contacts=16)
    assert int(bad["nefc"][1]) == -1 and int(bad["ncon"][1]) == -1
    for name in ("efc_force", "contact_force", "qfrc_constraint", "qacc"):
        assert bool(torch.isnan(bad[name][1]).all()), name
        keep = [0, 2, 3, 4]
        assert _same_bits(bad[name][keep], got[name][keep]), name


def test_every_error_path(work):
    """SG_ERR_INVALID before anything touches the device: n_ids <= 0, an env id out of range, max_rows <= 0 with a row array,
    max_contacts <= 0 with contact_force; nothing is written"""
    from softgrip_amd import native
    torch = _torch()
    key, sts = _five(work)
    m, b = _batch(key, sts, work)
    f = torch.full((5, 8), SENTINEL, dtype=torch.float64, device=b.device)
    cf = torch.full((5, 4, 3), SENTINEL, dtype=torch.float64, device=b.device)
    def err():
        msg = b.L.sg_last_error()
        assert msg.startswith(b"sg_get_forces:"), msg
        return msg

    assert _raw(b, None, 0, 8, 4, {"efc_force": f}) == native.SG_ERR_INVALID and b"n_ids" in err()
    assert _raw(b, [0, 5], 2, 8, 4, {"efc_force": f}) == native.SG_ERR_INVALID and b"out of range" in err()
    assert _raw(b, [-1], 1, 8, 4, {"efc_force": f}) == native.SG_ERR_INVALID and b"out of range" in err()
    assert _raw(b, None, 5, 0, 4, {"efc_force": f}) == native.SG_ERR_INVALID and b"max_rows" in err()
    assert _raw(b, None, 5, 8, 0, {"contact_force": cf}) == native.SG_ERR_INVALID and b"max_contacts" in err()
    assert _raw(b, None, 3, 8, 4, {"efc_force": f}) == native.SG_ERR_INVALID and b"env_ids == NULL" in err()
    assert bool((f == SENTINEL).all()) and bool((cf == SENTINEL).all())
    # max_rows <= 0 is fine where no row array is given, and every output NULL is a call that does nothing
    n = torch.zeros(5, dtype=torch.int32, device=b.device)
    assert _raw(b, None, 5, 0, 0, {"nefc": n}) == native.SG_OK and int(n.min()) == 57
    assert _raw(b, None, 5, 0, 0, {}) == native.SG_OK


def test_a_model_sg_solve_mass_refuses_is_refused_under_each_name(tmp_path):
    """450 bodies (test_gpu_dyn's padded gripper), one past sg_get_mass_matrix' limit: sg_get_forces, sg_model_max_rows and
    sg_set_forces_workspace each return SG_ERR_MODEL under their own name with "more than 449 bodies", and nothing is written.  (The
    other refusals of the forces table -- condim, equality type, the row list's LDS block -- are models sg_model_create does not
    accept: tests/test_forces_host.py holds them on the table builder)"""
    import test_gpu_dyn as TD
    from softgrip_amd import native
    from test_gpu_smooth import _state_batch
    torch = _torch()
    m = TD._padded(tmp_path, 450)
    jids, tids = DR.sweep_ids(m)
    q, v, ks = TD._padded_states(m, tmp_path)
    b = _state_batch(m, q, v, np.zeros((2, m.nu)), ks, jids, tids)
    out = {"efc_force": torch.full((2, 8), SENTINEL, dtype=torch.float64, device=b.device), "qacc": torch.full((2, m.nv), SENTINEL, dtype=torch.float64, device=b.device),
           "nefc": torch.full((2,), -77, dtype=torch.int32, device=b.device)}
    calls = (("sg_get_forces", lambda: _raw(b, None, 2, 8, 4, out)), ("sg_model_max_rows", lambda: b.L.sg_model_max_rows(b.nmodel.ptr)),
             ("sg_set_forces_workspace", lambda: b.L.sg_set_forces_workspace(b.ptr, C.c_size_t(1 << 30))))
    for name, call in calls:
        assert call() == native.SG_ERR_MODEL, name
        msg = b.L.sg_last_error()
        assert msg.startswith(name.encode() + b":") and b"more than 449 bodies" in msg, (name, msg)
    torch.cuda.synchronize()
    assert bool((out["efc_force"] == SENTINEL).all()) and bool((out["qacc"] == SENTINEL).all()) and bool((out["nefc"] == -77).all())


def test_manenv_get_forces_and_contact_forces():
    """ManEnv on softball 30 steps into the squeeze: get_forces() has the bits of NativeBatch.forces(); get_contact_forces() is
    get_contacts()' dict plus force, the bits of contact_force, and force_world, which is the sum of the frame's rows weighted by the
    force's components (checked against that sum written out in NumPy: the transpose would fail) -- so force_world . normal is the
    normal force, and that is positive on some contact of every env; an env subset follows the list"""
    from helpers import model_path
    from softgrip_amd.manenv import ManEnv
    env = ManEnv(1, 7, [model_path("softball")], is_vis=False, n_envs=4, tendon_damper="implicit")
    env.reset()
    env.close_hand()
    for _ in range(30):
        env.step()
    f, d = env.get_forces(max_contacts=64), env.get_env().forces(max_contacts=64)
    assert set(f) == set(d) == set(NAMES)
    for k in d:
        assert f[k].is_cuda and f[k].cpu().numpy().tobytes() == d[k].cpu().numpy().tobytes(), k
    assert f["efc_force"].shape[1] == env.get_env().max_rows() and int(f["nefc"].min()) > 0
    c, base = env.get_contact_forces(max_contacts=64), env.get_contacts(max_contacts=64)
    assert set(c) == set(base) | {"force", "force_world"}
    for k in ("ncon", "geom", "dist", "pos", "frame"):
        assert c[k].cpu().numpy().tobytes() == base[k].cpu().numpy().tobytes(), k
    assert c["force"].cpu().numpy().tobytes() == d["contact_force"].cpu().numpy().tobytes()
    force, frame, world, ncon = c["force"].cpu().numpy(), c["frame"].cpu().numpy().reshape(4, 64, 3, 3), c["force_world"].cpu().numpy(), c["ncon"].cpu().numpy()
    assert (ncon > 0).all() and (ncon <= 64).all()
    want = force[..., 0:1] * frame[:, :, 0] + force[..., 1:2] * frame[:, :, 1] + force[..., 2:3] * frame[:, :, 2]
    scale = max(1.0, float(np.abs(force).max()))
    assert np.abs(world - want).max() <= 1e-14 * scale, np.abs(world - want).max()
    for e in range(4):
        n = ncon[e]
        normal = frame[e, :n, 0]
        assert np.abs((world[e, :n] * normal).sum(1) - force[e, :n, 0]).max() <= 1e-13 * scale
        assert force[e, :n, 0].max() > 0 and (force[e, :n, 0] >= 0).all()
        tangential = np.abs(force[e, :n, 1:]).max()
        assert tangential > 0 and np.abs(world[e, :n] - force[e, :n, 0:1] * normal).max() > 0.1 * tangential      # (the tangential part is there, in world axes)
    sub = env.get_contact_forces(env_ids=[2, 0], max_contacts=16)
    assert sub["force"].shape == (2, 16, 3) and np.array_equal(sub["force_world"].cpu().numpy(), world[[2, 0], :16])
