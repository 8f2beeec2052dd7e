"""sg_get_point_motion / sg_get_jacobians on the GPU: the two entry points against the NumPy reference (tests/point_ref.py, itself pinned
to the oracle's gyro and accelerometer channels by tests/test_point_host.py) over the whole sweep of random grippers, straight against
the oracle's sensordata on the five scenes, the model's own sensors reproduced on the device alone (the virtual-IMU recipe), the
Jacobians summed to sg_get_mass_matrix's M, the calls' interface (env lists, point lists, NULL outputs, NaN envs, determinism, sentinels,
error paths), the body limit, and that the batch is never written.  Bounds: test_point_host.py's, unchanged -- dyn_ref.ARR
max(1, max |value|) per array, ARR point_ref.acc_scale() for acc and accel.  Shapes: 3 envs (dyn_ref.KS) wherever the env count is
free; 1, 64, 65 and 130 points (the 64-stride over points); nv = 118 and 283 (softbox, fourfinger: the row tails of the Jacobians)."""
import ctypes as C
import itertools

import numpy as np
import pytest

import dyn_ref as DR
import point_ref as PR
import smooth_ref as SR

pytestmark = pytest.mark.gpu

SENTINEL = -7.5
SHAPE = dict(pos=(3,), mat=(9,), vel=(6,), acc=(6,), gyro=(3,), accel=(3,))


def _torch():
    import torch
    return torch


def _T(b, a):
    torch = _torch()
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=b.device)


def _state_batch(m, qpos, qvel):
    """a batch with one env per state: one sg_set_state(qpos, qvel)"""
    from softgrip_amd import native
    b = native.NativeBatch(native.NativeModel(m), len(qpos), 0)
    b.set_state(qpos=_T(b, qpos), qvel=_T(b, qvel))
    return b


def _all(b, pts, qpos=None, qvel=None, qacc=None, env_ids=None):
    """each entry point once: dict of device tensors pos, mat [k, P, 9], vel, acc, gyro, accel, jacp, jacr"""
    body, pos, quat = pts
    out = b.point_motion(body, pos, quat, qpos=qpos, qvel=qvel, qacc=qacc, env_ids=env_ids)
    out["mat"] = out["mat"].reshape(out["mat"].shape[0], -1, 9)
    out.update(b.jacobians(body, pos, qpos=qpos, env_ids=env_ids))
    return out


def _host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _same_bits(a, b):
    torch = _torch()
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)))


def _against_reference(m, got, qpos, qvel, qacc, pts, what):
    """every env of `got` against point_ref.reference at the CPU tests' bounds -> the worst deviation per output in units of the bound"""
    worst = dict.fromkeys(PR.NAMES, 0.0)
    for e in range(len(qpos)):
        ref = PR.reference(m, qpos[e], qvel[e], None if qacc is None else qacc[e], *pts)
        for name, dev in PR.deviations({n: got[n][e] for n in PR.NAMES}, ref, None if qacc is None else qacc[e]).items():
            worst[name] = max(worst[name], dev)
            assert dev <= 1.0, (what, e, name, dev)
    return worst


@pytest.mark.parametrize("gripper,offset", DR.SWEEP_CASES)
def test_sweep_of_random_grippers_matches_the_reference(gripper, offset, tmp_path):
    """64 states of a random gripper (smooth_ref.sweep: qvel of scale 0, 1 and 30, qacc of scale 0, 1 and 1000) as 64 envs of one batch,
    the points of point_ref.points (sites, every body's centre of mass, the world, 12 random points in unnormalised frames): every
    output against the NumPy reference, no state left out.  Then the same states passed EXPLICITLY, in reversed order, to a batch
    that holds other states: the rows' bits are those of the first call, reversed.
    Measured on the MI355X, worst over the cases, in units of the bound: pos 4.9e-4, mat 1.2e-3, vel 1.0e-3, acc 1.5e-3,
    gyro 8.7e-4, accel 2.0e-3, jacp 1.0e-3, jacr 9.4e-4"""
    m, qpos, qvel, ks, jids, tids, act, qacc = SR.sweep(gripper, tmp_path, offset)
    body, pos, quat, groups = PR.points(m)
    pts = (body, pos, quat)
    b = _state_batch(m, qpos, qvel)
    dev = _all(b, pts, qacc=_T(b, qacc))
    what = "gripper %d%s" % (gripper, " with offset anchors" if offset else "")
    worst = _against_reference(m, _host(dev), qpos, qvel, qacc, pts, what)
    print("%s: %d bodies, %d dofs, %d points, %d states; in units of the bound %s" % (what, m.nbody, m.nv, len(body), len(ks), {k: "%.2e" % v for k, v in worst.items()}))
    b.set_state(qpos=_T(b, np.roll(qpos, 5, 0)), qvel=_T(b, np.roll(qvel, 7, 0)))
    rev = _all(b, pts, qpos=_T(b, qpos[::-1]), qvel=_T(b, qvel[::-1]), qacc=_T(b, qacc[::-1]))
    for name in PR.NAMES:
        assert _same_bits(rev[name], dev[name].flip(0)), name
    assert len(ks) == 64 and len(body) > 64


@pytest.mark.parametrize("scene", sorted(DR.SCENES))
def test_scenes_match_the_oracle(scene):
    """the five scenes (nv = 118 and 283 among them), three envs at the oracle's states a squeeze in (dyn_ref.states), put into the batch
    with sg_set_state: gyro and accel at the model's sites with the ORACLE's qacc against the gyro and accelerometer channels of its
    sensordata after dyn_ref.oracle_forward -- every channel of the scene, 12 or 24 --, then every output at point_ref.points against
    the reference with a drawn qacc"""
    from oracle import oracle as O
    m, om, sts = DR.states(scene)
    qpos, qvel = np.stack([s["qpos"] for s in sts]), np.stack([s["qvel"] for s in sts])
    b = _state_batch(m, qpos, qvel)
    sim = O.OracleSim(om)
    oq, sens = [], []
    for st in sts:
        DR.oracle_forward(sim, st["qpos"], st["qvel"], *DR.stiffness(m, scene, st["k"]))
        oq.append(sim.qacc.copy())
        sens.append(sim.sensordata.copy())
    sites = PR.site_points(m)
    got = _host(b.point_motion(*sites, qacc=_T(b, np.stack(oq))))
    worst, channels = dict(gyro=0.0, accel=0.0), 0
    for e in range(len(sts)):
        for adr, site, kind in PR.sensor_channels(m):
            want = sens[e][adr:adr + 3]
            dev = DR.close(got[kind][e, site], want) if kind == "gyro" else np.abs(got[kind][e, site] - want).max() / (DR.ARR * PR.acc_scale(want, oq[e]))
            worst[kind] = max(worst[kind], dev)
            channels += 3
            assert dev <= 1.0, (scene, e, kind, site, dev)
    assert channels == 3 * om.nsensordata and om.nsensordata in (12, 24)
    rs = np.random.RandomState(79)
    qacc = np.stack([SR.QACC_SCALES[e % 3] * rs.standard_normal(m.nv) for e in range(len(sts))])
    pts = PR.points(m)[:3]
    wr = _against_reference(m, _host(_all(b, pts, qacc=_T(b, qacc))), qpos, qvel, qacc, pts, scene)
    print(scene, "nv = %d; against the oracle" % m.nv, {k: "%.2e" % v for k, v in worst.items()}, "against the reference", {k: "%.2e" % v for k, v in wr.items()})


def _squeezed(scene, ks, nsteps=4):
    """a batch of len(ks) envs, sg_reset and nsteps env steps of a squeeze: real positions, velocities and activations"""
    from softgrip_amd import native
    torch = _torch()
    m = DR.load(scene)
    _, jids, tids, nu = DR.SCENES[scene]
    b = native.NativeBatch(native.NativeModel(m), len(ks), 0)
    b.set_stiffness(np.asarray(ks, dtype=np.float64), jids, tids)
    flags = torch.zeros(b.n, dtype=torch.int32, device=b.device)
    b.reset(1, flags=flags)
    b.set_ctrl_broadcast(np.full(nu, -0.2))
    for _ in range(nsteps):
        b.step(7, flags=flags)
    assert int(flags.abs().sum()) == 0
    return m, b


def _imu_matches(m, sens, out, qacc, site_of_point, what):
    """gyro / accel of `out` at the points that are the model's sensor sites against the channels of sens [k, nsensordata], both within
    the accel bound ARR (1 + max |sample| + max |qacc|) -> the worst deviation in units of it"""
    worst, channels = 0.0, 0
    for e in range(len(sens)):
        scale = DR.ARR * PR.acc_scale(sens[e], qacc[e])
        for adr, site, kind in PR.sensor_channels(m):
            dev = float(np.abs(out[kind][e, site_of_point[site]] - sens[e][adr:adr + 3]).max() / scale)
            worst = max(worst, dev)
            channels += 3
            assert dev <= 1.0, (what, e, kind, site, dev)
    assert channels == sens.size > 0
    return worst


@pytest.mark.parametrize("scene", ["softbox", "softbox_fix", "fourfinger_softball_fix"])
def test_the_models_own_sensors_are_reproduced_on_the_device(scene):
    """the header's recipe with n = 1, on the device alone: a batch four env steps into a squeeze (the two-finger scenes run the rows
    pipeline, the four-finger scene the tree pipeline); qpos and qvel copied out, sg_step(1), then sg_get_point_motion at the copied
    state with that step's qacc_warmstart: gyro / accel at the model's sites equal the step's sens_out within the accel bound, and no
    env raised a flag.  Measured on the MI355X: 2.3e-5, 4.2e-5 and 1.5e-4 of the bound"""
    torch = _torch()
    m, b = _squeezed(scene, DR.KS)
    st = b.get_state()
    sens = torch.zeros(b.n, b.nmodel.nsensordata, dtype=torch.float64, device=b.device)
    flags = torch.zeros(b.n, dtype=torch.int32, device=b.device)
    b.step(1, sens=sens, flags=flags)
    assert int(flags.abs().sum()) == 0
    qacc = b.get_state()["qacc_warmstart"]
    out = _host(b.point_motion(*b.nmodel.sites(), qpos=st["qpos"], qvel=st["qvel"], qacc=qacc))
    worst = _imu_matches(m, sens.cpu().numpy(), out, qacc.cpu().numpy(), {s: s for s in range(m.nsite)}, scene)
    assert float(sens.abs().max()) > 1.0, "the sensors must read something"
    print(scene, "virtual IMU against sens_out: %.2e of the bound" % worst)


def test_virtual_imu_of_the_env_returns_the_official_sensordata():
    """ManEnv.virtual_imu(*ManEnv.sensor_sites()) three env steps into a squeeze: the sensordata it returns is what step() returns on a
    twin env, bit for bit, and gyro / accel at the sensor sites equal it within the accel bound"""
    import softgrip_amd as sg
    from helpers import model_path
    envs = [sg.ManEnv(1, 7, [model_path("softbox")], is_vis=False, n_envs=3, check_scene=False) for _ in range(2)]
    for env in envs:
        env.rng = np.random.RandomState(3)
        env.reset()
        env.close_hand()
        for _ in range(2):
            env.step()
    sites = envs[0].sensor_sites()
    m = envs[0].model
    imu = sorted({site for _, site, _ in PR.sensor_channels(m)})
    assert len(sites[0]) == len(imu) > 0 and (sites[0] == np.asarray(m.site_bodyid)[imu]).all()
    sens, gyro, accel = envs[0].virtual_imu(*sites)
    twin, _ = envs[1].step()
    assert _same_bits(sens, twin)
    qacc = envs[0].env.get_state()["qacc_warmstart"].cpu().numpy()
    worst = _imu_matches(m, sens.cpu().numpy(), dict(gyro=gyro.cpu().numpy(), accel=accel.cpu().numpy()), qacc, {s: p for p, s in enumerate(imu)}, "ManEnv")
    print("ManEnv.virtual_imu against its sensordata: %.2e of the bound" % worst)


@pytest.mark.parametrize("scene", ["softbox_fix", "freeball_fix"])
def test_jacobians_sum_to_the_mass_matrix(scene):
    """one point per body at body_ipos: sum over the bodies of m jacp' jacp + jacr' R I R' jacr (R from the same call's mat) plus the
    armature is sg_get_mass_matrix's M of the same batch, at ARR max(1, max |M|)"""
    m, b = _squeezed(scene, DR.KS)
    body, pos = np.arange(m.nbody, dtype=np.int32), np.asarray(m.body_ipos, np.float64).reshape(-1, 3)
    J = _host(b.jacobians(body, pos))
    mat = b.point_motion(body, pos, outputs=("mat",))["mat"].cpu().numpy()
    M = b.mass_matrix().cpu().numpy()
    for e in range(b.n):
        S = np.diag(np.asarray(m.dof_armature, np.float64)).copy()
        for i in range(1, m.nbody):
            R = mat[e, i]
            S += m.body_mass[i] * J["jacp"][e, i].T @ J["jacp"][e, i] + J["jacr"][e, i].T @ (R @ np.reshape(m.body_imat[i], (3, 3)) @ R.T) @ J["jacr"][e, i]
        dev = DR.close(S, M[e])
        print(scene, e, "sum of J' I J against sg_get_mass_matrix: %.2e of the bound" % dev)
        assert dev <= 1.0, (scene, e, dev)


# ---- the calls' interface ----
def _raw(b, pts, ids, n_ids, out, qpos=None, qvel=None, qacc=None):
    """the two entry points with any output left out (None -> NULL)"""
    from softgrip_amd.native import _ptr
    body, pos, quat = (None if x is None else np.ascontiguousarray(x) for x in pts)
    arr = None if ids is None else np.ascontiguousarray(ids, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    hp = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)  # noqa: E731
    L, s = b.L, b._stream()
    bp = body.ctypes.data_as(C.POINTER(C.c_int32))
    rc = [L.sg_get_point_motion(b.ptr, arr, n_ids, len(body), bp, hp(pos), hp(quat), _ptr(qpos), _ptr(qvel), _ptr(qacc), *[_ptr(out.get(n)) for n in PR.MOTION], s),
          L.sg_get_jacobians(b.ptr, arr, n_ids, len(body), bp, hp(pos), _ptr(qpos), _ptr(out.get("jacp")), _ptr(out.get("jacr")), s)]
    return rc


def _guarded(full, keep):
    """for each kept output one flat buffer with 64 sentinels before and after the output's span -> (buffers, views on the spans)"""
    torch = _torch()
    bufs, views = {}, {}
    for n in keep:
        bufs[n] = torch.full((full[n].numel() + 128,), SENTINEL, dtype=torch.float64, device=full[n].device)
        views[n] = bufs[n][64:64 + full[n].numel()].view(full[n].shape)
    return bufs, views


def _guards_intact(bufs):
    return all(bool((x[:64] == SENTINEL).all()) and bool((x[-64:] == SENTINEL).all()) for x in bufs.values())


def _cycled(pts, n):
    """n points: the list repeated as often as it takes"""
    idx = np.arange(n) % len(pts[0])
    return tuple(np.ascontiguousarray(x[idx]) for x in pts)


@pytest.mark.parametrize("scene", ["softbox", "fourfinger_softball_fix"])
def test_point_counts_and_point_lists(scene):
    """nv = 118 and 283, three envs a squeeze in, 1, 64, 65 and 130 points (point_ref.points, repeated): against the reference at
    every count; a point's bits depend neither on the count nor on its place -- every count reproduces the 130-point call's rows, and a
    permuted list its rows, permuted"""
    torch = _torch()
    m, b = _squeezed(scene, DR.KS)
    st = {k: v.cpu().numpy() for k, v in b.get_state().items()}
    qacc = np.random.RandomState(4).standard_normal((3, m.nv))
    base = PR.points(m)[:3]
    full_pts = _cycled(base, 130)
    full = _all(b, full_pts, qacc=_T(b, qacc))
    worst = _against_reference(m, _host(full), st["qpos"], st["qvel"], qacc, full_pts, scene)
    for n in (1, 64, 65):
        part = _all(b, _cycled(base, n), qacc=_T(b, qacc))
        for name in PR.NAMES:
            assert _same_bits(part[name], full[name][:, :n]), (n, name)
    perm = np.random.RandomState(8).permutation(130)
    mixed = _all(b, tuple(np.ascontiguousarray(x[perm]) for x in full_pts), qacc=_T(b, qacc))
    sel = torch.as_tensor(perm, device=b.device)
    for name in PR.NAMES:
        assert _same_bits(mixed[name], full[name][:, sel]), name
    print(scene, "nv = %d, 130 points: %s" % (m.nv, {k: "%.2e" % v for k, v in worst.items()}))
    assert m.nv % 64 != 0


def test_listing_and_determinism():
    """softbox_fix, 9 envs a squeeze in, 65 points: env_ids as a subset, a permutation and with a repeated id reproduce the rows of the
    all-env call bit for bit (the given qacc rows follow the list); two calls give the same bits; outputs passed as NULL in any
    combination leave the others' bits as they are; the 64 sentinels before and after every output buffer are untouched; an env id
    out of range is refused"""
    from softgrip_amd import native
    torch = _torch()
    m, b = _squeezed("softbox_fix", np.linspace(300, 1400, 9))
    pts = _cycled(PR.points(m)[:3], 65)
    qacc = _T(b, np.random.RandomState(5).standard_normal((9, m.nv)))
    full = _all(b, pts, qacc=qacc)
    again = _all(b, pts, qacc=qacc)
    for name in full:
        assert _same_bits(full[name], again[name]), name
        assert bool(torch.isfinite(full[name]).all()), name
    for ids in ([4, 1], [8, 3, 0, 6, 2, 7, 1, 5, 4], [2, 2, 5], [7]):
        sel = torch.as_tensor(ids, device=b.device)
        part = _all(b, pts, qacc=qacc[sel].contiguous(), env_ids=ids)
        for name in full:
            assert _same_bits(part[name], full[name][sel]), (ids, name)
    for keep in [c for r in (1, 2, 7) for c in itertools.combinations(PR.NAMES, r)][::3]:
        bufs, out = _guarded(full, keep)
        assert _raw(b, pts, None, b.n, out, qacc=qacc) == [0, 0]
        for n in keep:
            assert _same_bits(out[n], full[n]), (keep, n)
        assert _guards_intact(bufs), keep
    assert _raw(b, pts, None, b.n, {}, qacc=qacc) == [0, 0]      # every output NULL: nothing to write, no error
    bufs, out = _guarded(full, PR.NAMES)
    assert _raw(b, pts, None, b.n, out, qacc=qacc) == [0, 0]
    for n in full:
        assert _same_bits(out[n], full[n]), n
    assert _guards_intact(bufs)
    two = torch.as_tensor([6, 3], device=b.device)
    bufs, out = _guarded({n: x[:2] for n, x in full.items()}, PR.NAMES)      # a partial list writes its rows and nothing behind them
    assert _raw(b, pts, [6, 3], 2, out, qacc=qacc[two].contiguous()) == [0, 0]
    for n in full:
        assert _same_bits(out[n], full[n][two]), n
    assert _guards_intact(bufs)
    for ids, n in (([0, 9], 2), (None, 3)):      # (NULL ids need n_ids == n_envs)
        assert _raw(b, pts, ids, n, {}) == [native.SG_ERR_INVALID] * 2
    assert b.L.sg_last_error().startswith(b"sg_get_jacobians:")


def test_error_paths_write_nothing():
    """n_ids <= 0, n_pts <= 0 (an empty list), an env id out of range, a NULL-ids count that is not the batch's, NULL pt_body / pt_pos,
    a body id of -1 and of nbody, a NaN and an inf in pt_pos and in pt_quat, a pt_quat of zero length: SG_ERR_INVALID under the entry
    point's own name before the device is touched -- every output buffer keeps its sentinels"""
    from softgrip_amd import native
    torch = _torch()
    m, b = _squeezed("softbox_fix", DR.KS, nsteps=1)
    good = _cycled(PR.points(m)[:3], 5)
    kw = dict(dtype=torch.float64, device=b.device)
    out = {n: torch.full((3, 5) + SHAPE[n], SENTINEL, **kw) for n in PR.MOTION}
    out.update({n: torch.full((3, 5, 3, m.nv), SENTINEL, **kw) for n in ("jacp", "jacr")})

    def changed(which, row, value):
        pts = [x.copy() for x in good]
        pts[which][row] = value
        return tuple(pts)

    both = [native.SG_ERR_INVALID] * 2
    for ids, n in ((None, 0), (None, -1), ([0, 3], 2), ([-1], 1), (None, 2)):
        assert _raw(b, good, ids, n, out) == both, (ids, n)
        assert b.L.sg_last_error().startswith(b"sg_get_jacobians:"), b.L.sg_last_error()
    for pts, word in ((changed(0, 2, -1), b"body id -1"), (changed(0, 4, m.nbody), b"body id %d" % m.nbody), (changed(1, 3, [0.0, np.nan, 0.0]), b"pt_pos"),
                      (changed(1, 0, [np.inf, 0.0, 0.0]), b"pt_pos")):
        assert _raw(b, pts, None, 3, out) == both, word
        assert b.L.sg_last_error().startswith(b"sg_get_jacobians:") and word in b.L.sg_last_error(), b.L.sg_last_error()
    for pts, word in ((changed(2, 1, [1.0, np.nan, 0.0, 0.0]), b"pt_quat"), (changed(2, 4, [0.0, 0.0, 0.0, 0.0]), b"zero length")):
        assert _raw(b, pts, None, 3, {n: out[n] for n in PR.MOTION}) == [native.SG_ERR_INVALID, 0], word      # (sg_get_jacobians takes no pt_quat)
    empty = tuple(x[:0] for x in good)
    assert _raw(b, empty, None, 3, out) == both and b"n_pts" in b.L.sg_last_error()
    L, s = b.L, b._stream()
    nul = [None] * 6
    assert L.sg_get_point_motion(b.ptr, None, 3, 5, None, good[1].ctypes.data_as(C.c_void_p), None, None, None, None, *nul, s) == native.SG_ERR_INVALID
    assert L.sg_last_error().startswith(b"sg_get_point_motion:") and b"pt_body" in L.sg_last_error()
    assert L.sg_get_jacobians(b.ptr, None, 3, 5, good[0].ctypes.data_as(C.POINTER(C.c_int32)), None, None, None, None, s) == native.SG_ERR_INVALID
    torch.cuda.synchronize()
    for n, x in out.items():
        assert bool((x == SENTINEL).all()), n


def test_nan_envs_get_nan_and_disturb_no_other():
    """a NaN planted in env 1's qvel and in env 3's qpos, an inf in env 4's qvel, through the given rows and then in the batch's own
    state: NaN everywhere in those envs' rows of every motion output, unchanged bits in the others'; the Jacobians, which use qpos
    alone, are NaN in env 3 (every entry) and keep their bits in all others.  A NaN in env 2's qacc row alone: NaN in that env's motion
    outputs, every other row as it was"""
    torch = _torch()
    m, b = _squeezed("freeball_fix", np.linspace(300, 1400, 6), nsteps=3)
    pts = _cycled(PR.points(m)[:3], 65)
    qacc = _T(b, np.random.RandomState(6).standard_normal((6, m.nv)))
    clean = _all(b, pts, qacc=qacc)
    qbad = qacc.clone()
    qbad[2, 7] = float("nan")
    got = _all(b, pts, qacc=qbad)
    for name in PR.MOTION:
        for e in range(6):
            assert bool(torch.isnan(got[name][e]).all()) if e == 2 else _same_bits(got[name][e], clean[name][e]), (name, e)
    for name in ("jacp", "jacr"):      # (sg_get_jacobians takes no qacc)
        assert _same_bits(got[name], clean[name]), name
    st = b.get_state()
    qpos, qvel = st["qpos"].clone(), st["qvel"].clone()
    qvel[1, 17] = float("nan")
    qpos[3, 5] = float("nan")
    qvel[4, 0] = float("inf")

    def check(got, names):
        for name in names:
            for e in range(6):
                if e in (1, 3, 4):
                    assert bool(torch.isnan(got[name][e]).all()), (name, e)
                else:
                    assert _same_bits(got[name][e], clean[name][e]), (name, e)

    def check_jac(got):      # (the Jacobians use qpos alone: env 3 is NaN there, envs 1 and 4 keep their bits whatever their qvel holds)
        for name in ("jacp", "jacr"):
            for e in range(6):
                assert bool(torch.isnan(got[name][e]).all()) if e == 3 else _same_bits(got[name][e], clean[name][e]), (name, e)

    given = _all(b, pts, qpos=qpos, qvel=qvel, qacc=qacc)
    check(given, PR.MOTION)
    check_jac(given)
    b.set_state(qpos=qpos, qvel=qvel)
    current = _all(b, pts, qacc=qacc)
    check(current, PR.MOTION)
    check_jac(current)


# ---- the body limit on the device ----
def test_body_limit_is_reached_on_the_device(tmp_path):
    """627 bodies: what the velocity read-out, whose tables these calls walk, can run (SGD_MAXBODY; the point kernel's own LDS budget,
    SGP_MAXBODY = 672, lies above it): gripper 1 of the sweep (on a free joint) padded with jointless children of its static body, as
    tests/test_gpu_dyn.py pads it -- the launch asks for more dynamic LDS than the 64 KB a launch gets without the attribute.  Two
    envs -- a swept pose and the rest pose, qvel of scale 1 -- match the reference at the sweep's bounds, one point per body among the points"""
    import test_gpu_dyn as TD
    assert TD.MAXBODY <= PR.MAXBODY
    m = TD._padded(tmp_path, TD.MAXBODY)
    q, v, ks = TD._padded_states(m, tmp_path)
    qacc = np.random.RandomState(9).standard_normal((2, m.nv))
    pts = PR.points(m)[:3]
    b = _state_batch(m, q, v)
    worst = _against_reference(m, _host(_all(b, pts, qacc=_T(b, qacc))), q, v, qacc, pts, "%d bodies" % m.nbody)
    print("%d bodies, %d points: %s" % (m.nbody, len(pts[0]), {k: "%.2e" % x for k, x in worst.items()}))
    assert 8 * (19 * m.nbody + 7 * m.nv) + 4 * m.nv > 65536 and len(pts[0]) > m.nbody


def test_one_body_beyond_the_limit_is_refused(tmp_path):
    """628 bodies: both entry points return SG_ERR_MODEL under their own name with "more than 627 bodies" and write nothing
    (sentinels), and sg_get_poses of the same batch still answers correctly"""
    import test_gpu_dyn as TD
    from softgrip_amd import native
    torch = _torch()
    m = TD._padded(tmp_path, TD.MAXBODY + 1)
    q, v, ks = TD._padded_states(m, tmp_path)
    b = _state_batch(m, q, v)
    pts = _cycled(PR.points(m)[:3], 5)
    kw = dict(dtype=torch.float64, device=b.device)
    out = {n: torch.full((2, 5) + SHAPE[n], SENTINEL, **kw) for n in PR.MOTION}
    out.update({n: torch.full((2, 5, 3, m.nv), SENTINEL, **kw) for n in ("jacp", "jacr")})
    for k, name in enumerate(("sg_get_point_motion", "sg_get_jacobians")):
        assert _raw(b, pts, None, 2, out)[k] == native.SG_ERR_MODEL, name
    msg = b.L.sg_last_error()
    assert msg.startswith(b"sg_get_jacobians:") and b"more than %d bodies" % TD.MAXBODY in msg, msg
    torch.cuda.synchronize()
    for n, x in out.items():
        assert bool((x == SENTINEL).all()), n
    TD._against_kinematics(m, {k: x.cpu().numpy() for k, x in b.poses().items()}, q, "%d bodies" % (TD.MAXBODY + 1))


def test_calls_change_nothing():
    """the state (sg_get_state's five arrays) is bit-identical before and after any number of the new calls -- all envs, a list, given
    rows --, and a twin batch that made none produces bit-identical sensordata, flags and state from the next sg_step"""
    torch = _torch()
    outs = []
    for read in (True, False):
        m, b = _squeezed("softbox", np.linspace(300, 1400, 5))
        if read:
            pts = PR.points(m)[:3]
            before = b.get_state()
            qacc = _T(b, np.random.RandomState(2).standard_normal((5, m.nv)))
            _all(b, pts, qacc=qacc)
            _all(b, pts, qpos=before["qpos"][:2].contiguous(), qvel=before["qvel"][:2].contiguous(), qacc=qacc[:2].contiguous(), env_ids=[3, 0])
            _all(b, _cycled(pts, 1))
            after = b.get_state()
            for name in before:
                assert _same_bits(before[name], after[name]), name
        sens = torch.zeros(b.n, b.nmodel.nsensordata, dtype=torch.float64, device=b.device)
        flags = torch.zeros(b.n, dtype=torch.int32, device=b.device)
        b.step(7, sens=sens, flags=flags)
        outs.append((sens, flags, b.get_state()))
    assert _same_bits(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    for name in outs[0][2]:
        assert _same_bits(outs[0][2][name], outs[1][2][name]), name
