"""sg_get_mass_matrix / sg_get_joint_forces / sg_inverse_dynamics on the GPU: the three entry points against the NumPy reference
(tests/smooth_ref.py, itself pinned to the oracle by tests/test_smooth_host.py) over the whole sweep of random grippers, straight against
the oracle's qM and qfrc_bias on the five scenes, M's symmetry and definiteness, the kinetic identity against sg_get_energy, the calls'
interface (env lists, NULL outputs, NaN envs, determinism, sentinels, error paths, stream ordering against sg_set_stiffness) and the
body limit.  Bounds: dyn_ref's, unchanged -- ARR max(1, max |value|) per array, REL for the kinetic identity."""
import ctypes as C
import itertools

import numpy as np
import pytest

import dyn_ref as DR
import smooth_ref as SR

pytestmark = pytest.mark.gpu

FRC = ("bias", "passive", "actuator")
SENTINEL = -7.5


def _torch():
    import torch
    return torch


def _T(b, a):
    torch = _torch()
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=b.device)


def _state_batch(m, qpos, qvel, act, ks, jids, tids):
    """a batch with one env per state: one sg_set_state(qpos, qvel, act), one sg_set_stiffness"""
    from softgrip_amd import native
    b = native.NativeBatch(native.NativeModel(m), len(ks), 0)
    b.set_state(qpos=_T(b, qpos), qvel=_T(b, qvel), act=_T(b, act))
    b.set_stiffness(np.asarray(ks, dtype=np.float64), jids, tids)
    return b


def _all(b, qacc, env_ids=None):
    """each entry point once: dict of device tensors M, bias, passive, actuator, inverse"""
    out = dict(M=b.mass_matrix(env_ids))
    out.update(b.joint_forces(env_ids))
    out["inverse"] = b.inverse_dynamics(qacc, env_ids)
    return out


def _host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _same_bits(a, b):
    torch = _torch()
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)))


def _against_reference(got, refs, what):
    """every env of `got` against its reference at dyn_ref.close's bound -> the worst deviation per output in units of the bound"""
    worst = dict.fromkeys(SR.NAMES + ("inverse",), 0.0)
    for e, ref in enumerate(refs):
        for name in worst:
            dev = DR.close(got[name][e], ref[name])
            worst[name] = max(worst[name], dev)
            assert dev <= 1.0, (what, e, name, dev)
    return worst


SINGULAR = 1e-10      # a reference M whose smallest eigenvalue is below this fraction of its largest is singular: see _mass_properties
# the sweep's states with a singular M, per case, counted on the CPU from the reference alone: 17 of 448
SWEEP_SINGULAR = {(0, False): 4, (1, False): 4, (2, False): 0, (3, False): 3, (4, False): 3, (5, False): 3, (3, True): 0}


def _mass_properties(got, refs, qvel, energy, what):
    """M is symmetric to the bit and numpy.linalg.cholesky succeeds on every env whose M is not singular; 1/2 qvel' M qvel is
    sg_get_energy's kinetic term within REL (exactly zero at rest) -> (the worst relative deviation, the number of singular envs).
    Singular: the sweep leaves some links with two of their hinges' axes on one line through one point (the generator puts all
    joints of a link at its origin), where the true M has a zero eigenvalue and the oracle's qM fails cholesky as well.  Which envs
    those are is read from the REFERENCE's M, never from the device's: its smallest eigenvalue relative to the largest is below 1e-15
    in magnitude there and above 5e-8 everywhere else (measured on the CPU), SINGULAR = 1e-10 lies between; the counts are asserted.
    On such an env the device's M must still be positive semidefinite to the bound: smallest eigenvalue >= -nv ARR max(1, max |M|)"""
    worst, singular = 0.0, 0
    for e in range(len(qvel)):
        M = got["M"][e]
        assert M.tobytes() == np.ascontiguousarray(M.T).tobytes(), (what, e)
        ev = np.linalg.eigvalsh(refs[e]["M"])
        if ev[0] < SINGULAR * ev[-1]:
            singular += 1
            assert np.linalg.eigvalsh(M)[0] >= -len(M) * DR.ARR * max(1.0, np.abs(M).max()), (what, e)
        else:
            np.linalg.cholesky(M)
        ke = 0.5 * qvel[e] @ M @ qvel[e]
        if not qvel[e].any():
            assert ke == 0.0 and energy[e, 3] == 0.0, (what, e)
            continue
        dev = abs(ke - energy[e, 3]) / energy[e, 3]
        worst = max(worst, dev)
        assert dev <= DR.REL, (what, e, ke, energy[e, 3])
    return worst, singular


@pytest.mark.parametrize("gripper,offset", DR.SWEEP_CASES)
def test_sweep_of_random_grippers_matches_the_reference(gripper, offset, tmp_path):
    """64 states of a random gripper (dyn_ref.sweep, with smooth_ref.sweep's activation in U(-1, 1) and qacc of scale 0, 1 and 1000) as
    64 envs of one batch: one sg_set_state, one sg_set_stiffness, then each entry point once.  Every output against the NumPy
    reference at ARR max(1, max |value|) per array, no state left out; M symmetric to the bit and positive definite (cholesky; 17 of
    the 448 states have a singular M, see _mass_properties); the kinetic
    identity against sg_get_energy.  The seventh case is gripper 3 with every hinge's anchor off its body's origin.
    Measured on the MI355X, worst over the cases, in units of the bound: M 4.7e-4, bias 9.2e-3, passive 8.2e-4,
    actuator 7.1e-3, inverse 3.8e-3; the kinetic identity 1.2e-14 relative"""
    import contacts_ref as CR
    m, qpos, qvel, ks, jids, tids, act, qacc = SR.sweep(gripper, tmp_path, offset)
    refs = SR.sweep_refs(gripper, tmp_path, offset)
    b = _state_batch(m, qpos, qvel, act, ks, jids, tids)
    got = _host(_all(b, _T(b, qacc)))
    energy = b.energy().cpu().numpy()
    what = "gripper %d%s" % (gripper, " with offset anchors" if offset else "")
    worst = _against_reference(got, refs, what)
    ke, singular = _mass_properties(got, refs, qvel, energy, what)
    print("%s: %d bodies, %d dofs, %d states, %d of them with a singular M; in units of the bound %s; kinetic identity %.2e"
          % (what, m.nbody, m.nv, len(ks), singular, {k: "%.2e" % v for k, v in worst.items()}, ke))
    assert singular == SWEEP_SINGULAR[gripper, offset]
    assert len(ks) == CR.SWEEP_POSES == 64 and len(DR.SWEEP_CASES) == CR.SWEEP_GRIPPERS + 1


@pytest.mark.parametrize("scene", sorted(DR.SCENES))
def test_scenes_match_the_oracle(scene):
    """the five scenes, three envs of distinct stiffness at the oracle's states a squeeze in (dyn_ref.states), put into the batch with
    sg_set_state: M against the oracle's qM and bias against its qfrc_bias after dyn_ref.oracle_forward, every output against the
    reference, M's properties.  Measured on the MI355X, in units of the bound: against the oracle M <= 8.3e-4, bias <= 8.3e-4; against the reference <= 1.5e-3"""
    from oracle import oracle as O
    m, om, sts = DR.states(scene)
    _, jids, tids, nu = DR.SCENES[scene]
    rs = np.random.RandomState(78)
    act, qacc = rs.uniform(-1.0, 1.0, (len(sts), m.nu)), np.stack([SR.QACC_SCALES[e % 3] * rs.standard_normal(m.nv) for e in range(len(sts))])
    qpos, qvel, ks = np.stack([s["qpos"] for s in sts]), np.stack([s["qvel"] for s in sts]), [s["k"] for s in sts]
    b = _state_batch(m, qpos, qvel, act, ks, jids, tids)
    got = _host(_all(b, _T(b, qacc)))
    sim = O.OracleSim(om)
    refs, worst = [], dict(M=0.0, bias=0.0)
    for e, st in enumerate(sts):
        kj, kt = DR.stiffness(m, scene, st["k"])
        DR.oracle_forward(sim, st["qpos"], st["qvel"], kj, kt)
        for name, orc in (("M", sim.qM), ("bias", sim.qfrc_bias)):
            dev = DR.close(got[name][e], orc)
            worst[name] = max(worst[name], dev)
            assert dev <= 1.0, (scene, e, name, dev)
        refs.append(SR.reference(m, st["qpos"], st["qvel"], kj, kt, act[e], qacc[e]))
    wr = _against_reference(got, refs, scene)
    ke, singular = _mass_properties(got, refs, qvel, b.energy().cpu().numpy(), scene)
    assert singular == 0
    print(scene, "against the oracle", {k: "%.2e" % v for k, v in worst.items()}, "against the reference", {k: "%.2e" % v for k, v in wr.items()},
          "kinetic identity %.2e" % ke)


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


def _raw(b, ids, n_ids, out, qacc):
    """the three entry points with any output left out (None -> NULL)"""
    from softgrip_amd.native import _ptr
    arr = None if ids is None else np.ascontiguousarray(ids, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    L, s = b.L, b._stream()
    b._check(L.sg_get_mass_matrix(b.ptr, arr, n_ids, _ptr(out.get("M")), s))
    b._check(L.sg_get_joint_forces(b.ptr, arr, n_ids, _ptr(out.get("bias")), _ptr(out.get("passive")), _ptr(out.get("actuator")), s))
    b._check(L.sg_inverse_dynamics(b.ptr, arr, n_ids, _ptr(qacc), _ptr(out.get("inverse")), s))


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


def test_listing_and_determinism():
    """softbox_fix, 9 envs a squeeze in: env_ids as a subset, a permutation and with a repeated id reproduce the rows of the all-env
    call bit for bit (qacc rows follow the list); two calls give the same bits; outputs passed as NULL in any combination leave the
    others' bits as they are; the 64 sentinels before and after every output buffer are untouched; an env id out of range is refused"""
    from softgrip_amd import native
    torch = _torch()
    ks = np.linspace(300, 1400, 9)
    m, b = _squeezed("softbox_fix", ks)
    st = b.get_state()
    assert float(st["qvel"].abs().max()) > 1e-3 and float(st["act"].abs().max()) > 1e-3, "the state must move and pull"
    qacc = _T(b, np.random.RandomState(5).standard_normal((9, m.nv)))
    full = _all(b, qacc)
    again = _all(b, qacc)
    for name in full:
        assert _same_bits(full[name], again[name]), name
        assert bool(torch.isfinite(full[name]).all()), name
    for ids in ([4, 1], [8, 3, 0, 6, 2, 7, 1, 5, 4], [2, 2, 5], [7]):
        sel = torch.as_tensor(ids, device=b.device)
        part = _all(b, qacc[sel].contiguous(), ids)
        for name in full:
            assert _same_bits(part[name], full[name][sel]), (ids, name)
    for r in range(1, len(FRC)):
        for keep in itertools.combinations(FRC, r):
            bufs, out = _guarded(full, keep)
            _raw(b, None, b.n, out, qacc)
            for n in keep:
                assert _same_bits(out[n], full[n]), (keep, n)
            assert _guards_intact(bufs), keep
    _raw(b, None, b.n, {}, qacc)      # every output NULL: nothing to write, no error
    bufs, out = _guarded(full, tuple(full))
    _raw(b, None, b.n, out, qacc)
    for n in full:
        assert _same_bits(out[n], full[n]), n
    assert _guards_intact(bufs)
    bufs, out = _guarded({n: x[:2] for n, x in full.items()}, tuple(full))      # a partial list writes its rows and nothing behind them
    _raw(b, [6, 3], 2, out, qacc[torch.as_tensor([6, 3], device=b.device)].contiguous())
    for n in full:
        assert _same_bits(out[n], full[n][torch.as_tensor([6, 3], device=b.device)]), n
    assert _guards_intact(bufs)
    bad = np.array([0, 9], np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    from softgrip_amd.native import _ptr
    for fn, args in (("sg_get_mass_matrix", (None,)), ("sg_get_joint_forces", (None, None, None)), ("sg_inverse_dynamics", (_ptr(qacc), None))):
        assert getattr(b.L, fn)(b.ptr, bad, 2, *args, None) == native.SG_ERR_INVALID
        assert b.L.sg_last_error().startswith(fn.encode() + b": env id 9 out of range"), b.L.sg_last_error()
        assert getattr(b.L, fn)(b.ptr, None, 3, *args, None) == native.SG_ERR_INVALID      # (NULL ids need n_ids == n_envs)


def test_error_paths_write_nothing():
    """NULL qacc, n_ids <= 0, an env id out of range and a NULL-ids count that is not the batch's: SG_ERR_INVALID under the entry point's
    own name before the device is touched -- every output buffer keeps its sentinels"""
    from softgrip_amd import native
    from softgrip_amd.native import _ptr
    torch = _torch()
    m, b = _squeezed("softbox_fix", np.linspace(300, 1400, 3), nsteps=1)
    kw = dict(dtype=torch.float64, device=b.device)
    out = dict(M=torch.full((3, m.nv, m.nv), SENTINEL, **kw), inverse=torch.full((3, m.nv), SENTINEL, **kw))
    out.update({n: torch.full((3, m.nv), SENTINEL, **kw) for n in FRC})
    qacc = torch.zeros(3, m.nv, **kw)
    L, s = b.L, b._stream()
    ids = lambda *a: np.array(a, np.int32).ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    assert L.sg_inverse_dynamics(b.ptr, None, 3, None, _ptr(out["inverse"]), s) == native.SG_ERR_INVALID
    assert L.sg_last_error().startswith(b"sg_inverse_dynamics:") and b"qacc" in L.sg_last_error()
    for arr, n in ((None, 0), (None, -1), (ids(0, 3), 2), (ids(-1), 1), (None, 2)):
        calls = (("sg_get_mass_matrix", lambda: L.sg_get_mass_matrix(b.ptr, arr, n, _ptr(out["M"]), s)),
                 ("sg_get_joint_forces", lambda: L.sg_get_joint_forces(b.ptr, arr, n, _ptr(out["bias"]), _ptr(out["passive"]), _ptr(out["actuator"]), s)),
                 ("sg_inverse_dynamics", lambda: L.sg_inverse_dynamics(b.ptr, arr, n, _ptr(qacc), _ptr(out["inverse"]), s)))
        for name, call in calls:
            assert call() == native.SG_ERR_INVALID, (name, n)
            assert L.sg_last_error().startswith(name.encode() + b":"), L.sg_last_error()
    torch.cuda.synchronize()
    for n, x in out.items():
        assert bool((x == SENTINEL).all()), n


def test_nan_envs_get_nan_and_disturb_no_other():
    """a NaN planted in env 1's qvel and in env 3's qpos, an inf in env 4's qvel: NaN everywhere in those envs' rows of every output (M's
    every entry), unchanged bits in the others'.  A NaN in env 2's qacc row alone: NaN in that env's qfrc_inverse, every other row as it was"""
    torch = _torch()
    ks = np.linspace(300, 1400, 6)
    m, b = _squeezed("freeball_fix", ks, nsteps=3)
    qacc = _T(b, np.random.RandomState(6).standard_normal((6, m.nv)))
    clean = _all(b, qacc)
    qbad = qacc.clone()
    qbad[2, 7] = float("nan")
    inv = b.inverse_dynamics(qbad)
    for e in range(6):
        assert bool(torch.isnan(inv[e]).all()) if e == 2 else _same_bits(inv[e], clean["inverse"][e]), e
    st = b.get_state()
    st["qvel"][1, 17] = float("nan")
    st["qpos"][3, 5] = float("nan")
    st["qvel"][4, 0] = float("inf")
    b.set_state(qpos=st["qpos"], qvel=st["qvel"])
    got = _all(b, qacc)
    for name, x in got.items():
        for e in range(6):
            if e in (1, 3, 4):
                assert bool(torch.isnan(x[e]).all()), (name, e)
            else:
                assert _same_bits(x[e], clean[name][e]), (name, e)


def test_stiffness_is_read_in_stream_order():
    """sg_set_stiffness with a DEVICE k on the same stream, then sg_get_joint_forces: passive is the reference's at the new k (and was
    at the old k before), bias and actuator keep their bits"""
    from softgrip_amd.native import _ptr
    torch = _torch()
    scene = "softbox_fix"
    k_old, k_new = np.array([640.0, 300.0, 1400.0, 512.25]), np.array([350.0, 1225.0, 777.0, 901.5])
    m, b = _squeezed(scene, k_old, nsteps=5)
    _, jids, tids, _ = DR.SCENES[scene]
    st = {k: v.cpu().numpy() for k, v in b.get_state().items()}
    kd = torch.tensor(k_new, dtype=torch.float64, device=b.device)
    ja, ta = (C.c_int * len(jids))(*jids), (C.c_int * len(tids))(*tids)
    f_old = b.joint_forces()
    b._check(b.L.sg_set_stiffness(b.ptr, _ptr(kd), 0, ja, len(jids), ta, len(tids), b._stream()))
    f_new = b.joint_forces()
    for ks, got in ((k_old, f_old), (k_new, f_new)):
        for e in range(4):
            ref = SR.reference(m, st["qpos"][e], st["qvel"][e], *DR.stiffness(m, scene, ks[e]), st["act"][e])
            assert DR.close(got["passive"][e].cpu().numpy(), ref["passive"]) <= 1.0, (e, ks[e])
    assert _same_bits(f_old["bias"], f_new["bias"]) and _same_bits(f_old["actuator"], f_new["actuator"])
    assert not _same_bits(f_old["passive"], f_new["passive"])


# ---- the body limit (SGS_MAXBODY, csrc/sg_smooth.h) on the device ----
def test_body_limit_is_reached_on_the_device(tmp_path):
    """449 bodies, SGS_MAXBODY: gripper 1 of the sweep (on a free joint) padded with jointless children of its static body, as
    tests/test_gpu_dyn.py pads it -- the launch asks for 108 120 B of dynamic LDS, above the 64 KB a launch gets without the attribute,
    and one body gathers ~400 children.  Two envs -- a swept pose and the rest pose, qvel of scale 1 -- match the reference at the
    sweep's bounds.  Measured on the MI355X: 398 children of one body, <= 3.4e-4 of the bound"""
    import test_gpu_dyn as TD
    m = TD._padded(tmp_path, SR.MAXBODY)
    jids, tids = DR.sweep_ids(m)
    q, v, ks = TD._padded_states(m, tmp_path)
    rs = np.random.RandomState(9)
    act, qacc = rs.uniform(-1.0, 1.0, (2, m.nu)), rs.standard_normal((2, m.nv))
    b = _state_batch(m, q, v, act, ks, jids, tids)
    got = _host(_all(b, _T(b, qacc)))
    refs = [SR.reference(m, q[e], v[e], *DR.stiffness(m, None, ks[e], jids, tids), act[e], qacc[e]) for e in range(2)]
    worst = _against_reference(got, refs, "%d bodies" % SR.MAXBODY)
    assert _mass_properties(got, refs, v, b.energy().cpu().numpy(), "%d bodies" % SR.MAXBODY)[1] == 0
    widest = int(np.bincount(np.asarray(m.body_parentid)[1:]).max())
    print("%d bodies, %d of them children of one body: %s" % (m.nbody, widest, {k: "%.2e" % x for k, x in worst.items()}))
    assert widest > 6 * 64 and 8 * (29 * m.nbody + 7 * m.nv + 2 * m.ntendon) > 65536


def test_one_body_beyond_the_limit_is_refused(tmp_path):
    """450 bodies: each of the three entry points returns SG_ERR_MODEL under its own name with "more than 449 bodies" and writes
    nothing (sentinels), and sg_get_poses of the same batch still answers correctly"""
    import test_gpu_dyn as TD
    from softgrip_amd import native
    from softgrip_amd.native import _ptr
    torch = _torch()
    m = TD._padded(tmp_path, SR.MAXBODY + 1)
    jids, tids = DR.sweep_ids(m)
    q, v, ks = TD._padded_states(m, tmp_path)
    b = _state_batch(m, q, v, np.zeros((2, m.nu)), ks, jids, tids)
    kw = dict(dtype=torch.float64, device=b.device)
    out = dict(M=torch.full((2, m.nv, m.nv), SENTINEL, **kw), inverse=torch.full((2, m.nv), SENTINEL, **kw))
    out.update({n: torch.full((2, m.nv), SENTINEL, **kw) for n in FRC})
    qacc = torch.zeros(2, m.nv, **kw)
    L, s = b.L, b._stream()
    calls = (("sg_get_mass_matrix", lambda: L.sg_get_mass_matrix(b.ptr, None, 2, _ptr(out["M"]), s)),
             ("sg_get_joint_forces", lambda: L.sg_get_joint_forces(b.ptr, None, 2, _ptr(out["bias"]), _ptr(out["passive"]), _ptr(out["actuator"]), s)),
             ("sg_inverse_dynamics", lambda: L.sg_inverse_dynamics(b.ptr, None, 2, _ptr(qacc), _ptr(out["inverse"]), s)))
    for name, call in calls:
        assert call() == native.SG_ERR_MODEL, name
        msg = L.sg_last_error()
        assert msg.startswith(name.encode() + b":") and b"more than %d bodies" % SR.MAXBODY in msg, (name, msg)
    torch.cuda.synchronize()
    for n, x in out.items():
        assert bool((x == SENTINEL).all()), n
    TD._against_kinematics(m, {k: x.cpu().numpy() for k, x in b.poses().items()}, q, "%d bodies" % (SR.MAXBODY + 1))
