"""Helpers of the velocity / tendon / energy read-out tests (sg_get_velocities, sg_get_tendons, sg_get_energy; csrc/sg_dyn.h):

  * reference(): a NumPy (fp64) restatement written from the definitions, NOT from the header: Model.kinematics() for the poses, one
    Jacobian column per dof (axis, anchor, the bodies it moves), velocities as column sums, energies from the bodies' masses and inertias;
  * build_host() / host(): the g++ build of csrc/sg_dyn.h run serially, body by body and wrap by wrap, as the kernel's lanes run it
    (sgd_host_env of csrc/sg_readout_host.h, on the tables csrc/sg_tables.cpp builds of the model's blob);
  * the scenes and states every test uses: a few oracle steps into a squeeze, a seeded perturbation of qvel, a stiffness per env;
  * sweep(): contacts_ref's random grippers and poses with velocities and a stiffness per state, for the g++ build and the device alike.
"""
import ctypes as C
import os

import numpy as np

import readout_host as RH
import softgrip_amd as sg
from helpers import ROOT, model_path
from softgrip_amd.mjcf import JNT_FREE, JNT_SLIDE, WRAP_JOINT

# scene -> (tendon damper, joints / tendons that take the per-env stiffness, actuators)
SCENES = {
    "mini_gripper": (None, list(range(8, 42)), [0], 2),
    "softbox_fix": (None, list(range(11, 64)), [0], 2),
    "softbox": (None, list(range(11, 64)), [0], 2),
    "fourfinger_softball_fix": ("implicit", list(range(65, 283)), [0], 4),
    "freeball_fix": ("implicit", list(range(9, 227)), [0], 2),
}
KS = [640.0, 300.0, 1400.0]      # a stiffness per env
REL = 1e-11                       # sums of <= ~300 like-sized terms: n eps ~ 7e-14, two orders of margin
ARR = 1e-12                       # per array, times max(1, max |value|): ~100 fp64 operations per body at O(1 - 10)


def load(scene):
    damper = SCENES[scene][0]
    if scene == "mini_gripper":
        m = sg.compile_mjcf(os.path.join(ROOT, "tests", "data", "mini_gripper.xml"), composite_neighbors=False)
        m.opt_implicit_tendon_damping = 0
        return m
    return sg.load_model(model_path(scene), damper)


_STATES = {}


def states(scene, nsteps=60):
    """(model, [dict(qpos, qvel, k)] per env of KS): the oracle's reset; forward; step, ctrl = -0.2, nsteps steps; then qvel gains a
    seeded perturbation of a tenth of its own scale (never changed afterwards: computed once per scene and shared)"""
    if scene not in _STATES:
        from oracle import oracle as O
        m = load(scene)
        _, jids, tids, nu = SCENES[scene]
        om = O.OracleModel(m.to_blob())
        rs = np.random.RandomState(1234)
        out = []
        for k in KS:
            s = O.OracleSim(om)
            s.jnt_stiffness[jids] = k
            s.tendon_stiffness[tids] = k
            s.reset(); s.forward(); s.step()
            s.ctrl[:] = -0.2
            for _ in range(nsteps):
                assert s.step() == 0, scene
            scale = max(np.abs(s.qvel).max(), 1e-3)
            out.append(dict(qpos=s.qpos.copy(), qvel=s.qvel + 0.1 * scale * rs.standard_normal(m.nv), k=k))
        _STATES[scene] = (m, om, out)
    return _STATES[scene]


def _ids(scene, jids, tids):
    """the joints / tendons that take the per-env stiffness: the explicit lists, or the scene's where one is None"""
    return (SCENES[scene][1] if jids is None else jids), (SCENES[scene][2] if tids is None else tids)


def stiffness(m, scene, k, jids=None, tids=None):
    """the stiffness vectors env k's next step uses: (jnt_stiffness [njnt], tendon_stiffness [ntendon]).  jids / tids: the listed joints
    and tendons (None: SCENES[scene]'s; with both given, scene may be None)"""
    jids, tids = _ids(scene, jids, tids)
    kj, kt = np.array(m.jnt_stiffness, dtype=np.float64), np.array(m.tendon_stiffness, dtype=np.float64)
    if k is not None:
        kj[jids] = k
        kt[tids] = k
    return kj, kt


# ---- the sweep of the random grippers: contacts_ref's grippers and poses, given velocities and a stiffness per env ----
SWEEP_VEL = (0.0, 1.0, 30.0)      # pose i moves at SWEEP_VEL[i % 3] N(0, 1) per dof
SWEEP_QUAT_SCALE = 1.7            # every fourth pose of a gripper on a free joint carries its free quaternion times this
SWEEP_VEL_SEED = 4100             # gripper i's velocities are drawn with seed SWEEP_VEL_SEED + its pose seed


def sweep_ids(model):
    """the joints and tendons that take the per-env stiffness in the random grippers: the sliders from the first non-hinge joint on
    (the shell's; the fingers' hinges come first), tendon 0"""
    jt = np.asarray(model.jnt_type)
    nchain = int(np.flatnonzero(jt != 3)[0])
    return [j for j in range(nchain, model.njnt) if jt[j] == JNT_SLIDE], [0]


def velocity_sweep(model, n, seed):
    """(qpos [n, nq], qvel [n, nv], k [n]): contacts_ref.pose_sweep(model, n, seed) with a state of motion.  Pose i gets qvel =
    SWEEP_VEL[i % 3] N(0, 1) (so every third pose is at rest); every fourth pose (i % 4 == 0) of a model with a free joint gets that
    joint's quaternion multiplied by SWEEP_QUAT_SCALE (kinematics normalises it; 3 and 4 are coprime, so every velocity scale meets
    one); env i's stiffness is KS[i % 3]"""
    import contacts_ref as CR
    qpos = CR.pose_sweep(model, n, seed).copy()
    rs = np.random.RandomState(SWEEP_VEL_SEED + seed)
    qvel = np.stack([SWEEP_VEL[i % 3] * rs.standard_normal(model.nv) for i in range(n)])
    for j in np.flatnonzero(np.asarray(model.jnt_type) == JNT_FREE):
        a = int(model.jnt_qposadr[j])
        qpos[::4, a + 3:a + 7] *= SWEEP_QUAT_SCALE
    return qpos, qvel, np.array([KS[i % len(KS)] for i in range(n)])


_SWEEP = {}
OFFSET_GRIPPER = 3        # the sweep's gripper that is swept a second time with its hinges' anchors moved off the body origins
OFFSET_SEED = 515


def offset_anchors(xml, seed=OFFSET_SEED):
    """the gripper's XML with every hinge given a pos of its own, U(-0.05, 0.05) per axis: random_gripper_xml leaves all joints at
    their body's origin, where a body's second and third hinge have the anchor the first one had, whatever frame it is taken in"""
    rs = np.random.RandomState(seed)
    head, parts = '<joint type="hinge" ', xml.split('<joint type="hinge" ')
    assert len(parts) > 1
    return parts[0] + "".join(head + 'pos="%.4f %.4f %.4f" ' % tuple(rs.uniform(-0.05, 0.05, 3)) + rest for rest in parts[1:])


def sweep(gripper, tmpdir, offset=False):
    """gripper `gripper` of contacts_ref's sweep and its states: (model, qpos, qvel, k, joint ids, tendon ids) -- compiled and drawn once,
    shared and left unchanged.  offset=True: the same gripper through offset_anchors(), swept with the same seeds"""
    import contacts_ref as CR
    if (gripper, offset) not in _SWEEP:
        path = os.path.join(str(tmpdir), "sweep_g%d%s.xml" % (gripper, "_offset" if offset else ""))
        xml = CR.sweep_gripper_xmls()[gripper]
        with open(path, "w") as f:
            f.write(offset_anchors(xml) if offset else xml)
        m = sg.compile_mjcf(path, composite_neighbors=False)
        _SWEEP[gripper, offset] = (m,) + velocity_sweep(m, CR.SWEEP_POSES, CR.SWEEP_POSE_SEED + gripper) + sweep_ids(m)
    return _SWEEP[gripper, offset]


SWEEP_CASES = [(g, False) for g in range(6)] + [(OFFSET_GRIPPER, True)]      # (gripper, offset anchors): what both sweep tests run


def sweep_reach(m, qpos, qvel, refs):
    """what a gripper's swept states reach, from the model and the reference's outputs alone: a dict of
    joints_per_body (set of joint counts over the bodies), slider_on_turning_body (some slider's parent body has |ang| > 1e-3 in some
    state), nonunit_free_quat (some free quaternion's norm is off 1 by more than 0.1), spatial_sites (set of site counts over the
    spatial tendons), fixed_tendon_wraps (set of wrap counts over the fixed ones), scales (set of max |qvel| per state, rounded to
    the sweep's scales), later_hinge_off_origin (some body's second or third hinge has its anchor off the body's origin)"""
    jt = np.asarray(m.jnt_type)
    out = dict(joints_per_body={int(x) for x in np.asarray(m.body_jntnum)[1:]}, slider_on_turning_body=False, nonunit_free_quat=False,
               spatial_sites=set(), fixed_tendon_wraps=set(), scales=set(), later_hinge_off_origin=False)
    for b in range(1, m.nbody):
        j0, nj = int(m.body_jntadr[b]), int(m.body_jntnum[b])
        out["later_hinge_off_origin"] |= bool(nj > 1 and (jt[j0 + 1:j0 + nj] == 3).any() and np.abs(np.asarray(m.jnt_pos)[j0 + 1:j0 + nj]).max() > 1e-3)
    for t in range(m.ntendon):
        a, n = int(m.tendon_adr[t]), int(m.tendon_num[t])
        (out["fixed_tendon_wraps"] if m.wrap_type[a] == WRAP_JOINT else out["spatial_sites"]).add(n)
    slider_parent = [int(m.body_parentid[b]) for b in range(1, m.nbody)
                     if (jt[m.body_jntadr[b]:m.body_jntadr[b] + m.body_jntnum[b]] == JNT_SLIDE).any()]
    for q, v, ref in zip(qpos, qvel, refs):
        out["slider_on_turning_body"] |= bool(slider_parent) and bool((np.abs(ref["ang"][slider_parent]).max(1) > 1e-3).any())
        for j in np.flatnonzero(jt == JNT_FREE):
            a = int(m.jnt_qposadr[j])
            out["nonunit_free_quat"] |= bool(abs(np.linalg.norm(q[a + 3:a + 7]) - 1.0) > 0.1)
        top = float(np.abs(v).max())
        out["scales"].add(0.0 if top == 0 else 1.0 if top < 8 else 30.0)
    return out


# ---- the NumPy reference ----
def dof_columns(m, kin):
    """per dof: is it a rotation, its world axis, its anchor, the body it belongs to"""
    nv = m.nv
    rot, axis, anchor, body = np.zeros(nv, bool), np.zeros((nv, 3)), np.zeros((nv, 3)), np.zeros(nv, int)
    for b in range(1, m.nbody):
        for j in range(m.body_jntadr[b], m.body_jntadr[b] + m.body_jntnum[b]):
            d = m.jnt_dofadr[j]
            if m.jnt_type[j] == JNT_FREE:
                R = kin["xmat"][b]
                for c in range(3):
                    axis[d + c, c] = 1.0
                    rot[d + 3 + c], axis[d + 3 + c], anchor[d + 3 + c] = True, R[:, c], kin["xpos"][b]
                body[d:d + 6] = b
            else:
                rot[d], axis[d], anchor[d], body[d] = m.jnt_type[j] != JNT_SLIDE, kin["xaxis"][j], kin["xanchor"][j], b
    return rot, axis, anchor, body


def moved_by(m, body):
    """[nbody, nv] bool: dof d moves body b (the dof's body is b or one of its ancestors)"""
    nb = m.nbody
    anc = np.zeros((nb, nb), bool)      # anc[b, a]: a is b or an ancestor of b
    for b in range(1, nb):
        anc[b] = anc[m.body_parentid[b]]
        anc[b, b] = True
    return anc[:, body]


def point_jac(cols, moved_row, p):
    """3 x nv translational Jacobian of the world point p on a body whose dofs are moved_row"""
    rot, axis, anchor, _ = cols
    jp = np.where(rot[:, None], np.cross(axis, p[None] - anchor), axis)
    return (jp * moved_row[:, None]).T


def reference(m, qpos, qvel, kj=None, kt=None):
    """dict: ang, lin, com_lin [nbody, 3]; length, velocity [ntendon]; energy [4] (gravity, joint springs, tendon springs, kinetic);
    and the pieces the oracle pins: xipos, site positions.  kj / kt: the stiffness vectors in force (None: the model's own)"""
    qpos, qvel = np.asarray(qpos, np.float64), np.asarray(qvel, np.float64)
    kin = m.kinematics(qpos)
    cols = dof_columns(m, kin)
    rot, axis, anchor, body = cols
    mv = moved_by(m, body)
    nb = m.nbody
    ang, lin, com_lin, xipos = np.zeros((nb, 3)), np.zeros((nb, 3)), np.zeros((nb, 3)), np.zeros((nb, 3))
    for b in range(1, nb):
        ang[b] = ((axis * rot[:, None] * mv[b][:, None]).T) @ qvel
        lin[b] = point_jac(cols, mv[b], kin["xpos"][b]) @ qvel
        xipos[b] = kin["xpos"][b] + kin["xmat"][b] @ m.body_ipos[b]
        com_lin[b] = point_jac(cols, mv[b], xipos[b]) @ qvel
    sx = m.site_xpos(kin) if m.nsite else np.zeros((0, 3))
    sv = np.array([point_jac(cols, mv[m.site_bodyid[s]], sx[s]) @ qvel for s in range(m.nsite)]).reshape(-1, 3)
    nt = m.ntendon
    length, velocity = np.zeros(nt), np.zeros(nt)
    for t in range(nt):
        a, n = m.tendon_adr[t], m.tendon_num[t]
        if m.wrap_type[a] == WRAP_JOINT:
            js = m.wrap_objid[a:a + n]
            length[t] = np.dot(m.wrap_prm[a:a + n], qpos[m.jnt_qposadr[js]])
            velocity[t] = np.dot(m.wrap_prm[a:a + n], qvel[m.jnt_dofadr[js]])
        else:
            for w in range(a, a + n - 1):
                s0, s1 = m.wrap_objid[w], m.wrap_objid[w + 1]
                d = sx[s1] - sx[s0]
                ln = np.linalg.norm(d)
                length[t] += ln
                if ln >= 1e-15:
                    velocity[t] += np.dot(d / ln, sv[s1] - sv[s0])
    kj = np.asarray(m.jnt_stiffness, np.float64) if kj is None else kj
    kt = np.asarray(m.tendon_stiffness, np.float64) if kt is None else kt
    g = np.asarray(m.opt_gravity, np.float64)
    e_grav = -float(np.sum(m.body_mass[1:] * (xipos[1:] @ g)))
    scalar = np.asarray(m.jnt_type) != JNT_FREE
    qa = np.asarray(m.jnt_qposadr)[scalar]
    e_jnt = float(np.sum(0.5 * kj[scalar] * (qpos[qa] - m.qpos_spring[qa]) ** 2))
    e_ten = float(np.sum(0.5 * kt * (length - m.tendon_lengthspring) ** 2))
    e_kin = 0.5 * float(np.sum(m.dof_armature * qvel ** 2))
    for b in range(1, nb):
        R = kin["xmat"][b]
        Iw = R @ np.reshape(m.body_imat[b], (3, 3)) @ R.T
        e_kin += 0.5 * (m.body_mass[b] * com_lin[b] @ com_lin[b] + ang[b] @ Iw @ ang[b])
    return dict(ang=ang, lin=lin, com_lin=com_lin, length=length, velocity=velocity, energy=np.array([e_grav, e_jnt, e_ten, e_kin]),
                xipos=xipos, site_xpos=sx, kin=kin)


def close(got, ref, tol=ARR):
    """|got - ref| <= tol * max(1, max |ref|) over the array; returns the largest deviation in units of that bound"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if ref.size == 0:
        return 0.0
    return float(np.abs(got - ref).max() / (tol * max(1.0, np.abs(ref).max())))


ALLOW_FIXED_TENDON = ("fourfinger_softball_fix",)      # scenes whose tendon-spring term needs energy_scale's allowance (see there)


def energy_scale(m, ref, kj, kt, qpos, qvel, allowance=False):
    """per energy term what REL is relative to: the sum of the absolute values of its summands (for the tendon springs sum 1/2 |k| x^2,
    x = L - tendon_lengthspring).
    allowance=True (the scenes of ALLOW_FIXED_TENDON only) adds, for FIXED tendons, |k| |x| sum |coef q|: what the length's own bound
    REL sum |coef q| does to 1/2 k x^2.  The four-finger scene needs it: its volume tendon is the only tendon with a stiffness, its
    length a sum of 218 cancelling coef q terms (sum |coef q| = 3e-3 .. 5e-3 m) that comes to 7e-21 .. 9e-20 m in these states, so the
    term is 1e-38 .. 6e-36 J and two correct summation orders differ by most of it (measured, g++ build against NumPy: 0.75 and 0.94
    of the term in two of three states; with the allowance at most 1.2e-17 of the scale)"""
    g = np.asarray(m.opt_gravity, np.float64)
    scalar = np.asarray(m.jnt_type) != JNT_FREE
    qa = np.asarray(m.jnt_qposadr)[scalar]
    x = ref["length"] - m.tendon_lengthspring
    e_ten = np.sum(0.5 * np.abs(kt) * x ** 2)
    if allowance:
        for t in range(m.ntendon):
            if m.wrap_type[m.tendon_adr[t]] == WRAP_JOINT:
                e_ten += abs(kt[t]) * abs(x[t]) * length_scale(m, t, qpos, ref["length"])
    return np.array([np.sum(np.abs(m.body_mass[1:] * (ref["xipos"][1:] @ g))), np.sum(0.5 * np.abs(kj[scalar]) * (qpos[qa] - m.qpos_spring[qa]) ** 2),
                     e_ten, max(ref["energy"][3], 0.0)])


def length_scale(m, t, qpos, length):
    """the sum of the absolute values of the terms of tendon t's length: |coef q| over a fixed tendon's wraps, the length itself for a
    spatial one (its segments are all positive)"""
    a, n = m.tendon_adr[t], m.tendon_num[t]
    if m.wrap_type[a] == WRAP_JOINT:
        return float(np.sum(np.abs(m.wrap_prm[a:a + n] * np.asarray(qpos)[m.jnt_qposadr[m.wrap_objid[a:a + n]]])))
    return float(length[t])


# ---- the g++ build of csrc/sg_dyn.h: sgd_host_env of csrc/sg_readout_host.h through tests/readout_host.py's shim ----
def build_host(tmpdir):
    """the ctypes library with dyn_host"""
    return RH.build(tmpdir)


def host(L, m, scene, qpos, qvel, k, jids=None, tids=None):
    """the host build's outputs for one env at stiffness k (None: no joint or tendon is listed): reference()'s dict, plus poses [nbody, 7].
    jids / tids as in stiffness()"""
    jids, tids = _ids(scene, jids, tids)
    kmj, kmt = np.zeros(m.njnt, np.int32), np.zeros(max(m.ntendon, 1), np.int32)
    if k is not None:
        kmj[jids] = 1
        kmt[tids] = 1
    nb, nt = m.nbody, m.ntendon
    out = dict(ang=np.zeros((nb, 3)), lin=np.zeros((nb, 3)), com_lin=np.zeros((nb, 3)), length=np.zeros(nt), velocity=np.zeros(nt), energy=np.zeros(4),
               poses=np.zeros((nb, 7)))
    p = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    q, v = np.ascontiguousarray(qpos, np.float64), np.ascontiguousarray(qvel, np.float64)
    RH.call(L.dyn_host, RH.tables(L, m), p(q), p(v), C.c_double(0.0 if k is None else k), p(kmj), p(kmt), p(out["ang"]), p(out["lin"]), p(out["com_lin"]),
            p(out["length"]), p(out["velocity"]), p(out["energy"]), p(out["poses"]))
    return out


def oracle_forward(sim, qpos, qvel, kj=None, kt=None):
    """the oracle's forward pass at (qpos, qvel) with the stiffness vectors in force; its views then hold qM, ten_length, sensordata"""
    sim.qpos[:], sim.qvel[:] = qpos, qvel
    if kj is not None:
        sim.jnt_stiffness[:], sim.tendon_stiffness[:] = kj, kt
    sim.forward()
    return sim


def gyro_channels(m):
    """[(sensordata address, site)] of the model's gyros (the velocity-stage sensor)"""
    from softgrip_amd.mjcf import SENS_GYRO
    return [(int(m.sensor_adr[s]), int(m.sensor_objid[s])) for s in range(len(m.sensor_type)) if m.sensor_type[s] == SENS_GYRO]


def site_xmat(m, kin, site):
    from softgrip_amd.mjcf import quat_to_mat
    return kin["xmat"][m.site_bodyid[site]] @ quat_to_mat(m.site_quat[site])


def integrate(m, qpos, qvel, h):
    """qpos moved by h qvel as mj_integratePos does: scalar joints q + h qvel; a free joint's position + h v (world), its quaternion
    q (x) exp(h w / 2), w the angular components in the body frame"""
    from softgrip_amd.mjcf import quat_mul
    q = np.array(qpos, dtype=np.float64)
    for j in range(m.njnt):
        qa, da = m.jnt_qposadr[j], m.jnt_dofadr[j]
        if m.jnt_type[j] == JNT_FREE:
            q[qa:qa + 3] += h * qvel[da:da + 3]
            w = h * np.asarray(qvel[da + 3:da + 6])
            a = np.linalg.norm(w)
            dq = np.concatenate([[np.cos(a / 2)], (np.sin(a / 2) / a) * w]) if a > 0 else np.array([1.0, 0, 0, 0])
            quat = quat_mul(q[qa + 3:qa + 7], dq)
            q[qa + 3:qa + 7] = quat / np.linalg.norm(quat)
        else:
            q[qa] += h * qvel[da]
    return q
