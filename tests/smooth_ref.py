"""Helpers of the mass-matrix / joint-force / inverse-dynamics read-out tests (sg_get_mass_matrix, sg_get_joint_forces,
sg_inverse_dynamics; csrc/sg_smooth.h), on top of tests/dyn_ref.py:

  * reference(): a NumPy (fp64) restatement written from the definitions, NOT from the header: one Jacobian column per dof
    (dyn_ref.dof_columns / moved_by / point_jac).  M is the sum over bodies of m Jp' Jp + Jr' R I R' Jr plus the armature; passive and
    actuator apply the tendons' scalar forces through tendon Jacobians built from the same columns; bias differentiates the columns in
    time analytically (d/dt u = W x u, d/dt (x - anchor) = v_x - v_anchor) and projects every body's m a_com and I al + w x I w through
    its Jacobians -- no recursion over parents anywhere, where the header has two; inverse = M qacc + bias - passive;
  * build_host() / host(): the g++ build of csrc/sg_smooth.h run serially, body by body and dof by dof, as the kernel's lanes run it
    (sgs_host_env of csrc/sg_readout_host.h, on the tables csrc/sg_tables.cpp builds of the model's blob); patch= builds a header with one piece of arithmetic broken (the tests that show the tests bite).
"""
import ctypes as C

import numpy as np

import dyn_ref as DR
import readout_host as RH
from softgrip_amd.mjcf import JNT_FREE, WRAP_JOINT

MAXBODY, MAXDOF, MAXTENDON = 449, 1024, 128      # SGS_MAXBODY, SGS_MAXDOF, SGS_MAXTENDON of csrc/sg_smooth.h
NAMES = ("M", "bias", "passive", "actuator")


def tendon_jac(m, ref, cols, mv):
    """[ntendon, nv]: the gradient of reference()'s tendon lengths (a segment shorter than 1e-15 has none)"""
    J = np.zeros((m.ntendon, m.nv))
    sx = ref["site_xpos"]
    for t in range(m.ntendon):
        a, n = m.tendon_adr[t], m.tendon_num[t]
        if m.wrap_type[a] == WRAP_JOINT:
            for w in range(a, a + n):
                J[t, m.jnt_dofadr[m.wrap_objid[w]]] += m.wrap_prm[w]
            continue
        for w in range(a, a + n - 1):
            s0, s1 = m.wrap_objid[w], m.wrap_objid[w + 1]
            d = sx[s1] - sx[s0]
            ln = np.linalg.norm(d)
            if ln >= 1e-15:
                J[t] += (d / ln) @ (DR.point_jac(cols, mv[m.site_bodyid[s1]], sx[s1]) - DR.point_jac(cols, mv[m.site_bodyid[s0]], sx[s0]))
    return J


def reference(m, qpos, qvel, kj=None, kt=None, act=None, qacc=None):
    """dict: M [nv, nv], bias, passive, actuator [nv], inverse [nv] (with qacc; act None: zero); passive_spring, the springs of joints
    and tendons alone (no damper); ten_J [ntendon, nv]; dyn: dyn_ref.reference()'s dict"""
    qpos, qvel = np.asarray(qpos, np.float64), np.asarray(qvel, np.float64)
    ref = DR.reference(m, qpos, qvel, kj, kt)
    kin = ref["kin"]
    cols = DR.dof_columns(m, kin)
    rot, axis, anchor, body = cols
    mv = DR.moved_by(m, body)
    nv, nb = m.nv, m.nbody
    kj = np.asarray(m.jnt_stiffness, np.float64) if kj is None else kj
    kt = np.asarray(m.tendon_stiffness, np.float64) if kt is None else kt
    g = np.asarray(m.opt_gravity, np.float64)
    arm = np.asarray(m.dof_armature, np.float64)
    # ---- per dof: W, the angular velocity of the frame its axis is fixed in (after its joint), and the velocity of its anchor as a
    # point carried by the dofs before it
    idx = np.arange(nv)
    jnt = np.zeros(nv, int)
    for j in range(m.njnt):
        jnt[m.jnt_dofadr[j]:m.jnt_dofadr[j] + (6 if m.jnt_type[j] == JNT_FREE else 1)] = j
    W, vA = np.zeros((nv, 3)), np.zeros((nv, 3))
    for d in range(nv):
        chain = mv[body[d]]
        # (a free joint's angular axes all turn with the body, so with all three of its angular dofs; its linear axes are the world's
        # and turn with nothing of the joint)
        upto = chain & ((idx <= d) | (jnt == jnt[d])) if rot[d] or m.jnt_type[jnt[d]] != JNT_FREE else chain & (jnt < jnt[d])
        W[d] = (axis * (rot & upto)[:, None]).T @ qvel
        vA[d] = DR.point_jac(cols, chain & (idx < d), anchor[d]) @ qvel
    udot = np.cross(W, axis)
    M, bias = np.diag(arm).copy(), np.zeros(nv)
    for b in range(1, nb):
        x, vx, w = ref["xipos"][b], ref["com_lin"][b], ref["ang"][b]
        mass = m.body_mass[b]
        R = kin["xmat"][b]
        Iw = R @ np.reshape(m.body_imat[b], (3, 3)) @ R.T
        Jp = DR.point_jac(cols, mv[b], x)
        Jr = (axis * (rot & mv[b])[:, None]).T
        M += mass * Jp.T @ Jp + Jr.T @ Iw @ Jr
        # d/dt of the columns, times qvel: the acceleration of the centre of mass and the angular acceleration at qacc = 0
        cdot = np.where(rot[:, None], np.cross(udot, x[None] - anchor) + np.cross(axis, vx[None] - vA), udot) * mv[b][:, None]
        a_com = cdot.T @ qvel - g
        al = (udot * (rot & mv[b])[:, None]).T @ qvel
        f, n = mass * a_com, Iw @ al + np.cross(w, Iw @ w)
        bias += Jp.T @ f + Jr.T @ n
    # ---- springs, dampers, tendons, actuators
    J = tendon_jac(m, ref, cols, mv)
    spring = np.zeros(nv)
    for j in range(m.njnt):
        if m.jnt_type[j] != JNT_FREE:
            spring[m.jnt_dofadr[j]] = -kj[j] * (qpos[m.jnt_qposadr[j]] - m.qpos_spring[m.jnt_qposadr[j]])
    damp = -np.asarray(m.dof_damping, np.float64) * qvel
    f_ts = -kt * (ref["length"] - m.tendon_lengthspring)
    f_td = -np.asarray(m.tendon_damping, np.float64) * ref["velocity"]
    passive = spring + damp + J.T @ (f_ts + f_td)
    act = np.zeros(m.nu) if act is None else np.asarray(act, np.float64)
    actuator = np.zeros(nv)
    for u in range(m.nu):
        t, gear, b3 = m.actuator_trnid[u], m.actuator_gear[u], np.reshape(m.actuator_bias, (-1, 3))[u]
        terms = np.array([m.actuator_gain[u] * act[u], b3[0], b3[1] * gear * ref["length"][t], b3[2] * gear * ref["velocity"][t]])
        actuator += gear * J[t] * terms.sum()
    out = dict(M=M, bias=bias, passive=passive, actuator=actuator, passive_spring=spring + J.T @ f_ts, ten_J=J, dyn=ref)
    if qacc is not None:
        qacc = np.asarray(qacc, np.float64)
        out["inverse"] = M @ qacc + bias - passive
    return out


# ---- the sweep of dyn_ref with an activation and an acceleration per state ----
QACC_SCALES = (0.0, 1.0, 1000.0)      # state i's qacc is QACC_SCALES[(i // 3) % 3] N(0, 1) per dof: every scale meets every velocity scale
SWEEP_ACC_SEED = 9100
USABLE_ORACLE_STATES = 447            # of the sweep's 448 states: those on which sgo_forward raises no warning (counted on the CPU)
_SWEEP = {}


def sweep(gripper, tmpdir, offset=False):
    """dyn_ref.sweep()'s (model, qpos, qvel, k, joint ids, tendon ids) and, seeded per gripper, act [n, nu] in U(-1, 1) and qacc [n, nv];
    drawn once, shared and left unchanged"""
    if (gripper, offset) not in _SWEEP:
        base = DR.sweep(gripper, tmpdir, offset)
        m, n = base[0], len(base[3])
        rs = np.random.RandomState(SWEEP_ACC_SEED + gripper)
        act = rs.uniform(-1.0, 1.0, (n, m.nu))
        qacc = np.stack([QACC_SCALES[(i // 3) % 3] * rs.standard_normal(m.nv) for i in range(n)])
        _SWEEP[gripper, offset] = base + (act, qacc)
    return _SWEEP[gripper, offset]


_SWEEP_REFS = {}


def sweep_refs(gripper, tmpdir, offset=False):
    """reference() on every state of sweep(): computed once, shared and left unchanged"""
    if (gripper, offset) not in _SWEEP_REFS:
        m, qpos, qvel, ks, jids, tids, act, qacc = sweep(gripper, tmpdir, offset)
        _SWEEP_REFS[gripper, offset] = [reference(m, qpos[e], qvel[e], *DR.stiffness(m, None, ks[e], jids, tids), act[e], qacc[e]) for e in range(len(ks))]
    return _SWEEP_REFS[gripper, offset]


# ---- the g++ build of csrc/sg_smooth.h: sgs_host_env of csrc/sg_readout_host.h through tests/readout_host.py's shim ----
# the four arithmetic-only breaks of csrc/sg_smooth.h (name -> header, text to replace, its replacement); each text occurs exactly once
BREAKS = {
    "gyroscopic term dropped": ("sg_smooth.h", "nl[k] = Ia[k] + t1[k];", "nl[k] = Ia[k];"),
    "free angular columns in world axes": ("sg_smooth.h", "const double u[3] = {R[k], R[3 + k], R[6 + k]};",
                                           "const double u[3] = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0};"),
    "tendon damper sign flipped": ("sg_smooth.h", "- SD[s.tdamp + t] * Ld;", "+ SD[s.tdamp + t] * Ld;"),
    "armature left out of M": ("sg_smooth.h", "if (c == i) val += DD[d.arm + i];", ""),
}


def build_host(tmpdir, patch=None):
    """the ctypes library with smooth_host.  patch: a key of BREAKS -- the header is compiled from a copy with that one replacement made"""
    return RH.build(tmpdir, BREAKS, patch)


def host(L, m, scene, qpos, qvel, k, jids=None, tids=None, act=None, qacc=None):
    """the host build's outputs for one env at stiffness k (None: no joint or tendon is listed): dict of M, bias, passive, actuator and,
    with qacc, inverse.  jids / tids as in dyn_ref.stiffness()"""
    jids, tids = DR._ids(scene, jids, tids)
    kmj, kmt = np.zeros(m.njnt, np.int32), np.zeros(max(m.ntendon, 1), np.int32)
    if k is not None:
        kmj[jids] = 1
        kmt[tids] = 1
    nv = m.nv
    out = dict(M=np.full((nv, nv), np.nan), bias=np.zeros(nv), passive=np.zeros(nv), actuator=np.zeros(nv))
    if qacc is not None:
        out["inverse"] = np.zeros(nv)
    p = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)  # noqa: E731
    c = lambda x: None if x is None else np.ascontiguousarray(x, np.float64)  # noqa: E731
    q, v, a, acc = c(qpos), c(qvel), c(np.zeros(max(m.nu, 1)) if act is None else act), c(qacc)
    RH.call(L.smooth_host, RH.tables(L, m), p(q), p(v), p(a), p(acc), C.c_double(0.0 if k is None else k), p(kmj), p(kmt), p(out["M"]), p(out["bias"]),
            p(out["passive"]), p(out["actuator"]), p(out.get("inverse")))
    return out


def limits(L):
    out = np.zeros(7, np.int32)
    L.smooth_limits(out.ctypes.data_as(C.c_void_p))
    return dict(zip(("maxbody", "maxdof", "maxtendon", "static_lds", "lds_max", "rec", "dof"), (int(x) for x in out)))
