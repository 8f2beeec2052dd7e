"""Helpers of the point read-out tests (sg_get_point_motion, sg_get_jacobians; csrc/sg_point.h), on top of tests/dyn_ref.py:

  * reference(): a NumPy (fp64) restatement written from the definitions, NOT from the header: one Jacobian column per dof
    (dyn_ref.dof_columns / moved_by / point_jac).  J is those columns at the point, vel = J qvel, acc = J qacc + Jdot qvel with the
    columns differentiated in time analytically (d/dt u = W x u, d/dt (x - anchor) = v_x - v_anchor, as smooth_ref does for bias) --
    no recursion over parents anywhere, where the header's walk is one; gyro and accel turn velocity and acceleration less gravity
    into the probe's frame;
  * points(): the point lists the tests use -- the model's sites, every body's centre of mass, the world body, seeded random points
    with unnormalised quaternions;
  * build_host() / host(): the g++ build of csrc/sg_point.h run serially, body by body and point by point, as the kernel's lanes run
    it (sgp_host_env of csrc/sg_readout_host.h, on the tables csrc/sg_tables.cpp builds of the model's blob); patch= builds a header with one piece of arithmetic broken (the tests that show the tests bite).
"""
import ctypes as C

import numpy as np

import dyn_ref as DR
import readout_host as RH
from softgrip_amd.mjcf import JNT_FREE, SENS_ACCELEROMETER, SENS_GYRO, quat_to_mat

MAXBODY, MAXDOF = 672, 1024      # SGP_MAXBODY, SGP_MAXDOF of csrc/sg_point.h
MOTION = ("pos", "mat", "vel", "acc", "gyro", "accel")
NAMES = MOTION + ("jacp", "jacr")
PLAIN = ("pos", "mat", "vel", "gyro", "jacp", "jacr")      # held to dyn_ref.ARR max(1, max |value|) per array
SUMS = ("acc", "accel")                                      # sums of |qacc| r terms that cancel: held to acc_scale()
WIDTH = dict(pos=3, mat=9, vel=6, acc=6, gyro=3, accel=3)


# ---- the points ----
def site_points(m):
    """the model's sites as points: (body [nsite], pos [nsite, 3], quat [nsite, 4])"""
    return (np.asarray(m.site_bodyid, np.int32).reshape(-1), np.asarray(m.site_pos, np.float64).reshape(-1, 3),
            np.asarray(m.site_quat, np.float64).reshape(-1, 4))


def points(m, seed=31, nrandom=12):
    """(body, pos, quat, groups): the sites; every body's body_ipos (identity frame), the world included; a point off the world's origin
    in a turned frame; nrandom seeded points on random bodies at U(-0.1, 0.1) with quaternions of N(0, 1) components times 3, so none
    is normalised.  groups: name -> slice"""
    rs = np.random.RandomState(seed)
    sb, sp, sq = site_points(m)
    ident = np.array([1.0, 0, 0, 0])
    nb = m.nbody
    body = [sb, np.arange(nb, dtype=np.int32), np.zeros(1, np.int32), rs.randint(0, nb, nrandom).astype(np.int32)]
    pos = [sp, np.asarray(m.body_ipos, np.float64).reshape(nb, 3), np.array([[0.1, -0.2, 0.3]]), rs.uniform(-0.1, 0.1, (nrandom, 3))]
    quat = [sq, np.tile(ident, (nb, 1)), np.array([[0.5, -1.0, 0.25, 2.0]]), 3.0 * rs.standard_normal((nrandom, 4))]
    groups, at = {}, 0
    for name, b in zip(("sites", "com", "world", "random"), body):
        groups[name] = slice(at, at + len(b))
        at += len(b)
    return np.concatenate(body), np.concatenate(pos), np.concatenate(quat), groups


def sensor_channels(m):
    """[(sensordata address, site, 'gyro' | 'accel')] of the model's gyros and accelerometers"""
    kinds = {SENS_GYRO: "gyro", SENS_ACCELEROMETER: "accel"}
    return [(int(m.sensor_adr[s]), int(m.sensor_objid[s]), kinds[int(m.sensor_type[s])]) for s in range(len(m.sensor_type)) if int(m.sensor_type[s]) in kinds]


# ---- the NumPy reference ----
def reference(m, qpos, qvel, qacc, body, pos, quat=None):
    """dict over the P points: pos [P, 3], mat [P, 9], vel [P, 6], acc [P, 6], gyro [P, 3], accel [P, 3], jacp, jacr [P, 3, nv].
    qacc None: zero"""
    qpos, qvel = np.asarray(qpos, np.float64), np.asarray(qvel, np.float64)
    nv = m.nv
    qacc = np.zeros(nv) if qacc is None else np.asarray(qacc, np.float64)
    kin = m.kinematics(qpos)
    cols = DR.dof_columns(m, kin)
    rot, axis, anchor, dbody = cols
    mv = DR.moved_by(m, dbody)
    g = np.asarray(m.opt_gravity, np.float64)
    # per dof: W, the angular velocity of the frame its axis is fixed in, and the velocity of its anchor as a point carried by the dofs
    # before it (a free joint's angular axes turn with all three of its angular dofs, its linear axes are the world's)
    idx = np.arange(nv)
    jnt = np.zeros(nv, int)
    for j in range(m.njnt):
        jnt[m.jnt_dofadr[j]:m.jnt_dofadr[j] + (6 if m.jnt_type[j] == JNT_FREE else 1)] = j
    W, vA = np.zeros((nv, 3)), np.zeros((nv, 3))
    for d in range(nv):
        chain = mv[dbody[d]]
        upto = chain & ((idx <= d) | (jnt == jnt[d])) if rot[d] or m.jnt_type[jnt[d]] != JNT_FREE else chain & (jnt < jnt[d])
        W[d] = (axis * (rot & upto)[:, None]).T @ qvel
        vA[d] = DR.point_jac(cols, chain & (idx < d), anchor[d]) @ qvel
    udot = np.cross(W, axis)
    P = len(body)
    out = dict(pos=np.zeros((P, 3)), mat=np.zeros((P, 9)), vel=np.zeros((P, 6)), acc=np.zeros((P, 6)), gyro=np.zeros((P, 3)), accel=np.zeros((P, 3)),
               jacp=np.zeros((P, 3, nv)), jacr=np.zeros((P, 3, nv)))
    for p in range(P):
        b = int(body[p])
        R = kin["xmat"][b] if b else np.eye(3)
        x = (kin["xpos"][b] if b else np.zeros(3)) + R @ pos[p]
        q = np.array([1.0, 0, 0, 0]) if quat is None else np.asarray(quat[p], np.float64)
        mat = R @ quat_to_mat(q / np.linalg.norm(q))
        moved = mv[b] if b else np.zeros(nv, bool)
        jp = DR.point_jac(cols, moved, x)
        jr = (axis * (rot & moved)[:, None]).T
        w, v = jr @ qvel, jp @ qvel
        cdot = np.where(rot[:, None], np.cross(udot, x[None] - anchor) + np.cross(axis, v[None] - vA), udot) * moved[:, None]
        al = jr @ qacc + (udot * (rot & moved)[:, None]).T @ qvel
        a = jp @ qacc + cdot.T @ qvel
        out["pos"][p], out["mat"][p], out["jacp"][p], out["jacr"][p] = x, mat.reshape(9), jp, jr
        out["vel"][p], out["acc"][p] = np.concatenate([w, v]), np.concatenate([al, a])
        out["gyro"][p], out["accel"][p] = mat.T @ w, mat.T @ (a - g)
    return out


def acc_scale(sample, qacc):
    """what the bound ARR of an accelerometer sample or a point acceleration is relative to: 1 + max |sample| + max |qacc|,
    tests/test_tree_emu.py's scale for accelerometer samples (sums of |qacc| r terms that may cancel).  No |w|^2 r term: the CPU
    measurement (tests/test_point_host.py) did not need one, even at the sweep's 30 rad/s"""
    qmax = 0.0 if qacc is None or not np.size(qacc) else float(np.abs(qacc).max())
    return 1.0 + float(np.abs(sample).max()) + qmax


def deviations(got, ref, qacc, names=NAMES):
    """per output the deviation of got from ref in units of its bound: dyn_ref.close for PLAIN, ARR acc_scale() for SUMS"""
    out = {}
    for name in names:
        if name in SUMS:
            out[name] = float(np.abs(np.asarray(got[name]) - ref[name]).max() / (DR.ARR * acc_scale(ref[name], qacc)))
        else:
            out[name] = DR.close(got[name], ref[name])
    return out


# ---- the g++ build of csrc/sg_point.h: sgp_host_env of csrc/sg_readout_host.h through tests/readout_host.py's shim ----
# the arithmetic-only breaks (name -> header, text to replace, its replacement); each text occurs exactly once.  The free joint's dof
# convention lives in the walk sg_point.h takes from sg_smooth.h, so that break is made there
BREAKS = {
    "centripetal term dropped": ("sg_point.h", "acc[3 + k] = a[k] + c1[k] + c2[k] + g[k];", "acc[3 + k] = a[k] + c1[k] + g[k];"),
    "free angular columns in world axes": ("sg_smooth.h", "const double u[3] = {R[k], R[3 + k], R[6 + k]};",
                                           "const double u[3] = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0};"),
    "gravity's sign flipped in accel": ("sg_point.h", "f[k] = acc[3 + k] - g[k];", "f[k] = acc[3 + k] + g[k];"),
    "pt_quat ignored": ("sg_point.h", "  if (quat) {\n    double q[4]", "  if (quat && false) {\n    double q[4]"),
}


def build_host(tmpdir, patch=None):
    """the ctypes library with point_host.  patch: a key of BREAKS -- its header is compiled from a copy with that one replacement made"""
    return RH.build(tmpdir, BREAKS, patch)


def host(L, m, qpos, qvel, qacc, body, pos, quat=None):
    """the host build's outputs for one env: reference()'s dict.  qacc / quat None: NULL"""
    P, nv = len(body), m.nv
    out = {n: np.full((P, WIDTH[n]), np.nan) for n in MOTION}
    out.update(jacp=np.full((P, 3, nv), np.nan), jacr=np.full((P, 3, nv), np.nan))
    p = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)  # noqa: E731
    c = lambda x, dt=np.float64: None if x is None else np.ascontiguousarray(x, dt)  # noqa: E731
    q, v, a, pb, pp, pq = c(qpos), c(qvel), c(qacc), c(body, np.int32), c(pos), c(quat)
    RH.call(L.point_host, RH.tables(L, m), p(q), p(v), p(a), C.c_int(P), p(pb), p(pp), p(pq), *[p(out[n]) for n in NAMES])
    return out


def limits(L):
    out = np.zeros(6, np.int32)
    L.point_limits(out.ctypes.data_as(C.c_void_p))
    return dict(zip(("maxbody", "maxdof", "static_lds", "lds_max", "rec", "dof"), (int(x) for x in out)))
