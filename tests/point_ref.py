"""Helpers of the point read-out tests (sg_get_point_motion, sg_get_jacobians; csrc/sg_point.h), on top of tests/dyn_ref.py:

  * reference(): a NumPy (fp64) restatement written from the definitions, NOT from the header: one Jacobian column per dof
    (dyn_ref.dof_columns / moved_by / point_jac).  J is those columns at the point, vel = J qvel, acc = J qacc + Jdot qvel with the
    columns differentiated in time analytically (d/dt u = W x u, d/dt (x - anchor) = v_x - v_anchor, as smooth_ref does for bias) --
    no recursion over parents anywhere, where the header's walk is one; gyro and accel turn velocity and acceleration less gravity
    into the probe's frame;
  * points(): the point lists the tests use -- the model's sites, every body's centre of mass, the world body, seeded random points
    with unnormalised quaternions;
  * build_host() / host(): the g++ build of csrc/sg_point.h run serially, body by body and point by point, as the kernel's lanes run
    it; patch= builds a header with one piece of arithmetic broken (the tests that show the tests bite).
"""
import ctypes as C
import os
import subprocess

import numpy as np

import dyn_ref as DR
from helpers import ROOT
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


# ---- the g++ build of csrc/sg_point.h ----
HOST_DRIVER = r"""
#include <cstring>
#include <vector>
#include "sg_point.h"
// one env, serially, in the kernel's order: bodies by index (parents precede children), then the points' motion, then the Jacobians
// point by point: the chain walk that stamps the dofs, then column by column
extern "C" void point_host(const int* ko, const double* D, const int* I, const int* dof, const double* DD, const int* DI, const int* po, const int* PI,
                           const double* qpos, const double* qvel, const double* qacc, int n_pts, const int* pt_body, const double* pt_pos, const double* pt_quat,
                           double* pos, double* mat, double* vel, double* acc, double* gyro, double* accel, double* jacp, double* jacr) {
  SgKinOff o;
  SgDynOff d;
  SgPointOff pt;
  static_assert(sizeof(SgKinOff) == 22 * sizeof(int) && sizeof(SgDynOff) == 21 * sizeof(int) && sizeof(SgPointOff) == 2 * sizeof(int), "offset blocks are plain ints");
  memcpy(&o, ko, sizeof o);
  memcpy(&d, dof, sizeof d);
  memcpy(&pt, po, sizeof pt);
  std::vector<double> rec((size_t)SGP_REC * o.nbody), S((size_t)SGP_DOF * d.nv + 1, 0.0);
  sgp_world(DD, d, rec.data());
  for (int i = 1; i < o.nbody; i++) sgs_body(D, I, o, DD, d, DI + d.jdof, qpos, qvel, qacc, i, &rec[SGP_REC * I[o.bpar + i]], &rec[SGP_REC * i], S.data());
  const size_t nv = d.nv;
  for (int p = 0; p < n_pts; p++) {
    sgp_motion(DD, d, &rec[SGP_REC * pt_body[p]], pt_pos + 3 * p, pt_quat ? pt_quat + 4 * p : nullptr, pos + 3 * p, mat + 9 * p, vel + 6 * p, acc + 6 * p,
               gyro + 3 * p, accel + 3 * p);
    double P[3];
    sgp_pos(&rec[SGP_REC * pt_body[p]], pt_pos + 3 * p, P);
    sgp_mark(PI, pt, PI + pt.dpar, pt_body[p], S.data(), (double)(p + 1));
    for (int i = 0; i < d.nv; i++) {
      double jp[3], jr[3];
      sgp_jac_col(&S[SGP_DOF * i], (double)(p + 1), P, jp, jr);
      for (int r = 0; r < 3; r++) { jacp[(3 * p + r) * nv + i] = jp[r]; jacr[(3 * p + r) * nv + i] = jr[r]; }
    }
  }
}
extern "C" int point_limits(int* out) {
  out[0] = SGP_MAXBODY; out[1] = SGP_MAXDOF; out[2] = SGP_STATIC_LDS; out[3] = SGP_LDS_MAX; out[4] = SGP_REC; out[5] = SGP_DOF;
  return 6;
}
"""

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
    """compiles sg_point.h with g++ into tmpdir -> the ctypes library with point_host.  patch: a key of BREAKS -- sg_point.h and
    sg_smooth.h are compiled from copies, one of them with that one replacement made"""
    tmpdir = str(tmpdir)
    csrc = os.path.join(ROOT, "soft-grip_amd", "csrc")
    inc = [csrc]
    if patch is not None:
        tmpdir = os.path.join(tmpdir, "break_%d" % sorted(BREAKS).index(patch))
        os.makedirs(tmpdir, exist_ok=True)
        which, old, new = BREAKS[patch]
        for name in ("sg_point.h", "sg_smooth.h"):
            text = open(os.path.join(csrc, name)).read()
            if name == which:
                assert text.count(old) == 1, (patch, text.count(old))
                text = text.replace(old, new)
            with open(os.path.join(tmpdir, name), "w") as f:
                f.write(text)
        inc = [tmpdir, csrc]
    src = os.path.join(tmpdir, "point_host.cpp")
    so = os.path.join(tmpdir, "libpoint_host.so")
    with open(src, "w") as f:
        f.write(HOST_DRIVER)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC"] + [x for d in inc for x in ("-I", d)] + ["-o", so, src])
    L = C.CDLL(so)
    L.point_host.restype = None
    return L


_TABLES = {}


def point_table(m):
    """the point table as the library lays it out (sgp_build), from the model alone: per body the last dof of its nearest
    ancestor-or-self that has one, per dof the dof before it on the chain"""
    i = np.int32
    nv, nb = m.nv, m.nbody
    own = [[] for _ in range(nb)]
    for b in range(1, nb):
        for j in range(m.body_jntadr[b], m.body_jntadr[b] + m.body_jntnum[b]):
            own[b] += list(range(m.jnt_dofadr[j], m.jnt_dofadr[j] + (6 if m.jnt_type[j] == JNT_FREE else 1)))
    bdof, dpar = np.full(nb, -1, i), np.full(nv, -1, i)
    for b in range(1, nb):
        enter = bdof[m.body_parentid[b]]
        for d in own[b]:
            dpar[d], enter = enter, d
        bdof[b] = enter
    return np.array([0, nb], i), np.concatenate([bdof, dpar, np.zeros(1, i)])


def host(L, m, qpos, qvel, qacc, body, pos, quat=None):
    """the host build's outputs for one env: reference()'s dict.  qacc / quat None: NULL"""
    if id(m) not in _TABLES:
        _TABLES[id(m)] = (m,) + DR._tables(m) + (point_table(m),)
    _, K, Dn, Pt = _TABLES[id(m)]
    P, nv = len(body), m.nv
    out = {n: np.full((P, WIDTH[n]), np.nan) for n in MOTION}
    out.update(jacp=np.full((P, 3, nv), np.nan), jacr=np.full((P, 3, nv), np.nan))
    p = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)  # noqa: E731
    c = lambda x, dt=np.float64: None if x is None else np.ascontiguousarray(x, dt)  # noqa: E731
    q, v, a, pb, pp, pq = c(qpos), c(qvel), c(qacc), c(body, np.int32), c(pos), c(quat)
    L.point_host(p(K[0]), p(K[1]), p(K[2]), p(Dn[0]), p(Dn[1]), p(Dn[2]), p(Pt[0]), p(Pt[1]), p(q), p(v), p(a), C.c_int(P), p(pb), p(pp), p(pq),
                 *[p(out[n]) for n in NAMES])
    return out


def limits(L):
    out = np.zeros(6, np.int32)
    L.point_limits(out.ctypes.data_as(C.c_void_p))
    return dict(zip(("maxbody", "maxdof", "static_lds", "lds_max", "rec", "dof"), (int(x) for x in out)))
