"""Helpers of the tests of the read-outs that start with the inverse of the mass matrix (sg_solve_mass, sg_forward_smooth,
sg_get_point_inertia; csrc/sg_solve.h), on top of tests/dyn_ref.py and tests/smooth_ref.py:

  * the reference: numpy.linalg.solve on a dense M (the oracle's qM on the scenes, smooth_ref.reference's M on the sweep), qfrc_smooth
    from smooth_ref's passive / actuator and the oracle's or the reference's bias, J from dyn_ref.point_jac;
  * tree_factor(): the level-scheduled tree factorisation M = L' D L as plain NumPy on a dense M, for the pivot figure and the
    structure counts -- written from the definition (mj_factorM's sparsity), not from the header;
  * build_host() / host(): the g++ build of csrc/sg_solve.h run serially, entry by entry and dof by dof, as the kernel's lanes run it;
    patch= builds a header with one piece of arithmetic broken (the tests that show the tests bite);
  * the bounds: the residual unit nv eps (|M| |x| + |y|) and the forward unit nv eps cond2(M) max |x_ref|, in infinity norms.
"""
import ctypes as C
import os
import subprocess

import numpy as np

import dyn_ref as DR
import smooth_ref as SR
from helpers import ROOT

EPS = 2.0 ** -53
SINGULAR = 1e-10      # test_gpu_smooth.py's criterion: smallest eigenvalue of the reference M below this fraction of the largest
# the sweep's states with a singular M, per case of dyn_ref.SWEEP_CASES, counted on the CPU from the reference alone: 17 of 448
SWEEP_SINGULAR = (4, 4, 0, 3, 3, 3, 0)
RHS_SCALES = (1.0, 1e3, 1e-3)      # right-hand side r is RHS_SCALES[r % 3] N(0, 1) per dof
# scene -> (nM, dofs per depth level) of the table at the top of DESIGN.md 8.8
STRUCTURE = {
    "mini_gripper": (54, [36, 2, 2, 2]),
    "softbox": (130, [112, 2, 2, 2]),
    "softbox_fix": (130, [112, 2, 2, 2]),
    "fourfinger_softball_fix": (779, [222] + [4] * 15 + [1]),
    "freeball_fix": (1567, [3, 3, 3, 3, 1, 1, 218]),
}


# ---- structure and the NumPy tree factorisation ----
def dof_parents(m):
    """[nv] the dof-parent chain (sgs_build's dpar) and [nv] the dofs' bodies"""
    off, _, ints = SR.smooth_table(m)
    return ints[off[8]:off[8] + m.nv].copy(), ints[off[7]:off[7] + m.nv].copy()


def structure(dpar):
    """depth [nv], ancestors (nearest first, self excluded) and descendants (ascending) per dof, nM"""
    nv = len(dpar)
    depth = np.zeros(nv, int)
    anc, desc = [], [[] for _ in range(nv)]
    for i in range(nv):
        depth[i] = 0 if dpar[i] < 0 else depth[dpar[i]] + 1
        chain, j = [], dpar[i]
        while j >= 0:
            chain.append(int(j))
            desc[j].append(i)
            j = dpar[j]
        anc.append(chain)
    return depth, anc, desc, int(depth.sum() + nv)


def tree_factor(M, dpar):
    """(L [nv, nv] unit lower triangular, D [nv]) with M = L' D L, levels from the deepest, every entry a gather over the row's
    descendants in ascending order"""
    nv = len(dpar)
    depth, anc, desc, _ = structure(dpar)
    L, D = np.eye(nv), np.zeros(nv)
    with np.errstate(all="ignore"):
        for lev in range(depth.max(), -1, -1):
            for i in np.flatnonzero(depth == lev):
                cols = [i] + anc[i]
                vals = [M[i, j] - sum(L[k, i] * D[k] * L[k, j] for k in desc[i]) for j in cols]
                D[i] = vals[0]
                for j, val in zip(cols[1:], vals[1:]):
                    L[i, j] = val / D[i]
    return L, D


def pivot_of(M, dpar):
    """min D_i / M_ii of tree_factor (NaN if any ratio is)"""
    _, D = tree_factor(M, dpar)
    with np.errstate(all="ignore"):
        r = D / np.diag(M)
    return float("nan") if np.isnan(r).any() else float(r.min())


def is_singular(M):
    ev = np.linalg.eigvalsh(M)
    return bool(ev[0] < SINGULAR * ev[-1])


# ---- the bounds ----
def residual_unit(M, x, y):
    """nv eps (|M| |x| + |y|), infinity norms; x, y [nv] or [R, nv] (per right-hand side)"""
    x, y = np.atleast_2d(x), np.atleast_2d(y)
    return len(M) * EPS * (np.abs(M).sum(1).max() * np.abs(x).max(1) + np.abs(y).max(1))


def _ratio(num, den):
    """num / den with 0 / 0 = 0 (a right-hand side of zeros, solved to zeros); a NaN anywhere stays a NaN"""
    with np.errstate(all="ignore"):
        return np.where((num == 0) & (den == 0), 0.0, num / den)


def residual_dev(M, x, y):
    """max over the right-hand sides of |M x - y| in units of residual_unit"""
    x, y = np.atleast_2d(x), np.atleast_2d(y)
    return float(_ratio(np.abs(x @ M.T - y).max(1), residual_unit(M, x, y)).max())


def cond2(M):
    ev = np.linalg.eigvalsh(M)
    return float(ev[-1] / ev[0])


def forward_dev(M, x, x_ref, floor=0.0):
    """max |x - x_ref| in units of nv eps cond2(M) max(floor, max |x_ref|) per right-hand side (rows of 2-d x; anything else as one)"""
    x, x_ref = np.asarray(x), np.asarray(x_ref)
    if x.ndim != 2:
        x, x_ref = x.reshape(1, -1), x_ref.reshape(1, -1)
    scale = np.maximum(floor, np.abs(x_ref).max(1))
    return float(_ratio(np.abs(x - x_ref).max(1), len(M) * EPS * cond2(M) * scale).max())


def pivot_dev(M, got, ref):
    return abs(got - ref) / (len(M) * EPS * cond2(M))


def smooth_unit(terms):
    """the bound of qfrc_smooth against the reference: the sum of dyn_ref.ARR max(1, max |term|) over its four terms"""
    return sum(DR.ARR * max(1.0, float(np.abs(t).max())) for t in terms)


def rhs(nv, n, seed):
    """[n, nv]: right-hand side r of scale RHS_SCALES[r % 3]"""
    rs = np.random.RandomState(seed)
    return np.stack([RHS_SCALES[r % 3] * rs.standard_normal(nv) for r in range(n)])


# ---- points and their 6 x nv Jacobians (jacr above jacp) from dyn_ref's columns ----
def points(m, seed=41, nrandom=6):
    """(body [P] int32, pos [P, 3]): the model's sites, nrandom seeded points at U(-0.1, 0.1) on random bodies other than the world
    (finger boxes and shell elements alike), and one point on body 0"""
    rs = np.random.RandomState(seed)
    body = np.concatenate([np.asarray(m.site_bodyid, np.int32).reshape(-1), rs.randint(1, m.nbody, nrandom).astype(np.int32), np.zeros(1, np.int32)])
    pos = np.concatenate([np.asarray(m.site_pos, np.float64).reshape(-1, 3), rs.uniform(-0.1, 0.1, (nrandom, 3)), [[0.3, -0.2, 0.1]]])
    return body, pos


def point_jacobians(m, qpos, body, pos):
    """[P, 6, nv]: rows 0 - 2 jacr, rows 3 - 5 jacp of the points at qpos"""
    kin = m.kinematics(np.asarray(qpos, np.float64))
    cols = DR.dof_columns(m, kin)
    rot, axis, _, dbody = cols
    mv = DR.moved_by(m, dbody)
    J = np.zeros((len(body), 6, m.nv))
    for p, (b, local) in enumerate(zip(body, pos)):
        if b == 0:
            continue
        J[p, :3] = (axis * (rot & mv[b])[:, None]).T
        J[p, 3:] = DR.point_jac(cols, mv[b], kin["xpos"][b] + kin["xmat"][b] @ local)
    return J


def reference_W(M, J):
    """[P, 6, 6] = J M^-1 J'"""
    return np.stack([Jp @ np.linalg.solve(M, Jp.T) for Jp in J])


# ---- the g++ build of csrc/sg_solve.h ----
HOST_DRIVER = r"""
#include <cmath>
#include <cstring>
#include <vector>
#include "sg_solve.h"
#include "sg_point.h"
// one right-hand side, in the kernel's order: up sweep by levels from the deepest, scaling, down sweep by levels from the roots
static void solve_rhs(const int* VI, const SgSolveOff& v, int nv, const double* F, double* x) {
  for (int L = v.nlevel - 2; L >= 0; L--)
    for (int s = VI[v.lstart + L]; s < VI[v.lstart + L + 1]; s++) { const int j = VI[v.ldof + s]; x[j] = sgv_up(VI, v, F, x, j); }
  for (int i = 0; i < nv; i++) x[i] = sgv_scale(VI, v, F, x, i);
  for (int L = 1; L < v.nlevel; L++)
    for (int s = VI[v.lstart + L]; s < VI[v.lstart + L + 1]; s++) { const int i = VI[v.ldof + s]; x[i] = sgv_down(VI, v, F, x, i); }
}
// one env, serially, in the kernel's order.  info: nM, nlevel, right-hand sides per tile, 1 if some D is not finite or not positive;
// levels[nlevel]: dofs per depth.  Mp, Fp [nM]: the packed M and the packed factor.  Returns 0, or -1 with the table's reason in err
extern "C" int solve_host(const int* ko, const double* D, const int* I, const int* dof, const double* DD, const int* DI, const int* so, const double* SD,
                          const int* SI, const double* qpos, const double* qvel, const double* act, double kenv, const int* kmask_jnt, const int* kmask_ten,
                          int n_rhs, const double* y, double* x, const double* applied, double* qacc_s, double* qfrc_s, int n_pts, const int* pt_body,
                          const double* pt_pos, double* W, double* Mp, double* Fp, double* pivot, int* info, int* levels, char* err) {
  SgKinOff o;
  SgDynOff d;
  SgSmoothOff s;
  static_assert(sizeof(SgKinOff) == 22 * sizeof(int) && sizeof(SgDynOff) == 21 * sizeof(int) && sizeof(SgSmoothOff) == 12 * sizeof(int), "offset blocks are plain ints");
  memcpy(&o, ko, sizeof o);
  memcpy(&d, dof, sizeof d);
  memcpy(&s, so, sizeof s);
  SgSolveHost V;
  sgv_build(o.nbody, I + o.bpar, d.nv, SI + s.dbody, SI + s.dpar, d.ntendon, &V);
  if (!V.ok) { strncpy(err, V.err.c_str(), 255); return -1; }
  const SgSolveOff& v = V.o;
  const int* VI = V.ints.data();
  const int nv = d.nv;
  const double qnan = NAN;
  info[0] = v.nM; info[1] = v.nlevel; info[2] = (int)sgv_tile(o.nbody, nv, d.ntendon, v.nM);
  for (int L = 0; L < v.nlevel; L++) levels[L] = VI[v.lstart + L + 1] - VI[v.lstart + L];
  std::vector<double> rec((size_t)SGS_REC * o.nbody), S((size_t)SGS_DOF * nv + 1), ften(2 * (size_t)d.ntendon + 1), F(v.nM), mdiag(nv), X(6 * (size_t)nv);
  sgs_world(DD, d, rec.data());
  for (int i = 1; i < o.nbody; i++) sgs_body(D, I, o, DD, d, DI + d.jdof, qpos, qvel, nullptr, i, &rec[SGS_REC * I[o.bpar + i]], &rec[SGS_REC * i], S.data());
  for (int i = 1; i < o.nbody; i++) sgs_body_force(DD, d, &rec[SGS_REC * i], i);
  for (int i = o.nbody - 1; i >= 1; i--) sgs_gather(SI, s, rec.data(), i, SGS_ACC, SGS_REC - SGS_ACC);
  for (int i = 0; i < nv; i++) S[SGS_DOF * i + 6] = sgs_project(&S[SGS_DOF * i], &rec[SGS_REC * SI[s.dbody + i] + SGS_ACC]);
  for (int e = 0; e < v.nM; e++) {
    F[e] = sgv_mass_entry(VI, v, SI, s, DD, d, rec.data(), S.data(), e);
    if (VI[v.anc + e] == VI[v.erow + e]) mdiag[VI[v.erow + e]] = F[e];
  }
  memcpy(Mp, F.data(), sizeof(double) * v.nM);
  for (int L = v.nlevel - 1; L >= 0; L--) {
    const int e0 = VI[v.elstart + L], e1 = VI[v.elstart + L + 1];
    std::vector<double> val(e1 - e0);
    for (int q = e0; q < e1; q++) val[q - e0] = sgv_factor_entry(VI, v, F.data(), VI[v.eidx + q]);
    for (int q = e0; q < e1; q++) F[VI[v.eidx + q]] = val[q - e0];
    for (int q = e0; q < e1; q++) {
      const int e = VI[v.eidx + q];
      if (VI[v.anc + e] != VI[v.erow + e]) F[e] = sgv_factor_scale(VI, v, F.data(), e);
    }
  }
  memcpy(Fp, F.data(), sizeof(double) * v.nM);
  double pmin = INFINITY;
  bool pbad = false, pnan = false;
  for (int i = 0; i < nv; i++) {
    const double Di = F[VI[v.rstart + i]], r = sgv_pivot_ratio(VI, v, F.data(), mdiag.data(), i);
    pbad |= !std::isfinite(Di) || !(Di > 0.0);
    pnan |= r != r;
    pmin = fmin(pmin, r);
  }
  *pivot = pnan ? qnan : pmin;
  info[3] = pbad;
  if (pbad) {
    for (int i = 0; i < n_rhs * nv; i++) x[i] = qnan;
    for (int i = 0; i < nv; i++) qacc_s[i] = qfrc_s[i] = qnan;
    for (int i = 0; i < n_pts * 36; i++) W[i] = qnan;
    return 0;
  }
  for (int r = 0; r < n_rhs; r++) {
    memcpy(x + (size_t)r * nv, y + (size_t)r * nv, sizeof(double) * nv);
    solve_rhs(VI, v, nv, F.data(), x + (size_t)r * nv);
  }
  for (int p = 0; p < n_pts; p++) {   // (before the tendons' pulls overwrite the records' slots; the poses stay)
    const int body = pt_body[p], e0 = VI[v.bdof + body];
    double P[3];
    sgp_pos(&rec[SGS_REC * body], pt_pos + 3 * p, P);
    std::fill(X.begin(), X.end(), 0.0);
    if (e0 >= 0)
      for (int t = 0; t <= VI[v.depth + e0]; t++) {
        const int dd = VI[v.anc + VI[v.rstart + e0] + t];
        double c6[6];
        sgv_jcol(&S[SGS_DOF * dd], P, c6);
        for (int c = 0; c < 6; c++) X[(size_t)c * nv + dd] = c6[c];
      }
    for (int c = 0; c < 6; c++) solve_rhs(VI, v, nv, F.data(), &X[(size_t)c * nv]);
    for (int b = 0; b < 6; b++)
      for (int c = 0; c <= b; c++) W[36 * p + 6 * c + b] = W[36 * p + 6 * b + c] = sgv_w_entry(VI, v, S.data(), X.data(), nv, e0, P, c, b);
  }
  for (int t = 0; t < d.ntendon; t++) {
    double L = 0, Vl = 0;
    const int w0 = DI[d.tadr + t], n = sgd_nshare(DI, d, t);
    for (int k = 0; k < n; k++) {
      double l1, v1;
      sgs_wrap(I, o, DD, DI, d, qpos, qvel, rec.data(), w0 + k, &l1, &v1);
      L += l1; Vl += v1;
    }
    sgs_tendon_force(SD, SI, s, DD, d, act, t, L, Vl, kmask_ten[t], kenv, &ften[2 * t]);
  }
  if (s.nspatial) {
    for (int i = 0; i < o.nbody; i++) sgs_body_tendons(DD, DI, d, ften.data(), rec.data(), i);
    for (int i = o.nbody - 1; i >= 1; i--) sgs_gather(SI, s, rec.data(), i, SGS_ACC, 12);
  }
  for (int i = 0; i < nv; i++) {
    double f[2];
    sgs_dof_applied(SD, SI, s, I, o, DD, DI, d, qpos, qvel, rec.data(), S.data(), ften.data(), kmask_jnt, kenv, i, f);
    qfrc_s[i] = qacc_s[i] = f[0] + f[1] + (applied ? applied[i] : 0.0) - S[SGS_DOF * i + 6];
  }
  solve_rhs(VI, v, nv, F.data(), qacc_s);
  return 0;
}
// the table alone, from a dof-parent chain: info as above (nM, nlevel, tile), levels; -1 and the reason where the model is refused
extern "C" int solve_structure(int nbody, const int* bpar, int nv, const int* dbody, const int* dpar, int ntendon, int* info, int* levels, char* err) {
  SgSolveHost V;
  sgv_build(nbody, bpar, nv, dbody, dpar, ntendon, &V);
  if (!V.ok) { strncpy(err, V.err.c_str(), 255); return -1; }
  info[0] = V.o.nM; info[1] = V.o.nlevel; info[2] = (int)sgv_tile(nbody, nv, ntendon, V.o.nM);
  for (int L = 0; L < V.o.nlevel; L++) levels[L] = V.ints[V.o.lstart + L + 1] - V.ints[V.o.lstart + L];
  return 0;
}
extern "C" int solve_limits(int* out) {
  out[0] = SGV_STATIC_LDS; out[1] = SGV_LDS_MAX; out[2] = SGV_MINRHS; out[3] = SGS_REC; out[4] = SGS_DOF;
  return 5;
}
"""

# the four arithmetic-only breaks of csrc/sg_solve.h (name -> text to replace, its replacement); each text occurs exactly once
BREAKS = {
    "a: division by D dropped in the solve": ("return x[i] / F[VI[v.rstart + i]];", "return x[i];"),
    "b: last descendant of every gather skipped": ("{ return VI[v.dstart + i + 1]; }", "{ return VI[v.dstart + i + 1] - 1; }"),
    "c: down sweep reads the parent only": ("for (int t = 1; t <= n; t++) acc -=", "for (int t = 1; t <= (n < 1 ? n : 1); t++) acc -="),
    "d: u x p dropped from jacp in W": ("c6[3 + k] = Sd[3 + k] + c[k];", "c6[3 + k] = Sd[3 + k];"),
}


def build_host(tmpdir, patch=None):
    """compiles sg_solve.h with g++ into tmpdir -> the ctypes library with solve_host.  patch: a key of BREAKS -- the header is
    compiled from a copy with that one replacement made"""
    tmpdir = str(tmpdir)
    tag = "" if patch is None else "_%d" % sorted(BREAKS).index(patch)
    src = os.path.join(tmpdir, "solve_host%s.cpp" % tag)
    so = os.path.join(tmpdir, "libsolve_host%s.so" % tag)
    csrc = os.path.join(ROOT, "soft-grip_amd", "csrc")
    driver = HOST_DRIVER
    if patch is not None:
        old, new = BREAKS[patch]
        text = open(os.path.join(csrc, "sg_solve.h")).read()
        assert text.count(old) == 1, (patch, text.count(old))
        with open(os.path.join(tmpdir, "sg_solve%s.h" % tag), "w") as f:
            f.write(text.replace(old, new))
        driver = driver.replace('#include "sg_solve.h"', '#include "sg_solve%s.h"' % tag)
    with open(src, "w") as f:
        f.write(driver)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", tmpdir, "-I", csrc, "-o", so, src])
    L = C.CDLL(so)
    L.solve_host.restype = C.c_int
    L.solve_structure.restype = C.c_int
    return L


_TABLES = {}
_p = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)  # noqa: E731
_c = lambda x: None if x is None else np.ascontiguousarray(x, np.float64)  # noqa: E731


def host(L, m, scene, qpos, qvel, k, jids=None, tids=None, act=None, y=None, applied=None, body=None, pos=None):
    """the host build's outputs for one env at stiffness k (smooth_ref.host's conventions): dict of x [R, nv] (y given), qacc_smooth,
    qfrc_smooth [nv], W [P, 6, 6] (points given), pivot, pbad, the dense M and the factor (L [nv, nv], D [nv]) unpacked from the
    build's own packed arrays, nM, levels (dofs per depth) and tile"""
    if id(m) not in _TABLES:
        _TABLES[id(m)] = (m,) + DR._tables(m) + (SR.smooth_table(m),)
    _, K, Dn, Sm = _TABLES[id(m)]
    jids, tids = DR._ids(scene, jids, tids)
    kmj, kmt = np.zeros(m.njnt, np.int32), np.zeros(max(m.ntendon, 1), np.int32)
    if k is not None:
        kmj[jids] = 1
        kmt[tids] = 1
    nv = m.nv
    dpar, _ = dof_parents(m)
    depth, anc, _, nM = structure(dpar)
    y = np.zeros((0, nv)) if y is None else _c(np.atleast_2d(y))
    body = np.zeros(0, np.int32) if body is None else np.ascontiguousarray(body, np.int32)
    pos = np.zeros((0, 3)) if pos is None else _c(pos)
    x, W = np.zeros_like(y), np.zeros((len(body), 6, 6))
    qa, qf, piv = np.zeros(nv), np.zeros(nv), np.zeros(1)
    Mp, Fp = np.zeros(nM), np.zeros(nM)
    info, levels, err = np.zeros(4, np.int32), np.zeros(nv, np.int32), C.create_string_buffer(256)
    q, v, a, ap = _c(qpos), _c(qvel), _c(np.zeros(max(m.nu, 1)) if act is None else act), _c(applied)
    rc = L.solve_host(_p(K[0]), _p(K[1]), _p(K[2]), _p(Dn[0]), _p(Dn[1]), _p(Dn[2]), _p(Sm[0]), _p(Sm[1]), _p(Sm[2]), _p(q), _p(v), _p(a),
                      C.c_double(0.0 if k is None else k), _p(kmj), _p(kmt), len(y), _p(y), _p(x), _p(ap), _p(qa), _p(qf), len(body), _p(body), _p(pos),
                      _p(W), _p(Mp), _p(Fp), _p(piv), _p(info), _p(levels), err)
    assert rc == 0 and info[0] == nM, (rc, err.value, info, nM)
    M, Lm, D = np.zeros((nv, nv)), np.eye(nv), np.zeros(nv)
    e = 0
    for i in range(nv):      # row i of the packed arrays: the diagonal, then the ancestors nearest first
        M[i, i], D[i] = Mp[e], Fp[e]
        for t, j in enumerate(anc[i]):
            M[i, j] = M[j, i] = Mp[e + 1 + t]
            Lm[i, j] = Fp[e + 1 + t]
        e += depth[i] + 1
    return dict(x=x, qacc_smooth=qa, qfrc_smooth=qf, W=W, pivot=float(piv[0]), pbad=bool(info[3]), M=M, L=Lm, D=D, nM=int(info[0]),
                levels=[int(n) for n in levels[:info[1]]], tile=int(info[2]))


def table_of(L, nbody, bpar, dbody, dpar, ntendon=0):
    """sgv_build on a bare dof-parent chain -> (nM, levels, tile) or the refusal's text"""
    i32 = lambda a: np.ascontiguousarray(a, np.int32)  # noqa: E731
    bpar, dbody, dpar = i32(bpar), i32(dbody), i32(dpar)
    info, levels, err = np.zeros(4, np.int32), np.zeros(max(len(dpar), 1), np.int32), C.create_string_buffer(256)
    if L.solve_structure(nbody, _p(bpar), len(dpar), _p(dbody), _p(dpar), ntendon, _p(info), _p(levels), err) != 0:
        return err.value.decode()
    return int(info[0]), [int(n) for n in levels[:info[1]]], int(info[2])


def limits(L):
    out = np.zeros(5, np.int32)
    L.solve_limits(out.ctypes.data_as(C.c_void_p))
    return dict(zip(("static_lds", "lds_max", "minrhs", "rec", "dof"), (int(x) for x in out)))
