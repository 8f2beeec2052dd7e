"""Helpers of the tests of the read-outs that start with the inverse of the mass matrix (sg_solve_mass, sg_forward_smooth,
sg_get_point_inertia; csrc/sg_solve.h), on top of tests/dyn_ref.py and tests/smooth_ref.py:

  * the reference: numpy.linalg.solve on a dense M (the oracle's qM on the scenes, smooth_ref.reference's M on the sweep), qfrc_smooth
    from smooth_ref's passive / actuator and the oracle's or the reference's bias, J from dyn_ref.point_jac;
  * tree_factor(): the level-scheduled tree factorisation M = L' D L as plain NumPy on a dense M, for the pivot figure and the
    structure counts -- written from the definition (mj_factorM's sparsity), not from the header;
  * build_host() / host(): the g++ build of csrc/sg_solve.h run serially, entry by entry and dof by dof, as the kernel's lanes run it
    (sgv_host_env of csrc/sg_readout_host.h, on the tables csrc/sg_tables.cpp builds of the model's blob); patch= builds a header with one piece of arithmetic broken (the tests that show the tests bite);
  * the bounds: the residual unit nv eps (|M| |x| + |y|) and the forward unit nv eps cond2(M) max |x_ref|, in infinity norms.
"""
import ctypes as C

import numpy as np

import dyn_ref as DR
import readout_host as RH
from tables_ref import smooth_table

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
    off, _, ints = smooth_table(m)
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


# ---- the g++ build of csrc/sg_solve.h: sgv_host_env of csrc/sg_readout_host.h through tests/readout_host.py's shim ----
# the four arithmetic-only breaks of csrc/sg_solve.h (name -> header, text to replace, its replacement); each text occurs exactly once
BREAKS = {
    "a: division by D dropped in the solve": ("sg_solve.h", "return x[i] / F[VI[v.rstart + i]];", "return x[i];"),
    "b: last descendant of every gather skipped": ("sg_solve.h", "{ return VI[v.dstart + i + 1]; }", "{ return VI[v.dstart + i + 1] - 1; }"),
    "c: down sweep reads the parent only": ("sg_solve.h", "for (int t = 1; t <= n; t++) acc -=", "for (int t = 1; t <= (n < 1 ? n : 1); t++) acc -="),
    "d: u x p dropped from jacp in W": ("sg_solve.h", "c6[3 + k] = Sd[3 + k] + c[k];", "c6[3 + k] = Sd[3 + k];"),
}


def build_host(tmpdir, patch=None):
    """the ctypes library with solve_host and solve_structure.  patch: a key of BREAKS -- the header is compiled from a copy with that
    one replacement made"""
    return RH.build(tmpdir, BREAKS, patch)


_p = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)  # noqa: E731
_c = lambda x: None if x is None else np.ascontiguousarray(x, np.float64)  # noqa: E731


def host(L, m, scene, qpos, qvel, k, jids=None, tids=None, act=None, y=None, applied=None, body=None, pos=None):
    """the host build's outputs for one env at stiffness k (smooth_ref.host's conventions): dict of x [R, nv] (y given), qacc_smooth,
    qfrc_smooth [nv], W [P, 6, 6] (points given), pivot, pbad, the dense M and the factor (L [nv, nv], D [nv]) unpacked from the
    build's own packed arrays, nM, levels (dofs per depth) and tile"""
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
    rc = L.solve_host(RH.tables(L, m), _p(q), _p(v), _p(a), C.c_double(0.0 if k is None else k), _p(kmj), _p(kmt), len(y), _p(y), _p(x), _p(ap), _p(qa), _p(qf),
                      len(body), _p(body), _p(pos), _p(W), _p(Mp), _p(Fp), _p(piv), _p(info), _p(levels), err)
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
