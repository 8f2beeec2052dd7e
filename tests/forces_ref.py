"""Helpers of the constraint-force read-out's tests (sg_get_forces; csrc/sg_forces.h):

  * the states: ONE oracle rollout per scene / gripper and stiffness -- reset, forward, step, ctrl = -0.2, then N steps -- with qpos,
    qvel, act, ctrl and qacc_warmstart kept as the step left them (computed once, shared, never changed);
  * the reference: the oracle's forward pass seated at such a state (row list, efc_force, qacc, constraint_problem()); the oracle
    exports neither J nor qfrc_constraint, so qfrc_constraint's reference is J' f with the oracle's f and reference_J(), a NumPy
    Jacobian of the oracle's row list written from the definitions;
  * unit(): the oracle's OWN response to rounding its input -- qpos perturbed by 1e-14 N(0, 1) per entry over 10 seeds, the largest
    change of each quantity -- and whether the 10 runs disagree among themselves on (nefc, ncon, solver_iter): a knife edge;
  * the bound: |x - x_ref| <= max(TOL, 10 unit_x) max(1, max |x_ref|) for f, qacc and qfrc_constraint;
  * build_host() / host(): the g++ build of csrc/sg_forces.h (through csrc/sg_forces_host.h, which runs one env serially in the
    kernels' order) with the table builders of csrc/sg_tables.cpp; patch= builds a header with one piece of arithmetic broken.
"""
import ctypes as C
import os

import numpy as np

import contacts_ref as CR
import dyn_ref as DR
import host_build
import softgrip_amd as sg

TOL = CR.TOL
KS = DR.KS
SCENE_STEPS = {"mini_gripper": (20, 60), "softbox": (20, 60), "freeball_fix": (20,), "fourfinger_softball_fix": (20,)}
GRIPPERS = tuple(range(6))
GRIPPER_STEPS = (10, 30)
UNIT_SEEDS = 10
UNIT_EPS = 1e-14

_MODELS, _STATES, _REFS = {}, {}, {}


def model(key, tmpdir=None):
    """(Model, OracleModel, joint ids, tendon ids) of a scene name or of random gripper `key` (an int) of contacts_ref's sweep"""
    if key not in _MODELS:
        from oracle import oracle as O
        if isinstance(key, str):
            scene, _, opt = key.partition("@")      # "mini_gripper@impratio4": the scene with opt.impratio = 4 (every committed scene has 1)
            m = DR.load(scene)
            if opt:
                assert opt == "impratio4", key
                m.opt_impratio = 4.0
            jids, tids = DR.SCENES[scene][1], DR.SCENES[scene][2]
        else:
            path = os.path.join(str(tmpdir), "forces_g%d.xml" % key)
            with open(path, "w") as f:
                f.write(CR.sweep_gripper_xmls()[key])
            m = sg.compile_mjcf(path, composite_neighbors=False)
            jids, tids = DR.sweep_ids(m)
        _MODELS[key] = (m, O.OracleModel(m.to_blob()), list(jids), list(tids))
    return _MODELS[key]


def states(key, steps, tmpdir=None):
    """{N: [dict(qpos, qvel, act, ctrl, warm, k) per env of KS]} after N steps of the rollout, N in steps"""
    from oracle import oracle as O
    m, om, jids, tids = model(key, tmpdir)
    if key not in _STATES:
        _STATES[key] = {}
    have = _STATES[key]
    if all(n in have for n in steps):
        return have
    for n in steps:
        have[n] = []
    for k in KS:
        s = O.OracleSim(om)
        s.jnt_stiffness[jids] = k
        s.tendon_stiffness[tids] = k
        s.reset(); s.forward(); s.step()
        s.ctrl[:] = -0.2
        for n in range(1, max(steps) + 1):
            assert s.step() == 0, (key, k, n)
            if n in steps:
                have[n].append(dict(qpos=s.qpos.copy(), qvel=s.qvel.copy(), act=s.act.copy(), ctrl=s.ctrl.copy(), warm=s.qacc_warmstart.copy(), k=k))
    return have


def seat(sim, st, jids, tids, qpos=None):
    sim.qpos[:] = st["qpos"] if qpos is None else qpos
    sim.qvel[:], sim.act[:], sim.ctrl[:], sim.qacc_warmstart[:] = st["qvel"], st["act"], st["ctrl"], st["warm"]
    sim.jnt_stiffness[jids] = st["k"]
    sim.tendon_stiffness[tids] = st["k"]


def oracle_forward(key, st, qpos=None, problem=False, tmpdir=None):
    """the oracle's forward pass at the state (qpos: a perturbed one in its place): dict of nefc, ncon, iters, type, id, f, qacc, its
    contacts, J = reference_J of its row list and qfrc = J' f (the oracle exports neither J nor qfrc_constraint)"""
    from oracle import oracle as O
    m, om, jids, tids = model(key, tmpdir)
    sim = O.OracleSim(om)
    seat(sim, st, jids, tids, qpos)
    sim.forward()
    n = sim.nefc
    L = O.lib()
    ty = np.ctypeslib.as_array(L.sgo_efc_type(sim.ptr), shape=(max(n, 1),))[:n].copy()
    ids = np.ctypeslib.as_array(L.sgo_efc_id(sim.ptr), shape=(max(n, 1),))[:n].copy()
    out = dict(nefc=n, ncon=sim.ncon, iters=sim.solver_iter, type=ty, id=ids, f=sim.efc_force() if n else np.zeros(0), qacc=sim.qacc.copy(),
               contacts=sim.contacts())
    out["J"] = reference_J(m, sim.qpos, ty, ids, out["contacts"])
    out["qfrc"] = out["J"].T @ out["f"] if n else np.zeros(m.nv)
    if problem and n:
        out["AR"], out["b"] = sim.constraint_problem()[:2]
    return out


def reference_J(m, qpos, ty, ids, contacts):
    """[nefc, nv]: the rows' Jacobian in NumPy, from the definitions and the oracle's row list and contacts (dyn_ref's Jacobian
    columns): an equality's +1 / -poly' or its tendon's Jacobian, a limit's -side, a contact's frame row on jac(geom2) - jac(geom1)"""
    qpos = np.asarray(qpos, np.float64)
    kin = m.kinematics(qpos)
    cols = DR.dof_columns(m, kin)
    mv = DR.moved_by(m, cols[3])
    sx = m.site_xpos(kin) if m.nsite else np.zeros((0, 3))
    J = np.zeros((len(ty), m.nv))
    qa, da = np.asarray(m.jnt_qposadr), np.asarray(m.jnt_dofadr)
    i = 0
    while i < len(ty):
        t, e = int(ty[i]), int(ids[i])
        if t == 0:
            if m.eq_type[e] == 2:
                j, j2 = int(m.eq_obj1id[e]), int(m.eq_obj2id[e])
                J[i, da[j]] = 1.0
                if j2 >= 0:
                    pc = np.asarray(m.eq_data, np.float64).reshape(-1, 5)[e]
                    dif = qpos[qa[j2]] - m.qpos0[qa[j2]]
                    J[i, da[j2]] += -(pc[1] + dif * (2 * pc[2] + dif * (3 * pc[3] + dif * 4 * pc[4])))
            else:
                tn = int(m.eq_obj1id[e])
                a, n = int(m.tendon_adr[tn]), int(m.tendon_num[tn])
                if m.wrap_type[a] == DR.WRAP_JOINT:
                    J[i, da[np.asarray(m.wrap_objid[a:a + n])]] = m.wrap_prm[a:a + n]
                else:
                    for w in range(a, a + n - 1):
                        s0, s1 = int(m.wrap_objid[w]), int(m.wrap_objid[w + 1])
                        d = sx[s1] - sx[s0]
                        ln = np.linalg.norm(d)
                        if ln >= 1e-15:
                            J[i] += (d / ln) @ (DR.point_jac(cols, mv[m.site_bodyid[s1]], sx[s1]) - DR.point_jac(cols, mv[m.site_bodyid[s0]], sx[s0]))
            i += 1
        elif t == 3:
            rng, q = np.asarray(m.jnt_range, np.float64).reshape(-1, 2)[e], qpos[qa[e]]
            lower = (q - rng[0]) < m.jnt_margin[e]
            second = i > 0 and int(ty[i - 1]) == 3 and int(ids[i - 1]) == e
            J[i, da[e]] = 1.0 if (lower and not second) else -1.0
            i += 1
        else:
            c = contacts[e]
            dim = 1 if t == 5 else 3
            b1, b2 = int(m.geom_bodyid[c["geom1"]]), int(m.geom_bodyid[c["geom2"]])
            dj = DR.point_jac(cols, mv[b2], c["pos"]) - DR.point_jac(cols, mv[b1], c["pos"])
            J[i:i + dim] = c["frame"].reshape(3, 3)[:dim] @ dj
            i += dim
    return J


def reference_at(key, st, seed, tmpdir=None):
    """the oracle's outputs at a state of model `key` (oracle_forward's dict with A + R and b), its units -- the largest change of f,
    qacc and qfrc over UNIT_SEEDS runs at qpos + UNIT_EPS N(0, 1) -- and `knife`: do those runs disagree among themselves on
    (nefc, ncon, solver_iter)?"""
    ref = oracle_forward(key, st, problem=True, tmpdir=tmpdir)
    rs = np.random.RandomState(seed)
    seen, unit = set(), dict(f=0.0, qacc=0.0, qfrc=0.0)
    for _ in range(UNIT_SEEDS):
        p = oracle_forward(key, st, qpos=st["qpos"] + UNIT_EPS * rs.standard_normal(len(st["qpos"])), tmpdir=tmpdir)
        seen.add((p["nefc"], p["ncon"], p["iters"]))
        if p["nefc"] == ref["nefc"]:
            for q in unit:
                if len(ref[q]):
                    unit[q] = max(unit[q], float(np.abs(p[q] - ref[q]).max()))
    ref["unit"], ref["knife"] = unit, len(seen) > 1
    return ref


def reference(key, n, env, tmpdir=None):
    """reference_at() of state (key, n, env) of the rollouts; computed once and shared"""
    if (key, n, env) not in _REFS:
        _REFS[key, n, env] = reference_at(key, states(key, (n,), tmpdir)[n][env], 1000 + env, tmpdir)
    return _REFS[key, n, env]


def check_discrete(got, ref, what):
    """nefc, ncon, iters, row types and ids exact (got: dict of nefc, ncon, iters, type, id with at least nefc rows)"""
    assert (got["nefc"], got["ncon"], got["iters"]) == (ref["nefc"], ref["ncon"], ref["iters"]), (what, got["nefc"], got["ncon"], got["iters"], ref["nefc"], ref["ncon"], ref["iters"])
    n = ref["nefc"]
    assert (np.asarray(got["type"])[:n] == ref["type"]).all() and (np.asarray(got["id"])[:n] == ref["id"]).all(), what


def worse(worst, key, d):
    d = float(d)
    worst[key] = max(worst.get(key, 0.0), d if d == d else np.inf)


def report(what, worst):
    print(what, {k: "%.2e" % v for k, v in sorted(worst.items())})
    for key, d in worst.items():
        assert d <= 1.0, (what, key, d)


def cost_change_numpy(A, f, old, res):
    """sol_pgs' cost_change: (the change of the cost, the force kept): an update that raises the cost by more than 1e-10 is taken back"""
    A, f, old, res = (np.asarray(x, np.float64) for x in (A, f, old, res))
    delta = f - old
    change = float(0.5 * delta @ (A @ delta) + delta @ res)
    return (0.0, old.copy()) if change > 1e-10 else (change, f.copy())


def bound(ref, q):
    return max(TOL, 10.0 * ref["unit"][q]) * max(1.0, float(np.abs(ref[q]).max()) if len(ref[q]) else 1.0)


def dev(got, ref, q):
    """the largest deviation of quantity q in units of its bound (inf for a NaN or a shape that differs)"""
    got = np.asarray(got, np.float64)
    if got.shape != ref[q].shape or not np.isfinite(got).all():
        return float("inf")
    return float(np.abs(got - ref[q]).max() / bound(ref, q)) if got.size else 0.0


# ---- the g++ build ----
HOST_DRIVER = r"""
#include "sg_forces_host.h"
extern "C" void* forces_model_new(const void* blob, size_t n, char* err) {
  SgHostTables* m = new SgHostTables();
  sg_host_tables(blob, n, m);
  if (!m->forces.ok) { strncpy(err, m->forces.err.c_str(), 255); delete m; return nullptr; }
  return m;
}
extern "C" void forces_model_free(void* h) { delete (SgHostTables*)h; }
// info: nv, nrows, cap, neq, nlim, njmax, iterations, env bytes (two ints)
extern "C" void forces_model_info(void* h, long long* info) {
  const SgHostTables* m = (const SgHostTables*)h;
  const SgForceOff& f = m->forces.o;
  info[0] = m->dyn.o.nv; info[1] = f.nrows; info[2] = f.cap; info[3] = f.neq; info[4] = f.nlim; info[5] = f.njmax; info[6] = f.iterations;
  info[7] = (long long)sgf_env_bytes(f, m->dyn.o.nv);
}
// counts: nefc, ncon, iters, warm start kept.  rows [nrows][3]: type, id, aux; caddr [cap]; f [nrows]; J, W [nrows][nv]; sc [nrows][SGF_SC]
extern "C" int forces_host(void* h, const double* qpos, const double* qvel, const double* act, const double* warm, double kenv, const int* kmj, const int* kmt,
                           int* counts, int* rows, int* caddr, double* f, double* J, double* W, double* sc, double* qfrc, double* qacc, double* qacc_smooth) {
  const SgHostTables* m = (const SgHostTables*)h;
  SgfHostOut o;
  const int rc = sgf_host_env(*m, qpos, qvel, act, warm, kenv, kmj, kmt, &o);
  if (rc) return rc;
  const int nv = m->dyn.o.nv, ne = o.nefc;
  counts[0] = ne; counts[1] = o.ncon; counts[2] = o.iters; counts[3] = o.warm_kept;
  for (int i = 0; i < ne; i++) { rows[3 * i] = o.rtype[i]; rows[3 * i + 1] = o.rid[i]; rows[3 * i + 2] = o.raux[i]; f[i] = o.f[i]; }
  for (int c = 0; c < o.ncon; c++) caddr[c] = o.caddr[c];
  memcpy(J, o.J.data(), sizeof(double) * ne * nv);
  memcpy(W, o.W.data(), sizeof(double) * ne * nv);
  memcpy(sc, o.sc.data(), sizeof(double) * ne * SGF_SC);
  memcpy(qfrc, o.qfrc.data(), sizeof(double) * nv);
  memcpy(qacc, o.qacc.data(), sizeof(double) * nv);
  memcpy(qacc_smooth, o.qacc_smooth.data(), sizeof(double) * nv);
  return 0;
}
// sgf_cost_change on a block of dim rows: f is updated in place, the change is returned
extern "C" double forces_cost_change(const double* A, double* f, const double* old, const double* res, int dim) { return sgf_cost_change(A, f, old, res, dim); }
extern "C" int forces_limits(int* out) { out[0] = SGF_SC; out[1] = SGF_STATIC_LDS; out[2] = SGF_LDS_MAX; return 3; }
"""

# the four arithmetic-only breaks of csrc/sg_forces.h (name -> text to replace, its replacement); each text occurs exactly once
BREAKS = {
    "a: the warm start's cost gate dropped": ("return !(cost > 0.0);", "return true;"),
    "b: the cost-change revert dropped": ("if (change > 1e-10) { for (int j = 0; j < dim; j++) f[j] = old[j]; change = 0; }", ""),
    "c: the friction rows' R without impratio": ("R[1] = R[0] / fmax(SGF_MINVAL, impratio);", "R[1] = R[0];"),
    "d: limit sides swapped": ("return side * (FD[f.jrange + 2 * j + (side + 1) / 2] - qpos[I[o.jqadr + j]]);",
                               "return side * (FD[f.jrange + 2 * j + (1 - side) / 2] - qpos[I[o.jqadr + j]]);"),
}


def build_host(tmpdir, patch=None):
    """csrc/sg_forces.h through sg_forces_host.h, with sg_tables.cpp -> the ctypes library.  patch: a key of BREAKS, made in sg_forces.h"""
    L = host_build.build(tmpdir, "forces_host", HOST_DRIVER, copy=("sg_forces.h", "sg_tables.h", "sg_readout_host.h", "sg_forces_host.h", "sg_tables.cpp"),
                         patch=None if patch is None else ("sg_forces.h",) + BREAKS[patch], tag="plain" if patch is None else "break%d" % sorted(BREAKS).index(patch))
    L.forces_model_new.restype = C.c_void_p
    L.forces_model_new.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p]
    L.forces_model_free.argtypes = [C.c_void_p]
    L.forces_model_info.argtypes = [C.c_void_p, C.c_void_p]
    L.forces_host.restype = C.c_int
    L.forces_cost_change.restype = C.c_double
    L._models = {}
    return L


_p = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731


def host_model(L, key, tmpdir=None):
    """(handle, info dict) of the g++ build's tables for a scene or gripper"""
    if key not in L._models:
        m = model(key, tmpdir)[0]
        blob, err = m.to_blob(), C.create_string_buffer(256)
        h = L.forces_model_new(blob, len(blob), err)
        assert h, err.value
        info = np.zeros(8, np.int64)
        L.forces_model_info(h, _p(info))
        L._models[key] = (h, dict(zip(("nv", "nrows", "cap", "neq", "nlim", "njmax", "iterations", "env_bytes"), (int(x) for x in info))))
    return L._models[key]


def host(L, key, st, tmpdir=None):
    """the g++ build's outputs at a state: dict of nefc, ncon, iters, warm_kept, type, id, aux, caddr, f, J, W [nefc, nv], sc [nefc, SGF_SC],
    qfrc, qacc, qacc_smooth; None for an env the build ends in NaN"""
    m, _, jids, tids = model(key, tmpdir)
    h, info = host_model(L, key, tmpdir)
    nv, nr = info["nv"], info["nrows"]
    kmj, kmt = np.zeros(m.njnt, np.int32), np.zeros(max(m.ntendon, 1), np.int32)
    kmj[jids] = 1
    kmt[tids] = 1
    counts, rows, caddr = np.zeros(4, np.int32), np.zeros((nr, 3), np.int32), np.full(info["cap"], -1, np.int32)
    f, J, W, sc = np.zeros(nr), np.zeros((nr, nv)), np.zeros((nr, nv)), np.zeros((nr, 8))
    qfrc, qacc, qs = np.zeros(nv), np.zeros(nv), np.zeros(nv)
    c = lambda x: np.ascontiguousarray(x, np.float64)  # noqa: E731
    q, v, a, w = c(st["qpos"]), c(st["qvel"]), c(st["act"] if len(st["act"]) else np.zeros(1)), c(st["warm"])
    rc = L.forces_host(C.c_void_p(h), _p(q), _p(v), _p(a), _p(w), C.c_double(st["k"]), _p(kmj), _p(kmt), _p(counts), _p(rows), _p(caddr), _p(f), _p(J), _p(W), _p(sc),
                       _p(qfrc), _p(qacc), _p(qs))
    if rc:
        return None
    n = int(counts[0])
    return dict(nefc=n, ncon=int(counts[1]), iters=int(counts[2]), warm_kept=int(counts[3]), type=rows[:n, 0].copy(), id=rows[:n, 1].copy(), aux=rows[:n, 2].copy(),
                caddr=caddr[:int(counts[1])].copy(), f=f[:n].copy(), J=J[:n].copy(), W=W[:n].copy(), sc=sc[:n].copy(), qfrc=qfrc, qacc=qacc, qacc_smooth=qs)


def all_states():
    """[(key, N)] of every state the issue lists: the four scenes' and the six grippers'"""
    return [(s, n) for s, ns in SCENE_STEPS.items() for n in ns] + [(g, n) for g in GRIPPERS for n in GRIPPER_STEPS]


# ---- the sizes the library derives from a model (csrc/sg_forces.h), restated ----
def host_cap(m):
    """the contacts the list keeps at most: the model's nconmax when positive, and the oracle's 512"""
    return int(m.nconmax) if 0 < int(m.nconmax) < 512 else 512


def row_capacity(m):
    """sg_model_max_rows: every equality, both sides of every limited scalar joint, three rows per contact of the list, cut by njmax"""
    nlim = int(sum(1 for j in range(m.njnt) if m.jnt_limited[j] and m.jnt_type[j] != DR.JNT_FREE))
    fixed = len(m.eq_type) + 2 * nlim
    rows = fixed + 3 * host_cap(m)
    return max(fixed, int(m.njmax)) if 0 < int(m.njmax) < rows else rows


def host_env_bytes(m):
    """one env's share of sg_get_forces' work space in bytes"""
    nrows, cap, nv = row_capacity(m), host_cap(m), m.nv
    return 8 * (2 * nrows * nv + 8 * nrows + nv + 13 * cap + (3 * nrows + 3 * cap + 4 + 1) // 2)
