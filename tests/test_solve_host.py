"""sg_solve_mass / sg_forward_smooth / sg_get_point_inertia without a GPU: the g++ build of csrc/sg_solve.h, run entry by entry and dof by
dof as the kernel's lanes run it (tests/solve_ref.py), against numpy.linalg.solve on the REFERENCE's dense M -- the oracle's qM on the
five scenes' squeeze states, smooth_ref.reference's M on all 448 states of the sweep of random grippers.  Beside that: the structure
counts, identities on the build's own outputs, the LDS limit against the kept assembly, the refusal of a chain past it, the entry
points' argument checks, and four deliberate breaks of the header's arithmetic that these tests must catch.

Bounds (solve_ref.py; eps = 2^-53, infinity norms per right-hand side):
  residual   |M x - y| <= nv eps (|M| |x| + |y|) with the reference's M
  forward    |x - x_ref| <= nv eps cond2(M) max |x_ref|; for W with max(1, max |W_ref|); absolute nv eps cond2(M) for the pivot figure
  qfrc_smooth against the reference: the sum of dyn_ref.ARR max(1, max |term|) over its four terms
The 17 states of the sweep whose reference M is singular (smallest eigenvalue < 1e-10 of the largest; 4, 4, 0, 3, 3, 3, 0 per case) are
left out of the accuracy checks -- exactly those -- and must report a pivot figure that is NaN or <= 1e-10.
Measured on the CPU first (the tests' docstrings).  The residual of the g++ build is 0.013 of its unit against the build's
OWN M -- LAPACK's on the reference's M is 0.022 to 0.041 -- and up to 0.53 against the REFERENCE's M, which is what the bound asks
for: the difference is the few ulps by which the two M differ (|M_build - M_ref| |x| alone reaches 0.76 of the unit; LAPACK on the
build's M has the build's residual against the reference's to three digits).  It stays inside the bound, which stands as stated."""
import os
import re

import numpy as np
import pytest

import dyn_ref as DR
import smooth_ref as SR
import solve_ref as VR

SCENE_NAMES = sorted(DR.SCENES)


@pytest.fixture(scope="module")
def hostlib(tmp_path_factory):
    return VR.build_host(tmp_path_factory.mktemp("solve_host"))


@pytest.fixture(scope="module")
def sweepdir(tmp_path_factory):
    return tmp_path_factory.mktemp("solve_sweep")


def _worse(worst, key, dev):
    dev = float(dev)
    worst[key] = max(worst.get(key, 0.0), dev if dev == dev else np.inf)      # (a NaN is a failure, not a zero)


def inputs(m, qpos, M, seed):
    """what one state is asked: the points (solve_ref.points) and their reference Jacobians J [P, 6, nv]; y [8, nv] -- 3 random
    right-hand sides of scale 1, 1e3 and 1e-3, M v for 3 more (v3), J' f for the first two points (f2) --; a qfrc_applied of N(0, 1)"""
    body, pos = VR.points(m, seed)
    J = VR.point_jacobians(m, qpos, body, pos)
    rs = np.random.RandomState(seed)
    v3, f2 = VR.rhs(m.nv, 3, seed + 1), rs.standard_normal((2, 6))
    y = np.concatenate([VR.rhs(m.nv, 3, seed), v3 @ M.T, np.stack([J[p].T @ f2[p] for p in range(2)])])
    return dict(body=body, pos=pos, J=J, v3=v3, f2=f2, y=y, applied=rs.standard_normal(m.nv))


def check_outputs(m, got, inp, M, bias, ref, worst, what=None):
    """one state's outputs (the g++ build's or the device's: x [8, nv], qacc_smooth, qfrc_smooth, W [P, 6, 6], pivot; where present M, L,
    D of the build) against the reference's dense M, bias and smooth_ref.reference()'s dict `ref` -> True where M is singular (then
    only the pivot figure is checked).  J solve(J' f) = W f is held to the unit of W times 6 max |f|: six terms of W f, each at W's bound"""
    nv = m.nv
    dpar, _ = VR.dof_parents(m)
    body, J, v3, f2, y, applied = (inp[k] for k in ("body", "J", "v3", "f2", "y", "applied"))
    if VR.is_singular(M):
        assert got["pivot"] != got["pivot"] or got["pivot"] <= VR.SINGULAR, (what, got["pivot"])
        pr = VR.pivot_of(M, dpar)
        assert pr != pr or pr <= VR.SINGULAR, (what, pr)
        return True
    regular = got["pivot"] >= VR.SINGULAR and np.isfinite(got["x"]).all()
    _worse(worst, "a regular M has a pivot figure >= 1e-10", 0.0 if regular else np.inf)
    if not regular:
        return False
    x_ref = np.linalg.solve(M, y.T).T
    # the reference's own error first: LAPACK's solve and the NumPy tree factorisation in the same units
    _worse(worst, "LAPACK residual", VR.residual_dev(M, x_ref, y))
    Lr, Dr = VR.tree_factor(M, dpar)
    _worse(worst, "NumPy tree factor reproduces M", np.abs(Lr.T @ np.diag(Dr) @ Lr - M).max() / (nv * VR.EPS * np.abs(M).max()))
    _worse(worst, "build residual", VR.residual_dev(M, got["x"], y))
    _worse(worst, "build x against LAPACK", VR.forward_dev(M, got["x"], x_ref))
    _worse(worst, "build pivot against the NumPy tree factor", VR.pivot_dev(M, got["pivot"], float((Dr / np.diag(M)).min())))
    if "M" in got:      # identities on the build's own factor
        _worse(worst, "build M against the reference", DR.close(got["M"], M))
        Lb, Db = got["L"], got["D"]
        scale = np.abs(Lb).T @ np.diag(np.abs(Db)) @ np.abs(Lb)
        _worse(worst, "L' D L reproduces the packed M", (np.abs(Lb.T @ np.diag(Db) @ Lb - got["M"]) / (nv * VR.EPS * np.maximum(scale, 1e-300))).max())
    _worse(worst, "solve(M v) = v", VR.forward_dev(M, got["x"][3:6], v3))
    W_ref = VR.reference_W(M, J)
    for p in range(2):
        _worse(worst, "J solve(J' f) = W f", np.abs(J[p] @ got["x"][6 + p] - got["W"][p] @ f2[p]).max()
               / (nv * VR.EPS * VR.cond2(M) * max(1.0, np.abs(W_ref[p]).max()) * 6 * np.abs(f2[p]).max()))
    # smooth forward dynamics
    terms = (ref["passive"], ref["actuator"], applied, bias)
    _worse(worst, "build qfrc_smooth against the reference", np.abs(got["qfrc_smooth"] - (terms[0] + terms[1] + terms[2] - terms[3])).max() / VR.smooth_unit(terms))
    _worse(worst, "build qacc_smooth residual", VR.residual_dev(M, got["qacc_smooth"], got["qfrc_smooth"]))
    _worse(worst, "build qacc_smooth against LAPACK", VR.forward_dev(M, got["qacc_smooth"], np.linalg.solve(M, got["qfrc_smooth"])))
    # point inertias
    W = got["W"]
    floor = nv * VR.EPS * VR.cond2(M)
    for p in range(len(body)):
        assert W[p].tobytes() == np.ascontiguousarray(W[p].T).tobytes(), (what, p)
        wmax = max(1.0, float(np.abs(W_ref[p]).max()))
        _worse(worst, "build W against J solve(M, J')", np.abs(W[p] - W_ref[p]).max() / (floor * wmax))
        _worse(worst, "W positive semidefinite", -np.linalg.eigvalsh(W[p])[0] / (floor * wmax))
    assert body[-1] == 0 and not W[-1].any(), what
    return False


def check_state(L, m, scene, qpos, qvel, k, jids, tids, act, M, bias, ref, seed, worst):
    """one state through the g++ build and check_outputs"""
    inp = inputs(m, qpos, M, seed)
    got = VR.host(L, m, scene, qpos, qvel, k, jids, tids, act=act, y=inp["y"], applied=inp["applied"], body=inp["body"], pos=inp["pos"])
    return check_outputs(m, got, inp, M, bias, ref, worst, scene)


def check_scene(L, scene, worst, states=None):
    from oracle import oracle as O
    m, om, sts = DR.states(scene)
    sim = O.OracleSim(om)
    rs = np.random.RandomState(79)
    for e, st in enumerate(sts[:states]):
        act = rs.uniform(-1.0, 1.0, m.nu)
        kj, kt = DR.stiffness(m, scene, st["k"])
        DR.oracle_forward(sim, st["qpos"], st["qvel"], kj, kt)
        ref = SR.reference(m, st["qpos"], st["qvel"], kj, kt, act)
        assert not check_state(L, m, scene, st["qpos"], st["qvel"], st["k"], None, None, act, sim.qM.copy(), sim.qfrc_bias.copy(), ref, 100 + e, worst), scene


def check_sweep(L, tmp, case, worst, states=None):
    g, offset = case
    m, qpos, qvel, ks, jids, tids, act, _ = SR.sweep(g, tmp, offset)
    refs = SR.sweep_refs(g, tmp, offset)
    singular = 0
    for e in range(len(ks))[:states]:
        singular += check_state(L, m, None, qpos[e], qvel[e], ks[e], jids, tids, act[e], refs[e]["M"], refs[e]["bias"], refs[e], 200 + e, worst)
    return singular


def _report(what, worst):
    print(what, {k: "%.2e" % v for k, v in sorted(worst.items())})
    for key, dev in worst.items():
        assert dev <= 1.0, (what, key, dev)


@pytest.mark.parametrize("scene", SCENE_NAMES)
def test_scenes_match_the_reference(scene, hostlib):
    """the five scenes' three squeeze states at three stiffnesses, M and bias the ORACLE's (qM, qfrc_bias after dyn_ref.oracle_forward).
    Measured on the CPU, in units of the bound, worst over the scenes: LAPACK residual 2.2e-2; build residual 0.31 (see the module's
    docstring), x against LAPACK 0.17, pivot 3.0e-2, M 8.0e-4, qfrc_smooth 1.3e-3, qacc_smooth residual 0.12 and against LAPACK 3.2e-2,
    W 0.13, its smallest eigenvalue -1.7e-3; L' D L = M 4.1e-2, solve(M v) = v 0.17, J solve(J' f) = W f 6.1e-5; the NumPy tree
    factorisation reproduces M to 5.1e-2 nv eps max |M|"""
    worst = {}
    check_scene(hostlib, scene, worst)
    _report(scene, worst)


def test_structure_counts_are_pinned(hostlib):
    """nM and the dofs per depth level of the five scenes, from the build's own table and from the NumPy structure alike"""
    for scene, (nM, levels) in VR.STRUCTURE.items():
        m, om, sts = DR.states(scene)
        got = VR.host(hostlib, m, scene, sts[0]["qpos"], sts[0]["qvel"], sts[0]["k"])
        depth, _, desc, nM_np = VR.structure(VR.dof_parents(m)[0])
        assert (got["nM"], got["levels"]) == (nM, levels) and nM_np == nM and np.bincount(depth).tolist() == levels, (scene, got["nM"], got["levels"])
        assert got["tile"] >= 6, (scene, got["tile"])
    assert max(len(d) for d in desc) == 223      # freeball_fix (the last of the dict): the first free dof's descendants


def test_sweep_of_random_grippers_matches_the_reference(hostlib, sweepdir):
    """all 448 states of dyn_ref's sweep, M and bias smooth_ref.reference's; the 17 states with a singular M (counts per case asserted)
    are left out of the accuracy checks and report a pivot figure that is NaN or <= 1e-10, the 431 others one >= 1e-10.
    Measured on the CPU, in units of the bound: LAPACK residual 4.1e-2; build residual 0.53 (0.013 against the build's own M, see the
    module's docstring), x against LAPACK 0.15, pivot 1.8e-2, M 3.7e-4, qfrc_smooth 2.7e-3, qacc_smooth residual 0.16 and against
    LAPACK 6.0e-2, W 0.24, its smallest eigenvalue -1.7e-3; L' D L = M 0.20, solve(M v) = v 0.13, J solve(J' f) = W f 5.3e-6; the NumPy
    tree factorisation reproduces M to 0.11 nv eps max |M|"""
    worst, counts = {}, []
    for case in DR.SWEEP_CASES:
        counts.append(check_sweep(hostlib, sweepdir, case, worst))
    assert tuple(counts) == VR.SWEEP_SINGULAR, counts
    _report("sweep, %d singular states" % sum(counts), worst)


def test_a_diagonal_mass_matrix_has_pivot_one(hostlib, tmp_path):
    """three bodies on a slider each, all children of the world: M is diagonal, every D_i is M_ii and the pivot figure is exactly 1"""
    import softgrip_amd as sg
    xml = open(os.path.join(DR.ROOT, "tests", "data", "slider.xml")).read()
    one = xml[xml.index("<body"):xml.index("</body>") + len("</body>")]
    p = tmp_path / "three_sliders.xml"
    p.write_text(xml.replace(one, one + one.replace('pos="0 0 1"', 'pos="1 0 1"').replace('axis="0 0 1"', 'axis="1 0 0"') + one.replace('pos="0 0 1"', 'pos="0 2 1"')))
    m = sg.compile_mjcf(str(p))
    assert m.nv == 3
    got = VR.host(hostlib, m, None, np.array([0.1, -0.2, 0.3]), np.zeros(3), None, [], [], y=np.ones((1, 3)))
    assert got["pivot"] == 1.0 and got["levels"] == [3] and got["nM"] == 3
    assert np.abs(got["x"][0] - 1.0 / np.diag(got["M"])).max() <= 3 * VR.EPS * np.abs(got["x"]).max()


# ---- the limits ----
def test_limits_are_pinned_against_the_kept_assembly(hostlib):
    """the kept assembly (sg_readout.device.s): one sg_solve_kernel, 0 bytes of scratch, no VGPR spills, static LDS within SGV_STATIC_LDS
    and a multiple of 16 (the dynamic block starts aligned); the tile the table computes fills the 160 KB a workgroup can have and
    not a right-hand side more; the build's assembly check is clean on the file"""
    from softgrip_amd import build_native, devasm, isa_check
    build_native.build()
    api = build_native.device_asm("sg_readout.hip")
    seen = devasm.kernels(open(api).read())
    k = [v for name, v in seen.items() if "sg_solve_kernel" in name]
    assert len(k) == 1, sorted(seen)
    assert k[0]["scratch"] == 0 and k[0]["vgpr_spill"] == 0, k[0]
    lim = VR.limits(hostlib)
    hdr = open(os.path.join(DR.ROOT, "soft-grip_amd", "csrc", "sg_solve.h")).read()
    assert int(re.search(r"#define SGV_STATIC_LDS (\d+)", hdr).group(1)) == lim["static_lds"] and k[0]["lds"] <= lim["static_lds"] and k[0]["lds"] % 16 == 0, (k[0], lim)
    assert lim["lds_max"] == 160 * 1024 and lim["minrhs"] == 6
    for scene, (nM, _) in VR.STRUCTURE.items():
        m = DR.load(scene)
        dpar, dbody = VR.dof_parents(m)
        got = VR.table_of(hostlib, m.nbody, m.body_parentid, dbody, dpar, m.ntendon)
        fixed = 8 * (lim["rec"] * m.nbody + lim["dof"] * m.nv + 2 * m.ntendon + nM + m.nv)
        assert got[0] == nM and fixed + 8 * m.nv * got[2] + k[0]["lds"] <= lim["lds_max"] < fixed + 8 * m.nv * (got[2] + 1) + lim["static_lds"], (scene, got)
    assert not isa_check.check_asm(api)


def test_a_serial_chain_past_the_limit_is_refused(hostlib):
    """a serial chain of 1024 dofs has nM = 524 800: the table's builder, which sg_model_create runs, refuses it with the limit named and
    before anything of that size is built; a chain of 100 dofs (nM = 5050) runs"""
    n = 1024
    got = VR.table_of(hostlib, 2, [0, 0], np.ones(n), np.arange(n) - 1)
    assert isinstance(got, str) and "524800 entries" in got and "6 right-hand sides" in got and "160 KB of LDS" in got, got
    n = 100
    got = VR.table_of(hostlib, 2, [0, 0], np.ones(n), np.arange(n) - 1)
    assert got[0] == 5050 and got[1] == [1] * 100 and got[2] >= 6, got


def test_sanitizer_run_of_the_table_and_the_per_lane_functions(tmp_path):
    """scripts/sanitize/solve_main.cpp -- a stand-alone program: sgv_build and the factor, sweep and point-inertia functions on one dof,
    a serial chain, the free ball's fan under a chain, random forests and a chain past the limit -- built by g++ with AddressSanitizer
    and UBSan and run on the CPU: no report, the factor gives L and D back, solve(M v) = v"""
    import subprocess
    exe = str(tmp_path / "solve_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                           os.path.join(DR.ROOT, "soft-grip_amd", "csrc"), "-o", exe, os.path.join(DR.ROOT, "scripts", "sanitize", "solve_main.cpp")])
    res = subprocess.run([exe], capture_output=True, text=True)
    print(res.stdout)
    assert res.returncode == 0 and res.stdout.rstrip().endswith("ok") and "refused" in res.stdout and not res.stderr, (res.stdout, res.stderr)


def test_invalid_arguments_are_refused_under_the_entry_points_own_name():
    """without a device: n_ids <= 0, n_rhs / n_pts <= 0 and a NULL batch, each under the calling entry point's name"""
    from softgrip_amd import native
    L = native.lib()
    calls = {
        "sg_solve_mass": lambda n, r=1: L.sg_solve_mass(None, None, n, r, None, None, None, None),
        "sg_forward_smooth": lambda n, r=1: L.sg_forward_smooth(None, None, n, None, None, None, None, None),
        "sg_get_point_inertia": lambda n, r=1: L.sg_get_point_inertia(None, None, n, r, None, None, None, None, None),
    }
    for name, call in calls.items():
        assert call(1) == native.SG_ERR_INVALID, name
        msg = L.sg_last_error()
        assert msg.startswith(name.encode() + b":") and b"null batch" in msg, (name, msg)
        for n in (0, -3):
            assert call(n) == native.SG_ERR_INVALID, name
            msg = L.sg_last_error()
            assert msg.startswith(name.encode() + b":") and b"n_ids" in msg, (name, msg)
        if name != "sg_forward_smooth":
            for r in (0, -2):
                assert call(1, r) == native.SG_ERR_INVALID, name
                msg = L.sg_last_error()
                assert msg.startswith(name.encode() + b":") and (b"n_rhs" in msg or b"n_pts" in msg), (name, msg)
    assert set(calls) <= set(native.SYMBOLS)


# ---- do the tests bite?  Four arithmetic-only breaks of the header, one g++ build each ----
# what each break must trip, found by running them: the checks whose deviation exceeds its bound on the reduced set below
_SOLVE = {"build residual", "build x against LAPACK", "solve(M v) = v", "build qacc_smooth residual", "build qacc_smooth against LAPACK",
          "build W against J solve(M, J')"}
EXPECT = {
    # (both sides of J solve(J' f) = W f lose the division alike: that identity cannot see it)
    "a: division by D dropped in the solve": _SOLVE,
    "b: last descendant of every gather skipped": _SOLVE | {"L' D L reproduces the packed M", "build pivot against the NumPy tree factor", "W positive semidefinite"},
    "c: down sweep reads the parent only": _SOLVE | {"J solve(J' f) = W f", "W positive semidefinite"},
    "d: u x p dropped from jacp in W": {"build W against J solve(M, J')", "J solve(J' f) = W f"},
}


def reduced_set(L, sweepdir, worst, scenes=("softbox_fix", "freeball_fix", "fourfinger_softball_fix")):
    for scene in scenes:
        check_scene(L, scene, worst, states=1)
    check_sweep(L, sweepdir, (2, False), worst, states=6)


@pytest.mark.parametrize("name", sorted(VR.BREAKS))
def test_a_broken_header_is_caught(name, tmp_path, sweepdir):
    """sg_solve.h with one piece of arithmetic changed (solve_ref.BREAKS), built by g++ and put through the checks above on a reduced
    set -- the first state of softbox_fix, freeball_fix and fourfinger_softball_fix and 6 states of the sweep's gripper 2 (no singular
    state among them): the checks named in EXPECT must fail, and no check of the reference itself may move.
    Break c cannot show on dofs with at most one ancestor; the finger chains of the four-finger scene (depth 16), the free ball's
    sliders under its six free dofs and the sweep's chains see it"""
    L = VR.build_host(tmp_path, patch=name)
    worst = {}
    reduced_set(L, sweepdir, worst)
    failed = {k for k, v in worst.items() if not v <= 1.0}
    print(name, "fails:", sorted(failed), {k: "%.2e" % worst[k] for k in sorted(failed)})
    assert failed == EXPECT[name], (name, sorted(failed))
    assert not any(k.startswith(("LAPACK", "NumPy")) for k in failed)
