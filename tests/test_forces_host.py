"""sg_get_forces without a GPU: the g++ build of csrc/sg_forces.h, run row by row as the kernels' lanes run it (csrc/sg_forces_host.h,
tests/forces_ref.py), against the oracle's forward pass on every state of forces_ref.all_states() -- the four scenes (mini_gripper at 20 and
60 steps, softbox at 20 and 60, freeball_fix and fourfinger_softball_fix at 20) and contacts_ref's random grippers 0 - 5 at 10 and 30
steps, three envs each at dyn_ref.KS.

Exact: nefc, ncon, the row types and ids, and the sweeps run against solver_iter.  The implied J M^-1 J' + R and b against
OracleSim.constraint_problem() with dyn_ref.close.  Forces, qacc and qfrc_constraint inside
    |x - x_ref| <= max(TOL, 10 unit_x) max(1, max |x_ref|),    TOL = 1e-9,
unit_x the oracle's own largest change of x over 10 runs at qpos + 1e-14 N(0, 1).  qfrc_constraint's reference is J' f with the oracle's
f and forces_ref.reference_J(), a NumPy Jacobian of the oracle's row list (the oracle exports neither J nor qfrc_constraint).
A state is a knife edge only where those 10 runs disagree among themselves on (nefc, ncon, solver_iter); the count is asserted: none
of the 36 x 3 states is one (stiffness 300 and 1400 included).
Measured on the CPU, worst over all states, in units of the bound: f 5.1e-5, qacc 6.9e-6, qfrc_constraint 1.2e-4; J 3.8e-4, A + R
4.2e-3 and b 0.18 of dyn_ref.close's."""
import os
import subprocess

import numpy as np
import pytest

import dyn_ref as DR
import forces_ref as FR

KEYS = list(FR.SCENE_STEPS) + list(FR.GRIPPERS)


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return tmp_path_factory.mktemp("forces_host")


@pytest.fixture(scope="module")
def hostlib(work):
    return FR.build_host(work)


def check_state(L, key, n, env, tmp, worst):
    """one state through the g++ build -> True where it is a knife edge (left out)"""
    st = FR.states(key, (n,), tmp)[n][env]
    ref = FR.reference(key, n, env, tmp)
    if ref["knife"]:
        return True
    got = FR.host(L, key, st, tmp)
    if got is None or got["nefc"] != ref["nefc"] or (got["type"] != ref["type"]).any() or (got["id"] != ref["id"]).any():
        FR.worse(worst, "row list", np.inf)
        return False
    FR.worse(worst, "row list", 0.0)
    FR.worse(worst, "ncon and sweeps", 0.0 if (got["ncon"], got["iters"]) == (ref["ncon"], ref["iters"]) else np.inf)
    if ref["nefc"]:
        FR.worse(worst, "J against the NumPy Jacobian", DR.close(got["J"], ref["J"]))
        FR.worse(worst, "J M^-1 J' + R", DR.close(got["J"] @ got["W"].T + np.diag(got["sc"][:, 1]), ref["AR"]))
        FR.worse(worst, "b", DR.close(got["sc"][:, 0], ref["b"]))
    for q in ("f", "qacc", "qfrc"):
        FR.worse(worst, q, FR.dev(got[q], ref, q))
    return False


def steps_of(key):
    return FR.SCENE_STEPS[key] if isinstance(key, str) else FR.GRIPPER_STEPS


@pytest.mark.parametrize("key", KEYS)
def test_states_match_the_oracle(key, hostlib, work):
    """every state of one scene or gripper; no state is left out (the knife-edge count is asserted to be zero)"""
    worst, knife = {}, 0
    for n in steps_of(key):
        for env in range(len(FR.KS)):
            knife += check_state(hostlib, key, n, env, work, worst)
    assert knife == 0, (key, knife)
    FR.report("%s" % (key,), worst)


def test_the_states_cover_what_they_are_chosen_for(hostlib, work):
    """mini_gripper at 20: no contact, an early exit after 2 sweeps; at 60: 6 contacts, all 20 sweeps.  softbox: 355 and 389 rows, all 30
    sweeps.  freeball_fix: 32 contacts.  fourfinger_softball_fix: nv 283, an early exit at 29.  Gripper 0 at 10: 70 contacts, 15 limit
    rows, 260 rows"""
    r = lambda key, n: FR.reference(key, n, 0, work)  # noqa: E731
    a, b = r("mini_gripper", 20), r("mini_gripper", 60)
    assert (a["ncon"], a["iters"]) == (0, 2) and (b["ncon"], b["iters"]) == (6, 20)
    a, b = r("softbox", 20), r("softbox", 60)
    assert (a["nefc"], a["iters"], b["nefc"], b["iters"]) == (355, 30, 389, 30)
    assert r("freeball_fix", 20)["ncon"] == 32
    a = r("fourfinger_softball_fix", 20)
    assert FR.model("fourfinger_softball_fix")[0].nv == 283 and a["iters"] == 29
    a = r(0, 10)
    assert (a["ncon"], int((a["type"] == 3).sum()), a["nefc"]) == (70, 15, 260)
    info = FR.host_model(hostlib, "fourfinger_softball_fix")[1]
    assert info["nrows"] == info["neq"] + 2 * info["nlim"] + 3 * info["cap"] == 2285 and info["env_bytes"] > 10e6


def test_the_cost_change_revert_against_numpy(hostlib):
    """sgf_cost_change against a NumPy restatement of sol_pgs' cost_change on seeded blocks of one and three rows, half of them updates
    that raise the cost by more than 1e-10 and must be taken back.  No state of the list takes the revert (measured: the build with
    the revert dropped gives the same bits on all 108), so this is where a dropped revert shows"""
    import ctypes as C
    rs = np.random.RandomState(7)
    reverted = 0
    for case in range(64):
        dim = (1, 3)[case % 2]
        B = rs.standard_normal((dim, dim))
        A = np.ascontiguousarray(B @ B.T + np.eye(dim))
        old, res = rs.standard_normal(dim), rs.standard_normal(dim)
        f = old - np.linalg.solve(A, res) * (1.0 if case % 4 < 2 else -1.5)      # a descent step, or a step uphill
        want_change, want_f = FR.cost_change_numpy(A, f, old, res)
        got_f = f.copy()
        p = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
        got_change = hostlib.forces_cost_change(p(A), p(got_f), p(np.ascontiguousarray(old)), p(np.ascontiguousarray(res)), dim)
        assert abs(got_change - want_change) <= 1e-12 * max(1.0, abs(want_change)) and np.abs(got_f - want_f).max() == 0.0, case
        reverted += int((want_f == old).all())
    assert reverted == 32


# ---- do the tests bite?  Four arithmetic-only breaks of the header, one g++ build each ----
REDUCED = [("mini_gripper", 60), ("mini_gripper@impratio4", 60), ("softbox", 20), (0, 10), ("fourfinger_softball_fix", 20)]
EXPECT = {
    # softbox at 20, gripper 0 at 10 and the four-finger scene reject their warm start: kept, it starts the sweeps elsewhere
    "a: the warm start's cost gate dropped": {"f", "qacc", "qfrc", "ncon and sweeps"},
    # no state takes the revert: test_the_cost_change_revert_against_numpy is what fails
    "b: the cost-change revert dropped": set(),
    # every committed scene has impratio 1: mini_gripper with opt.impratio = 4 is what sees it
    "c: the friction rows' R without impratio": {"f", "qacc", "qfrc", "J M^-1 J' + R"},
    "d: limit sides swapped": {"row list"},
}


@pytest.mark.parametrize("name", sorted(FR.BREAKS))
def test_a_broken_header_is_caught(name, work):
    """sg_forces.h with one piece of arithmetic changed (forces_ref.BREAKS), built by g++ and put through the checks above on a reduced
    set (env 0 of five states; mini_gripper once more with opt.impratio = 4): the checks named in EXPECT must fail.  Break b passes
    them all and fails the direct test of sgf_cost_change"""
    L = FR.build_host(work, patch=name)
    worst = {}
    for key, n in REDUCED:
        assert not check_state(L, key, n, 0, work, worst)
    failed = {k for k, v in worst.items() if not v <= 1.0}
    print(name, "fails:", sorted(failed))
    assert failed == EXPECT[name], (name, sorted(failed))
    if name.startswith("b:"):
        with pytest.raises(AssertionError):
            test_the_cost_change_revert_against_numpy(L)


# ---- the table builder's refusals (SG_ERR_MODEL at the entry points: the message is the builder's) ----
def _refusal(L, m):
    import ctypes as C
    blob, err = m.to_blob(), C.create_string_buffer(256)
    h = L.forces_model_new(blob, len(blob), err)
    if h:
        L.forces_model_free(C.c_void_p(h))
        return None
    return err.value.decode()


def _slider_fan(tmp, n, equalities):
    """n bodies on a limited slider each, all children of the world, colliding with nothing; with `equalities` a one-joint equality
    per slider (set on the compiled model: the rows the table must reserve are what matters here)"""
    import copy
    import softgrip_amd as sg
    bodies = "".join('<body pos="%d 0 1"><joint type="slide" axis="0 0 1" limited="true" range="-1 1"/>'
                     '<geom type="sphere" size="0.1" mass="0.25" contype="0" conaffinity="0"/></body>\n' % k for k in range(n))
    path = os.path.join(str(tmp), "fan_%d.xml" % n)
    with open(path, "w") as f:
        f.write('<mujoco><compiler angle="radian"/><option timestep="0.005" solver="PGS" iterations="30" tolerance="1e-7" cone="elliptic"/>'
                '<worldbody>%s</worldbody></mujoco>' % bodies)
    m = copy.copy(sg.compile_mjcf(path))
    assert m.nv == n and int(np.sum(m.jnt_limited)) == n
    if equalities:
        m.eq_type, m.eq_obj1id, m.eq_obj2id = np.full(n, 2, np.int32), np.arange(n, dtype=np.int32), np.full(n, -1, np.int32)
        m.eq_data, m.eq_solref, m.eq_solimp = np.zeros((n, 5)), np.tile([0.02, 1.0], (n, 1)), np.tile([0.9, 0.95, 0.001, 0.5, 2.0], (n, 1))
    return m


def test_the_table_builder_refuses_by_name(hostlib, work):
    """sgf_build, whose message the three entry points hand on under SG_ERR_MODEL: a candidate pair of condim 4 (mini_gripper with every
    geom's condim raised); an equality that is neither a joint nor a tendon equality; a row list that does not fit the LDS -- 440
    limited sliders with an equality each are 2856 rows, whose directory beside 441 bodies' records is 163 272 bytes, while 400 of them
    (2736 rows) run; a model sg_solve_mass refuses -- a serial chain is not needed: 450 bodies are past sg_get_mass_matrix' limit and
    the message is that read-out's.  sg_model_create itself refuses the first two models for the step kernels' reasons before any
    read-out table counts, so their refusal cannot be reached through the C ABI: this is where those guards are held"""
    import copy
    m = FR.model("mini_gripper")[0]
    bad = copy.copy(m)
    bad.geom_condim = np.full_like(np.asarray(m.geom_condim), 4)
    msg = _refusal(hostlib, bad)
    assert msg and "condim 4 of geoms" in msg and "(1 and 3 only)" in msg, msg
    bad = copy.copy(m)
    bad.eq_type = np.array(m.eq_type).copy()
    bad.eq_type[3] = 1
    msg = _refusal(hostlib, bad)
    assert msg and "equality type 1" in msg and "joint and tendon equalities only" in msg, msg
    assert _refusal(hostlib, m) is None
    msg = _refusal(hostlib, _slider_fan(work, 440, True))
    assert msg and "the row list of 2856 rows" in msg and "(163272 bytes)" in msg and "does not fit the 160 KB of LDS" in msg, msg
    assert _refusal(hostlib, _slider_fan(work, 400, True)) is None
    msg = _refusal(hostlib, _slider_fan(work, 450, False))
    assert msg and "more than 449 bodies" in msg, msg


def test_invalid_arguments_are_refused_under_the_entry_points_own_name():
    """without a device: a NULL batch or model, n_ids <= 0 -- each under the calling entry point's name; the model's row capacity is
    the table's"""
    import softgrip_amd as sg
    from helpers import model_path
    from softgrip_amd import native
    L = native.lib()
    assert L.sg_get_forces(None, None, 1, 1, 1, None, None, None, None, None, None, None, None, None, None) == native.SG_ERR_INVALID
    assert L.sg_last_error().startswith(b"sg_get_forces:") and b"null batch" in L.sg_last_error()
    assert L.sg_model_max_rows(None) == native.SG_ERR_INVALID and L.sg_last_error().startswith(b"sg_model_max_rows:")
    assert L.sg_set_forces_workspace(None, 1 << 20) == native.SG_ERR_INVALID and L.sg_last_error().startswith(b"sg_set_forces_workspace:")
    nm = native.NativeModel(sg.load_model(model_path("softbox_fix")))
    assert L.sg_model_max_rows(nm.ptr) == 111 + 2 * 8 + 3 * 500
    assert {"sg_get_forces", "sg_model_max_rows", "sg_set_forces_workspace"} <= set(native.SYMBOLS)


def test_kernel_resources_of_the_kept_assembly():
    """the kept assembly (sg_readout.device.s): one sg_forces_rows_kernel and one sg_forces_pgs_kernel, 0 bytes of scratch, no VGPR
    spills, static LDS within SGF_STATIC_LDS; the build's assembly check is clean on the file"""
    from softgrip_amd import build_native, devasm, isa_check
    build_native.build()
    api = build_native.device_asm("sg_readout.hip")
    seen = devasm.kernels(open(api).read())
    for name in ("sg_forces_rows_kernel", "sg_forces_pgs_kernel"):
        k = [v for n, v in seen.items() if name in n]
        assert len(k) == 1, sorted(seen)
        assert k[0]["scratch"] == 0 and k[0]["vgpr_spill"] == 0 and k[0]["lds"] <= 1024, (name, k[0])
    assert not isa_check.check_asm(api)


def test_sanitizer_run_of_the_row_builder_and_a_full_solve(work):
    """scripts/sanitize/forces_main.cpp -- a stand-alone program: the tables, the row builder and a full solve on mini_gripper 60 steps
    into the squeeze and on a one-dof slider pushed past its range (one limit row) -- built by g++ with AddressSanitizer and UBSan and
    run on the CPU: no report"""
    import softgrip_amd as sg
    d = str(work)
    files = []
    m = FR.model("mini_gripper")[0]
    st = FR.states("mini_gripper", (60,), work)[60][0]
    xml = open(os.path.join(DR.ROOT, "tests", "data", "slider.xml")).read().replace('stiffness="50"', 'limited="true" range="-0.1 0.1" stiffness="50"')
    with open(os.path.join(d, "limited_slider.xml"), "w") as f:
        f.write(xml)
    one = sg.compile_mjcf(os.path.join(d, "limited_slider.xml"))
    assert one.nv == 1 and int(one.jnt_limited[0]) == 1
    slider = dict(qpos=np.array([0.15]), qvel=np.array([0.3]), warm=np.zeros(1), act=np.zeros(1), k=0.0)
    for name, model, s in (("mini", m, st), ("slider", one, slider)):
        blob, state = os.path.join(d, name + ".blob"), os.path.join(d, name + ".state")
        with open(blob, "wb") as f:
            f.write(model.to_blob())
        act = s["act"] if len(s["act"]) else np.zeros(1)
        np.concatenate([s["qpos"], s["qvel"], s["warm"], act, [s["k"]]]).astype(np.float64).tofile(state)
        files += [blob, state]
    exe = os.path.join(d, "forces_san")
    csrc = os.path.join(DR.ROOT, "soft-grip_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wno-unknown-pragmas", "-I", csrc, "-o", exe,
                           os.path.join(DR.ROOT, "scripts", "sanitize", "forces_main.cpp"), os.path.join(csrc, "sg_tables.cpp")])
    res = subprocess.run([exe] + files, capture_output=True, text=True)
    print(res.stdout)
    assert res.returncode == 0 and res.stdout.rstrip().endswith("ok") and not res.stderr, (res.stdout, res.stderr)
    lines = res.stdout.splitlines()
    assert "contacts 6" in lines[0] and "rows 1 " in lines[1], lines
