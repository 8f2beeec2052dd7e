"""The mass-matrix / joint-force / inverse-dynamics read-outs without a GPU.  THE YARDSTICK IS THE ORACLE: the g++ build of
csrc/sg_smooth.h and the NumPy reference (tests/smooth_ref.py) are both held to OracleSim.qM and OracleSim.qfrc_bias, on the five scenes'
squeeze states and on every state of the sweep of random grippers on which the oracle's forward pass raises no warning (qM on all of
them); the reference, so pinned, carries the outputs the oracle does not export (passive, actuator, inverse) over the whole sweep.
Beside that: cross-checks of the reference against dyn_ref's energy terms, the linearity of the inverse dynamics in qacc, the body
limit against the kept assembly, the entry points' argument checks, and four deliberate breaks of the header's arithmetic that these
tests must catch.

Bounds: dyn_ref's, unchanged -- ARR max(1, max |value|) per array (dyn_ref.close) for every output, REL for the kinetic identity.
Measured on the CPU (in units of the bound): reference against oracle M <= 2.4e-4, bias <= 2.7e-3; g++ build against oracle M <= 8.0e-4,
bias <= 4.8e-3; g++ build against reference M <= 8.0e-4, bias <= 4.9e-3, passive <= 2.6e-3, actuator <= 7.3e-3, inverse <= 2.9e-3 --
all more than two orders of magnitude inside, so the per-array scale stands for these arrays too."""
import os
import re

import numpy as np
import pytest

import dyn_ref as DR
import smooth_ref as SR

SCENE_NAMES = sorted(DR.SCENES)
OUT = ("M", "bias", "passive", "actuator", "inverse")


@pytest.fixture(scope="module")
def hostlib(tmp_path_factory):
    return SR.build_host(tmp_path_factory.mktemp("smooth_host"))


@pytest.fixture(scope="module")
def sweepdir(tmp_path_factory):
    return tmp_path_factory.mktemp("smooth_sweep")


_SCENE = {}


def scene_inputs(scene):
    """(model, oracle model, [dict(qpos, qvel, k, act, qacc, ref)]): dyn_ref.states() with a seeded activation and acceleration, and
    the reference there; computed once per scene and shared"""
    if scene not in _SCENE:
        m, om, sts = DR.states(scene)
        rs = np.random.RandomState(77)
        out = []
        for e, st in enumerate(sts):
            act, qacc = rs.uniform(-1.0, 1.0, m.nu), SR.QACC_SCALES[e % 3] * rs.standard_normal(m.nv)
            kj, kt = DR.stiffness(m, scene, st["k"])
            out.append(dict(st, act=act, qacc=qacc, ref=SR.reference(m, st["qpos"], st["qvel"], kj, kt, act, qacc)))
        _SCENE[scene] = (m, om, out)
    return _SCENE[scene]


def _worse(worst, key, dev):
    worst[key] = max(worst.get(key, 0.0), float(dev))


def linearity(worst, got, got0):
    """inverse(qacc) - inverse(0) = M qacc and inverse(0) = bias - passive on the build's own outputs, each array known to its own bound
    ARR max(1, max |value|): the bounds of the arrays on both sides add"""
    one = lambda x: DR.ARR * max(1.0, float(np.abs(x).max()))  # noqa: E731
    if "qacc" in got:
        mq = got["M"] @ got["qacc"]
        _worse(worst, "inverse(qacc) - inverse(0) = M qacc",
               np.abs(got["inverse"] - got0["inverse"] - mq).max() / (one(got["inverse"]) + one(got0["inverse"]) + one(mq)))
    _worse(worst, "inverse(0) = bias - passive",
           np.abs(got0["inverse"] - (got0["bias"] - got0["passive"])).max() / (one(got0["inverse"]) + one(got0["bias"]) + one(got0["passive"])))


def check_scene(L, scene, worst, states=None):
    """one scene: the build against the oracle (M, bias) and against the reference (everything), the reference against the oracle"""
    from oracle import oracle as O
    m, om, sts = scene_inputs(scene)
    sim = O.OracleSim(om)
    for st in sts[:states]:
        kj, kt = DR.stiffness(m, scene, st["k"])
        DR.oracle_forward(sim, st["qpos"], st["qvel"], kj, kt)
        ref = st["ref"]
        got = SR.host(L, m, scene, st["qpos"], st["qvel"], st["k"], act=st["act"], qacc=st["qacc"])
        got0 = SR.host(L, m, scene, st["qpos"], st["qvel"], st["k"], act=st["act"], qacc=np.zeros(m.nv))
        for name, orc in (("M", sim.qM), ("bias", sim.qfrc_bias)):
            _worse(worst, "reference %s against the oracle" % name, DR.close(ref[name], orc))
            _worse(worst, "build %s against the oracle" % name, DR.close(got[name], orc))
        for name in OUT:
            _worse(worst, "build %s against the reference" % name, DR.close(got[name], ref[name]))
        assert (got["M"] == got["M"].T).all() and np.isfinite(got["M"]).all(), scene
        linearity(worst, dict(got, qacc=st["qacc"]), got0)


def check_sweep(L, tmp, case, worst, states=None):
    """one gripper of the sweep: as check_scene, qM on every state, qfrc_bias where the oracle's forward pass raises no warning
    -> the number of those states"""
    from oracle import oracle as O
    g, offset = case
    m, qpos, qvel, ks, jids, tids, act, qacc = SR.sweep(g, tmp, offset)
    refs = SR.sweep_refs(g, tmp, offset)
    sim = O.OracleSim(O.OracleModel(m.to_blob()))
    usable = 0
    for e in range(len(ks))[:states]:
        kj, kt = DR.stiffness(m, None, ks[e], jids, tids)
        ref = refs[e]
        got = SR.host(L, m, None, qpos[e], qvel[e], ks[e], jids, tids, act=act[e], qacc=qacc[e])
        got0 = SR.host(L, m, None, qpos[e], qvel[e], ks[e], jids, tids, act=act[e], qacc=np.zeros(m.nv))
        sim.reset()      # (clears the warnings of the state before)
        DR.oracle_forward(sim, qpos[e], qvel[e], kj, kt)
        clean = sim.forward() == 0
        usable += clean
        for name, orc in (("M", sim.qM), ("bias", sim.qfrc_bias)):
            if name == "M" or clean:      # (qM is formed before the collision stage and valid regardless)
                _worse(worst, "reference %s against the oracle" % name, DR.close(ref[name], orc))
                _worse(worst, "build %s against the oracle" % name, DR.close(got[name], orc))
        for name in OUT:
            _worse(worst, "build %s against the reference" % name, DR.close(got[name], ref[name]))
        assert (got["M"] == got["M"].T).all() and np.isfinite(got["M"]).all(), (case, e)
        linearity(worst, dict(got, qacc=qacc[e]), got0)
        ke = 0.5 * qvel[e] @ ref["M"] @ qvel[e]
        _worse(worst, "1/2 qvel' M qvel = the kinetic term", abs(ke - ref["dyn"]["energy"][3]) / (DR.REL * max(ref["dyn"]["energy"][3], 1e-300)) if qvel[e].any() else abs(ke))
    return usable


@pytest.mark.parametrize("scene", SCENE_NAMES)
def test_scenes_match_the_oracle(scene, hostlib):
    """the five scenes' squeeze states (dyn_ref.states: real squeeze velocities), after dyn_ref.oracle_forward: the g++ build's and the
    reference's M and bias against OracleSim.qM and .qfrc_bias, the build's five outputs against the reference, the inverse dynamics'
    linearity (qacc at scales 0, 1 and 1000 over the three states); 1/2 qvel' M qvel against dyn_ref's kinetic term.
    Measured, in units of the bound: against the oracle <= 1.1e-3; against the reference <= 2.6e-3; linearity <= 1.4e-3"""
    worst = {}
    check_scene(hostlib, scene, worst)
    m, om, sts = scene_inputs(scene)
    for st in sts:
        ke, want = 0.5 * st["qvel"] @ st["ref"]["M"] @ st["qvel"], st["ref"]["dyn"]["energy"][3]
        _worse(worst, "1/2 qvel' M qvel = the kinetic term", abs(ke - want) / (DR.REL * want))
    print(scene, {k: "%.2e" % v for k, v in sorted(worst.items())})
    assert len(worst) == 12, sorted(worst)
    for key, dev in worst.items():
        assert dev <= 1.0, (scene, key, dev)


def test_sweep_of_random_grippers_matches_the_oracle_and_the_reference(hostlib, sweepdir):
    """all 448 states of dyn_ref's sweep (six random grippers and gripper 3 with offset anchors, 64 poses each far out of the joint
    ranges, qvel of scale 0, 1 and 30) with an activation in U(-1, 1) and a qacc of scale 0, 1 and 1000 per state: the build's and the
    reference's M against the oracle's qM on every state, bias against its qfrc_bias on the 447 states where sgo_forward raises no
    warning (the count is asserted: a silent drop to nothing fails); the build's five outputs against the reference on all 448; the
    linearity of the inverse dynamics; 1/2 qvel' M qvel against the kinetic term.
    Measured, in units of the bound: reference against oracle M 1.9e-4, bias 2.7e-3; build against oracle M 3.7e-4, bias 4.8e-3; build
    against reference M 3.7e-4, bias 4.9e-3, passive 9.1e-4, actuator 7.3e-3, inverse 2.9e-3; linearity 2.3e-3 and exactly 0"""
    worst, usable, states = {}, 0, 0
    for case in DR.SWEEP_CASES:
        usable += check_sweep(hostlib, sweepdir, case, worst)
        states += len(SR.sweep(case[0], sweepdir, case[1])[3])
    print("%d states, %d with a clean oracle forward pass: %s" % (states, usable, {k: "%.2e" % v for k, v in sorted(worst.items())}))
    assert states == 448 and usable == SR.USABLE_ORACLE_STATES
    assert len(worst) == 12, sorted(worst)
    for key, dev in worst.items():
        assert dev <= 1.0, (key, dev)


# ---- independent cross-checks of the reference itself, at finite-difference accuracy ----
H = 1e-6
# the bound of a central difference here, times max(1, |value|).  Measured: the same differences taken at h = 1e-6 and at h = 2e-6 differ
# by at most 3.6e-9 max(1, |value|) over the scenes (fourfinger_softball_fix; the others <= 4.4e-10: round-off eps E / h of the energies,
# truncation h^2 is below it), the h = 1e-6 difference from the analytic value by at most 3.5e-9: the bound is test_dyn_host.py's FD,
# 1e-8, three times the error between the two step sizes
FD = 1e-8


@pytest.mark.parametrize("scene", SCENE_NAMES)
def test_reference_forces_are_the_gradients_of_the_energy_terms(scene):
    """at qvel = 0, along 6 seeded dofs: the spring part of the reference's passive force is minus the central difference of the two
    spring energies (joint and tendon) of dyn_ref.reference along dyn_ref.integrate, and its bias is plus the central difference of
    the gravity term -- the relation DESIGN 8.5 found for the oracle's qfrc_bias"""
    m, om, sts = scene_inputs(scene)
    st = sts[1]
    kj, kt = DR.stiffness(m, scene, st["k"])
    zero = np.zeros(m.nv)
    ref = SR.reference(m, st["qpos"], zero, kj, kt)
    assert np.abs(ref["passive"] - ref["passive_spring"]).max() == 0.0      # at rest the dampers give nothing
    rs = np.random.RandomState(11)
    worst, steps = 0.0, 0.0
    for d in rs.choice(m.nv, 6, replace=False):
        e = np.zeros(m.nv)
        e[d] = 1.0
        grad = {}
        for h in (H, 2 * H):
            ep = DR.reference(m, DR.integrate(m, st["qpos"], e, h), zero, kj, kt)["energy"]
            em = DR.reference(m, DR.integrate(m, st["qpos"], e, -h), zero, kj, kt)["energy"]
            grad[h] = (ep - em) / (2 * h)
        for got, want2 in ((ref["passive_spring"][d], {h: -(grad[h][1] + grad[h][2]) for h in grad}), (ref["bias"][d], {h: grad[h][0] for h in grad})):
            scale = FD * max(1.0, abs(got))
            worst = max(worst, abs(got - want2[H]) / scale)
            steps = max(steps, abs(want2[H] - want2[2 * H]) / scale)
    print(scene, "in units of the bound: analytic against the h = 1e-6 difference %.3f, h = 1e-6 against h = 2e-6 %.3f" % (worst, steps))
    assert worst <= 1.0, (scene, worst)


# ---- the limits ----
def test_limits_are_pinned_against_the_kept_assembly(hostlib):
    """the kept assembly (sg_readout.device.s): one sg_smooth_kernel, 0 bytes of scratch, no VGPR spills, static LDS within
    SGS_STATIC_LDS; with it 449 bodies, 1024 dofs and 128 tendons fill the 160 KB a workgroup can have and not a byte more; the build's
    assembly check is clean on the file"""
    from softgrip_amd import build_native, devasm, isa_check
    build_native.build()
    api = build_native.device_asm("sg_readout.hip")
    seen = devasm.kernels(open(api).read())
    k = [v for name, v in seen.items() if "sg_smooth_kernel" in name]
    assert len(k) == 1, sorted(seen)
    assert k[0]["scratch"] == 0 and k[0]["vgpr_spill"] == 0, k[0]
    lim = SR.limits(hostlib)
    hdr = open(os.path.join(DR.ROOT, "soft-grip_amd", "csrc", "sg_smooth.h")).read()
    assert int(re.search(r"#define SGS_STATIC_LDS (\d+)", hdr).group(1)) == lim["static_lds"] and k[0]["lds"] <= lim["static_lds"], (k[0], lim)
    assert (lim["maxbody"], lim["maxdof"], lim["maxtendon"]) == (SR.MAXBODY, SR.MAXDOF, SR.MAXTENDON) and lim["lds_max"] == 160 * 1024
    dynamic = 8 * (lim["rec"] * lim["maxbody"] + lim["dof"] * lim["maxdof"] + 2 * lim["maxtendon"])
    assert dynamic + k[0]["lds"] <= lim["lds_max"] < dynamic + 8 * lim["rec"] + lim["static_lds"]
    # the four-finger scene runs
    m = DR.load("fourfinger_softball_fix")
    assert m.nbody <= SR.MAXBODY and m.nv <= SR.MAXDOF and m.ntendon <= SR.MAXTENDON and (m.nbody, m.nv) == (257, 283)
    assert not isa_check.check_asm(api)


def test_invalid_arguments_are_refused_under_the_entry_points_own_name():
    """without a device: n_ids <= 0 and a NULL batch, each under the calling entry point's name"""
    from softgrip_amd import native
    L = native.lib()
    calls = {
        "sg_get_mass_matrix": lambda n: L.sg_get_mass_matrix(None, None, n, None, None),
        "sg_get_joint_forces": lambda n: L.sg_get_joint_forces(None, None, n, None, None, None, None),
        "sg_inverse_dynamics": lambda n: L.sg_inverse_dynamics(None, None, n, None, None, None),
    }
    for name, call in calls.items():
        assert call(1) == native.SG_ERR_INVALID, name
        msg = L.sg_last_error()
        assert msg.startswith(name.encode() + b":") and b"null batch" in msg, (name, msg)
        for n in (0, -3):
            assert call(n) == native.SG_ERR_INVALID, name
            msg = L.sg_last_error()
            assert msg.startswith(name.encode() + b":") and b"n_ids" in msg, (name, msg)
    assert set(calls) <= set(native.SYMBOLS)


# ---- do the tests bite?  Four arithmetic-only breaks of the header, one g++ build each ----
def armature_case(hostlib_or_broken, worst):
    """mini_gripper with a seeded armature of U(0.01, 0.1) per dof: no committed scene and no gripper of the sweep has any, so without
    this case nothing here would see the armature term of M.  The build's and the reference's M against the oracle's qM, and the
    inverse dynamics' linearity, at the scene's first state"""
    from oracle import oracle as O
    m = DR.load("mini_gripper")
    m.dof_armature = np.random.RandomState(3).uniform(0.01, 0.1, m.nv)
    st = DR.states("mini_gripper")[2][0]
    sim = O.OracleSim(O.OracleModel(m.to_blob()))
    DR.oracle_forward(sim, st["qpos"], st["qvel"])
    qacc = np.random.RandomState(4).standard_normal(m.nv)
    ref = SR.reference(m, st["qpos"], st["qvel"], qacc=qacc)
    got = SR.host(hostlib_or_broken, m, "mini_gripper", st["qpos"], st["qvel"], None, qacc=qacc)
    got0 = SR.host(hostlib_or_broken, m, "mini_gripper", st["qpos"], st["qvel"], None, qacc=np.zeros(m.nv))
    assert np.abs(sim.qM - SR.reference(DR.load("mini_gripper"), st["qpos"], st["qvel"])["M"]).max() > 0.005      # the oracle counts it
    _worse(worst, "reference M against the oracle", DR.close(ref["M"], sim.qM))
    _worse(worst, "build M against the oracle", DR.close(got["M"], sim.qM))
    _worse(worst, "build inverse against the reference", DR.close(got["inverse"], ref["inverse"]))
    linearity(worst, dict(got, qacc=qacc), got0)


def test_armature_enters_M(hostlib):
    """the case the four breaks below called for (see armature_case).  Measured: <= 1.3e-4 of the bound"""
    worst = {}
    armature_case(hostlib, worst)
    print({k: "%.2e" % v for k, v in sorted(worst.items())})
    for key, dev in worst.items():
        assert dev <= 1.0, (key, dev)


# what each break must trip, found by running them: the checks whose deviation exceeds its bound on the reduced set below
EXPECT = {
    "gyroscopic term dropped": {"build bias against the oracle", "build bias against the reference", "build inverse against the reference"},
    "free angular columns in world axes": {"build M against the oracle", "build M against the reference", "build bias against the oracle",
                                           "build bias against the reference", "build inverse against the reference", "inverse(qacc) - inverse(0) = M qacc"},
    "tendon damper sign flipped": {"build passive against the reference", "build inverse against the reference"},
    "armature left out of M": {"build M against the oracle", "inverse(qacc) - inverse(0) = M qacc"},
}


@pytest.mark.parametrize("name", sorted(SR.BREAKS))
def test_a_broken_header_is_caught(name, tmp_path, sweepdir):
    """sg_smooth.h with one piece of arithmetic changed (smooth_ref.BREAKS), built by g++ and put through the checks above on a reduced
    set -- softbox_fix's and freeball_fix's first state, 12 states each of the sweep's grippers 1 (free joint) and 2, and the armature
    case: the checks named in EXPECT must fail, and no check that compares the reference with the oracle may move.
    The armature break trips nothing on the scenes and the sweep (none has an armature): test_armature_enters_M is the case added
    for it."""
    L = SR.build_host(tmp_path, patch=name)
    worst = {}
    for scene in ("softbox_fix", "freeball_fix"):
        check_scene(L, scene, worst, states=1)
    for case in ((1, False), (2, False)):
        check_sweep(L, sweepdir, case, worst, states=12)
    plain = dict(worst)
    armature_case(L, worst)
    failed = {k for k, v in worst.items() if not v <= 1.0}
    print(name, "fails:", sorted(failed), {k: "%.2e" % worst[k] for k in sorted(failed)})
    assert failed == EXPECT[name], (name, sorted(failed))
    assert not any(k.startswith("reference") for k in failed)
    if name == "armature left out of M":
        assert not {k for k, v in plain.items() if not v <= 1.0}, "scenes and sweep have no armature"
