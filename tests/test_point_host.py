"""The point read-outs (sg_get_point_motion, sg_get_jacobians) without a GPU.  THE YARDSTICK IS THE ORACLE: with the points placed at
the model's sensor sites and the oracle's OWN qacc fed in, the gyro and accel of the g++ build of csrc/sg_point.h and of the NumPy
reference (tests/point_ref.py) are held to the gyro and accelerometer channels of sgo_forward's sensordata, on the five scenes' squeeze
states and on the sweep of random grippers (accel on the 447 of 448 states where the oracle's forward pass raises no warning); the
reference, so pinned, carries the other outputs over the sites, every body's centre of mass, the world body and random points in
random frames.  Beside that: the reference against central differences of itself, identities on the build's own outputs (J qvel = vel,
linearity in qacc, the Jacobians summed to the oracle's qM), the limits against the kept assembly, the entry points' argument checks,
and four deliberate breaks of the arithmetic that these tests must catch.

Bounds: the project's own.  pos, mat, vel, gyro, jacp, jacr: dyn_ref.ARR max(1, max |value|) per array (dyn_ref.close).  acc and accel:
ARR (1 + max |sample| + max |qacc|) (point_ref.acc_scale), tests/test_tree_emu.py's scale for accelerometer samples.  MEASURED FIRST,
on the CPU, in units of the bound: the reference against the oracle gyro <= 1.1e-3, accel <= 2.7e-4; the build against the oracle
gyro exactly 0 (the oracle walks the tree as the header does), accel <= 2.9e-4; the build against the reference acc <= 1.7e-3,
accel <= 2.7e-3, the other arrays <= 1.1e-3.  Everything sits more than two orders of magnitude inside, also on the 30 rad/s
states: the scale needs no max |w|^2 r term, and has none."""
import os
import re

import numpy as np
import pytest

import dyn_ref as DR
import point_ref as PR
import smooth_ref as SR

SCENE_NAMES = sorted(DR.SCENES)


@pytest.fixture(scope="module")
def hostlib(tmp_path_factory):
    return PR.build_host(tmp_path_factory.mktemp("point_host"))


@pytest.fixture(scope="module")
def sweepdir(tmp_path_factory):
    return tmp_path_factory.mktemp("point_sweep")


def _worse(worst, key, dev):
    worst[key] = max(worst.get(key, 0.0), float(dev))


def _one(x):
    return DR.ARR * max(1.0, float(np.abs(x).max()))


def identities(worst, m, got, got0, qvel, qacc):
    """on the build's own outputs: jacr qvel and jacp qvel are vel; acc(qacc) - acc(0) = J qacc; each side known to its own bound, the
    bounds add"""
    jv = np.concatenate([got["jacr"] @ qvel, got["jacp"] @ qvel], 1)
    _worse(worst, "J qvel = vel", np.abs(jv - got["vel"]).max() / (_one(jv) + _one(got["vel"])))
    ja = np.concatenate([got["jacr"] @ qacc, got["jacp"] @ qacc], 1)
    s = DR.ARR * (PR.acc_scale(got["acc"], qacc) + PR.acc_scale(got0["acc"], None)) + _one(ja)
    _worse(worst, "acc(qacc) - acc(0) = J qacc", np.abs(got["acc"] - got0["acc"] - ja).max() / s)


def mass_identity(worst, m, got, com, qM):
    """sum over the bodies of m jacp' jacp at body_ipos + jacr' R I R' jacr, plus the armature, is the oracle's qM (com: the slice of the
    one-point-per-body group, whose frames are the bodies')"""
    M = np.diag(np.asarray(m.dof_armature, np.float64)).copy()
    jp, jr, mat = got["jacp"][com], got["jacr"][com], got["mat"][com]
    for b in range(1, m.nbody):
        R = mat[b].reshape(3, 3)
        M += m.body_mass[b] * jp[b].T @ jp[b] + jr[b].T @ (R @ np.reshape(m.body_imat[b], (3, 3)) @ R.T) @ jr[b]
    _worse(worst, "sum of J' I J = the oracle's qM", DR.close(M, qM))


def check_state(L, m, sim, q, v, kj, kt, qacc, worst):
    """one state: the oracle's forward pass there; reference and build at the sensor sites with the oracle's qacc against its gyro and
    accelerometer channels; the build against the reference on all of point_ref.points() with the drawn qacc; the identities
    -> (the forward pass raised no warning, gyro channels compared, accel channels compared)"""
    sim.reset()      # (clears the warnings of the state before)
    DR.oracle_forward(sim, q, v, kj, kt)
    clean = sim.forward() == 0
    oq = sim.qacc.copy()
    sb, sp, sq = PR.site_points(m)
    ref = PR.reference(m, q, v, oq, sb, sp, sq)
    got = PR.host(L, m, q, v, oq, sb, sp, sq)
    ngyro = naccel = 0
    for adr, site, kind in PR.sensor_channels(m):
        want = sim.sensordata[adr:adr + 3]
        if kind == "gyro":
            ngyro += 3
            for who, x in (("reference", ref), ("build", got)):
                _worse(worst, "%s gyro against the oracle" % who, DR.close(x["gyro"][site], want))
        elif clean:      # (the accelerometer needs the forward pass's qacc: valid where it raised no warning)
            naccel += 3
            for who, x in (("reference", ref), ("build", got)):
                _worse(worst, "%s accel against the oracle" % who, np.abs(x["accel"][site] - want).max() / (DR.ARR * PR.acc_scale(want, oq)))
    body, pos, quat, groups = PR.points(m)
    ref = PR.reference(m, q, v, qacc, body, pos, quat)
    got = PR.host(L, m, q, v, qacc, body, pos, quat)
    got0 = PR.host(L, m, q, v, None, body, pos, quat)
    for name, dev in PR.deviations(got, ref, qacc).items():
        _worse(worst, "build %s against the reference" % name, dev)
    for name in PR.NAMES:
        assert np.isfinite(got[name]).all(), name
    w = got["accel"][groups["world"]][0]      # a probe on the world reads minus gravity in its own frame
    up = got["mat"][groups["world"]][0].reshape(3, 3).T @ -np.asarray(m.opt_gravity, np.float64)
    _worse(worst, "the world's accelerometer reads -g", np.abs(w - up).max() / _one(up))
    assert not got["vel"][groups["world"]].any() and not got["acc"][groups["world"]].any() and not got["jacp"][groups["world"]].any()
    identities(worst, m, got, got0, v, qacc)
    mass_identity(worst, m, got, groups["com"], sim.qM)
    return clean, ngyro, naccel


def _report(what, worst):
    """every check of check_state was made (4 against the oracle, 8 against the reference, the world's reading, 2 identities, qM) and holds"""
    print(what, {k: "%.2e" % v for k, v in sorted(worst.items())})
    assert len(worst) == 16, sorted(worst)
    for key, dev in worst.items():
        assert dev <= 1.0, (what, key, dev)


@pytest.mark.parametrize("scene", SCENE_NAMES)
def test_scenes_match_the_oracle_and_the_reference(scene, hostlib):
    """the five scenes' squeeze states (dyn_ref.states), a qacc of scale 0, 1 and 1000 over the three: see check_state.  The scenes
    declare 12 or 24 channels, all compared.  Measured, in units of the bound: against the oracle <= 1.9e-4 (the build's gyro exactly
    0); against the reference <= 1.7e-3; identities <= 5.4e-4"""
    from oracle import oracle as O
    m, om, sts = DR.states(scene)
    sim = O.OracleSim(om)
    rs = np.random.RandomState(77)
    worst = {}
    for e, st in enumerate(sts):
        qacc = SR.QACC_SCALES[e % 3] * rs.standard_normal(m.nv)
        clean, ngyro, naccel = check_state(hostlib, m, sim, st["qpos"], st["qvel"], *DR.stiffness(m, scene, st["k"]), qacc, worst)
        assert clean and ngyro == naccel and ngyro + naccel == om.nsensordata and ngyro + naccel in (12, 24), (scene, e, ngyro, naccel)
    _report(scene, worst)


def test_sweep_of_random_grippers_matches_the_oracle_and_the_reference(hostlib, sweepdir):
    """all 448 states of smooth_ref.sweep (six random grippers and gripper 3 with offset anchors, 64 poses each far out of the joint
    ranges, qvel of scale 0, 1 and 30, qacc of scale 0, 1 and 1000): see check_state.  Every gripper declares an accelerometer and a
    gyro per finger; gyro is compared on every state, accel on the 447 where sgo_forward raises no warning (the count is asserted: a
    silent drop to nothing fails).  Measured, in units of the bound: reference against oracle gyro 1.1e-3, accel 2.7e-4; build
    against oracle gyro 0, accel 2.9e-4; build against reference <= 2.7e-3 (accel); identities <= 4.6e-4"""
    from oracle import oracle as O
    worst, usable, states = {}, 0, 0
    for g, offset in DR.SWEEP_CASES:
        m, qpos, qvel, ks, jids, tids, act, qacc = SR.sweep(g, sweepdir, offset)
        sim = O.OracleSim(O.OracleModel(m.to_blob()))
        channels = 0
        for e in range(len(ks)):
            clean, ngyro, naccel = check_state(hostlib, m, sim, qpos[e], qvel[e], *DR.stiffness(m, None, ks[e], jids, tids), qacc[e], worst)
            assert ngyro > 0 and (naccel == ngyro if clean else naccel == 0), (g, offset, e)
            usable += clean
            channels += ngyro + naccel
        assert channels > 0, (g, offset)
        states += len(ks)
    print("%d states, %d with a clean oracle forward pass" % (states, usable))
    assert states == 448 and usable == SR.USABLE_ORACLE_STATES
    _report("sweep", worst)


# ---- independent cross-checks of the reference itself, at finite-difference accuracy (test_dyn_host.py's step and bound) ----
H = 1e-6
FD = 1e-8


def _vee(R):
    return 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])


@pytest.mark.parametrize("scene", SCENE_NAMES)
def test_reference_velocity_and_acceleration_are_time_derivatives(scene):
    """the reference's vel is the central difference of its pos (linear part) and of its mat's rotation (angular part, from
    mat+ mat-') along dyn_ref.integrate; its acc is the central difference of its vel along (integrate, qvel + h qacc): h = 1e-6,
    bound 1e-8 max(1, |value|); the same differences at h and 2h are reported beside.  Sites and the random points, every state"""
    m, om, sts = DR.states(scene)
    body, pos, quat, groups = PR.points(m)
    sel = np.r_[groups["sites"], groups["random"]]
    body, pos, quat = body[sel], pos[sel], quat[sel]
    rs = np.random.RandomState(5)
    worst, steps = 0.0, 0.0
    for st in sts:
        q, v = st["qpos"], st["qvel"]
        qacc = rs.standard_normal(m.nv)
        ref = PR.reference(m, q, v, qacc, body, pos, quat)
        fd = {}
        for h in (H, 2 * H):
            rp = PR.reference(m, DR.integrate(m, q, v, h), v + h * qacc, qacc, body, pos, quat)
            rm = PR.reference(m, DR.integrate(m, q, v, -h), v - h * qacc, qacc, body, pos, quat)
            ang = np.array([_vee(rp["mat"][p].reshape(3, 3) @ rm["mat"][p].reshape(3, 3).T) for p in range(len(body))]) / (2 * h)
            fd[h] = (np.concatenate([ang, (rp["pos"] - rm["pos"]) / (2 * h)], 1), (rp["vel"] - rm["vel"]) / (2 * h))
        for got, k in ((ref["vel"], 0), (ref["acc"], 1)):
            scale = FD * np.maximum(1.0, np.abs(got))
            worst = max(worst, float((np.abs(got - fd[H][k]) / scale).max()))
            steps = max(steps, float((np.abs(fd[H][k] - fd[2 * H][k]) / scale).max()))
    print(scene, "in units of the bound: analytic against the h = 1e-6 difference %.3f, h = 1e-6 against h = 2e-6 %.3f" % (worst, steps))
    assert worst <= 1.0, (scene, worst)


# ---- the limits ----
def test_limits_are_pinned_against_the_kept_assembly(hostlib):
    """the kept assembly (sg_readout.device.s): one sg_point_kernel, 0 bytes of scratch, no VGPR spills, static LDS within
    SGP_STATIC_LDS; with it 672 bodies and 1024 dofs fill the 160 KB a workgroup can have and one body more does not fit; the limits
    are not below sg_get_mass_matrix's; the build's assembly check is clean on the file"""
    from softgrip_amd import build_native, devasm, isa_check
    build_native.build()
    api = build_native.device_asm("sg_readout.hip")
    seen = devasm.kernels(open(api).read())
    k = [v for name, v in seen.items() if "sg_point_kernel" in name]
    assert len(k) == 1, sorted(seen)
    assert k[0]["scratch"] == 0 and k[0]["vgpr_spill"] == 0, k[0]
    lim = PR.limits(hostlib)
    hdr = open(os.path.join(DR.ROOT, "soft-grip_amd", "csrc", "sg_point.h")).read()
    assert int(re.search(r"#define SGP_STATIC_LDS (\d+)", hdr).group(1)) == lim["static_lds"] and k[0]["lds"] <= lim["static_lds"], (k[0], lim)
    assert (lim["maxbody"], lim["maxdof"]) == (PR.MAXBODY, PR.MAXDOF) and lim["lds_max"] == 160 * 1024 and (lim["rec"], lim["dof"]) == (19, 7)
    assert PR.MAXBODY >= SR.MAXBODY and PR.MAXDOF >= SR.MAXDOF
    dynamic = 8 * (lim["rec"] * lim["maxbody"] + lim["dof"] * lim["maxdof"]) + 4 * lim["maxdof"]
    assert dynamic + k[0]["lds"] <= lim["lds_max"] < dynamic + 8 * lim["rec"] + lim["static_lds"]
    m = DR.load("fourfinger_softball_fix")
    assert m.nbody <= PR.MAXBODY and m.nv <= PR.MAXDOF and (m.nbody, m.nv) == (257, 283)
    assert not isa_check.check_asm(api)


def test_point_table_and_sites_follow_the_model():
    """sg_model_nsite / sg_model_sites hand out the model's sites (no device needed), NULL outputs allowed"""
    from softgrip_amd import native
    for scene in ("softbox_fix", "freeball_fix"):
        m = DR.load(scene)
        nm = native.NativeModel(m)
        body, pos, quat = nm.sites()
        sb, sp, sq = PR.site_points(m)
        assert len(body) == m.nsite > 0 and (body == sb).all() and (pos == sp).all() and (quat == sq).all()
        assert nm.L.sg_model_sites(nm.ptr, None, None, None) == 0
    L = native.lib()
    assert L.sg_model_nsite(None) == 0
    assert L.sg_model_sites(None, None, None, None) == native.SG_ERR_INVALID and L.sg_last_error().startswith(b"sg_model_sites:")


def test_invalid_arguments_are_refused_under_the_entry_points_own_name():
    """without a device: n_ids <= 0, n_pts <= 0 and a NULL batch, each under the calling entry point's name"""
    from softgrip_amd import native
    L = native.lib()
    calls = {
        "sg_get_point_motion": lambda n, p: L.sg_get_point_motion(None, None, n, p, None, None, None, None, None, None, None, None, None, None, None, None, None),
        "sg_get_jacobians": lambda n, p: L.sg_get_jacobians(None, None, n, p, None, None, None, None, None, None),
    }
    for name, call in calls.items():
        assert call(1, 1) == native.SG_ERR_INVALID, name
        msg = L.sg_last_error()
        assert msg.startswith(name.encode() + b":") and b"null batch" in msg, (name, msg)
        for n in (0, -3):
            assert call(n, 1) == native.SG_ERR_INVALID, name
            msg = L.sg_last_error()
            assert msg.startswith(name.encode() + b":") and b"n_ids" in msg, (name, msg)
            assert call(1, n) == native.SG_ERR_INVALID, name
            msg = L.sg_last_error()
            assert msg.startswith(name.encode() + b":") and b"n_pts" in msg, (name, msg)
    assert set(calls) <= set(native.SYMBOLS)


# ---- do the tests bite?  Four arithmetic-only breaks, one g++ build each ----
# what each break must trip, found by running them: the checks whose deviation exceeds its bound on the reduced set below
EXPECT = {
    "centripetal term dropped": {"build acc against the reference", "build accel against the reference", "build accel against the oracle"},
    # (the walk's own velocity and acceleration do not pass through the dofs' twists: only the Jacobians move)
    "free angular columns in world axes": {"build jacp against the reference", "build jacr against the reference", "J qvel = vel",
                                           "acc(qacc) - acc(0) = J qacc", "sum of J' I J = the oracle's qM"},
    "gravity's sign flipped in accel": {"build accel against the reference", "build accel against the oracle", "the world's accelerometer reads -g"},
    # (every sensor site of the scenes and of the grippers has the identity for its site_quat, so the oracle's channels cannot see this
    # one; the random points' frames do)
    "pt_quat ignored": {"build mat against the reference", "build gyro against the reference", "build accel against the reference"},
}


@pytest.mark.parametrize("name", sorted(PR.BREAKS))
def test_a_broken_header_is_caught(name, tmp_path, sweepdir):
    """sg_point.h (for the free joint's columns: the walk it takes from sg_smooth.h) with one piece of arithmetic changed
    (point_ref.BREAKS), built by g++ and put through check_state on a reduced set -- softbox_fix's and freeball_fix's first state, 12
    states each of the sweep's grippers 1 (free joint) and 2: the checks named in EXPECT must fail, and no check that compares the
    reference with the oracle may move"""
    from oracle import oracle as O
    L = PR.build_host(tmp_path, patch=name)
    worst = {}
    for scene in ("softbox_fix", "freeball_fix"):
        m, om, sts = DR.states(scene)
        st = sts[0]
        qacc = np.random.RandomState(78).standard_normal(m.nv)
        check_state(L, m, O.OracleSim(om), st["qpos"], st["qvel"], *DR.stiffness(m, scene, st["k"]), qacc, worst)
    for g in (1, 2):
        m, qpos, qvel, ks, jids, tids, act, qacc = SR.sweep(g, sweepdir, False)
        sim = O.OracleSim(O.OracleModel(m.to_blob()))
        for e in range(12):
            check_state(L, m, sim, qpos[e], qvel[e], *DR.stiffness(m, None, ks[e], jids, tids), qacc[e], worst)
    failed = {k for k, v in worst.items() if not v <= 1.0}
    print(name, "fails:", sorted(failed), {k: "%.2e" % worst[k] for k in sorted(failed)})
    assert failed == EXPECT[name], (name, sorted(failed))
    assert not any(k.startswith("reference") for k in failed)
