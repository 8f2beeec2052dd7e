"""The velocity / tendon / energy read-outs without a GPU: the NumPy reference (tests/dyn_ref.py) pinned to the oracle and to finite
differences of the poses, the g++ build of csrc/sg_dyn.h against that reference (on the scenes' states and over the sweep of random
grippers the device test runs), the per-env stiffness in the spring terms, and the entry
points' argument checks.

Sign convention found for the gravity term (test 1d): the oracle's qfrc_bias is the left-hand side's bias, M qacc + qfrc_bias = applied
forces, so at qvel = 0 it is MINUS the generalised gravity force, i.e. PLUS the gradient of the gravity potential: d E_gravity / d q_d =
+qfrc_bias[d], with E_gravity = -sum m g . xipos as sg_get_energy reports it."""
import os
import re

import numpy as np
import pytest

import dyn_ref as DR

SCENE_NAMES = sorted(DR.SCENES)
H = 1e-6
FD = 1e-8      # finite differences, times max(1, |value|): round-off eps |x| / h ~ 2e-10, truncation h^2 |x'''| ~ 1e-12 -- 50 x margin


@pytest.fixture(scope="module")
def hostlib(tmp_path_factory):
    return DR.build_host(tmp_path_factory.mktemp("dyn_host"))


_REFS = {}


def refs(scene):
    """the reference's outputs for the scene's states, computed once"""
    if scene not in _REFS:
        m, om, sts = DR.states(scene)
        out = []
        for st in sts:
            kj, kt = DR.stiffness(m, scene, st["k"])
            out.append(DR.reference(m, st["qpos"], st["qvel"], kj, kt))
        _REFS[scene] = out
    return _REFS[scene]


@pytest.mark.parametrize("scene", SCENE_NAMES)
def test_reference_matches_the_oracle(scene):
    """(a) gyro channels = R_site' ang[site body]; (b) ten_length; (c) kinetic = 1/2 qvel' qM qvel -- each within 1e-11 of the sum of the
    absolute values of its terms"""
    from oracle import oracle as O
    m, om, sts = DR.states(scene)
    sim = O.OracleSim(om)
    worst = dict(gyro=0.0, length=0.0, kinetic=0.0)
    for st, ref in zip(sts, refs(scene)):
        kj, kt = DR.stiffness(m, scene, st["k"])
        DR.oracle_forward(sim, st["qpos"], st["qvel"], kj, kt)
        cols = DR.dof_columns(m, ref["kin"])
        mv = DR.moved_by(m, cols[3])
        gy = DR.gyro_channels(m)
        assert gy, scene
        for adr, site in gy:
            b = m.site_bodyid[site]
            want = sim.sensordata[adr:adr + 3]
            got = DR.site_xmat(m, ref["kin"], site).T @ ref["ang"][b]
            scale = max(float(np.sum(np.abs(st["qvel"]) * cols[0] * mv[b])), 1e-300)
            worst["gyro"] = max(worst["gyro"], float(np.abs(got - want).max() / scale))
        for t in range(m.ntendon):
            scale = DR.length_scale(m, t, st["qpos"], ref["length"])
            worst["length"] = max(worst["length"], abs(ref["length"][t] - sim.ten_length[t]) / max(scale, 1e-300))
        ke = 0.5 * st["qvel"] @ sim.qM @ st["qvel"]
        worst["kinetic"] = max(worst["kinetic"], abs(ref["energy"][3] - ke) / ref["energy"][3])
    print(scene, worst)
    for name, w in worst.items():
        assert w <= DR.REL, (scene, name, w)


@pytest.mark.parametrize("scene", SCENE_NAMES)
def test_gravity_term_is_the_potential_of_qfrc_bias(scene):
    """(d) at qvel = 0 the central difference of the gravity term along each of 8 seeded dofs equals the oracle's qfrc_bias there"""
    from oracle import oracle as O
    m, om, sts = DR.states(scene)
    sim = O.OracleSim(om)
    st = sts[0]
    zero = np.zeros(m.nv)
    DR.oracle_forward(sim, st["qpos"], zero)
    bias = sim.qfrc_bias.copy()
    rs = np.random.RandomState(7)
    worst = 0.0
    for d in rs.choice(m.nv, 8, replace=False):
        e = np.zeros(m.nv)
        e[d] = 1.0
        ep = DR.reference(m, DR.integrate(m, st["qpos"], e, H), zero)["energy"][0]
        em = DR.reference(m, DR.integrate(m, st["qpos"], e, -H), zero)["energy"][0]
        dev = abs((ep - em) / (2 * H) - bias[d]) / (FD * max(1.0, abs(bias[d])))
        worst = max(worst, dev)
    print(scene, "gravity gradient, worst deviation in units of the bound:", worst)
    assert worst <= 1.0, (scene, worst)


def _vee(R):
    """sin(angle) axis of a rotation matrix: the vector of its skew part (R - R') / 2"""
    return np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / 2


@pytest.mark.parametrize("scene", SCENE_NAMES)
def test_velocities_are_the_time_derivative_of_the_poses(scene):
    """(e) lin, ang and com_lin against central differences of Model.kinematics() at qpos moved by +-h qvel (h = 1e-6; a free joint's
    quaternion by q (x) exp(+-h w / 2)); the angular velocity from the relative rotation R+ R-'"""
    m, om, sts = DR.states(scene)
    worst = 0.0
    for st, ref in zip(sts, refs(scene)):
        kp = m.kinematics(DR.integrate(m, st["qpos"], st["qvel"], H))
        km = m.kinematics(DR.integrate(m, st["qpos"], st["qvel"], -H))
        for b in range(m.nbody):
            lin = (kp["xpos"][b] - km["xpos"][b]) / (2 * H)
            com = lin + (kp["xmat"][b] - km["xmat"][b]) @ m.body_ipos[b] / (2 * H)
            Rr = kp["xmat"][b] @ km["xmat"][b].T
            ang = _vee(Rr) / (2 * H)
            for got, want in ((ref["lin"][b], lin), (ref["com_lin"][b], com), (ref["ang"][b], ang)):
                worst = max(worst, float(np.max(np.abs(got - want) / (FD * np.maximum(1.0, np.abs(want))))))
    print(scene, "pose differences, worst deviation in units of the bound:", worst)
    assert worst <= 1.0, (scene, worst)


@pytest.mark.parametrize("scene", SCENE_NAMES)
def test_host_build_matches_the_reference(scene, hostlib):
    """csrc/sg_dyn.h compiled by g++, all outputs: 1e-12 max(1, max |value|) per array, the energy terms 1e-11 relative to the sum of
    the absolute values of their summands; its poses are Model.kinematics()'.
    fourfinger_softball_fix alone takes dyn_ref.energy_scale's allowance on the tendon-spring term: its volume tendon's length is a
    cancelling sum that comes to 7e-21 .. 9e-20 m, the term to 1e-38 .. 6e-36 J, and the g++ build deviates from NumPy by 0.75 and 0.94 of
    the term in two of the three states (0 in the third); with the allowance REL k |x| sum |coef q| the measured deviation is <= 1.2e-17
    of the scale.  The other four scenes meet the plain bound: measured 3e-15 .. 9e-14 of sum 1/2 k x^2"""
    m, om, sts = DR.states(scene)
    for st, ref in zip(sts, refs(scene)):
        got = DR.host(hostlib, m, scene, st["qpos"], st["qvel"], st["k"])
        for name in ("ang", "lin", "com_lin", "length", "velocity"):
            dev = DR.close(got[name], ref[name])
            assert dev <= 1.0, (scene, name, dev)
        assert DR.close(got["poses"], np.concatenate([ref["kin"]["xpos"], ref["kin"]["xquat"]], 1)) <= 1.0
        kj, kt = DR.stiffness(m, scene, st["k"])
        scale = DR.energy_scale(m, ref, kj, kt, st["qpos"], st["qvel"], allowance=scene in DR.ALLOW_FIXED_TENDON)
        dev = np.abs(got["energy"] - ref["energy"]) / np.maximum(scale, 1e-300)
        print(scene, "energy", got["energy"], "relative deviation", dev)
        assert (dev <= DR.REL).all(), (scene, dev)
        assert (got["ang"][0] == 0).all() and (got["lin"][0] == 0).all() and (got["com_lin"][0] == 0).all()


def test_sweep_of_random_grippers_matches_the_reference(hostlib, tmp_path):
    """the sweep of dyn_ref (contacts_ref's six random grippers, 64 poses each far out of the joint ranges, qvel of scale 0, 1 and 30, a
    stiffness per state; and gripper 3 once more with every hinge's anchor moved off its body's origin) on the g++ build against the NumPy reference: 1e-12 max(1, max |value|) per array, the energy terms 1e-11 of
    the PLAIN scale (no fixed-tendon allowance: every pose moves the sliders, the volume tendon's length does not cancel), poses
    against Model.kinematics().  And what the device test of the same states (tests/test_gpu_dyn.py) relies on the sweep to reach:
    bodies with 1, 2 and 3 joints, a slider on a turning body, a free quaternion off unit length, spatial tendons of 2 sites and of
    >= 5, a fixed tendon, a second or third hinge with an anchor off the body's origin, all three velocity scales -- with every
    velocity output exactly zero at scale 0.
    Measured: arrays <= 1.3e-2 of their bound, energy terms <= 2.7e-13 of their scale, poses <= 5.6e-16"""
    import contacts_ref as CR
    worst = dict(arrays=0.0, energy=0.0, poses=0.0)
    reach = dict(joints_per_body=set(), slider_on_turning_body=False, nonunit_free_quat=False, spatial_sites=set(), fixed_tendon_wraps=set(), scales=set(),
                 later_hinge_off_origin=False)
    states = 0
    assert len(DR.SWEEP_CASES) == CR.SWEEP_GRIPPERS + 1
    for g, offset in DR.SWEEP_CASES:
        m, qpos, qvel, ks, jids, tids = DR.sweep(g, tmp_path, offset)
        refs = []
        for q, v, k in zip(qpos, qvel, ks):
            kj, kt = DR.stiffness(m, None, k, jids, tids)
            ref = DR.reference(m, q, v, kj, kt)
            refs.append(ref)
            got = DR.host(hostlib, m, None, q, v, k, jids, tids)
            for name in ("ang", "lin", "com_lin", "length", "velocity"):
                dev = DR.close(got[name], ref[name])
                worst["arrays"] = max(worst["arrays"], dev)
                assert dev <= 1.0, (g, states, name, dev)
                if not v.any():
                    assert name == "length" or not got[name].any(), (g, states, name)
            dev = float(np.abs(got["poses"] - np.concatenate([ref["kin"]["xpos"], ref["kin"]["xquat"]], 1)).max())
            worst["poses"] = max(worst["poses"], dev)
            assert dev <= 1e-12, (g, states, dev)
            scale = DR.energy_scale(m, ref, kj, kt, q, v)
            dev = np.abs(got["energy"] - ref["energy"]) / np.maximum(scale, 1e-300)
            worst["energy"] = max(worst["energy"], float(dev.max()))
            assert (dev <= DR.REL).all(), (g, states, dev)
            assert v.any() or got["energy"][3] == 0.0
            states += 1
        r = DR.sweep_reach(m, qpos, qvel, refs)
        print("gripper %d%s: %d bodies, %d joints, %s" % (g, " with offset anchors" if offset else "", m.nbody, m.njnt, r))
        for key, val in r.items():
            reach[key] = reach[key] | val
    print("%d states, worst deviations: %s" % (states, worst))
    assert states == (CR.SWEEP_GRIPPERS + 1) * CR.SWEEP_POSES
    assert {1, 2, 3} <= reach["joints_per_body"], reach
    assert reach["slider_on_turning_body"] and reach["nonunit_free_quat"] and reach["later_hinge_off_origin"], reach
    assert 2 in reach["spatial_sites"] and max(reach["spatial_sites"]) >= 5, reach
    assert reach["fixed_tendon_wraps"], reach
    assert reach["scales"] == {0.0, 1.0, 30.0}, reach


@pytest.mark.parametrize("scene", ["softbox_fix", "freeball_fix"])
def test_spring_terms_follow_the_envs_stiffness(scene, hostlib):
    """E(k) = k A + B per spring term, A over the listed joints / tendons and B over the others: B is the term at k = 0 and equals the
    reference's sum over the unlisted ones, (E(k1) - B) / (E(k2) - B) = k1 / k2, and with nothing listed the model's own stiffness
    counts.  Gravity and kinetic terms do not move a bit."""
    m, om, sts = DR.states(scene)
    st = sts[0]
    k1, k2 = 350.0, 1225.0
    e0, e1, e2, own = (DR.host(hostlib, m, scene, st["qpos"], st["qvel"], k)["energy"] for k in (0.0, k1, k2, None))
    kj0, kt0 = DR.stiffness(m, scene, 0.0)
    ref0 = DR.reference(m, st["qpos"], st["qvel"], kj0, kt0)["energy"]
    refown = DR.reference(m, st["qpos"], st["qvel"])["energy"]
    sc = {k: DR.energy_scale(m, DR.reference(m, st["qpos"], st["qvel"], *DR.stiffness(m, scene, k)), *DR.stiffness(m, scene, k), st["qpos"], st["qvel"])
          for k in (0.0, k1, k2, None)}
    for c in (1, 2):
        assert abs(e0[c] - ref0[c]) <= DR.REL * sc[0.0][c], (c, e0[c], ref0[c])
        assert abs(own[c] - refown[c]) <= DR.REL * sc[None][c], (c, own[c], refown[c])
        a1, a2 = e1[c] - e0[c], e2[c] - e0[c]          # k1 A and k2 A, each known to the bounds of its two terms
        d1, d2 = DR.REL * (sc[k1][c] + sc[0.0][c]), DR.REL * (sc[k2][c] + sc[0.0][c])
        assert a1 > 0 and a2 > 0, (c, e0, e1, e2)
        assert abs(a1 * k2 - a2 * k1) <= d1 * k2 + d2 * k1, (c, a1 / a2, k1 / k2)
    for c in (0, 3):
        assert e0[c] == e1[c] == e2[c] == own[c]


def test_invalid_arguments_are_refused_under_the_entry_points_own_name():
    """without a device: n_ids <= 0 and a NULL batch, each under the calling entry point's name"""
    from softgrip_amd import native
    L = native.lib()
    calls = {
        "sg_get_velocities": lambda n: L.sg_get_velocities(None, None, n, None, None, None, None),
        "sg_get_tendons": lambda n: L.sg_get_tendons(None, None, n, None, None, None),
        "sg_get_energy": lambda n: L.sg_get_energy(None, None, n, None, None),
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


def test_dyn_kernel_has_no_scratch_and_no_spills():
    """the kept assembly (sg_readout.device.s: sg_dyn_kernel.h is compiled inside sg_readout.hip): one sg_dyn_kernel, 0 bytes of scratch, no
    VGPR spills, no static LDS beyond the compiler's own; the build's assembly check is clean on the file"""
    from softgrip_amd import build_native, devasm, isa_check
    build_native.build()
    api = build_native.device_asm("sg_readout.hip")
    seen = devasm.kernels(open(api).read())
    dyn = [v for k, v in seen.items() if "sg_dyn_kernel" in k]
    assert len(dyn) == 1, sorted(seen)
    assert dyn[0]["scratch"] == 0 and dyn[0]["vgpr_spill"] == 0, dyn[0]
    # the body limit the entry points refuse beyond (SGD_MAXBODY) counts on this much static LDS: with it the block stays within 64 KB
    hdr = open(os.path.join(DR.ROOT, "soft-grip_amd", "csrc", "sg_dyn.h")).read()
    static = int(re.search(r"#define SGD_STATIC_LDS (\d+)", hdr).group(1))
    assert dyn[0]["lds"] <= static, (dyn[0], static)
    maxbody = (65536 - static) // (13 * 8)
    assert maxbody == 627 and maxbody * 13 * 8 + dyn[0]["lds"] <= 65536
    assert not isa_check.check_asm(api)

