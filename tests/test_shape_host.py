"""The soft object's read-outs on the CPU (sg_get_skin_vertices, sg_get_shape, sg_get_subtree): the g++ build of csrc/sg_shape.h and of
the table builder in csrc/sg_tables.cpp against known answers and against the NumPy reference of tests/shape_ref.py, the reference's
own identities, the skins of the committed scenes, the builder's refusals and the stand-alone sanitizer program.  Bounds: shape_ref's.
Worst deviations of the g++ build against the reference, in units of the bound: test_host_build_matches_the_reference's docstring."""
import os
import subprocess

import numpy as np
import pytest

import dyn_ref as DR
import shape_ref as SR

SCENES = ("softbox_fix", "softbox", "fourfinger_softball_fix", "freeball_fix")


@pytest.fixture(scope="module")
def hostlib(tmp_path_factory):
    return SR.build_host(tmp_path_factory.mktemp("shape_host"))


def _rot(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


# ---- 1. known answers through the g++ build ----
def test_tetrahedron_known_answers(hostlib):
    """4 vertices and 4 faces, fewer than a wavefront's stride: V = 1/6, A = (3 + sqrt 3) / 2, centroid (1/4, 1/4, 1/4), the central
    second moments of the unit corner tetrahedron, V / 80 (3, 3, 3, -1, -1, -1), at rest;
    moved away from the origin and turned, the same numbers in the turned frame"""
    P, face = SR.tetrahedron()
    assert SR.is_closed(face)
    got = SR.mesh_shape(hostlib, P, np.zeros_like(P), face)
    V = 1.0 / 6.0
    want = np.concatenate([[V, (3 + np.sqrt(3)) / 2], [0.25] * 3, V / 80 * np.array([3, 3, 3, -1, -1, -1.0]), [0.0]])
    assert np.abs(got - want).max() <= 4e-16, got - want
    R, t = _rot([1, 2, 3], 0.7), np.array([3.0, -2.0, 5.0])
    got = SR.mesh_shape(hostlib, P @ R.T + t, np.zeros_like(P), face)
    C = R @ (V / 80 * np.array([[3, -1, -1], [-1, 3, -1], [-1, -1, 3.0]])) @ R.T
    want = np.concatenate([[V, (3 + np.sqrt(3)) / 2], R @ np.full(3, 0.25) + t, [C[x, y] for x, y in SR.PAIRS], [0.0]])
    assert np.abs(got - want).max() <= 2e-15, got - want


def test_box_known_answers_and_the_volume_rate(hostlib):
    """a 0.9 x 1.2 x 1.8 box turned and moved, 8 vertices and 12 faces: V = abc, A = 2 (ab + bc + ca), the centroid, the central second
    moments R V diag(a^2, b^2, c^2) / 12 R' in closed form (all within 1e-15 of the value's scale); under the linear velocity field
    v = G (x - x0) + v0 the rate is V tr G (the off-diagonal and the rigid parts give none)"""
    size = np.array([0.9, 1.2, 1.8])
    P0, face = SR.box_mesh(size)
    assert SR.is_closed(face)
    R, t = _rot([2, -1, 0.5], 1.1), np.array([0.4, 1.7, -0.6])
    P = P0 @ R.T + t
    G = np.array([[0.3, 0.2, -0.5], [0.1, -0.7, 0.4], [0.6, 0.0, 0.9]])
    Vel = (P - np.array([5.0, 1.0, 2.0])) @ G.T + np.array([0.2, -0.1, 0.3])
    got = SR.mesh_shape(hostlib, P, Vel, face)
    V = size.prod()
    C = R @ np.diag(V * size ** 2 / 12) @ R.T
    want = np.concatenate([[V, 2 * (size[0] * size[1] + size[1] * size[2] + size[2] * size[0])], t, [C[x, y] for x, y in SR.PAIRS], [V * np.trace(G)]])
    dev = np.abs(got - want)
    print("box deviations", dev)
    assert dev.max() <= 4e-15, dev
    # the reference restates the same integrals: both agree within the reference's own bounds
    I = SR.mesh_integrals(P, Vel, face)
    assert (np.abs(got - SR.shape_of(I, P[0])) <= SR.shape_bound(I, P)).all()
    # inward winding: the same solid counted negatively
    got_in = SR.mesh_shape(hostlib, P, Vel, face[:, ::-1])
    eps12 = 12 * np.finfo(np.float64).eps      # 12 faces' round-off, relative
    assert abs(got_in[0] + V) <= eps12 * V and np.abs(got_in[2:5] - t).max() <= 4e-15 and abs(got_in[1] - got[1]) <= eps12 * got[1]


def test_zero_volume_gives_nan_in_the_quotients(hostlib):
    """a closed mesh folded flat (all four vertices in one plane): V = 0 exactly, so the centroid and the central moments are NaN --
    no clamping -- while V, A and the rate stay finite"""
    P = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]])
    _, face = SR.tetrahedron()
    got = SR.mesh_shape(hostlib, P, np.zeros_like(P), face)
    assert got[0] == 0.0 and got[1] > 0 and got[11] == 0.0 and np.isnan(got[2:11]).all(), got


# ---- 2. the g++ build against the NumPy reference ----
@pytest.mark.parametrize("scene", SCENES)
def test_host_build_matches_the_reference(hostlib, scene):
    """dyn_ref.states (the oracle's squeeze, 3 stiffnesses): every output of the three calls for the composite skin, in the object's
    frame and with six directions (two palm-fixed), against the reference.  Worst deviations in units of the bound, over the four
    scenes (measured): pos 1.8e-4, vel 1.1e-4, local 4.4e-4, V 2.3e-5, A 1.8e-5, centroid 4.9e-5, moments 7.3e-5, rate 1.6e-5, extents
    1.7e-4, com 2.1e-4, linvel 1.7e-4, angmom 6.0e-5"""
    m, _, sts = DR.states(scene)
    skin = m.composite_skin()
    H = SR.Host(hostlib, m)
    assert H.set_skin(skin) is None and H.closed == 1
    dirs, db = SR.directions(m, 3)
    worst = {}
    for e, st in enumerate(sts):
        ref = SR.reference(m, skin, st["qpos"], st["qvel"], H.root, dirs, db)
        assert ref["integrals"]["V"] > 1.0
        SR.compare(H.env(st["qpos"], st["qvel"], H.root, dirs, db), ref, "%s env %d" % (scene, e), worst)
    print(scene, {k: "%.2e" % v for k, v in sorted(worst.items())})


def test_outputs_do_not_depend_on_what_else_is_asked(hostlib):
    """sgh_host_env with the shape left out, other directions beside one and another frame: the remaining outputs keep their bits"""
    m, _, sts = DR.states("softbox_fix")
    H = SR.Host(hostlib, m)
    H.set_skin(m.composite_skin())
    dirs, db = SR.directions(m, 3)
    st = sts[0]
    full = H.env(st["qpos"], st["qvel"], H.root, dirs, db)
    part = H.env(st["qpos"], st["qvel"], -1, dirs[[5, 3]], db[[5, 3]], shape=False)
    assert (part["pos"] == full["pos"]).all() and (part["local"] == full["pos"]).all() and (part["com"] == full["com"]).all()
    for name in ("lo", "hi", "lo_vert", "hi_vert"):
        assert (part[name] == full[name][[5, 3]]).all(), name


# ---- 3. the volume rate against a central difference of the reference's own volume ----
@pytest.mark.parametrize("scene", ["softbox_fix", "freeball_fix"])
def test_volume_rate_is_the_derivative_of_the_volume(scene):
    """V(q (+) h qvel) - V(q (-) h qvel) over 2h at h = 1e-4, qpos moved as mj_integratePos moves it, against the reference's dV/dt:
    within 1e-9 of the sum of the absolute values of the rate's summands (measured on softbox_fix: 1.2e-12 against a sum of 0.18)"""
    m, _, sts = DR.states(scene)
    skin = m.composite_skin()
    h = 1e-4
    for st in sts:
        ref = SR.reference(m, skin, st["qpos"], st["qvel"])
        vol = [SR.reference(m, skin, DR.integrate(m, st["qpos"], st["qvel"], s * h), st["qvel"])["integrals"]["V"] for s in (1, -1)]
        fd = (vol[0] - vol[1]) / (2 * h)
        print(scene, "fd", fd, "rate", ref["integrals"]["rate"], "sum |summands|", ref["integrals"]["absrate"])
        assert abs(fd - ref["integrals"]["rate"]) <= 1e-9 * ref["integrals"]["absrate"]


# ---- 4. closedness and the object's body ----
@pytest.mark.parametrize("scene", SR.SCENES_SKIN)
def test_committed_skins_are_closed_and_rooted(hostlib, scene):
    """every committed scene's composite skin: closed (the builder and the Python restatement agree), wound outward (V > 0 at qpos0,
    equal to sum |det| / 6), 1 -> 0 after dropping one face and after reversing one face, -1 without a skin; the object is body 10 in
    the two-finger scenes and body 38 in the four-finger scenes; rest positions in the object's frame against the reference"""
    m = SR.load(scene)
    skin = m.composite_skin()
    H = SR.Host(hostlib, m)
    assert H.closed == -1 and H.root == -1 and H.nvert == 0
    assert H.set_skin(skin) is None
    assert H.closed == 1 and SR.is_closed(skin["face"])
    assert H.root == (38 if scene.startswith("fourfinger") else 10)
    assert all(int(p) < i for i, p in enumerate(m.body_parentid) if i > 0)
    ref = SR.reference(m, skin, m.qpos0, np.zeros(m.nv), H.root)
    I = ref["integrals"]
    assert I["V"] > 1.0 and abs(I["V"] - I["absV"]) <= 1e-12 * I["absV"]
    assert DR.close(H.rest(H.root), ref["local"]) <= 1.0 and DR.close(H.rest(-1), ref["pos"]) <= 1.0
    dropped = dict(skin, face=skin["face"][:-1])
    assert H.set_skin(dropped) is None and H.closed == 0 and not SR.is_closed(dropped["face"])
    rev = skin["face"].copy()
    rev[7] = rev[7, ::-1]
    assert H.set_skin(dict(skin, face=rev)) is None and H.closed == 0 and not SR.is_closed(rev)
    twice = dict(skin, face=np.concatenate([skin["face"], skin["face"][:1]]))
    assert H.set_skin(twice) is None and H.closed == 0
    assert H.set_skin(None) is None and H.closed == -1 and H.root == -1


def test_root_of_skins_bound_across_the_tree(hostlib):
    """vertices on one element: that body; on an element and a finger link: their deepest common ancestor; on the world: body 0"""
    m = SR.load("softbox_fix")
    H = SR.Host(hostlib, m)
    P, face = SR.tetrahedron()
    par = np.asarray(m.body_parentid)
    for bodies in ([15, 15, 15, 15], [15, 40, 100, 11], [15, 3, 15, 15], [0, 15, 15, 15], [5, 5, 6, 6]):
        H.set_skin(SR.skin_of(bodies, P, face))
        anc = None
        for b in bodies:
            chain = [b]
            while chain[-1] != 0:
                chain.append(int(par[chain[-1]]))
            anc = set(chain) if anc is None else anc & set(chain)
        assert H.root == max(anc), (bodies, H.root)


# ---- 5. the subtree rows ----
@pytest.mark.parametrize("scene", SCENES)
def test_subtree_identities(hostlib, scene):
    """the g++ build's rows: com[0] = sum m xipos / sum m and M linvel[0] = sum m com_lin over the whole model; a leaf's row is the body
    itself with angmom = R I R' w; angmom[0] equals the direct sum about com[0]; the subtree masses are the reference's"""
    m, _, sts = DR.states(scene)
    H = SR.Host(hostlib, m)
    mass = np.asarray(m.body_mass, np.float64)
    sub = SR.subtree_lists(m)
    assert np.abs(H.subtree_mass() - np.array([mass[s].sum() for s in sub])).max() <= 1e-13 * mass.sum()
    assert H.nlist == sum(len(s) for s in sub)
    st = sts[1]
    got = H.env(st["qpos"], st["qvel"])
    ref = SR.reference(m, None, st["qpos"], st["qvel"])
    SR.compare(got, ref, scene, skin=False)
    d = ref["dyn"]
    M = mass.sum()
    tol = SR.REL * np.abs(mass[:, None] * d["xipos"]).sum(0) / M + SR.REL * np.abs(got["com"][0])
    assert (np.abs(got["com"][0] - (mass[:, None] * d["xipos"]).sum(0) / M) <= tol).all()
    tol = SR.REL * np.abs(mass[:, None] * d["com_lin"]).sum(0)
    assert (np.abs(M * got["linvel"][0] - (mass[:, None] * d["com_lin"]).sum(0)) <= tol + SR.REL * M * np.abs(got["linvel"][0])).all()
    leaf = max(i for i, s in enumerate(sub) if len(s) == 1 and mass[i] > 0)
    R = d["kin"]["xmat"][leaf]
    spin = R @ np.reshape(m.body_imat[leaf], (3, 3)) @ R.T @ d["ang"][leaf]
    assert DR.close(got["com"][leaf], d["xipos"][leaf]) <= 1.0 and DR.close(got["linvel"][leaf], d["com_lin"][leaf]) <= 1.0
    assert (np.abs(got["angmom"][leaf] - spin) <= ref["bound_angmom"][leaf]).all() and ref["bound_angmom"][leaf].max() <= 1e-11 * max(1.0, np.abs(spin).max())
    direct = sum(ref["dyn"]["kin"]["xmat"][b] @ np.reshape(m.body_imat[b], (3, 3)) @ ref["dyn"]["kin"]["xmat"][b].T @ d["ang"][b]
                 + mass[b] * np.cross(d["xipos"][b] - got["com"][0], d["com_lin"][b]) for b in range(1, m.nbody))
    assert (np.abs(got["angmom"][0] - direct) <= ref["bound_angmom"][0]).all()


# ---- 6. builder refusals, limits and the sanitizer program ----
def test_builder_refusals(hostlib):
    """an LDS block past 160 KB is refused with the limit named, before any array is read (22 doubles per body and 6 per vertex: 1000
    bodies); a vertex bound to a body that does not exist and a face with a vertex that does not exist are refused by name"""
    import ctypes as C
    lim = np.zeros(6, np.int32)
    hostlib.shp_limits(lim.ctypes.data_as(C.c_void_p))
    assert list(lim) == [160 * 1024, 256, 22, 6, 256, 12]
    err = C.create_string_buffer(512)
    assert hostlib.shp_refusal(1000, 0, err, 512) == 0 and b"160 KB of LDS" in err.value and b"1000 bodies" in err.value, err.value
    assert hostlib.shp_refusal(10, 30000, err, 512) == 0 and b"160 KB of LDS" in err.value
    m = SR.load("softbox_fix")
    H = SR.Host(hostlib, m)
    P, face = SR.tetrahedron()
    assert "vertex body" in H.set_skin(SR.skin_of([0, 1, 2, m.nbody], P, face))
    bad = face.copy()
    bad[2, 1] = 4
    assert "face vertex" in H.set_skin(SR.skin_of([0, 1, 2, 3], P, bad))
    assert H.set_skin(SR.skin_of([0, 1, 2, 3], P, face)) is None and H.closed == 1


def test_kernel_resources_in_the_kept_assembly():
    """sg_shape_kernel in the kept device assembly of sg_readout.hip: no scratch, no spilled vector registers, and the static LDS the
    header's limit reserves (SGH_STATIC_LDS)"""
    import re
    import softgrip_amd  # noqa: F401
    from softgrip_amd import build_native, devasm
    k = [rec for name, rec in devasm.kernels(open(build_native.device_asm("sg_readout.hip")).read()).items() if "sg_shape_kernel" in name]
    assert len(k) == 1
    hdr = open(os.path.join(DR.ROOT, "soft-grip_amd", "csrc", "sg_shape.h")).read()
    assert k[0]["scratch"] == 0 and k[0]["vgpr_spill"] == 0 and k[0]["lds"] <= int(re.search(r"#define SGH_STATIC_LDS (\d+)", hdr).group(1)), k[0]


def test_invalid_arguments_are_refused_under_the_entry_points_own_name():
    """without a device: a NULL batch under each entry point's name, and the host queries on a NULL model"""
    from softgrip_amd import native
    L = native.lib()
    calls = {
        "sg_get_skin_vertices": lambda: L.sg_get_skin_vertices(None, None, 1, -1, None, None, None, None),
        "sg_get_shape": lambda: L.sg_get_shape(None, None, 1, 0, None, None, None, None, None, None, None, None),
        "sg_get_subtree": lambda: L.sg_get_subtree(None, None, 1, None, None, None, None),
        "sg_model_skin_closed": lambda: L.sg_model_skin_closed(None),
        "sg_model_skin_root": lambda: L.sg_model_skin_root(None),
        "sg_model_skin_rest": lambda: L.sg_model_skin_rest(None, -1, None),
        "sg_model_subtree_mass": lambda: L.sg_model_subtree_mass(None, None),
    }
    for name, call in calls.items():
        assert call() == native.SG_ERR_INVALID, name
        assert L.sg_last_error().startswith(name.encode() + b":"), (name, L.sg_last_error())
    assert set(calls) <= set(native.SYMBOLS)


def test_model_queries_through_the_library():
    """sg_model_skin_closed / _root / _rest / sg_model_subtree_mass of the product library need no device: softbox_fix before and after
    its composite skin is attached, against the reference"""
    from softgrip_amd import native
    m = SR.load("softbox_fix")
    nm = native.NativeModel(m)
    if nm.skin() is not None:
        nm.set_skin(None)
    assert nm.skin_closed() == -1 and nm.skin_root() == -1
    with pytest.raises(native.SoftgripError) as e:
        nm.skin_rest(-1)
    assert e.value.code == native.SG_ERR_MODEL and "no skin" in str(e.value)
    skin = m.composite_skin()
    nm.set_skin(skin)
    assert nm.skin_closed() == 1 and nm.skin_root() == 10
    ref = SR.reference(m, skin, m.qpos0, np.zeros(m.nv), 10)
    assert DR.close(nm.skin_rest(10), ref["local"]) <= 1.0 and DR.close(nm.skin_rest(-1), ref["pos"]) <= 1.0
    assert np.abs(nm.subtree_mass() - ref["subtree_mass"]).max() <= 1e-13 * ref["subtree_mass"][0]
    with pytest.raises(native.SoftgripError) as e:
        nm.skin_rest(m.nbody)
    assert e.value.code == native.SG_ERR_INVALID
    nm.set_skin(dict(skin, face=skin["face"][:-1]))
    assert nm.skin_closed() == 0


def test_sanitizer_run_of_the_builder_and_the_per_lane_functions(tmp_path):
    """scripts/sanitize/shape_main.cpp -- a stand-alone program: sgh_build, sgh_rest and sgh_host_env (every per-lane function, in the
    kernel's order) on softbox_fix and on the free ball a squeeze in, with the skin closed, open, a tetrahedron on the world and no skin,
    and the LDS refusal -- built by g++ with AddressSanitizer and UBSan and run on the CPU: no report, every verdict as expected"""
    exe = str(tmp_path / "shape_san")
    csrc = os.path.join(DR.ROOT, "soft-grip_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wno-unknown-pragmas", "-I", csrc, "-o", exe,
                           os.path.join(DR.ROOT, "scripts", "sanitize", "shape_main.cpp"), os.path.join(csrc, "sg_tables.cpp")])
    args = []
    for scene in ("softbox_fix", "freeball_fix"):
        m, _, sts = DR.states(scene)
        skin = m.composite_skin()
        paths = [str(tmp_path / (scene + ext)) for ext in (".blob", ".ints", ".dbl")]
        with open(paths[0], "wb") as f:
            f.write(m.to_blob())
        np.concatenate([[len(skin["vert_body"]), len(skin["face"])], skin["vert_body"], skin["face"].reshape(-1)]).astype(np.int32).tofile(paths[1])
        np.concatenate([np.asarray(skin["vert_pos"], np.float64).reshape(-1), sts[0]["qpos"], sts[0]["qvel"]]).astype(np.float64).tofile(paths[2])
        args += paths
    res = subprocess.run([exe] + args, capture_output=True, text=True)
    print(res.stdout)
    assert res.returncode == 0 and res.stdout.rstrip().endswith("ok") and res.stdout.count("refused") == 2 and not res.stderr, (res.stdout, res.stderr)
