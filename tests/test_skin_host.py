"""The soft object's skin without a GPU: the two compilers' skins against each other, the topology of every skin the repository can
build, the blob left alone, the g++ build of the per-ray triangle math (csrc/sg_render.h) against the independent NumPy caster
(tests/skin_ref.py) on single triangles, closed meshes and whole images, the ABI's argument checks and the kept assembly."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import render_ref as R
import skin_ref as S
from helpers import ROOT, model_path

import softgrip_amd as sg

SKIN_SCENES = ["skin_ball", "skin_box"]      # 3 x 3 x 3 ellipsoid, 4 x 3 x 2 box (tests/data/skin)
BLOB_MODELS = [s + v for s in ("softbox", "softcylinder", "softball", "freeball", "fourfinger_softball") for v in ("", "_fix")]


def scene_path(name):
    return os.path.join(ROOT, "tests", "data", "skin", name + ".xml")      # (a folder of their own: tests/data/*.xml is the pinned input set of the plan digests)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return S.build_host(str(tmp_path_factory.mktemp("skin_host")))


@pytest.fixture(scope="module")
def squeezed():
    """oracle states of the two mini scenes after 20 env steps of the squeeze schedule (computed once)"""
    from oracle import oracle as O
    out = {}
    for name in SKIN_SCENES:
        m = sg.compile_mjcf(scene_path(name))
        sim = O.OracleSim(O.OracleModel(m.to_blob()))
        sim.reset(); sim.forward(); sim.step()
        sim.ctrl[:] = -0.2
        for _ in range(20 * 7):
            assert sim.step() == 0
        out[name] = sim.qpos.copy()
        assert np.abs(out[name] - m.qpos0).max() > 1e-3
    return out


def native_skin(path, flags=0):
    """the native compiler's skin: sg_model_compile + sg_model_skin (no device)"""
    from softgrip_amd import native
    L = native.lib()
    ptr = C.c_void_p()
    native.check(L.sg_model_compile(os.fsencode(path), flags, C.byref(ptr)))
    try:
        nv, nf = C.c_int(), C.c_int()
        native.check(L.sg_model_skin(ptr, C.byref(nv), C.byref(nf), None, None, None, None))
        vb, vp = np.empty(nv.value, np.int32), np.empty((nv.value, 3), np.float64)
        fc, rgba = np.empty((nf.value, 3), np.int32), np.empty(4, np.float32)
        native.check(L.sg_model_skin(ptr, None, None, vb.ctypes.data_as(C.c_void_p), vp.ctypes.data_as(C.c_void_p), fc.ctypes.data_as(C.c_void_p),
                                     rgba.ctypes.data_as(C.POINTER(C.c_float))))
        return dict(vert_body=vb, vert_pos=vp, face=fc, rgba=rgba)
    finally:
        L.sg_model_destroy(ptr)


def assert_skins_equal(a, b):
    np.testing.assert_array_equal(a["vert_body"], b["vert_body"])
    np.testing.assert_array_equal(a["face"], b["face"])
    assert a["vert_pos"].shape == b["vert_pos"].shape and np.abs(a["vert_pos"] - b["vert_pos"]).max() <= 1e-15
    assert np.abs(np.asarray(a["rgba"], np.float64) - np.asarray(b["rgba"], np.float64)).max() <= 1e-15


def check_topology(m, skin):
    """nvert = the shell count, V - E + F = 2, every edge in exactly two faces with opposite direction, every face normal at qpos0
    pointing away from the composite's centre body"""
    vb, face = np.asarray(skin["vert_body"]), np.asarray(skin["face"])
    shell = [i for i, n in enumerate(m.body_names) if re.match(r"^.*B\d+_\d+_\d+$", n)]
    assert len(vb) == len(shell) and sorted(vb.tolist()) == shell
    assert len(vb) <= 256 and len(face) <= 512
    directed = {}
    for f in face:
        assert len(set(f.tolist())) == 3
        for k in range(3):
            e = (int(f[k]), int(f[(k + 1) % 3]))
            assert e not in directed, "edge %s runs the same way in two faces" % (e,)
            directed[e] = True
    for (p, q) in directed:
        assert (q, p) in directed, "edge %s has no partner" % ((p, q),)
    V, E, F = len(vb), len(directed) // 2, len(face)
    assert V - E + F == 2 and F == 2 * V - 4
    kin = m.kinematics(np.asarray(m.qpos0, dtype=np.float64))
    verts = S.skin_vertices(skin, kin["xpos"], kin["xmat"])
    centre = set(int(m.body_parentid[b]) for b in vb)
    assert len(centre) == 1
    c = kin["xpos"][centre.pop()]
    a, b, cc = (verts[face[:, k]] for k in range(3))
    n = np.cross(b - a, cc - a)
    out = np.einsum("fi,fi->f", n, (a + b + cc) / 3 - c)
    assert (np.linalg.norm(n, axis=1) > 0).all() and (out > 0).all()


# ---- topology ----
@pytest.mark.parametrize("scene", SKIN_SCENES)
@pytest.mark.parametrize("neighbors", [True, False])
def test_both_compilers_build_the_same_skin(scene, neighbors):
    from softgrip_amd import native
    m = sg.compile_mjcf(scene_path(scene), composite_neighbors=neighbors)
    assert m.skin is not None
    got = native_skin(scene_path(scene), 0 if neighbors else native.SG_COMPILE_NO_NEIGHBORS)
    assert_skins_equal(m.skin, got)
    want = {"skin_ball": (26, 48, 0.01, (0.9, 0.8, 0.2, 1.0)), "skin_box": (24, 44, 0.02, (0.2, 0.7, 0.3, 0.5))}[scene]
    assert (len(got["vert_body"]), len(got["face"])) == want[:2]
    np.testing.assert_array_equal(got["vert_pos"], np.tile([0.0, 0.0, want[2]], (want[0], 1)))
    np.testing.assert_array_equal(got["rgba"], np.array(want[3], np.float32))
    check_topology(m, m.skin)
    # the same routine from the names alone (what a blob-loaded model gets), and through NativeModel, which attaches m.skin
    assert_skins_equal(m.skin, sg.Model.from_blob(m.to_blob()).composite_skin(inflate=want[2], rgba=want[3]))
    assert_skins_equal(m.skin, native.NativeModel(m).skin())


@pytest.mark.parametrize("name", BLOB_MODELS)
def test_composite_skin_of_the_committed_models(name):
    from softgrip_amd import native
    m = sg.load_model(model_path(name))
    assert m.skin is None
    skin = m.composite_skin()
    assert skin is not None
    check_topology(m, skin)
    np.testing.assert_array_equal(skin["rgba"], np.array([0.8, 0.2, 0.1, 1.0], np.float32))
    assert (skin["vert_pos"] == 0).all()
    nm = native.NativeModel(m)
    assert nm.skin() is None and len(skin["vert_body"]) == nm.nelem
    nm.set_skin(skin)
    assert_skins_equal(skin, nm.skin())
    if name.startswith("softball"):
        assert (len(skin["vert_body"]), len(skin["face"])) == (218, 432)


def test_a_model_without_a_composite_has_no_skin():
    m = sg.compile_mjcf(os.path.join(ROOT, "tests", "data", "arm2.xml"))
    assert m.skin is None and m.composite_skin() is None
    assert sg.compile_mjcf(os.path.join(ROOT, "tests", "data", "mini_gripper.xml")).skin is None     # (a composite, but no <skin>)


@pytest.mark.parametrize("scene", SKIN_SCENES)
def test_the_blob_does_not_change_with_the_skin_element(scene, tmp_path):
    from softgrip_amd import native
    text = open(scene_path(scene)).read()
    bare = re.sub(r"\n\s*<skin [^>]*/>", "", text)
    assert bare != text and "<skin" not in bare
    p = tmp_path / (scene + "_bare.xml")
    p.write_text(bare)
    for nb in (True, False):
        assert sg.compile_mjcf(scene_path(scene), nb).to_blob() == sg.compile_mjcf(str(p), nb).to_blob()
    assert native.compile_mjcf_native(scene_path(scene)) == native.compile_mjcf_native(str(p))
    assert native_skin(str(p)) is not None and len(native_skin(str(p))["vert_body"]) == 0


# ---- per-ray math ----
def _random_triangles(rs, n):
    """front-facing triangles 1 .. 5 m from the origin, 0.05 .. 0.5 m across, seen at less than ~84 degrees from their normal"""
    out = []
    while len(out) < n:
        ctr = rs.normal(size=3)
        ctr *= rs.uniform(1.0, 5.0) / np.linalg.norm(ctr)
        tri = ctr + rs.uniform(0.05, 0.5) * rs.normal(size=(3, 3)) * 0.5
        nrm = np.cross(tri[1] - tri[0], tri[2] - tri[0])
        if np.linalg.norm(nrm) < 1e-3:
            continue
        if nrm @ tri[0] > 0:
            tri = tri[[0, 2, 1]]
            nrm = -nrm
        if (-(tri @ nrm) / (np.linalg.norm(nrm) * np.linalg.norm(tri, axis=1))).min() < 0.1:      # (cos of the incidence at every corner)
            continue
        out.append(tri.astype(np.float32))
    return np.array(out)


def test_single_triangles_match_the_numpy_caster(host):
    rs = np.random.RandomState(5)
    n = 4000
    tri = _random_triangles(rs, n)
    idx = np.array([rs.permutation(256)[:3] for _ in range(n)], dtype=np.int32)
    bary = rs.dirichlet((1, 1, 1), n)
    inside = np.arange(n) % 2 == 0
    bary[~inside, 0] = -rs.uniform(1e-3, 0.5, (~inside).sum())           # the other half aims past edge b - c
    bary[~inside, 1:] *= ((1 - bary[~inside, 0]) / bary[~inside, 1:].sum(1))[:, None]
    keep = ~inside | (bary.min(1) > 1e-3)
    target = np.einsum("nk,nkj->nj", bary, tri.astype(np.float64))
    d = (target / np.linalg.norm(target, axis=1, keepdims=True)).astype(np.float32)
    t, w = S.tri_with(host, d, tri[:, 0], tri[:, 1], tri[:, 2], idx)
    d64 = d.astype(np.float64)
    d64 /= np.linalg.norm(d64, axis=1, keepdims=True)
    for i in np.flatnonzero(keep):
        rt, rf, rw = S.cast_triangles(d64[i:i + 1], {int(idx[i, k]): tri[i, k].astype(np.float64) for k in range(3)}, [idx[i]])
        assert np.isfinite(rt[0]) == bool(inside[i]), i
        assert np.isfinite(t[i]) == bool(inside[i]), i
        if inside[i]:
            # fp32: the rounding of n . a and n . d, each ~1e-7 / cos(incidence) relative with cos > 0.1 by construction
            assert abs(t[i] - rt[0]) <= 2e-5 * rt[0], (i, t[i], rt[0])
            np.testing.assert_allclose(w[i] / w[i].sum(), rw[0] / rw[0].sum(), atol=2e-4)
    # back faces are never hit: the same rays against the triangles wound the other way
    tb, _ = S.tri_with(host, d, tri[:, 0], tri[:, 2], tri[:, 1], idx[:, [0, 2, 1]])
    assert np.isinf(tb).all()
    for i in np.flatnonzero(inside)[:200]:
        assert np.isinf(S.cast_triangles(d64[i:i + 1], {int(idx[i, k]): tri[i, k].astype(np.float64) for k in range(3)}, [idx[i, [0, 2, 1]]])[0][0])


def _closed_meshes():
    out = []
    for name, src in (("softball_fix", None), ("skin_box", "xml"), ("skin_ball", "xml")):
        m = sg.compile_mjcf(scene_path(name)) if src else sg.load_model(model_path(name))
        skin = m.skin if src else m.composite_skin()
        kin = m.kinematics(np.asarray(m.qpos0, dtype=np.float64))
        out.append((name, S.skin_vertices(skin, kin["xpos"], kin["xmat"]), np.asarray(skin["face"])))
    return out


def test_closed_meshes_are_watertight_on_shared_edges_and_vertices(host):
    """rays aimed at the vertices and at points on the edges of a closed mesh hit something, in the g++ build and in the reference.
    Left out: the vertices of the outline and the edges that end in one (a front and a back face meet there: a ray aimed at one may
    rightly pass outside by its own rounding)"""
    rs = np.random.RandomState(11)
    for name, verts, face in _closed_meshes():
        ctr = verts.mean(0)
        for trial in range(3):
            away = rs.normal(size=3)
            eye = ctr + away / np.linalg.norm(away) * rs.uniform(3.0, 6.0) * np.linalg.norm(verts - ctr, axis=1).max()      # (outside)
            rel32 = (verts - eye).astype(np.float32)
            rel = rel32.astype(np.float64)
            a, b, c = (rel[face[:, k]] for k in range(3))
            nrm = np.cross(b - a, c - a)
            facing = np.einsum("fi,fi->f", nrm, a) / (np.linalg.norm(nrm, axis=1) * np.linalg.norm(a, axis=1))     # < 0: front
            vfaces = [np.flatnonzero((face == v).any(1)) for v in range(len(verts))]
            clear = lambda fs: (np.abs(facing[fs]) > 1e-3).all() and ((facing[fs] < 0).all() or (facing[fs] > 0).all())  # noqa: E731
            targets = [rel[v] for v in range(len(verts)) if clear(vfaces[v])]
            nv = len(targets)
            edges = {tuple(sorted((int(f[k]), int(f[(k + 1) % 3])))) for f in face for k in range(3)}
            for p, q in sorted(edges):
                fs = np.flatnonzero((face == p).any(1) & (face == q).any(1))
                assert len(fs) == 2
                if clear(fs) and clear(vfaces[p]) and clear(vfaces[q]):      # (1e-4 along the edge is within rounding of its end)
                    for s in (0.5, 0.123, 0.9, 1e-4):
                        targets.append((1 - s) * rel[p] + s * rel[q])
            targets = np.array(targets)
            assert nv >= len(verts) // 4 and len(targets) >= nv + len(edges) // 2      # (enough of either kind left)
            d = (targets / np.linalg.norm(targets, axis=1, keepdims=True)).astype(np.float32)
            t, fi = S.mesh_with(host, d, rel32, face)
            assert np.isfinite(t).all() and (fi >= 0).all(), (name, trial, np.flatnonzero(~np.isfinite(t))[:10].tolist())
            d64 = d.astype(np.float64)
            d64 /= np.linalg.norm(d64, axis=1, keepdims=True)
            rt, rf, _ = S.cast_triangles(d64, rel, face)
            assert np.isfinite(rt).all(), (name, trial)
            assert np.abs(t - rt).max() <= 1e-4
            assert (facing[fi] < 0).all() and (facing[rf] < 0).all()      # front faces only


# ---- whole images ----
def _side_camera(model):
    c = R.default_camera(model)
    c[4], c[5] = 180.0, -25.0
    return c


def _images(host, m, skin, q, what):
    cats = R.categories(m)
    kin = m.kinematics(np.asarray(q, dtype=np.float64))
    gx, gm = R.geom_poses(m, q)
    verts = S.skin_vertices(skin, kin["xpos"], kin["xmat"])
    hidden = S.hidden_geoms(m, skin)
    for cam in (R.default_camera(m), _side_camera(m)):
        for w, h in ((64, 48), (37, 53)):
            ref = S.render(gx, gm, m.geom_type, m.geom_size, cats, cam, w, h, verts, skin["face"], skin["rgba"], hidden)
            d, s, rgba, fidx = S.render_with(host, gx, gm, m.geom_type, m.geom_size, cats, cam, w, h, verts, skin["face"], skin["rgba"], hidden)
            tag = "%s cam %s %dx%d" % (what, cam[4:6], w, h)
            assert (rgba[..., 3] == 255).all()
            S.compare(ref, (d, s, rgba[..., :3]), skin["face"], tag)
            assert (ref[1] == m.ngeom).any() and not np.isin(ref[1], np.flatnonzero(hidden)).any(), tag
            assert not np.isin(s, np.flatnonzero(hidden)).any() and ((s == m.ngeom) == (fidx >= 0)).all(), tag


@pytest.mark.parametrize("scene", SKIN_SCENES)
def test_host_images_match_the_numpy_caster(host, squeezed, scene):
    m = sg.compile_mjcf(scene_path(scene))
    _images(host, m, m.skin, m.qpos0, scene + " qpos0")
    _images(host, m, m.skin, squeezed[scene], scene + " squeezed")


def test_host_image_of_the_432_face_ball(host):
    m = sg.load_model(model_path("softball_fix"))
    skin = m.composite_skin()
    assert len(skin["face"]) == 432      # (more than 256: the kernel's cull takes two passes)
    cats = R.categories(m)
    kin = m.kinematics(np.asarray(m.qpos0, dtype=np.float64))
    gx, gm = R.geom_poses(m, m.qpos0)
    verts, hidden = S.skin_vertices(skin, kin["xpos"], kin["xmat"]), S.hidden_geoms(m, skin)
    assert hidden.sum() == 218
    cam = R.default_camera(m)
    for w, h in ((64, 48), (37, 53)):
        ref = S.render(gx, gm, m.geom_type, m.geom_size, cats, cam, w, h, verts, skin["face"], skin["rgba"], hidden)
        d, s, rgba, fidx = S.render_with(host, gx, gm, m.geom_type, m.geom_size, cats, cam, w, h, verts, skin["face"], skin["rgba"], hidden)
        S.compare(ref, (d, s, rgba[..., :3]), skin["face"], "softball_fix %dx%d" % (w, h))
        assert (s == m.ngeom).mean() > 0.02


def test_the_fold_cap_holds_on_the_states_the_image_tests_use(squeezed):
    """the NumPy reference alone: fold silhouettes stay under 2 % of the image at qpos0 and at the oracle's squeezed states"""
    for scene in SKIN_SCENES:
        m = sg.compile_mjcf(scene_path(scene))
        for q in (m.qpos0, squeezed[scene]):
            for cam in (R.default_camera(m), _side_camera(m)):
                ref = S.render_model(m, m.skin, q, cam, 64, 64)
                assert S.fold_fraction(ref, m.skin["face"]) <= S.FOLD_CAP, (scene, S.fold_fraction(ref, m.skin["face"]))


# ---- ABI ----
def test_set_skin_rejections_leave_the_old_skin_in_place():
    from softgrip_amd import native
    m = sg.compile_mjcf(scene_path("skin_box"))
    nm = native.NativeModel(m)
    L = nm.L
    good = nm.skin()
    vb, vp, fc, col = (np.ascontiguousarray(good[k]) for k in ("vert_body", "vert_pos", "face", "rgba"))

    def call(vb=vb, vp=vp, fc=fc, col=col, nvert=None, nface=None):
        p = lambda x, t=C.c_void_p: None if x is None else x.ctypes.data_as(t)  # noqa: E731
        return L.sg_model_set_skin(nm.ptr, len(vb) if nvert is None else nvert, p(vb), p(vp), len(fc) if nface is None else nface, p(fc),
                                   p(col, C.POINTER(C.c_float)))

    def changed(a, i, v):
        a = a.copy()
        a.reshape(-1)[i] = v
        return a

    INV, MOD = native.SG_ERR_INVALID, native.SG_ERR_MODEL
    cases = [
        (dict(vb=None, nvert=len(vb)), INV), (dict(vp=None), INV), (dict(fc=None, nface=len(fc)), INV), (dict(col=None), INV),
        (dict(vb=changed(vb, 3, m.nbody)), INV), (dict(vb=changed(vb, 0, -1)), INV),
        (dict(fc=changed(fc, 5, len(vb))), INV), (dict(fc=changed(fc, 4, -1)), INV), (dict(fc=changed(fc, 1, fc[0, 0])), INV),
        (dict(vp=changed(vp, 7, np.nan)), INV), (dict(vp=changed(vp, 2, np.inf)), INV), (dict(col=changed(col, 1, np.nan)), INV),
        (dict(vb=np.zeros(257, np.int32), vp=np.zeros((257, 3))), MOD),
        (dict(fc=np.tile(fc[:1], (513, 1))), MOD),
    ]
    for kw, code in cases:
        assert call(**kw) == code, (list(kw), code)
        assert b"sg_model_set_skin" in L.sg_last_error()
        assert_skins_equal(good, nm.skin())
    assert L.sg_model_set_skin(None, 0, None, None, 0, None, None) == INV
    # limits themselves are accepted; nvert = 0 removes the skin
    assert call(vb=np.zeros(256, np.int32), vp=np.zeros((256, 3)), fc=np.tile(np.array([[0, 1, 2]], np.int32), (512, 1))) == 0
    assert len(nm.skin()["face"]) == 512
    nm.set_skin(None)
    assert nm.skin() is None
    nm.set_skin(good)
    assert_skins_equal(good, nm.skin())
    # sg_render_ex's own checks come before any device work
    cam = (C.c_double * 7)(0, 0, 0, 1, 90, -30, 45)
    assert L.sg_render_ex(None, cam, None, 1, 8, 8, 2, None, None, None, None) == INV and b"flag" in L.sg_last_error()
    assert L.sg_render_ex(None, cam, None, 1, 8, 8, 1, None, None, None, None) == INV


def test_skin_kernels_keep_no_scratch_and_five_workgroups_per_cu():
    """the kept assembly: the skin's two kernels without scratch or spills, the render sibling within 128 registers and at five
    workgroups per CU by its LDS; sg_render_kernel itself still at its 21.4 KB"""
    from softgrip_amd import build_native, devasm
    build_native.build()
    api = build_native.device_asm("sg_readout.hip")
    seen = devasm.kernels(open(api).read())
    vert = [v for k, v in seen.items() if "sg_skin_vert_kernel" in k]
    ren = [v for k, v in seen.items() if "sg_rskin_kernel" in k]
    plain = [v for k, v in seen.items() if "sg_render_kernel" in k]
    assert len(vert) == 1 and len(ren) == 1 and len(plain) == 1, sorted(seen)
    for v in vert + ren:
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0, v
    assert ren[0]["vgpr"] + ren[0]["agpr"] <= 128, ren[0]
    assert 5 * ren[0]["lds"] <= 160 * 1024, ren[0]
    assert plain[0]["lds"] == 21392, plain[0]
