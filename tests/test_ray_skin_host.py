"""sg_ray with SG_RAY_SKIN without a GPU: the g++ build of csrc/sg_ray_skin.h + sg_ray.h -- the per-ray math both kernel layouts run -- against
the independent NumPy caster (tests/ray_skin_ref.py), known answers on single triangles, watertightness on the ball's skin, categories and
exclusion, the ABI entry point's checks that need no device, the kept assembly of the three new kernels, a sanitizer run of the host walk
as a stand-alone program, and ManEnv.tactile_depth(skin=True)'s ray construction and gap arithmetic over a batch that casts on the host."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ray_ref as RR
import ray_skin_ref as RS
from helpers import ROOT, model_path
from test_render_host import perturbed

import softgrip_amd as sg

SCENES = ["softbox", "softball", "fourfinger_softball", "freeball"]
REG_LIMIT_RAYS = 96     # the lane-per-ray kernel's registers (five waves per SIMD; its LDS allows three)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return RS.build_host(str(tmp_path_factory.mktemp("ray_skin_host")))


def _geoms(m):
    return np.asarray(m.geom_type), np.asarray(m.geom_size, dtype=np.float64), RR.categories(m), np.asarray(m.geom_bodyid)


def _state(host, m, skin, q):
    """geom poses, body poses and the skin's vertices of a state: the reference's and the host build's (within 1e-12 of each other)"""
    gx, gm = RR.geom_poses(m, q)
    kin = m.kinematics(np.asarray(q, dtype=np.float64))
    verts = RS.vertices(skin, kin["xpos"], kin["xquat"])
    hv = RS.vertices_with(host, skin, kin["xpos"], kin["xquat"])
    assert np.abs(hv - verts).max() <= 1e-12
    return gx, gm, kin, verts, hv


@pytest.mark.parametrize("scene", SCENES)
def test_host_build_matches_numpy_caster(host, scene):
    """256 rays of the test recipe per state, world frame; then the same rays bound to a moving body with that body excluded, a category
    mask without the ground and max_dist = 2.  Ids exact (so the face too), distances and normals within 1e-9 (both sides fp64), both
    reduction orders bit-identical.  Left out: only rays the reference itself marks unstable, at most 2 % of a comparison"""
    m = sg.load_model(model_path(scene))
    skin = m.composite_skin()
    assert skin is not None
    ty, sz, cats, gb = _geoms(m)
    ng = len(ty)
    left = total = on_skin = 0
    for k, q in enumerate([np.array(m.qpos0, dtype=np.float64)] + [perturbed(m, s) for s in range(3)]):
        gx, gm, kin, verts, hv = _state(host, m, skin, q)
        o, d = RR.scene_rays(gx, ty, 256, 100 + k)
        ref = RS.cast(gx, gm, ty, sz, cats, gb, skin, verts, o, d)
        got = RS.cast_with(host, gx, gm, ty, sz, cats, gb, skin, hv, o, d)
        alt = RS.cast_with(host, gx, gm, ty, sz, cats, gb, skin, hv, o, d, layout=1)
        for x, y in zip(got, alt):
            assert x.tobytes() == y.tobytes(), (scene, k)
        edge = RS.unstable(gx, gm, ty, sz, cats, gb, skin, verts, o, d, RR.ALL_BITS, None, 0.0, ref)
        left += RR.compare(got, ref, edge, "%s state %d" % (scene, k))
        total += len(o)
        on_skin += int((ref[1] >= ng).sum())
        assert not np.isin(ref[1], np.flatnonzero(RS.hidden_geoms(gb, skin))).any()
        # body-frame rays with exclusion, a category mask without the ground and a distance limit
        body = int(np.flatnonzero(np.asarray(m.body_weldid) != 0)[k % 5])
        R = kin["xmat"][body]
        ol, dl = (o - kin["xpos"][body]) @ R, d @ R                     # the same world rays, written in the body's frame
        rb = np.full(len(o), body, np.int32)
        mask = RR.ALL_BITS & ~RR.GROUND_BIT
        ow, dw = RR.map_rays(kin["xpos"], kin["xquat"], ol, dl, rb)
        ref2 = RS.cast(gx, gm, ty, sz, cats, gb, skin, verts, ow, dw, mask, rb, 2.0)
        edge2 = RS.unstable(gx, gm, ty, sz, cats, gb, skin, verts, ow, dw, mask, rb, 2.0, ref2)
        got2 = [RS.cast_with(host, gx, gm, ty, sz, cats, gb, skin, hv, ol, dl, kin["xpos"], kin["xquat"], rb, rb, mask, 2.0, layout) for layout in (0, 1)]
        for x, y in zip(*got2):
            assert x.tobytes() == y.tobytes(), (scene, k)
        RR.compare(got2[0], ref2, edge2, "%s state %d body %d" % (scene, k, body))
        hit = ref2[1][(ref2[1] >= 0) & (ref2[1] < ng)]
        assert not ((gb[hit] == body) | (cats[hit] == 0)).any() and (ref2[0] <= 2.0).all()
    print("%s: %d rays, %d on the skin, %d left out" % (scene, total, on_skin, left))
    assert on_skin >= 0.25 * total


# ---- one triangle: a = (-1, -.25, -1), b = (2, -.25, -1), c = (-1, -.25, 2) faces -y (n = (0, -9, 0)), bound to body 1; geoms ride on body 0 ----
TRI = dict(vert_body=np.array([1, 1, 1]), vert_pos=np.zeros((3, 3)), face=np.array([[0, 1, 2]]), rgba=np.ones(4))
TRI_VERTS = np.array([[-1.0, -0.25, -1.0], [2.0, -0.25, -1.0], [-1.0, -0.25, 2.0]])
NO_GEOMS = (np.zeros((0, 3)), np.zeros((0, 3, 3)), np.zeros(0, int), np.zeros((0, 3)), np.zeros(0, int), np.zeros(0, int))
SPHERE = (np.zeros((1, 3)), np.eye(3)[None], np.array([RR.SPHERE]), np.array([[0.25, 0.0, 0.0]]), np.array([1]), np.array([0]))


def _both(host, geoms, skin, verts, o, d, **kw):
    """the host build (both reduction orders) and the reference on one ray -> (dist, id, normal) of the host, checked equal"""
    gx, gm, ty, sz, cats, gb = geoms
    ref = RS.cast(gx, gm, ty, sz, cats, gb, skin, verts, [o], [d], kw.get("cat_mask", RR.ALL_BITS), kw.get("exclude"), kw.get("max_dist", 0.0))
    out = None
    for layout in (0, 1):
        got = RS.cast_with(host, gx, gm, ty, sz, cats, gb, skin, verts, [o], [d], layout=layout, **kw)
        assert got[1][0] == ref[1][0] and abs(got[0][0] - ref[0][0]) <= 1e-12 and np.abs(got[2][0] - ref[2][0]).max() <= 1e-12, (got, ref)
        out = got
    return out[0][0], out[1][0], out[2][0]


def test_known_answers_on_one_triangle(host):
    # head-on, and slanted: distance and the flat normal analytically
    dist, gid, n = _both(host, NO_GEOMS, TRI, TRI_VERTS, (0, -3, 0), (0, 2, 0))
    assert gid == 0 and dist == 2.75 and n.tolist() == [0, -1, 0]
    dist, gid, n = _both(host, NO_GEOMS, TRI, TRI_VERTS, (-0.5 - 1.5, -0.25 - 2.0, 0.25), (3, 4, 0))
    assert gid == 0 and abs(dist - 2.5) < 1e-12 and np.abs(n - (0, -1, 0)).max() < 1e-12
    # from behind, edge-on, with the origin past the plane, and beside the triangle: misses
    for o, d in (((0, 3, 0), (0, -1, 0)), ((-3, -0.25, 0), (1, 0, 0)), ((0, 0, 0), (0, 1, 0)), ((0, 0, 0), (0, -1, 0)), ((1.5, -3, 1.5), (0, 1, 0))):
        dist, gid, n = _both(host, NO_GEOMS, TRI, TRI_VERTS, o, d)
        assert (dist, gid) == (-1.0, -1) and not n.any(), (o, d)
    # the winding decides the side: the same vertices wound the other way are seen from +y only
    flip = dict(TRI, face=np.array([[0, 2, 1]]))
    assert _both(host, NO_GEOMS, flip, TRI_VERTS, (0, -3, 0), (0, 1, 0))[1] == -1
    dist, gid, n = _both(host, NO_GEOMS, flip, TRI_VERTS, (0, 3, 0), (0, -1, 0))
    assert gid == 0 and dist == 3.25 and n.tolist() == [0, 1, 0]
    # max_dist 1e-9 short of the hit and 1e-9 past it
    assert _both(host, NO_GEOMS, TRI, TRI_VERTS, (0, -3, 0), (0, 1, 0), max_dist=2.75 - 1e-9)[1] == -1
    dist, gid, _ = _both(host, NO_GEOMS, TRI, TRI_VERTS, (0, -3, 0), (0, 1, 0), max_dist=2.75 + 1e-9)
    assert gid == 0 and dist == 2.75
    # a direction without length, or not finite: a miss
    for dd in ((0, 0, 0), (np.nan, 1, 0), (0, np.inf, 0)):
        got = RS.cast_with(host, *NO_GEOMS, TRI, TRI_VERTS, [(0, -3, 0)], [dd])
        assert got[0][0] == -1.0 and got[1][0] == -1 and not got[2].any()
    # (a ray aimed at the lone triangle's own border may rightly pass outside by its rounding: closed meshes, test_watertight_on_the_ball)


def test_tie_rules(host):
    # two coincident faces: the smaller index wins, in both reduction orders, whichever comes first in the list
    two = dict(TRI, face=np.array([[0, 1, 2], [0, 1, 2]]))
    assert _both(host, NO_GEOMS, two, TRI_VERTS, (0, -3, 0), (0, 1, 0))[:2] == (2.75, 0)
    rot = dict(TRI, face=np.array([[1, 2, 0], [0, 1, 2], [2, 0, 1]]))
    assert _both(host, NO_GEOMS, rot, TRI_VERTS, (0.1, -3, 0.2), (0, 1, 0))[:2] == (2.75, 0)
    # a sphere of radius 0.25 about 0 is met at t = 2.75 too: the geom (id 0) wins against the triangle (id 1 + 0) ...
    dist, gid, n = _both(host, SPHERE, TRI, TRI_VERTS, (0, -3, 0), (0, 1, 0))
    assert (dist, gid) == (2.75, 0) and n.tolist() == [0, -1, 0]
    # ... and loses once it is a hair smaller; without the element bit the triangle is no candidate, without the sphere's the sphere
    small = SPHERE[:3] + (np.array([[0.25 - 1e-9, 0.0, 0.0]]),) + SPHERE[4:]
    assert _both(host, small, TRI, TRI_VERTS, (0, -3, 0), (0, 1, 0))[:2] == (2.75, 1)
    assert _both(host, small, TRI, TRI_VERTS, (0, -3, 0), (0, 1, 0), cat_mask=RR.ALL_BITS & ~RR.ELEM_BIT)[1] == 0
    assert _both(host, SPHERE, TRI, TRI_VERTS, (0, -3, 0), (0, 1, 0), cat_mask=RR.ELEM_BIT)[:2] == (2.75, 1)
    # a geom on a body a vertex is bound to is hidden, whatever the mask says
    bound = SPHERE[:5] + (np.array([1]),)
    assert _both(host, bound, TRI, TRI_VERTS, (0, -3, 0), (0, 1, 0))[:2] == (2.75, 1)
    assert _both(host, bound, TRI, TRI_VERTS, (0, -3, 0), (0, 1, 0), cat_mask=RR.ALL_BITS & ~RR.ELEM_BIT)[1] == -1
    # the excluded body removes the triangle (a vertex bound to it) and, as before, the geoms on it
    assert _both(host, SPHERE, TRI, TRI_VERTS, (0, -3, 0), (0, 1, 0), exclude=[1])[:2] == (2.75, 0)
    assert _both(host, SPHERE, TRI, TRI_VERTS, (0, -3, 0), (0, 1, 0), exclude=[0])[:2] == (2.75, 1)
    mixed = dict(TRI, vert_body=np.array([1, 2, 1]))
    assert _both(host, NO_GEOMS, mixed, TRI_VERTS, (0, -3, 0), (0, 1, 0), exclude=[2])[1] == -1
    assert _both(host, NO_GEOMS, mixed, TRI_VERTS, (0, -3, 0), (0, 1, 0), exclude=[3])[1] == 0


def _ball():
    m = sg.load_model(model_path("softball"))
    return m, m.composite_skin()


@pytest.mark.parametrize("state", ["qpos0", "perturbed"])
def test_watertight_on_the_ball(host, state):
    """rays from outside aimed exactly at every vertex whose faces all face the ray, and at the midpoint (and three more points) of every
    edge between two such faces, on the 432-face ball: every one hits the skin, on a face that contains that vertex or edge, at the
    target's distance.  Each ray starts 5 cm above its target along the mean normal of the faces there, so that nothing of a dented
    surface lies in between"""
    m, skin = _ball()
    q = np.array(m.qpos0, dtype=np.float64) if state == "qpos0" else perturbed(m, 1)
    gx, gm, kin, verts, hv = _state(host, m, skin, q)
    ty, sz, cats, gb = _geoms(m)
    face = np.asarray(skin["face"])
    assert len(face) == 432
    a, b, c = (hv[face[:, k]] for k in range(3))
    fn = np.cross(b - a, c - a)
    fn /= np.linalg.norm(fn, axis=1, keepdims=True)
    targets, origins, want = [], [], []
    vfaces = [np.flatnonzero((face == v).any(1)) for v in range(len(hv))]
    for v in range(len(hv)):
        nrm = fn[vfaces[v]].sum(0)
        nrm /= np.linalg.norm(nrm)
        if (fn[vfaces[v]] @ nrm > 0.05).all():
            targets.append(hv[v]); origins.append(hv[v] + 0.05 * nrm); want.append(vfaces[v])
    nv = len(targets)
    edges = sorted({tuple(sorted((int(f[k]), int(f[(k + 1) % 3])))) for f in face for k in range(3)})
    for p, r in edges:
        fs = np.flatnonzero((face == p).any(1) & (face == r).any(1))
        assert len(fs) == 2
        nrm = fn[fs].sum(0)
        nrm /= np.linalg.norm(nrm)
        if (fn[fs] @ nrm > 0.05).all():
            for s in (0.5, 0.123, 0.9, 1e-4):
                t = (1 - s) * hv[p] + s * hv[r]
                targets.append(t); origins.append(t + 0.05 * nrm); want.append(fs if s > 1e-3 else np.union1d(vfaces[p], fs))
    targets, origins = np.array(targets), np.array(origins)
    assert nv >= 0.9 * len(hv) and len(targets) - nv >= 0.9 * 4 * len(edges), (nv, len(targets))
    for layout in (0, 1):
        dist, gid, n = RS.cast_with(host, gx, gm, ty, sz, cats, gb, skin, hv, origins, targets - origins, cat_mask=RR.ELEM_BIT, layout=layout)
        assert (gid >= len(ty)).all(), (state, np.flatnonzero(gid < len(ty))[:10].tolist())
        fhit = gid - len(ty)
        assert all(f in w for f, w in zip(fhit, want)), [i for i, (f, w) in enumerate(zip(fhit, want)) if f not in w][:10]
        assert np.abs(dist - 0.05).max() <= 1e-9
        assert np.abs(np.linalg.norm(n, axis=1) - 1).max() <= 1e-12 and (np.einsum("ri,ri->r", n, targets - origins) < 0).all()


def test_category_mask_and_exclusion_on_the_ball(host):
    m, skin = _ball()
    gx, gm, kin, verts, hv = _state(host, m, skin, perturbed(m, 2))
    ty, sz, cats, gb = _geoms(m)
    ng = len(ty)
    hidden = np.flatnonzero(RS.hidden_geoms(gb, skin))
    assert len(hidden) > 200 and (cats[hidden] == 3).all()
    o, d = RR.scene_rays(gx, ty, 256, 5)
    full = RS.cast_with(host, gx, gm, ty, sz, cats, gb, skin, hv, o, d)
    assert (full[1] >= ng).mean() > 0.25 and not np.isin(full[1], hidden).any()
    # without the element bit: no triangle and no hidden geom in any answer (the capsules do NOT come back)
    for mask in (RR.ALL_BITS & ~RR.ELEM_BIT, RR.CENTER_BIT, RR.GROUND_BIT | RR.FINGER_BIT):
        for layout in (0, 1):
            dist, gid, _ = RS.cast_with(host, gx, gm, ty, sz, cats, gb, skin, hv, o, d, cat_mask=mask, layout=layout)
            assert (gid < ng).all() and not np.isin(gid, hidden).any() and ((mask >> cats[gid[gid >= 0]]) & 1).all()
    assert (RS.cast_with(host, gx, gm, ty, sz, cats, gb, skin, hv, o, d, cat_mask=RR.CENTER_BIT)[1] >= 0).any()      # (the centre sphere shows through)
    # ray_exclude of an element body: no triangle bound to it in any answer; the rays that saw one before now see something else
    face, vb = np.asarray(skin["face"]), np.asarray(skin["vert_body"])
    seen = np.bincount(full[1][full[1] >= ng] - ng, minlength=len(face))
    body = int(vb[face[seen.argmax()][0]])
    gone = np.flatnonzero((vb[face] == body).any(1))
    ref = RS.cast(gx, gm, ty, sz, cats, gb, skin, verts, o, d, RR.ALL_BITS, np.full(len(o), body), 0.0)
    for layout in (0, 1):
        got = RS.cast_with(host, gx, gm, ty, sz, cats, gb, skin, hv, o, d, exclude=np.full(len(o), body), layout=layout)
        assert not np.isin(got[1] - ng, gone).any() and np.isin(full[1] - ng, gone).any()
        RR.compare(got, ref, RS.unstable(gx, gm, ty, sz, cats, gb, skin, verts, o, d, RR.ALL_BITS, np.full(len(o), body), 0.0, ref), "excluded element body")


def test_abi_flag_without_a_device():
    """SG_RAY_SKIN is a known flag bit: with a NULL batch the call now fails for the NULL batch; bits 2, 8 and up are still unknown"""
    from softgrip_amd import native
    with open(os.path.join(ROOT, "include", "softgrip.h")) as f:
        hdr = f.read()
    assert re.search(r"\bSG_RAY_SKIN = 4\b", hdr) and native.SG_RAY_SKIN == 4
    assert "geomid >= ngeom" in hdr and "NOT interpolated" in hdr
    L = native.lib()
    dummy = C.c_void_p(8)      # never dereferenced: the argument checks come first

    def call(flags):
        return L.sg_ray(None, None, 1, 1, dummy, dummy, None, None, 31, 0.0, flags, None, None, None, None)

    for flags in (native.SG_RAY_SKIN, native.SG_RAY_SKIN | native.SG_RAY_PER_ENV):
        assert call(flags) == native.SG_ERR_INVALID
        assert b"sg_ray" in L.sg_last_error() and b"null batch" in L.sg_last_error(), L.sg_last_error()
    for flags in (2, 3, 8, 8 | native.SG_RAY_SKIN, 16, -1):
        assert call(flags) == native.SG_ERR_INVALID
        assert b"unknown flag bits" in L.sg_last_error(), (flags, L.sg_last_error())


def test_kernels_in_the_kept_assembly():
    """the three kernels of sg_ray_skin_kernels.h are in sg_readout.device.s exactly once each, the assembly check is clean, none has
    scratch or spills, and the lane-per-ray kernel stays within the registers DESIGN.md 8.4 states, with 256 B of static LDS"""
    from softgrip_amd import build_native, isa_check, devasm
    build_native.build()
    api = build_native.device_asm("sg_readout.hip")
    assert not isa_check.check_asm(api)
    seen = devasm.kernels(open(api).read())
    kern = {}
    for key in ("sg_skinray_vert_kernel", "sg_skinray_rays_kernel", "sg_skinray_geoms_kernel"):
        found = [v for k, v in seen.items() if key in k]
        assert len(found) == 1, (key, sorted(seen))
        kern[key] = found[0]
        assert found[0]["scratch"] == 0 and found[0]["vgpr_spill"] == 0 and found[0]["sgpr_spill"] == 0, (key, found[0])
    print(kern)
    rays = kern["sg_skinray_rays_kernel"]
    assert rays["vgpr"] + rays["agpr"] <= REG_LIMIT_RAYS and rays["lds"] <= 256, rays
    assert kern["sg_skinray_geoms_kernel"]["vgpr"] + kern["sg_skinray_geoms_kernel"]["agpr"] <= 128 and kern["sg_skinray_geoms_kernel"]["lds"] == 0
    assert kern["sg_skinray_vert_kernel"]["lds"] == 0
    # the dynamic LDS of the lane-per-ray kernel at the model limits (320 visible geoms, 256 vertices, 512 faces): three workgroups per CU
    lds = 8 * (16 * 320 + 3 * 256) + 4 * 512 + 4 * 256 + 2 * 320
    assert lds == 50816 and lds + rays["lds"] <= 53 * 1024


def test_sanitizer_run_of_the_host_walk(tmp_path):
    """scripts/sanitize/ray_skin_main.cpp -- a stand-alone program: no skin, one face, a skin at the limits (256 vertices, 512 faces) --
    under AddressSanitizer and UBSan: clean, and the two reduction orders agree"""
    exe = str(tmp_path / "ray_skin_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                           os.path.join(ROOT, "soft-grip_amd", "csrc"), "-o", exe, os.path.join(ROOT, "scripts", "sanitize", "ray_skin_main.cpp")])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout.strip() == "ray_skin_main: 1800 rays, 530 hits, 499 on a skin, checksum 08cf6f9906f7ed90" and not res.stderr.strip(), res.stdout + res.stderr


def test_tactile_depth_with_the_skin(host, monkeypatch):
    """ManEnv.tactile_depth(skin=True) over a batch whose raycast is the host build on a perturbed state: the rays, exclusion, max_dist
    and gap formula are tactile_depth's own; gap, geom and face equal the reference on the same rays, and skin=False asks for the
    plain call and carries no face"""
    import torch
    from fake_native import FakeBatch, FakeModel
    from softgrip_amd import manenv, native
    m = sg.load_model(model_path("softball"))
    skin = m.composite_skin()
    q = perturbed(m, 3)
    gx, gm, kin, verts, hv = _state(host, m, skin, q)
    ty, sz, cats, gb = _geoms(m)
    ng = len(ty)
    calls = []

    class RayBatch(FakeBatch):
        def raycast(self, origin, direction, body=None, exclude=None, env_ids=None, cat_mask=native.SG_RAY_ALL, max_dist=0.0, normals=False, skin=False):
            calls.append(dict(skin=skin, cat_mask=cat_mask, max_dist=max_dist, body=np.array(body), exclude=np.array(exclude)))
            o, d = origin.numpy(), direction.numpy()
            none = dict(vert_body=np.zeros(0, int), vert_pos=np.zeros((0, 3)), face=np.zeros((0, 3), int))      # (the plain call: no skin)
            dist, gid, _ = RS.cast_with(host, gx, gm, ty, sz, cats, gb, self.nmodel.model.composite_skin() if skin else none, hv if skin else np.zeros((0, 3)),
                                        o, d, kin["xpos"], kin["xquat"], body, exclude, cat_mask, max_dist)
            k = self.n if env_ids is None else len(env_ids)
            out = dict(dist=torch.from_numpy(np.tile(dist, (k, 1))), geom=torch.from_numpy(np.tile(gid, (k, 1))))
            if skin:
                out["face"] = torch.from_numpy(np.tile(RS.faces_of(gid, ng), (k, 1)))
            return out

    monkeypatch.setattr(native, "NativeModel", FakeModel)
    monkeypatch.setattr(native, "NativeBatch", RayBatch)
    env = manenv.ManEnv(1, 7, [model_path("softball")], is_vis=False, n_envs=2)
    res, max_gap = (5, 4), 0.05
    tr = manenv.tactile_rays(env.model, res)
    o, d, body = tr["origin"].reshape(-1, 3), tr["direction"].reshape(-1, 3), tr["body"].reshape(-1)
    B = len(tr["geoms"])
    thick = np.repeat(tr["thickness"], res[0] * res[1])
    lim = float(tr["thickness"].max()) + max_gap
    out = env.tactile_depth(res=res, max_gap=max_gap, skin=True)
    assert set(out) == {"gap", "geom", "face"} and out["gap"].shape == (2, B, res[1], res[0]) and out["face"].dtype == torch.int32
    c = calls[-1]
    assert c["skin"] is True and c["cat_mask"] == RR.ELEM_BIT | RR.CENTER_BIT and c["max_dist"] == lim
    assert c["body"].tolist() == body.tolist() and c["exclude"].tolist() == body.tolist()
    ow, dw = RR.map_rays(kin["xpos"], kin["xquat"], o, d, body)
    ref = RS.cast(gx, gm, ty, sz, cats, gb, skin, verts, ow, dw, RR.ELEM_BIT | RR.CENTER_BIT, body, lim)
    edge = RS.unstable(gx, gm, ty, sz, cats, gb, skin, verts, ow, dw, RR.ELEM_BIT | RR.CENTER_BIT, body, lim, ref)
    rgap = ref[0] - thick
    seen = (ref[1] >= 0) & (rgap <= max_gap)
    want_gap, want_geom = np.where(seen, rgap, np.inf), np.where(seen, ref[1], -1)
    want_face = RS.faces_of(want_geom, ng)
    for e in range(2):
        gap, geom, fc = (out[k][e].numpy().reshape(-1) for k in ("gap", "geom", "face"))
        with np.errstate(invalid="ignore"):
            wrong = (geom != want_geom) | (fc != want_face) | ~((gap == want_gap) | (np.abs(gap - want_gap) <= 1e-9))
        assert not (wrong & ~edge).any(), (e, np.flatnonzero(wrong & ~edge)[:5])
        assert (wrong & edge).sum() <= 0.02 * len(o)
    plain = env.tactile_depth(res=res, max_gap=max_gap)
    assert set(plain) == {"gap", "geom"} and calls[-1]["skin"] is False
    assert env.raycast(torch.from_numpy(o), torch.from_numpy(d), body=body, exclude=body, skin=True)["face"].shape == (2, len(o))
