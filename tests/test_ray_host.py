"""Ray queries (sg_ray) without a GPU: the g++ build of csrc/sg_ray.h -- the per-ray math both kernel layouts run -- against the
independent NumPy caster (tests/ray_ref.py) on the committed scenes and over a pose sweep of random grippers, analytic known answers
per primitive, the tie rule, the ABI entry point's checks that need no device, the kept assembly of the two kernels and the ray
construction of ManEnv.tactile_depth."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ray_ref as RR
from helpers import ROOT, model_path
from test_render_host import perturbed

import softgrip_amd as sg

SCENES = ["softbox", "softball", "fourfinger_softball", "freeball"]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return RR.build_host(str(tmp_path_factory.mktemp("ray_host")))


def _scene(m, q):
    gx, gm = RR.geom_poses(m, q)
    return gx, gm, np.asarray(m.geom_type), np.asarray(m.geom_size, dtype=np.float64), RR.categories(m), np.asarray(m.geom_bodyid)


@pytest.mark.parametrize("scene", SCENES)
def test_host_build_matches_numpy_caster(host, scene):
    """256 rays of the test recipe per state, world frame; then the same rays bound to a moving body with that body excluded.  Ids
    exact, distances and normals within 1e-9 (both sides fp64), both reduction orders bit-identical"""
    m = sg.load_model(model_path(scene))
    left = total = hits = 0
    for k, q in enumerate([np.array(m.qpos0, dtype=np.float64)] + [perturbed(m, s) for s in range(3)]):
        gx, gm, ty, sz, cats, gb = _scene(m, q)
        o, d = RR.scene_rays(gx, ty, 256, 100 + k)
        ref = RR.cast(gx, gm, ty, sz, o, d)
        got = RR.cast_with(host, gx, gm, ty, sz, cats, gb, o, d)
        alt = RR.cast_with(host, gx, gm, ty, sz, cats, gb, o, d, layout=1)
        for x, y in zip(got, alt):
            assert x.tobytes() == y.tobytes(), (scene, k)
        edge = RR.unstable(gx, gm, ty, sz, o, d, None, 0.0, ref)
        left += RR.compare(got, ref, edge, "%s state %d" % (scene, k))
        total += len(o)
        hits += int((ref[1] >= 0).sum())
        # body-frame rays with exclusion, a category mask and a distance limit
        kin = m.kinematics(q)
        body = int(np.flatnonzero(np.asarray(m.body_weldid) != 0)[k % 5])
        R = kin["xmat"][body]
        ol, dl = (o - kin["xpos"][body]) @ R, d @ R                     # the same world rays, written in the body's frame
        rb = np.full(len(o), body, np.int32)
        mask = RR.ALL_BITS & ~RR.GROUND_BIT
        keep = RR.candidates(cats, gb, mask, rb, len(o))
        ow, dw = RR.map_rays(kin["xpos"], kin["xquat"], ol, dl, rb)
        ref2 = RR.cast(gx, gm, ty, sz, ow, dw, keep, 2.0)
        for layout in (0, 1):
            got2 = RR.cast_with(host, gx, gm, ty, sz, cats, gb, ol, dl, kin["xpos"], kin["xquat"], rb, rb, mask, 2.0, layout)
            edge2 = RR.unstable(gx, gm, ty, sz, ow, dw, keep, 2.0, ref2)
            RR.compare(got2, ref2, edge2, "%s state %d body %d layout %d" % (scene, k, body, layout))
        assert not np.isin(ref2[1], np.flatnonzero((gb == body) | (cats == 0))).any()
    print("%s: %d rays, %d hits, %d left out" % (scene, total, hits, left))
    assert hits > 0.5 * total


def test_sweep_of_random_grippers_matches_numpy_caster(host, tmp_path):
    """the ray sweep of ray_ref: six random grippers, 16 of each one's swept poses (links turned up to 3 rad about up to three axes,
    every second gripper's shell on a free joint at a random attitude), 256 rays of the recipe per pose.  Ids exact, distances and
    normals within 1e-9, both reduction orders bit-identical.  Left out, at most 2 % of a gripper's rays: rays on which the
    reference's own answer changes under a 1e-7 m shift of the origin, and coplanar ties -- the returned geom is another one, the
    reference's own distance to it is within 1e-12 of its best (the two boxes of a link have coplanar faces), distance and normal
    still agree.  Also the same sweep with rays in a random link's frame, that link excluded: origins inside the scene.
    Measured: 24 576 world rays, 23 810 hits (planes 7 914, boxes 14 854, capsules 1 039, the centre sphere 3), 82 rays unstable by
    the reference alone (0.33 %), 5 left out; 24 576 link rays, 16 662 hits (planes 9 120, boxes 6 632, capsules 899), 16 left out; of
    the 21 rays left out 8 are coplanar ties off the knife edges: without the rule the comparison fails"""
    import contacts_ref as CR
    kinds, total, edges, left_all, ties = {}, 0, 0, 0, 0
    lkinds, lleft = {}, 0
    for g in range(CR.SWEEP_GRIPPERS):
        m, qs = RR.sweep_poses(g, tmp_path)
        left = lcount = 0
        for p, q in enumerate(qs):
            gx, gm, ty, sz, cats, gb = _scene(m, q)
            o, d = RR.scene_rays(gx, ty, RR.SWEEP_RAYS, RR.SWEEP_RAY_SEED + 100 * g + p)
            ref = RR.cast(gx, gm, ty, sz, o, d, per_geom=True)
            got = RR.cast_with(host, gx, gm, ty, sz, cats, gb, o, d)
            alt = RR.cast_with(host, gx, gm, ty, sz, cats, gb, o, d, layout=1)
            for x, y in zip(got, alt):
                assert x.tobytes() == y.tobytes(), (g, p)
            edge = RR.unstable(gx, gm, ty, sz, o, d, None, 0.0, ref)
            left += RR.compare(got, ref, edge, "gripper %d pose %d" % (g, p), cap=1.0, per_geom=ref[3])
            ties += int((RR.coplanar_ties(got, ref, ref[3]) & ~edge).sum())
            edges += int(edge.sum())
            total += len(o)
            RR.count_types(ty, ref[1], kinds)
            # rays bound to a link, which they do not see
            kin = m.kinematics(q)
            ol, dl, rb = RR.link_rays(m, RR.SWEEP_RAYS, RR.SWEEP_RAY_SEED + 100 * g + p)
            keep = RR.candidates(cats, gb, RR.ALL_BITS, rb, len(ol))
            ow, dw = RR.map_rays(kin["xpos"], kin["xquat"], ol, dl, rb)
            ref2 = RR.cast(gx, gm, ty, sz, ow, dw, keep, per_geom=True)
            edge2 = RR.unstable(gx, gm, ty, sz, ow, dw, keep, 0.0, ref2)
            for lay in (0, 1):
                got2 = RR.cast_with(host, gx, gm, ty, sz, cats, gb, ol, dl, kin["xpos"], kin["xquat"], rb, rb, RR.ALL_BITS, 0.0, lay)
                n2 = RR.compare(got2, ref2, edge2, "gripper %d pose %d link %d layout %d" % (g, p, rb[0], lay), cap=1.0, per_geom=ref2[3])
            ties += int((RR.coplanar_ties(got2, ref2, ref2[3]) & ~edge2).sum())
            lcount += n2
            assert not (gb[ref2[1][ref2[1] >= 0]] == rb[0]).any()
            RR.count_types(ty, ref2[1], lkinds)
        print("gripper %d: %d rays, left out %d; link rays: left out %d" % (g, len(qs) * RR.SWEEP_RAYS, left, lcount))
        assert len(qs) == 16
        assert left <= 0.02 * len(qs) * RR.SWEEP_RAYS and lcount <= 0.02 * len(qs) * RR.SWEEP_RAYS, (g, left, lcount)
        left_all += left
        lleft += lcount
    print("%d rays, hits by geom type %s, %d knife-edge rays by the reference alone, %d left out; link rays: hits %s, %d left out; coplanar ties off the knife edges, both kinds: %d"
          % (total, kinds, edges, left_all, lkinds, lleft, ties))
    assert total == CR.SWEEP_GRIPPERS * 16 * RR.SWEEP_RAYS
    for t in (RR.PLANE, RR.BOX, RR.CAPSULE):
        assert kinds.get(t, 0) > 0, kinds
    assert lkinds.get(RR.BOX, 0) > 0 and lkinds.get(RR.CAPSULE, 0) > 0, lkinds


def _single(type_, size, pos=(0.0, 0.0, 0.0), mat=None):
    return (np.array([pos], dtype=np.float64), (np.eye(3) if mat is None else mat)[None], np.array([type_]), np.array([size], dtype=np.float64),
            np.array([1]), np.array([0]))


def _both(host, geom, o, d, **kw):
    """the host build (both reduction orders) and the reference on one ray -> (dist, geom id, normal) of the host, checked equal"""
    gx, gm, ty, sz, cats, gb = geom
    ref = RR.cast(gx, gm, ty, sz, [o], [d], None, kw.get("max_dist", 0.0))
    out = None
    for layout in (0, 1):
        got = RR.cast_with(host, gx, gm, ty, sz, cats, gb, [o], [d], layout=layout, **kw)
        assert got[1][0] == ref[1][0] and abs(got[0][0] - ref[0][0]) <= 1e-12 and np.abs(got[2][0] - ref[2][0]).max() <= 1e-12, (got, ref)
        out = got
    return out[0][0], out[1][0], out[2][0]


KNOWN = {   # type, size, (origin, direction, distance, normal) head-on, an origin inside
    "sphere": (RR.SPHERE, (0.25, 0, 0), ((0, -3, 0), (0, 2, 0), 2.75, (0, -1, 0)), (0.1, 0, 0)),
    "capsule": (RR.CAPSULE, (0.1, 0.3, 0), ((0, -3, 0.2), (0, 1, 0), 2.9, (0, -1, 0)), (0, 0, 0)),
    "box": (RR.BOX, (0.2, 0.15, 0.1), ((0.05, -3, 0.02), (0, 1, 0), 2.85, (0, -1, 0)), (0.1, 0.1, 0.05)),
    "plane": (RR.PLANE, (0, 0, 1), ((0.3, 0.4, 2), (0, 0, -1), 2.0, (0, 0, 1)), (0, 0, -0.5)),
}


@pytest.mark.parametrize("case", sorted(KNOWN))
def test_known_answers(host, case):
    type_, size, (o, d, want, normal), inside = KNOWN[case]
    geom = _single(type_, size)
    dist, gid, n = _both(host, geom, o, d)
    assert gid == 0 and abs(dist - want) < 1e-12 and np.abs(n - normal).max() < 1e-12, (dist, gid, n)
    # an origin inside the primitive (the plane: below it) sees nothing of it, in whatever direction
    for dd in ((0, 1, 0), (0, 0, 1), (0, 0, -1), (1, 0, 0), (0.3, -0.2, 0.9)):
        dist, gid, n = _both(host, geom, inside, dd)
        assert (dist, gid) == (-1.0, -1) and not n.any(), (case, dd, dist, gid)
    # max_dist just short of the hit and just past it
    unit = np.asarray(d, dtype=np.float64) / np.linalg.norm(d)
    assert _both(host, geom, o, unit, max_dist=want - 1e-9)[1] == -1
    dist, gid, _ = _both(host, geom, o, unit, max_dist=want + 1e-9)
    assert gid == 0 and abs(dist - want) < 1e-12
    # a direction without length, or not finite: a miss
    for dd in ((0, 0, 0), (np.nan, 1, 0), (np.inf, 0, 0)):
        got = RR.cast_with(host, *geom, [o], [dd])
        assert got[0][0] == -1.0 and got[1][0] == -1 and not got[2].any()


def test_known_answers_of_the_details(host):
    # the plane from below, and seen edge-on
    plane = _single(RR.PLANE, (0, 0, 1))
    assert _both(host, plane, (0, 0, -1), (0, 0, 1))[1] == -1
    assert _both(host, plane, (0, 0, 1), (1, 0, 0))[1] == -1
    # a bounded plane ends at its size
    small = _single(RR.PLANE, (0.5, 0.5, 1))
    assert _both(host, small, (0.4, 0, 1), (0, 0, -1))[1] == 0 and _both(host, small, (0.6, 0, 1), (0, 0, -1))[1] == -1
    # a ray parallel to a box slab: inside the slab it hits the face it runs into, outside it misses
    box = _single(RR.BOX, (0.2, 0.15, 0.1))
    dist, gid, n = _both(host, box, (0.1, -3, 0.05), (0, 1, 0))
    assert gid == 0 and abs(dist - 2.85) < 1e-12 and n.tolist() == [0, -1, 0]
    assert _both(host, box, (0.1, -3, 0.1000001), (0, 1, 0))[1] == -1
    assert _both(host, box, (0.2000001, -3, 0.0), (0, 1, 0))[1] == -1
    # a capsule's cap from above, its side, and from inside the cylinder along the axis (no surface on the cap's inner half)
    cap = _single(RR.CAPSULE, (0.1, 0.3, 0))
    dist, gid, n = _both(host, cap, (0, 0, 2), (0, 0, -1))
    assert gid == 0 and abs(dist - 1.6) < 1e-12 and np.abs(n - (0, 0, 1)).max() < 1e-12
    for z in (0.0, 0.15, -0.25, 0.35):
        for dd in ((0, 0, 1), (0, 0, -1), (0.6, 0, 0.8)):
            assert _both(host, cap, (0.02, 0.01, z), dd)[1] == -1, (z, dd)
    # a turned and shifted box: distance along a diagonal, world normal
    c, s = np.cos(0.5), np.sin(0.5)
    Rz = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])
    tb = _single(RR.BOX, (0.2, 0.15, 0.1), (1.0, 2.0, 0.5), Rz)
    dist, gid, n = _both(host, tb, np.array([1.0, 2.0, 0.5]) + Rz @ np.array([-3.0, 0.05, 0.0]), Rz @ np.array([1.0, 0, 0]))
    assert gid == 0 and abs(dist - 2.8) < 1e-12 and np.abs(n - Rz @ np.array([-1.0, 0, 0])).max() < 1e-12


def test_tie_rule_smaller_geom_id_wins(host):
    m = sg.compile_mjcf(os.path.join(ROOT, "tests", "data", "ray", "ray_ties.xml"), composite_neighbors=False)
    gx, gm, ty, sz, cats, gb = _scene(m, m.qpos0)
    names = list(m.geom_names)
    a, b, fl = names.index("twin_a"), names.index("twin_b"), names.index("flush")
    assert a < b < fl
    xs, ys = np.meshgrid(np.linspace(-0.2, 0.2, 5), np.linspace(-0.4, 0.4, 9))
    o = np.stack([xs.ravel(), ys.ravel(), np.full(xs.size, 2.0)], -1)
    d = np.tile([0.0, 0.0, -1.0], (len(o), 1))
    for layout in (0, 1):
        dist, gid, n = RR.cast_with(host, gx, gm, ty, sz, cats, gb, o, d, layout=layout)
        assert (gid == a).all() and (dist == 1.375).all() and (n == [0, 0, 1]).all(), (layout, gid, dist)
    # the same geoms in reversed order: what is then the smallest id at that distance
    rev = slice(None, None, -1)
    dist, gid, _ = RR.cast_with(host, gx[rev], gm[rev], ty[rev], sz[rev], cats[rev], gb[rev], o, d)
    ng = len(ty)
    assert (dist == 1.375).all() and set(gid.tolist()) == {ng - 1 - fl, ng - 1 - b}
    assert (RR.cast(gx, gm, ty, sz, o, d)[1] == a).all()


def test_abi_entry_point_without_a_device():
    from softgrip_amd import native
    with open(os.path.join(ROOT, "include", "softgrip.h")) as f:
        hdr = f.read()
    assert "sg_ray" in set(re.findall(r"(sg_[a-z_]+)\s*\(", hdr)) and "sg_ray" in native.SYMBOLS
    assert "mj_ray, which reports the exit" in " ".join(hdr.split())      # (the departure from mj_ray is stated)
    for name, val in (("SG_RAY_GROUND", 1), ("SG_RAY_STATIC", 2), ("SG_RAY_FINGER", 4), ("SG_RAY_ELEM", 8), ("SG_RAY_CENTER", 16), ("SG_RAY_ALL", 31),
                      ("SG_RAY_PER_ENV", 1)):
        assert re.search(r"\b%s = %d\b" % (name, val), hdr) and getattr(native, name) == val
    L = native.lib()
    assert hasattr(L, "sg_ray")
    dummy = C.c_void_p(8)      # never dereferenced: the argument checks come first

    def call(b=None, n_ids=1, n_rays=1, origin=dummy, dir_=dummy, cat_mask=31, max_dist=0.0, flags=0):
        return L.sg_ray(b, None, n_ids, n_rays, origin, dir_, None, None, cat_mask, max_dist, flags, None, None, None, None)

    for kw, word in ((dict(), b"null batch"), (dict(n_ids=0), b"n_ids"), (dict(n_rays=0), b"n_rays"), (dict(n_rays=-2), b"n_rays"),
                     (dict(cat_mask=0), b"cat_mask"), (dict(cat_mask=32), b"cat_mask"), (dict(flags=2), b"flag"),
                     (dict(max_dist=float("nan")), b"max_dist"), (dict(max_dist=float("inf")), b"max_dist")):
        assert call(**kw) == native.SG_ERR_INVALID, kw
        assert b"sg_ray" in L.sg_last_error() and word in L.sg_last_error(), (kw, L.sg_last_error())
    # (NULL origin / dir, env and body ids out of range need a batch: tests/test_gpu_ray.py)


def test_kernels_in_the_kept_assembly():
    """sg_ray_kernels.h is compiled inside sg_readout.hip: both kernels are in sg_readout.device.s, the assembly check is clean, and they hold what
    DESIGN.md 8.3 states: no scratch, no spills, the lane-per-ray kernel at most 64 registers (eight waves per SIMD) with 256 B of
    static LDS beside the staged records, the lanes-over-geoms kernel at most 128 registers and no LDS"""
    from softgrip_amd import build_native, isa_check, devasm
    build_native.build()
    api = build_native.device_asm("sg_readout.hip")
    assert not isa_check.check_asm(api)
    seen = devasm.kernels(open(api).read())
    rays = [v for k, v in seen.items() if "sg_ray_rays_kernel" in k]
    geoms = [v for k, v in seen.items() if "sg_ray_geoms_kernel" in k]
    assert len(rays) == 1 and len(geoms) == 1, sorted(seen)
    print(rays[0], geoms[0])
    for v in rays + geoms:
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0, v
    assert rays[0]["vgpr"] + rays[0]["agpr"] <= 64 and rays[0]["lds"] <= 256, rays[0]
    assert geoms[0]["vgpr"] + geoms[0]["agpr"] <= 128 and geoms[0]["lds"] == 0, geoms[0]


def _formula_rays(m, res, faces):
    """the issue's formula, evaluated cell by cell with plain loops"""
    from softgrip_amd.mjcf import quat_to_mat
    W, H = res
    boxes = [g for g in range(m.ngeom) if m.geom_type[g] == 6 and m.body_weldid[m.geom_bodyid[g]] != 0]
    out = []
    for g, (a, sig) in zip(boxes, faces):
        s = m.geom_size[g]
        R = quat_to_mat(m.geom_quat[g])
        u, v = (a + 1) % 3, (a + 2) % 3
        for j in range(H):
            for i in range(W):
                p, e = np.zeros(3), np.zeros(3)
                p[u] = s[u] * (2 * (i + .5) / W - 1)
                p[v] = s[v] * (2 * (j + .5) / H - 1)
                p[a] = -sig * s[a]
                e[a] = sig
                out.append((m.geom_pos[g] + R @ p, R @ e, m.geom_bodyid[g], 2 * s[a]))
    return boxes, out


@pytest.mark.parametrize("scene", ["softbox", "fourfinger_softball"])
def test_tactile_ray_construction(scene, host):
    from softgrip_amd.manenv import tactile_rays
    m = sg.load_model(model_path(scene))
    res = (5, 3)
    rays = tactile_rays(m, res)
    boxes = [g for g in range(m.ngeom) if m.geom_type[g] == 6 and m.body_weldid[m.geom_bodyid[g]] != 0]
    B = len(boxes)
    assert rays["origin"].shape == (B, 3, 5, 3) and rays["body"].shape == (B, 3, 5) and rays["geoms"].tolist() == boxes
    # the default faces, independently: of the six outward normals at qpos0 the one that points most at the centre sphere
    gx, gm = RR.geom_poses(m, m.qpos0)
    centre = gx[list(m.geom_type).index(2)]
    for k, g in enumerate(boxes):
        best = max(((sig * gm[g][:, a]) @ (centre - gx[g]), a, sig) for a in range(3) for sig in (1, -1))
        second = sorted(((sig * gm[g][:, a]) @ (centre - gx[g])) for a in range(3) for sig in (1, -1))[-2]
        if best[0] - second > 1e-9:
            assert tuple(rays["faces"][k]) == best[1:], (k, rays["faces"][k], best)
    _, want = _formula_rays(m, res, [tuple(f) for f in rays["faces"]])
    o, d, b = rays["origin"].reshape(-1, 3), rays["direction"].reshape(-1, 3), rays["body"].reshape(-1)
    th = np.repeat(rays["thickness"], 15)
    assert len(want) == len(o)
    for r, (wo, wd, wb, wt) in enumerate(want):
        assert np.abs(o[r] - wo).max() < 1e-15 and np.abs(d[r] - wd).max() < 1e-15 and b[r] == wb and th[r] == wt, r
    # cast at qpos0 through the host build, as tactile_depth casts them: the host build agrees with the reference on what the pads see
    kin = m.kinematics(np.array(m.qpos0, dtype=np.float64))
    ty, sz, cats, gb = np.asarray(m.geom_type), np.asarray(m.geom_size, dtype=np.float64), RR.categories(m), np.asarray(m.geom_bodyid)
    dist, gid, _ = RR.cast_with(host, gx, gm, ty, sz, cats, gb, o, d, kin["xpos"], kin["xquat"], b, b, RR.ELEM_BIT | RR.CENTER_BIT, 0.0)
    ow, dw = RR.map_rays(kin["xpos"], kin["xquat"], o, d, b)
    ref = RR.cast(gx, gm, ty, sz, ow, dw, RR.candidates(cats, gb, RR.ELEM_BIT | RR.CENTER_BIT, b, len(o)), 0.0)
    RR.compare((dist, gid, None), ref, np.zeros(len(o), bool), scene)
    assert (gid >= 0).any() and np.isin(cats[gid[gid >= 0]], (3, 4)).all()
    # explicit faces override; a wrong count or a model without a centre sphere and no faces: ValueError
    over = tactile_rays(m, res, faces=[(0, -1)] * B)
    assert (over["faces"] == [0, -1]).all() and np.allclose(over["thickness"], 2 * sz[boxes][:, 0])
    with pytest.raises(ValueError):
        tactile_rays(m, res, faces=[(0, 1)])
    nosphere = sg.compile_mjcf(os.path.join(ROOT, "tests", "data", "mini_gripper.xml"), composite_neighbors=False)
    if 2 not in list(nosphere.geom_type):
        with pytest.raises(ValueError):
            tactile_rays(nosphere, res)
