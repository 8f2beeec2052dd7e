"""sg_ray on the GPU: world-frame rays against the NumPy reference (tests/ray_ref.py) on the device's own poses, under both kernel
layouts, on the committed scenes and over a pose sweep of random grippers; body-frame rays and exclusion; the call's interface (shapes around the block and wavefront sizes, per-env rays, env subsets, NULL
outputs, a zero direction, NaN envs, category masks, every argument error); bit-identical layouts; no side effect on a following step;
the renderer's picture through sg_ray; and ManEnv.tactile_depth."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

import ray_ref as RR
import render_ref as R
from helpers import JOINT_IDS, model_path

import softgrip_amd as sg
from softgrip_amd.create_dataset import episode_schedule

pytestmark = pytest.mark.gpu

LAYOUTS = ("rays", "geoms")
SCENES = {"softbox": ("explicit", JOINT_IDS, 2), "fourfinger_softball_fix": ("implicit", list(range(65, 283)), 4)}


@contextlib.contextmanager
def layout(name):
    """SG_RAY_LAYOUT for the calls inside (the library reads it per call); None: the automatic choice"""
    old = os.environ.pop("SG_RAY_LAYOUT", None)
    if name:
        os.environ["SG_RAY_LAYOUT"] = name
    try:
        yield
    finally:
        os.environ.pop("SG_RAY_LAYOUT", None)
        if old is not None:
            os.environ["SG_RAY_LAYOUT"] = old


def _batch(scene, n, pipeline=None, seed=11):
    import torch
    from softgrip_amd import native
    damper, jids, nu = SCENES[scene]
    m = sg.load_model(model_path(scene), damper)
    nm = native.NativeModel(m)
    b = native.NativeBatch(nm, n, 0)
    if pipeline:
        b.set_pipeline(pipeline)
    b.set_stiffness(np.random.RandomState(seed).uniform(300, 1400, n), jids, [0])
    b.reset(1)
    return m, nm, b, torch


def _run(b, nu, t0, t1):
    sched = episode_schedule()
    for t in range(t0, t1):
        if sched[t] is not None:
            b.set_ctrl_broadcast(np.full(nu, sched[t]))
        b.step(7)


def _geoms(m):
    return np.asarray(m.geom_type), np.asarray(m.geom_size, dtype=np.float64), RR.categories(m), np.asarray(m.geom_bodyid)


def _host(out):
    return out["dist"].cpu().numpy(), out["geom"].cpu().numpy(), out["normal"].cpu().numpy() if "normal" in out else None


def _poses(b, ids=None):
    p = b.poses(ids)
    return {k: v.cpu().numpy() for k, v in p.items()}


@pytest.mark.parametrize("scene,nenv,nrays", [("softbox", 3, 512), ("fourfinger_softball_fix", 2, 256)])
def test_world_rays_match_reference(scene, nenv, nrays):
    """rays of the recipe (ray_ref.scene_rays), different ones per env, at the reset state and at env steps 60 and 100 of the reference
    schedule: geom ids exact, distances and normals within 1e-9 of the reference on the device's poses, under both layouts, which also
    agree bit for bit.  Left out: only rays on which the reference's own answer changes under a 1e-7 m shift of the origin, at most 2 %"""
    m, nm, b, torch = _batch(scene, nenv)
    ty, sz, cats, gb = _geoms(m)
    nu = SCENES[scene][2]
    t_at, total, left, hits, seen = 0, 0, 0, 0, set()
    for t in (0, 60, 100):
        _run(b, nu, t_at, t)
        t_at = t
        p = _poses(b)
        rays = [RR.scene_rays(p["geom_xpos"][e], ty, nrays, 1000 * t + e) for e in range(nenv)]
        o = torch.tensor(np.stack([r[0] for r in rays]), device=b.device)
        d = torch.tensor(np.stack([r[1] for r in rays]), device=b.device)
        got = {}
        for lay in LAYOUTS:
            with layout(lay):
                got[lay] = _host(b.raycast(o, d, normals=True))
        for x, y in zip(got["rays"], got["geoms"]):
            assert x.tobytes() == y.tobytes(), (scene, t)
        for e in range(nenv):
            gx, gm = p["geom_xpos"][e], p["geom_xmat"][e].reshape(-1, 3, 3)
            ref = RR.cast(gx, gm, ty, sz, *rays[e])
            edge = RR.unstable(gx, gm, ty, sz, rays[e][0], rays[e][1], None, 0.0, ref)
            left += RR.compare(tuple(x[e] for x in got["rays"]), ref, edge, "%s step %d env %d" % (scene, t, e))
            total += nrays
            hits += int((ref[1] >= 0).sum())
            seen |= set(ref[1][ref[1] >= 0].tolist())
    print("%s: %d rays, %d hits on %d distinct geoms, %d left out" % (scene, total, hits, len(seen), left))
    assert hits > 0.8 * total and len(seen) >= 30
    assert left <= 0.02 * total


@pytest.mark.parametrize("gripper", range(6))
def test_sweep_of_random_grippers_matches_reference(gripper, tmp_path):
    """the ray sweep of ray_ref on the device: 16 swept poses of a random gripper (links turned up to 3 rad about up to three axes,
    every second gripper's shell on a free joint at a random attitude) as 16 envs of one batch, one sg_set_state, nothing stepped; 256
    rays of the recipe per env, rays of its own for each.  Both layouts, which agree bit for bit, against the reference on the
    device's own poses: ids exact, distances and normals within 1e-9.  Then one call of 256 rays in the frame of a random link, that
    link excluded: origins inside the scene, among the fingers.  Left out, at most 2 % of the gripper's rays of either kind: rays on
    which the reference's own answer changes under a 1e-7 m shift of the origin, and coplanar ties (ray_ref.coplanar_ties: another
    geom, to which the reference's own distance is within 1e-12 of its best; distance and normal still within 1e-9).  That the sweep
    hits planes, boxes and capsules is asserted on the CPU by tests/test_ray_host.py's test of the same sweep.
    Measured on the MI355X over the six grippers: 24 576 world rays, 23 810 hits (planes 7 914, boxes 14 854, capsules
    1 039, the centre sphere 3), 3 left out; 24 576 link rays, 16 127 hits (planes 8 736, boxes 6 745, capsules 642, sphere 4), 9 left
    out, one of the 12 a coplanar tie off the knife edges (gripper 5)"""
    import torch
    from softgrip_amd import native
    m, qs = RR.sweep_poses(gripper, tmp_path)
    ty, sz, cats, gb = _geoms(m)
    nenv, nrays = len(qs), RR.SWEEP_RAYS
    assert nenv == 16
    b = native.NativeBatch(native.NativeModel(m), nenv, 0)
    b.set_state(qpos=torch.tensor(np.ascontiguousarray(qs), dtype=torch.float64, device=b.device))
    p = _poses(b)
    rays = [RR.scene_rays(p["geom_xpos"][e], ty, nrays, RR.SWEEP_RAY_SEED + 100 * gripper + e) for e in range(nenv)]
    o = torch.tensor(np.stack([r[0] for r in rays]), device=b.device)
    d = torch.tensor(np.stack([r[1] for r in rays]), device=b.device)
    got = {}
    for lay in LAYOUTS:
        with layout(lay):
            got[lay] = _host(b.raycast(o, d, normals=True))
    for x, y in zip(got["rays"], got["geoms"]):
        assert x.tobytes() == y.tobytes(), gripper
    ol, dl, rb = RR.link_rays(m, nrays, RR.SWEEP_RAY_SEED + gripper)
    link = _host(b.raycast(torch.tensor(ol, device=b.device), torch.tensor(dl, device=b.device), body=rb, exclude=rb, normals=True))
    keep = RR.candidates(cats, gb, RR.ALL_BITS, rb, nrays)
    left = lleft = ties = 0
    kinds, lkinds = {}, {}
    for e in range(nenv):
        gx, gm = p["geom_xpos"][e], p["geom_xmat"][e].reshape(-1, 3, 3)
        ref = RR.cast(gx, gm, ty, sz, *rays[e], per_geom=True)
        edge = RR.unstable(gx, gm, ty, sz, rays[e][0], rays[e][1], None, 0.0, ref)
        mine = tuple(x[e] for x in got["rays"])
        left += RR.compare(mine, ref, edge, "gripper %d env %d" % (gripper, e), cap=1.0, per_geom=ref[3])
        ties += int((RR.coplanar_ties(mine, ref, ref[3]) & ~edge).sum())
        RR.count_types(ty, ref[1], kinds)
        ow, dw = RR.map_rays(p["xpos"][e], p["xquat"][e], ol, dl, rb)
        ref = RR.cast(gx, gm, ty, sz, ow, dw, keep, per_geom=True)
        edge = RR.unstable(gx, gm, ty, sz, ow, dw, keep, 0.0, ref)
        mine = tuple(x[e] for x in link)
        lleft += RR.compare(mine, ref, edge, "gripper %d env %d link %d" % (gripper, e, rb[0]), cap=1.0, per_geom=ref[3])
        ties += int((RR.coplanar_ties(mine, ref, ref[3]) & ~edge).sum())
        assert not (gb[ref[1][ref[1] >= 0]] == rb[0]).any()
        RR.count_types(ty, ref[1], lkinds)
    print("gripper %d: %d world rays, hits by geom type %s, %d left out; %d rays of link %d, hits %s, %d left out; coplanar ties off the knife edges: %d"
          % (gripper, nenv * nrays, kinds, left, nenv * nrays, rb[0], lkinds, lleft, ties))
    assert sum(kinds.values()) > 0.8 * nenv * nrays and sum(lkinds.values()) > 0.3 * nenv * nrays
    assert left <= 0.02 * nenv * nrays and lleft <= 0.02 * nenv * nrays, (left, lleft)


def test_body_frame_rays_and_exclusion():
    """rays bound to every moving finger body, after a squeeze: with the body excluded the device equals the reference on the world rays
    built from poses() with that body's geoms removed; the same rays without the exclusion hit the own body's box"""
    from softgrip_amd.manenv import tactile_rays
    m, nm, b, torch = _batch("softbox", 3)
    ty, sz, cats, gb = _geoms(m)
    _run(b, 2, 0, 70)
    tr = tactile_rays(m, (4, 4))
    d_body = tr["direction"].reshape(-1, 3)
    o_body = tr["origin"].reshape(-1, 3) - 0.01 * d_body        # 1 cm behind the face opposite the pad: outside the box
    body = tr["body"].reshape(-1)
    rs = np.random.RandomState(4)                                # and a fan of slanted rays from the same points
    o_body = np.concatenate([o_body, o_body])
    d_body = np.concatenate([d_body, d_body + rs.uniform(-0.4, 0.4, d_body.shape)])
    body = np.concatenate([body, body])
    assert len(set(body.tolist())) >= 2
    o, d = torch.tensor(o_body, device=b.device), torch.tensor(d_body, device=b.device)
    p = _poses(b)
    for lay in LAYOUTS:
        with layout(lay):
            excl = _host(b.raycast(o, d, body=body, exclude=body, normals=True))
            own = _host(b.raycast(o, d, body=body, normals=True))
        for e in range(3):
            gx, gm = p["geom_xpos"][e], p["geom_xmat"][e].reshape(-1, 3, 3)
            ow, dw = RR.map_rays(p["xpos"][e], p["xquat"][e], o_body, d_body, body)
            keep = RR.candidates(cats, gb, RR.ALL_BITS, body, len(body))
            ref = RR.cast(gx, gm, ty, sz, ow, dw, keep)
            RR.compare(tuple(x[e] for x in excl), ref, RR.unstable(gx, gm, ty, sz, ow, dw, keep, 0.0, ref), "excluded, env %d, %s" % (e, lay))
            assert not (gb[ref[1][ref[1] >= 0]] == body[ref[1] >= 0]).any()
            ref = RR.cast(gx, gm, ty, sz, ow, dw)
            RR.compare(tuple(x[e] for x in own), ref, RR.unstable(gx, gm, ty, sz, ow, dw, None, 0.0, ref), "not excluded, env %d, %s" % (e, lay))
            straight = slice(0, len(body) // 2)
            assert (own[1][e][straight] >= 0).all() and (gb[own[1][e][straight]] == body[straight]).all()
            assert np.abs(own[0][e][straight] - 0.01).max() < 1e-9


def _raw(b, ids, n_ids, n_rays, origin, dir_, body, excl, cat_mask, max_dist, flags, dist, geom, normal):
    from softgrip_amd.native import _ptr
    i32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    return b.L.sg_ray(b.ptr, i32(ids), n_ids, n_rays, _ptr(origin), _ptr(dir_), i32(body), i32(excl), cat_mask, max_dist, flags, _ptr(dist), _ptr(geom),
                      _ptr(normal), b._stream())


@pytest.fixture(scope="module")
def squeezed():
    """a 6-env softbox batch at env step 80 of the schedule, 257 rays of the recipe and the reference's answer per env"""
    m, nm, b, torch = _batch("softbox", 6)
    _run(b, 2, 0, 80)
    p = _poses(b)
    ty, sz, cats, gb = _geoms(m)
    o, d = RR.scene_rays(p["geom_xpos"][0], ty, 257, 7)
    refs = []
    for e in range(6):
        gx, gm = p["geom_xpos"][e], p["geom_xmat"][e].reshape(-1, 3, 3)
        ref = RR.cast(gx, gm, ty, sz, o, d)
        refs.append((ref, RR.unstable(gx, gm, ty, sz, o, d, None, 0.0, ref)))
    return dict(m=m, nm=nm, b=b, torch=torch, p=p, o=o, d=d, refs=refs, ot=torch.tensor(o, device=b.device), dt=torch.tensor(d, device=b.device))


@pytest.mark.parametrize("lay", LAYOUTS)
def test_shapes_and_interface(squeezed, lay):
    from softgrip_amd import native
    S = squeezed
    b, torch, ot, dt = S["b"], S["torch"], S["ot"], S["dt"]
    m = S["m"]
    ty, sz, cats, gb = _geoms(m)
    with layout(lay):
        full = _host(b.raycast(ot, dt, normals=True))
        for e in range(6):
            RR.compare(tuple(x[e] for x in full), S["refs"][e][0], S["refs"][e][1], "env %d" % e)
        # ray counts around the wavefront and the block: the first n rays give the first n answers
        for n in (1, 63, 64, 65, 257):
            got = _host(b.raycast(ot[:n], dt[:n], normals=True))
            for x, y in zip(got, full):
                assert x.tobytes() == np.ascontiguousarray(y[:, :n]).tobytes(), n
        # per-env rays equal shared rays when every env is given the same ones
        per = _host(b.raycast(ot[None].repeat(6, 1, 1), dt[None].repeat(6, 1, 1), normals=True))
        for x, y in zip(per, full):
            assert x.tobytes() == y.tobytes()
        # an env subset in permuted order (one env twice)
        ids = [4, 1, 1, 5, 0]
        sub = _host(b.raycast(ot, dt, env_ids=ids, normals=True))
        for x, y in zip(sub, full):
            assert x.tobytes() == np.ascontiguousarray(y[ids]).tobytes()
        # NULL outputs one at a time, and all of them
        kw = dict(dtype=torch.float64, device=b.device)
        for drop in ("dist", "geom", "normal", "all"):
            out = dict(dist=torch.full((6, 257), -7.5, **kw), geom=torch.full((6, 257), -77, dtype=torch.int32, device=b.device),
                       normal=torch.full((6, 257, 3), -7.5, **kw))
            args = {k: (None if drop in (k, "all") else v) for k, v in out.items()}
            assert _raw(b, None, 6, 257, ot, dt, None, None, 31, 0.0, 0, args["dist"], args["geom"], args["normal"]) == native.SG_OK
            for k, ref in zip(("dist", "geom", "normal"), full):
                h = out[k].cpu().numpy()
                if drop in (k, "all"):
                    assert (h == (-77 if k == "geom" else -7.5)).all(), (drop, k)
                else:
                    assert h.tobytes() == ref.tobytes(), (drop, k)
        # a direction without length, or not finite, is a miss; its neighbours are not affected
        d2 = dt.clone()
        d2[3] = 0.0
        d2[70, 1] = float("nan")
        d2[200, 2] = float("inf")
        got = _host(b.raycast(ot, d2, normals=True))
        for r in (3, 70, 200):
            assert (got[0][:, r] == -1).all() and (got[1][:, r] == -1).all() and not got[2][:, r].any()
        rest = np.setdiff1d(np.arange(257), [3, 70, 200])
        for x, y in zip(got, full):
            assert x[:, rest].tobytes() == y[:, rest].tobytes()
        # max_dist: hits beyond it are misses, the others stay
        lim = float(np.median(full[0][full[0] > 0]))
        got = _host(b.raycast(ot, dt, max_dist=lim, normals=True))
        near = (full[0] > 0) & (full[0] <= lim)
        assert (got[1][~near] == -1).all() and (got[0][~near] == -1).all() and near.any() and (full[1][~near] >= 0).any()
        for x, y in zip(got, full):
            assert x[near].tobytes() == y[near].tobytes()
        # category masks against the reference with those geoms removed
        for mask in (RR.GROUND_BIT, RR.ELEM_BIT | RR.CENTER_BIT, RR.ALL_BITS & ~RR.FINGER_BIT, RR.STATIC_BIT | RR.FINGER_BIT):
            got = _host(b.raycast(ot, dt, cat_mask=mask, normals=True))
            keep = RR.candidates(cats, gb, mask, None, 257)
            for e in (0, 5):
                gx, gm = S["p"]["geom_xpos"][e], S["p"]["geom_xmat"][e].reshape(-1, 3, 3)
                ref = RR.cast(gx, gm, ty, sz, S["o"], S["d"], keep)
                RR.compare(tuple(x[e] for x in got), ref, RR.unstable(gx, gm, ty, sz, S["o"], S["d"], keep, 0.0, ref), "mask %d env %d" % (mask, e))
                assert ((mask >> cats[ref[1][ref[1] >= 0]]) & 1).all()
        # a NaN env: NaN / -1 for it, the other envs unaffected
        st = b.get_state()
        q = st["qpos"].clone()
        q[2, 17] = float("nan")
        q[4, 3] = float("inf")
        b.set_state(qpos=q)
        try:
            got = _host(b.raycast(ot, dt, normals=True))
        finally:
            b.set_state(qpos=st["qpos"])
        for e in range(6):
            if e in (2, 4):
                assert np.isnan(got[0][e]).all() and (got[1][e] == -1).all() and np.isnan(got[2][e]).all()
            else:
                for x, y in zip(got, full):
                    assert x[e].tobytes() == y[e].tobytes()
        # every argument error
        good = dict(ids=None, n_ids=6, n_rays=257, origin=ot, dir_=dt, body=None, excl=None, cat_mask=31, max_dist=0.0, flags=0, dist=None, geom=None,
                    normal=None)
        assert _raw(b, **good) == native.SG_OK
        nb = S["nm"].nbody
        for bad in (dict(origin=None), dict(dir_=None), dict(n_ids=0), dict(n_rays=0), dict(n_ids=-1), dict(n_ids=3), dict(ids=[0, 6], n_ids=2),
                    dict(ids=[-1], n_ids=1), dict(body=[0] * 256 + [nb]), dict(body=[-2] + [0] * 256), dict(excl=[0] * 256 + [nb]),
                    dict(excl=[-2] + [0] * 256), dict(cat_mask=0), dict(cat_mask=32), dict(cat_mask=-1), dict(flags=2), dict(flags=3),
                    dict(max_dist=float("nan")), dict(max_dist=float("inf")), dict(max_dist=-float("inf"))):
            assert _raw(b, **dict(good, **bad)) == native.SG_ERR_INVALID, bad
            assert b"sg_ray" in b.L.sg_last_error(), bad
        assert b.L.sg_ray(None, None, 1, 1, _ptr8(), _ptr8(), None, None, 31, 0.0, 0, None, None, None, None) == native.SG_ERR_INVALID
        # the edge ids are fine: body nbody - 1, exclude -1
        assert _raw(b, **dict(good, body=[nb - 1] * 257, excl=[-1] * 257)) == native.SG_OK


def _ptr8():
    return C.c_void_p(8)      # never dereferenced: the NULL batch is refused first


def test_the_two_layouts_agree_bit_for_bit(squeezed):
    """on all three outputs, with body-frame rays, exclusion, a category mask and a distance limit in play; and the automatic choice
    gives those same bits on either side of its crossover"""
    S = squeezed
    b, torch = S["b"], S["torch"]
    m = S["m"]
    rs = np.random.RandomState(9)
    nb = S["nm"].nbody
    body = rs.randint(-1, nb, 257).astype(np.int32)
    excl = np.where(rs.rand(257) < 0.5, body, -1).astype(np.int32)
    ob = torch.tensor(rs.uniform(-0.3, 0.3, (257, 3)), device=b.device)
    db = torch.tensor(rs.normal(size=(257, 3)), device=b.device)
    res = {}
    for lay in LAYOUTS + (None,):
        with layout(lay):
            res[lay] = [_host(b.raycast(ob[:n], db[:n], body=body[:n], exclude=excl[:n], cat_mask=RR.ALL_BITS & ~RR.STATIC_BIT, max_dist=1.5, normals=True))
                        for n in (257, 8)]
    for lay in ("geoms", None):
        for got, want in zip(res[lay], res["rays"]):
            for x, y in zip(got, want):
                assert x.tobytes() == y.tobytes(), lay
    assert (res["rays"][0][1] >= 0).mean() > 0.2


@pytest.mark.parametrize("pipeline", ["rows", "tree"])
def test_no_side_effect_on_the_following_steps(pipeline):
    """two identical batches, one of them casting rays between the steps (both layouts, body-frame rays): sensors, flags, touch bits
    and state stay bit-identical"""
    runs = []
    for cast in (False, True):
        m, nm, b, torch = _batch("softbox", 5, pipeline)
        sens = torch.zeros(5, nm.nsensordata, dtype=torch.float64, device=b.device)
        flags = torch.zeros(5, dtype=torch.int32, device=b.device)
        touch = torch.zeros(5, dtype=torch.int32, device=b.device)
        b.set_ctrl_broadcast(np.full(2, -0.2))
        rs = np.random.RandomState(2)
        o = torch.tensor(rs.uniform(-0.5, 0.5, (70, 3)) + [0, 0, 1.5], device=b.device)
        d = torch.tensor(rs.normal(size=(70, 3)), device=b.device)
        body = rs.randint(-1, nm.nbody, 70)
        rec = []
        for t in range(12):
            if cast:
                with layout(LAYOUTS[t % 2]):
                    out = b.raycast(o, d, body=body, exclude=body, env_ids=None if t % 3 else [3, 0], normals=True)
                assert out["dist"].shape[1] == 70
            b.step(7, sens=sens, flags=flags, touch=touch)
            st = b.get_state()
            rec.append([sens.cpu().numpy().copy(), flags.cpu().numpy().copy(), touch.cpu().numpy().copy()] +
                       [st[k].cpu().numpy() for k in ("qpos", "qvel", "act", "qacc_warmstart")])
        runs.append(rec)
    for t, (a, c) in enumerate(zip(*runs)):
        for x, y in zip(a, c):
            assert x.tobytes() == y.tobytes(), t


def test_renderer_cross_check(squeezed):
    """the camera's rays (render_ref.camera_rays) through sg_ray at 32 x 24: the geom ids are sg_render's segid off the reference's
    silhouettes and dist x (d . forward) lies within the renderer's 1e-4 of its depth"""
    S = squeezed
    b, torch, m = S["b"], S["torch"], S["m"]
    W, H = 32, 24
    cam = S["nm"].default_camera()
    img = b.render(cam, None, W, H, rgb=False)
    eye, f, d = R.camera_rays(cam, W, H)
    dd = torch.tensor(d.reshape(-1, 3), device=b.device)
    oo = torch.tensor(np.tile(eye, (W * H, 1)), device=b.device)
    cats = R.categories(m)
    for lay in LAYOUTS:
        with layout(lay):
            dist, gid, _ = _host(b.raycast(oo, dd))
        for e in range(6):
            gx, gm = S["p"]["geom_xpos"][e], S["p"]["geom_xmat"][e].reshape(-1, 3, 3)
            ref_seg = R.render(gx, gm, m.geom_type, m.geom_size, cats, cam, W, H)[1]
            inner = ~R.silhouette(ref_seg)
            seg = img["seg"][e].cpu().numpy()
            depth = img["depth"][e].cpu().numpy().astype(np.float64)
            g = gid[e].reshape(H, W)
            assert (g[inner] == seg[inner]).all(), (lay, e)
            assert (g[inner] == ref_seg[inner]).all(), (lay, e)
            z = np.where(g >= 0, dist[e].reshape(H, W) * (d @ f), np.inf)
            hit = inner & (g >= 0)
            assert hit.mean() > 0.5 and np.isinf(depth[inner & (g < 0)]).all()
            assert np.abs(z - depth)[hit].max() <= 1e-4, (lay, e, np.abs(z - depth)[hit].max())


def test_tactile_depth_map():
    """ManEnv.tactile_depth(res=(4, 4)) on softbox at the reset state and at env step 100 equals the reference on the same rays; at the
    reset state (fingers open) every gap is +inf; at step 100 a box whose touch bit is set reports a gap below max_gap"""
    import torch
    from softgrip_amd.manenv import ManEnv, tactile_rays
    n, max_gap = 4, 0.05
    np.random.seed(5)
    env = ManEnv(1, 7, [model_path("softbox")], is_vis=False, n_envs=n)
    env.reset()
    m = env.model
    ty, sz, cats, gb = _geoms(m)
    tr = tactile_rays(m, (4, 4))
    o, d, body = tr["origin"].reshape(-1, 3), tr["direction"].reshape(-1, 3), tr["body"].reshape(-1)
    thick = np.repeat(tr["thickness"], 16)
    B = len(tr["geoms"])
    assert B == env.nmodel.nboxes
    keep = RR.candidates(cats, gb, RR.ELEM_BIT | RR.CENTER_BIT, body, len(o))
    lim = float(tr["thickness"].max()) + max_gap
    sched = episode_schedule()

    def check(what):
        got = {}
        for lay in LAYOUTS:
            with layout(lay):
                out = env.tactile_depth(res=(4, 4), max_gap=max_gap)
            assert out["gap"].shape == (n, B, 4, 4) and out["gap"].dtype == torch.float64 and out["geom"].dtype == torch.int32
            got[lay] = (out["gap"].cpu().numpy(), out["geom"].cpu().numpy())
        assert got["rays"][0].tobytes() == got["geoms"][0].tobytes() and got["rays"][1].tobytes() == got["geoms"][1].tobytes()
        gap, geom = got["rays"]
        p = _poses(env.get_env())
        left = 0
        for e in range(n):
            gx, gm = p["geom_xpos"][e], p["geom_xmat"][e].reshape(-1, 3, 3)
            ow, dw = RR.map_rays(p["xpos"][e], p["xquat"][e], o, d, body)
            ref = RR.cast(gx, gm, ty, sz, ow, dw, keep, lim)
            edge = RR.unstable(gx, gm, ty, sz, ow, dw, keep, lim, ref)
            rgap = ref[0] - thick
            seen = (ref[1] >= 0) & (rgap <= max_gap)
            want_gap, want_geom = np.where(seen, rgap, np.inf), np.where(seen, ref[1], -1)
            ge, ie = gap[e].reshape(-1), geom[e].reshape(-1)
            with np.errstate(invalid="ignore"):
                wrong = (ie != want_geom) | ~((ge == want_gap) | (np.abs(ge - want_gap) <= 1e-9))
            assert not (wrong & ~edge).any(), (what, e, np.flatnonzero(wrong & ~edge)[:5], ge[wrong & ~edge][:5], want_gap[wrong & ~edge][:5])
            left += int((wrong & edge).sum())
        assert left <= 0.02 * n * len(o), (what, left)
        return gap, geom

    gap, geom = check("reset")
    assert np.isposinf(gap).all() and (geom == -1).all()
    for t in range(100):
        if sched[t] is not None:
            (env.close_hand if sched[t] < 0 else env.loose_hand)()
        env.step()
    gap, geom = check("step 100")
    touch = env._touch.cpu().numpy()
    assert touch.any()
    found = 0
    for e in range(n):
        for k in range(B):
            if (int(touch[e]) >> k) & 1:
                found += int((gap[e, k] < max_gap).any())
    assert found >= 1
    assert np.isin(cats[geom[geom >= 0]], (3, 4)).all()
    # raycast passes through
    ot, dt = torch.tensor(o, device=env.get_env().device), torch.tensor(d, device=env.get_env().device)
    a = env.raycast(ot, dt, body=body, exclude=body, env_ids=[1])
    c = env.get_env().raycast(ot, dt, body=body, exclude=body, env_ids=[1])
    assert a["dist"].cpu().numpy().tobytes() == c["dist"].cpu().numpy().tobytes() and set(a) == {"dist", "geom"}
