"""sg_ray with SG_RAY_SKIN on the GPU: per-env rays against the NumPy reference (tests/ray_skin_ref.py) on the device's own poses under both
kernel layouts, which agree bit for bit; ray counts around the wavefront and block sizes, env subsets, NULL outputs, a skin at the
limits; the plain path untouched; a skin replaced under a live batch; NaN envs; ManEnv.tactile_depth(skin=True); no side effect on a
following step."""
import numpy as np
import pytest

import ray_ref as RR
import ray_skin_ref as RS
from helpers import model_path
from test_gpu_ray import LAYOUTS, _host, _poses, _raw, _run, layout

import softgrip_amd as sg
from softgrip_amd.mjcf import quat_to_mat

pytestmark = pytest.mark.gpu


def _batch(scene, n, attach=True):
    import torch
    from softgrip_amd import native
    m = sg.load_model(model_path(scene), "implicit")
    nm = native.NativeModel(m)
    if attach:
        nm.set_skin(m.composite_skin())
    b = native.NativeBatch(nm, n, 0)
    b.reset(1)
    return m, nm, b, torch


def _geoms(m):
    return np.asarray(m.geom_type), np.asarray(m.geom_size, dtype=np.float64), RR.categories(m), np.asarray(m.geom_bodyid)


def _reference(m, skin, p, e, o, d, cat_mask=RR.ALL_BITS, exclude=None, max_dist=0.0):
    """the reference's answer and its unstable rays for env e of poses p (world rays o, d)"""
    ty, sz, cats, gb = _geoms(m)
    gx, gm = p["geom_xpos"][e], p["geom_xmat"][e].reshape(-1, 3, 3)
    verts = RS.vertices(skin, p["xpos"][e], p["xquat"][e])
    ref = RS.cast(gx, gm, ty, sz, cats, gb, skin, verts, o, d, cat_mask, exclude, max_dist)
    return ref, RS.unstable(gx, gm, ty, sz, cats, gb, skin, verts, o, d, cat_mask, exclude, max_dist, ref)


def _same(a, b, what=""):
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes(), what


@pytest.mark.parametrize("scene", ["softball", "fourfinger_softball_fix"])
def test_per_env_rays_match_reference(scene):
    """256 rays of the recipe per env, different ones per env (SG_RAY_PER_ENV), at the reset state and at env step 20 of the reference
    schedule: ids exact (the face with them), distances and normals within 1e-9 of the reference on the device's poses; the two layouts
    bit-identical.  Left out: only rays the reference itself marks unstable, at most 2 %; more than 25 % of the rays hit the skin"""
    m, nm, b, torch = _batch(scene, 2)
    skin = nm.skin()
    ty = np.asarray(m.geom_type)
    total = left = on_skin = 0
    t_at = 0
    for t in (0, 20):
        _run(b, nm.nu, t_at, t)
        t_at = t
        p = _poses(b)
        rays = [RR.scene_rays(p["geom_xpos"][e], ty, 256, 1000 * t + e) for e in range(2)]
        o = torch.tensor(np.stack([r[0] for r in rays]), device=b.device)
        d = torch.tensor(np.stack([r[1] for r in rays]), device=b.device)
        got = {}
        for lay in LAYOUTS:
            with layout(lay):
                out = b.raycast(o, d, normals=True, skin=True)
            got[lay] = _host(out)
            face = out["face"].cpu().numpy()
            assert face.dtype == np.int32 and (face == RS.faces_of(got[lay][1], m.ngeom)).all()
        _same(got["rays"], got["geoms"], (scene, t))
        for e in range(2):
            ref, edge = _reference(m, skin, p, e, *rays[e])
            left += RR.compare(tuple(x[e] for x in got["rays"]), ref, edge, "%s step %d env %d" % (scene, t, e))
            total += 256
            on_skin += int((ref[1] >= m.ngeom).sum())
    print("%s: %d rays, %d on the skin, %d left out" % (scene, total, on_skin, left))
    assert left <= 0.02 * total and on_skin > 0.25 * total


@pytest.fixture(scope="module")
def ball():
    """a 3-env softball batch (432 faces) at env step 5, 257 rays of the recipe, the skin answer of the env subset [2, 0, 1] under the
    lane-per-ray layout, checked against the reference once"""
    m, nm, b, torch = _batch("softball", 3)
    _run(b, nm.nu, 0, 5)
    ids = [2, 0, 1]
    p = _poses(b, ids)
    o, d = RR.scene_rays(p["geom_xpos"][0], np.asarray(m.geom_type), 257, 7)
    ot, dt = torch.tensor(o, device=b.device), torch.tensor(d, device=b.device)
    with layout("rays"):
        full = _host(b.raycast(ot, dt, env_ids=ids, normals=True, skin=True))
    skin = nm.skin()
    assert len(skin["face"]) == 432
    for k in range(3):
        ref, edge = _reference(m, skin, p, k, o, d)
        RR.compare(tuple(x[k] for x in full), ref, edge, "listed env %d" % k)
    assert (full[1] >= m.ngeom).mean() > 0.25
    return dict(m=m, nm=nm, b=b, torch=torch, ids=ids, o=o, d=d, ot=ot, dt=dt, full=full, p=p)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_ray_counts_around_wavefront_and_block(ball, n):
    """the first n rays give the first n answers, shared and per-env rays alike, under both layouts, on an env subset in non-ascending
    order"""
    S = ball
    b, ids = S["b"], S["ids"]
    want = tuple(np.ascontiguousarray(x[:, :n]) for x in S["full"])
    on, dn = S["ot"][:n].contiguous(), S["dt"][:n].contiguous()
    for lay in LAYOUTS:
        with layout(lay):
            _same(_host(b.raycast(on, dn, env_ids=ids, normals=True, skin=True)), want, (lay, n, "shared"))
            _same(_host(b.raycast(on[None].repeat(3, 1, 1), dn[None].repeat(3, 1, 1), env_ids=ids, normals=True, skin=True)), want, (lay, n, "per env"))


@pytest.mark.parametrize("lay", LAYOUTS)
def test_null_outputs(ball, lay):
    from softgrip_amd import native
    S = ball
    b, torch, ids = S["b"], S["torch"], S["ids"]
    kw = dict(dtype=torch.float64, device=b.device)
    with layout(lay):
        for drop in ("dist", "geom", "normal", "all"):
            out = dict(dist=torch.full((3, 257), -7.5, **kw), geom=torch.full((3, 257), -77, dtype=torch.int32, device=b.device),
                       normal=torch.full((3, 257, 3), -7.5, **kw))
            args = {k: (None if drop in (k, "all") else v) for k, v in out.items()}
            assert _raw(b, ids, 3, 257, S["ot"], S["dt"], None, None, 31, 0.0, native.SG_RAY_SKIN, args["dist"], args["geom"], args["normal"]) == native.SG_OK
            for k, ref in zip(("dist", "geom", "normal"), S["full"]):
                h = out[k].cpu().numpy()
                if drop in (k, "all"):
                    assert (h == (-77 if k == "geom" else -7.5)).all(), (drop, k)
                else:
                    assert h.tobytes() == ref.tobytes(), (drop, k)


def _limit_skin(skin):
    """the composite's skin padded to the limits, 256 vertices and 512 faces: vertices 218 .. 255 repeat vertices 0 .. 37 (other
    indices, the same bodies and places), faces 432 .. 511 repeat faces 0 .. 79 over them where they can"""
    vb, vp, fc = np.asarray(skin["vert_body"]), np.asarray(skin["vert_pos"]), np.asarray(skin["face"])
    nv, extra = len(vb), 256 - len(vb)
    assert extra > 0 and 512 - len(fc) > 0
    twin = np.arange(nv)
    twin[:extra] = nv + np.arange(extra)
    more = twin[fc[:512 - len(fc)]]
    return dict(vert_body=np.concatenate([vb, vb[:extra]]), vert_pos=np.concatenate([vp, vp[:extra]]), face=np.concatenate([fc, more]), rgba=skin["rgba"])


def test_a_skin_at_the_limits(ball):
    """256 vertices and 512 faces through set_skin: both layouts bit-identical and equal to the reference; the batch picks it up, and the
    composite's own skin again afterwards"""
    S = ball
    m, nm, b, ids = S["m"], S["nm"], S["b"], S["ids"]
    old = nm.skin()
    big = _limit_skin(old)
    assert len(big["vert_body"]) == 256 and len(big["face"]) == 512
    nm.set_skin(big)
    try:
        got = {}
        for lay in LAYOUTS:
            with layout(lay):
                got[lay] = _host(b.raycast(S["ot"], S["dt"], env_ids=ids, normals=True, skin=True))
        _same(got["rays"], got["geoms"])
        for k in (0, 2):
            ref, edge = _reference(m, big, S["p"], k, S["o"], S["d"])
            RR.compare(tuple(x[k] for x in got["rays"]), ref, edge, "limits, listed env %d" % k)
        assert (got["rays"][1] >= m.ngeom).mean() > 0.25 and got["rays"][1].max() < m.ngeom + 512
    finally:
        nm.set_skin(old)
    with layout("geoms"):
        _same(_host(b.raycast(S["ot"], S["dt"], env_ids=ids, normals=True, skin=True)), S["full"])


def test_category_mask_exclusion_and_body_frame(ball):
    """on the device as on the host: without the element bit no triangle and no hidden geom; an excluded element body takes its triangles
    along; body-frame rays with a distance limit -- all against the reference, both layouts bit-identical"""
    S = ball
    m, nm, b, torch, ids = S["m"], S["nm"], S["b"], S["torch"], S["ids"]
    skin = nm.skin()
    ty, sz, cats, gb = _geoms(m)
    hidden = np.flatnonzero(RS.hidden_geoms(gb, skin))
    vb, face = np.asarray(skin["vert_body"]), np.asarray(skin["face"])
    seen = np.bincount(S["full"][1][S["full"][1] >= m.ngeom] - m.ngeom, minlength=len(face))
    body = int(vb[face[seen.argmax()][0]])
    ex = np.full(257, body, np.int32)
    finger = int(np.flatnonzero(np.asarray(m.body_weldid) != 0)[0])
    fb = np.full(257, finger, np.int32)
    rs = np.random.RandomState(3)
    ol, dl = rs.uniform(-0.05, 0.05, (257, 3)), rs.normal(size=(257, 3))
    olt, dlt = torch.tensor(ol, device=b.device), torch.tensor(dl, device=b.device)
    cases = [dict(cat_mask=RR.ALL_BITS & ~RR.ELEM_BIT), dict(cat_mask=RR.ELEM_BIT | RR.CENTER_BIT), dict(exclude=ex), dict(body=fb, exclude=fb, max_dist=0.6)]
    for kw in cases:
        got = {}
        for lay in LAYOUTS:
            with layout(lay):
                local = "body" in kw
                got[lay] = _host(b.raycast(olt if local else S["ot"], dlt if local else S["dt"], env_ids=ids, normals=True, skin=True, **kw))
        _same(got["rays"], got["geoms"], kw)
        gid = got["rays"][1]
        assert not np.isin(gid, hidden).any()
        if "cat_mask" in kw and not kw["cat_mask"] & RR.ELEM_BIT:
            assert (gid < m.ngeom).all()
        if "exclude" in kw and "body" not in kw:
            assert not np.isin(gid - m.ngeom, np.flatnonzero((vb[face] == body).any(1))).any()
        for k in (1,):
            p = S["p"]
            o, d = (RR.map_rays(p["xpos"][k], p["xquat"][k], ol, dl, fb) if "body" in kw else (S["o"], S["d"]))
            ref, edge = _reference(m, skin, p, k, o, d, kw.get("cat_mask", RR.ALL_BITS), kw.get("exclude"), kw.get("max_dist", 0.0))
            RR.compare(tuple(x[k] for x in got["rays"]), ref, edge, str(sorted(kw)))


def test_the_plain_path_is_untouched():
    """SG_RAY_SKIN on a model without a skin, flags = 0 on a model with one, and SG_RAY_SKIN after the skin was removed: the plain call's
    bytes"""
    from softgrip_amd import native
    m, nm, b, torch = _batch("softball", 2, attach=False)
    _run(b, nm.nu, 0, 3)
    assert nm.skin() is None
    o, d = RR.scene_rays(_poses(b)["geom_xpos"][0], np.asarray(m.geom_type), 70, 1)
    ot, dt = torch.tensor(o, device=b.device), torch.tensor(d, device=b.device)

    def call(flags):
        out = dict(dist=torch.zeros(2, 70, dtype=torch.float64, device=b.device), geom=torch.zeros(2, 70, dtype=torch.int32, device=b.device),
                   normal=torch.zeros(2, 70, 3, dtype=torch.float64, device=b.device))
        assert _raw(b, None, 2, 70, ot, dt, None, None, 31, 0.0, flags, out["dist"], out["geom"], out["normal"]) == native.SG_OK
        return _host(out)

    for lay in LAYOUTS:
        with layout(lay):
            plain = call(0)
            assert plain[1].max() < m.ngeom and (plain[1] >= 0).any()
            _same(call(native.SG_RAY_SKIN), plain, "no skin")
            nm.set_skin(m.composite_skin())
            _same(call(0), plain, "a skin, no flag")
            assert (call(native.SG_RAY_SKIN)[1] >= m.ngeom).any()
            nm.set_skin(None)
            _same(call(native.SG_RAY_SKIN), plain, "the skin removed")
    # the Python interface: skin=True on a model without a skin attaches the composite's; `face` only with skin=True
    out = b.raycast(ot, dt, skin=True)
    assert nm.skin() is not None and set(out) == {"dist", "geom", "face"} and (out["face"] >= 0).any()
    assert set(b.raycast(ot, dt)) == {"dist", "geom"}
    assert _raw(b, None, 2, 70, ot, dt, None, None, 31, 0.0, 8, None, None, None) == native.SG_ERR_INVALID and b"unknown flag bits" in b.L.sg_last_error()


def test_a_new_skin_is_picked_up():
    """set_skin between two calls: one vertex moved 5 cm outward (its body's +z); a ray aimed at its new place from 5 cm farther out hits
    a face of that vertex at 5 cm in the second call and the old surface, farther away, in the first"""
    m, nm, b, torch = _batch("softball", 2)
    skin = nm.skin()
    p = _poses(b)
    v = 17
    body = int(skin["vert_body"][v])
    out_w = quat_to_mat(p["xquat"][0][body]) @ np.array([0.0, 0.0, 1.0])
    new = RS.vertices(skin, p["xpos"][0], p["xquat"][0])[v] + 0.05 * out_w
    o = torch.tensor((new + 0.05 * out_w)[None], device=b.device)
    d = torch.tensor(-out_w[None], device=b.device)
    moved = dict(skin, vert_pos=np.array(skin["vert_pos"], dtype=np.float64))
    moved["vert_pos"][v, 2] += 0.05
    for lay in LAYOUTS:
        with layout(lay):
            nm.set_skin(skin)
            before = b.raycast(o, d, env_ids=[0], skin=True)
            nm.set_skin(moved)
            after = b.raycast(o, d, env_ids=[0], skin=True)
        f = int(after["face"][0, 0])
        assert f >= 0 and v in skin["face"][f] and abs(float(after["dist"][0, 0]) - 0.05) <= 1e-9, (lay, f, float(after["dist"][0, 0]))
        assert float(before["dist"][0, 0]) > 0.05 + 0.04 and int(before["face"][0, 0]) >= 0, (lay, float(before["dist"][0, 0]))


def test_nan_envs(ball):
    S = ball
    b, ids = S["b"], S["ids"]
    st = b.get_state()
    q = st["qpos"].clone()
    q[0, 9] = float("nan")
    b.set_state(qpos=q)
    try:
        got = {}
        for lay in LAYOUTS:
            with layout(lay):
                got[lay] = _host(b.raycast(S["ot"], S["dt"], env_ids=ids, normals=True, skin=True))
    finally:
        b.set_state(qpos=st["qpos"])
    for lay in LAYOUTS:
        for k, e in enumerate(ids):
            if e == 0:
                assert np.isnan(got[lay][0][k]).all() and (got[lay][1][k] == -1).all() and np.isnan(got[lay][2][k]).all()
            else:
                _same(tuple(x[k] for x in got[lay]), tuple(x[k] for x in S["full"]), (lay, e))


def test_tactile_depth_with_the_skin():
    """ManEnv.tactile_depth(res=(4, 4), skin=True) on 2 envs of softball after 20 env steps of the squeeze: gap, geom and face against the
    reference on the same rays; skin=False on the same state is the plain map, byte for byte"""
    import torch
    from softgrip_amd import native
    from softgrip_amd.create_dataset import episode_schedule
    from softgrip_amd.manenv import ManEnv, tactile_rays
    n, max_gap = 2, 0.05
    np.random.seed(5)
    env = ManEnv(1, 7, [model_path("softball")], is_vis=False, n_envs=n)
    env.reset()
    sched = episode_schedule()
    for t in range(20):
        if sched[t] is not None:
            (env.close_hand if sched[t] < 0 else env.loose_hand)()
        env.step()
    m = env.model
    tr = tactile_rays(m, (4, 4))
    o, d, body = tr["origin"].reshape(-1, 3), tr["direction"].reshape(-1, 3), tr["body"].reshape(-1)
    thick = np.repeat(tr["thickness"], 16)
    B = len(tr["geoms"])
    lim = float(tr["thickness"].max()) + max_gap
    mask = RR.ELEM_BIT | RR.CENTER_BIT
    got = {}
    for lay in LAYOUTS:
        with layout(lay):
            out = env.tactile_depth(res=(4, 4), max_gap=max_gap, skin=True)
        assert set(out) == {"gap", "geom", "face"} and out["face"].shape == (n, B, 4, 4) and out["face"].dtype == torch.int32
        got[lay] = tuple(out[k].cpu().numpy() for k in ("gap", "geom", "face"))
    _same(got["rays"], got["geoms"])
    skin = env.nmodel.skin()
    assert skin is not None
    p = _poses(env.get_env())
    left = 0
    for e in range(n):
        ow, dw = RR.map_rays(p["xpos"][e], p["xquat"][e], o, d, body)
        ref, edge = _reference(m, skin, p, e, ow, dw, mask, body, lim)
        rgap = ref[0] - thick
        seen = (ref[1] >= 0) & (rgap <= max_gap)
        want_gap, want_geom = np.where(seen, rgap, np.inf), np.where(seen, ref[1], -1)
        ge, ie, fe = (x[e].reshape(-1) for x in got["rays"])
        with np.errstate(invalid="ignore"):
            wrong = (ie != want_geom) | (fe != RS.faces_of(want_geom, m.ngeom)) | ~((ge == want_gap) | (np.abs(ge - want_gap) <= 1e-9))
        assert not (wrong & ~edge).any(), (e, np.flatnonzero(wrong & ~edge)[:5], ge[wrong & ~edge][:5], want_gap[wrong & ~edge][:5])
        left += int((wrong & edge).sum())
    assert left <= 0.02 * n * len(o)
    # skin=False: the plain call and the formula, as before
    plain = env.tactile_depth(res=(4, 4), max_gap=max_gap, skin=False)
    assert set(plain) == {"gap", "geom"}
    dev = env.get_env().device
    raw = env.get_env().raycast(torch.tensor(o, device=dev), torch.tensor(d, device=dev), body=body, exclude=body, cat_mask=mask, max_dist=lim)
    dist = raw["dist"].view(n, B, 4, 4)
    gap = dist - torch.tensor(tr["thickness"], device=dev).view(1, B, 1, 1)
    seen = (dist >= 0) & (gap <= max_gap)
    assert torch.equal(plain["gap"], torch.where(seen, gap, torch.full_like(gap, float("inf"))))
    assert torch.equal(plain["geom"], torch.where(seen, raw["geom"].view(n, B, 4, 4), torch.full_like(plain["geom"], -1)))
    assert int(plain["geom"].max()) < m.ngeom
    assert native.SG_RAY_SKIN == 4


def test_no_side_effect_on_the_following_step():
    """two identical batches, one of them casting skin rays (both layouts) in front of every step: the state bytes stay equal"""
    runs = []
    for cast in (False, True):
        m, nm, b, torch = _batch("softball", 3)
        b.set_ctrl_broadcast(np.full(nm.nu, -0.2))
        rs = np.random.RandomState(2)
        o = torch.tensor(rs.uniform(-0.3, 0.3, (70, 3)) + [0, 0, 1.5], device=b.device)
        d = torch.tensor(rs.normal(size=(70, 3)), device=b.device)
        rec = []
        for t in range(6):
            if cast:
                with layout(LAYOUTS[t % 2]):
                    out = b.raycast(o, d, env_ids=None if t % 3 else [2, 0], normals=True, skin=True)
                assert out["face"].shape[1] == 70
            b.step(7)
            st = b.get_state()
            rec.append([st[k].cpu().numpy() for k in ("qpos", "qvel", "act", "qacc_warmstart")])
        runs.append(rec)
    for t, (a, c) in enumerate(zip(*runs)):
        _same(a, c, t)
