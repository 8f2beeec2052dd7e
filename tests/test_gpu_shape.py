"""sg_get_skin_vertices / sg_get_shape / sg_get_subtree on the GPU: every output of the three entry points against the NumPy reference
(tests/shape_ref.py, held against the g++ build and known answers by tests/test_shape_host.py) at the device's own read-back states,
synthetic skins through sg_model_set_skin up to the vertex limit, the calls' interface (env lists, NULL outputs, direction lists, NaN
envs, determinism, no side effect), every refusal, and ManEnv's methods.  Bounds: shape_ref's.  Each test: 3 envs of dyn_ref.KS,
sg_reset and 6 env steps of a squeeze.
Worst deviations measured on the MI355X, in units of the bound: see test_every_output_matches_the_reference."""
import ctypes as C

import numpy as np
import pytest

import dyn_ref as DR
import shape_ref as SR
from helpers import model_path

pytestmark = pytest.mark.gpu

VERT, EXT, SUB = ("pos", "vel", "local"), ("lo", "hi", "lo_vert", "hi_vert"), ("com", "linvel", "angmom")


def _torch():
    import torch
    return torch


def _object_joints(m, root):
    """the slide joints of the object's bodies: what takes the per-env stiffness"""
    from softgrip_amd.mjcf import JNT_SLIDE
    sub = SR.subtree_lists(m)[root]
    return [j for b in sub for j in range(m.body_jntadr[b], m.body_jntadr[b] + m.body_jntnum[b]) if m.jnt_type[j] == JNT_SLIDE]


def _batch(scene, ks=DR.KS, skin="composite"):
    """(model, NativeModel, batch, skin dict): the scene with its composite skin attached (skin=None: none)"""
    from softgrip_amd import native
    m = SR.load(scene)
    nm = native.NativeModel(m)
    made = m.composite_skin() if skin == "composite" else skin
    nm.set_skin(made)
    b = native.NativeBatch(nm, len(ks), 0)
    if scene in DR.SCENES:
        jids, tids = DR.SCENES[scene][1:3]
    else:
        jids, tids = _object_joints(m, 38 if scene.startswith("fourfinger") else 10), [0]
    b.set_stiffness(np.asarray(ks, dtype=np.float64), jids, tids)
    return m, nm, b, made


def _squeeze(b, nu, nsteps=6):
    torch = _torch()
    flags = torch.zeros(b.n, dtype=torch.int32, device=b.device)
    b.reset(1, flags=flags)
    assert int(flags.abs().sum()) == 0
    b.set_ctrl_broadcast(np.full(nu, -0.2))
    for _ in range(nsteps):
        b.step(7, flags=flags)
        assert int(flags.abs().sum()) == 0


def _all(b, frame=-1, dirs=None, db=None, env_ids=None, shape=True):
    """the three calls' outputs as one dict of device tensors"""
    out = dict(b.skin_vertices(frame_body=frame, env_ids=env_ids))
    out.update(b.shape(dirs=dirs, dir_body=db, env_ids=env_ids, shape=shape))
    out.update(b.subtree(env_ids=env_ids))
    return out


def _host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _same_bits(a, b):
    torch = _torch()
    view = torch.int64 if a.dtype == torch.float64 else a.dtype
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(a.contiguous().view(view), b.contiguous().view(view)))


def _state(b):
    st = b.get_state()
    return st["qpos"].cpu().numpy(), st["qvel"].cpu().numpy()


def _check_envs(m, skin, got, qpos, qvel, frame, dirs, db, what, worst, physical=False):
    for e in range(len(qpos)):
        ref = SR.reference(m, skin, qpos[e], qvel[e], frame, dirs, db)
        if physical:
            # the isoperimetric inequality and the centroid inside every extent: of the reference first, then of the device
            for src, sh, lo, hi in (("reference", ref["shape"], ref["lo"], ref["hi"]), ("device", got["shape"][e], got["lo"][e], got["hi"][e])):
                assert sh[1] ** 3 >= 36 * np.pi * sh[0] ** 2, (what, e, src)
                hc = np.einsum("di,di->d", ref["dir_world"], sh[2:5] - ref["dir_origin"])
                assert (lo <= hc).all() and (hc <= hi).all(), (what, e, src)
        SR.compare({k: v[e] for k, v in got.items()}, ref, "%s env %d" % (what, e), worst)


# ---- 1. every output against the reference at the read-back state ----
@pytest.mark.parametrize("scene", ["softbox", "softbox_fix", "softball", "fourfinger_softball_fix", "freeball_fix"])
def test_every_output_matches_the_reference(scene):
    """softbox (rows pipeline), softbox_fix (tree), softball (218 vertices and 432 faces: 4 and 7 strides with a ragged last one),
    the four-finger scene and the free ball, whose object moves as a whole: pos, vel, local in the object's frame, the shape, six
    directions (a skew one that is not unit, two palm-fixed) and the subtree rows of all bodies, per env against the reference at
    shape_ref's bounds; A^3 >= 36 pi V^2 and lo <= d . (centroid - o) <= hi hold for the reference and for the device.
    Worst deviations on the MI355X in units of the bound, over the five scenes: pos 1.8e-4, vel 1.1e-4, local 5.6e-4, V 4.1e-5,
    A 1.8e-5, centroid 4.0e-5, moments 6.0e-5, dV/dt 2.7e-5, extents 1.1e-4, com 2.1e-4, linvel 1.5e-4, angmom 7.8e-5"""
    m, nm, b, skin = _batch(scene)
    nu = DR.SCENES[scene][3] if scene in DR.SCENES else 2
    _squeeze(b, nu)
    qpos, qvel = _state(b)
    assert np.abs(qvel).max() > 1e-3, "the state must move"
    root = nm.skin_root()
    assert root == (38 if scene.startswith("fourfinger") else 10) and nm.skin_closed() == 1
    dirs, db = SR.directions(m, 3)
    worst = {}
    _check_envs(m, skin, _host(_all(b, root, dirs, db)), qpos, qvel, root, dirs, db, scene, worst, physical=True)
    print(scene, "worst deviation in units of the bound:", {k: "%.2e" % v for k, v in sorted(worst.items())})


# ---- 2. synthetic skins through sg_model_set_skin ----
def test_synthetic_skins_and_a_replaced_skin():
    """on softbox_fix a squeeze in, one batch throughout: the tetrahedron (4 vertices, 4 faces: fewer than a stride) on four bodies;
    the 10 x 8 x 5 box-grid shell of exactly 256 vertices and 508 faces -- the vertex limit -- bound to bodies spread over the whole
    tree; a skin bound to the world body alone, whose vel and dV/dt are exactly 0; after every sg_model_set_skin the next call answers
    for the new skin"""
    m, nm, b, _ = _batch("softbox_fix", skin=None)
    _squeeze(b, 2)
    qpos, qvel = _state(b)
    P, face = SR.tetrahedron()
    Pg, fg = SR.grid_shell()
    assert len(Pg) == 256 and len(fg) == 508 and SR.is_closed(fg)
    dirs, db = SR.directions(m, 5)
    skins = [("tetrahedron", SR.skin_of([12, 40, 77, 3], 0.1 * P, face), 12), ("grid shell", SR.skin_of((np.arange(256) * 7) % m.nbody, Pg - Pg.mean(0), fg), -1),
             ("world", SR.skin_of([0, 0, 0, 0], P + [0.5, 0.2, 1.0], face), 4), ("tetrahedron again", SR.skin_of([12, 40, 77, 3], 0.1 * P, face), 0)]
    for name, skin, frame in skins:
        nm.set_skin(skin)
        assert nm.skin_closed() == 1
        got = _host(_all(b, frame, dirs, db))
        assert got["pos"].shape == (3, len(skin["vert_body"]), 3)
        worst = {}
        _check_envs(m, skin, got, qpos, qvel, frame, dirs, db, name, worst)
        print(name, {k: "%.2e" % v for k, v in sorted(worst.items())})
        if name == "world":
            assert (got["vel"] == 0).all() and (got["shape"][:, 11] == 0).all()
            assert (got["pos"] == got["pos"][0]).all() and np.abs(got["shape"][:, 0] - 1.0 / 6.0).max() <= 1e-15


# ---- 3. the interface ----
def _raw(b, ids, frame, dirs, db, out):
    """the three entry points with any output left out (None -> NULL); dirs / db host arrays or None"""
    from softgrip_amd.native import _ptr
    n_ids = b.n if ids is None else len(ids)
    arr = None if ids is None else np.ascontiguousarray(ids, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    L, s, g = b.L, b._stream(), lambda n: _ptr(out.get(n))  # noqa: E731
    hd = None if dirs is None else np.ascontiguousarray(dirs, np.float64)
    hb = None if db is None else np.ascontiguousarray(db, np.int32)
    b._check(L.sg_get_skin_vertices(b.ptr, arr, n_ids, frame, g("pos"), g("vel"), g("local"), s))
    b._check(L.sg_get_shape(b.ptr, arr, n_ids, 0 if hd is None else len(hd), None if hd is None else hd.ctypes.data_as(C.c_void_p),
                            None if hb is None else hb.ctypes.data_as(C.POINTER(C.c_int32)), g("shape"), g("lo"), g("hi"), g("lo_vert"), g("hi_vert"), s))
    b._check(L.sg_get_subtree(b.ptr, arr, n_ids, g("com"), g("linvel"), g("angmom"), s))


def test_listing_directions_and_determinism():
    """softball, 5 envs: two calls give the same bits; env_ids as a subset, a permutation and with a repeated id reproduce the all-env
    rows bit for bit; every output alone (the others NULL) and the extents without the shape keep their bits; a direction keeps its
    bits alone, in another place and among 256; n_dirs = 0 with NULL arrays runs"""
    torch = _torch()
    ks = np.linspace(300, 1400, 5)
    m, nm, b, skin = _batch("softball", ks)
    _squeeze(b, 2, nsteps=4)
    dirs, db = SR.directions(m, 3)
    full = _all(b, 10, dirs, db)
    again = _all(b, 10, dirs, db)
    for name in full:
        assert _same_bits(full[name], again[name]), name
    for ids in ([4, 1], [3, 0, 2, 4, 1], [2, 2, 0], [3]):
        part = _all(b, 10, dirs, db, env_ids=ids)
        for name in full:
            assert _same_bits(part[name], full[name][torch.as_tensor(ids, device=b.device)]), (ids, name)
    for keep in [(n,) for n in VERT + ("shape",) + EXT + SUB] + [EXT, ("pos", "lo_vert", "angmom")]:
        out = {n: torch.full_like(full[n], -7) for n in keep}
        _raw(b, None, 10, dirs, db, out)
        for n in keep:
            assert _same_bits(out[n], full[n]), (keep, n)
    _raw(b, None, 10, None, None, {})      # every output NULL, n_dirs = 0 with NULL arrays: nothing to write, no error
    out = {"shape": torch.full_like(full["shape"], -7)}
    _raw(b, None, 10, None, None, out)
    assert _same_bits(out["shape"], full["shape"])
    order = [5, 3, 0]
    part = b.shape(dirs=dirs[order], dir_body=db[order])
    for n in EXT:
        assert _same_bits(part[n], full[n][:, order]), n
    rs = np.random.RandomState(7)
    many = rs.standard_normal((256, 3))
    mb = rs.randint(-1, m.nbody, 256)
    many[200], mb[200] = dirs[4], db[4]
    big = b.shape(dirs=many, dir_body=mb, shape=False)
    assert "shape" not in big
    for n in EXT:
        assert _same_bits(big[n][:, 200], full[n][:, 4]), n
    got = _host(big)
    qpos, qvel = _state(b)
    ref = SR.reference(m, skin, qpos[2], qvel[2], -1, many, mb)
    SR.compare({k: v[2] for k, v in got.items()}, ref, "256 directions")


def test_nan_envs_get_nan_and_disturb_no_other():
    """a NaN in env 1's qvel, one in env 3's qpos and an inf in env 4's qvel: NaN in every double output and -1 in every int output of
    those envs, unchanged bits in the others'"""
    torch = _torch()
    ks = np.linspace(300, 1400, 6)
    m, nm, b, _ = _batch("freeball_fix", ks)
    _squeeze(b, 2, nsteps=3)
    dirs, db = SR.directions(m, 3)
    clean = _all(b, 10, dirs, db)
    st = b.get_state()
    st["qvel"][1, 17] = float("nan")
    st["qpos"][3, 5] = float("nan")
    st["qvel"][4, 0] = float("inf")
    b.set_state(qpos=st["qpos"], qvel=st["qvel"])
    got = _all(b, 10, dirs, db)
    for name, x in got.items():
        for e in range(6):
            if e in (1, 3, 4):
                assert bool((x[e] == -1).all() if x.dtype == torch.int32 else torch.isnan(x[e]).all()), (name, e)
            else:
                assert _same_bits(x[e], clean[name][e]), (name, e)


def test_calls_change_nothing():
    """the state is bit-identical before and after the calls, and a twin batch that made no call produces bit-identical sensors, flags,
    touch and state from the next sg_step"""
    torch = _torch()
    outs = []
    for read in (True, False):
        m, nm, b, _ = _batch("softbox", DR.KS)
        _squeeze(b, 2, nsteps=4)
        if read:
            dirs, db = SR.directions(m, 3)
            before = b.get_state()
            _all(b, 10, dirs, db)
            _all(b, -1, dirs[:2], None, env_ids=[2, 0])
            after = b.get_state()
            for name in before:
                assert _same_bits(before[name], after[name]), name
        sens = torch.zeros(b.n, nm.nsensordata, dtype=torch.float64, device=b.device)
        flags = torch.zeros(b.n, dtype=torch.int32, device=b.device)
        touch = torch.zeros(b.n, dtype=torch.int32, device=b.device)
        b.step(7, sens=sens, flags=flags, touch=touch)
        outs.append((sens, flags, touch, b.get_state()))
    assert _same_bits(outs[0][0], outs[1][0])
    assert torch.equal(outs[0][1], outs[1][1]) and torch.equal(outs[0][2], outs[1][2])
    for name in outs[0][3]:
        assert _same_bits(outs[0][3][name], outs[1][3][name]), name


# ---- 4. errors ----
def test_refusals_write_nothing():
    """every SG_ERR_INVALID case (n_ids <= 0, an env id out of range, NULL ids with another count, frame_body and dir_body outside
    [-1, nbody), n_dirs < 0 and above 256, n_dirs > 0 with NULL dir, a direction that is not finite or of zero length) and every
    SG_ERR_MODEL case that a model can reach (no skin for the two skin calls, an open skin with shape given) under the entry point's
    own name, the outputs untouched; the open skin still gives its vertices and extents, a model without a skin its subtree rows.
    (The NULL batch and the builder's LDS limit: tests/test_shape_host.py -- no model within sg_get_velocities' 627 bodies and the
    skin's 256 vertices reaches 160 KB.)"""
    from softgrip_amd import native
    from softgrip_amd.native import _ptr
    torch = _torch()
    m, nm, b, skin = _batch("softbox_fix")
    _squeeze(b, 2, nsteps=2)
    nv, nb = len(skin["vert_body"]), m.nbody
    kw = dict(dtype=torch.float64, device=b.device)
    out = {n: torch.full((3, nv, 3), -7.5, **kw) for n in VERT}
    out.update({n: torch.full((3, nb, 3), -7.5, **kw) for n in SUB})
    out.update(shape=torch.full((3, 12), -7.5, **kw), lo=torch.full((3, 2), -7.5, **kw), hi=torch.full((3, 2), -7.5, **kw),
               lo_vert=torch.full((3, 2), -7, dtype=torch.int32, device=b.device), hi_vert=torch.full((3, 2), -7, dtype=torch.int32, device=b.device))
    L, s, g = b.L, b._stream(), lambda n: _ptr(out[n])  # noqa: E731
    i32 = lambda a: np.ascontiguousarray(a, np.int32).ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    f64 = lambda a: np.ascontiguousarray(a, np.float64).ctypes.data_as(C.c_void_p)  # noqa: E731
    two = np.array([[1.0, 0, 0], [0, 1, 0]])

    def vertices(ids=None, n=3, frame=-1):
        return L.sg_get_skin_vertices(b.ptr, ids, n, frame, g("pos"), g("vel"), g("local"), s)

    def shape(ids=None, n=3, nd=2, d=two, db=None, with_shape=True):
        return L.sg_get_shape(b.ptr, ids, n, nd, None if d is None else f64(d), None if db is None else i32(db), g("shape") if with_shape else None, g("lo"), g("hi"),
                              g("lo_vert"), g("hi_vert"), s)

    def subtree(ids=None, n=3):
        return L.sg_get_subtree(b.ptr, ids, n, g("com"), g("linvel"), g("angmom"), s)

    def refused(code, name, call, word):
        assert call() == code, (name, word)
        msg = L.sg_last_error()
        assert msg.startswith(name.encode() + b":") and word in msg, (name, msg)

    inv = native.SG_ERR_INVALID
    for name, fn in (("sg_get_skin_vertices", vertices), ("sg_get_shape", shape), ("sg_get_subtree", subtree)):
        refused(inv, name, lambda: fn(n=0), b"n_ids")
        refused(inv, name, lambda: fn(n=-2), b"n_ids")
        refused(inv, name, lambda: fn(ids=i32([0, 3]), n=2), b"env id 3 out of range")
        refused(inv, name, lambda: fn(ids=i32([-1]), n=1), b"env id -1 out of range")
        refused(inv, name, lambda: fn(n=2), b"env_ids == NULL")
    refused(inv, "sg_get_skin_vertices", lambda: vertices(frame=-2), b"frame_body")
    refused(inv, "sg_get_skin_vertices", lambda: vertices(frame=nb), b"frame_body")
    refused(inv, "sg_get_shape", lambda: shape(db=[0, nb]), b"direction 1")
    refused(inv, "sg_get_shape", lambda: shape(db=[-2, 0]), b"direction 0")
    refused(inv, "sg_get_shape", lambda: shape(nd=-1), b"n_dirs")
    refused(inv, "sg_get_shape", lambda: shape(nd=257, d=np.ones((257, 3))), b"n_dirs")
    refused(inv, "sg_get_shape", lambda: shape(d=None), b"null dir")
    refused(inv, "sg_get_shape", lambda: shape(d=[[1, 0, 0], [0, np.nan, 0]]), b"direction 1 is not finite")
    refused(inv, "sg_get_shape", lambda: shape(d=[[np.inf, 0, 0], [0, 1, 0]]), b"direction 0 is not finite")
    refused(inv, "sg_get_shape", lambda: shape(d=[[1, 0, 0], [0, 0, 0]]), b"direction 1 has zero length")
    # an open skin: the shape is refused, vertices and extents are not
    nm.set_skin(dict(skin, face=skin["face"][:-1]))
    refused(native.SG_ERR_MODEL, "sg_get_shape", shape, b"not closed")
    torch.cuda.synchronize()
    for n, x in out.items():
        assert bool((x == (-7 if x.dtype == torch.int32 else -7.5)).all()), n
    assert shape(with_shape=False) == 0 and vertices() == 0
    torch.cuda.synchronize()
    assert bool((out["shape"] == -7.5).all()) and bool((out["lo"] < out["hi"]).all()) and bool((out["pos"] != -7.5).all())
    for n in VERT + EXT:
        out[n].fill_(-7 if out[n].dtype == torch.int32 else -7.5)
    # no skin: the two skin calls are refused, the subtree rows are not
    nm.set_skin(None)
    refused(native.SG_ERR_MODEL, "sg_get_skin_vertices", vertices, b"no skin")
    refused(native.SG_ERR_MODEL, "sg_get_shape", shape, b"no skin")
    torch.cuda.synchronize()
    for n in VERT + EXT + ("shape",):
        assert bool((out[n] == (-7 if out[n].dtype == torch.int32 else -7.5)).all()), n
    assert subtree() == 0
    qpos, qvel = _state(b)
    SR.compare({n: out[n][1].cpu().numpy() for n in SUB}, SR.reference(m, None, qpos[1], qvel[1]), "no skin", skin=False)


def test_a_model_the_velocity_read_out_refuses_is_refused(tmp_path):
    """628 bodies, one past sg_get_velocities' limit: the three calls return SG_ERR_MODEL under their own names with that read-out's
    reason and write nothing"""
    from softgrip_amd import native
    from softgrip_amd.native import _ptr
    from test_gpu_dyn import MAXBODY, _padded, _padded_states, _state_batch
    torch = _torch()
    m = _padded(tmp_path, MAXBODY + 1)
    jids, tids = DR.sweep_ids(m)
    q, v, ks = _padded_states(m, tmp_path)
    b = _state_batch(m, q, v, ks, jids, tids)
    P, face = SR.tetrahedron()
    b.nmodel.set_skin(SR.skin_of([1, 2, 3, 4], P, face))
    x = torch.full((2, m.nbody, 3), -7.5, dtype=torch.float64, device=b.device)
    L, s = b.L, b._stream()
    calls = (("sg_get_skin_vertices", lambda: L.sg_get_skin_vertices(b.ptr, None, 2, -1, _ptr(x), None, None, s)),
             ("sg_get_shape", lambda: L.sg_get_shape(b.ptr, None, 2, 0, None, None, _ptr(x), None, None, None, None, s)),
             ("sg_get_subtree", lambda: L.sg_get_subtree(b.ptr, None, 2, _ptr(x), None, None, s)))
    for name, call in calls:
        assert call() == native.SG_ERR_MODEL, name
        msg = L.sg_last_error()
        assert msg.startswith(name.encode() + b":") and b"more than %d bodies" % MAXBODY in msg, (name, msg)
    torch.cuda.synchronize()
    assert bool((x == -7.5).all())


# ---- 5. ManEnv ----
def test_manenv_deformation_and_rollout():
    """ManEnv on softbox_fix, 3 envs, no skin attached beforehand (the composite's is attached by the first call): object_body() is 10;
    right after sg_set_state(qpos0) get_deformation() is zero to the array bound; rollout(shape_out=...) fills [n, T, 12 + 2 D] with
    get_shape() after every env step -- the bits of per-step calls in a second rollout of the same schedule -- and leaves the sensor
    block's bits as a rollout without it has them"""
    import softgrip_amd as sg
    torch = _torch()
    scene, T = "softbox_fix", 4
    env = sg.ManEnv(1, 7, [model_path(scene)], n_envs=3, check_scene=False, tendon_damper="explicit")
    env.set_stiffness_values(np.array(DR.KS))
    assert env.object_body() == 10
    m = env.model
    q0 = torch.tensor(np.tile(np.asarray(m.qpos0, np.float64), (3, 1)), device=env.env.device).contiguous()
    env.env.set_state(qpos=q0, qvel=torch.zeros(3, m.nv, dtype=torch.float64, device=env.env.device))
    dfm = env.get_deformation()
    rest = env.nmodel.skin_rest(10)
    assert dfm["disp"].shape == (3, len(rest), 3) and float(dfm["max_disp"].max()) <= SR.ARR * max(1.0, np.abs(rest).max())
    dirs, db = SR.directions(m, 3)
    sched = [np.array([-0.2, -0.2])] + [None] * (T - 1)
    plain, f0 = env.rollout(sched)
    block = torch.full((3, T, 12 + 2 * len(dirs)), -7.5, dtype=torch.float64, device=env.env.device)
    sens, f1 = env.rollout(sched, shape_out=block, shape_dirs=dirs, shape_dir_body=db)
    assert _same_bits(plain, sens) and int(f0.abs().sum()) == 0 and int(f1.abs().sum()) == 0
    assert bool(torch.isfinite(block).all()) and bool((block != -7.5).all())
    for t in range(T):
        env.rollout(sched[:t + 1])
        s = env.get_shape(dirs, db)
        assert _same_bits(block[:, t].contiguous(), torch.cat([s["shape"], s["lo"], s["hi"]], dim=1)), t
    dfm = env.get_deformation()
    assert float(dfm["max_disp"].min()) > 1e-6 and bool((dfm["disp"][torch.arange(3), dfm["max_vert"]].norm(dim=-1) == dfm["max_disp"]).all())
    sv = env.get_skin_vertices()
    assert _same_bits(sv["local"] - torch.from_numpy(rest).to(sv["local"].device), dfm["disp"])
    sub = env.get_subtree()
    assert sub["com"].shape == (3, m.nbody, 3)
