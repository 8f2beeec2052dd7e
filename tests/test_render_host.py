"""Headless renderer and pose read-out without a GPU: the g++ build of csrc/sg_render.h against the independent NumPy caster
(tests/render_ref.py), analytic known answers, the Python forward kinematics against the oracle, the default camera, the new ABI
entry points that need no device, the kept assembly of the new kernels and the PNG writer."""
import ctypes as C
import os
import re
import zlib

import numpy as np
import pytest

import render_ref as R
from helpers import ROOT, model_path

import softgrip_amd as sg

SCENES = ["softbox", "softcylinder", "softball", "freeball", "fourfinger_softball"]
ALL_MODELS = sorted(f[:-8] for f in os.listdir(os.path.join(ROOT, "models")) if f.endswith(".sgmodel"))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return R.build_host(str(tmp_path_factory.mktemp("render_host")))


def perturbed(model, seed):
    """qpos0 moved: hinges +-0.3 rad, sliders +-2 cm, a free body shifted and turned"""
    rs = np.random.RandomState(seed)
    q = np.array(model.qpos0, dtype=np.float64)
    for j, t in enumerate(model.jnt_type):
        a = model.jnt_qposadr[j]
        if t == 3:
            q[a] += rs.uniform(-0.3, 0.3)
        elif t == 2:
            q[a] += rs.uniform(-0.02, 0.02)
        else:
            q[a:a + 3] += rs.uniform(-0.05, 0.05, 3)
            q[a + 3:a + 7] += rs.uniform(-0.2, 0.2, 4)
    return q


def side_camera(model):
    c = R.default_camera(model)
    c[4], c[5] = 180.0, -25.0
    return c


@pytest.mark.parametrize("scene", SCENES)
def test_host_build_matches_numpy_caster(host, scene):
    m = sg.load_model(model_path(scene))
    cats = R.categories(m)
    for k, q in enumerate([m.qpos0] + [perturbed(m, s) for s in range(3)]):
        gx, gm = R.geom_poses(m, q)
        for cam in (R.default_camera(m), side_camera(m)):
            for w, h in ((64, 64), (37, 53)):
                ref = R.render(gx, gm, m.geom_type, m.geom_size, cats, cam, w, h)
                d, s, rgba = R.render_with(host, gx, gm, m.geom_type, m.geom_size, cats, cam, w, h)
                assert (rgba[..., 3] == 255).all()
                R.compare(ref, (d, s, rgba[..., :3]), "%s state %d cam %s %dx%d" % (scene, k, cam[4:6], w, h))
                assert (s >= 0).mean() > 0.5        # (the pictures are not empty)


def _single(type_, size, pos=(0.0, 0.0, 0.0)):
    gx = np.array([pos], dtype=np.float64)
    gm = np.eye(3)[None]
    return gx, gm, np.array([type_]), np.array([size], dtype=np.float64), np.array([R.STATIC])


@pytest.mark.parametrize("case", ["sphere", "capsule", "box", "plane"])
def test_known_answers_at_the_centre_pixel(host, case):
    """a primitive straight ahead: the centre pixel's depth is the analytic one (odd image size: a pixel sits on the optical axis)"""
    W = H = 33
    if case == "plane":    # camera 2 m above the ground looking straight down
        gx, gm, ty, sz, ct = _single(R.PLANE, (0, 0, 1))
        cam = np.array([0.0, 0.0, 0.0, 2.0, 90.0, -90.0, 45.0])
        want = 2.0
    else:                  # camera on the -y side at 3 m from the origin, looking along +y
        spec = {"sphere": (R.SPHERE, (0.25, 0, 0), 3.0 - 0.25), "capsule": (R.CAPSULE, (0.1, 0.3, 0), 3.0 - 0.1),
                "box": (R.BOX, (0.2, 0.15, 0.1), 3.0 - 0.15)}[case]
        gx, gm, ty, sz, ct = _single(spec[0], spec[1])
        cam = np.array([0.0, 0.0, 0.0, 3.0, 90.0, 0.0, 45.0])
        want = spec[2]
    d, s, _ = R.render_with(host, gx, gm, ty, sz, ct, cam, W, H)
    assert s[H // 2, W // 2] == 0
    assert abs(d[H // 2, W // 2] - want) < 1e-6, (case, d[H // 2, W // 2], want)
    rd, rs = R.render(gx, gm, ty, sz, ct, cam, W, H)[:2]
    assert abs(rd[H // 2, W // 2] - want) < 1e-12


@pytest.mark.parametrize("scene", ["softbox", "freeball_fix", "fourfinger_softball_fix"])
def test_python_kinematics_matches_oracle_site_positions(scene):
    """Model.kinematics() + site_pos reproduce the oracle's site_xpos after 20 env steps of the squeeze schedule"""
    from oracle import oracle as O
    m = sg.load_model(model_path(scene), "explicit" if scene == "softbox" else "implicit")   # (the ball scenes need D5)
    om = O.OracleModel(m.to_blob())
    sim = O.OracleSim(om)
    sim.reset(); sim.forward(); sim.step()
    sim.ctrl[:] = -0.2
    for _ in range(20 * 7):
        assert sim.step() == 0
    sim.forward()     # site_xpos of the current qpos
    L = O.lib()
    got = np.ctypeslib.as_array(L.sgo_site_xpos(sim.ptr), shape=(m.nsite, 3)).copy()
    kin = m.kinematics(sim.qpos.copy())
    ref = m.site_xpos(kin)
    assert np.abs(ref - got).max() < 1e-12, np.abs(ref - got).max()
    assert np.abs(sim.qpos - m.qpos0).max() > 1e-4        # (the state did move)


@pytest.mark.parametrize("name", ALL_MODELS)
def test_default_camera_frames_object_and_fingers(name):
    from softgrip_amd import native
    m = sg.load_model(model_path(name))
    cam = R.default_camera(m)
    cats = R.categories(m)
    seg = R.render_model(m, m.qpos0, cam, 128, 128, cats)[1]
    obj = np.isin(seg, np.flatnonzero((cats == R.ELEM) | (cats == R.CENTER)))
    fing = np.isin(seg, np.flatnonzero(cats == R.FINGER))
    assert obj.mean() >= 0.03, obj.mean()
    border = np.zeros_like(obj)
    border[0] = border[-1] = border[:, 0] = border[:, -1] = True
    assert not (obj | fing)[border].any()
    if os.path.exists(native.LIB_PATH):
        np.testing.assert_allclose(native.NativeModel(m).default_camera(), cam, rtol=1e-12, atol=1e-12)


def test_abi_entry_points_without_a_device():
    from softgrip_amd import native
    with open(os.path.join(ROOT, "include", "softgrip.h")) as f:
        declared = set(re.findall(r"(sg_[a-z_]+)\s*\(", f.read()))
    new = {"sg_get_poses", "sg_model_nbody", "sg_model_ngeom", "sg_model_default_camera", "sg_render"}
    assert new <= declared and new <= set(native.SYMBOLS)
    L = native.lib()
    for s in new:
        assert hasattr(L, s)
    cam = (C.c_double * 7)(0, 0, 0, 1, 90, -30, 45)
    assert L.sg_render(None, cam, None, 1, 8, 8, None, None, None, None) == native.SG_ERR_INVALID
    assert b"sg_render" in L.sg_last_error()
    assert L.sg_get_poses(None, None, 1, None, None, None, None, None) == native.SG_ERR_INVALID
    assert b"sg_get_poses" in L.sg_last_error()
    assert L.sg_model_default_camera(None, cam) == native.SG_ERR_INVALID
    for name in ("softbox", "fourfinger_softball"):
        m = sg.load_model(model_path(name))
        nm = native.NativeModel(m)
        assert (nm.nbody, nm.ngeom) == (m.nbody, m.ngeom)
        np.testing.assert_allclose(nm.default_camera(), R.default_camera(m), rtol=1e-12, atol=1e-12)


def test_new_kernels_have_no_scratch_and_no_spills():
    """the kept assembly (sg_readout.device.s: sg_kin_kernels.h is compiled inside sg_readout.hip): both kernels 0 bytes of scratch and no VGPR spills, the render
    kernel at least 4 waves per SIMD by its registers (<= 128) and its LDS (4 waves of 256-lane workgroups per SIMD = 4 per CU)"""
    from softgrip_amd import build_native, devasm
    build_native.build()
    api = build_native.device_asm("sg_readout.hip")
    seen = devasm.kernels(open(api).read())
    kin = [v for k, v in seen.items() if "sg_kin_kernel" in k]
    ren = [v for k, v in seen.items() if "sg_render_kernel" in k]
    assert len(kin) == 1 and len(ren) == 1, sorted(seen)
    for v in kin + ren:
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0, v
    assert ren[0]["vgpr"] + ren[0]["agpr"] <= 128, ren[0]
    assert 4 * ren[0]["lds"] <= 160 * 1024, ren[0]


def test_png_writer_round_trips():
    from softgrip_amd import pngio
    rs = np.random.RandomState(3)
    for shape in ((7, 5, 3), (16, 9, 4), (1, 1, 3)):
        img = rs.randint(0, 256, shape).astype(np.uint8)
        data = pngio.encode_png(img)
        assert data[:8] == b"\x89PNG\r\n\x1a\n"
        w, h = np.frombuffer(data[16:24], ">u4")
        assert (w, h) == (shape[1], shape[0])
        idat = b""
        pos = 8
        while pos < len(data):
            n = int.from_bytes(data[pos:pos + 4], "big")
            tag = data[pos + 4:pos + 8]
            chunk = data[pos + 8:pos + 8 + n]
            assert zlib.crc32(tag + chunk) == int.from_bytes(data[pos + 8 + n:pos + 12 + n], "big")
            if tag == b"IDAT":
                idat += chunk
            pos += 12 + n
        raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(shape[0], 1 + shape[1] * shape[2])
        assert (raw[:, 0] == 0).all()
        np.testing.assert_array_equal(raw[:, 1:].reshape(shape), img)
