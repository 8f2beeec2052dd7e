"""Pose read-out (sg_get_poses) and the headless renderer (sg_render) on the GPU: poses against Model.kinematics(), images against the
NumPy caster (tests/render_ref.py) on the GPU's own poses, no side effects on the simulation, batch independence, flagged envs and the
dataset tool's frames."""
import os
import pickle

import numpy as np
import pytest

import render_ref as R
from helpers import model_path

import softgrip_amd as sg

pytestmark = pytest.mark.gpu

CASES = [("softbox", None), ("softbox_fix", "tree"), ("fourfinger_softball_fix", None), ("freeball_fix", None)]


def _batch(scene, n, pipeline=None, seed=0):
    import torch
    from softgrip_amd import native
    damper = "explicit" if scene.startswith("softbox") else "implicit"
    m = sg.load_model(model_path(scene), damper)
    nm = native.NativeModel(m)
    b = native.NativeBatch(nm, n, 0)
    if pipeline:
        b.set_pipeline(pipeline)
    b.reset(1)
    b.set_ctrl_broadcast(np.full(nm.nu, -0.2))
    return m, nm, b, torch


def _check_poses(m, b, ids):
    p = b.poses(ids)
    q = b.get_state()["qpos"].cpu().numpy()
    for k, e in enumerate(ids):
        kin = m.kinematics(q[e])
        gx, gm = R.geom_poses(m, q[e])
        assert np.abs(p["xpos"][k].cpu().numpy() - kin["xpos"]).max() < 1e-12
        assert np.abs(p["xquat"][k].cpu().numpy() - kin["xquat"]).max() < 1e-12
        assert np.abs(p["geom_xpos"][k].cpu().numpy() - gx).max() < 1e-12
        assert np.abs(p["geom_xmat"][k].cpu().numpy().reshape(-1, 3, 3) - gm).max() < 1e-12
    return p


@pytest.mark.parametrize("scene,pipeline", CASES)
def test_poses_match_python_kinematics(scene, pipeline):
    m, nm, b, torch = _batch(scene, 16, pipeline)
    ids = [5, 0, 15, 5, 3]     # unsorted, one env twice
    _check_poses(m, b, ids)
    for n in (20, 80):
        for _ in range(n):
            b.step(7)
        _check_poses(m, b, ids)
    p = b.poses()
    assert p["xpos"].shape == (16, m.nbody, 3) and p["geom_xmat"].shape == (16, m.ngeom, 9)


@pytest.mark.parametrize("scene,pipeline", CASES)
def test_images_match_numpy_caster(scene, pipeline):
    m, nm, b, torch = _batch(scene, 8, pipeline)
    for _ in range(20):
        b.step(7)
    cam = nm.default_camera()
    cats = R.categories(m)
    p = b.poses()
    for w, h in ((64, 64), (37, 53)):
        img = b.render(cam, None, w, h)
        assert img["rgb"].shape == (8, h, w, 3) and (img["rgba"][..., 3] == 255).all()
        for e in range(8):
            gx = p["geom_xpos"][e].cpu().numpy()
            gm = p["geom_xmat"][e].cpu().numpy().reshape(-1, 3, 3)
            ref = R.render(gx, gm, m.geom_type, m.geom_size, cats, cam, w, h)
            got = (img["depth"][e].cpu().numpy(), img["seg"][e].cpu().numpy(), img["rgb"][e].cpu().numpy())
            R.compare(ref, got, "%s env %d %dx%d" % (scene, e, w, h))


@pytest.mark.parametrize("scene,pipeline", [("softbox", None), ("softbox_fix", "tree")])
def test_no_side_effects_over_an_episode(scene, pipeline):
    """sensors and flags bit-identical over 200 env steps when poses and a render are taken after every step"""
    _, nm, a, torch = _batch(scene, 8, pipeline)
    _, _, b, _ = _batch(scene, 8, pipeline)
    sa = torch.zeros(8, nm.nsensordata, dtype=torch.float64, device=a.device)
    sb, fa, fb = sa.clone(), torch.zeros(8, dtype=torch.int32, device=a.device), torch.zeros(8, dtype=torch.int32, device=a.device)
    for t in range(200):
        a.step(7, sens=sa, flags=fa)
        b.step(7, sens=sb, flags=fb)
        a.poses([1, 3])
        a.render(None, [0, 2, 7], 48, 32)
        assert torch.equal(sa, sb) and torch.equal(fa, fb), t
    for k in ("qpos", "qvel", "act", "qacc_warmstart"):
        assert torch.equal(a.get_state()[k], b.get_state()[k]), k


def test_batch_independence_4096_envs():
    m, nm, b, torch = _batch("softbox", 4096)
    for _ in range(10):
        b.step(7)
    cam = nm.default_camera()
    allimg = b.render(cam, None, 32, 32)
    for e in np.random.RandomState(1).choice(4096, 16, replace=False):
        one = b.render(cam, [int(e)], 32, 32)
        for k in ("rgba", "depth", "seg"):
            assert torch.equal(one[k][0], allimg[k][e]), (e, k)


def test_flagged_env_renders_as_background():
    m, nm, b, torch = _batch("softbox", 4)
    for _ in range(5):
        b.step(7)
    before = b.render(None, None, 40, 24)
    st = b.get_state()
    q = st["qpos"].clone()
    q[2, 7] = float("nan")
    b.set_state(qpos=q)
    after = b.render(None, None, 40, 24)
    assert (after["seg"][2] == -1).all() and torch.isinf(after["depth"][2]).all()
    bg = [int(np.floor(np.float32(c) * np.float32(255) + np.float32(0.5))) for c in R.BACKGROUND]     # (the kernel's fp32 rounding)
    assert (after["rgb"][2] == torch.tensor(bg, dtype=torch.uint8, device=b.device)).all()
    for e in (0, 1, 3):
        for k in ("rgba", "depth", "seg"):
            assert torch.equal(before[k][e], after[k][e])
    p = b.poses([2, 1])
    assert torch.isnan(p["xpos"][0]).all() and torch.isnan(p["geom_xmat"][0]).all() and torch.isfinite(p["xpos"][1]).all()


def test_bad_arguments():
    from softgrip_amd import native
    m, nm, b, torch = _batch("softbox", 4)
    with pytest.raises(native.SoftgripError) as e:
        b.render(None, [0, 4], 8, 8)
    assert e.value.code == native.SG_ERR_INVALID and "sg_render" in str(e.value)
    with pytest.raises(native.SoftgripError) as e:
        b.poses([-1])
    assert e.value.code == native.SG_ERR_INVALID and "sg_get_poses" in str(e.value)


def test_dataset_tool_frames_leave_the_data_alone(tmp_path):
    from softgrip_amd import create_dataset
    base = ["--mujoco-model-paths", model_path("softbox"), "--n-envs", "16", "--seed", "3", "--data-name", "d"]
    create_dataset.main(base + ["--data-folder", str(tmp_path / "a")])
    create_dataset.main(base + ["--data-folder", str(tmp_path / "b"), "--render-dir", str(tmp_path / "frames"), "--render-envs", "2",
                                "--render-size", "48", "36", "--render-every", "40"])
    pa, pb = (open(tmp_path / x / "d.pickle", "rb").read() for x in ("a", "b"))
    assert pa == pb
    frames = sorted(os.listdir(tmp_path / "frames" / "d"))
    assert frames == sorted("s0_b0_e%d_t%d.png" % (e, t) for e in (0, 1) for t in (0, 40, 80, 120)), frames
    data = open(tmp_path / "frames" / "d" / frames[0], "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n" and tuple(np.frombuffer(data[16:24], ">u4")) == (48, 36)
    assert pickle.loads(pa)["stiffness"]
