"""The soft object's skin on the GPU (sg_render_ex, SG_RENDER_SKIN): the plain path bit for bit, skin images against the NumPy caster
(tests/skin_ref.py) on the GPU's own poses, flagged envs, no side effects on the simulation, a skin replaced under a live batch and the
dataset tool's --render-skin."""
import ctypes as C
import os

import numpy as np
import pytest

import render_ref as R
import skin_ref as S
from helpers import ROOT, model_path

import softgrip_amd as sg
from softgrip_amd.mjcf import quat_to_mat

pytestmark = pytest.mark.gpu

# scene, pipeline (None: the model's default), where the skin comes from
CASES = [("skin_ball", None, "xml"), ("skin_box", None, "xml"), ("softball_fix", "rows", "names"), ("softbox_fix", "tree", "names"),
         ("fourfinger_softball_fix", None, "names"), ("freeball_fix", None, "names")]


def _batch(scene, n, pipeline=None, attach=True):
    import torch
    from softgrip_amd import native
    if scene.startswith("skin_"):
        m = sg.compile_mjcf(os.path.join(ROOT, "tests", "data", "skin", scene + ".xml"))
    else:
        m = sg.load_model(model_path(scene), "explicit" if scene.startswith("softbox") else "implicit")
    nm = native.NativeModel(m)
    if attach and nm.skin() is None:
        nm.set_skin(m.composite_skin())
    b = native.NativeBatch(nm, n, 0)
    if pipeline:
        b.set_pipeline(pipeline)
    b.reset(1)
    b.set_ctrl_broadcast(np.full(nm.nu, -0.2))
    return m, nm, b, torch


def _render_ex(b, cam, ids, w, h, flags):
    """sg_render_ex itself (NativeBatch.render(skin=True) would attach a skin first)"""
    t = b.torch
    ia = None if ids is None else np.ascontiguousarray(ids, dtype=np.int32)
    k = b.n if ids is None else len(ia)
    cam = np.ascontiguousarray(cam, dtype=np.float64)
    out = dict(rgba=t.zeros(k, h, w, 4, dtype=t.uint8, device=b.device), depth=t.zeros(k, h, w, dtype=t.float32, device=b.device),
               seg=t.zeros(k, h, w, dtype=t.int32, device=b.device))
    b._check(b.L.sg_render_ex(b.ptr, cam.ctypes.data_as(C.POINTER(C.c_double)), None if ia is None else ia.ctypes.data_as(C.POINTER(C.c_int32)), k,
                              w, h, flags, C.c_void_p(out["rgba"].data_ptr()), C.c_void_p(out["depth"].data_ptr()),
                              C.c_void_p(out["seg"].data_ptr()), b._stream()))
    return out


def _reference(m, skin, poses, k, cam, w, h):
    xpos = poses["xpos"][k].cpu().numpy()
    xmat = np.array([quat_to_mat(q) for q in poses["xquat"][k].cpu().numpy()])
    gx = poses["geom_xpos"][k].cpu().numpy()
    gm = poses["geom_xmat"][k].cpu().numpy().reshape(-1, 3, 3)
    return S.render(gx, gm, m.geom_type, m.geom_size, R.categories(m), cam, w, h, S.skin_vertices(skin, xpos, xmat), skin["face"], skin["rgba"],
                    S.hidden_geoms(m, skin))


def _check_images(m, nm, b, ids, tag):
    skin = nm.skin()
    hidden = np.flatnonzero(S.hidden_geoms(m, skin))
    cam = nm.default_camera()
    poses = b.poses(ids)
    for w, h in ((64, 64), (37, 53)):
        img = b.render(cam, ids, w, h, skin=True)
        assert (img["rgba"][..., 3] == 255).all()
        seg_all = img["seg"].cpu().numpy()
        assert not np.isin(seg_all, hidden).any() and (seg_all == m.ngeom).any() and seg_all.max() == m.ngeom
        first = {}
        for k, e in enumerate(ids):
            if e in first:         # the env listed twice: the same picture, bit for bit
                for name in ("rgba", "depth", "seg"):
                    assert b.torch.equal(img[name][k], img[name][first[e]]), (tag, name)
                continue
            first[e] = k
            ref = _reference(m, skin, poses, k, cam, w, h)
            got = (img["depth"][k].cpu().numpy(), seg_all[k], img["rgb"][k].cpu().numpy())
            S.compare(ref, got, skin["face"], "%s env %d %dx%d" % (tag, e, w, h))
            assert ((ref[1] == m.ngeom).mean() > 0.01)


@pytest.mark.parametrize("scene,pipeline,source", CASES)
def test_skin_images_match_numpy_caster(scene, pipeline, source):
    m, nm, b, torch = _batch(scene, 6, pipeline)
    assert (m.skin is not None) == (source == "xml")
    ids = [5, 0, 5]      # unsorted, one env twice
    _check_images(m, nm, b, ids, scene + " at reset")
    for _ in range(20):
        b.step(7)
    _check_images(m, nm, b, ids, scene + " squeezed")


def test_flags_zero_and_a_model_without_skin_are_the_plain_renderer():
    from softgrip_amd import native
    m, nm, b, torch = _batch("softbox", 8, attach=False)
    for _ in range(20):
        b.step(7)
    cam = nm.default_camera()
    ids = [6, 1, 3]
    for w, h in ((64, 64), (37, 53)):
        plain = b.render(cam, ids, w, h)
        assert nm.skin() is None
        for flags in (0, native.SG_RENDER_SKIN):
            ex = _render_ex(b, cam, ids, w, h, flags)
            for k in ("rgba", "depth", "seg"):
                assert torch.equal(ex[k], plain[k]), (flags, k)
    nm.set_skin(m.composite_skin())
    ex = _render_ex(b, cam, ids, 64, 64, 0)         # a skin attached, the flag not given: still the plain picture
    plain = b.render(cam, ids, 64, 64)
    for k in ("rgba", "depth", "seg"):
        assert torch.equal(ex[k], plain[k]), k
    assert (_render_ex(b, cam, ids, 64, 64, native.SG_RENDER_SKIN)["seg"] == m.ngeom).any()
    with pytest.raises(native.SoftgripError) as e:
        _render_ex(b, cam, ids, 8, 8, 4)
    assert e.value.code == native.SG_ERR_INVALID


def test_flagged_env_renders_as_background_with_the_skin():
    m, nm, b, torch = _batch("skin_ball", 4)
    for _ in range(5):
        b.step(7)
    before = b.render(None, None, 40, 24, skin=True)
    q = b.get_state()["qpos"].clone()
    q[2, 7] = float("nan")
    b.set_state(qpos=q)
    after = b.render(None, None, 40, 24, skin=True)
    assert (after["seg"][2] == -1).all() and torch.isinf(after["depth"][2]).all()
    bg = [int(np.floor(np.float32(c) * np.float32(255) + np.float32(0.5))) for c in R.BACKGROUND]
    assert (after["rgb"][2] == torch.tensor(bg, dtype=torch.uint8, device=b.device)).all()
    for e in (0, 1, 3):
        for k in ("rgba", "depth", "seg"):
            assert torch.equal(before[k][e], after[k][e])
        assert (after["seg"][e] == m.ngeom).any()


@pytest.mark.parametrize("scene,pipeline", [("skin_box", None), ("softbox_fix", "tree")])
def test_skin_render_has_no_side_effects(scene, pipeline):
    """sensors, flags and state bit-identical over 40 env steps when a skin render is taken after every step"""
    _, nm, a, torch = _batch(scene, 4, pipeline)
    _, _, b, _ = _batch(scene, 4, pipeline)
    sa = torch.zeros(4, nm.nsensordata, dtype=torch.float64, device=a.device)
    sb, fa, fb = sa.clone(), torch.zeros(4, dtype=torch.int32, device=a.device), torch.zeros(4, dtype=torch.int32, device=a.device)
    for t in range(40):
        a.step(7, sens=sa, flags=fa)
        b.step(7, sens=sb, flags=fb)
        a.render(None, [3, 0], 48, 32, skin=True)
        assert torch.equal(sa, sb) and torch.equal(fa, fb), t
    for k in ("qpos", "qvel", "act", "qacc_warmstart", "ctrl"):
        assert torch.equal(a.get_state()[k], b.get_state()[k]), k


def test_a_new_skin_shows_in_the_next_render():
    """set_skin on a model whose batch has already rendered (the version counter): the picture follows, and removing the skin gives the
    plain picture back"""
    m, nm, b, torch = _batch("skin_box", 4)
    for _ in range(10):
        b.step(7)
    cam = nm.default_camera()
    ids = [2, 1]
    old = b.render(cam, ids, 64, 64, skin=True)
    new = dict(m.skin)
    new["vert_pos"] = m.skin["vert_pos"] + np.array([0.0, 0.0, 0.05])
    new["rgba"] = np.array([0.1, 0.3, 0.9, 1.0], np.float32)
    new["face"] = m.skin["face"][4:]          # (a hole: another face count too)
    nm.set_skin(new)
    img = b.render(cam, ids, 64, 64, skin=True)
    assert not torch.equal(img["rgba"], old["rgba"]) and not torch.equal(img["depth"], old["depth"])
    poses = b.poses(ids)
    for k in range(2):
        ref = _reference(m, new, poses, k, cam, 64, 64)
        S.compare(ref, (img["depth"][k].cpu().numpy(), img["seg"][k].cpu().numpy(), img["rgb"][k].cpu().numpy()), new["face"], "new skin env %d" % ids[k])
    nm.set_skin(None)
    plain = b.render(cam, ids, 64, 64)
    gone = _render_ex(b, cam, ids, 64, 64, 1)
    for k in ("rgba", "depth", "seg"):
        assert torch.equal(gone[k], plain[k]), k
    nm.set_skin(m.skin)
    back = b.render(cam, ids, 64, 64, skin=True)
    for k in ("rgba", "depth", "seg"):
        assert torch.equal(back[k], old[k]), k


def test_dataset_tool_render_skin_changes_the_frames_only(tmp_path):
    from softgrip_amd import create_dataset
    base = ["--mujoco-model-paths", model_path("softbox"), "--n-envs", "16", "--seed", "3", "--data-name", "d", "--render-envs", "1",
            "--render-size", "48", "36", "--render-every", "60"]
    create_dataset.main(base + ["--data-folder", str(tmp_path / "a"), "--render-dir", str(tmp_path / "fa")])
    create_dataset.main(base + ["--data-folder", str(tmp_path / "b"), "--render-dir", str(tmp_path / "fb"), "--render-skin"])
    pa, pb = (open(tmp_path / x / "d.pickle", "rb").read() for x in ("a", "b"))
    assert pa == pb
    fa, fb = (sorted(os.listdir(tmp_path / x / "d")) for x in ("fa", "fb"))
    assert fa == fb and len(fa) >= 2
    assert any(open(tmp_path / "fa" / "d" / f, "rb").read() != open(tmp_path / "fb" / "d" / f, "rb").read() for f in fa)
