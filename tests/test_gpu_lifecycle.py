"""Life cycle of a batch's device memory through the C ABI: a creation that cannot be granted fails cleanly, create / use everything /
destroy repeats bit for bit, a pipeline's buffers allocated late compute what those allocated at creation do, and the read-outs' env
lists grow and are reused without changing a row."""
import math

import numpy as np
import pytest

import softgrip_amd as sg
from helpers import JOINT_IDS, TENDON_IDS, model_path

pytestmark = pytest.mark.gpu


def _model(scene, damper=None):
    from softgrip_amd import native
    return native.NativeModel(sg.load_model(model_path(scene), damper))


def _host(d):
    return {k: v.cpu().numpy().copy() for k, v in d.items()}


def _run(b, nsteps, out, tag):
    """nsteps env steps; the sensors, flags and touch bits after each go to out[tag + step]"""
    import torch
    n = b.n
    sens = torch.zeros(n, b.nmodel.nsensordata, dtype=torch.float64, device=b.device)
    flags = torch.zeros(n, dtype=torch.int32, device=b.device)
    touch = torch.zeros(n, dtype=torch.int32, device=b.device)
    for t in range(nsteps):
        b.step(7, sens=sens, flags=flags, touch=touch)
        out.update({"%s%d_%s" % (tag, t, k): v.cpu().numpy().copy() for k, v in (("sens", sens), ("flags", flags), ("touch", touch))})


def _start(nm, ks, jids, tids, prepare=None):
    """a fresh batch (after prepare(batch), if given) through set_stiffness, reset and 3 steps -> (batch, what it computed on the way)"""
    import torch
    from softgrip_amd import native
    b = native.NativeBatch(nm, len(ks), 0)
    if prepare:
        prepare(b)
    b.set_stiffness(np.asarray(ks, dtype=np.float64), jids, tids)
    sens = torch.zeros(len(ks), nm.nsensordata, dtype=torch.float64, device=b.device)
    b.reset(1, sens=sens)
    out = {"reset_sens": sens.cpu().numpy().copy()}
    b.set_ctrl_broadcast(np.full(nm.nu, -0.2))
    _run(b, 3, out, "step")
    return b, out


def _assert_same(got, want, what):
    assert sorted(got) == sorted(want)
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg="%s: %s" % (what, k))


def test_allocation_failure_at_creation_is_clean():
    import torch
    from softgrip_amd import native
    nm = _model("softbox_fix")
    ks = np.linspace(400, 1300, 4)
    ref, want = _start(nm, ks, JOINT_IDS, TENDON_IDS)      # (alive across the failed call)
    total = torch.cuda.mem_get_info()[1]
    n = 2 * math.ceil(total / (8 * nm.nq))     # qpos, the first per-env array, alone asks for twice the card: refused, nothing written
    with pytest.raises(native.SoftgripError) as e:
        native.NativeBatch(nm, n, 0)
    assert e.value.code == native.SG_ERR_NOMEM, e.value
    b, got = _start(nm, ks, JOINT_IDS, TENDON_IDS)
    _assert_same(got, want, "after the failed creation")
    assert int(np.abs(got["step2_flags"]).sum()) == 0 and np.abs(got["step2_sens"]).max() > 0


@pytest.mark.parametrize("scene,damper,n,jids,tids,switch", [("softbox_fix", None, 4, JOINT_IDS, TENDON_IDS, True),
                                                            ("fourfinger_softball_fix", "implicit", 2, list(range(65, 283)), [0], False)])
def test_create_use_everything_destroy_repeats_bit_for_bit(scene, damper, n, jids, tids, switch):
    """three batches of one model, one after the other, each through every entry point that allocates (the pose, contact and render
    read-outs, the tree pipeline's group when it is selected late); `switch`: the model also runs on the rows pipeline"""
    nm = _model(scene, damper)
    ks = np.linspace(400, 1300, n)
    first = None
    for cycle in range(3):
        b, out = _start(nm, ks, jids, tids)
        out.update({"poses_" + k: v for k, v in _host(b.poses()).items()})
        out.update({"contacts_" + k: v for k, v in _host(b.contacts()).items()})
        out.update({"render_" + k: v for k, v in _host(b.render(width=32, height=24)).items()})
        if switch:
            b.set_pipeline("tree")
            _run(b, 2, out, "tree")
            b.set_pipeline("rows")
            _run(b, 1, out, "rows")
        out["touch_words"] = b.touch_words().cpu().numpy().copy()
        out.update({"state_" + k: v for k, v in _host(b.get_state()).items()})
        del b      # sg_batch_destroy
        if first is None:
            first = out
            assert np.abs(out["step2_sens"]).max() > 0 and (out["contacts_ncon"] >= 0).all() and (out["render_seg"] >= 0).any()
        else:
            _assert_same(out, first, "cycle %d" % (cycle + 1))


def _everything(b, out, tag):
    out.update({"%s_%s" % (tag, k): v for k, v in _host(b.solver_stats()).items()})
    out.update({"%s_state_%s" % (tag, k): v for k, v in _host(b.get_state()).items()})
    out[tag + "_touch_words"] = b.touch_words().cpu().numpy().copy()


@pytest.mark.parametrize("scene", ["softbox_fix", "softbox"])
def test_rows_pipeline_allocated_late_gives_the_same_bits(scene, monkeypatch):
    """a batch that starts on the tree pipeline holds no rows work space (rows_alloc); switched to the rows pipeline it allocates it then
    and computes what a batch created on the rows pipeline does.  9 envs: two 8-env row blocks, three 4-env solver wavefronts, the last ragged"""
    nm = _model(scene)
    ks = np.linspace(400, 1300, 9)
    monkeypatch.delenv("SG_PIPELINE", raising=False)
    x, want = _start(nm, ks, JOINT_IDS, TENDON_IDS)
    assert x.tree_workgroups_per_cu() == 0      # (created plainly: on the rows pipeline, nothing of the tree pipeline allocated)
    monkeypatch.setenv("SG_PIPELINE", "tree")
    started_on_tree = []

    def to_rows(b):
        started_on_tree.append(b.tree_workgroups_per_cu() > 0)
        b.set_pipeline("rows")

    y, got = _start(nm, ks, JOINT_IDS, TENDON_IDS, prepare=to_rows)
    monkeypatch.delenv("SG_PIPELINE")
    if not started_on_tree[0]:
        assert scene == "softbox"
        pytest.skip("the model has no tree plan: SG_PIPELINE=tree does not apply to it")
    _everything(x, want, "rows")
    _everything(y, got, "rows")
    _assert_same(got, want, "rows pipeline allocated by sg_set_pipeline")
    assert int(np.abs(want["step2_flags"]).sum()) == 0 and np.abs(want["step2_sens"]).max() > 0 and want["rows_iters"].max() > 0
    for b, out in ((x, want), (y, got)):
        b.set_pipeline("tree")
        _run(b, 2, out, "tree")
        _everything(b, out, "tree")
    _assert_same(got, want, "back on the tree pipeline")
    assert np.abs(want["tree1_sens"]).max() > 0


@pytest.mark.parametrize("readout", ["poses", "contacts", "render"])
def test_env_lists_grow_and_are_reused(readout):
    """[2], then [0, 1, 3] (the id buffer and the per-env scratch grow), then [3, 1] (reused as they are): every row is the env's row of
    the all-env call"""
    nm = _model("softbox_fix")
    b, _ = _start(nm, np.linspace(400, 1300, 4), JOINT_IDS, TENDON_IDS)
    call = {"poses": b.poses, "contacts": b.contacts, "render": lambda env_ids=None: b.render(env_ids=env_ids, width=32, height=24)}[readout]
    full = _host(call())
    for ids in ([2], [0, 1, 3], [3, 1]):
        sub = _host(call(env_ids=ids))
        assert sorted(sub) == sorted(full)
        for k in full:
            np.testing.assert_array_equal(sub[k], full[k][ids], err_msg="%s %s %s" % (readout, k, ids))
