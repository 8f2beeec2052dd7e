"""sg_get_contacts on the GPU: the contact list of the current state against the oracle's forward(); contacts() along whole squeeze
episodes and over a pose sweep of random grippers (every pair type, every box - box branch, the queue's carry, the model's cap, the
kernel that keeps its poses in global memory), the call's interface (env subsets, truncation, NaN envs, NULL outputs, no side effect on
a following step), agreement with the touch bits where nothing lies between the two, and ManEnv.get_contacts."""
import ctypes as C

import numpy as np
import pytest

import contacts_ref as CR
import softgrip_amd as sg
from helpers import JOINT_IDS, model_path, oracle_sim
from softgrip_amd.create_dataset import episode_schedule

pytestmark = pytest.mark.gpu

# scene -> (tendon damper, joints / tendons that take the stiffness, actuators)
SCENES = {"softbox": (None, JOINT_IDS, [0], 2), "softball": ("implicit", JOINT_IDS, [0], 2), "softcylinder": ("implicit", JOINT_IDS, [0], 2),
          "fourfinger_softball_fix": ("implicit", list(range(65, 283)), [0], 4), "freeball_fix": ("implicit", list(range(9, 227)), [0], 2)}
MAXC = 256


def _torch():
    import torch
    return torch


def _batch(model, ks, jids, tids, pipeline=None):
    from softgrip_amd import native
    torch = _torch()
    nm = native.NativeModel(model)
    b = native.NativeBatch(nm, len(ks), 0)
    if pipeline:
        b.set_pipeline(pipeline)
    b.set_stiffness(np.asarray(ks, dtype=np.float64), jids, tids)
    sens = torch.zeros(len(ks), nm.nsensordata, dtype=torch.float64, device=b.device)
    flags = torch.zeros(len(ks), dtype=torch.int32, device=b.device)
    touch = torch.zeros(len(ks), dtype=torch.int32, device=b.device)
    return nm, b, sens, flags, touch


def _rows(out):
    """the device dict as per-env host lists in contacts_ref's layout"""
    h = {k: v.cpu().numpy() for k, v in out.items()}
    res = []
    for e in range(len(h["ncon"])):
        n = int(h["ncon"][e])
        k = max(0, min(n, h["geom"].shape[1]))
        res.append(dict(ncon=n, geom=h["geom"][e, :k], dist=h["dist"][e, :k], pos=h["pos"][e, :k], frame=h["frame"][e, :k]))
    return res


def _kinds(m, ref):
    """the pair types of a list, by name"""
    return {CR.PAIR_NAMES[int(m.geom_type[a]), int(m.geom_type[b])] for a, b in ref["geom"]}


@pytest.mark.parametrize("scene", sorted(SCENES))
def test_episode_lists_match_oracle(scene):
    """9 envs with k spread over U(300, 1400), the reference's 200-step schedule, free running; at the reset state and after every 10th
    env step the device's list of every env against the oracle's forward() on the device's qpos: counts and geom pairs exact, dist /
    pos / frame within 1e-9.  A sample may be left out only where the oracle's own list changes under a +-1e-12 perturbation of that
    qpos, and at most 2 % of a scene's samples."""
    damper, jids, tids, nu = SCENES[scene]
    m = sg.load_model(model_path(scene), damper)
    rs = np.random.RandomState(11)
    ks = rs.uniform(300, 1400, 9)
    nm, b, sens, flags, touch = _batch(m, ks, jids, tids)
    sim = oracle_sim(m)
    b.reset(1, sens=sens, flags=flags)
    samples = left_out = most = 0
    worst = 0.0
    kinds = set()

    def sample(t):
        nonlocal samples, left_out, most, worst
        qpos = b.get_state()["qpos"].cpu().numpy()
        got = _rows(b.contacts(max_contacts=MAXC))
        for e in range(len(ks)):
            if not np.isfinite(qpos[e]).all():
                assert got[e]["ncon"] == -1, (t, e)
                continue
            samples += 1
            ref = CR.oracle_contacts(sim, qpos[e])
            most = max(most, ref["ncon"])
            kinds.update(_kinds(m, ref))
            assert ref["ncon"] <= MAXC, (t, e, ref["ncon"])
            try:
                worst = max(worst, CR.compare(got[e], ref, "%s step %d env %d" % (scene, t, e)))
            except AssertionError:
                if not CR.knife_edge(sim, qpos[e], ref, rs):
                    raise
                left_out += 1

    sample(0)
    for t, c in enumerate(episode_schedule()):
        if c is not None:
            b.set_ctrl_broadcast(np.full(nu, c))
        b.step(7, sens=sens, flags=flags)
        if (t + 1) % 10 == 0:
            sample(t + 1)
    print("%s: %d samples, %d left out (knife edges), up to %d contacts, max deviation %.2e" % (scene, samples, left_out, most, worst))
    print("%s: pair types that produced contacts: %s" % (scene, ", ".join(sorted(kinds))))
    assert samples >= 9 * 21 * 0.9, samples
    assert most >= 10, most
    assert left_out <= 0.02 * samples, (left_out, samples)


def _call(b, ids, n_ids, mc, out):
    from softgrip_amd.native import _ptr
    arr = None if ids is None else np.ascontiguousarray(ids, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    return b.L.sg_get_contacts(b.ptr, arr, n_ids, mc, _ptr(out.get("ncon")), _ptr(out.get("geom")), _ptr(out.get("dist")), _ptr(out.get("pos")),
                               _ptr(out.get("frame")), b._stream())


def _canary(torch, b, k, mc, tail=64):
    """contact tensors [k, mc, ...] cut out of longer buffers filled with a canary value; -> (dict, {name: whole buffer})"""
    out, whole = {}, {}
    for name, w, dt, val in (("ncon", 0, torch.int32, -77), ("geom", 2, torch.int32, -77), ("dist", 1, torch.float64, -7.5), ("pos", 3, torch.float64, -7.5),
                             ("frame", 9, torch.float64, -7.5)):
        n = k if name == "ncon" else k * mc * w
        buf = torch.full((n + tail,), val, dtype=dt, device=b.device)
        whole[name] = buf
        shape = (k,) if name == "ncon" else ((k, mc) if w == 1 else (k, mc, w))
        out[name] = buf[:n].view(shape)
    return out, whole


def test_interface_behaviour():
    from softgrip_amd import native
    torch = _torch()
    m = sg.load_model(model_path("softball"), "implicit")
    ks = np.linspace(300, 1400, 6)
    nm, b, sens, flags, touch = _batch(m, ks, JOINT_IDS, [0])
    b.reset(1, sens=sens, flags=flags)
    b.set_ctrl_broadcast(np.full(2, -0.2))
    for _ in range(45):
        b.step(7, sens=sens, flags=flags)
    full = {k: v.cpu().numpy() for k, v in b.contacts(max_contacts=MAXC).items()}
    ncon = full["ncon"]
    assert (ncon >= 10).all() and (ncon <= MAXC).all() and len(set(ncon.tolist())) > 1, ncon
    # env subsets and permutations (with a repeat) give the rows of the all-env call
    for ids in ([4, 1, 1, 3], [5, 4, 3, 2, 1, 0], [2]):
        sub = {k: v.cpu().numpy() for k, v in b.contacts(env_ids=ids, max_contacts=MAXC).items()}
        for key in full:
            np.testing.assert_array_equal(sub[key], full[key][ids], err_msg="%s %s" % (key, ids))
    # truncation: the full count, the in-order prefix, nothing written past it (canary fill, also behind the tensors)
    for mc in (8, int(ncon.min()) + 1, int(ncon.max()) + 3):
        out, whole = _canary(torch, b, len(ks), mc)
        b.contacts_into(out)
        h = {k: v.cpu().numpy() for k, v in out.items()}
        np.testing.assert_array_equal(h["ncon"], ncon)
        for e in range(len(ks)):
            k = min(int(ncon[e]), mc)
            for key, val in (("geom", -77), ("dist", -7.5), ("pos", -7.5), ("frame", -7.5)):
                np.testing.assert_array_equal(h[key][e, :k], full[key][e, :k], err_msg="%s env %d mc %d" % (key, e, mc))
                assert (h[key][e, k:] == val).all(), (key, e, mc)
        for key, buf in whole.items():
            tail = buf[-64:].cpu().numpy()
            assert (tail == tail[0]).all() and tail[0] in (-77, -7.5), key
    # a NaN-poisoned env reports -1, its rows stay untouched, its neighbours are intact
    st = b.get_state()
    q = st["qpos"].clone()
    q[2, 17] = float("nan")
    q[4, 3] = float("inf")
    b.set_state(qpos=q)
    out, whole = _canary(torch, b, len(ks), MAXC)
    b.contacts_into(out)
    h = {k: v.cpu().numpy() for k, v in out.items()}
    assert h["ncon"][2] == -1 and h["ncon"][4] == -1
    for e in range(len(ks)):
        if e in (2, 4):
            assert (h["geom"][e] == -77).all() and (h["dist"][e] == -7.5).all() and (h["pos"][e] == -7.5).all() and (h["frame"][e] == -7.5).all()
        else:
            k = int(ncon[e])
            assert h["ncon"][e] == k
            for key in ("geom", "dist", "pos", "frame"):
                np.testing.assert_array_equal(h[key][e, :k], full[key][e, :k])
    b.set_state(qpos=st["qpos"])
    # all outputs NULL; only ncon; argument errors that need a batch
    assert _call(b, None, len(ks), 0, {}) == native.SG_OK
    only = {"ncon": torch.zeros(len(ks), dtype=torch.int32, device=b.device)}
    assert _call(b, None, len(ks), 0, only) == native.SG_OK
    np.testing.assert_array_equal(only["ncon"].cpu().numpy(), ncon)
    for ids, n in (([0, 6], 2), ([-1], 1), (None, 3)):
        assert _call(b, ids, n, 0, {}) == native.SG_ERR_INVALID, (ids, n)
        assert b"sg_get_contacts" in b.L.sg_last_error()
    assert _call(b, None, 0, 0, {}) == native.SG_ERR_INVALID
    assert _call(b, None, len(ks), 0, {"dist": torch.zeros(len(ks), 1, dtype=torch.float64, device=b.device)}) == native.SG_ERR_INVALID


# ---- the pose sweep of contacts_ref: random grippers turned far out of their joint ranges, one env per pose, nothing stepped ----
_SWEEP = {}      # gripper -> (model, poses [n, nq], the oracle's list per pose): computed once, shared, left unchanged
CAP_GRIPPER = 0          # (its longest list stays below the model's nconmax = 300: the sweep's lists of it are uncapped)
MANY_GEOMS_GRIPPER = 3   # (the gripper with the most broadphase survivors)
POSE_LDS_LIMIT = 159 * 1024    # sg_get_contacts keeps an env's poses in LDS up to here (35 328 B of staging + 8 (7 nbody + 12 ngeom))


def _compile(tmp_path, name, xml):
    path = tmp_path / name
    path.write_text(xml)
    return sg.compile_mjcf(str(path), composite_neighbors=False)


def _sweep(gripper, tmp_path):
    if gripper not in _SWEEP:
        m = _compile(tmp_path, "g%d.xml" % gripper, CR.sweep_gripper_xmls()[gripper])
        qs = CR.pose_sweep(m, CR.SWEEP_POSES, CR.SWEEP_POSE_SEED + gripper)
        sim = oracle_sim(m)
        _SWEEP[gripper] = (m, qs, [CR.oracle_contacts(sim, q) for q in qs])
    return _SWEEP[gripper]


def _pose_batch(m, qs):
    """a batch of the model's default pipeline with one env per pose: one sg_set_state, nothing stepped"""
    from softgrip_amd import native
    torch = _torch()
    b = native.NativeBatch(native.NativeModel(m), len(qs), 0)
    b.set_state(qpos=torch.tensor(np.ascontiguousarray(qs), dtype=torch.float64, device=b.device))
    return b


def _same_bits(a, b):
    for key in ("ncon", "geom", "dist", "pos", "frame"):
        assert a[key].cpu().numpy().tobytes() == b[key].cpu().numpy().tobytes(), key


@pytest.mark.parametrize("gripper", range(CR.SWEEP_GRIPPERS))
def test_pose_sweep_matches_oracle(gripper, tmp_path):
    """64 poses of a random gripper as 64 envs of one batch, one sg_set_state and one read-out: every env's list against the oracle's
    forward(); contacts() at that qpos, counts and geom pairs exact, dist / pos / frame within 1e-9.  What the poses reach -- every pair
    type, box - box contacts off a face of either box and off two edges with 1 to 7 records, more than 128 survivors in an env, up to
    47 box - box pairs among 64 survivors, a list cut by the model's nconmax -- is asserted on the CPU by
    tests/test_contacts_host.py::test_pose_sweep_of_random_grippers_matches_oracle.  A pose may be left out only where the device's
    list differs AND the oracle's own list changes under a +-1e-12 perturbation of that qpos, and at most one per gripper (2 % of 64)."""
    m, qs, refs = _sweep(gripper, tmp_path)
    b = _pose_batch(m, qs)
    out = b.contacts(max_contacts=512)
    _same_bits(out, b.contacts(max_contacts=512))
    got = _rows(out)
    sim, rs = oracle_sim(m), np.random.RandomState(13)
    left_out, worst, kinds = [], 0.0, set()
    for e, (q, ref) in enumerate(zip(qs, refs)):
        kinds |= _kinds(m, ref)
        try:
            worst = max(worst, CR.compare(got[e], ref, "gripper %d pose %d" % (gripper, e)))
        except AssertionError:
            if not CR.knife_edge(sim, q, ref, rs):
                raise
            left_out.append(e)
    print("gripper %d: %d poses, left out %s (knife edges), up to %d contacts, max deviation %.2e, pair types %s"
          % (gripper, len(qs), left_out, max(r["ncon"] for r in refs), worst, ", ".join(sorted(kinds))))
    assert len(qs) == CR.SWEEP_POSES
    assert len(left_out) <= 1, left_out


def _choose_cap(m, refs):
    """a cap C from the uncapped lists: the C for which the most poses have record C and record C + 1 in one box - box pair, among those
    that leave at least one pose below C records and one above (the smallest such C on a tie).  C >= 32: a smaller cap would cut every
    list within the first pairs of the table"""
    best, where = (0, 0), None
    counts = [r["ncon"] for r in refs]
    for c in range(32, max(counts)):
        if not (min(counts) < c and max(counts) > c):
            continue
        cut = [e for e, r in enumerate(refs) if r["ncon"] > c and (r["geom"][c - 1] == r["geom"][c]).all() and m.geom_type[r["geom"][c, 0]] == 6]
        if len(cut) > best[0]:
            best, where = (len(cut), c), cut
    assert best[0] >= 1, "no cap cuts a box - box pair's records"
    return best[1], where


def test_model_cap_cuts_the_list_where_the_oracle_cuts_it(tmp_path):
    """the model's own nconmax as the cap, chosen from the oracle's uncapped lists so that it falls between two records of one box - box
    pair in some poses, above the whole list in others and below it in others: ncon = min(records, C), the first ncon slots are the
    oracle's (built from the capped model), every slot from ncon on and the memory behind the tensors keep their canary.  Then again
    with max_contacts = C - 3, which cuts first: ncon stays the capped count."""
    torch = _torch()
    m, qs, refs = _sweep(CAP_GRIPPER, tmp_path)
    assert max(r["ncon"] for r in refs) < min(int(m.nconmax), 512)      # (the lists of the sweep's model are uncapped)
    cap, cut = _choose_cap(m, refs)
    xml = CR.sweep_gripper_xmls()[CAP_GRIPPER]
    assert xml.count('nconmax="300"') == 1
    mc = _compile(tmp_path, "capped.xml", xml.replace('nconmax="300"', 'nconmax="%d"' % cap))
    assert int(mc.nconmax) == cap
    sim = oracle_sim(mc)
    capped = [CR.oracle_contacts(sim, q) for q in qs]
    below = sum(r["ncon"] < cap for r in refs)
    print("cap %d: %d poses cut inside a box - box pair, %d poses below the cap, %d above" % (cap, len(cut), below, sum(r["ncon"] > cap for r in refs)))
    b = _pose_batch(mc, qs)
    worst = 0.0
    for mcs in (cap + 5, cap - 3):
        out, whole = _canary(torch, b, len(qs), mcs)
        b.contacts_into(out)
        h = {k: v.cpu().numpy() for k, v in out.items()}
        for e, (ref, cref) in enumerate(zip(refs, capped)):
            n = min(ref["ncon"], cap)
            assert cref["ncon"] == n and h["ncon"][e] == n, (e, mcs, h["ncon"][e], cref["ncon"], ref["ncon"])
            k = min(n, mcs)
            row = dict(ncon=n, geom=h["geom"][e, :k], dist=h["dist"][e, :k], pos=h["pos"][e, :k], frame=h["frame"][e, :k])
            worst = max(worst, CR.compare(row, cref, "cap %d max_contacts %d pose %d" % (cap, mcs, e)))
            for key, val in (("geom", -77), ("dist", -7.5), ("pos", -7.5), ("frame", -7.5)):
                assert (h[key][e, k:] == val).all(), (key, e, mcs)
        for key, buf in whole.items():
            tail = buf[-64:].cpu().numpy()
            assert (tail == tail[0]).all() and tail[0] in (-77, -7.5), key
    print("cap %d: max deviation %.2e" % (cap, worst))


def test_poses_in_global_memory_match_oracle(tmp_path):
    """sg_contacts_kernel<false>: a model whose poses do not fit LDS beside the staging block.  The plan builder bounds the geoms that
    collide, not the ones that collide with nothing: a gripper of the sweep with 1400 such geoms on its static body is accepted, and
    its read-out keeps the poses in a per-env block of global memory.  Two envs, the rest pose and the swept pose with the most
    contacts, against the oracle."""
    xml = CR.sweep_gripper_xmls()[MANY_GEOMS_GRIPPER]
    extra = "".join('<geom type="sphere" size="0.01" pos="%.2f %.2f 1.6" contype="0" conaffinity="0" mass="1e-6"/>\n'
                    % (0.3 + 0.05 * (k % 37), -0.9 + 0.05 * (k // 37)) for k in range(1400))
    roof = '<geom class="link" name="roof"'
    assert xml.count(roof) == 1
    m = _compile(tmp_path, "many_geoms.xml", xml.replace(roof, extra + roof))
    assert 35328 + 8 * (7 * m.nbody + 12 * m.ngeom) > POSE_LDS_LIMIT, (m.nbody, m.ngeom)
    sim = oracle_sim(m)
    swept = max(CR.pose_sweep(m, 16, CR.SWEEP_POSE_SEED + MANY_GEOMS_GRIPPER), key=lambda q: CR.oracle_contacts(sim, q)["ncon"])
    qs = np.stack([np.array(m.qpos0, dtype=np.float64), swept])
    refs = [CR.oracle_contacts(sim, q) for q in qs]
    assert refs[0]["ncon"] >= 10 and refs[1]["ncon"] >= 64, [r["ncon"] for r in refs]
    b = _pose_batch(m, qs)
    out = b.contacts(max_contacts=512)
    _same_bits(out, b.contacts(max_contacts=512))
    got = _rows(out)
    worst = max(CR.compare(got[e], refs[e], "many geoms, env %d" % e) for e in range(2))
    print("%d bodies, %d geoms: ncon %s, max deviation %.2e" % (m.nbody, m.ngeom, [r["ncon"] for r in refs], worst))


@pytest.mark.parametrize("scene,pipeline", [("softbox", "rows"), ("softbox", "tree"), ("freeball_fix", "tree")])
def test_read_out_leaves_the_following_steps_bit_identical(scene, pipeline):
    """two batches of the same envs, one of them reading its contacts between the steps: state, sensors and touch bits stay bit-identical"""
    damper, jids, tids, nu = SCENES[scene]
    m = sg.load_model(model_path(scene), damper)
    ks = np.linspace(350, 1350, 5)
    runs = []
    for read in (False, True):
        nm, b, sens, flags, touch = _batch(m, ks, jids, tids, pipeline)
        b.reset(1, sens=sens, flags=flags, touch=touch)
        b.set_ctrl_broadcast(np.full(nu, -0.2))
        rec = []
        for t in range(12):
            if read:
                c = b.contacts(env_ids=None if t % 2 else [3, 0], max_contacts=64)
                assert int(c["ncon"].min()) >= 0
            b.step(7, sens=sens, flags=flags, touch=touch)
            st = b.get_state()
            rec.append([sens.cpu().numpy().copy(), touch.cpu().numpy().copy(), b.touch_words(2).cpu().numpy(), flags.cpu().numpy().copy()] +
                       [st[k].cpu().numpy() for k in ("qpos", "qvel", "act", "qacc_warmstart")])
        runs.append(rec)
    for t, (a, c) in enumerate(zip(*runs)):
        for x, y in zip(a, c):
            assert x.tobytes() == y.tobytes(), t


def _bits_from_list(m, rows):
    """the touch bits recomputed from a contact list: bit g = moving finger box g (geom-id order) against a geom whose name holds OBJ"""
    boxes = [g for g in range(m.ngeom) if m.geom_type[g] == 6 and m.body_weldid[m.geom_bodyid[g]] != 0]
    index = {g: i for i, g in enumerate(boxes)}
    obj = ["OBJ" in (n or "") for n in m.geom_names]
    want = 0
    for g1, g2 in rows["geom"]:
        for g, o in ((g1, g2), (g2, g1)):
            if g in index and obj[o]:
                want |= 1 << index[g]
    return want


@pytest.mark.parametrize("scene", ["softbox", "softball", "softcylinder", "fourfinger_softball_fix"])
def test_list_agrees_with_the_touch_bits_after_reset(scene):
    """after sg_reset(mask = NULL, sim_start = 0) nothing lies between the collision pass behind the touch bits and the current qpos: the
    bits recomputed from the list equal sg_get_touch_words for every env, in every pipeline that runs the scene"""
    from softgrip_amd import native
    damper, jids, tids, nu = SCENES[scene]
    m = sg.load_model(model_path(scene), damper)
    ks = np.random.RandomState(5).uniform(300, 1400, 7)
    ran, any_bits = [], 0
    for pipeline in ("rows", "tree"):
        try:
            nm, b, sens, flags, touch = _batch(m, ks, jids, tids, pipeline)
        except native.SoftgripError as err:
            assert err.code == native.SG_ERR_MODEL, err     # (the four-finger gripper is outside the two-finger kernels' class)
            continue
        ran.append(pipeline)
        b.reset(0, sens=sens, flags=flags, touch=touch)
        words = b.touch_words(2).cpu().numpy().astype(np.int64) & 0xFFFFFFFF
        rows = _rows(b.contacts(max_contacts=MAXC))
        for e in range(len(ks)):
            assert 0 <= rows[e]["ncon"] <= MAXC
            want = _bits_from_list(m, rows[e])
            assert int(words[e, 0]) | (int(words[e, 1]) << 32) == want, (scene, pipeline, e, rows[e]["ncon"])
            if nm.nboxes <= 32:
                assert int(touch[e].item()) & 0xFFFFFFFF == want & 0xFFFFFFFF, (scene, pipeline, e)
            any_bits |= want
        print("%s %s: ncon %s, bits %x" % (scene, pipeline, [r["ncon"] for r in rows], any_bits))
    assert ran == (["tree"] if scene.startswith("fourfinger") else ["rows", "tree"]) or (scene != "softbox" and ran == ["rows"]), ran
    if scene in ("softball", "softcylinder"):
        assert any_bits, scene       # (these scenes start with the shell inside the fingers: tens of contacts at reset)


def test_manenv_get_contacts():
    from softgrip_amd.manenv import ManEnv
    env = ManEnv(1, 7, [model_path("softball")], is_vis=False, n_envs=4, tendon_damper="implicit")
    env.reset()
    env.close_hand()
    for _ in range(30):
        env.step()
    c = env.get_contacts()
    d = env.get_env().contacts()
    assert set(c) == set(d) | {"geom_names"}
    for k in d:
        assert c[k].is_cuda and c[k].cpu().numpy().tobytes() == d[k].cpu().numpy().tobytes(), k
    names = c["geom_names"]
    assert names == [n or "" for n in env.model.geom_names] and len(names) == env.nmodel.ngeom
    ncon, geom = c["ncon"].cpu().numpy(), c["geom"].cpu().numpy()
    assert (ncon > 0).all()
    for e in range(4):
        for g1, g2 in geom[e, :ncon[e]]:
            # every contact of this scene is a shell capsule (geom1: capsule < box) against a finger box
            assert "OBJ" in names[g1] and "OBJ" not in names[g2], (names[g1], names[g2])
            assert env.model.geom_type[g1] == 3 and env.model.geom_type[g2] == 6
    sub = env.get_contacts(env_ids=[2, 0], max_contacts=16)
    assert sub["geom"].shape == (2, 16, 2) and sub["ncon"].cpu().numpy().tolist() == ncon[[2, 0]].tolist()
