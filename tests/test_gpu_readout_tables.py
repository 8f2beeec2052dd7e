"""Which tables a read-out pulls in when it is the FIRST call on a fresh batch (csrc/sg_readout.hip Readout::need_*): every family of
read-outs -- poses, contacts, ray, dyn, smooth, point, solve -- goes first once and is followed by all the others, and every output must be
bit-equal to a batch that made the same calls in the opposite order.  sg_get_jacobians and sg_get_point_inertia walk at the batch's row
of zeros, which belongs to neither table: each of them is the very first call once (they lead their families).  No tolerance: the same
kernels on the same state.

Models: tests/data/mini_gripper.xml, and models/freeball_fix.sgmodel for the blob that carries jnt_qposadr / jnt_dofadr.
tests/data/free_body.xml carries them too but is no model of the library: both plan builders refuse it (held below), so no batch of it
exists.  Shape: 3 envs, env ids [2, 0], two points, n_rhs = 2; the state is a few steps into a squeeze, copied into every batch."""
import numpy as np
import pytest

import dyn_ref as DR

pytestmark = pytest.mark.gpu

ENV_IDS = [2, 0]
# the calls of a family in the order they are made when the family's turn comes (the opposite batch makes them back to front)
FAMILIES = {
    "poses": ["poses"],
    "contacts": ["contacts"],
    "ray": ["ray"],
    "dyn": ["velocities", "tendons", "energy"],
    "smooth": ["mass_matrix", "joint_forces", "inverse_dynamics"],
    "point": ["jacobians", "point_motion"],
    "solve": ["point_inertia", "solve_mass", "forward_smooth"],
}


def _torch():
    import torch
    return torch


def _load(name):
    return DR.load(name)


_STATE = {}


def _state(name):
    """(model, state): the state of a 3-env batch after sg_reset and four env steps of a squeeze, every env at its own stiffness --
    device tensors, computed once per model and never changed"""
    if name not in _STATE:
        from softgrip_amd import native
        torch = _torch()
        m = _load(name)
        _, jids, tids, nu = DR.SCENES[name]
        b = native.NativeBatch(native.NativeModel(m), 3, 0)
        b.set_stiffness(np.asarray(DR.KS), jids, tids)
        flags = torch.zeros(b.n, dtype=torch.int32, device=b.device)
        b.reset(1, flags=flags)
        b.set_ctrl_broadcast(np.full(nu, -0.2))
        for _ in range(4):
            b.step(7, flags=flags)
        assert int(flags.abs().sum()) == 0
        st = b.get_state()
        assert all(bool(torch.isfinite(v).all()) for v in st.values())
        _STATE[name] = (m, {k: v.clone() for k, v in st.items()})
    return _STATE[name]


def _inputs(m, b):
    """what the calls are asked: two points (one of them on the last body, off its origin, with a frame of its own), two right-hand
    sides, an acceleration and four rays per env -- seeded, the same for every batch"""
    torch = _torch()
    rs = np.random.RandomState(22)
    T = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=b.device)  # noqa: E731
    k = len(ENV_IDS)
    origin = np.array([[0.0, 0.0, 3.0], [0.3, 0.1, 3.0], [2.0, 0.0, 0.4], [0.0, -2.0, 0.3]])
    direction = np.array([[0.0, 0.0, -1.0], [0.0, 0.0, -1.0], [-1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    return dict(body=np.array([m.nbody - 1, 1], np.int32), pos=rs.uniform(-0.05, 0.05, (2, 3)), quat=rs.standard_normal((2, 4)),
                y=T(rs.standard_normal((k, 2, m.nv))), qacc=T(rs.standard_normal((k, m.nv))), origin=T(origin), direction=T(direction))


def _call(b, name, x):
    """one entry point -> dict of its device tensors"""
    ids = ENV_IDS
    if name == "poses":
        return b.poses(ids)
    if name == "contacts":
        return b.contacts(ids, max_contacts=64)
    if name == "ray":
        return b.raycast(x["origin"], x["direction"], env_ids=ids, normals=True)
    if name == "velocities":
        return b.velocities(ids)
    if name == "tendons":
        return b.tendons(ids)
    if name == "energy":
        return dict(energy=b.energy(ids))
    if name == "mass_matrix":
        return dict(M=b.mass_matrix(ids))
    if name == "joint_forces":
        return b.joint_forces(ids)
    if name == "inverse_dynamics":
        return dict(inverse=b.inverse_dynamics(x["qacc"], ids))
    if name == "jacobians":
        return b.jacobians(x["body"], x["pos"], env_ids=ids)
    if name == "point_motion":
        return b.point_motion(x["body"], x["pos"], x["quat"], env_ids=ids)
    if name == "point_inertia":
        return dict(zip(("W", "pivot"), b.point_inertia(x["body"], x["pos"], ids)))
    if name == "solve_mass":
        return dict(zip(("x", "pivot"), b.solve_mass(x["y"], ids)))
    assert name == "forward_smooth", name
    return b.forward_smooth(env_ids=ids)


def _run(name, calls):
    """a fresh batch at the model's state, the calls in the given order -> {call: {output: host bytes}}"""
    from softgrip_amd import native
    torch = _torch()
    m, st = _state(name)
    b = native.NativeBatch(native.NativeModel(m), 3, 0)
    _, jids, tids, _ = DR.SCENES[name]
    b.set_stiffness(np.asarray(DR.KS), jids, tids)
    b.set_state(qpos=st["qpos"], qvel=st["qvel"], act=st["act"])
    x = _inputs(m, b)
    out = {}
    for c in calls:
        out[c] = _call(b, c, x)
    torch.cuda.synchronize()
    return {c: {k: v.cpu().numpy().tobytes() for k, v in o.items()} for c, o in out.items()}


@pytest.mark.parametrize("first", sorted(FAMILIES))
@pytest.mark.parametrize("name", ["mini_gripper", "freeball_fix"])
def test_a_family_that_goes_first_pulls_in_the_tables_it_needs(name, first):
    calls = [c for fam in [first] + [f for f in FAMILIES if f != first] for c in FAMILIES[fam]]
    assert len(calls) == len(set(calls)) == 14 and calls[0] == FAMILIES[first][0]
    got, back = _run(name, calls), _run(name, calls[::-1])
    seen = 0
    for c in calls:
        assert sorted(got[c]) == sorted(back[c]) and got[c], c
        for k in got[c]:
            assert len(got[c][k]) > 0 and got[c][k] == back[c][k], (name, first, c, k)
            seen += 1
    assert seen >= 30
    # the outputs are no sentinels of an empty call: a mass matrix with a positive diagonal, poses off the origin
    m = _state(name)[0]
    M = np.frombuffer(got["mass_matrix"]["M"]).reshape(len(ENV_IDS), m.nv, m.nv)
    assert (np.diagonal(M, axis1=1, axis2=2) > 0).all()
    assert np.abs(np.frombuffer(got["poses"]["xpos"])).max() > 0.1 and np.isfinite(np.frombuffer(got["point_inertia"]["W"])).all()


def test_free_body_xml_is_no_model_of_the_library():
    """why the second model above is freeball_fix: sg_model_create refuses tests/data/free_body.xml (no composite for the two-finger
    kernels' plan, none for the tree pipeline's), so no batch can hold it"""
    import os

    import softgrip_amd as sg
    from softgrip_amd import native
    m = sg.compile_mjcf(os.path.join(DR.ROOT, "tests", "data", "free_body.xml"), composite_neighbors=False)
    assert m.has_free_joint
    with pytest.raises(native.SoftgripError) as e:
        native.NativeModel(m)
    assert "sg_model_create" in str(e.value)
