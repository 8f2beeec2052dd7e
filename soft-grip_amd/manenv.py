"""Batched ``ManEnv``: the reference's env API (reference environment/manenv.py:8-126,
environment/interface/environment.py:1-10) over the MI355X-native simulator.

Same constructor, methods, class attributes and defaults as the reference; the one
extension is ``n_envs`` (default 1).  With ``n_envs == 1`` every method returns what the
reference returns (``step() -> (ndarray(12,), bool)``, ``reset() -> float``); with
``n_envs > 1`` the same calls act on all envs in lockstep and return device tensors
(``[n,12]`` float64, ``[n]`` bool) / an ``ndarray[n]`` of stiffnesses.
"""
import os

import numpy as np

from . import native
from .mjcf import load_model


def tactile_rays(model, res=(8, 8), faces=None):
    """The rays of ``ManEnv.tactile_depth``: per moving finger box (those of sg_model_nboxes, in geom-id order) a W x H grid of rays that
    cross the box from the face OPPOSITE its pad and leave through the pad.  res = (W, H).  Body-frame rays, the same for every env.

    A box has half extents s and a pad face (a, sigma): axis a in {0, 1, 2} of the geom's frame, sigma = +-1.  By default the face whose
    outward normal at qpos0 has the largest dot product with (centre-sphere geom position - box centre); ``faces`` = one (axis, sign)
    per box overrides it (a model without a centre sphere needs it: ValueError otherwise).  With u = (a + 1) % 3, v = (a + 2) % 3,
    cell (i, j), i < W, j < H, in the geom's frame:
        p[u] = s[u] (2 (i + .5) / W - 1),  p[v] = s[v] (2 (j + .5) / H - 1),  p[a] = -sigma s[a],  direction = sigma e_a
    both mapped by the geom's local pose (geom_pos, geom_quat) into its body's frame; ray_body = ray_exclude = the geom's body.
    Returns dict(origin [B, H, W, 3], direction [B, H, W, 3], body [B, H, W] int32, thickness [B] = 2 s[a], geoms [B], faces [B, 2])."""
    from .mjcf import quat_to_mat
    m = model
    W, H = int(res[0]), int(res[1])
    if W < 1 or H < 1:
        raise ValueError("tactile_rays: res must be (W, H) with both >= 1")
    boxes = [g for g in range(m.ngeom) if m.body_weldid[m.geom_bodyid[g]] != 0 and m.geom_type[g] == 6]
    if faces is None:
        centre = [g for g in range(m.ngeom) if m.geom_type[g] == 2]
        if len(centre) != 1:
            raise ValueError("tactile_rays: the model has no centre sphere to aim the pads at -- pass faces=[(axis, sign), ...], one per finger box")
        kin = m.kinematics(np.asarray(m.qpos0, dtype=np.float64))
        world = lambda g: (kin["xpos"][m.geom_bodyid[g]] + kin["xmat"][m.geom_bodyid[g]] @ m.geom_pos[g],  # noqa: E731
                           kin["xmat"][m.geom_bodyid[g]] @ quat_to_mat(m.geom_quat[g]))
        target = world(centre[0])[0]
        faces = []
        for g in boxes:
            x, R = world(g)
            dots = [(sg_ * float(R[:, a] @ (target - x)), -a, a, sg_) for a in range(3) for sg_ in (1, -1)]
            faces.append(max(dots)[2:])      # (of equal dot products the smaller axis, then the + side)
    faces = [(int(a), int(sg_)) for a, sg_ in faces]
    if len(faces) != len(boxes) or any(a not in (0, 1, 2) or sg_ not in (1, -1) for a, sg_ in faces):
        raise ValueError("tactile_rays: faces needs one (axis in 0..2, sign +-1) per finger box (%d)" % len(boxes))
    B = len(boxes)
    origin, direction = np.zeros((B, H, W, 3)), np.zeros((B, H, W, 3))
    body, thick = np.zeros((B, H, W), dtype=np.int32), np.zeros(B)
    ci = 2.0 * (np.arange(W) + 0.5) / W - 1.0
    cj = 2.0 * (np.arange(H) + 0.5) / H - 1.0
    for k, (g, (a, sg_)) in enumerate(zip(boxes, faces)):
        s = np.asarray(m.geom_size[g], dtype=np.float64)
        u, v = (a + 1) % 3, (a + 2) % 3
        p = np.zeros((H, W, 3))
        p[..., u] = s[u] * ci[None, :]
        p[..., v] = s[v] * cj[:, None]
        p[..., a] = -sg_ * s[a]
        R = quat_to_mat(m.geom_quat[g])
        origin[k] = np.asarray(m.geom_pos[g]) + p @ R.T
        direction[k] = sg_ * R[:, a]
        body[k] = m.geom_bodyid[g]
        thick[k] = 2.0 * s[a]
    return dict(origin=origin, direction=direction, body=body, thickness=thick, geoms=np.array(boxes, dtype=np.int32), faces=np.array(faces, dtype=np.int32).reshape(B, 2))


class Env(object):
    """reference environment/interface/environment.py:1-10"""

    def __init__(self, sim_start, sim_step):
        self.sim_start = sim_start
        self.sim_step = sim_step

    def step(self, *args):
        raise NotImplementedError("Not implemented")

    def reset(self):
        raise NotImplementedError("Not implemented")


class SimulationError(Exception):
    """Counterpart of mujoco_py.builder.MujocoException (reference manenv.py:50)."""


class ManEnv(Env):
    # ids / names exactly as the reference (environment/manenv.py:12-18)
    joint_ids = list(range(11, 64))
    tendon_ids = list(range(1))
    finger_names = ['g12', 'g2']
    obj_name = 'OBJ'
    n_actuated = 2    # close_hand / loose_hand drive ctrl[0 .. n_actuated - 1] (`for i in range(2)`, reference manenv.py:93-101); 4 for the four-finger gripper

    def __init__(self, sim_start, sim_step, env_paths, is_vis=True, n_envs=1, device=0, contact_flag_mode="intent", check_scene=True,
                 tendon_damper="auto", joint_ids=None, tendon_ids=None, finger_names=None, n_actuated=None, max_cached_scenes=4,
                 render_dir=None, render_envs=(0,), render_size=(320, 240), render_every=1, camera=None, render_skin=False):
        """``joint_ids`` / ``tendon_ids``: which model entries ``set_new_stiffness`` writes; default = the reference's class attributes
        (joints 11..63 and tendon 0: manenv.py:12-13), to be overridden for a scene with another layout (e.g. a smaller shell).
        ``tendon_damper``: how the damper of the composite's volume tendon is integrated (mjcf.load_model).
        "explicit" = MuJoCo's Euler step as restated; "implicit" = the rank-one implicit treatment; "auto" (default) = explicit,
        and a scene that fails the load-time check under it (the reference's soft ball / cylinder) is reloaded with "implicit",
        with a printed notice.  ``self.tendon_damper`` holds what the loaded scene runs with.
        ``render_dir``: when set, every ``render_every``-th call of ``render()`` writes PNGs of the envs ``render_envs`` at
        ``render_size`` (width, height) seen through ``camera`` (7 numbers of MuJoCo's free camera; None = the scene's default camera)
        as <render_dir>/<render_prefix>_e<env>_t<call>.png; ``render_prefix`` defaults to s<scene>_b<episode>.  Without it
        ``render()`` stays the no-op it is (``is_vis`` starts nothing).  ``render_skin``: those frames show the soft object as its skin
        (``render_frames(skin=True)``) and not as its element capsules."""
        super().__init__(sim_start, sim_step)
        assert len(env_paths) > 0
        assert contact_flag_mode in ("intent", "reference")
        assert tendon_damper in ("auto", "explicit", "implicit")
        self._tendon_damper_arg = tendon_damper
        if joint_ids is not None:
            self.joint_ids = [int(j) for j in joint_ids]      # instance attributes shadow the class lists (which stay the reference's)
        if tendon_ids is not None:
            self.tendon_ids = [int(t) for t in tendon_ids]
        if finger_names is not None:      # e.g. ['g11', 'g12', 'g13', 'g2'] for the four-finger gripper (reference manenv.py:16)
            self.finger_names = list(finger_names)
        if n_actuated is not None:
            self.n_actuated = int(n_actuated)
        self.check_scene = check_scene
        self.max_cached_scenes = int(max_cached_scenes)   # scenes whose native batch stays allocated across load_env() calls (LRU; close() drops them)
        self.is_vis = is_vis  # no viewer exists; kept for signature parity (render() is a no-op)
        self.env_paths = env_paths
        self.n_envs = int(n_envs)
        self.device_index = device
        self.contact_flag_mode = contact_flag_mode
        self.rng = np.random  # the reference draws from the global NumPy RNG (manenv.py:104)
        self.n_resets = 0     # envs reset after a simulation warning (what `except MujocoException: self.reset()` did, manenv.py:50-51)
        self.n_capacity_resets = 0   # ... of which: envs that ran out of the KERNELS' contact capacity (SG_FLAG_CONTACTFULL: 64 per finger stream /
                                     # 128 per env) -- not a MuJoCo warning: the reference's nconmax is 500 (soft_grip_two_fingers.xml:8) and MuJoCo
                                     # would have carried on.  Counted apart so that a dataset job can refuse to paper over it (create_dataset)
        self.render_dir, self.render_envs, self.render_every, self.camera = render_dir, [int(e) for e in render_envs], int(render_every), camera
        self.render_size = (int(render_size[0]), int(render_size[1]))
        self.render_skin = bool(render_skin)
        self.render_prefix = None     # file-name prefix of the frames (None: s<scene>_b<episode>)
        self.current_scene, self._episode, self._render_calls = 0, -1, 0
        self._scenes = {}     # path -> the loaded scene (model, batch, buffers, the damper it runs with): load_env() of a scene seen before
                              # neither compiles, allocates nor dry-runs again (the reference's loop switches scene after EVERY episode)
        self._load(env_paths[0])
        self.is_closing = True

    # ---- model / batch management (reference manenv.py:27-41) ----
    _SCENE_STATE = ("model", "tendon_damper", "nmodel", "env", "_sens", "_flags", "_touch", "_ctrl", "_finger_bits", "_finger_bits_names", "_fingers_left")

    def _load(self, path, _damper=None):
        import torch
        if _damper is None and path in self._scenes:
            # A scene this instance has loaded before: its batch is kept alive, the load-time verdict (which damper it needs) with it.
            # What the reference's load_env leaves behind is a fresh MjSim -- the state after mj_resetData, the XML's own stiffness --
            # so: that state, no per-env stiffness, the reference-mode finger list refilled.
            self._scenes[path] = self._scenes.pop(path)      # most recently used last
            for k, v in self._scenes[path].items():
                setattr(self, k, v)
            self._ctrl[:] = 0
            self._sens.zero_()      # a fresh MjSim's sensordata and contact list are empty: get_sensor_sensordata() right after
            self._touch.zero_()     # load_env() must not show the previous episode's last sample
            self.stiffness = np.full(self.n_envs, np.nan)
            self._k_range = (300, 1400)
            self.env.set_stiffness(np.zeros(self.n_envs), [], [])
            self.env.reset(0, flags=self._flags)
            self._fingers_left.fill_((1 << len(self._finger_bits_names)) - 1)
            return
        want = _damper or self._tendon_damper_arg
        self.model = load_model(path, None if want == "auto" else want)
        self.tendon_damper = "implicit" if self.model.opt_implicit_tendon_damping else "explicit"
        if max(self.joint_ids) >= self.model.njnt or max(self.tendon_ids) >= self.model.ntendon:
            raise ValueError("scene %s has %d joints and %d tendons: the stiffness ids (joints %d..%d, tendons %s) do not fit it -- pass "
                             "joint_ids / tendon_ids" % (path, self.model.nv, self.model.ntendon, min(self.joint_ids), max(self.joint_ids),
                                                         self.tendon_ids))
        self.nmodel = native.NativeModel(self.model)
        if self.check_scene:
            # the load-time check runs BEFORE the batch is made, on a batch of ONE env: the dry run uses the model's own stiffness, so
            # every env of a batch would do exactly the same (r04 ran it on all n_envs and, for a scene that needs the implicit damper,
            # allocated two full batches: a third of the three-scene quick start's wall time, profiles/r05_dataset_end_to_end.txt)
            try:
                self._check_scene(path)
            except SimulationError as err:
                if want != "auto" or self.tendon_damper == "implicit":
                    raise
                print("NOTICE: %s\n        reloading it with tendon_damper=\"implicit\" (DESIGN.md D5)" % err)
                self._load(path, "implicit")
                return
        self.env = native.NativeBatch(self.nmodel, self.n_envs, self.device_index)
        dev = self.env.device
        self._sens = torch.zeros(self.n_envs, self.nmodel.nsensordata, dtype=torch.float64, device=dev)
        self._flags = torch.zeros(self.n_envs, dtype=torch.int32, device=dev)
        self._touch = torch.zeros(self.n_envs, dtype=torch.int32, device=dev)
        self._ctrl = np.zeros(self.nmodel.nu)
        self.stiffness = np.full(self.n_envs, np.nan)
        self._k_range = (300, 1400)  # range of the last set_new_stiffness draw: re-draws after a failure stay inside it
        # which finger boxes (bit 2*chain+box of `touch`) match each name in finger_names
        self._finger_bits = []
        bits = self._chain_geom_bits()
        for name in self.finger_names:
            v = sum(1 << b for b, gname in bits.items() if name in gname)
            self._finger_bits.append(v - (1 << 64) if v >= (1 << 63) else v)      # as a signed 64-bit pattern (torch has no uint64 ops)
        self._finger_bits_names = list(self.finger_names)
        # "reference" mode state: which names are still in the list the reference aliases and never refills (manenv.py:70,80), one
        # list per env, kept on the device as a bit mask (bit i = finger_names[i] not yet removed)
        self._fingers_left = torch.full((self.n_envs,), (1 << len(self._finger_bits_names)) - 1, dtype=torch.int32, device=dev)
        if self.check_scene:
            self.env.reset(0, flags=self._flags)   # the state after mj_resetData (a fresh MjSim's), as the check on the whole batch used to leave it
        self._scenes[path] = {k: getattr(self, k) for k in self._SCENE_STATE}
        while len(self._scenes) > max(1, self.max_cached_scenes):      # least recently used first; never the scene just loaded
            self._scenes.pop(next(iter(self._scenes)))

    def close(self):
        """drops every cached scene but the current one (a cached scene pins its native batch: state + work space, ~0.1 MB per env on
        the rows pipeline, ~0.5 MB per env on the tree pipeline -- hundreds of MB at 4096 envs)"""
        cur = [p for p, sc in self._scenes.items() if sc.get("env") is self.env]
        self._scenes = {p: self._scenes[p] for p in cur}

    def _check_scene(self, path, n_steps=40):
        """Fail loudly at load time for a scene that cannot produce data: the idle phase of an episode (reset + 40 env steps at
        ctrl = 0, the model's own stiffness) must run without a simulation warning.  The reference's soft ball / cylinder scenes
        start with the shell 0.14 / 0.30 deep inside the fingers (45 / 37 contacts at reset); with the volume tendon's damper
        integrated explicitly that start diverges within a few env steps (profiles/r02_ball_stability_probe.txt),
        and every reset starts there again -- the reference's `except MujocoException: self.reset()` (manenv.py:50-51) would
        loop forever."""
        import torch
        probe = native.NativeBatch(self.nmodel, 1, self.device_index)      # (one env: see _load)
        flags = torch.zeros(1, dtype=torch.int32, device=probe.device)
        bad = torch.zeros_like(flags)
        probe.reset(max(self.sim_start, 0), flags=flags)
        bad |= flags
        for _ in range(n_steps):
            probe.step(self.sim_step, flags=flags)
            bad |= flags
        if bool((bad != 0).any()):
            names = {1: "BADQPOS", 2: "BADQVEL", 4: "BADQACC", 8: "CONTACTFULL", 16: "CNSTRFULL", 32: "UNSUPPORTED_PAIR"}
            f = int(bad.max())
            raise SimulationError("scene %s does not survive its own idle phase with the %s tendon damper (flags %s within %d env steps "
                                  "at ctrl = 0); no dataset can be generated from it this way (check_scene=False loads it anyway)"
                                  % (path, self.tendon_damper, "|".join(v for k, v in names.items() if f & k), n_steps))

    def _chain_geom_bits(self):
        """bit index -> geom name for the moving finger boxes, in the kernels' order: (chain, body, geom) = geom id order (two boxes
        per finger in the two-finger class: bit 2 * chain + box)"""
        m = self.model
        moving = [g for g in range(m.ngeom) if m.body_weldid[m.geom_bodyid[g]] != 0 and m.geom_type[g] == 6]
        return {i: m.geom_names[g] or "" for i, g in enumerate(moving)}

    def _touch_bits(self):
        """per env the contact read-out as one integer: int32 word of sg_step for up to 32 finger boxes, else the words of
        sg_get_touch_words combined into an int64 (the four-finger gripper has 64 boxes)"""
        import torch
        if self.nmodel.nboxes <= 32:
            return self._touch
        w = self.env.touch_words(2).to(torch.int64) & 0xFFFFFFFF
        return w[:, 0] | (w[:, 1] << 32)

    def load_env(self, num):
        if num < len(self.env_paths):
            self._load(self.env_paths[num])
            self.current_scene = num
        else:
            print("Wrong number,")

    # ---- main methods ----
    def step(self, num_steps=-1, actions=None, min_dist=0.1):
        """reference manenv.py:44-53 (``actions`` / ``min_dist`` are unused there too)"""
        if num_steps < 1:
            num_steps = self.sim_step
        self.env.step(num_steps, sens=self._sens, flags=self._flags, touch=self._touch)
        bad = (self._flags != 0)
        if bool(bad.any()):  # mujoco_py raised -> the reference resets (re-drawing the stiffness) and carries on
            self.n_capacity_resets += int(((self._flags & native.SG_FLAG_CONTACTFULL) != 0).sum())
            self._reset_envs(bad)
        return self._result()

    def reset(self, range_min=300, range_max=1400):
        """reference manenv.py:55-63; the stiffness range is an extension (the reference always draws from U(300, 1400)):
        a rank of a sharded run passes its stiffness bin"""
        current_stiffness = self.set_new_stiffness(range_min, range_max)
        self._episode += 1
        self._render_calls = 0
        self.env.reset(max(self.sim_start, 0), sens=self._sens, flags=self._flags, touch=self._touch)
        self._ctrl[:] = 0  # mj_resetData clears ctrl
        bad = (self._flags != 0)
        if bool(bad.any()):
            self.n_capacity_resets += int(((self._flags & native.SG_FLAG_CONTACTFULL) != 0).sum())
            self._reset_envs(bad)
        return current_stiffness

    def _reset_envs(self, bad_mask, max_tries=5):
        """what `except MujocoException: self.reset()` does (reference manenv.py:50-51), for the flagged envs only: a new
        stiffness from the range of the last draw, mj_resetData (ctrl of those envs stays 0 until the next close / toggle, as in
        the reference), forward, sim_start steps.  Raises only when envs are still flagged after max_tries resets."""
        import torch
        lo, hi = self._k_range
        for _ in range(max_tries):
            idx = torch.nonzero(bad_mask).flatten().cpu().numpy()
            if idx.size == 0:
                return
            self.n_resets += int(idx.size)
            self.stiffness[idx] = self.rng.uniform(lo, hi, size=idx.size) if idx.size > 1 else self.rng.uniform(lo, hi)
            self.env.set_stiffness(self.stiffness, self.joint_ids, self.tendon_ids)
            mask = bad_mask.to(torch.uint8).contiguous()
            flags = torch.zeros_like(self._flags)
            self.env.reset(max(self.sim_start, 0), sens=self._sens, flags=flags, touch=self._touch, mask=mask)
            bad_mask = bad_mask & (flags != 0)
        idx = torch.nonzero(bad_mask).flatten().cpu().numpy()
        if idx.size:
            raise SimulationError("envs keep failing after %d resets: %s" % (max_tries, idx))

    def _contact_flags(self):
        import torch
        touch = self._touch_bits()
        if self.contact_flag_mode == "intent":
            ok = torch.ones(self.n_envs, dtype=torch.bool, device=touch.device)
            for bits in self._finger_bits:
                ok &= (touch & bits) != 0
            return ok
        # "reference": reproduce the aliased, never-refilled list of manenv.py:70-83 per env -- on the device, no host round trip:
        # a name leaves an env's list the first time one of its boxes touches an object geom; once the list is empty the flag is up
        # whenever there is any contact at all
        ncon = self.env.solver_stats()["ncon"]
        for i, bits in enumerate(self._finger_bits):
            self._fingers_left &= ~(((touch & bits) != 0).to(torch.int32) << i)   # (touch: int32, or int64 beyond 32 boxes)
        return (self._fingers_left == 0) & (ncon > 0)

    def _result(self):
        flag = self._contact_flags()
        if self.n_envs == 1:
            return self._sens[0].cpu().numpy().copy(), bool(flag[0])
        return self._sens.clone(), flag

    def get_sensor_sensordata(self):
        """reference manenv.py:65-85"""
        return self._result()

    def toggle_grip(self):
        if self.is_closing:
            self.loose_hand()
        else:
            self.close_hand()

    def close_hand(self):
        self._ctrl[:self.n_actuated] = -0.2
        self.env.set_ctrl_broadcast(self._ctrl)
        self.is_closing = True

    def loose_hand(self):
        self._ctrl[:self.n_actuated] = 0.2
        self.env.set_ctrl_broadcast(self._ctrl)
        self.is_closing = False

    def set_new_stiffness(self, range_min=300, range_max=1400):
        """reference manenv.py:103-109: one draw per env from the global NumPy RNG, written to
        jnt_stiffness[joint_ids] and tendon_stiffness[tendon_ids]"""
        self._k_range = (range_min, range_max)
        if self.n_envs == 1:
            new_value = self.rng.uniform(range_min, range_max)
            self.stiffness[0] = new_value
        else:
            new_value = self.rng.uniform(range_min, range_max, size=self.n_envs)
            self.stiffness[:] = new_value
        self.env.set_stiffness(self.stiffness, self.joint_ids, self.tendon_ids)
        return new_value

    def set_stiffness_values(self, values):
        """batched extension: explicit per-env stiffness (e.g. a stiffness-bin sweep)"""
        self.stiffness[:] = np.asarray(values, dtype=np.float64).reshape(self.n_envs)
        self.env.set_stiffness(self.stiffness, self.joint_ids, self.tendon_ids)

    def get_env(self):
        return self.env

    def render(self):
        """reference manenv.py:114-116 drives MuJoCo's viewer; here a no-op unless the env was made with ``render_dir``: then every
        ``render_every``-th call since the last reset() writes PNG frames of ``render_envs`` (headless renderer, sg_render)"""
        if self.render_dir is None or not self.render_envs:
            return
        t = self._render_calls
        self._render_calls += 1
        if t % max(1, self.render_every):
            return
        from .pngio import write_png
        rgb = self.render_frames(envs=self.render_envs, camera=self.camera, size=self.render_size, depth=False, seg=False, skin=self.render_skin)["rgb"].cpu().numpy()
        os.makedirs(self.render_dir, exist_ok=True)
        prefix = self.render_prefix or "s%d_b%d" % (self.current_scene, max(self._episode, 0))
        for k, e in enumerate(self.render_envs):
            write_png(os.path.join(self.render_dir, "%s_e%d_t%d.png" % (prefix, e, t)), rgb[k])

    def render_frames(self, envs=None, camera=None, size=(320, 240), rgb=True, depth=True, seg=True, skin=False):
        """images of the listed envs (None: all) on the current state: NativeBatch.render's dict of device tensors (rgba / rgb
        [k, H, W, 4|3] uint8, depth [k, H, W] float32, seg [k, H, W] int32); size = (width, height).  skin=True: the soft object as
        its skin (the scene's <skin>, else the one built from the composite's body names; seg = ngeom there)"""
        return self.env.render(camera=camera, env_ids=envs, width=int(size[0]), height=int(size[1]), rgb=rgb, depth=depth, seg=seg, skin=skin)

    def get_contacts(self, env_ids=None, max_contacts=256):
        """the contact list of the listed envs (None: all) at the current state -- what `sim.forward(); sim.data.contact[:ncon]` holds
        in the reference's read-out loop (manenv.py:65-85): NativeBatch.contacts' dict of device tensors (ncon [k], geom [k, C, 2],
        dist [k, C], pos [k, C, 3], frame [k, C, 9]) plus ``geom_names``, the model's list, so that a caller can write the reference's
        substring test itself: ``"OBJ" in geom_names[geom[e, i, 0]]``.  After step() the list is the NEXT forward pass's (qpos is one
        integration past the collision pass behind the touch flags); after reset() with sim_start = 0 the two coincide."""
        out = self.env.contacts(env_ids=env_ids, max_contacts=max_contacts)
        out["geom_names"] = [n or "" for n in self.model.geom_names]
        return out

    def get_forces(self, env_ids=None, max_rows=None, max_contacts=256):
        """how hard the constraints push at the current state (data.efc_force, data.qfrc_constraint and data.qacc after sim.forward()):
        NativeBatch.forces' dict of device tensors -- nefc, iters, ncon [k], efc_type, efc_id, efc_force [k, R], contact_force [k, C, 3],
        qfrc_constraint, qacc [k, nv].  After step() these are the NEXT forward pass's forces, as with get_contacts()."""
        return self.env.forces(env_ids=env_ids, max_rows=max_rows, max_contacts=max_contacts)

    def get_contact_forces(self, env_ids=None, max_contacts=256):
        """get_contacts()' dict plus ``force`` [k, C, 3], contact i's force in its own frame with the normal first (mj_contactForce's
        first three numbers; zero for a contact without constraint rows), and ``force_world`` [k, C, 3] = frame' force, the force on
        geom2 in world axes (geom1 feels its negative)"""
        out = self.get_contacts(env_ids=env_ids, max_contacts=max_contacts)
        out["force"] = self.env.forces(env_ids=env_ids, max_rows=1, max_contacts=max_contacts)["contact_force"]
        frame = out["frame"].reshape(out["frame"].shape[0], -1, 3, 3)
        out["force_world"] = (frame.transpose(2, 3) @ out["force"].unsqueeze(-1)).squeeze(-1)
        return out

    def object_body(self):
        """the soft object's body: the deepest body that is an ancestor of every body its skin is bound to (sg_model_skin_root).  A
        model without a skin gets ``model.composite_skin()`` attached first; -1 when there is none"""
        self.env._need_skin()
        return self.nmodel.skin_root()

    def get_skin_vertices(self, frame=None, env_ids=None):
        """the soft object's surface at the current state (sg_get_skin_vertices): dict of device tensors pos, vel, local [k, nvert, 3]
        -- world position, the material point's velocity, and the position in body ``frame``'s frame (None: the object's own body)"""
        body = self.object_body() if frame is None else int(frame)
        return self.env.skin_vertices(frame_body=body, env_ids=env_ids)

    def get_deformation(self, env_ids=None):
        """how far the squeeze has moved the surface, in the object's own frame: dict of device tensors disp [k, nvert, 3] = local - rest
        (rest: the vertices at qpos0, sg_model_skin_rest), max_disp [k] the largest |disp| of each env and max_vert [k] its vertex"""
        import torch
        body = self.object_body()
        local = self.env.skin_vertices(frame_body=body, env_ids=env_ids, outputs=("local",))["local"]
        disp = local - torch.from_numpy(self.nmodel.skin_rest(body)).to(local.device)
        mag, vert = disp.norm(dim=-1).max(dim=-1)
        return dict(disp=disp, max_disp=mag, max_vert=vert)

    def get_shape(self, dirs=None, dir_body=None, env_ids=None):
        """the soft object as one solid at the current state (sg_get_shape): NativeBatch.shape's dict of device tensors -- shape [k, 12]
        = volume, area, centroid, central second moments (xx yy zz xy xz yz), dV/dt; with dirs [D, 3] in the frames of dir_body [D]
        (-1 / None: world) also lo, hi [k, D], the extent along each (hi - lo: the width along a palm-fixed grip axis), and lo_vert,
        hi_vert [k, D]"""
        return self.env.shape(dirs=dirs, dir_body=dir_body, env_ids=env_ids)

    def get_subtree(self, env_ids=None):
        """centre of mass, its velocity and the angular momentum about it of every body's subtree at the current state
        (data.subtree_com, mj_subtreeVel): NativeBatch.subtree's dict of device tensors com, linvel, angmom [k, nbody, 3]; row
        object_body() is the soft object's, row 0 the whole model's"""
        return self.env.subtree(env_ids=env_ids)

    def get_velocities(self, env_ids=None):
        """body velocities of the listed envs (None: all) at the current state, world axes: NativeBatch.velocities' dict of device
        tensors ang, lin, com_lin [k, nbody, 3] -- the time derivative of the poses when qpos moves as qvel says (data.cvel /
        mj_objectVelocity).  A point p fixed on body i moves at lin[:, i] + cross(ang[:, i], p - xpos[:, i])."""
        return self.env.velocities(env_ids=env_ids)

    def get_tendons(self, env_ids=None):
        """tendon travel and its rate of the listed envs (None: all) at the current state (data.ten_length, data.ten_velocity):
        NativeBatch.tendons' dict of device tensors length, velocity [k, ntendon]"""
        return self.env.tendons(env_ids=env_ids)

    def get_energy(self, env_ids=None):
        """[k, 4] device tensor of the listed envs (None: all) at the current state: gravity, joint-spring and tendon-spring potential
        (at each env's own stiffness) and kinetic energy; data.energy is (the sum of the first three, the fourth)"""
        return self.env.energy(env_ids=env_ids)

    def get_mass_matrix(self, env_ids=None):
        """[k, nv, nv] device tensor of the listed envs (None: all) at the current state: the dense joint-space mass matrix
        (mj_fullM(data.qM)), symmetric to the bit.  nv * nv * 8 bytes per env: list fewer envs per call where memory is short"""
        return self.env.mass_matrix(env_ids=env_ids)

    def get_joint_forces(self, env_ids=None):
        """the smooth joint-space forces of the listed envs (None: all) at the current state (data.qfrc_bias, qfrc_passive,
        qfrc_actuator): NativeBatch.joint_forces' dict of device tensors bias, passive, actuator [k, nv]"""
        return self.env.joint_forces(env_ids=env_ids)

    def inverse_dynamics(self, qacc, env_ids=None):
        """mj_inverse at the current state: qacc [k, nv] (device, float64) -> qfrc_inverse [k, nv] = M qacc + bias - passive"""
        return self.env.inverse_dynamics(qacc, env_ids=env_ids)

    def get_point_motion(self, body, pos, quat=None, qpos=None, qvel=None, qacc=None, env_ids=None):
        """pose, velocity, acceleration and gyro / accelerometer readings of body-fixed points (sg_get_point_motion):
        NativeBatch.point_motion's arguments and dict of device tensors pos, mat, vel, acc, gyro, accel"""
        return self.env.point_motion(body, pos, quat, qpos=qpos, qvel=qvel, qacc=qacc, env_ids=env_ids)

    def get_jacobians(self, body, pos, qpos=None, env_ids=None):
        """mj_jac of body-fixed points (sg_get_jacobians): NativeBatch.jacobians' dict of device tensors jacp, jacr [k, P, 3, nv]"""
        return self.env.jacobians(body, pos, qpos=qpos, env_ids=env_ids)

    def solve_mass(self, y, env_ids=None, out=None):
        """mj_solveM at the current state: y [k, R, nv] or [k, nv] (device, float64) -> (x = M^-1 y, pivot [k]); NativeBatch.solve_mass"""
        return self.env.solve_mass(y, env_ids=env_ids, out=out)

    def get_qacc_smooth(self, qfrc_applied=None, env_ids=None):
        """the smooth forward dynamics at the current state (data.qacc_smooth, data.qfrc_smooth): NativeBatch.forward_smooth's dict of
        device tensors qacc_smooth, qfrc_smooth [k, nv] and pivot [k]"""
        return self.env.forward_smooth(qfrc_applied, env_ids=env_ids)

    def get_point_inertia(self, body, pos, quat=None, env_ids=None):
        """J M^-1 J' at body-fixed points (sg_get_point_inertia): (W [k, P, 6, 6], pivot [k]).  quat is accepted and ignored -- W is in
        world axes -- so that ``get_point_inertia(*env.sensor_sites())`` works as ``get_point_motion(*env.sensor_sites())`` does"""
        return self.env.point_inertia(body, pos, env_ids=env_ids)

    def sensor_sites(self):
        """the model's IMU sites -- every site a gyro or an accelerometer sits at, in ascending order -- as (body [S] int32, pos [S, 3],
        quat [S, 4]), ready to pass as points: ``get_point_motion(*env.sensor_sites())``"""
        body, pos, quat = self.nmodel.sites()
        m = self.model
        from .mjcf import SENS_ACCELEROMETER, SENS_GYRO
        imu = sorted({int(m.sensor_objid[s]) for s in range(len(m.sensor_type)) if int(m.sensor_type[s]) in (SENS_ACCELEROMETER, SENS_GYRO)})
        return body[imu], pos[imu], quat[imu]

    def virtual_imu(self, body, pos, quat=None, n_substeps=-1):
        """one env step with gyros and accelerometers at the given points for the SAME forward pass as the sensordata it returns (the
        header's recipe): n - 1 substeps, qpos and qvel saved, one substep, then sg_get_point_motion at the saved state with that
        substep's qacc (qacc_warmstart).  Returns (sensordata [n_envs, nsensordata], gyro [n_envs, P, 3], accel [n_envs, P, 3]),
        ALWAYS as device tensors, also with n_envs == 1 (step() returns an ndarray and a bool there), and no contact flag.
        While no env raises a flag the batch ends in the state step() leaves and the sensordata has step()'s bits.  For an env that
        does raise one the two differ: the env is reset as in step(), but the sensordata returned is that of the step that FAILED,
        which the virtual readings belong to -- step() returns the sensordata after the reset --, and an env flagged BADQPOS / BADQVEL /
        BADQACC in the first n - 1 substeps is taken through the last substep by the second sg_step call, where one sg_step(n) would
        have left it where it stopped; it is reset right after, so nothing of that substep survives"""
        n = self.sim_step if n_substeps < 1 else n_substeps
        if n > 1:
            self.env.step(n - 1, sens=self._sens, flags=self._flags, touch=self._touch)
            early = self._flags.clone()
        st = self.env.get_state()
        self.env.step(1, sens=self._sens, flags=self._flags, touch=self._touch)
        if n > 1:
            self._flags |= early
        out = self.env.point_motion(body, pos, quat, qpos=st["qpos"], qvel=st["qvel"], qacc=self.env.get_state()["qacc_warmstart"], outputs=("gyro", "accel"))
        sens = self._sens.clone()
        bad = (self._flags != 0)
        if bool(bad.any()):
            self.n_capacity_resets += int(((self._flags & native.SG_FLAG_CONTACTFULL) != 0).sum())
            self._reset_envs(bad)
        return sens, out["gyro"], out["accel"]

    def raycast(self, origin, direction, body=None, exclude=None, env_ids=None, cat_mask=native.SG_RAY_ALL, max_dist=0.0, normals=False, skin=False):
        """ray queries on the current state (mj_ray; sg_ray): NativeBatch.raycast's arguments and dict of device tensors (dist [k, R],
        geom [k, R], normal [k, R, 3] with normals=True).  skin=True (SG_RAY_SKIN): the soft object is seen as its skin (the scene's
        <skin>, else the one built from the composite's body names; the plain call when there is none) -- its triangles are candidates
        with SG_RAY_ELEM in cat_mask, the element geoms never; front faces only, t > 0, watertight on shared edges and vertices;
        geom = ngeom + face index there (a geom wins a tie), normal = the flat face normal, and ``face`` [k, R] (-1 off the skin) is added"""
        return self.env.raycast(origin, direction, body=body, exclude=exclude, env_ids=env_ids, cat_mask=cat_mask, max_dist=max_dist, normals=normals,
                                skin=skin)

    def tactile_depth(self, res=(8, 8), max_gap=0.05, env_ids=None, faces=None, cat_mask=native.SG_RAY_ELEM | native.SG_RAY_CENTER, skin=False):
        """A tactile depth map of the finger pads: for every moving finger box (sg_model_nboxes, its order) a res = (W, H) grid of
        distances from the pad's face to the object surface in front of it.  Returns dict(gap [k, nboxes, H, W] float64 device tensor:
        metres, NEGATIVE where the object has pushed into the pad (the penetration depth), +inf where nothing lies within max_gap;
        geom [k, nboxes, H, W] int32: the geom seen, -1 for none).

        The rays are ``tactile_rays(model, res, faces)`` -- built once per scene and cached; the formula is in that function's
        docstring so that a C caller can build the same -- cast with ray_body = ray_exclude = the box's body, cat_mask (default: the
        soft object's elements and centre) and max_dist = max over boxes of 2 s[a] + max_gap.  A ray starts on the face opposite the
        pad and crosses the box from inside (an origin inside a geom does not see it, and the box's body is excluded), so
        gap = dist - 2 s[a].

        skin=True: the same rays, exclusion, max_dist and gap formula against the soft object's SKIN (raycast(skin=True): the surface
        a depth-type sensor sees) and not against the element capsules the solver collides with: the triangles are candidates with
        SG_RAY_ELEM in cat_mask, front faces only, watertight; geom is then ngeom + face index on the skin and the dict carries
        ``face`` [k, nboxes, H, W] int32 (the triangle seen, -1 off the skin or for none) next to it."""
        import torch
        key = (tuple(int(r) for r in res), None if faces is None else tuple((int(a), int(s)) for a, s in faces))
        cache = self.__dict__.setdefault("_tactile_cache", {})
        ent = cache.get((id(self.model), key))
        if ent is None:
            rays = tactile_rays(self.model, res, faces)
            dev = self.env.device
            ent = dict(origin=torch.from_numpy(rays["origin"].reshape(-1, 3).copy()).to(dev), direction=torch.from_numpy(rays["direction"].reshape(-1, 3).copy()).to(dev),
                       body=rays["body"].reshape(-1), thickness=rays["thickness"], thick_t=torch.from_numpy(rays["thickness"]).to(dev),
                       shape=rays["body"].shape, model=self.model)
            cache[(id(self.model), key)] = ent
        B, H, W = ent["shape"]
        max_gap = float(max_gap)
        if B == 0:
            k = self.n_envs if env_ids is None else len(env_ids)
            empty = dict(gap=torch.empty(k, 0, H, W, dtype=torch.float64, device=self.env.device), geom=torch.empty(k, 0, H, W, dtype=torch.int32, device=self.env.device))
            if skin:
                empty["face"] = torch.empty_like(empty["geom"])
            return empty
        out = self.env.raycast(ent["origin"], ent["direction"], body=ent["body"], exclude=ent["body"], env_ids=env_ids, cat_mask=cat_mask,
                               max_dist=float(ent["thickness"].max()) + max_gap, skin=skin)
        dist = out["dist"].view(-1, B, H, W)
        geom = out["geom"].view(-1, B, H, W)
        gap = dist - ent["thick_t"].view(1, B, 1, 1)
        seen = (dist >= 0) & (gap <= max_gap)
        inf = torch.full_like(gap, float("inf"))
        res_ = dict(gap=torch.where(seen | torch.isnan(dist), gap, inf), geom=torch.where(seen, geom, torch.full_like(geom, -1)))
        if skin:
            res_["face"] = torch.where(seen, out["face"].view(-1, B, H, W), torch.full_like(geom, -1))
        return res_

    # ---- fused episode: the create_dataset.py schedule without a host round trip per step ----
    def rollout(self, schedule, out=None, reset=True, energy_out=None, shape_out=None, shape_dirs=None, shape_dir_body=None):
        """Runs ``len(schedule)`` env steps; ``schedule[t]`` is the broadcast ctrl (or None = unchanged) applied
        before step t.  Writes sensordata into ``out[n, T, 12]`` (allocated when None) and returns
        ``(out, flags_or[n])``.  Envs that fail are NOT reset here (their flags are returned).
        ``energy_out``: a ``[n, T, 4]`` float64 device tensor that receives get_energy() of the state after every env step (one
        sg_get_energy per step, on the same stream); None: no such call is made.
        ``shape_out``: a ``[n, T, 12 + 2 D]`` float64 device tensor that receives get_shape(shape_dirs, shape_dir_body) of the state
        after every env step -- shape, lo, hi side by side, D the number of shape_dirs (one sg_get_shape per step, on the same
        stream); None: no such call is made."""
        import torch
        T = len(schedule)
        dev = self.env.device
        nsd = self.nmodel.nsensordata
        if out is None:
            out = torch.empty(self.n_envs, T, nsd, dtype=torch.float64, device=dev)
        assert out.shape == (self.n_envs, T, nsd) and out.is_contiguous()
        flags_or = torch.zeros(self.n_envs, dtype=torch.int32, device=dev)
        if energy_out is not None:
            assert energy_out.shape == (self.n_envs, T, 4) and energy_out.dtype == torch.float64 and energy_out.device == dev
            e_row = torch.empty(self.n_envs, 4, dtype=torch.float64, device=dev)
        if shape_out is not None:
            nd = 0 if shape_dirs is None else len(np.asarray(shape_dirs, dtype=np.float64).reshape(-1, 3))
            assert shape_out.shape == (self.n_envs, T, 12 + 2 * nd) and shape_out.dtype == torch.float64 and shape_out.device == dev
        if reset:
            self.env.reset(max(self.sim_start, 0), sens=self._sens, flags=self._flags, touch=self._touch)
            self._ctrl[:] = 0
            flags_or |= self._flags
        for t in range(T):
            if schedule[t] is not None:
                self._ctrl[:] = schedule[t]
                self.env.set_ctrl_broadcast(self._ctrl)
            self.env.step(self.sim_step, sens=out[:, t], sens_stride=T * nsd, flags=self._flags, touch=self._touch)
            flags_or |= self._flags
            if energy_out is not None:
                energy_out[:, t] = self.env.energy(out=e_row)
            if shape_out is not None:
                s = self.env.shape(dirs=shape_dirs, dir_body=shape_dir_body)
                shape_out[:, t] = torch.cat([s["shape"]] + ([s["lo"], s["hi"]] if nd else []), dim=1)
        return out, flags_or

    # specs
    @staticmethod
    def get_std_spec(args):
        spec = {
            "sim_start": args.sim_start,
            "sim_step": args.sim_step,
            "env_paths": args.mujoco_model_paths,
            "is_vis": args.vis,
        }
        for extra in ("n_envs", "device", "contact_flag_mode", "check_scene", "tendon_damper", "joint_ids", "tendon_ids", "finger_names", "n_actuated"):
            if hasattr(args, extra):
                spec[extra] = getattr(args, extra)
        return spec
