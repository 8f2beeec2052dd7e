"""ctypes binding of libsoftgrip.so (include/softgrip.h).  There is no CPU fallback: every
compute entry point needs the HIP library and a GPU, and fails loudly otherwise."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsoftgrip.so")
_LIB = None

SG_OK, SG_ERR_INVALID, SG_ERR_MODEL, SG_ERR_NO_DEVICE, SG_ERR_HIP, SG_ERR_NOMEM = 0, -1, -2, -3, -4, -5
# per-env flags (include/softgrip.h: sg_flag)
SG_FLAG_BADQPOS, SG_FLAG_BADQVEL, SG_FLAG_BADQACC, SG_FLAG_CONTACTFULL, SG_FLAG_CNSTRFULL, SG_FLAG_UNSUPPORTED_PAIR = 1, 2, 4, 8, 16, 32
FLAG_BADQPOS, FLAG_BADQVEL, FLAG_BADQACC, FLAG_CONTACTFULL, FLAG_CNSTRFULL, FLAG_UNSUPPORTED_PAIR = 1, 2, 4, 8, 16, 32

# every symbol include/softgrip.h declares (tests/test_abi.py checks the library exports them all)
SYMBOLS = [
    "sg_last_error", "sg_version", "sg_model_create", "sg_model_destroy", "sg_model_nq", "sg_model_nu",
    "sg_model_nsensordata", "sg_model_ntendon", "sg_model_nelem", "sg_batch_create", "sg_batch_destroy",
    "sg_batch_nenvs", "sg_batch_device", "sg_set_stiffness", "sg_set_ctrl", "sg_reset", "sg_step", "sg_get_state",
    "sg_set_state", "sg_get_solver_stats", "sg_set_pipeline", "sg_profile_enable", "sg_profile_read", "sg_profile_read_solver",
    "sg_model_compile", "sg_mjcf_compile", "sg_blob_free", "sg_set_solver_envs_per_wavefront", "sg_solver_envs_per_wavefront",
    "sg_get_touch_words", "sg_model_nboxes", "sg_model_nv", "sg_model_njnt", "sg_tree_workgroups_per_cu",
    "sg_get_poses", "sg_model_nbody", "sg_model_ngeom", "sg_model_default_camera", "sg_render",
    "sg_get_contacts", "sg_model_ncollision_pairs", "sg_model_set_skin", "sg_model_skin", "sg_render_ex", "sg_ray",
    "sg_lstm_forward", "sg_lstm_backward", "sg_get_velocities", "sg_get_tendons", "sg_get_energy",
    "sg_get_mass_matrix", "sg_get_joint_forces", "sg_inverse_dynamics",
    "sg_get_point_motion", "sg_get_jacobians", "sg_model_nsite", "sg_model_sites",
    "sg_solve_mass", "sg_forward_smooth", "sg_get_point_inertia",
    "sg_get_forces", "sg_model_max_rows", "sg_set_forces_workspace",
    "sg_model_skin_closed", "sg_model_skin_root", "sg_model_skin_rest", "sg_model_subtree_mass",
    "sg_get_skin_vertices", "sg_get_shape", "sg_get_subtree",
]
SG_SHAPE_N = 12      # sg_get_shape's doubles per env: V, A, centroid 3, central second moments xx yy zz xy xz yz, dV/dt
SG_RENDER_SKIN = 1
# sg_ray: category bits of cat_mask (ground plane, static, moving finger box, shell element, centre sphere) and flags
SG_RAY_GROUND, SG_RAY_STATIC, SG_RAY_FINGER, SG_RAY_ELEM, SG_RAY_CENTER, SG_RAY_ALL = 1, 2, 4, 8, 16, 31
SG_RAY_PER_ENV = 1
SG_RAY_SKIN = 4
SG_COMPILE_NO_NEIGHBORS, SG_COMPILE_IMPLICIT_TENDON_DAMPER = 1, 2


class SoftgripError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("softgrip error %d: %s" % (code, msg))
        self.code = code


def lib():
    """the product library (soft-grip_amd/libsoftgrip.so; SOFTGRIP_LIB: a profiling / experiment build of it)"""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "libsoftgrip.so is missing (%s).  Build it with `python -c 'import __graft_entry__ as g; g.build()'`; "
                "there is no CPU fallback for the simulator." % LIB_PATH)
        _LIB = load_library(os.environ.get("SOFTGRIP_LIB", LIB_PATH))
    return _LIB


def load_library(path):
    """a build of the library as a configured ctypes handle.  `NativeModel(model, library=...)` binds a model -- and the batches made
    from it -- to another build than the product's (the cross-check tests load the test build with r01's pipelines this way)."""
    import torch  # noqa: F401  -- first: PyTorch-ROCm ships its own HIP runtime, and the process must end up with ONE (loading
    # libsoftgrip.so first would pull in /opt/rocm's copy and torch would then find no devices)
    L = C.CDLL(path)
    vp, dp, ip, i64 = C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong
    L.sg_last_error.restype = C.c_char_p
    L.sg_version.restype = C.c_char_p
    L.sg_model_create.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(vp)]
    L.sg_model_destroy.argtypes = [vp]
    L.sg_model_destroy.restype = None
    L.sg_model_compile.argtypes = [C.c_char_p, C.c_int, C.POINTER(vp)]
    L.sg_mjcf_compile.argtypes = [C.c_char_p, C.c_int, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.sg_blob_free.argtypes = [vp]
    L.sg_blob_free.restype = None
    L.sg_get_touch_words.argtypes = [vp, ip, C.c_int, vp]
    for f in ("sg_model_nq", "sg_model_nv", "sg_model_njnt", "sg_model_nu", "sg_model_nsensordata", "sg_model_ntendon", "sg_model_nelem", "sg_model_nboxes"):
        getattr(L, f).argtypes = [vp]
    L.sg_batch_create.argtypes = [vp, C.c_int, C.c_int, C.POINTER(vp)]
    L.sg_batch_destroy.argtypes = [vp]
    L.sg_batch_destroy.restype = None
    L.sg_batch_nenvs.argtypes = [vp]
    L.sg_batch_device.argtypes = [vp]
    L.sg_set_stiffness.argtypes = [vp, vp, C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int), C.c_int, vp]
    L.sg_set_ctrl.argtypes = [vp, vp, C.c_int, vp]
    L.sg_reset.argtypes = [vp, vp, C.c_int, dp, ip, ip, vp]
    L.sg_step.argtypes = [vp, C.c_int, dp, i64, ip, ip, vp]
    L.sg_get_state.argtypes = [vp, dp, dp, dp, dp, dp, vp]
    L.sg_set_state.argtypes = [vp, dp, dp, dp, dp, dp, vp]
    L.sg_get_solver_stats.argtypes = [vp, ip, ip, ip, vp]
    L.sg_set_pipeline.argtypes = [vp, C.c_int]
    L.sg_set_solver_envs_per_wavefront.argtypes = [vp, C.c_int]
    L.sg_solver_envs_per_wavefront.argtypes = [vp]
    L.sg_tree_workgroups_per_cu.argtypes = [vp]
    L.sg_model_nbody.argtypes = [vp]
    L.sg_model_ngeom.argtypes = [vp]
    L.sg_model_default_camera.argtypes = [vp, C.POINTER(C.c_double)]
    L.sg_get_poses.argtypes = [vp, C.POINTER(C.c_int32), C.c_int, dp, dp, dp, dp, vp]
    L.sg_render.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]
    L.sg_model_set_skin.argtypes = [vp, C.c_int, ip, dp, C.c_int, ip, C.POINTER(C.c_float)]
    L.sg_model_skin.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), ip, dp, ip, C.POINTER(C.c_float)]
    L.sg_render_ex.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]
    L.sg_get_contacts.argtypes = [vp, C.POINTER(C.c_int32), C.c_int, C.c_int, ip, ip, dp, dp, dp, vp]
    L.sg_model_ncollision_pairs.argtypes = [vp]
    L.sg_ray.argtypes = [vp, C.POINTER(C.c_int32), C.c_int, C.c_int, dp, dp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int, C.c_double, C.c_int,
                         dp, ip, dp, vp]
    L.sg_get_velocities.argtypes = [vp, C.POINTER(C.c_int32), C.c_int, dp, dp, dp, vp]
    L.sg_get_tendons.argtypes = [vp, C.POINTER(C.c_int32), C.c_int, dp, dp, vp]
    L.sg_get_energy.argtypes = [vp, C.POINTER(C.c_int32), C.c_int, dp, vp]
    L.sg_get_mass_matrix.argtypes = [vp, C.POINTER(C.c_int32), C.c_int, dp, vp]
    L.sg_get_joint_forces.argtypes = [vp, C.POINTER(C.c_int32), C.c_int, dp, dp, dp, vp]
    L.sg_inverse_dynamics.argtypes = [vp, C.POINTER(C.c_int32), C.c_int, dp, dp, vp]
    L.sg_get_point_motion.argtypes = [vp, C.POINTER(C.c_int32), C.c_int, C.c_int, C.POINTER(C.c_int32), dp, dp, dp, dp, dp, dp, dp, dp, dp, dp, dp, vp]
    L.sg_get_jacobians.argtypes = [vp, C.POINTER(C.c_int32), C.c_int, C.c_int, C.POINTER(C.c_int32), dp, dp, dp, dp, vp]
    L.sg_model_nsite.argtypes = [vp]
    L.sg_model_sites.argtypes = [vp, C.POINTER(C.c_int32), dp, dp]
    L.sg_solve_mass.argtypes = [vp, C.POINTER(C.c_int32), C.c_int, C.c_int, dp, dp, dp, vp]
    L.sg_forward_smooth.argtypes = [vp, C.POINTER(C.c_int32), C.c_int, dp, dp, dp, dp, vp]
    L.sg_get_point_inertia.argtypes = [vp, C.POINTER(C.c_int32), C.c_int, C.c_int, C.POINTER(C.c_int32), dp, dp, dp, vp]
    L.sg_get_forces.argtypes = [vp, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, ip, ip, ip, ip, dp, ip, dp, dp, dp, vp]
    L.sg_model_max_rows.argtypes = [vp]
    L.sg_set_forces_workspace.argtypes = [vp, C.c_size_t]
    L.sg_model_skin_closed.argtypes = [vp]
    L.sg_model_skin_root.argtypes = [vp]
    L.sg_model_skin_rest.argtypes = [vp, C.c_int, dp]
    L.sg_model_subtree_mass.argtypes = [vp, dp]
    L.sg_get_skin_vertices.argtypes = [vp, C.POINTER(C.c_int32), C.c_int, C.c_int, dp, dp, dp, vp]
    L.sg_get_shape.argtypes = [vp, C.POINTER(C.c_int32), C.c_int, C.c_int, dp, C.POINTER(C.c_int32), dp, dp, dp, ip, ip, vp]
    L.sg_get_subtree.argtypes = [vp, C.POINTER(C.c_int32), C.c_int, dp, dp, dp, vp]
    L.sg_lstm_forward.argtypes = [C.c_int, C.c_int, C.c_int, dp, dp, dp, dp, dp, dp, dp, dp, C.c_int, vp]
    L.sg_lstm_backward.argtypes = [C.c_int, C.c_int, C.c_int, dp, dp, dp, dp, dp, dp, dp, dp, dp, vp]
    L.sg_profile_enable.argtypes = [vp, C.c_int]
    L.sg_profile_read.argtypes = [vp, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_longlong)]
    L.sg_profile_read_solver.argtypes = [vp, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_longlong)]
    return L


def check(code, L=None):
    if code != SG_OK:
        raise SoftgripError(code, (L or lib()).sg_last_error().decode())


def compile_mjcf_native(xml_path, composite_neighbors=True, implicit_tendon_damping=False):
    """The library's own MJCF compiler (csrc/sg_mjcf.cpp, ``sg_mjcf_compile``): XML file -> blob bytes.  The Python host uses
    mjcf.py; this is what a caller without Python gets from ``sg_model_compile`` (tests/test_mjcf.py compares the two)."""
    flags = (0 if composite_neighbors else SG_COMPILE_NO_NEIGHBORS) | (SG_COMPILE_IMPLICIT_TENDON_DAMPER if implicit_tendon_damping else 0)
    blob, n = C.c_void_p(), C.c_size_t()
    check(lib().sg_mjcf_compile(os.fsencode(xml_path), flags, C.byref(blob), C.byref(n)))
    try:
        return C.string_at(blob, n.value)
    finally:
        lib().sg_blob_free(blob)


class NativeModel:
    """sg_model handle built from a compiled ``mjcf.Model``."""

    def __init__(self, model, library=None):
        self.model = model
        self.L = L = library or lib()
        blob = model.to_blob()
        self.ptr = C.c_void_p()
        check(L.sg_model_create(blob, len(blob), C.byref(self.ptr)), L)
        self.nq = L.sg_model_nq(self.ptr)
        self.nv = L.sg_model_nv(self.ptr)        # == nq unless the model has a free joint (7 positions, 6 dofs)
        self.nu = L.sg_model_nu(self.ptr)
        self.nsensordata = L.sg_model_nsensordata(self.ptr)
        self.ntendon = L.sg_model_ntendon(self.ptr)
        self.nelem = L.sg_model_nelem(self.ptr)
        self.nboxes = L.sg_model_nboxes(self.ptr)     # moving finger boxes = bits of the contact read-out
        self.nbody = L.sg_model_nbody(self.ptr)
        self.ngeom = L.sg_model_ngeom(self.ptr)
        self.ncollision_pairs = L.sg_model_ncollision_pairs(self.ptr)   # candidate geom pairs of the contact read-out
        if getattr(model, "skin", None) is not None:     # the composite's <skin> (mjcf.py; no part of the blob)
            self.set_skin(model.skin)

    def set_skin(self, skin):
        """attach a skin (sg_model_set_skin): dict of vert_body [nvert] int, vert_pos [nvert, 3] float, face [nface, 3] int, rgba [4];
        None removes it.  Batches of this model show it from their next render(skin=True) on."""
        if skin is None:
            check(self.L.sg_model_set_skin(self.ptr, 0, None, None, 0, None, None), self.L)
            return
        vb = np.ascontiguousarray(skin["vert_body"], dtype=np.int32).reshape(-1)
        vp = np.ascontiguousarray(skin["vert_pos"], dtype=np.float64).reshape(-1, 3)
        fc = np.ascontiguousarray(skin["face"], dtype=np.int32).reshape(-1, 3)
        rgba = np.ascontiguousarray(skin["rgba"], dtype=np.float32).reshape(4)
        if len(vp) != len(vb):
            raise ValueError("skin: vert_pos needs one row per vertex")
        check(self.L.sg_model_set_skin(self.ptr, len(vb), vb.ctypes.data_as(C.c_void_p), vp.ctypes.data_as(C.c_void_p), len(fc),
                                       fc.ctypes.data_as(C.c_void_p), rgba.ctypes.data_as(C.POINTER(C.c_float))), self.L)

    def skin(self):
        """the attached skin as set_skin's dict (sg_model_skin); None without one"""
        nv, nf = C.c_int(), C.c_int()
        check(self.L.sg_model_skin(self.ptr, C.byref(nv), C.byref(nf), None, None, None, None), self.L)
        if nv.value == 0:
            return None
        vb, vp = np.empty(nv.value, np.int32), np.empty((nv.value, 3), np.float64)
        fc, rgba = np.empty((nf.value, 3), np.int32), np.empty(4, np.float32)
        check(self.L.sg_model_skin(self.ptr, None, None, vb.ctypes.data_as(C.c_void_p), vp.ctypes.data_as(C.c_void_p),
                                   fc.ctypes.data_as(C.c_void_p), rgba.ctypes.data_as(C.POINTER(C.c_float))), self.L)
        return dict(vert_body=vb, vert_pos=vp, face=fc, rgba=rgba)

    def _code(self, n):
        if n < -1:      # (-1 is an answer of the skin queries; SG_ERR_INVALID needs a null model, which this handle never is)
            check(n, self.L)
        return n

    def skin_closed(self):
        """1: every directed edge of the skin's faces has its reverse exactly once; 0: not; -1: no skin (sg_model_skin_closed)"""
        return self._code(self.L.sg_model_skin_closed(self.ptr))

    def skin_root(self):
        """the deepest body that is an ancestor of every body the skin's vertices are bound to, "the object"; -1 without a skin"""
        return self._code(self.L.sg_model_skin_root(self.ptr))

    def skin_rest(self, frame_body=-1):
        """[nvert, 3]: the skin's vertices at qpos0 in frame_body's frame (-1: world) (sg_model_skin_rest)"""
        nv = C.c_int()
        check(self.L.sg_model_skin(self.ptr, C.byref(nv), None, None, None, None, None), self.L)
        rest = np.empty((nv.value, 3), np.float64)
        check(self.L.sg_model_skin_rest(self.ptr, int(frame_body), rest.ctypes.data_as(C.c_void_p)), self.L)
        return rest

    def subtree_mass(self):
        """[nbody]: the mass of every body's subtree, row 0 the whole model's (sg_model_subtree_mass)"""
        mass = np.empty(self.nbody, np.float64)
        check(self.L.sg_model_subtree_mass(self.ptr, mass.ctypes.data_as(C.c_void_p)), self.L)
        return mass

    def sites(self):
        """the model's sites as points of NativeBatch.point_motion / jacobians (sg_model_sites): (body [nsite] int32, pos [nsite, 3],
        quat [nsite, 4])"""
        n = self.L.sg_model_nsite(self.ptr)
        body, pos, quat = np.empty(n, np.int32), np.empty((n, 3), np.float64), np.empty((n, 4), np.float64)
        check(self.L.sg_model_sites(self.ptr, body.ctypes.data_as(C.POINTER(C.c_int32)), pos.ctypes.data_as(C.c_void_p), quat.ctypes.data_as(C.c_void_p)), self.L)
        return body, pos, quat

    def default_camera(self):
        """MuJoCo free camera [lookat xyz, distance, azimuth, elevation, fovy] that frames the scene at qpos0 (sg_model_default_camera)"""
        cam = (C.c_double * 7)()
        check(self.L.sg_model_default_camera(self.ptr, cam), self.L)
        return np.array(cam[:], dtype=np.float64)

    def __del__(self):
        if getattr(self, "ptr", None) and getattr(self, "L", None) is not None:
            self.L.sg_model_destroy(self.ptr)
            self.ptr = None


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class NativeBatch:
    """sg_batch handle; all array arguments are torch tensors on the batch's device."""

    def __init__(self, nmodel: NativeModel, n_envs: int, device: int = 0):
        import torch
        self.torch = torch
        self.nmodel, self.n, self.device_index = nmodel, n_envs, device
        self.L = nmodel.L
        self.ptr = C.c_void_p()
        self._check(self.L.sg_batch_create(nmodel.ptr, n_envs, device, C.byref(self.ptr)))
        self.device = torch.device("cuda", device)

    def _check(self, code):
        check(code, self.L)

    def __del__(self):
        if getattr(self, "ptr", None) and getattr(self, "L", None) is not None:
            self.L.sg_batch_destroy(self.ptr)
            self.ptr = None

    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def set_stiffness(self, k, jnt_ids, ten_ids):
        k = np.ascontiguousarray(k, dtype=np.float64)
        assert k.shape == (self.n,)
        ja = (C.c_int * len(jnt_ids))(*jnt_ids)
        ta = (C.c_int * len(ten_ids))(*ten_ids)
        self._check(self.L.sg_set_stiffness(self.ptr, k.ctypes.data_as(C.c_void_p), 1, ja, len(jnt_ids), ta, len(ten_ids), self._stream()))

    def set_ctrl_broadcast(self, ctrl):
        c = np.ascontiguousarray(ctrl, dtype=np.float64)
        assert c.shape == (self.nmodel.nu,)
        self._check(self.L.sg_set_ctrl(self.ptr, c.ctypes.data_as(C.c_void_p), 1, self._stream()))

    def set_ctrl(self, ctrl_t):
        assert ctrl_t.is_cuda and ctrl_t.dtype == self.torch.float64 and ctrl_t.shape == (self.n, self.nmodel.nu) and ctrl_t.is_contiguous()
        self._check(self.L.sg_set_ctrl(self.ptr, _ptr(ctrl_t), 0, self._stream()))

    def reset(self, sim_start, sens=None, flags=None, touch=None, mask=None):
        self._check(self.L.sg_reset(self.ptr, _ptr(mask), sim_start, _ptr(sens), _ptr(flags), _ptr(touch), self._stream()))

    def step(self, n_substeps, sens=None, sens_stride=0, flags=None, touch=None):
        self._check(self.L.sg_step(self.ptr, n_substeps, _ptr(sens), sens_stride, _ptr(flags), _ptr(touch), self._stream()))

    def get_state(self):
        t, m = self.torch, self.nmodel
        kw = dict(dtype=t.float64, device=self.device)
        out = dict(qpos=t.empty(self.n, m.nq, **kw), qvel=t.empty(self.n, m.nv, **kw), act=t.empty(self.n, m.nu, **kw),
                   qacc_warmstart=t.empty(self.n, m.nv, **kw), ctrl=t.empty(self.n, m.nu, **kw))
        self._check(self.L.sg_get_state(self.ptr, _ptr(out["qpos"]), _ptr(out["qvel"]), _ptr(out["act"]), _ptr(out["qacc_warmstart"]),
                                 _ptr(out["ctrl"]), self._stream()))
        return out

    def set_state(self, qpos=None, qvel=None, act=None, qacc_warmstart=None, ctrl=None):
        for x in (qpos, qvel, act, qacc_warmstart, ctrl):
            assert x is None or (x.is_cuda and x.dtype == self.torch.float64 and x.is_contiguous())
        self._check(self.L.sg_set_state(self.ptr, _ptr(qpos), _ptr(qvel), _ptr(act), _ptr(qacc_warmstart), _ptr(ctrl), self._stream()))

    def solver_stats(self):
        t = self.torch
        out = [t.empty(self.n, dtype=t.int32, device=self.device) for _ in range(3)]
        self._check(self.L.sg_get_solver_stats(self.ptr, _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), self._stream()))
        return dict(ncon=out[0], nefc=out[1], iters=out[2])

    def set_pipeline(self, name):
        self._check(self.L.sg_set_pipeline(self.ptr, {"fused": 0, "split": 1, "rows": 2, "tree": 3}[name]))

    def touch_words(self, nwords=2):
        """[n, nwords] int32: bit g of an env's words = moving finger box g touches an object geom (sg_get_touch_words)"""
        t = self.torch
        out = t.empty(self.n, nwords, dtype=t.int32, device=self.device)
        self._check(self.L.sg_get_touch_words(self.ptr, _ptr(out), nwords, self._stream()))
        return out

    def _ids(self, env_ids):
        if env_ids is None:
            return None, self.n
        ids = np.ascontiguousarray(env_ids, dtype=np.int32).reshape(-1)
        return ids, len(ids)

    def poses(self, env_ids=None):
        """mj_kinematics of the listed envs (None: all) on the current state (sg_get_poses): dict of float64 device tensors
        xpos [k, nbody, 3], xquat [k, nbody, 4], geom_xpos [k, ngeom, 3], geom_xmat [k, ngeom, 9]"""
        t, m = self.torch, self.nmodel
        ids, k = self._ids(env_ids)
        kw = dict(dtype=t.float64, device=self.device)
        out = dict(xpos=t.empty(k, m.nbody, 3, **kw), xquat=t.empty(k, m.nbody, 4, **kw), geom_xpos=t.empty(k, m.ngeom, 3, **kw),
                   geom_xmat=t.empty(k, m.ngeom, 9, **kw))
        self._check(self.L.sg_get_poses(self.ptr, None if ids is None else ids.ctypes.data_as(C.POINTER(C.c_int32)), k, _ptr(out["xpos"]),
                                        _ptr(out["xquat"]), _ptr(out["geom_xpos"]), _ptr(out["geom_xmat"]), self._stream()))
        return out

    def velocities(self, env_ids=None):
        """body velocities of the listed envs (None: all) on the current state (sg_get_velocities), world axes: dict of float64 device
        tensors [k, nbody, 3]: ang, the angular velocity; lin, the linear velocity of the body frame's origin (the xpos of poses());
        com_lin, that of the centre of mass.  The time derivative of poses() when qpos moves as qvel says.  A point p fixed on body i
        moves at ``lin[:, i] + torch.cross(ang[:, i], p - xpos[:, i], dim=-1)``."""
        t, m = self.torch, self.nmodel
        ids, k = self._ids(env_ids)
        out = {name: t.empty(k, m.nbody, 3, dtype=t.float64, device=self.device) for name in ("ang", "lin", "com_lin")}
        self._check(self.L.sg_get_velocities(self.ptr, None if ids is None else ids.ctypes.data_as(C.POINTER(C.c_int32)), k, _ptr(out["ang"]),
                                             _ptr(out["lin"]), _ptr(out["com_lin"]), self._stream()))
        return out

    def tendons(self, env_ids=None):
        """tendon lengths and their rates of the listed envs (None: all) on the current state (sg_get_tendons; data.ten_length,
        data.ten_velocity): dict of float64 device tensors length, velocity [k, ntendon]"""
        t, m = self.torch, self.nmodel
        ids, k = self._ids(env_ids)
        out = {name: t.empty(k, m.ntendon, dtype=t.float64, device=self.device) for name in ("length", "velocity")}
        self._check(self.L.sg_get_tendons(self.ptr, None if ids is None else ids.ctypes.data_as(C.POINTER(C.c_int32)), k, _ptr(out["length"]),
                                          _ptr(out["velocity"]), self._stream()))
        return out

    def energy(self, env_ids=None, out=None):
        """the energy of the listed envs (None: all) on the current state (sg_get_energy): float64 device tensor [k, 4] = gravity, joint
        springs, tendon springs (each env at the stiffness its next step uses), kinetic; data.energy is (the sum of the first three,
        the fourth).  out: a contiguous [k, 4] tensor to fill."""
        t = self.torch
        ids, k = self._ids(env_ids)
        if out is None:
            out = t.empty(k, 4, dtype=t.float64, device=self.device)
        assert out.is_cuda and out.dtype == t.float64 and out.is_contiguous() and out.shape == (k, 4)
        self._check(self.L.sg_get_energy(self.ptr, None if ids is None else ids.ctypes.data_as(C.POINTER(C.c_int32)), k, _ptr(out), self._stream()))
        return out

    def mass_matrix(self, env_ids=None):
        """the joint-space mass matrix of the listed envs (None: all) on the current state (sg_get_mass_matrix; mj_fullM(data.qM)):
        float64 device tensor [k, nv, nv], dense and symmetric to the bit.  nv * nv * 8 bytes per env: list fewer envs per call
        where memory is short."""
        t = self.torch
        ids, k = self._ids(env_ids)
        nv = self.nmodel.nv
        out = t.empty(k, nv, nv, dtype=t.float64, device=self.device)
        self._check(self.L.sg_get_mass_matrix(self.ptr, None if ids is None else ids.ctypes.data_as(C.POINTER(C.c_int32)), k, _ptr(out), self._stream()))
        return out

    def joint_forces(self, env_ids=None):
        """the smooth joint-space forces of the listed envs (None: all) on the current state (sg_get_joint_forces): dict of float64
        device tensors [k, nv]: bias (data.qfrc_bias: Coriolis, centrifugal and gravity terms, on the left-hand side), passive
        (data.qfrc_passive: springs at the stiffness the env's next step uses, dampers, the tendon damper also where the model
        integrates it implicitly), actuator (data.qfrc_actuator at the current activation)."""
        t = self.torch
        ids, k = self._ids(env_ids)
        out = {name: t.empty(k, self.nmodel.nv, dtype=t.float64, device=self.device) for name in ("bias", "passive", "actuator")}
        self._check(self.L.sg_get_joint_forces(self.ptr, None if ids is None else ids.ctypes.data_as(C.POINTER(C.c_int32)), k, _ptr(out["bias"]),
                                               _ptr(out["passive"]), _ptr(out["actuator"]), self._stream()))
        return out

    def inverse_dynamics(self, qacc, env_ids=None):
        """mj_inverse of the listed envs (None: all) on the current state (sg_inverse_dynamics): qacc, a float64 device tensor [k, nv]
        (row i: the i-th listed env's acceleration) -> qfrc_inverse [k, nv] = M qacc + bias - passive, one Newton-Euler pass.
        ``inverse_dynamics(qacc) - joint_forces()["actuator"]`` is the generalised force the constraints must have applied."""
        t = self.torch
        ids, k = self._ids(env_ids)
        nv = self.nmodel.nv
        assert qacc.is_cuda and qacc.dtype == t.float64 and qacc.is_contiguous() and qacc.shape == (k, nv)
        out = t.empty(k, nv, dtype=t.float64, device=self.device)
        self._check(self.L.sg_inverse_dynamics(self.ptr, None if ids is None else ids.ctypes.data_as(C.POINTER(C.c_int32)), k, _ptr(qacc), _ptr(out),
                                               self._stream()))
        return out

    def _points(self, body, pos, quat):
        """the host arrays of a point list: body [P] int32, pos [P, 3], quat [P, 4] or None"""
        body = np.ascontiguousarray(body, dtype=np.int32).reshape(-1)
        pos = np.ascontiguousarray(pos, dtype=np.float64).reshape(-1, 3)
        if len(pos) != len(body):
            raise ValueError("points: pos needs one row per body id")
        if quat is not None:
            quat = np.ascontiguousarray(quat, dtype=np.float64).reshape(-1, 4)
            if len(quat) != len(body):
                raise ValueError("points: quat needs one row per body id")
        return body, pos, quat

    def _rows(self, x, k, n):
        assert x is None or (x.is_cuda and x.dtype == self.torch.float64 and x.is_contiguous() and x.shape == (k, n))
        return _ptr(x)

    def point_motion(self, body, pos, quat=None, qpos=None, qvel=None, qacc=None, env_ids=None, outputs=None):
        """pose, velocity and acceleration of body-fixed points and the gyro / accelerometer readings there (sg_get_point_motion).
        Points: body [P] (0 is the world), pos [P, 3] in the body's frame, quat [P, 4] the probe's frame in the body's (None:
        identity; normalised by the call) -- host arrays; a site's site_bodyid, site_pos, site_quat is that site.  qpos [k, nq], qvel
        [k, nv], qacc [k, nv]: float64 device tensors, row i the i-th listed env's (None: the batch's current qpos / qvel, qacc zero).
        Returns a dict of float64 device tensors, world axes: pos [k, P, 3], mat [k, P, 3, 3] (the probe's frame), vel [k, P, 6]
        (angular, then linear of the material point), acc [k, P, 6] (kinematic, without gravity), gyro [k, P, 3] = mat' ang, accel
        [k, P, 3] = mat' (a - gravity).  outputs: the names wanted (None: all)."""
        t, m = self.torch, self.nmodel
        ids, k = self._ids(env_ids)
        body, pos, quat = self._points(body, pos, quat)
        P = len(body)
        shapes = dict(pos=(3,), mat=(3, 3), vel=(6,), acc=(6,), gyro=(3,), accel=(3,))
        out = {n: t.empty((k, P) + shapes[n], dtype=t.float64, device=self.device) for n in (shapes if outputs is None else outputs)}
        vp = C.c_void_p
        self._check(self.L.sg_get_point_motion(self.ptr, None if ids is None else ids.ctypes.data_as(C.POINTER(C.c_int32)), k, P,
                                               body.ctypes.data_as(C.POINTER(C.c_int32)), pos.ctypes.data_as(vp), None if quat is None else quat.ctypes.data_as(vp),
                                               self._rows(qpos, k, m.nq), self._rows(qvel, k, m.nv), self._rows(qacc, k, m.nv),
                                               *[_ptr(out.get(n)) for n in shapes], self._stream()))
        return out

    def jacobians(self, body, pos, qpos=None, env_ids=None):
        """the Jacobians of body-fixed points (sg_get_jacobians; mj_jac): points as in point_motion, qpos [k, nq] (None: the batch's
        current one) -> dict of float64 device tensors jacp, jacr [k, P, 3, nv], every entry written.  Column d is dof d's effect
        under velocities()' dof conventions, so ``jacp @ qvel`` is the point's linear and ``jacr @ qvel`` its angular velocity."""
        t, m = self.torch, self.nmodel
        ids, k = self._ids(env_ids)
        body, pos, _ = self._points(body, pos, None)
        P = len(body)
        out = {n: t.empty(k, P, 3, m.nv, dtype=t.float64, device=self.device) for n in ("jacp", "jacr")}
        self._check(self.L.sg_get_jacobians(self.ptr, None if ids is None else ids.ctypes.data_as(C.POINTER(C.c_int32)), k, P,
                                            body.ctypes.data_as(C.POINTER(C.c_int32)), pos.ctypes.data_as(C.c_void_p), self._rows(qpos, k, m.nq),
                                            _ptr(out["jacp"]), _ptr(out["jacr"]), self._stream()))
        return out

    def solve_mass(self, y, env_ids=None, out=None):
        """x = M^-1 y of the listed envs (None: all) on the current state (sg_solve_mass; mj_solveM): y, a float64 device tensor
        [k, R, nv] (or [k, nv]: one right-hand side), row i the i-th listed env's -> (x, pivot): x of y's shape, pivot [k] = min D_i /
        M_ii of the factor M = L' D L (1 for a diagonal M, towards 0 as M nears singularity; an env whose pivot is NaN or <= 0 has NaN
        in x).  out: a contiguous tensor of y's shape to fill; it may be y itself."""
        t = self.torch
        ids, k = self._ids(env_ids)
        nv = self.nmodel.nv
        assert y.is_cuda and y.dtype == t.float64 and y.is_contiguous() and y.shape[0] == k and y.shape[-1] == nv and y.dim() in (2, 3)
        if out is None:
            out = t.empty_like(y)
        assert out.is_cuda and out.dtype == t.float64 and out.is_contiguous() and out.shape == y.shape
        pivot = t.empty(k, dtype=t.float64, device=self.device)
        self._check(self.L.sg_solve_mass(self.ptr, None if ids is None else ids.ctypes.data_as(C.POINTER(C.c_int32)), k, 1 if y.dim() == 2 else y.shape[1],
                                         _ptr(y), _ptr(out), _ptr(pivot), self._stream()))
        return out, pivot

    def forward_smooth(self, qfrc_applied=None, env_ids=None):
        """the smooth forward dynamics of the listed envs (None: all) on the current state (sg_forward_smooth; mj_fwdAcceleration):
        dict of float64 device tensors qfrc_smooth [k, nv] = passive + actuator + qfrc_applied - bias (joint_forces()' arrays;
        qfrc_applied [k, nv] on the device, None: zero), qacc_smooth [k, nv] = M^-1 qfrc_smooth, the acceleration without contacts,
        equalities and limits, and pivot [k] as in solve_mass.  ``inverse_dynamics(qacc_smooth) = actuator + qfrc_applied``."""
        t = self.torch
        ids, k = self._ids(env_ids)
        nv = self.nmodel.nv
        out = {name: t.empty(k, nv, dtype=t.float64, device=self.device) for name in ("qacc_smooth", "qfrc_smooth")}
        out["pivot"] = t.empty(k, dtype=t.float64, device=self.device)
        self._check(self.L.sg_forward_smooth(self.ptr, None if ids is None else ids.ctypes.data_as(C.POINTER(C.c_int32)), k, self._rows(qfrc_applied, k, nv),
                                             _ptr(out["qacc_smooth"]), _ptr(out["qfrc_smooth"]), _ptr(out["pivot"]), self._stream()))
        return out

    def point_inertia(self, body, pos, env_ids=None):
        """the inverse inertia seen at body-fixed points (sg_get_point_inertia): points as in jacobians() -> (W, pivot): W [k, P, 6, 6]
        = J M^-1 J' with J = (jacr; jacp), angular rows first, symmetric to the bit, zero for a point on the world; pivot [k] as in
        solve_mass.  ``1 / (n @ W[e, p, 3:, 3:] @ n)`` is the effective mass along a unit vector n."""
        t = self.torch
        ids, k = self._ids(env_ids)
        body, pos, _ = self._points(body, pos, None)
        P = len(body)
        W = t.empty(k, P, 6, 6, dtype=t.float64, device=self.device)
        pivot = t.empty(k, dtype=t.float64, device=self.device)
        self._check(self.L.sg_get_point_inertia(self.ptr, None if ids is None else ids.ctypes.data_as(C.POINTER(C.c_int32)), k, P,
                                                body.ctypes.data_as(C.POINTER(C.c_int32)), pos.ctypes.data_as(C.c_void_p), _ptr(W), _ptr(pivot), self._stream()))
        return W, pivot

    def forces(self, env_ids=None, max_rows=None, max_contacts=256):
        """mj_forward's constraint stage of the listed envs (None: all) on the current state (sg_get_forces): dict of device tensors
        nefc, iters, ncon [k] int32 (nefc may exceed max_rows; nefc = ncon = -1: the env's state is not finite, its double outputs are
        NaN), efc_type, efc_id [k, max_rows] int32 and efc_force [k, max_rows] float64 (the first min(nefc, max_rows) rows in
        mj_makeConstraint's order: type 0 equality, 3 limit, 5 frictionless contact, 7 elliptic contact; id the equality, the joint or the
        contact's index in contacts()' list), contact_force [k, max_contacts, 3] (contact i's force in its own frame, normal first),
        qfrc_constraint [k, nv] = J' f and qacc [k, nv], data.qacc after mj_forward.  max_rows=None: the model's row capacity
        (sg_model_max_rows).  The slots past the written ones are zero.  Nothing in the batch changes."""
        t = self.torch
        ids, k = self._ids(env_ids)
        nv = self.nmodel.nv
        mr = self.max_rows() if max_rows is None else int(max_rows)
        mc = int(max_contacts)
        i32 = dict(dtype=t.int32, device=self.device)
        f64 = dict(dtype=t.float64, device=self.device)
        out = dict(nefc=t.zeros(k, **i32), iters=t.zeros(k, **i32), ncon=t.zeros(k, **i32), efc_type=t.zeros(k, mr, **i32), efc_id=t.zeros(k, mr, **i32),
                   efc_force=t.zeros(k, mr, **f64), contact_force=t.zeros(k, mc, 3, **f64), qfrc_constraint=t.zeros(k, nv, **f64), qacc=t.zeros(k, nv, **f64))
        self._check(self.L.sg_get_forces(self.ptr, None if ids is None else ids.ctypes.data_as(C.POINTER(C.c_int32)), k, mr, mc, _ptr(out["nefc"]), _ptr(out["iters"]),
                                         _ptr(out["efc_type"]), _ptr(out["efc_id"]), _ptr(out["efc_force"]), _ptr(out["ncon"]), _ptr(out["contact_force"]),
                                         _ptr(out["qfrc_constraint"]), _ptr(out["qacc"]), self._stream()))
        return out

    def max_rows(self):
        """the constraint rows sg_get_forces reserves per env (sg_model_max_rows)"""
        n = self.L.sg_model_max_rows(self.nmodel.ptr)
        if n < 0:
            self._check(n)
        return n

    def set_forces_workspace(self, nbytes):
        """caps the device work space of forces() (sg_set_forces_workspace; the env list is processed in chunks that fit)"""
        self._check(self.L.sg_set_forces_workspace(self.ptr, C.c_size_t(int(nbytes))))

    def _need_skin(self):
        """a model without a skin gets ``model.composite_skin()`` attached first, as raycast(skin=True) does"""
        if self.nmodel.skin() is None and hasattr(self.nmodel.model, "composite_skin"):
            made = self.nmodel.model.composite_skin()
            if made is not None:
                self.nmodel.set_skin(made)

    def nvert(self):
        """the vertices of the model's skin (0: none)"""
        nv = C.c_int()
        self._check(self.L.sg_model_skin(self.nmodel.ptr, C.byref(nv), None, None, None, None, None))
        return nv.value

    def skin_vertices(self, frame_body=-1, env_ids=None, outputs=None):
        """the skin's vertices of the listed envs (None: all) on the current state (sg_get_skin_vertices): dict of float64 device tensors
        [k, nvert, 3]: pos (world), vel (the material point's velocity, world axes), local (pos in frame_body's frame; -1: equal to
        pos).  outputs: the names wanted (None: all)."""
        t = self.torch
        self._need_skin()
        ids, k = self._ids(env_ids)
        names = ("pos", "vel", "local")
        out = {n: t.empty(k, self.nvert(), 3, dtype=t.float64, device=self.device) for n in (names if outputs is None else outputs)}
        self._check(self.L.sg_get_skin_vertices(self.ptr, None if ids is None else ids.ctypes.data_as(C.POINTER(C.c_int32)), k, int(frame_body),
                                                *[_ptr(out.get(n)) for n in names], self._stream()))
        return out

    def shape(self, dirs=None, dir_body=None, env_ids=None, shape=True):
        """the soft object's shape of the listed envs (None: all) on the current state (sg_get_shape): dict of device tensors shape
        [k, 12] float64 = volume, area, centroid (3), central second moments xx yy zz xy xz yz, dV/dt (closed skins only; shape=False
        leaves it out); and for dirs [D, 3] (host; need not be unit) given in the frames of dir_body [D] (host ints, -1 / None: world)
        lo, hi [k, D] float64, the object's extent along each, and lo_vert, hi_vert [k, D] int32, the vertices attaining them."""
        t = self.torch
        self._need_skin()
        ids, k = self._ids(env_ids)
        hd = None if dirs is None else np.ascontiguousarray(dirs, dtype=np.float64).reshape(-1, 3)
        nd = 0 if hd is None else len(hd)
        hb = None if dir_body is None or nd == 0 else np.ascontiguousarray(dir_body, dtype=np.int32).reshape(-1)
        assert hb is None or len(hb) == nd
        f64, i32 = dict(dtype=t.float64, device=self.device), dict(dtype=t.int32, device=self.device)
        res = {}
        if shape:
            res["shape"] = t.empty(k, SG_SHAPE_N, **f64)
        if nd:
            res.update(lo=t.empty(k, nd, **f64), hi=t.empty(k, nd, **f64), lo_vert=t.empty(k, nd, **i32), hi_vert=t.empty(k, nd, **i32))
        self._check(self.L.sg_get_shape(self.ptr, None if ids is None else ids.ctypes.data_as(C.POINTER(C.c_int32)), k, nd,
                                        None if nd == 0 else hd.ctypes.data_as(C.c_void_p), None if hb is None else hb.ctypes.data_as(C.POINTER(C.c_int32)),
                                        _ptr(res.get("shape")), _ptr(res.get("lo")), _ptr(res.get("hi")), _ptr(res.get("lo_vert")), _ptr(res.get("hi_vert")),
                                        self._stream()))
        return res

    def subtree(self, env_ids=None):
        """the body-tree sums of the listed envs (None: all) on the current state (sg_get_subtree; data.subtree_com, mj_subtreeVel):
        dict of float64 device tensors [k, nbody, 3], row i over body i and its descendants: com, linvel (of that centre of mass) and
        angmom (about it, world axes).  Row 0 is the whole model."""
        t = self.torch
        ids, k = self._ids(env_ids)
        out = {n: t.empty(k, self.nmodel.nbody, 3, dtype=t.float64, device=self.device) for n in ("com", "linvel", "angmom")}
        self._check(self.L.sg_get_subtree(self.ptr, None if ids is None else ids.ctypes.data_as(C.POINTER(C.c_int32)), k, _ptr(out["com"]), _ptr(out["linvel"]),
                                          _ptr(out["angmom"]), self._stream()))
        return out

    def contacts(self, env_ids=None, max_contacts=256):
        """mj_collision of the listed envs (None: all) on the current state (sg_get_contacts): dict of device tensors ncon [k] int32
        (the full count, may exceed max_contacts; -1: the env's qpos is not finite), geom [k, max_contacts, 2] int32, dist
        [k, max_contacts], pos [k, max_contacts, 3], frame [k, max_contacts, 9] float64.  Rows hold the first min(ncon, max_contacts)
        contacts in mj_collision's order; the slots past them are zero (the tensors start zeroed, the call writes nothing there)."""
        t = self.torch
        ids, k = self._ids(env_ids)
        mc = int(max_contacts)
        kw = dict(dtype=t.float64, device=self.device)
        out = dict(ncon=t.zeros(k, dtype=t.int32, device=self.device), geom=t.zeros(k, mc, 2, dtype=t.int32, device=self.device),
                   dist=t.zeros(k, mc, **kw), pos=t.zeros(k, mc, 3, **kw), frame=t.zeros(k, mc, 9, **kw))
        self.contacts_into(out, env_ids)
        return out

    def contacts_into(self, out, env_ids=None):
        """sg_get_contacts into caller-owned tensors: `out` maps any of ncon / geom / dist / pos / frame to contiguous device tensors of
        the shapes contacts() returns (max_contacts is read off the contact arrays; slots past an env's count keep their contents)"""
        t = self.torch
        ids, k = self._ids(env_ids)
        mc = 0
        for name, tail, dt in (("ncon", (), t.int32), ("geom", (2,), t.int32), ("dist", (), t.float64), ("pos", (3,), t.float64), ("frame", (9,), t.float64)):
            x = out.get(name)
            if x is None:
                continue
            assert x.is_cuda and x.dtype == dt and x.is_contiguous() and x.shape[0] == k, name
            if name != "ncon":
                assert x.shape[2:] == tail and (mc == 0 or x.shape[1] == mc), name
                mc = x.shape[1]
        self._check(self.L.sg_get_contacts(self.ptr, None if ids is None else ids.ctypes.data_as(C.POINTER(C.c_int32)), k, mc, _ptr(out.get("ncon")),
                                           _ptr(out.get("geom")), _ptr(out.get("dist")), _ptr(out.get("pos")), _ptr(out.get("frame")), self._stream()))

    def raycast(self, origin, direction, body=None, exclude=None, env_ids=None, cat_mask=SG_RAY_ALL, max_dist=0.0, normals=False, skin=False):
        """mj_ray for the listed envs (None: all) on the current state (sg_ray).  origin / direction: float64 device tensors [R, 3] --
        the same rays for every env -- or [k, R, 3], rays of their own per listed env; directions need not be unit.  body / exclude:
        R ints (host) or None: the body whose frame ray r is given in and follows (-1: world) and the body whose geoms it does not see
        (-1: none).  cat_mask: SG_RAY_* bits of the geom categories that are candidates; max_dist <= 0: unlimited.  Returns a dict of
        device tensors dist [k, R] float64 (metres, -1: miss), geom [k, R] int32 (-1: miss) and, with normals=True, normal [k, R, 3]
        (outward, world axes, zeros for a miss).  Entry hits only: an origin inside a geom does not see that geom.  An env whose qpos
        is not finite gets NaN / -1.

        skin=True (SG_RAY_SKIN): the rays see the soft object as its skin and not as its element geoms; a model without one gets
        ``model.composite_skin()`` attached first, and the call is the plain one when there is none.  The skin's triangles are
        candidates when cat_mask holds SG_RAY_ELEM; the geoms of the bodies its vertices are bound to never are; exclude[r] also
        removes the triangles with a vertex bound to that body.  Front faces only (counter-clockwise seen from outside, t > 0: an
        origin inside the closed skin sees nothing of it), watertight on shared edges and vertices.  ``geom`` is then the raw id --
        ngeom + face index on the skin, where a geom wins a tie against a triangle and the smaller face index among triangles --
        ``normal`` the flat unit face normal there, and the dict gains ``face`` [k, R] int32: geom - ngeom on skin hits, -1 elsewhere."""
        t = self.torch
        if skin and self.nmodel.skin() is None and hasattr(self.nmodel.model, "composite_skin"):
            made = self.nmodel.model.composite_skin()
            if made is not None:
                self.nmodel.set_skin(made)
        ids, k = self._ids(env_ids)
        assert origin.is_cuda and direction.is_cuda and origin.dtype == t.float64 and direction.dtype == t.float64
        assert origin.shape == direction.shape and origin.shape[-1] == 3 and origin.dim() in (2, 3), origin.shape
        per_env = origin.dim() == 3
        assert not per_env or origin.shape[0] == k, (origin.shape, k)
        origin, direction = origin.contiguous(), direction.contiguous()
        nr = origin.shape[-2]
        hb = None if body is None else np.ascontiguousarray(body, dtype=np.int32).reshape(-1)
        hx = None if exclude is None else np.ascontiguousarray(exclude, dtype=np.int32).reshape(-1)
        assert (hb is None or len(hb) == nr) and (hx is None or len(hx) == nr)
        out = dict(dist=t.empty(k, nr, dtype=t.float64, device=self.device), geom=t.empty(k, nr, dtype=t.int32, device=self.device))
        if normals:
            out["normal"] = t.empty(k, nr, 3, dtype=t.float64, device=self.device)
        i32 = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
        self._check(self.L.sg_ray(self.ptr, i32(ids), k, nr, _ptr(origin), _ptr(direction), i32(hb), i32(hx), int(cat_mask), float(max_dist),
                                  (SG_RAY_PER_ENV if per_env else 0) | (SG_RAY_SKIN if skin else 0), _ptr(out["dist"]), _ptr(out["geom"]),
                                  _ptr(out.get("normal")), self._stream()))
        if skin:
            ng = self.nmodel.ngeom
            out["face"] = t.where(out["geom"] >= ng, out["geom"] - ng, t.full_like(out["geom"], -1))
        return out

    def render(self, camera=None, env_ids=None, width=320, height=240, rgb=True, depth=True, seg=True, skin=False):
        """ray-cast images of the listed envs (None: all) on the current state (sg_render): dict of device tensors rgba [k, H, W, 4]
        uint8 with its view rgb [..., :3], depth [k, H, W] float32 (+inf = background), seg [k, H, W] int32 (geom id, -1 = background).
        camera: 7 numbers (lookat xyz, distance, azimuth, elevation, fovy); None = the model's default camera.
        skin=True (sg_render_ex, SG_RENDER_SKIN): the soft object is drawn as its skin -- seg reports ngeom there -- and not as its
        element geoms; a model without one gets ``model.composite_skin()`` attached first, and renders as before when there is none."""
        t = self.torch
        if skin and self.nmodel.skin() is None and hasattr(self.nmodel.model, "composite_skin"):
            made = self.nmodel.model.composite_skin()
            if made is not None:
                self.nmodel.set_skin(made)
        cam = np.ascontiguousarray(self.nmodel.default_camera() if camera is None else camera, dtype=np.float64).reshape(7)
        ids, k = self._ids(env_ids)
        out = {}
        if rgb:
            out["rgba"] = t.empty(k, height, width, 4, dtype=t.uint8, device=self.device)
            out["rgb"] = out["rgba"][..., :3]
        if depth:
            out["depth"] = t.empty(k, height, width, dtype=t.float32, device=self.device)
        if seg:
            out["seg"] = t.empty(k, height, width, dtype=t.int32, device=self.device)
        args = (_ptr(out.get("rgba")), _ptr(out.get("depth")), _ptr(out.get("seg")), self._stream())
        head = (self.ptr, cam.ctypes.data_as(C.POINTER(C.c_double)), None if ids is None else ids.ctypes.data_as(C.POINTER(C.c_int32)), k,
                int(width), int(height))
        if skin:
            self._check(self.L.sg_render_ex(*head, SG_RENDER_SKIN, *args))
        else:
            self._check(self.L.sg_render(*head, *args))
        return out

    def set_solver_envs_per_wavefront(self, epw):
        self._check(self.L.sg_set_solver_envs_per_wavefront(self.ptr, int(epw)))

    def solver_envs_per_wavefront(self):
        return self.L.sg_solver_envs_per_wavefront(self.ptr)

    def tree_workgroups_per_cu(self):
        """tree pipeline: workgroups (= envs) per CU the runtime grants the kernel with this model's LDS block; 0 on the rows pipeline"""
        return self.L.sg_tree_workgroups_per_cu(self.ptr)

    def profile_enable(self, on=True):
        self._check(self.L.sg_profile_enable(self.ptr, int(on)))

    def profile_read(self, reset=True):
        ms, n = C.c_double(), C.c_longlong()
        self._check(self.L.sg_profile_read(self.ptr, int(reset), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def profile_read_solver(self, reset=True):
        ms, n = C.c_double(), C.c_longlong()
        self._check(self.L.sg_profile_read_solver(self.ptr, int(reset), C.byref(ms), C.byref(n)))
        return ms.value, n.value
