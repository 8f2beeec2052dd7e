"""Helpers of the soft object's read-out tests (sg_get_skin_vertices, sg_get_shape, sg_get_subtree; csrc/sg_shape.h):

  * reference(): a NumPy (fp64) restatement written from the definitions of include/softgrip.h, NOT from the header: Model.kinematics()
    for the poses, dyn_ref.reference() for the twists, Model.composite_skin() (or any skin dict) for the mesh;
  * bounds(): the tolerances, spelled out below;
  * build_host() / Host: the g++ build of csrc/sg_shape.h and the table builder of csrc/sg_tables.cpp, run one env at a time in the
    kernel's order (sgh_host_env);
  * the synthetic skins the tests share: the tetrahedron, a box, the 10 x 8 x 5 box-grid shell at the vertex limit.

Tolerances (dyn_ref's: n eps with two orders of margin).
  ARR = 1e-12 max(1, max |value|) for the per-vertex and per-body arrays pos, vel, local -- and lo, hi, which are one vertex's height.
  REL = 1e-11 times the sum of the absolute values of a sum's summands for the sums: V, A, dV/dt, the first and second moments about
  p0 (F, S), a subtree's sum m xipos, sum m com_lin and angmom.
  The quotients take the first-order propagation of those:
    centroid c = p0 + F / V:          d c_a  = ARR(pos) + dF_a / |V| + |F_a| dV / V^2
    central moments C = S - F F' / V: d C_ab = dS_ab + (|F_a| dF_b + |F_b| dF_a) / |V| + |F_a F_b| dV / V^2
    com = sum m x / M:                d com  = REL sum |m x| / M + REL |com| + ARR(xipos)      (REL |com|: M is a sum itself; the
                                      last term: a weighted mean of values that each carry the per-body array bound)
    linvel likewise with com_lin; angmom = sum (R I R' w + m r x v), r = xipos - com, takes REL times the sum of the absolute values
    of its summands plus what the per-body bounds and the com's own bound do to them:
                                      sum (|I|_F ARR(ang) + m (|r|_1 ARR(com_lin) + |v|_1 (ARR(xipos) + max d com)))
    A massless subtree's row is the body's own xipos and com velocity (the array bounds) and an exact zero.
"""
import ctypes as C

import numpy as np

import dyn_ref as DR
import host_build

REL, ARR = DR.REL, DR.ARR
SHAPE_N = 12
PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))      # xx yy zz xy xz yz
SCENES_SKIN = ("softbox", "softbox_fix", "softball", "softball_fix", "softcylinder", "softcylinder_fix", "fourfinger_softball", "fourfinger_softball_fix",
               "freeball", "freeball_fix")


def load(scene):
    import softgrip_amd as sg
    from helpers import model_path
    return DR.load(scene) if scene in DR.SCENES else sg.load_model(model_path(scene), None if scene.startswith("softbox") else "implicit")


# ---- the NumPy reference ----
def mesh_integrals(P, Vel, face):
    """the integrals of a closed mesh about p0 = P[0] from the definitions: dict of V, A, F [3], S [6], rate and the sums of the absolute
    values of their summands (absV ...), each already divided as the value is"""
    a, b, c = (P[face[:, k]] - P[0] for k in range(3))
    va, vb, vc = (Vel[face[:, k]] - Vel[0] for k in range(3))
    bc = np.cross(b, c)
    det = np.einsum("fi,fi->f", a, bc)
    s = a + b + c
    area = np.linalg.norm(np.cross(b - a, c - a), axis=1)
    fm = det[:, None] * s
    sm = np.stack([det * (a[:, x] * a[:, y] + b[:, x] * b[:, y] + c[:, x] * c[:, y] + s[:, x] * s[:, y]) for x, y in PAIRS], axis=1)
    r = np.einsum("fi,fi->f", va, bc) + np.einsum("fi,fi->f", a, np.cross(vb, c)) + np.einsum("fi,fi->f", a, np.cross(b, vc))
    return dict(V=det.sum() / 6, A=area.sum() / 2, F=fm.sum(0) / 24, S=sm.sum(0) / 120, rate=r.sum() / 6,
                absV=np.abs(det).sum() / 6, absA=area.sum() / 2, absF=np.abs(fm).sum(0) / 24, absS=np.abs(sm).sum(0) / 120, absrate=np.abs(r).sum() / 6)


def shape_of(I, p0):
    """[12] from mesh_integrals' dict: V, A, centroid, central second moments, dV/dt"""
    cm = I["F"] / I["V"]
    C6 = np.array([I["S"][q] - I["F"][x] * I["F"][y] / I["V"] for q, (x, y) in enumerate(PAIRS)])
    return np.concatenate([[I["V"], I["A"]], p0 + cm, C6, [I["rate"]]])


def shape_bound(I, P):
    """[12]: the bound of every slot of shape_of (module docstring)"""
    dV, dA, dF, dS, dr = REL * I["absV"], REL * I["absA"], REL * I["absF"], REL * I["absS"], REL * I["absrate"]
    V, F = abs(I["V"]), np.abs(I["F"])
    dc = ARR * max(1.0, np.abs(P).max()) + dF / V + F * dV / V ** 2
    dC = np.array([dS[q] + (F[x] * dF[y] + F[y] * dF[x]) / V + F[x] * F[y] * dV / V ** 2 for q, (x, y) in enumerate(PAIRS)])
    return np.concatenate([[dV, dA], dc, dC, [dr]])


def subtree_lists(m):
    """per body the ascending list of itself and its descendants"""
    sub = [[] for _ in range(m.nbody)]
    for j in range(m.nbody):
        i = j
        while True:
            sub[i].append(j)
            if i == 0:
                break
            i = int(m.body_parentid[i])
    return sub


def reference(m, skin, qpos, qvel, frame_body=-1, dirs=None, dir_body=None):
    """every output of the three calls for one state, with the bounds of the sums and quotients beside them (``bound_*``).  skin: a
    composite_skin() dict or None (then only the subtree rows)"""
    d = DR.reference(m, qpos, qvel)
    kin = d["kin"]
    out = dict(dyn=d)
    if skin is not None:
        vb, vp, face = np.asarray(skin["vert_body"]), np.asarray(skin["vert_pos"], np.float64), np.asarray(skin["face"])
        P = kin["xpos"][vb] + np.einsum("vij,vj->vi", kin["xmat"][vb], vp)
        Vel = d["lin"][vb] + np.cross(d["ang"][vb], P - kin["xpos"][vb])
        local = P if frame_body < 0 else (P - kin["xpos"][frame_body]) @ kin["xmat"][frame_body]
        out.update(pos=P, vel=Vel, local=local)
        I = mesh_integrals(P, Vel, face)
        out["integrals"] = I
        if I["V"] != 0:
            out.update(shape=shape_of(I, P[0]), bound_shape=shape_bound(I, P))
        if dirs is not None:
            dirs = np.asarray(dirs, np.float64).reshape(-1, 3)
            db = -np.ones(len(dirs), int) if dir_body is None else np.asarray(dir_body)
            H, dw, og = np.zeros((len(dirs), len(P))), np.zeros((len(dirs), 3)), np.zeros((len(dirs), 3))
            for j, (u, b) in enumerate(zip(dirs, db)):
                u = u / np.linalg.norm(u)
                dw[j], og[j] = (u, 0.0) if b < 0 else (kin["xmat"][b] @ u, kin["xpos"][b])
                H[j] = (P - og[j]) @ dw[j]
            out.update(heights=H, lo=H.min(1), hi=H.max(1), lo_vert=H.argmin(1), hi_vert=H.argmax(1), dir_world=dw, dir_origin=og)
    nb = m.nbody
    mass, xi, vc = np.asarray(m.body_mass, np.float64), d["xipos"], d["com_lin"]
    com, linvel, angmom = np.zeros((nb, 3)), np.zeros((nb, 3)), np.zeros((nb, 3))
    bcom, blin, bang = np.zeros((nb, 3)), np.zeros((nb, 3)), np.zeros((nb, 3))
    spin = np.zeros((nb, 3))
    for b in range(1, nb):
        R = kin["xmat"][b]
        spin[b] = R @ np.reshape(m.body_imat[b], (3, 3)) @ R.T @ d["ang"][b]
    xi0 = xi.copy()
    xi0[0] = kin["xpos"][0] + kin["xmat"][0] @ np.asarray(m.body_ipos[0])
    dx, dv, dw = (ARR * max(1.0, np.abs(a).max()) for a in (xi0, vc, d["ang"]))
    inorm = np.array([np.linalg.norm(np.reshape(m.body_imat[b], (3, 3))) for b in range(nb)])
    for i, lst in enumerate(subtree_lists(m)):
        M = mass[lst].sum()
        if M == 0:
            com[i], linvel[i] = xi0[i], vc[i]
            bcom[i], blin[i], bang[i] = dx, dv, 0.0
            continue
        mx, mv = mass[lst, None] * xi0[lst], mass[lst, None] * vc[lst]
        com[i], linvel[i] = mx.sum(0) / M, mv.sum(0) / M
        bcom[i] = REL * np.abs(mx).sum(0) / M + REL * np.abs(com[i]) + dx
        blin[i] = REL * np.abs(mv).sum(0) / M + REL * np.abs(linvel[i]) + dv
        r = xi0[lst] - com[i]
        arm = mass[lst, None] * np.cross(r, vc[lst])
        angmom[i] = (spin[lst] + arm).sum(0)
        bang[i] = REL * (np.abs(spin[lst]) + np.abs(arm)).sum(0) + np.sum(
            inorm[lst] * dw + mass[lst] * (np.abs(r).sum(1) * dv + np.abs(vc[lst]).sum(1) * (dx + np.abs(bcom[i]).max())))
    out.update(com=com, linvel=linvel, angmom=angmom, bound_com=bcom, bound_linvel=blin, bound_angmom=bang, subtree_mass=np.array(
        [mass[lst].sum() for lst in subtree_lists(m)]))
    return out


def compare(got, ref, what, worst=None, subtree=True, skin=True):
    """every output in `got` (a dict of arrays for ONE env; missing names are skipped) against reference()'s dict at the bounds of the
    module docstring; prints and returns the worst deviation per output in units of its bound"""
    worst = {} if worst is None else worst

    def note(name, dev):
        worst[name] = max(worst.get(name, 0.0), float(dev))
        assert dev <= 1.0, (what, name, dev)

    for name in ("pos", "vel", "local"):
        if skin and name in got:
            note(name, DR.close(got[name], ref[name]))
    if skin and "shape" in got:
        dev = np.abs(got["shape"] - ref["shape"]) / np.maximum(ref["bound_shape"], 1e-300)
        names = ["V", "A"] + ["centroid"] * 3 + ["moments"] * 6 + ["rate"]
        for n, x in zip(names, dev):
            note("shape." + n, x)
    if skin and "lo" in got:
        H = ref["heights"]
        tol = ARR * max(1.0, np.abs(H).max())
        for side, ext in (("lo", H.min(1)), ("hi", H.max(1))):
            note(side, np.abs(got[side] - ext).max() / tol)
            for j, v in enumerate(got[side + "_vert"]):
                assert 0 <= v < H.shape[1] and abs(H[j, v] - ext[j]) <= tol, (what, side, j, v)
                clear = np.sort(np.abs(H[j] - ext[j]))[1] > 2 * tol       # the runner-up is further off than both bounds together
                assert not clear or v == ref[side + "_vert"][j], (what, side, j, v, ref[side + "_vert"][j])
    if subtree:
        for name in ("com", "linvel", "angmom"):
            if name in got:
                b = np.maximum(ref["bound_" + name], 1e-300)
                zero = ref["bound_" + name] == 0
                assert (got[name][zero] == ref[name][zero]).all(), (what, name)
                note(name, (np.abs(got[name] - ref[name]) / b)[~zero].max() if (~zero).any() else 0.0)
    return worst


# ---- synthetic meshes ----
def tetrahedron():
    """4 vertices, 4 faces wound outward: V = 1/6, A = (3 + sqrt 3) / 2, centroid (1/4, 1/4, 1/4)"""
    P = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
    face = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32)
    return P, face


def box_mesh(size):
    """8 vertices and 12 outward faces of the box [-size/2, size/2]"""
    s = np.asarray(size, np.float64) / 2
    P = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float64) * s
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]      # outward, counter-clockwise
    face = np.array([t for q in quads for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))], np.int32)
    return P, face


def grid_shell(n=(10, 8, 5), spacing=0.1):
    """the shell of an n[0] x n[1] x n[2] point grid: 256 vertices and 508 outward faces at (10, 8, 5), the vertex limit"""
    idx, P = {}, []
    for ix in range(n[0]):
        for iy in range(n[1]):
            for iz in range(n[2]):
                if ix in (0, n[0] - 1) or iy in (0, n[1] - 1) or iz in (0, n[2] - 1):
                    idx[ix, iy, iz] = len(P)
                    P.append([ix * spacing, iy * spacing, iz * spacing])
    face = []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        for side in (0, 1):
            for i in range(n[b] - 1):
                for j in range(n[c] - 1):
                    def at(di, dj):
                        q = [0, 0, 0]
                        q[a], q[b], q[c] = (n[a] - 1) * side, i + di, j + dj
                        return idx[tuple(q)]
                    p00, p10, p11, p01 = at(0, 0), at(1, 0), at(1, 1), at(0, 1)
                    face += [(p00, p10, p11), (p00, p11, p01)] if side else [(p00, p11, p10), (p00, p01, p11)]
    return np.array(P), np.array(face, np.int32)


def is_closed(face):
    """every directed edge once, and its reverse once"""
    e = [(int(f[k]), int(f[(k + 1) % 3])) for f in face for k in range(3)]
    return len(set(e)) == len(e) and all((b, a) in set(e) for a, b in e)


def skin_of(vert_body, vert_pos, face):
    return dict(vert_body=np.asarray(vert_body, np.int32), vert_pos=np.asarray(vert_pos, np.float64), face=np.asarray(face, np.int32),
                rgba=np.array((0.8, 0.2, 0.1, 1.0), np.float32))


# ---- the g++ build of csrc/sg_shape.h and the builder in csrc/sg_tables.cpp ----
HOST_DRIVER = r"""
#include <cstdio>
#include "sg_readout_host.h"
#include "sg_shape.h"
struct Shp {
  SgHostTables M;
  SgKinHost& K = M.kin;
  SgDynHost& D = M.dyn;
  SgSkinHost S;
  SgShapeHost T;
};
extern "C" {
void* shp_create(const void* blob, size_t n, char* err, int nerr) {
  Shp* h = new Shp;
  sg_host_tables(blob, n, &h->M);
  sgh_build(h->K, h->D, h->S, &h->T);
  if (!h->T.ok) { snprintf(err, nerr, "%s", h->T.err.c_str()); delete h; return nullptr; }
  return h;
}
void shp_destroy(void* p) { delete (Shp*)p; }
// (no range checks here: sg_model_set_skin's are the library's; the builder's own are what the refusal test drives)
int shp_set_skin(void* p, int nvert, const int* vb, const double* vp, int nface, const int* face, char* err, int nerr) {
  Shp* h = (Shp*)p;
  h->S.nvert = nvert; h->S.nface = nface;
  h->S.vert_body.assign(vb, vb + nvert); h->S.vert_pos.assign(vp, vp + 3 * (size_t)nvert); h->S.face.assign(face, face + 3 * (size_t)nface);
  h->T = SgShapeHost();
  sgh_build(h->K, h->D, h->S, &h->T);
  if (!h->T.ok) snprintf(err, nerr, "%s", h->T.err.c_str());
  return h->T.ok ? 0 : -2;
}
void shp_info(void* p, int* out) {
  Shp* h = (Shp*)p;
  out[0] = h->T.o.nvert; out[1] = h->T.o.nface; out[2] = h->T.o.closed; out[3] = h->T.o.root; out[4] = h->K.o.nbody; out[5] = h->T.o.nlist;
}
void shp_rest(void* p, int frame, double* rest) { Shp* h = (Shp*)p; sgh_rest(h->K, h->S, frame, rest); }
void shp_subtree_mass(void* p, double* mass) { Shp* h = (Shp*)p; memcpy(mass, h->T.dbl.data() + h->T.o.smass, sizeof(double) * h->K.o.nbody); }
int shp_env(void* p, const double* qpos, const double* qvel, int frame, int ndirs, const double* dir, const int* dir_body, double* pos, double* vel, double* local,
            double* shape, double* lo, double* hi, int* lov, int* hiv, double* com, double* linvel, double* angmom) {
  Shp* h = (Shp*)p;
  return sgh_host_env(h->K, h->D, h->T, qpos, qvel, frame, ndirs, dir, dir_body, pos, vel, local, shape, lo, hi, lov, hiv, com, linvel, angmom);
}
// the face shares, the kernel's sums and sgh_finish on a mesh given as vertex records [nvert][6] (position, velocity)
void shp_mesh(int nvert, const double* V, int nface, const int* face, double* shape) {
  double lane[SGH_NSUM][64] = {}, sum[SGH_NSUM];
  for (int f = 0; f < nface; f++) {
    double s1[SGH_NSUM];
    sgh_face(V, face[3 * f], face[3 * f + 1], face[3 * f + 2], s1);
    for (int q = 0; q < SGH_NSUM; q++) lane[q][f % 64] += s1[q];
  }
  for (int q = 0; q < SGH_NSUM; q++) sum[q] = sgh_host_wave_sum(lane[q]);
  sgh_finish(sum, V, shape);
}
// the builder on a model of nbody bodies and a skin of nvert vertices that exist as counts only: what it says before it reads an array
int shp_refusal(int nbody, int nvert, char* err, int nerr) {
  SgKinHost K;
  SgDynHost D;
  SgSkinHost S;
  SgShapeHost T;
  K.ok = D.ok = true;
  K.o = SgKinOff();
  K.o.nbody = nbody;
  S.nvert = nvert;
  sgh_build(K, D, S, &T);
  snprintf(err, nerr, "%s", T.err.c_str());
  return T.ok;
}
int shp_limits(int* out) { out[0] = SGH_LDS_MAX; out[1] = SGH_STATIC_LDS; out[2] = SGD_REC + SGH_SHARE; out[3] = SGH_VREC; out[4] = SGH_MAXDIR; out[5] = SGH_SHAPE_N; return 6; }
}
"""


def build_host(tmpdir):
    """compiles the driver above with csrc/sg_tables.cpp by g++ into tmpdir -> the ctypes library"""
    L = host_build.build(tmpdir, "shape_host", HOST_DRIVER, sources=("sg_tables.cpp",))
    L.shp_create.restype = C.c_void_p
    L.shp_create.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_int]
    L.shp_destroy.argtypes = [C.c_void_p]
    L.shp_set_skin.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_char_p, C.c_int]
    L.shp_info.argtypes = [C.c_void_p, C.c_void_p]
    L.shp_rest.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.shp_subtree_mass.argtypes = [C.c_void_p, C.c_void_p]
    L.shp_env.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 13
    L.shp_mesh.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.shp_refusal.argtypes = [C.c_int, C.c_int, C.c_char_p, C.c_int]
    L.shp_limits.argtypes = [C.c_void_p]
    return L


def _p(x):
    return None if x is None else x.ctypes.data_as(C.c_void_p)


class Host:
    """one model in the g++ build: the table builder's answers and sgh_host_env"""

    def __init__(self, L, m):
        self.L, self.m = L, m
        blob = m.to_blob()
        err = C.create_string_buffer(512)
        self.p = L.shp_create(blob, len(blob), err, 512)
        if not self.p:
            raise RuntimeError(err.value.decode())
        self.set_skin(None)

    def __del__(self):
        if getattr(self, "p", None):
            self.L.shp_destroy(self.p)

    def set_skin(self, skin):
        """-> None, or the builder's refusal"""
        err = C.create_string_buffer(512)
        if skin is None:
            rc = self.L.shp_set_skin(self.p, 0, None, None, 0, None, err, 512)
        else:
            vb, vp = np.ascontiguousarray(skin["vert_body"], np.int32), np.ascontiguousarray(skin["vert_pos"], np.float64)
            fc = np.ascontiguousarray(skin["face"], np.int32)
            rc = self.L.shp_set_skin(self.p, len(vb), _p(vb), _p(vp), len(fc), _p(fc), err, 512)
        info = np.zeros(6, np.int32)
        self.L.shp_info(self.p, _p(info))
        self.nvert, self.nface, self.closed, self.root, self.nbody, self.nlist = (int(x) for x in info)
        return None if rc == 0 else err.value.decode()

    def rest(self, frame=-1):
        out = np.zeros((self.nvert, 3))
        self.L.shp_rest(self.p, frame, _p(out))
        return out

    def subtree_mass(self):
        out = np.zeros(self.nbody)
        self.L.shp_subtree_mass(self.p, _p(out))
        return out

    def env(self, qpos, qvel, frame_body=-1, dirs=None, dir_body=None, shape=True):
        q, v = np.ascontiguousarray(qpos, np.float64), np.ascontiguousarray(qvel, np.float64)
        nv, nb = self.nvert, self.nbody
        out = dict(com=np.zeros((nb, 3)), linvel=np.zeros((nb, 3)), angmom=np.zeros((nb, 3)))
        if nv:
            out.update(pos=np.zeros((nv, 3)), vel=np.zeros((nv, 3)), local=np.zeros((nv, 3)))
            if shape:
                out["shape"] = np.zeros(SHAPE_N)
        nd = 0
        hd = hb = None
        if dirs is not None and nv:
            hd = np.ascontiguousarray(dirs, np.float64).reshape(-1, 3)
            nd = len(hd)
            hb = None if dir_body is None else np.ascontiguousarray(dir_body, np.int32)
            out.update(lo=np.zeros(nd), hi=np.zeros(nd), lo_vert=np.zeros(nd, np.int32), hi_vert=np.zeros(nd, np.int32))
        g = out.get
        rc = self.L.shp_env(self.p, _p(q), _p(v), frame_body, nd, _p(hd), _p(hb), _p(g("pos")), _p(g("vel")), _p(g("local")), _p(g("shape")), _p(g("lo")),
                            _p(g("hi")), _p(g("lo_vert")), _p(g("hi_vert")), _p(out["com"]), _p(out["linvel"]), _p(out["angmom"]))
        assert rc == 0, "a state that is not finite"
        return out


def mesh_shape(L, P, Vel, face):
    """[12] of the g++ build for a bare mesh: positions, velocities, faces"""
    V = np.ascontiguousarray(np.concatenate([P, Vel], axis=1), np.float64)
    fc = np.ascontiguousarray(face, np.int32)
    out = np.zeros(SHAPE_N)
    L.shp_mesh(len(V), _p(V), len(fc), _p(fc), _p(out))
    return out


# directions every test uses: the world axes, a skew one that is not unit, and palm-fixed ones (given in a body's frame)
def directions(m, body):
    dirs = np.array([[1.0, 0, 0], [0, 1, 0], [0, 0, 1], [0.3, -2.0, 0.7], [1.0, 0, 0], [0, 0.5, 0.5]])
    return dirs, np.array([-1, -1, -1, -1, body, body], np.int32)
