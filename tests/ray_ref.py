"""Independent NumPy (fp64) ray caster for sg_ray (include/softgrip.h, soft-grip_amd/csrc/sg_ray.h): written from the rules the header
states, not from the header's code.  World frame throughout: body-frame rays are mapped first (map_rays) with the body poses the caller
has -- NativeBatch.poses() on the GPU, mjcf.Model.kinematics() on the CPU.  Geom poses and categories are render_ref's.

Rules: entry hits only (the smallest t > 0 at which the ray enters the primitive from outside; an origin inside sees nothing of it),
planes one-sided, of equal distances the smaller geom id, a hit beyond max_dist (> 0) is a miss; a direction without length or with a
non-finite component is a miss.  Results: dist (-1 miss), geom (-1), outward unit normal in world axes (zeros)."""
import ctypes as C

import numpy as np

import host_build
from render_ref import BOX, CAPSULE, PLANE, SPHERE, categories, geom_poses  # noqa: F401
from softgrip_amd.mjcf import quat_to_mat

GROUND_BIT, STATIC_BIT, FINGER_BIT, ELEM_BIT, CENTER_BIT, ALL_BITS = 1, 2, 4, 8, 16, 31


def _sphere_entry(o, d, r):
    """entry root of |o + t d| = r per ray (unit d), inf where there is none or it is not positive"""
    tl = -np.sum(o * d, -1)
    q = o + tl[:, None] * d
    h2 = r * r - np.sum(q * q, -1)
    with np.errstate(invalid="ignore"):
        t = tl - np.sqrt(h2)
    return np.where((h2 >= 0) & (t > 0), t, np.inf)


def _primitive(type_, size, o, d):
    """rays o + t d [N, 3] in the primitive's own frame -> entry distance [N] (inf: none) and local outward normal [N, 3]"""
    n = len(d)
    nl = np.zeros((n, 3))
    nl[:, 2] = 1.0
    t = np.full(n, np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        if type_ == PLANE:
            tt = -o[:, 2] / d[:, 2]
            ok = (d[:, 2] < 0) & (o[:, 2] > 0)
            if size[0] > 0 and size[1] > 0:
                ok &= (np.abs(o[:, 0] + tt * d[:, 0]) <= size[0]) & (np.abs(o[:, 1] + tt * d[:, 1]) <= size[1])
            t = np.where(ok, tt, np.inf)
        elif type_ == SPHERE:
            t = _sphere_entry(o, d, size[0])
            nl = (o + np.where(np.isfinite(t), t, 0.0)[:, None] * d) / size[0]
        elif type_ == CAPSULE:
            r, hl = size[0], size[1]
            a = d[:, 0] ** 2 + d[:, 1] ** 2
            tl = -(o[:, 0] * d[:, 0] + o[:, 1] * d[:, 1]) / a
            q0, q1 = o[:, 0] + tl * d[:, 0], o[:, 1] + tl * d[:, 1]
            h2 = r * r - (q0 * q0 + q1 * q1)
            ts = tl - np.sqrt(h2 / a)
            side = (a > 1e-24) & (h2 >= 0) & (ts > 0) & (np.abs(o[:, 2] + ts * d[:, 2]) <= hl)
            t = np.where(side, ts, np.inf)
            for zc, sgn in ((hl, 1.0), (-hl, -1.0)):       # a cap is surface on its outer hemisphere only
                tc = _sphere_entry(o - np.array([0.0, 0.0, zc]), d, r)
                z = o[:, 2] + np.where(np.isfinite(tc), tc, 0.0) * d[:, 2]
                tc = np.where(sgn * (z - zc) >= 0, tc, np.inf)
                t = np.minimum(t, tc)
            h = o + np.where(np.isfinite(t), t, 0.0)[:, None] * d
            nl = (h - np.stack([np.zeros(n), np.zeros(n), np.clip(h[:, 2], -hl, hl)], -1)) / r
        elif type_ == BOX:
            t1 = (-size - o) / d
            t2 = (size - o) / d
            lo, hi = np.minimum(t1, t2), np.maximum(t1, t2)
            par = d == 0
            lo = np.where(par, -np.inf, lo)
            hi = np.where(par, np.inf, hi)
            miss = np.any(par & (np.abs(o) > size), -1)
            tn, tf = lo.max(-1), hi.min(-1)
            ax = lo.argmax(-1)
            t = np.where(~miss & (tn <= tf) & (tn > 0), tn, np.inf)
            nl = np.zeros((n, 3))
            nl[np.arange(n), ax] = -np.sign(d[np.arange(n), ax])
    return t, nl


def candidates(cats, geom_body, cat_mask=ALL_BITS, exclude=None, nrays=1):
    """[ngeom, nrays] bool: geom g is a candidate of ray r (its category's bit in cat_mask, not on the ray's excluded body)"""
    keep = ((int(cat_mask) >> np.asarray(cats)) & 1).astype(bool)[:, None] & np.ones((1, nrays), bool)
    if exclude is not None:
        ex = np.asarray(exclude).reshape(-1)
        keep = keep & ~((ex[None, :] >= 0) & (np.asarray(geom_body)[:, None] == ex[None, :]))
    return keep


def map_rays(xpos, xquat, origin, direction, body=None):
    """rays given in body frames (body [N], -1 / None: world) -> world origins and (unnormalised) directions"""
    o, d = np.array(origin, dtype=np.float64), np.array(direction, dtype=np.float64)
    if body is None:
        return o, d
    for r, b in enumerate(np.asarray(body).reshape(-1)):
        if b >= 0:
            R = quat_to_mat(xquat[b])
            o[r] = xpos[b] + R @ o[r]
            d[r] = R @ d[r]
    return o, d


def cast(gx, gm, types, sizes, origin, direction, keep=None, max_dist=0.0, per_geom=False):
    """world rays against the geoms -> dist [N] (-1), geom [N] int32 (-1), normal [N, 3] (zeros); with per_geom=True a fourth entry:
    the entry distance of every candidate geom on every ray [ngeom, N] (inf: none), what compare()'s coplanar rule reads"""
    o = np.asarray(origin, dtype=np.float64).reshape(-1, 3)
    d = np.asarray(direction, dtype=np.float64).reshape(-1, 3)
    n, ng = len(o), len(types)
    with np.errstate(invalid="ignore", over="ignore"):
        ln = np.sqrt(np.sum(d * d, -1))
    live = np.isfinite(ln) & (ln > 0) & np.isfinite(d).all(-1)
    u = np.where(live[:, None], d / np.where(live, ln, 1.0)[:, None], np.array([0.0, 0.0, 1.0]))
    T = np.full((ng, n), np.inf)
    NL = np.zeros((ng, n, 3))
    for g in range(ng):
        R = np.asarray(gm[g], dtype=np.float64).reshape(3, 3)
        T[g], NL[g] = _primitive(int(types[g]), np.asarray(sizes[g], dtype=np.float64), (o - gx[g]) @ R, u @ R)
    if keep is not None:
        T = np.where(keep, T, np.inf)
    T[:, ~live] = np.inf
    if ng == 0:
        return (np.full(n, -1.0), np.full(n, -1, np.int32), np.zeros((n, 3))) + ((T,) if per_geom else ())
    gid = np.argmin(T, 0)                    # (first = smallest id among equal distances)
    t = T[gid, np.arange(n)]
    hit = np.isfinite(t) & ((t <= max_dist) if max_dist > 0 else True)
    nw = np.einsum("nij,nj->ni", np.asarray(gm, dtype=np.float64).reshape(ng, 3, 3)[gid], NL[gid, np.arange(n)])
    return (np.where(hit, t, -1.0), np.where(hit, gid, -1).astype(np.int32), np.where(hit[:, None], nw, 0.0)) + ((T,) if per_geom else ())


def unstable(gx, gm, types, sizes, origin, direction, keep, max_dist, ref, shift=1e-7, tol=1e-5):
    """[N] bool: the reference's OWN answer changes (another geom, or the distance by more than tol) when the ray's origin is moved by
    +-shift along a world axis -- a ray that grazes a silhouette; only such rays may be left out of a comparison"""
    o = np.asarray(origin, dtype=np.float64).reshape(-1, 3)
    bad = np.zeros(len(o), bool)
    for ax in range(3):
        for sg_ in (-shift, shift):
            e = np.zeros(3)
            e[ax] = sg_
            dist, gid, _ = cast(gx, gm, types, sizes, o + e, direction, keep, max_dist)
            bad |= (gid != ref[1]) | (np.abs(dist - ref[0]) > tol)
    return bad


COPLANAR = 1e-12      # two candidates of a ray tie when the reference's own distances to them are this close


def coplanar_ties(got, ref, per_geom, tol=1e-9):
    """[N] bool: the returned geom is not the reference's, but the reference's OWN distance to the returned geom is within COPLANAR of
    its best distance -- two surfaces in one plane (the two boxes of a link with coplanar faces), where the last bits of two correct
    evaluations pick the winner -- and the returned distance and normal still agree with the reference's within tol"""
    gd, gg, gn = got
    rd, rg, rn = ref[:3]
    n = len(rd)
    both = (gg != rg) & (gg >= 0) & (rg >= 0) & (gg < len(per_geom))
    t_got = np.where(both, per_geom[np.where(both, gg, 0), np.arange(n)], np.inf)
    tie = both & (np.abs(t_got - rd) <= COPLANAR) & (np.abs(gd - rd) <= tol)
    if gn is not None:
        tie &= np.abs(gn - rn).max(-1) <= tol
    return tie


def compare(got, ref, edge, what="", tol=1e-9, cap=0.02, per_geom=None):
    """geom ids exact, dist and normals within tol, off the rays of `edge` (at most `cap` of them); -> number left out.
    per_geom (cast(..., per_geom=True)'s fourth entry; None: the rule is off): rays of coplanar_ties() may be left out too, and count
    against the same cap"""
    gd, gg, gn = got
    rd, rg, rn = ref[:3]
    wrong = (gg != rg) | ~(np.abs(gd - rd) <= tol)
    if gn is not None:
        wrong |= ~(np.abs(gn - rn).max(-1) <= tol)
    if per_geom is not None:
        edge = edge | coplanar_ties(got, ref, per_geom, tol)
    assert not (wrong & ~edge).any(), "%s: rays %s differ off the knife edges: got %s / %s, want %s / %s" % (
        what, np.flatnonzero(wrong & ~edge)[:5].tolist(), gg[wrong & ~edge][:5], gd[wrong & ~edge][:5], rg[wrong & ~edge][:5], rd[wrong & ~edge][:5])
    left = int((wrong & edge).sum())
    assert left <= cap * len(rd), "%s: %d of %d rays left out" % (what, left, len(rd))
    return left


def scene_rays(gx, types, n, seed):
    """the test recipe: c, half = centre and half-diagonal of the non-plane geom centres; origins c + 1.5 half u + (0, 0, 0.2) with u
    uniform on the upper unit hemisphere, aimed at targets c + U(-0.6, 0.6)^3 half"""
    rs = np.random.RandomState(seed)
    p = np.asarray(gx)[np.asarray(types) != PLANE]
    lo, hi = p.min(0), p.max(0)
    c, half = 0.5 * (lo + hi), 0.5 * np.linalg.norm(hi - lo)
    u = rs.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    u[:, 2] = np.abs(u[:, 2])
    o = c + 1.5 * half * u + np.array([0.0, 0.0, 0.2])
    tgt = c + rs.uniform(-0.6, 0.6, (n, 3)) * half
    return o, tgt - o


# ---- the ray sweep of the random grippers (tests/test_ray_host.py on the host build, tests/test_gpu_ray.py on the device) ----
SWEEP_POSES = slice(2, None, 4)      # of a gripper's 64 swept poses (dyn_ref.sweep) every fourth: 16, the last one an aligned pose
SWEEP_RAYS = 256                     # scene_rays per pose
SWEEP_RAY_SEED = 9000                # pose p of gripper g casts scene_rays(..., SWEEP_RAY_SEED + 100 g + p)


def sweep_poses(gripper, tmpdir):
    """(model, qpos [16, nq]) of a gripper of the sweep"""
    import dyn_ref
    s = dyn_ref.sweep(gripper, tmpdir)
    return s[0], s[1][SWEEP_POSES]


def link_rays(model, n, seed):
    """n rays in the frame of a random finger link (a body with hinges), which they also exclude: origins U(-0.3, 0.3)^3 around the
    link's origin -- inside the scene, among the fingers -- in random directions -> (origin [n, 3], direction [n, 3], body [n])"""
    rs = np.random.RandomState(seed)
    jt, adr, num = np.asarray(model.jnt_type), np.asarray(model.body_jntadr), np.asarray(model.body_jntnum)
    links = [b for b in range(1, model.nbody) if num[b] > 0 and (jt[adr[b]:adr[b] + num[b]] == 3).all()]
    body = int(links[rs.randint(len(links))])
    return rs.uniform(-0.3, 0.3, (n, 3)), rs.normal(size=(n, 3)), np.full(n, body, np.int32)


def count_types(types, gid, counts):
    """adds the hits of gid by geom type to counts (a dict)"""
    for t in np.asarray(types)[gid[gid >= 0]]:
        counts[int(t)] = counts.get(int(t), 0) + 1
    return counts


# ---- the g++ build of csrc/sg_ray_walk.h (over sg_ray.h and sg_ray_skin.h): the walk, the reduction and the finish the kernels compile ----
HOST_DRIVER = r"""
#include <vector>
#include "sg_ray_walk.h"
extern "C" void skin_vertex_host(int nvert, const int* vbody, const double* vpos, const double* xpos, const double* xquat, double* out) {
  for (int v = 0; v < nvert; v++) sgys_vertex(xpos + 3 * vbody[v], xquat + 4 * vbody[v], vpos + 3 * v, out + 3 * v);
}

// the arrays as records, packed faces and views, then sgyw_host_ray per ray (layout: which kernel layout's walkers).  No skin: nface = 0
extern "C" void ray_host(int layout, int ng, const double* gx, const double* gm, const double* gs, const int* type, const int* cat, const int* gbody,
                         const int* hidden, const double* verts, const int* vbody, int nface, const int* face, const double* xpos,
                         const double* xquat, int nr, const double* o_in, const double* d_in, const int* rbody, const int* rexcl, int cat_mask,
                         double max_dist, double* dist, int* geom, double* normal) {
  std::vector<double> recs((size_t)ng * SGY_REC);
  for (int g = 0; g < ng; g++) {
    double* r = &recs[(size_t)SGY_REC * g];
    for (int c = 0; c < 3; c++) r[c] = gx[3 * g + c];
    for (int c = 0; c < 9; c++) r[3 + c] = gm[9 * g + c];
    for (int c = 0; c < 3; c++) r[12 + c] = gs[3 * g + c];
    r[15] = sgy_meta_word(sgy_meta(type[g], cat[g], gbody[g]));
  }
  std::vector<uint32_t> packed(nface);
  for (int f = 0; f < nface; f++) packed[f] = (uint32_t)face[3 * f] | ((uint32_t)face[3 * f + 1] << 8) | ((uint32_t)face[3 * f + 2] << 16);
  SgywHostGeoms G = {recs.data(), hidden, ng};
  const SgywSkin K = {verts, packed.data(), vbody, nface};
  for (int q = 0; q < nr; q++) {
    const int body = rbody ? rbody[q] : -1;
    sgyw_host_ray(G, K, layout, body >= 0 ? xpos + 3 * body : nullptr, xquat + 4 * (body >= 0 ? body : 0), o_in + 3 * q, d_in + 3 * q,
                  rexcl ? rexcl[q] : -1, cat_mask, max_dist > 0 ? max_dist : INFINITY, dist + q, geom + q, normal + 3 * q);
  }
}
"""


def build_host(tmpdir):
    """compiles the driver above with g++ into tmpdir -> the ctypes library (ray_host, skin_vertex_host)"""
    L = host_build.build(tmpdir, "ray_host", HOST_DRIVER)
    L.ray_host.restype = None
    L.skin_vertex_host.restype = None
    return L


def _a(x, dt):
    return np.ascontiguousarray(x, dtype=dt)


def _p(x):
    return None if x is None else x.ctypes.data_as(C.c_void_p)


def cast_host(L, gx, gm, types, sizes, cats, geom_body, hidden, verts, vert_body, face, origin, direction, xpos, xquat, body, exclude, cat_mask,
              max_dist, layout):
    """the host build on the same inputs (body-frame rays mapped by the header's own code) -> dist, id, normal.  hidden None: no geom is"""
    gx, gm, gs = _a(np.reshape(gx, (-1, 3)), np.float64), _a(np.reshape(gm, (-1, 9)), np.float64), _a(np.reshape(sizes, (-1, 3)), np.float64)
    ty, ct, gb = _a(types, np.int32), _a(cats, np.int32), _a(geom_body, np.int32)
    hid = None if hidden is None else _a(hidden, np.int32)
    vs, vb, fc = _a(np.reshape(verts, (-1, 3)), np.float64), _a(vert_body, np.int32), _a(np.reshape(face, (-1, 3)), np.int32)
    o, d = _a(np.reshape(origin, (-1, 3)), np.float64), _a(np.reshape(direction, (-1, 3)), np.float64)
    xp = _a(np.zeros((1, 3)) if xpos is None else xpos, np.float64)
    xq = _a(np.array([[1.0, 0, 0, 0]]) if xquat is None else xquat, np.float64)
    rb = None if body is None else _a(body, np.int32)
    rx = None if exclude is None else _a(exclude, np.int32)
    n = len(o)
    dist, geom, normal = np.empty(n), np.empty(n, np.int32), np.empty((n, 3))
    L.ray_host(C.c_int(layout), C.c_int(len(ty)), _p(gx), _p(gm), _p(gs), _p(ty), _p(ct), _p(gb), _p(hid), _p(vs), _p(vb), C.c_int(len(fc)), _p(fc),
               _p(xp), _p(xq), C.c_int(n), _p(o), _p(d), _p(rb), _p(rx), C.c_int(int(cat_mask)), C.c_double(float(max_dist)), _p(dist), _p(geom), _p(normal))
    return dist, geom, normal


def cast_with(L, gx, gm, types, sizes, cats, geom_body, origin, direction, xpos=None, xquat=None, body=None, exclude=None, cat_mask=ALL_BITS,
              max_dist=0.0, layout=0):
    """the plain call: the skin call with no vertices, no faces and nothing hidden"""
    return cast_host(L, gx, gm, types, sizes, cats, geom_body, None, np.zeros((0, 3)), np.zeros(0), np.zeros((0, 3)), origin, direction, xpos, xquat,
                     body, exclude, cat_mask, max_dist, layout)
