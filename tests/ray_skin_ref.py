"""Independent NumPy (fp64) caster for sg_ray with SG_RAY_SKIN (include/softgrip.h, soft-grip_amd/csrc/sg_ray_skin.h): written from the
rules the header states, not from its code.  The geoms go through tests/ray_ref.py's caster with the hidden ones removed; the skin's
triangles are cast here:

* a vertex sits at xpos[body] + R(xquat[body]) vert_pos; the geoms of the bodies the vertices are bound to are never candidates;
* per ray the vertices are taken relative to its origin; the edge value of edge (p, q) is d . (p x q) with the endpoint of smaller
  vertex index first, oriented per triangle (a, b, c) as E_ab = d . (b x a); inside when all three are >= 0;
* front faces only: n = (b - a) x (c - a), n . d < 0, t = (n . a) / (n . d) > 0; a hit beyond max_dist (> 0) is a miss;
* the triangles are candidates when cat_mask holds the element bit; a ray's excluded body removes every triangle with a vertex bound
  to it;
* ids: ngeom + face index; smaller t, then smaller id: a geom wins a tie against a triangle, the smaller face index among triangles;
* normal: n / |n|, flat.

unstable() is ray_ref.unstable's notion for this caster, and the comparison is ray_ref.compare itself."""
import ctypes as C
import os
import subprocess

import numpy as np

import ray_ref as RR
from softgrip_amd.mjcf import quat_to_mat


def vertices(skin, xpos, xquat):
    """world positions [nvert, 3] from body poses xpos [nbody, 3], xquat [nbody, 4]"""
    vb = np.asarray(skin["vert_body"])
    vp = np.asarray(skin["vert_pos"], dtype=np.float64)
    return np.stack([np.asarray(xpos[b], dtype=np.float64) + quat_to_mat(xquat[b]) @ vp[v] for v, b in enumerate(vb)])


def hidden_geoms(geom_body, skin):
    return np.isin(np.asarray(geom_body), np.asarray(skin["vert_body"]))


def _edge(d, p, q, ip, iq):
    """oriented value E_pq = d . (q x p), the endpoint of smaller index first"""
    return -np.sum(d * np.cross(p, q), -1) if ip < iq else np.sum(d * np.cross(q, p), -1)


def cast_triangles(o, u, verts, face, vert_body=None, exclude=None):
    """rays o + t u [N, 3] (u unit) against the triangles -> t [N] (inf: none), face [N] (-1), unit normal [N, 3]"""
    n_ray = len(o)
    best = np.full(n_ray, np.inf)
    bf = np.full(n_ray, -1, dtype=np.int32)
    bn = np.zeros((n_ray, 3))
    rel = np.asarray(verts, dtype=np.float64)[None, :, :] - o[:, None, :]
    ex = None if exclude is None else np.asarray(exclude).reshape(-1)
    for f, (ia, ib, ic) in enumerate(np.asarray(face).reshape(-1, 3)):
        a, b, c = rel[:, ia], rel[:, ib], rel[:, ic]
        eab, ebc, eca = _edge(u, a, b, ia, ib), _edge(u, b, c, ib, ic), _edge(u, c, a, ic, ia)
        n = np.cross(b - a, c - a)
        den = np.sum(n * u, -1)
        with np.errstate(divide="ignore", invalid="ignore"):
            t = np.sum(n * a, -1) / den
            ok = (eab >= 0) & (ebc >= 0) & (eca >= 0) & (den < 0) & (t > 0) & np.isfinite(t) & (t < best)
        if ex is not None:
            vb = np.asarray(vert_body)
            ok &= ~((ex >= 0) & ((vb[ia] == ex) | (vb[ib] == ex) | (vb[ic] == ex)))
        best = np.where(ok, t, best)
        bf = np.where(ok, f, bf)
        with np.errstate(divide="ignore", invalid="ignore"):
            bn = np.where(ok[:, None], n / np.linalg.norm(n, axis=-1, keepdims=True), bn)
    return best, bf, bn


def cast(gx, gm, types, sizes, cats, geom_body, skin, verts, origin, direction, cat_mask=RR.ALL_BITS, exclude=None, max_dist=0.0):
    """world rays against the non-hidden geoms and the skin -> dist [N] (-1), id [N] int32 (-1; ngeom + face on the skin), normal [N, 3]"""
    o = np.asarray(origin, dtype=np.float64).reshape(-1, 3)
    d = np.asarray(direction, dtype=np.float64).reshape(-1, 3)
    n, ng = len(o), len(types)
    keep = RR.candidates(cats, geom_body, cat_mask, exclude, n) & ~hidden_geoms(geom_body, skin)[:, None]
    gd, gg, gn = RR.cast(gx, gm, types, sizes, o, d, keep, max_dist)
    if not (int(cat_mask) & RR.ELEM_BIT) or len(skin["face"]) == 0:
        return gd, gg, gn
    with np.errstate(invalid="ignore", over="ignore"):
        ln = np.sqrt(np.sum(d * d, -1))
    live = np.isfinite(ln) & (ln > 0) & np.isfinite(d).all(-1)
    u = np.where(live[:, None], d / np.where(live, ln, 1.0)[:, None], np.array([0.0, 0.0, 1.0]))
    tt, tf, tn = cast_triangles(o, u, verts, skin["face"], skin["vert_body"], exclude)
    tt = np.where(live, tt, np.inf)
    if max_dist > 0:
        tt = np.where(tt <= max_dist, tt, np.inf)
    tg = np.where(gg >= 0, gd, np.inf)
    sk = tt < tg                                   # (a geom wins at equal distance)
    return np.where(sk, tt, gd), np.where(sk, ng + tf, gg).astype(np.int32), np.where(sk[:, None], tn, gn)


def unstable(gx, gm, types, sizes, cats, geom_body, skin, verts, origin, direction, cat_mask, exclude, max_dist, ref, shift=1e-7, tol=1e-5):
    """[N] bool: the reference's OWN answer changes (another id, or the distance by more than tol) when the ray's origin is moved by
    +-shift along a world axis; only such rays may be left out of a comparison"""
    o = np.asarray(origin, dtype=np.float64).reshape(-1, 3)
    bad = np.zeros(len(o), bool)
    for ax in range(3):
        for s in (-shift, shift):
            e = np.zeros(3)
            e[ax] = s
            dist, gid, _ = cast(gx, gm, types, sizes, cats, geom_body, skin, verts, o + e, direction, cat_mask, exclude, max_dist)
            bad |= (gid != ref[1]) | (np.abs(dist - ref[0]) > tol)
    return bad


def faces_of(gid, ngeom):
    """the Python interface's `face`: geom - ngeom on skin hits, -1 elsewhere"""
    gid = np.asarray(gid)
    return np.where(gid >= ngeom, gid - ngeom, -1).astype(np.int32)


# ---- the g++ build of sg_ray_skin.h + sg_ray.h: vertices, the walk and the reduction as the two kernel layouts do them ----
HOST_DRIVER = r"""
#include <vector>
#include "sg_ray_skin.h"
extern "C" void skin_vertex_host(int nvert, const int* vbody, const double* vpos, const double* xpos, const double* xquat, double* out) {
  for (int v = 0; v < nvert; v++) sgys_vertex(xpos + 3 * vbody[v], xquat + 4 * vbody[v], vpos + 3 * v, out + 3 * v);
}

// layout 0: one walker over the visible geoms in id order, then the faces (the lane-per-ray kernel); 1: 64 walkers striding over geoms
// and faces, reduced by sgy_better in the butterfly order of the wave reduction (the lanes-over-candidates kernel)
extern "C" void skin_ray_host(int layout, int ng, const double* gx, const double* gm, const double* gs, const int* type, const int* cat, const int* gbody,
                              const int* hidden, int nvert, const double* verts, const int* vbody, int nface, const int* face, const double* xpos,
                              const double* xquat, int nr, const double* o_in, const double* d_in, const int* rbody, const int* rexcl, int cat_mask,
                              double max_dist, double* dist, int* geom, double* normal) {
  std::vector<double> recs((size_t)ng * SGY_REC + SGY_REC);
  for (int g = 0; g < ng; g++) {
    double* r = &recs[(size_t)SGY_REC * g];
    for (int c = 0; c < 3; c++) r[c] = gx[3 * g + c];
    for (int c = 0; c < 9; c++) r[3 + c] = gm[9 * g + c];
    for (int c = 0; c < 3; c++) r[12 + c] = gs[3 * g + c];
    r[15] = sgy_meta_word(sgy_meta(type[g], cat[g], gbody[g]));
  }
  std::vector<uint32_t> packed(nface + 1);
  for (int f = 0; f < nface; f++) packed[f] = (uint32_t)face[3 * f] | ((uint32_t)face[3 * f + 1] << 8) | ((uint32_t)face[3 * f + 2] << 16);
  const double limit = max_dist > 0 ? max_dist : INFINITY;
  const bool tris = (cat_mask >> SGYS_CAT_ELEM) & 1;
  for (int q = 0; q < nr; q++) {
    const int body = rbody ? rbody[q] : -1, excl = rexcl ? rexcl[q] : -1;
    double o[3], d[3];
    const bool live = sgy_map_ray(body >= 0 ? xpos + 3 * body : nullptr, xquat + 4 * (body >= 0 ? body : 0), o_in + 3 * q, d_in + 3 * q, o, d);
    SgysFrame fr;
    if (live) sgys_frame(d, &fr);
    auto tri = [&](int f, SgyBest* b) {
      int ia, ib, ic;
      sgys_face(packed[f], &ia, &ib, &ic);
      sgys_visit(ng + f, verts + 3 * ia, ia, verts + 3 * ib, ib, verts + 3 * ic, ic, vbody, fr, o, d, excl, b);
    };
    SgyBest best = {INFINITY, -1, 0};
    if (live && layout == 0) {
      for (int g = 0; g < ng; g++)
        if (!hidden[g]) sgy_visit(g, &recs[(size_t)SGY_REC * g], o, d, cat_mask, excl, limit, &best);
      for (int f = 0; tris && f < nface; f++) tri(f, &best);
    } else if (live) {
      SgyBest w[64];
      for (int l = 0; l < 64; l++) {
        w[l] = SgyBest{INFINITY, -1, 0};
        for (int g = l; g < ng; g += 64)
          if (!hidden[g]) sgy_visit(g, &recs[(size_t)SGY_REC * g], o, d, cat_mask, excl, limit, &w[l]);
        for (int f = l; tris && f < nface; f += 64) tri(f, &w[l]);
      }
      for (int m = 32; m >= 1; m >>= 1) {
        SgyBest nx[64];
        for (int l = 0; l < 64; l++) nx[l] = sgy_better(w[l ^ m].t, w[l ^ m].geom, w[l].t, w[l].geom) ? w[l ^ m] : w[l];
        for (int l = 0; l < 64; l++) w[l] = nx[l];
      }
      best = w[0];
    }
    if (best.geom >= ng) {
      int ia, ib, ic;
      sgys_face(packed[best.geom - ng], &ia, &ib, &ic);
      sgys_finish(best, verts + 3 * ia, verts + 3 * ib, verts + 3 * ic, limit, dist + q, geom + q, normal + 3 * q);
    } else {
      sgy_finish(best, &recs[(size_t)SGY_REC * (best.geom >= 0 ? best.geom : 0)], o, d, limit, dist + q, geom + q, normal + 3 * q);
    }
  }
}
"""


def build_host(tmpdir):
    """compiles the driver above (sg_ray_skin.h, sg_ray.h) with g++ into tmpdir -> the ctypes library"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(tmpdir, "ray_skin_host.cpp")
    so = os.path.join(tmpdir, "libray_skin_host.so")
    with open(src, "w") as f:
        f.write(HOST_DRIVER)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(root, "soft-grip_amd", "csrc"), "-o", so, src])
    L = C.CDLL(so)
    L.skin_ray_host.restype = None
    L.skin_vertex_host.restype = None
    return L


def _a(x, dt):
    return np.ascontiguousarray(x, dtype=dt)


def _p(x):
    return None if x is None else x.ctypes.data_as(C.c_void_p)


def vertices_with(L, skin, xpos, xquat):
    vb, vp = _a(skin["vert_body"], np.int32), _a(skin["vert_pos"], np.float64)
    xp, xq = _a(xpos, np.float64), _a(xquat, np.float64)
    out = np.empty((len(vb), 3))
    L.skin_vertex_host(C.c_int(len(vb)), _p(vb), _p(vp), _p(xp), _p(xq), _p(out))
    return out


def cast_with(L, gx, gm, types, sizes, cats, geom_body, skin, verts, origin, direction, xpos=None, xquat=None, body=None, exclude=None,
              cat_mask=RR.ALL_BITS, max_dist=0.0, layout=0):
    """the host build on the same inputs (body-frame rays mapped by the header's own code) -> dist, id, normal"""
    gx, gm, gs = _a(np.reshape(gx, (-1, 3)), np.float64), _a(np.reshape(gm, (-1, 9)), np.float64), _a(np.reshape(sizes, (-1, 3)), np.float64)
    ty, ct, gb = _a(types, np.int32), _a(cats, np.int32), _a(geom_body, np.int32)
    hid = _a(hidden_geoms(gb, skin), np.int32)
    vs, vb, fc = _a(np.reshape(verts, (-1, 3)), np.float64), _a(skin["vert_body"], np.int32), _a(np.reshape(skin["face"], (-1, 3)), np.int32)
    o, d = _a(np.reshape(origin, (-1, 3)), np.float64), _a(np.reshape(direction, (-1, 3)), np.float64)
    xp = _a(np.zeros((1, 3)) if xpos is None else xpos, np.float64)
    xq = _a(np.array([[1.0, 0, 0, 0]]) if xquat is None else xquat, np.float64)
    rb = None if body is None else _a(body, np.int32)
    rx = None if exclude is None else _a(exclude, np.int32)
    n = len(o)
    dist, geom, normal = np.empty(n), np.empty(n, np.int32), np.empty((n, 3))
    L.skin_ray_host(C.c_int(layout), C.c_int(len(ty)), _p(gx), _p(gm), _p(gs), _p(ty), _p(ct), _p(gb), _p(hid), C.c_int(len(vs)), _p(vs), _p(vb),
                    C.c_int(len(fc)), _p(fc), _p(xp), _p(xq), C.c_int(n), _p(o), _p(d), _p(rb), _p(rx), C.c_int(int(cat_mask)), C.c_double(float(max_dist)),
                    _p(dist), _p(geom), _p(normal))
    return dist, geom, normal
