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


# ---- the g++ build: tests/ray_ref.py's (one driver over csrc/sg_ray_walk.h for the plain call and this one) ----
build_host = RR.build_host


def vertices_with(L, skin, xpos, xquat):
    vb, vp = RR._a(skin["vert_body"], np.int32), RR._a(skin["vert_pos"], np.float64)
    xp, xq = RR._a(xpos, np.float64), RR._a(xquat, np.float64)
    out = np.empty((len(vb), 3))
    L.skin_vertex_host(C.c_int(len(vb)), RR._p(vb), RR._p(vp), RR._p(xp), RR._p(xq), RR._p(out))
    return out


def cast_with(L, gx, gm, types, sizes, cats, geom_body, skin, verts, origin, direction, xpos=None, xquat=None, body=None, exclude=None,
              cat_mask=RR.ALL_BITS, max_dist=0.0, layout=0):
    """the host build on the same inputs (body-frame rays mapped by the header's own code) -> dist, id, normal"""
    return RR.cast_host(L, gx, gm, types, sizes, cats, geom_body, hidden_geoms(geom_body, skin), verts, skin["vert_body"], skin["face"], origin,
                        direction, xpos, xquat, body, exclude, cat_mask, max_dist, layout)
