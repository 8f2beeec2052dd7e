"""Independent NumPy (fp64) caster for the renderer's skin path (sg_render_ex with SG_RENDER_SKIN; soft-grip_amd/csrc/sg_render.h): the
geoms through tests/render_ref.py's primitives, the skin's triangles from the rules the header documents and not from its code:

* a vertex sits at xpos[body] + xmat[body] @ vert_pos; the geoms of the bodies the vertices are bound to are not drawn;
* the ray starts at the eye, so the edge value of edge (p, q) is d . (p x q) with p, q relative to the eye, taken with the endpoint of
  smaller vertex index first and oriented per triangle (a, b, c) as E_ab = d . (b x a); a hit when all three are >= 0;
* front faces only: t = (n . a) / (n . d), n = (b - a) x (c - a), n . d < 0, t > 0; of equal t the smaller face index wins, and a geom
  wins against a triangle;
* shading: albedo = the skin's rgb, normal = the blend of the vertex normals with the weights (E_bc, E_ca, E_ab), normalised; a vertex
  normal is the normalised sum of the n of its faces, and the face's own normal stands in where a sum (or the blend) has no length;
* a skin pixel reports segid = ngeom.

compare() is render_ref.compare with the one extension for a surface that can fold over itself: the reference also returns the face
index, and a pixel counts as silhouette when a 4-neighbour has another segid or a face that shares no vertex with its own."""
import ctypes as C

import numpy as np

import host_build
import render_ref as R


def skin_vertices(skin, xpos, xmat):
    """world positions [nvert, 3] of the skin's vertices from body poses xpos [nbody, 3], xmat [nbody, 3, 3]"""
    b = np.asarray(skin["vert_body"])
    return np.asarray(xpos)[b] + np.einsum("vij,vj->vi", np.asarray(xmat).reshape(-1, 3, 3)[b], np.asarray(skin["vert_pos"], dtype=np.float64))


def hidden_geoms(model, skin):
    """[ngeom] bool: geoms of the bodies the skin's vertices are bound to"""
    return np.isin(np.asarray(model.geom_bodyid), np.asarray(skin["vert_body"]))


def vertex_normals(verts, face):
    a, b, c = (verts[face[:, k]] for k in range(3))
    n = np.cross(b - a, c - a)
    s = np.zeros_like(verts)
    for k in range(3):
        np.add.at(s, face[:, k], n)
    ln = np.linalg.norm(s, axis=1, keepdims=True)
    return np.where(ln > 0, s / np.where(ln > 0, ln, 1.0), 0.0)


def _edge(d, p, q, ip, iq):
    """oriented value E_pq = d . (q x p), the endpoint of smaller index first"""
    return -np.sum(d * np.cross(p, q), -1) if ip < iq else np.sum(d * np.cross(q, p), -1)


def cast_triangles(d, verts, face):
    """rays from 0 along unit d [N, 3] against triangles of verts (relative to the ray origin): t [N] (inf: none), face [N] (-1), weights [N, 3]"""
    n_ray = len(d)
    best = np.full(n_ray, np.inf)
    bf = np.full(n_ray, -1, dtype=np.int32)
    bw = np.zeros((n_ray, 3))
    for f, (ia, ib, ic) in enumerate(np.asarray(face)):
        a, b, c = verts[ia], verts[ib], verts[ic]
        eab, ebc, eca = _edge(d, a, b, ia, ib), _edge(d, b, c, ib, ic), _edge(d, c, a, ic, ia)
        n = np.cross(b - a, c - a)
        den = d @ n
        with np.errstate(divide="ignore", invalid="ignore"):
            t = (n @ a) / den
        ok = (eab >= 0) & (ebc >= 0) & (eca >= 0) & (den < 0) & (t > 0) & np.isfinite(t) & (t < best)
        best = np.where(ok, t, best)
        bf = np.where(ok, f, bf)
        bw = np.where(ok[:, None], np.stack([ebc, eca, eab], -1), bw)
    return best, bf, bw


def render(gx, gm, types, sizes, cats, cam, width, height, verts, face, rgb, hidden):
    """-> depth [H, W] (inf background), seg [H, W] int32 (-1; ngeom on the skin), rgb [H, W, 3] uint8, checker-line pixels [H, W] bool
    (as render_ref.render) and the hit face [H, W] int32 (-1 off the skin)"""
    eye, f, d = R.camera_rays(cam, width, height)
    d = d.reshape(-1, 3)
    ng = len(types)
    T = np.full((ng, len(d)), np.inf)
    NL = np.zeros((ng, len(d), 3))
    for g in range(ng):
        if hidden[g]:
            continue
        Rm = gm[g]
        T[g], NL[g] = R._intersect(int(types[g]), np.asarray(sizes[g], dtype=np.float64), Rm.T @ (eye - gx[g]), d @ Rm)
    seg = np.argmin(T, 0)
    t = T[seg, np.arange(len(d))]
    rel = np.asarray(verts, dtype=np.float64) - eye
    face = np.asarray(face)
    tt, tf, tw = cast_triangles(d, rel, face)
    skin = tt < t                                  # (a geom wins at equal distance)
    t = np.where(skin, tt, t)
    hitm = np.isfinite(t)
    seg = np.where(skin, ng, np.where(hitm, seg, -1))
    depth = np.where(hitm, t * (d @ f), np.inf)
    vn = vertex_normals(rel, face)
    out = np.tile(R.u8(R.BACKGROUND), (len(d), 1))
    edge = np.zeros(len(d), bool)
    for p in np.flatnonzero(hitm):
        if skin[p]:
            ia, ib, ic = face[tf[p]]
            fn = np.cross(rel[ib] - rel[ia], rel[ic] - rel[ia])
            fn = fn / np.linalg.norm(fn)
            n = sum(tw[p, k] * (vn[v] if vn[v].any() else fn) for k, v in enumerate((ia, ib, ic)))
            ln = np.linalg.norm(n)
            n = n / ln if ln > 0 else fn
            alb = np.asarray(rgb[:3], dtype=np.float64)
        else:
            g = seg[p]
            Rm = gm[g]
            n = Rm @ NL[g, p]
            c = cats[g]
            if c == R.GROUND:
                hl = Rm.T @ (eye + t[p] * d[p] - gx[g])
                alb = R.CHECKER[int(np.floor(hl[0] / 0.5) + np.floor(hl[1] / 0.5)) % 2]
                fr = np.abs(hl[:2] / 0.5 - np.round(hl[:2] / 0.5)) * 0.5
                edge[p] = fr.min() < 1e-4
            else:
                alb = R.ALBEDO.get(int(c), R.ALBEDO[R.STATIC])
        shade = 0.25 + 0.45 * max(0.0, -(n @ f)) + 0.30 * max(0.0, n[2])
        out[p] = R.u8(np.array(alb) * shade)
    sh = (height, width)
    return (depth.reshape(sh), seg.reshape(sh).astype(np.int32), out.reshape(height, width, 3), edge.reshape(sh),
            np.where(skin, tf, -1).reshape(sh).astype(np.int32))


def render_model(model, skin, qpos, cam, width, height, cats=None):
    kin = model.kinematics(np.asarray(qpos, dtype=np.float64))
    gx, gm = R.geom_poses(model, qpos)
    return render(gx, gm, model.geom_type, model.geom_size, R.categories(model) if cats is None else cats, cam, width, height,
                  skin_vertices(skin, kin["xpos"], kin["xmat"]), skin["face"], skin["rgba"], hidden_geoms(model, skin))


def fold_silhouette(fidx, face):
    """skin pixels with a 4-neighbour on a face that shares no vertex with their own (the surface folds over itself there)"""
    face = np.asarray(face)
    nf = len(face)
    share = np.zeros((nf + 1, nf + 1), bool)        # (row / column nf: off the skin, never a fold)
    inc = np.zeros((nf, int(face.max()) + 1), bool)
    inc[np.arange(nf)[:, None], face] = True
    share[:nf, :nf] = (inc.astype(np.int32) @ inc.T.astype(np.int32)) > 0
    share[nf, :] = share[:, nf] = True
    fi = np.where(fidx < 0, nf, fidx)
    s = np.zeros(fidx.shape, bool)
    s[1:] |= ~share[fi[1:], fi[:-1]]
    s[:-1] |= ~share[fi[:-1], fi[1:]]
    s[:, 1:] |= ~share[fi[:, 1:], fi[:, :-1]]
    s[:, :-1] |= ~share[fi[:, :-1], fi[:, 1:]]
    return s


FOLD_CAP = 0.02     # pixels that count as silhouette for the fold alone: at most 2 % of an image


def fold_fraction(ref, face):
    return float((fold_silhouette(ref[4], face) & ~R.silhouette(ref[1])).mean())


def compare(ref, got, face, what=""):
    """render_ref.compare's criteria -- depth within 1e-4 m off the silhouettes, at most 0.5 % differing ids and only on silhouettes, rgb
    within 2 levels where the ids agree (off the checker lines) -- with the silhouette extended by the folds of the skin (it governs the
    depth and id checks; the colour check is render_ref.compare's, fold pixels included)"""
    rd, rs, rc, redge, rf = ref
    gd, gs, gc = got
    fold = fold_silhouette(rf, face)
    plain = R.silhouette(rs)
    assert (fold & ~plain).mean() <= FOLD_CAP, "%s: %.2f %% of the pixels are fold silhouettes" % (what, 100 * (fold & ~plain).mean())
    sil = plain | fold
    diff = rs != gs
    assert diff.mean() <= 0.005, "%s: %d of %d pixels differ in segid" % (what, diff.sum(), diff.size)
    assert not (diff & ~sil).any(), "%s: segid differs off the silhouettes at %s" % (what, np.argwhere(diff & ~sil)[:5].tolist())
    inner = ~sil & ~diff
    both = inner & np.isfinite(rd)
    assert (np.isfinite(gd) == np.isfinite(rd))[inner].all(), what
    if both.any():
        err = np.abs(gd.astype(np.float64) - rd)[both].max()
        assert err <= 1e-4, "%s: depth off by %.3g m" % (what, err)
    same = ~diff & ~redge
    cerr = np.abs(gc.astype(np.int32) - rc.astype(np.int32)).max(-1)
    assert cerr[same].max(initial=0) <= 2, "%s: rgb off by %d levels at %s" % (what, cerr[same].max(), np.argwhere(same & (cerr > 2))[:5].tolist())


# ---- the g++ build of sg_render.h's skin path: camera, tile culling of geoms and triangles, vertex normals and trace, as the kernels do ----
HOST_DRIVER = r"""
#include <vector>
#include "sg_skin.h"
extern "C" void skin_render_host(const double* cam, int W, int H, int ng, const double* gx, const double* gm, const double* gs, const int* type,
                                 const int* cat, const int* hidden, int nvert, const double* verts, int nface, const int* face, const float* rgb,
                                 float* depth, int* seg, unsigned char* rgba, int* fidx) {
  SgrCam c;
  double eye[3];
  sgr_camera(cam, W, H, eye, &c);
  std::vector<float> recs((size_t)ng * SGR_REC);
  for (int g = 0; g < ng; g++) sgr_make_record(gx + 3 * g, gm + 9 * g, gs + 3 * g, type[g], cat[g], eye, &recs[(size_t)SGR_REC * g]);
  SgSkinHost S;
  S.nvert = nvert; S.nface = nface;
  S.vert_body.assign(nvert, 0);
  S.face.assign(face, face + 3 * nface);
  SgSkinTables T;
  std::vector<int> gb(ng, 0);
  sg_skin_tables(S, gb.data(), ng, 1, &T);
  std::vector<float> vpos(4 * (size_t)nvert, 0.0f), vrec((size_t)SGR_VREC * nvert, 0.0f);
  for (int v = 0; v < nvert; v++)
    for (int k = 0; k < 3; k++) vpos[4 * v + k] = (float)(verts[3 * v + k] - eye[k]);
  for (int v = 0; v < nvert; v++) {
    for (int k = 0; k < 3; k++) vrec[SGR_VREC * v + k] = vpos[4 * v + k];
    sgr_vertex_normal(v, vpos.data(), T.faces.data(), T.adj_start.data(), T.adj.data(), &vrec[SGR_VREC * v + 4]);
  }
  std::vector<unsigned short> list(ng), flist(nface);
  for (int ty = 0; ty < (H + SGR_TILE - 1) / SGR_TILE; ty++)
    for (int tx = 0; tx < (W + SGR_TILE - 1) / SGR_TILE; tx++) {
      const int i0 = tx * SGR_TILE, j0 = ty * SGR_TILE, i1 = i0 + SGR_TILE - 1 < W - 1 ? i0 + SGR_TILE - 1 : W - 1, j1 = j0 + SGR_TILE - 1 < H - 1 ? j0 + SGR_TILE - 1 : H - 1;
      float d0[3], d1[3], d2[3], d3[3], axis[3], cs, sn;
      sgr_ray(c, i0, j0, d0); sgr_ray(c, i1, j0, d1); sgr_ray(c, i0, j1, d2); sgr_ray(c, i1, j1, d3);
      sgr_tile_cone(d0, d1, d2, d3, axis, &cs, &sn);
      int n = 0, nf = 0;
      for (int g = 0; g < ng; g++)
        if (!hidden[g] && sgr_cone_keep(&recs[(size_t)SGR_REC * g], axis, cs, sn)) list[n++] = (unsigned short)g;
      for (int f = 0; f < nface; f++) {
        const uint32_t w = T.faces[f];
        if (sgr_tri_cone_keep(&vpos[4 * (w & 0xFF)], &vpos[4 * ((w >> 8) & 0xFF)], &vpos[4 * ((w >> 16) & 0xFF)], axis, cs, sn)) flist[nf++] = (unsigned short)f;
      }
      for (int j = j0; j <= j1; j++)
        for (int i = i0; i <= i1; i++) {
          float d[3];
          sgr_ray(c, i, j, d);
          int fi = -1;
          SgrHit h = sgr_trace_skin(recs.data(), list.data(), n, vpos.data(), T.faces.data(), flist.data(), nf, vrec.data(), rgb, ng, c, d, &fi);
          const size_t p = (size_t)j * W + i;
          depth[p] = h.depth; seg[p] = h.geom; fidx[p] = fi;
          for (int k = 0; k < 4; k++) rgba[4 * p + k] = h.rgba[k];
        }
    }
}

// rays from 0 along d [n][3] against one triangle each: a, b, c [n][3] with vertex indices idx [n][3] -> t [n], w [n][3]
extern "C" void tri_host(int n, const float* d, const float* a, const float* b, const float* c, const int* idx, float* t, float* w) {
  for (int i = 0; i < n; i++) {
    SgrRayFrame fr;
    sgr_ray_frame(d + 3 * i, &fr);
    w[3 * i] = w[3 * i + 1] = w[3 * i + 2] = 0.0f;
    t[i] = sgr_tri(d + 3 * i, fr, a + 3 * i, idx[3 * i], b + 3 * i, idx[3 * i + 1], c + 3 * i, idx[3 * i + 2], w + 3 * i);
  }
}

// rays from 0 along d [n][3] against a whole mesh (verts [nvert][3] fp32, every face tried): t [n] and face [n] (-1: no hit)
extern "C" void mesh_host(int n, const float* d, int nvert, const float* verts, int nface, const int* face, float* t, int* fidx) {
  for (int i = 0; i < n; i++) {
    SgrRayFrame fr;
    sgr_ray_frame(d + 3 * i, &fr);
    t[i] = INFINITY; fidx[i] = -1;
    for (int f = 0; f < nface; f++) {
      const int* q = face + 3 * f;
      float w[3];
      const float tt = sgr_tri(d + 3 * i, fr, verts + 3 * q[0], q[0], verts + 3 * q[1], q[1], verts + 3 * q[2], q[2], w);
      if (tt < t[i]) { t[i] = tt; fidx[i] = f; }
    }
  }
}
"""


def build_host(tmpdir):
    """compiles the driver above (sg_render.h, sg_skin.h) with g++ into tmpdir -> the ctypes library"""
    L = host_build.build(tmpdir, "skin_host", HOST_DRIVER)
    for fn in (L.skin_render_host, L.tri_host, L.mesh_host):
        fn.restype = None
    return L


def _p(x):
    return x.ctypes.data_as(C.c_void_p)


def render_with(L, gx, gm, types, sizes, cats, cam, width, height, verts, face, rgb, hidden):
    a = lambda x, dt: np.ascontiguousarray(x, dtype=dt)  # noqa: E731
    gx, gm, gs = a(gx, np.float64), a(np.reshape(gm, (-1, 9)), np.float64), a(sizes, np.float64)
    ty, ct, cm, hd = a(types, np.int32), a(cats, np.int32), a(cam, np.float64), a(hidden, np.int32)
    vs, fc, col = a(verts, np.float64), a(face, np.int32), a(rgb, np.float32)
    depth = np.empty((height, width), np.float32)
    seg = np.empty((height, width), np.int32)
    fidx = np.empty((height, width), np.int32)
    rgba = np.empty((height, width, 4), np.uint8)
    L.skin_render_host(_p(cm), C.c_int(width), C.c_int(height), C.c_int(len(ty)), _p(gx), _p(gm), _p(gs), _p(ty), _p(ct), _p(hd), C.c_int(len(vs)),
                       _p(vs), C.c_int(len(fc)), _p(fc), _p(col), _p(depth), _p(seg), _p(rgba), _p(fidx))
    return depth, seg, rgba, fidx


def tri_with(L, d, a, b, c, idx):
    f = lambda x: np.ascontiguousarray(x, dtype=np.float32)  # noqa: E731
    d, a, b, c, idx = f(d), f(a), f(b), f(c), np.ascontiguousarray(idx, dtype=np.int32)
    t, w = np.empty(len(d), np.float32), np.empty((len(d), 3), np.float32)
    L.tri_host(C.c_int(len(d)), _p(d), _p(a), _p(b), _p(c), _p(idx), _p(t), _p(w))
    return t, w


def mesh_with(L, d, verts, face):
    d, verts, face = np.ascontiguousarray(d, dtype=np.float32), np.ascontiguousarray(verts, dtype=np.float32), np.ascontiguousarray(face, dtype=np.int32)
    t, fidx = np.empty(len(d), np.float32), np.empty(len(d), np.int32)
    L.mesh_host(C.c_int(len(d)), _p(d), C.c_int(len(verts)), _p(verts), C.c_int(len(face)), _p(face), _p(t), _p(fidx))
    return t, fidx
