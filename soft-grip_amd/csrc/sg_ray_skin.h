// sg_ray_skin.h -- the per-(ray, triangle) math of sg_ray with SG_RAY_SKIN: the soft object's skin (sg_skin.h: triangles bound to bodies) as
// candidates of a ray query, in fp64.  Plain C++ like sg_ray.h, and compiled by the same three: the ray kernels (sg_ray_skin_kernels.h), the g++ test build (tests/test_ray_skin_host.py, against the NumPy caster tests/ray_skin_ref.py) and the sanitizer
// program -- all but the lane-per-ray kernel through the traversal in sg_ray_walk.h.
//
// Rules (include/softgrip.h restates them):
//   * a vertex sits at xpos[body] + R(xquat[body]) vert_pos (sgys_vertex); a triangle is taken relative to the ray's origin;
//   * front faces only, counter-clockwise seen from outside: n = (b - a) x (c - a), n . d < 0, t = (n . a) / (n . d) > 0.  The entry-hit rule of
//     sg_ray.h: an origin inside the closed skin sees nothing of it;
//   * the id of face f is ngeom + f, ordered with the geoms by sgy_better: smaller t, then smaller id -- a geom wins a tie against a triangle,
//     the smaller face index among triangles;
//   * the normal is the unit face normal n / |n|: flat, not interpolated;
//   * a triangle with a vertex bound to the ray's excluded body is no candidate.
// Watertightness: the edge value d . (p x q) is taken in a frame built from the ray direction, u x w = d, as
// (p.u)(q.w) - (p.w)(q.u).  The two coordinates of a vertex are fp64 numbers that depend on ray and vertex alone (explicit fma in a fixed
// order: every triangle that uses the vertex gets the same bits).  The difference of the two products is NOT exact in fp64, so both are
// split into head and rounding error with fma (sgys_cross2): its sign is the exact sign for those projected points, and its value is
// computed once per edge, the endpoint of smaller vertex index first.  So the triangles around an edge or a vertex tile the ray's plane
// without a gap: a ray that crosses the closed skin from outside hits it, also exactly through an edge or a vertex (zero counts as inside).
//
// Contraction is OFF as in sg_ray.h; the fma calls spelled here are the only fused operations.
#pragma once
#include "sg_ray.h"

#define SGYS_MAXVERT 256   // sg_model_set_skin's limits (SGR_MAXVERT, SGR_MAXFACE)
#define SGYS_MAXFACE 512
#define SGYS_CAT_ELEM 3    // the category whose bit in cat_mask (SG_RAY_ELEM) makes the skin's triangles candidates

// the three vertex indices of a packed face (sgr_pack_face: a byte each)
SGY_HD void sgys_face(uint32_t w, int* ia, int* ib, int* ic) { *ia = (int)(w & 0xFF); *ib = (int)((w >> 8) & 0xFF); *ic = (int)((w >> 16) & 0xFF); }

// world position of a vertex given in its body's frame
SGY_HD void sgys_vertex(const double* xpos, const double* xquat, const double* vp, double* out) {
  SGY_NO_CONTRACT
  double M[9];
  sgy_quat_mat(xquat, M);
  for (int k = 0; k < 3; k++) out[k] = xpos[k] + (M[3 * k] * vp[0] + M[3 * k + 1] * vp[1] + M[3 * k + 2] * vp[2]);
}

// the ray's own frame: u, w (nearly) orthonormal with u x w = d.  Any rounding in it moves every projected vertex alike
struct SgysFrame { double u[3], w[3]; };

SGY_HD void sgys_frame(const double* d, SgysFrame* fr) {
  SGY_NO_CONTRACT
  const double ax = fabs(d[0]), ay = fabs(d[1]), az = fabs(d[2]);
  double e[3] = {0.0, 0.0, 0.0};
  e[ax <= ay && ax <= az ? 0 : (ay <= az ? 1 : 2)] = 1.0;   // the axis d leans on least
  const double u[3] = {d[1] * e[2] - d[2] * e[1], d[2] * e[0] - d[0] * e[2], d[0] * e[1] - d[1] * e[0]};
  const double l = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
  for (int k = 0; k < 3; k++) fr->u[k] = u[k] / l;
  fr->w[0] = d[1] * fr->u[2] - d[2] * fr->u[1]; fr->w[1] = d[2] * fr->u[0] - d[0] * fr->u[2]; fr->w[2] = d[0] * fr->u[1] - d[1] * fr->u[0];
}

// one coordinate of a vertex (relative to the origin) in the ray's frame: a fixed order of fused operations
SGY_HD double sgys_coord(const double* p, const double* a) { return fma(p[0], a[0], fma(p[1], a[1], p[2] * a[2])); }

// pu qw - pw qu with the EXACT sign (and zero only when the two products are equal): a product is its rounded head plus the error fma
// returns; rounding is monotonic, so unequal heads decide, and equal heads leave the difference of the two errors
SGY_HD double sgys_cross2(double pu, double pw, double qu, double qw) {
  SGY_NO_CONTRACT
  const double h1 = pu * qw, h2 = pw * qu;
  if (h1 != h2) return h1 - h2;
  return fma(pu, qw, -h1) - fma(pw, qu, -h2);
}

// oriented edge value E_pq = d . (q x p) of a triangle's edge p -> q from the projected endpoints: the endpoint of smaller index first
SGY_HD double sgys_edge(double pu, double pw, int ip, double qu, double qw, int iq) {
  return ip < iq ? -sgys_cross2(pu, pw, qu, qw) : sgys_cross2(qu, qw, pu, pw);
}

// ray (origin 0, unit d, frame fr) against the triangle a, b, c (relative to the origin; vertex indices ia, ib, ic): the distance, INFINITY
// for none.  Early-out: three projected vertices strictly on one side of an axis through the origin leave the origin outside the
// projected triangle, where the exact edge signs cannot all be >= 0 unless all three are zero -- a triangle seen edge-on, which is a
// miss below too.  So it drops nothing the full test would report.
SGY_HD double sgys_tri(const SgysFrame& fr, const double* d, const double* a, int ia, const double* b, int ib, const double* c, int ic) {
  SGY_NO_CONTRACT
  const double au = sgys_coord(a, fr.u), bu = sgys_coord(b, fr.u), cu = sgys_coord(c, fr.u);
  if ((au > 0.0 && bu > 0.0 && cu > 0.0) || (au < 0.0 && bu < 0.0 && cu < 0.0)) return INFINITY;
  const double aw = sgys_coord(a, fr.w), bw = sgys_coord(b, fr.w), cw = sgys_coord(c, fr.w);
  if ((aw > 0.0 && bw > 0.0 && cw > 0.0) || (aw < 0.0 && bw < 0.0 && cw < 0.0)) return INFINITY;
  const double eab = sgys_edge(au, aw, ia, bu, bw, ib);
  const double ebc = sgys_edge(bu, bw, ib, cu, cw, ic);
  const double eca = sgys_edge(cu, cw, ic, au, aw, ia);
  if (!(eab >= 0.0 && ebc >= 0.0 && eca >= 0.0)) return INFINITY;
  if (eab == 0.0 && ebc == 0.0 && eca == 0.0) return INFINITY;   // edge-on
  const double p[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, q[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
  const double n[3] = {p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0]};
  const double den = n[0] * d[0] + n[1] * d[1] + n[2] * d[2];
  if (!(den < 0.0)) return INFINITY;
  const double t = (n[0] * a[0] + n[1] * a[1] + n[2] * a[2]) / den;
  return t > 0.0 && t < INFINITY ? t : INFINITY;
}

// one (ray, face): id = ngeom + face index; va, vb, vc: world positions; vbody: the bodies the skin's vertices are bound to.  The walker's
// best is updated by the order of sgy_better, as sgy_visit does for a geom
SGY_HD void sgys_visit(int id, const double* va, int ia, const double* vb, int ib, const double* vc, int ic, const int* vbody, const SgysFrame& fr,
                       const double* o, const double* d, int exclude, SgyBest* best) {
  SGY_NO_CONTRACT
  const double a[3] = {va[0] - o[0], va[1] - o[1], va[2] - o[2]}, b[3] = {vb[0] - o[0], vb[1] - o[1], vb[2] - o[2]};
  const double c[3] = {vc[0] - o[0], vc[1] - o[1], vc[2] - o[2]};
  const double t = sgys_tri(fr, d, a, ia, b, ib, c, ic);
  if (!sgy_better(t, id, best->t, best->geom)) return;
  if (exclude >= 0 && (vbody[ia] == exclude || vbody[ib] == exclude || vbody[ic] == exclude)) return;
  best->t = t; best->geom = id; best->ax = 0;
}

// the result of a ray whose reduced best is a face (best.geom >= ngeom): distance, id and the unit face normal; a miss beyond limit
SGY_HD void sgys_finish(const SgyBest& best, const double* va, const double* vb, const double* vc, double limit, double* dist, int* geom, double* n) {
  SGY_NO_CONTRACT
  if (!(best.t <= limit)) {
    *dist = -1.0; *geom = -1;
    n[0] = n[1] = n[2] = 0.0;
    return;
  }
  *dist = best.t; *geom = best.geom;
  const double p[3] = {vb[0] - va[0], vb[1] - va[1], vb[2] - va[2]}, q[3] = {vc[0] - va[0], vc[1] - va[1], vc[2] - va[2]};
  const double m[3] = {p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0]};
  const double l = sqrt(m[0] * m[0] + m[1] * m[1] + m[2] * m[2]);
  for (int k = 0; k < 3; k++) n[k] = m[k] / l;
}
