// sg_ray.h -- the per-(ray, geom) math of sg_ray (mj_ray in fp64): ray - primitive intersection, hit normal, bounding-sphere early-out, the body
// frame -> world map of a ray, one visit of a walker and the order hits are reduced by.  The traversal itself is sg_ray_walk.h.
//
// Plain C++: the ray kernels compile it for the device (sg_ray_kernels.h, sg_ray_skin_kernels.h), and through sg_ray_walk.h the g++ build of
// tests/ray_ref.py (tests/test_ray_host.py, against that file's independent NumPy caster) and scripts/sanitize/ray_skin_main.cpp for the
// host.  The renderer's header (sg_render.h) is NOT shared: its rays leave one eye in fp32 and its records are relative
// to that eye; a ray query has any origin, per env, and needs fp64 (millimetre gaps 1.7 m from the world origin).
//
// A geom is one record of SGY_REC doubles (128 B), world frame:
//   rec[0..2]   centre
//   rec[3..11]  orientation, row-major: world = R * local
//   rec[12..14] geom_size
//   rec[15]     the bits of an int: geom type | category << 8 | body id << 16
// Rules (the renderer's, restated in include/softgrip.h): only entry hits count -- the smallest root t > 0 at which the ray crosses the
// surface from outside, so an origin inside a geom does not see that geom (mj_ray reports the exit there); planes are one-sided (seen
// from their +z side); of equal distances the smaller geom id wins.  A capsule's cap counts on its outer hemisphere only (the inner
// half of the cap's sphere lies inside the cylinder: no surface).
//
// Every function computes with contraction OFF: no fused multiply-add is formed that the source does not spell, so the two kernel
// layouts, which inline this code into different surroundings, and the g++ build give the same bits for the same (ray, geom).
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define SGY_HD __host__ __device__ __forceinline__
#else
#define SGY_HD inline
#endif
#if defined(__clang__)
#define SGY_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define SGY_NO_CONTRACT
#endif

#define SGY_REC 16        // doubles per geom record
#define SGY_MAXGEOM 320   // records one workgroup stages in LDS (320 x 128 B = 40 KB): the renderer's limit

enum { SGY_PLANE = 0, SGY_SPHERE = 2, SGY_CAPSULE = 3, SGY_BOX = 6 };

SGY_HD int sgy_meta(int type, int cat, int body) { return (type & 0xFF) | ((cat & 0xFF) << 8) | (body << 16); }
SGY_HD int sgy_meta_type(int m) { return m & 0xFF; }
SGY_HD int sgy_meta_cat(int m) { return (m >> 8) & 0xFF; }
SGY_HD int sgy_meta_body(int m) { return m >> 16; }
SGY_HD double sgy_meta_word(int m) { double w = 0.0; memcpy(&w, &m, 4); return w; }
SGY_HD int sgy_word_meta(double w) { int m; memcpy(&m, &w, 4); return m; }

// is the geom a candidate of the ray?  (category bit of cat_mask set, not a geom of the excluded body)
SGY_HD bool sgy_candidate(int meta, int cat_mask, int exclude) {
  return ((cat_mask >> sgy_meta_cat(meta)) & 1) && !(exclude >= 0 && sgy_meta_body(meta) == exclude);
}

// bounding radius about the geom's centre (planes: none)
SGY_HD double sgy_bound(int type, const double* s) {
  SGY_NO_CONTRACT
  switch (type) {
    case SGY_SPHERE: return s[0];
    case SGY_CAPSULE: return s[0] + s[1];
    case SGY_BOX: return sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]);
    default: return INFINITY;
  }
}

// can the ray o + t d (d unit, t > 0) meet the geom's bounding sphere at a distance that still matters (t <= limit)?  Conservative: the
// radius is widened by 1e-6 of itself plus 1e-9 m, orders above the rounding of the test, so a geom it drops has no hit the full
// intersection would report.
SGY_HD bool sgy_bound_keep(int type, const double* c, const double* s, const double* o, const double* d, double limit) {
  SGY_NO_CONTRACT
  const double R = sgy_bound(type, s);
  if (!(R < INFINITY)) return true;
  const double Rw = R * (1.0 + 1e-6) + 1e-9;
  const double p0 = c[0] - o[0], p1 = c[1] - o[1], p2 = c[2] - o[2];
  const double a = p0 * d[0] + p1 * d[1] + p2 * d[2];            // distance of the closest approach along the ray
  const double q0 = p0 - a * d[0], q1 = p1 - a * d[1], q2 = p2 - a * d[2];
  if (q0 * q0 + q1 * q1 + q2 * q2 > Rw * Rw) return false;         // the line passes outside
  if (a + Rw < 0.0) return false;                                  // the sphere lies behind the origin
  return a - Rw <= limit;                                          // every point of it is farther than what is wanted
}

// smallest root t > 0 of |o + t d - (0, 0, cz)|^2 = r^2 (d unit) through the closest-approach point: no cancellation of |o - c|^2
// against r^2.  INFINITY: none (the origin inside the sphere has a negative entry root)
SGY_HD double sgy_sphere_t(const double* o, const double* d, double cz, double r) {
  SGY_NO_CONTRACT
  const double oz = o[2] - cz;
  const double tl = -(o[0] * d[0] + o[1] * d[1] + oz * d[2]);
  const double q0 = o[0] + tl * d[0], q1 = o[1] + tl * d[1], q2 = oz + tl * d[2];
  const double h2 = r * r - (q0 * q0 + q1 * q1 + q2 * q2);
  if (!(h2 >= 0.0)) return INFINITY;
  const double t = tl - sqrt(h2);
  return t > 0.0 ? t : INFINITY;
}

// ray (world origin o, unit direction d) into the geom's frame
SGY_HD void sgy_to_local(const double* c, const double* R, const double* o, const double* d, double* ol, double* dl) {
  SGY_NO_CONTRACT
  const double p0 = o[0] - c[0], p1 = o[1] - c[1], p2 = o[2] - c[2];
  for (int k = 0; k < 3; k++) {
    ol[k] = R[k] * p0 + R[3 + k] * p1 + R[6 + k] * p2;
    dl[k] = R[k] * d[0] + R[3 + k] * d[1] + R[6 + k] * d[2];
  }
}

// ray against one geom (centre c, orientation R, size s): the entry distance, INFINITY for none.  *ax: the box face's axis (0 otherwise)
SGY_HD double sgy_intersect(int type, const double* c, const double* R, const double* s, const double* o, const double* d, int* ax) {
  SGY_NO_CONTRACT
  double ol[3], dl[3];
  sgy_to_local(c, R, o, d, ol, dl);
  double t = INFINITY;
  *ax = 0;
  switch (type) {
    case SGY_PLANE: {
      if (dl[2] < 0.0 && ol[2] > 0.0) {
        const double tt = -ol[2] / dl[2];
        const double x = ol[0] + tt * dl[0], y = ol[1] + tt * dl[1];
        const bool bounded = s[0] > 0.0 && s[1] > 0.0;
        if (!bounded || (fabs(x) <= s[0] && fabs(y) <= s[1])) t = tt;
      }
      break;
    }
    case SGY_SPHERE: t = sgy_sphere_t(ol, dl, 0.0, s[0]); break;
    case SGY_CAPSULE: {
      const double r = s[0], hl = s[1];
      const double a = dl[0] * dl[0] + dl[1] * dl[1];
      if (a > 1e-24) {   // the side: infinite cylinder, entry root within |z| <= hl
        const double tl = -(ol[0] * dl[0] + ol[1] * dl[1]) / a;
        const double q0 = ol[0] + tl * dl[0], q1 = ol[1] + tl * dl[1];
        const double h2 = r * r - (q0 * q0 + q1 * q1);
        if (h2 >= 0.0) {
          const double tt = tl - sqrt(h2 / a);
          if (tt > 0.0 && fabs(ol[2] + tt * dl[2]) <= hl) t = tt;
        }
      }
      const double tp = sgy_sphere_t(ol, dl, hl, r);      // the caps: outer hemispheres only
      if (tp < t && ol[2] + tp * dl[2] >= hl) t = tp;
      const double tm = sgy_sphere_t(ol, dl, -hl, r);
      if (tm < t && ol[2] + tm * dl[2] <= -hl) t = tm;
      break;
    }
    case SGY_BOX: {
      double tn = -INFINITY, tf = INFINITY;
      int axis = -1;
      bool miss = false;
      for (int k = 0; k < 3; k++) {
        if (dl[k] == 0.0) {   // parallel to the slab: inside it or a miss
          if (fabs(ol[k]) > s[k]) miss = true;
          continue;
        }
        double t1 = (-s[k] - ol[k]) / dl[k], t2 = (s[k] - ol[k]) / dl[k];
        if (t1 > t2) { const double x = t1; t1 = t2; t2 = x; }
        if (t1 > tn) { tn = t1; axis = k; }
        tf = fmin(tf, t2);
      }
      if (!miss && axis >= 0 && tn <= tf && tn > 0.0) { t = tn; *ax = axis; }
      break;
    }
    default: break;
  }
  return t;
}

// outward unit normal (world axes) at the hit of distance t; ax: what sgy_intersect gave
SGY_HD void sgy_normal(int type, const double* c, const double* R, const double* s, const double* o, const double* d, double t, int ax, double* n) {
  SGY_NO_CONTRACT
  double ol[3], dl[3], nl[3] = {0.0, 0.0, 1.0};
  sgy_to_local(c, R, o, d, ol, dl);
  const double h0 = ol[0] + t * dl[0], h1 = ol[1] + t * dl[1], h2 = ol[2] + t * dl[2];
  if (type == SGY_SPHERE) {
    nl[0] = h0 / s[0]; nl[1] = h1 / s[0]; nl[2] = h2 / s[0];
  } else if (type == SGY_CAPSULE) {
    const double zc = fmin(s[1], fmax(-s[1], h2));
    nl[0] = h0 / s[0]; nl[1] = h1 / s[0]; nl[2] = (h2 - zc) / s[0];
  } else if (type == SGY_BOX) {
    for (int k = 0; k < 3; k++) nl[k] = k == ax ? (dl[k] > 0.0 ? -1.0 : 1.0) : 0.0;
  }
  for (int k = 0; k < 3; k++) n[k] = R[3 * k] * nl[0] + R[3 * k + 1] * nl[1] + R[3 * k + 2] * nl[2];
}

// rotation matrix (row-major) of a unit quaternion (w, x, y, z)
SGY_HD void sgy_quat_mat(const double* q, double* M) {
  SGY_NO_CONTRACT
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  M[0] = w * w + x * x - y * y - z * z; M[1] = 2 * (x * y - w * z); M[2] = 2 * (x * z + w * y);
  M[3] = 2 * (x * y + w * z); M[4] = w * w - x * x + y * y - z * z; M[5] = 2 * (y * z - w * x);
  M[6] = 2 * (x * z - w * y); M[7] = 2 * (y * z + w * x); M[8] = w * w - x * x - y * y + z * z;
}

// a ray given in a body's frame (xpos / xquat: that body's pose; NULL: the world frame) -> world origin and UNIT direction.
// false: the direction has no length or a component that is not finite (the ray is a miss)
SGY_HD bool sgy_map_ray(const double* xpos, const double* xquat, const double* o_in, const double* d_in, double* o, double* d) {
  SGY_NO_CONTRACT
  if (xpos) {
    double M[9];
    sgy_quat_mat(xquat, M);
    for (int k = 0; k < 3; k++) {
      o[k] = xpos[k] + (M[3 * k] * o_in[0] + M[3 * k + 1] * o_in[1] + M[3 * k + 2] * o_in[2]);
      d[k] = M[3 * k] * d_in[0] + M[3 * k + 1] * d_in[1] + M[3 * k + 2] * d_in[2];
    }
  } else {
    for (int k = 0; k < 3; k++) { o[k] = o_in[k]; d[k] = d_in[k]; }
  }
  const double l = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
  if (!(l > 0.0) || !(l < INFINITY)) return false;
  for (int k = 0; k < 3; k++) d[k] = d[k] / l;
  return true;
}

// the best hit so far of one walker; sgy_better is the order BOTH layouts reduce by: smaller t, then smaller geom id
struct SgyBest {
  double t;   // INFINITY: none
  int geom;   // -1: none
  int ax;
};
SGY_HD bool sgy_better(double t, int g, double bt, int bg) { return t < bt || (t == bt && t < INFINITY && g < bg); }

// one (ray, geom): the candidate and bounding tests first, then the full intersection; the walker's best is updated
SGY_HD void sgy_visit(int g, const double* rec, const double* o, const double* d, int cat_mask, int exclude, double limit, SgyBest* b) {
  const int meta = sgy_word_meta(rec[15]);
  if (!sgy_candidate(meta, cat_mask, exclude)) return;
  const int type = sgy_meta_type(meta);
  if (!sgy_bound_keep(type, rec, rec + 12, o, d, b->t < limit ? b->t : limit)) return;
  int ax;
  const double t = sgy_intersect(type, rec, rec + 3, rec + 12, o, d, &ax);
  if (sgy_better(t, g, b->t, b->geom)) { b->t = t; b->geom = g; b->ax = ax; }
}

// the result of a ray from its reduced best: distance (-1: miss), geom id (-1), normal (zeros).  limit: max_dist, INFINITY for none
SGY_HD void sgy_finish(const SgyBest& b, const double* rec, const double* o, const double* d, double limit, double* dist, int* geom, double* n) {
  if (b.geom < 0 || !(b.t <= limit)) {
    *dist = -1.0; *geom = -1;
    n[0] = n[1] = n[2] = 0.0;
    return;
  }
  *dist = b.t; *geom = b.geom;
  sgy_normal(sgy_meta_type(sgy_word_meta(rec[15])), rec, rec + 3, rec + 12, o, d, b.t, b.ax, n);
}
