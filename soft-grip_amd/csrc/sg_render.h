// sg_render.h -- the headless renderer's per-ray math: free camera, camera rays, ray - primitive intersection, tile culling, shading.
//
// Plain C++ that the render kernels (sg_kin_kernels.h) run per lane in fp32 and tests/test_render_host.py compiles with g++ against an
// independent NumPy ray caster (tests/render_ref.py).  A geom is one 16-float record, positioned RELATIVE TO THE CAMERA EYE: the eye is
// subtracted in fp64 before the cast (sgr_make_record), so the fp32 precision does not depend on where the scene sits.
//   rec[0..2]   centre - eye (world axes)
//   rec[3..11]  orientation, row-major: world = R * local
//   rec[12..14] geom_size
//   rec[15]     the bits of an int: geom type | category << 8
// Rules both casters share: only entry hits count (the smallest root > 0 of the primitive's surface; an eye inside a geom does not see
// it), planes are one-sided (seen from their +z side), and of two equal distances the smaller geom id wins.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define SGR_HD __host__ __device__ __forceinline__
#else
#define SGR_HD inline
#endif

#define SGR_REC 16        // floats per geom record
#define SGR_MAXGEOM 320   // records one workgroup stages in LDS (320 x 64 B = 20 KB)
#define SGR_TILE 16       // pixels per tile side: 256 lanes, one pixel each

enum { SGR_CAT_GROUND = 0, SGR_CAT_STATIC = 1, SGR_CAT_FINGER = 2, SGR_CAT_ELEM = 3, SGR_CAT_CENTER = 4 };
enum { SGR_PLANE = 0, SGR_SPHERE = 2, SGR_CAPSULE = 3, SGR_BOX = 6 };

// camera basis from cam[7] = lookat xyz, distance, azimuth, elevation, fovy (degrees): MuJoCo's free camera, up = +z
struct SgrCam {
  float fwd[3], right[3], up[3];
  float tan_half, aspect;
  int width, height;
};

SGR_HD void sgr_camera(const double* cam, int width, int height, double* eye, SgrCam* c) {
  const double d2r = 3.14159265358979323846 / 180.0;
  const double az = cam[4] * d2r, el = cam[5] * d2r;
  const double f[3] = {cos(el) * cos(az), cos(el) * sin(az), sin(el)};
  double r[3] = {f[1], -f[0], 0.0};   // forward x z
  double rn = sqrt(r[0] * r[0] + r[1] * r[1]);
  if (rn < 1e-12) { r[0] = 1.0; r[1] = 0.0; rn = 1.0; }   // looking straight up / down
  r[0] /= rn; r[1] /= rn;
  const double u[3] = {r[1] * f[2] - r[2] * f[1], r[2] * f[0] - r[0] * f[2], r[0] * f[1] - r[1] * f[0]};   // right x forward
  for (int k = 0; k < 3; k++) {
    eye[k] = cam[k] - cam[3] * f[k];
    c->fwd[k] = (float)f[k]; c->right[k] = (float)r[k]; c->up[k] = (float)u[k];
  }
  c->tan_half = (float)tan(0.5 * cam[6] * d2r);
  c->aspect = (float)width / (float)height;
  c->width = width; c->height = height;
}

// unit direction of the ray through the centre of pixel (i, j); row 0 is the top of the image
SGR_HD void sgr_ray(const SgrCam& c, int i, int j, float* d) {
  const float u = (2.0f * ((float)i + 0.5f) / (float)c.width - 1.0f) * c.tan_half * c.aspect;
  const float v = (1.0f - 2.0f * ((float)j + 0.5f) / (float)c.height) * c.tan_half;
  float x = c.fwd[0] + u * c.right[0] + v * c.up[0], y = c.fwd[1] + u * c.right[1] + v * c.up[1], z = c.fwd[2] + u * c.right[2] + v * c.up[2];
  const float s = 1.0f / sqrtf(x * x + y * y + z * z);
  d[0] = x * s; d[1] = y * s; d[2] = z * s;
}

SGR_HD int sgr_type(const float* rec) { int m; memcpy(&m, rec + 15, 4); return m & 0xFF; }
SGR_HD int sgr_cat(const float* rec) { int m; memcpy(&m, rec + 15, 4); return (m >> 8) & 0xFF; }

// fp64 world pose -> record relative to the eye
SGR_HD void sgr_make_record(const double* xpos, const double* xmat, const double* size, int type, int cat, const double* eye, float* rec) {
  for (int k = 0; k < 3; k++) rec[k] = (float)(xpos[k] - eye[k]);
  for (int k = 0; k < 9; k++) rec[3 + k] = (float)xmat[k];
  for (int k = 0; k < 3; k++) rec[12 + k] = (float)size[k];
  const int m = type | (cat << 8);
  memcpy(rec + 15, &m, 4);
}

// bounding radius about the record's centre (planes: never culled)
SGR_HD float sgr_bound(const float* rec) {
  const float* s = rec + 12;
  switch (sgr_type(rec)) {
    case SGR_SPHERE: return s[0];
    case SGR_CAPSULE: return s[0] + s[1];
    case SGR_BOX: return sqrtf(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]);
    default: return INFINITY;
  }
}

// the cone (apex at the eye) around a tile's pixel-centre rays d0..d3 (its corner pixels): unit axis, cos / sin of the half angle
SGR_HD void sgr_tile_cone(const float* d0, const float* d1, const float* d2, const float* d3, float* axis, float* cs, float* sn) {
  float a[3] = {d0[0] + d1[0] + d2[0] + d3[0], d0[1] + d1[1] + d2[1] + d3[1], d0[2] + d1[2] + d2[2] + d3[2]};
  const float s = 1.0f / sqrtf(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
  for (int k = 0; k < 3; k++) axis[k] = a[k] * s;
  const float* ds[4] = {d0, d1, d2, d3};
  float c = 1.0f;
  for (int q = 0; q < 4; q++) c = fminf(c, axis[0] * ds[q][0] + axis[1] * ds[q][1] + axis[2] * ds[q][2]);
  c = fmaxf(-1.0f, c - 1e-5f);   // (margin for the rounding of the rays)
  *cs = c;
  *sn = sqrtf(fmaxf(0.0f, 1.0f - c * c));
}

// can the record's bounding sphere meet a ray of the cone?  (conservative: p cos - a sin <= R is the distance test for a point in
// front of the apex and a lower bound of the distance behind it)
SGR_HD bool sgr_cone_keep(const float* rec, const float* axis, float cs, float sn) {
  const float R = sgr_bound(rec);
  if (!(R < INFINITY)) return true;
  const float* p = rec;
  const float a = p[0] * axis[0] + p[1] * axis[1] + p[2] * axis[2];
  const float q0 = p[0] - a * axis[0], q1 = p[1] - a * axis[1], q2 = p[2] - a * axis[2];
  const float perp = sqrtf(q0 * q0 + q1 * q1 + q2 * q2);
  return perp * cs - a * sn <= R * 1.001f + 1e-5f;
}

// smallest root t > 0 of |o + t d - c|^2 = r^2 (d unit) through the closest-approach point (no cancellation of |o - c|^2 against r^2)
SGR_HD float sgr_sphere_t(const float* o, const float* d, float cz, float r) {
  const float oz = o[2] - cz;
  const float tl = -(o[0] * d[0] + o[1] * d[1] + oz * d[2]);
  const float q0 = o[0] + tl * d[0], q1 = o[1] + tl * d[1], q2 = oz + tl * d[2];
  const float h2 = r * r - (q0 * q0 + q1 * q1 + q2 * q2);
  if (h2 < 0.0f) return INFINITY;
  const float t = tl - sqrtf(h2);
  return t > 0.0f ? t : INFINITY;
}

// ray (origin = eye = 0, unit direction d, world axes) against one record: distance t (INFINITY: no hit), local hit point and normal
SGR_HD float sgr_intersect(const float* rec, const float* d, float* hit, float* nl) {
  const float* p = rec;
  const float* R = rec + 3;
  const float* s = rec + 12;
  // origin and direction in the geom's frame: o = R' (0 - p), dl = R' d
  float o[3], dl[3];
  for (int k = 0; k < 3; k++) {
    o[k] = -(R[k] * p[0] + R[3 + k] * p[1] + R[6 + k] * p[2]);
    dl[k] = R[k] * d[0] + R[3 + k] * d[1] + R[6 + k] * d[2];
  }
  float t = INFINITY;
  nl[0] = nl[1] = 0.0f; nl[2] = 1.0f;
  switch (sgr_type(rec)) {
    case SGR_PLANE: {
      if (dl[2] < 0.0f && o[2] > 0.0f) {
        const float tt = -o[2] / dl[2];
        const float x = o[0] + tt * dl[0], y = o[1] + tt * dl[1];
        const bool inside = (s[0] <= 0.0f || fabsf(x) <= s[0]) && (s[1] <= 0.0f || fabsf(y) <= s[1]);
        if (inside) t = tt;
      }
      break;
    }
    case SGR_SPHERE: t = sgr_sphere_t(o, dl, 0.0f, s[0]); break;
    case SGR_CAPSULE: {
      const float r = s[0], hl = s[1];
      const float a = dl[0] * dl[0] + dl[1] * dl[1];
      if (a > 1e-12f) {   // the side: infinite cylinder, entry root within |z| <= hl
        const float tl = -(o[0] * dl[0] + o[1] * dl[1]) / a;
        const float q0 = o[0] + tl * dl[0], q1 = o[1] + tl * dl[1];
        const float h2 = r * r - (q0 * q0 + q1 * q1);
        if (h2 >= 0.0f) {
          const float tt = tl - sqrtf(h2 / a);
          if (tt > 0.0f && fabsf(o[2] + tt * dl[2]) <= hl) t = tt;
        }
      }
      t = fminf(t, sgr_sphere_t(o, dl, hl, r));
      t = fminf(t, sgr_sphere_t(o, dl, -hl, r));
      break;
    }
    case SGR_BOX: {
      float tn = -INFINITY, tf = INFINITY;
      int ax = -1;
      bool miss = false;
      for (int k = 0; k < 3; k++) {
        if (dl[k] == 0.0f) {
          if (fabsf(o[k]) > s[k]) miss = true;
          continue;
        }
        const float inv = 1.0f / dl[k];
        float t1 = (-s[k] - o[k]) * inv, t2 = (s[k] - o[k]) * inv;
        if (t1 > t2) { const float x = t1; t1 = t2; t2 = x; }
        if (t1 > tn) { tn = t1; ax = k; }
        tf = fminf(tf, t2);
      }
      if (!miss && ax >= 0 && tn <= tf && tn > 0.0f) t = tn;
      if (t < INFINITY) {
        nl[2] = 0.0f;
        nl[ax] = dl[ax] > 0.0f ? -1.0f : 1.0f;
      }
      break;
    }
    default: break;
  }
  if (!(t < INFINITY)) return INFINITY;
  for (int k = 0; k < 3; k++) hit[k] = o[k] + t * dl[k];
  const int ty = sgr_type(rec);
  if (ty == SGR_SPHERE) {
    const float ir = 1.0f / s[0];
    for (int k = 0; k < 3; k++) nl[k] = hit[k] * ir;
  } else if (ty == SGR_CAPSULE) {
    const float zc = fminf(s[1], fmaxf(-s[1], hit[2]));
    const float ir = 1.0f / s[0];
    nl[0] = hit[0] * ir; nl[1] = hit[1] * ir; nl[2] = (hit[2] - zc) * ir;
  }
  return t;
}

// fixed shading: albedo x (0.25 + 0.45 max(0, n.(-forward)) + 0.30 max(0, n.z)); the ground is a checker of 0.5 m squares in the
// plane's own frame, (0.2, 0.3, 0.4) / (0.1, 0.15, 0.2); background (0.3, 0.5, 0.7) unshaded.  Channels rounded as floor(255 c + 0.5).
SGR_HD uint8_t sgr_u8(float c) {
  const float v = floorf(c * 255.0f + 0.5f);
  return (uint8_t)(v < 0.0f ? 0.0f : (v > 255.0f ? 255.0f : v));
}

SGR_HD void sgr_background(uint8_t* rgba) { rgba[0] = sgr_u8(0.3f); rgba[1] = sgr_u8(0.5f); rgba[2] = sgr_u8(0.7f); rgba[3] = 255; }

SGR_HD void sgr_shade(const float* rec, const float* hit, const float* nl, const SgrCam& c, uint8_t* rgba) {
  const float* R = rec + 3;
  float n[3];
  for (int k = 0; k < 3; k++) n[k] = R[3 * k] * nl[0] + R[3 * k + 1] * nl[1] + R[3 * k + 2] * nl[2];
  float alb[3];
  switch (sgr_cat(rec)) {
    case SGR_CAT_ELEM: case SGR_CAT_CENTER: alb[0] = 0.8f; alb[1] = 0.2f; alb[2] = 0.1f; break;
    case SGR_CAT_FINGER: alb[0] = 0.3f; alb[1] = 0.45f; alb[2] = 0.8f; break;
    case SGR_CAT_GROUND: {
      const float ps = floorf(hit[0] * 2.0f) + floorf(hit[1] * 2.0f);
      const bool odd = ps - 2.0f * floorf(0.5f * ps) != 0.0f;
      if (!odd) { alb[0] = 0.2f; alb[1] = 0.3f; alb[2] = 0.4f; }
      else { alb[0] = 0.1f; alb[1] = 0.15f; alb[2] = 0.2f; }
      break;
    }
    default: alb[0] = alb[1] = alb[2] = 0.6f; break;
  }
  const float f = 0.25f + 0.45f * fmaxf(0.0f, -(n[0] * c.fwd[0] + n[1] * c.fwd[1] + n[2] * c.fwd[2])) + 0.30f * fmaxf(0.0f, n[2]);
  rgba[0] = sgr_u8(alb[0] * f); rgba[1] = sgr_u8(alb[1] * f); rgba[2] = sgr_u8(alb[2] * f); rgba[3] = 255;
}

// one pixel against a list of records (ids: indices into recs, ascending): nearest entry hit
struct SgrHit {
  float depth;   // t * (d . forward); INFINITY = background
  int geom;      // -1 = background
  uint8_t rgba[4];
};

// the pixel of that hit: background, or the geom shaded
SGR_HD void sgr_geom_pixel(const float* recs, float best, int bg, const float* bh, const float* bn, const SgrCam& c, const float* d, SgrHit& r) {
  r.geom = bg;
  if (bg < 0) {
    r.depth = INFINITY;
    sgr_background(r.rgba);
  } else {
    r.depth = best * (d[0] * c.fwd[0] + d[1] * c.fwd[1] + d[2] * c.fwd[2]);
    sgr_shade(recs + SGR_REC * bg, bh, bn, c, r.rgba);
  }
}

template <typename IdxT>
SGR_HD SgrHit sgr_trace(const float* recs, const IdxT* ids, int nids, const SgrCam& c, const float* d) {
  float best = INFINITY, bh[3] = {0, 0, 0}, bn[3] = {0, 0, 1};
  int bg = -1;
  for (int q = 0; q < nids; q++) {
    const int g = (int)ids[q];
    float h[3], nl[3];
    const float t = sgr_intersect(recs + SGR_REC * g, d, h, nl);
    if (t < best) {
      best = t; bg = g;
      bh[0] = h[0]; bh[1] = h[1]; bh[2] = h[2]; bn[0] = nl[0]; bn[1] = nl[1]; bn[2] = nl[2];
    }
  }
  SgrHit r;
  sgr_geom_pixel(recs, best, bg, bh, bn, c, d, r);
  return r;
}

// ---- the skin: triangles bound to bodies (sg_render_ex with SG_RENDER_SKIN) ----
// Vertices are positions relative to the eye in fp32 (the eye is subtracted in fp64 first, as sgr_make_record does), one float4 each; a face
// is three vertex indices in one 32-bit word (nvert <= 256: a byte each), front side counter-clockwise.  Rules both casters share:
//   * the ray starts at 0, so the edge value of edge (p, q) is d . (p x q).  It is computed with the endpoint of SMALLER VERTEX INDEX
//     first and with an exact sign (sgr_edge): two triangles that share an edge get bit-identical magnitudes.  Per triangle
//     (a, b, c) it is oriented as E_ab = d . (b x a); the ray hits when all three are >= 0 -- zero counts as inside, so no ray slips
//     between two triangles that share an edge;
//   * front faces only: t = (n . a) / (n . d) with the face normal n = (b - a) x (c - a), and n . d < 0, t > 0;
//   * of equal t the smaller face index wins; against a geom at equal t the geom wins;
//   * shading: the fixed formula with the skin's rgb as albedo and the normal = the barycentric blend (weights E_bc, E_ca, E_ab) of the
//     vertex normals, normalised.  A vertex normal is the normalised sum of the unnormalised n of its faces (area weighting); where that
//     sum is zero the hit face's normal stands in for it, and so it does for a blend that comes out zero.
#define SGR_MAXVERT 256
#define SGR_MAXFACE 512
#define SGR_VREC 8        // floats per vertex record: position - eye (xyz, 0), normal (xyz, 0)

SGR_HD uint32_t sgr_pack_face(int a, int b, int c) { return (uint32_t)a | ((uint32_t)b << 8) | ((uint32_t)c << 16); }

// The edge value is taken in the ray's own frame: with u, w orthonormal and u x w = d, d . (p x q) = (p.u)(q.w) - (p.w)(q.u).  The two
// coordinates of a vertex are fp32 numbers that depend on the ray and the vertex alone (explicit fmaf in a fixed order: every triangle
// that uses the vertex gets the same bits); the two products of such numbers are exact in fp64 and their difference is rounded once,
// whether or not the compiler contracts it.  So the sign of every edge value is the exact sign for the projected points: two triangles
// that share an edge get bit-identical magnitudes, and the fan of triangles around a vertex leaves no gap for a ray aimed at it either
// (with d . (p x q) taken in fp32 from the 3-D coordinates, rounding noise of the size of the value itself decides the signs there).
struct SgrRayFrame { float u[3], w[3]; };

SGR_HD void sgr_ray_frame(const float* d, SgrRayFrame* fr) {
  const float ax = fabsf(d[0]), ay = fabsf(d[1]), az = fabsf(d[2]);
  float e[3] = {0.0f, 0.0f, 0.0f};
  e[ax <= ay && ax <= az ? 0 : (ay <= az ? 1 : 2)] = 1.0f;   // the axis d leans on least
  float u[3] = {d[1] * e[2] - d[2] * e[1], d[2] * e[0] - d[0] * e[2], d[0] * e[1] - d[1] * e[0]};
  const float il = 1.0f / sqrtf(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
  for (int k = 0; k < 3; k++) fr->u[k] = u[k] * il;
  fr->w[0] = d[1] * fr->u[2] - d[2] * fr->u[1]; fr->w[1] = d[2] * fr->u[0] - d[0] * fr->u[2]; fr->w[2] = d[0] * fr->u[1] - d[1] * fr->u[0];
}

SGR_HD float sgr_dot_fixed(const float* p, const float* a) { return fmaf(p[0], a[0], fmaf(p[1], a[1], p[2] * a[2])); }

// d . (p x q)
SGR_HD double sgr_edge(const SgrRayFrame& fr, const float* p, const float* q) {
  const double pu = sgr_dot_fixed(p, fr.u), pw = sgr_dot_fixed(p, fr.w), qu = sgr_dot_fixed(q, fr.u), qw = sgr_dot_fixed(q, fr.w);
  return pu * qw - pw * qu;
}

// oriented edge value E_pq = d . (q x p) of the triangle's edge p -> q (vertex indices ip, iq): the endpoint of smaller index first
SGR_HD double sgr_edge_oriented(const SgrRayFrame& fr, const float* p, int ip, const float* q, int iq) {
  return ip < iq ? -sgr_edge(fr, p, q) : sgr_edge(fr, q, p);
}

// unnormalised face normal (b - a) x (c - a)
SGR_HD void sgr_face_normal(const float* a, const float* b, const float* c, float* n) {
  const float u[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, v[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
  n[0] = u[1] * v[2] - u[2] * v[1]; n[1] = u[2] * v[0] - u[0] * v[2]; n[2] = u[0] * v[1] - u[1] * v[0];
}

// ray (origin 0, unit d) against the triangle: distance (INFINITY: no hit) and the weights w = (E_bc, E_ca, E_ab) of a, b, c
SGR_HD float sgr_tri(const float* d, const SgrRayFrame& fr, const float* a, int ia, const float* b, int ib, const float* c, int ic, float* w) {
  const double eab = sgr_edge_oriented(fr, a, ia, b, ib);
  const double ebc = sgr_edge_oriented(fr, b, ib, c, ic);
  const double eca = sgr_edge_oriented(fr, c, ic, a, ia);
  if (!(eab >= 0.0 && ebc >= 0.0 && eca >= 0.0)) return INFINITY;
  float n[3];
  sgr_face_normal(a, b, c, n);
  const float den = n[0] * d[0] + n[1] * d[1] + n[2] * d[2];
  if (!(den < 0.0f)) return INFINITY;
  const float t = (n[0] * a[0] + n[1] * a[1] + n[2] * a[2]) / den;
  if (!(t > 0.0f && t < INFINITY)) return INFINITY;
  w[0] = (float)ebc; w[1] = (float)eca; w[2] = (float)eab;
  return t;
}

// bounding sphere of a triangle about its centroid against the tile cone (the test of sgr_cone_keep)
SGR_HD bool sgr_tri_cone_keep(const float* a, const float* b, const float* c, const float* axis, float cs, float sn) {
  const float third = 1.0f / 3.0f;
  const float p[3] = {(a[0] + b[0] + c[0]) * third, (a[1] + b[1] + c[1]) * third, (a[2] + b[2] + c[2]) * third};
  float r2 = 0.0f;
  const float* vs[3] = {a, b, c};
  for (int q = 0; q < 3; q++) {
    const float x = vs[q][0] - p[0], y = vs[q][1] - p[1], z = vs[q][2] - p[2];
    r2 = fmaxf(r2, x * x + y * y + z * z);
  }
  const float R = sqrtf(r2);
  const float al = p[0] * axis[0] + p[1] * axis[1] + p[2] * axis[2];
  const float q0 = p[0] - al * axis[0], q1 = p[1] - al * axis[1], q2 = p[2] - al * axis[2];
  const float perp = sqrtf(q0 * q0 + q1 * q1 + q2 * q2);
  return perp * cs - al * sn <= R * 1.001f + 1e-5f;
}

// normal of vertex v: normalised sum of the face normals of its faces adj[adj_start[v] .. adj_start[v + 1]) (ascending face index);
// (0, 0, 0) when the sum has no length.  vpos: float4 per vertex
SGR_HD void sgr_vertex_normal(int v, const float* vpos, const uint32_t* faces, const int* adj_start, const int* adj, float* n) {
  float s[3] = {0.0f, 0.0f, 0.0f};
  for (int q = adj_start[v]; q < adj_start[v + 1]; q++) {
    const uint32_t f = faces[adj[q]];
    float fn[3];
    sgr_face_normal(vpos + 4 * (f & 0xFF), vpos + 4 * ((f >> 8) & 0xFF), vpos + 4 * ((f >> 16) & 0xFF), fn);
    s[0] += fn[0]; s[1] += fn[1]; s[2] += fn[2];
  }
  const float l2 = s[0] * s[0] + s[1] * s[1] + s[2] * s[2];
  const float il = l2 > 0.0f ? 1.0f / sqrtf(l2) : 0.0f;
  n[0] = s[0] * il; n[1] = s[1] * il; n[2] = s[2] * il;
}

// one pixel against the listed geoms (ids ascending, the hidden ones left out) and then the listed faces (ascending).  vpos: float4 per
// vertex (position - eye); vrec: the env's vertex records (SGR_VREC floats each; only the hit's normals are read); skin_id: what a skin
// pixel reports as its geom (ngeom).  *face: the hit face (-1: none)
template <typename IdxT, typename FIdxT>
SGR_HD SgrHit sgr_trace_skin(const float* recs, const IdxT* ids, int nids, const float* vpos, const uint32_t* faces, const FIdxT* flist, int nf,
                             const float* vrec, const float* albedo, int skin_id, const SgrCam& c, const float* d, int* face) {
  float best = INFINITY, bh[3] = {0, 0, 0}, bn[3] = {0, 0, 1};
  int bg = -1;
  for (int q = 0; q < nids; q++) {
    const int g = (int)ids[q];
    float h[3], nl[3];
    const float t = sgr_intersect(recs + SGR_REC * g, d, h, nl);
    if (t < best) {
      best = t; bg = g;
      bh[0] = h[0]; bh[1] = h[1]; bh[2] = h[2]; bn[0] = nl[0]; bn[1] = nl[1]; bn[2] = nl[2];
    }
  }
  int bf = -1;
  float bw[3] = {0, 0, 0};
  SgrRayFrame fr;
  sgr_ray_frame(d, &fr);
  for (int q = 0; q < nf; q++) {
    const int f = (int)flist[q];
    const uint32_t w = faces[f];
    const int ia = w & 0xFF, ib = (w >> 8) & 0xFF, ic = (w >> 16) & 0xFF;
    float wt[3];
    const float t = sgr_tri(d, fr, vpos + 4 * ia, ia, vpos + 4 * ib, ib, vpos + 4 * ic, ic, wt);
    if (t < best) { best = t; bf = f; bw[0] = wt[0]; bw[1] = wt[1]; bw[2] = wt[2]; }
  }
  *face = bf;
  SgrHit r;
  if (bf >= 0) {
    const uint32_t w = faces[bf];
    const int iv[3] = {(int)(w & 0xFF), (int)((w >> 8) & 0xFF), (int)((w >> 16) & 0xFF)};
    float fn[3];
    sgr_face_normal(vpos + 4 * iv[0], vpos + 4 * iv[1], vpos + 4 * iv[2], fn);
    const float fl = 1.0f / sqrtf(fn[0] * fn[0] + fn[1] * fn[1] + fn[2] * fn[2]);
    fn[0] *= fl; fn[1] *= fl; fn[2] *= fl;
    float n[3] = {0.0f, 0.0f, 0.0f};
    for (int k = 0; k < 3; k++) {
      const float* vn = vrec + SGR_VREC * iv[k] + 4;
      const bool zero = vn[0] == 0.0f && vn[1] == 0.0f && vn[2] == 0.0f;
      for (int x = 0; x < 3; x++) n[x] += bw[k] * (zero ? fn[x] : vn[x]);
    }
    const float l2 = n[0] * n[0] + n[1] * n[1] + n[2] * n[2];
    if (l2 > 0.0f) {
      const float il = 1.0f / sqrtf(l2);
      n[0] *= il; n[1] *= il; n[2] *= il;
    } else {
      n[0] = fn[0]; n[1] = fn[1]; n[2] = fn[2];
    }
    const float f = 0.25f + 0.45f * fmaxf(0.0f, -(n[0] * c.fwd[0] + n[1] * c.fwd[1] + n[2] * c.fwd[2])) + 0.30f * fmaxf(0.0f, n[2]);
    r.geom = skin_id;
    r.depth = best * (d[0] * c.fwd[0] + d[1] * c.fwd[1] + d[2] * c.fwd[2]);
    r.rgba[0] = sgr_u8(albedo[0] * f); r.rgba[1] = sgr_u8(albedo[1] * f); r.rgba[2] = sgr_u8(albedo[2] * f); r.rgba[3] = 255;
    return r;
  }
  sgr_geom_pixel(recs, best, bg, bh, bn, c, d, r);
  return r;
}
