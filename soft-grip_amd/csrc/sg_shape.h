// sg_shape.h -- the per-env arithmetic of the soft object's read-outs (sg_get_skin_vertices, sg_get_shape, sg_get_subtree): the shape
// table beside the kinematics and dynamics tables, and what one lane does for one skin vertex, one face, one direction's candidate and
// one body's subtree.  Pure functions of their arguments, compiled for gfx950 (sg_shape_kernel.h, inside sg_readout.hip) and by g++ for
// the CPU tests (tests/shape_ref.py, scripts/sanitize/shape_main.cpp), which drive the same text through sgh_host_env below.
//
// Definitions.  A vertex bound to body b at vert_pos (body frame) sits at xpos_b + R(xquat_b) vert_pos and moves as a material point of
// that body: lin_b + ang_b x (pos - xpos_b), sg_dyn.h's record.  The integrals of the closed skin are taken about p0, vertex 0's
// position, so that their summands stay of the object's own size wherever it is: for face (i, j, k) with a, b, c its vertices minus p0,
// det = a . (b x c), s = a + b + c,
//   V = sum det / 6,  A = sum |(b - a) x (c - a)| / 2,  first moment sum det s / 24,  second moment sum det (aa' + bb' + cc' + ss') / 120,
//   dV/dt = sum (va . (b x c) + a . (vb x c) + a . (b x vc)) / 6 with the velocities relative to vertex 0's.
// Centroid = p0 + F / V and the central second moments S - F (F / V)' follow by one division and one subtraction, unclamped (V == 0: NaN).
// A subtree's row: com = sum m xipos / M, linvel = sum m com_lin / M, angmom = sum (R I R' w + m (xipos - com) x com_lin) over the body
// and its descendants in ascending body order; M == 0: the body's own xipos and com velocity, and a zero angmom.
#pragma once
#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif
#include "sg_dyn.h"
#include "sg_skin.h"

#define SGH_SHAPE_N 12    // doubles per env of `shape`: V, A, centroid 3, central second moments xx yy zz xy xz yz, dV/dt (SG_SHAPE_N)
#define SGH_NSUM 12       // a face's shares: det, area, det s (3), det (aa' + bb' + cc' + ss') (6), the rate's numerator
#define SGH_VREC 6        // doubles per vertex in LDS: position, velocity
#define SGH_SHARE 9       // doubles per body in LDS: xipos, com velocity, R I R' w
#define SGH_MAXDIR 256    // directions per sg_get_shape call
// the kernel's LDS block: nbody x (SGD_REC + SGH_SHARE) + nvert x SGH_VREC doubles beside its static LDS (the block-wide
// __syncthreads_or), within the 160 KB of a CU
#define SGH_STATIC_LDS 256
#define SGH_LDS_MAX (160 * 1024)

// ---- the shape table: one double and one int array, sections at the offsets below ----
struct SgShapeOff {
  int nvert, nface, closed, root, nlist;   // closed: 1 / 0, -1 without a skin; root: the object's body, -1 without a skin
  // doubles
  int vpos, smass;           // [nvert][3] vert_pos; [nbody] subtree masses
  // ints
  int vbody, face, sstart, slist;   // [nvert]; [nface][3]; [nbody + 1]; [nlist] every body's subtree, ascending
};

struct SgShapeHost {
  bool ok = false;
  std::string err;
  SgShapeOff o;
  std::vector<double> dbl;
  std::vector<int> ints;
};

inline long long sgh_lds_bytes(int nbody, int nvert) { return 8ll * ((long long)(SGD_REC + SGH_SHARE) * nbody + (long long)SGH_VREC * nvert); }

// the table from the kinematics and dynamics tables and the model's skin (which may be empty: the subtree call needs none); T->ok says
// whether the three read-outs can run the model (sg_tables.cpp)
void sgh_build(const SgKinHost& K, const SgDynHost& Dn, const SgSkinHost& S, SgShapeHost* T);
// the skin's vertices at qpos0 in frame_body's frame (-1: world) -> rest[nvert][3]
void sgh_rest(const SgKinHost& K, const SgSkinHost& S, int frame_body, double* rest);

// ---- one vertex ----
// vertex on the body of record rec at vp (body frame) -> pv[6]: world position, velocity of the material point
__host__ __device__ inline void sgh_vertex(const double* rec, const double* vp, double* pv) { sgd_point(rec, vp, pv, pv + 3); }
// the world point p in the frame of the body of record frec: R' (p - xpos)
__host__ __device__ inline void sgh_local(const double* frec, const double* p, double* out) {
  double R[9];
  sgk_quat_mat(R, frec + 3);
  const double d[3] = {p[0] - frec[0], p[1] - frec[1], p[2] - frec[2]};
  for (int k = 0; k < 3; k++) out[k] = R[k] * d[0] + R[3 + k] * d[1] + R[6 + k] * d[2];
}

// ---- one face's shares ----
// V: the vertices' records [nvert][SGH_VREC]; (i, j, k) the face -> sh[SGH_NSUM], unscaled (sgh_finish divides)
__host__ __device__ inline void sgh_face(const double* V, int i, int j, int k, double* sh) {
  const double *p0 = V, *pi = V + SGH_VREC * i, *pj = V + SGH_VREC * j, *pk = V + SGH_VREC * k;
  double a[3], b[3], c[3], va[3], vb[3], vc[3], s[3], bc[3], t[3], e1[3], e2[3], n[3];
  for (int x = 0; x < 3; x++) {
    a[x] = pi[x] - p0[x]; b[x] = pj[x] - p0[x]; c[x] = pk[x] - p0[x];
    va[x] = pi[3 + x] - p0[3 + x]; vb[x] = pj[3 + x] - p0[3 + x]; vc[x] = pk[3 + x] - p0[3 + x];
    s[x] = a[x] + b[x] + c[x];
    e1[x] = b[x] - a[x]; e2[x] = c[x] - a[x];
  }
  sgd_cross(bc, b, c);
  const double det = a[0] * bc[0] + a[1] * bc[1] + a[2] * bc[2];
  sgd_cross(n, e1, e2);
  sh[0] = det;
  sh[1] = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
  for (int x = 0; x < 3; x++) sh[2 + x] = det * s[x];
  const int ix[6] = {0, 1, 2, 0, 0, 1}, iy[6] = {0, 1, 2, 1, 2, 2};   // xx yy zz xy xz yz
  for (int q = 0; q < 6; q++) {
    const int x = ix[q], y = iy[q];
    sh[5 + q] = det * (a[x] * a[y] + b[x] * b[y] + c[x] * c[y] + s[x] * s[y]);
  }
  double rate = va[0] * bc[0] + va[1] * bc[1] + va[2] * bc[2];
  sgd_cross(t, vb, c);
  rate += a[0] * t[0] + a[1] * t[1] + a[2] * t[2];
  sgd_cross(t, b, vc);
  rate += a[0] * t[0] + a[1] * t[1] + a[2] * t[2];
  sh[11] = rate;
}
// the summed shares and p0 -> shape[SGH_SHAPE_N]
__host__ __device__ inline void sgh_finish(const double* sum, const double* p0, double* shape) {
  const double V = sum[0] / 6.0;
  const double F[3] = {sum[2] / 24.0, sum[3] / 24.0, sum[4] / 24.0};
  double cm[3];
  for (int x = 0; x < 3; x++) cm[x] = V == 0.0 ? NAN : F[x] / V;
  shape[0] = V;
  shape[1] = sum[1] / 2.0;
  for (int x = 0; x < 3; x++) shape[2 + x] = p0[x] + cm[x];
  const int ix[6] = {0, 1, 2, 0, 0, 1}, iy[6] = {0, 1, 2, 1, 2, 2};
  for (int q = 0; q < 6; q++) shape[5 + q] = sum[5 + q] / 120.0 - F[ix[q]] * cm[iy[q]];
  shape[11] = sum[11] / 6.0;
}

// ---- one direction ----
// direction dir[3] given in body's frame (-1: world) -> the unit direction in world axes and the origin o its heights are taken from
__host__ __device__ inline void sgh_direction(const double* recs, const double* dir, int body, double* dhat, double* o) {
  const double n = sqrt(dir[0] * dir[0] + dir[1] * dir[1] + dir[2] * dir[2]);
  const double u[3] = {dir[0] / n, dir[1] / n, dir[2] / n};
  if (body < 0) {
    for (int k = 0; k < 3; k++) { dhat[k] = u[k]; o[k] = 0.0; }
    return;
  }
  const double* rec = recs + SGD_REC * body;
  double R[9];
  sgk_quat_mat(R, rec + 3);
  sgk_mv(dhat, R, u);
  for (int k = 0; k < 3; k++) o[k] = rec[k];
}
// a vertex's height along the direction
__host__ __device__ inline double sgh_height(const double* dhat, const double* o, const double* p) {
  return dhat[0] * (p[0] - o[0]) + dhat[1] * (p[1] - o[1]) + dhat[2] * (p[2] - o[2]);
}
// candidate (v, i) against the best so far (bv, bi; bi < 0: none yet): the lower (upper) height wins, the smaller index on a tie
__host__ __device__ inline bool sgh_lower(double v, int i, double bv, int bi) { return i >= 0 && (bi < 0 || v < bv || (v == bv && i < bi)); }
__host__ __device__ inline bool sgh_upper(double v, int i, double bv, int bi) { return i >= 0 && (bi < 0 || v > bv || (v == bv && i < bi)); }

// ---- one body's subtree ----
// body i's shares -> sh[SGH_SHARE]: xipos, the centre of mass's velocity, the spin R I R' w about it (world axes)
__host__ __device__ inline void sgh_body_share(const double* DD, const SgDynOff& d, const double* rec, int i, double* sh) {
  double R[9], wl[3], Iw[3];
  sgd_com(DD, d, rec, i, sh, sh + 3);
  sgk_quat_mat(R, rec + 3);
  const double* w = rec + 7;
  for (int k = 0; k < 3; k++) wl[k] = R[k] * w[0] + R[3 + k] * w[1] + R[6 + k] * w[2];
  sgk_mv(Iw, DD + d.bimat + 9 * i, wl);
  sgk_mv(sh + 6, R, Iw);
}
// body i's row from the shares of every body: list[n] its subtree (ascending, itself first), M its subtree mass
__host__ __device__ inline void sgh_subtree(const double* DD, const SgDynOff& d, const double* shares, const int* list, int n, double M, int i, double* com,
                                            double* linvel, double* angmom) {
  const double* own = shares + SGH_SHARE * i;
  if (M == 0.0) {
    for (int k = 0; k < 3; k++) { com[k] = own[k]; linvel[k] = own[3 + k]; angmom[k] = 0.0; }
    return;
  }
  double sx[3] = {0, 0, 0}, sv[3] = {0, 0, 0}, L[3] = {0, 0, 0};
  for (int e = 0; e < n; e++) {
    const double* sh = shares + SGH_SHARE * list[e];
    const double m = DD[d.bmass + list[e]];
    for (int k = 0; k < 3; k++) { sx[k] += m * sh[k]; sv[k] += m * sh[3 + k]; }
  }
  for (int k = 0; k < 3; k++) { com[k] = sx[k] / M; linvel[k] = sv[k] / M; }
  for (int e = 0; e < n; e++) {
    const double* sh = shares + SGH_SHARE * list[e];
    const double m = DD[d.bmass + list[e]];
    const double r[3] = {sh[0] - com[0], sh[1] - com[1], sh[2] - com[2]};
    double c[3];
    sgd_cross(c, r, sh + 3);
    for (int k = 0; k < 3; k++) L[k] += sh[6 + k] + m * c[k];
  }
  for (int k = 0; k < 3; k++) angmom[k] = L[k];
}

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- one env on the host, in the kernel's order (the CPU tests and the sanitizer program) ----
// the kernel's wavefront sum: lane l adds its 64-strided shares in ascending order, then wave_sum2's xor butterfly
inline double sgh_host_wave_sum(double* lane) {
  for (int o = 32; o > 0; o >>= 1) {
    double next[64];
    for (int l = 0; l < 64; l++) next[l] = lane[l] + lane[l ^ o];
    for (int l = 0; l < 64; l++) lane[l] = next[l];
  }
  return lane[0];
}
// every output of the three calls for one state; any output may be NULL.  dir [n_dirs][3], dir_body [n_dirs] or NULL.
// Returns 1 (and writes nothing) for a state that is not finite
inline int sgh_host_env(const SgKinHost& K, const SgDynHost& Dn, const SgShapeHost& T, const double* qpos, const double* qvel, int frame_body, int n_dirs,
                        const double* dir, const int* dir_body, double* pos, double* vel, double* local, double* shape, double* lo, double* hi, int* lo_vert,
                        int* hi_vert, double* com, double* linvel, double* angmom) {
  const SgKinOff& o = K.o;
  const SgDynOff& d = Dn.o;
  const SgShapeOff& h = T.o;
  for (int i = 0; i < o.nq; i++)
    if (!std::isfinite(qpos[i])) return 1;
  for (int i = 0; i < d.nv; i++)
    if (!std::isfinite(qvel[i])) return 1;
  const double *DD = Dn.dbl.data(), *HD = T.dbl.data();
  const int* HI = T.ints.data();
  std::vector<double> rec, V((size_t)SGH_VREC * (h.nvert ? h.nvert : 1), 0.0), sh((size_t)SGH_SHARE * o.nbody, 0.0);
  sgd_host_walk(K, Dn, qpos, qvel, &rec);
  for (int v = 0; v < h.nvert; v++) {
    sgh_vertex(&rec[SGD_REC * HI[h.vbody + v]], HD + h.vpos + 3 * v, &V[SGH_VREC * v]);
    for (int c = 0; c < 3; c++) {
      if (pos) pos[3 * v + c] = V[SGH_VREC * v + c];
      if (vel) vel[3 * v + c] = V[SGH_VREC * v + 3 + c];
    }
    if (local) {
      if (frame_body < 0)
        for (int c = 0; c < 3; c++) local[3 * v + c] = V[SGH_VREC * v + c];
      else
        sgh_local(&rec[SGD_REC * frame_body], &V[SGH_VREC * v], local + 3 * v);
    }
  }
  if (shape) {
    double lane[SGH_NSUM][64] = {}, sum[SGH_NSUM];
    for (int f = 0; f < h.nface; f++) {
      double s1[SGH_NSUM];
      sgh_face(V.data(), HI[h.face + 3 * f], HI[h.face + 3 * f + 1], HI[h.face + 3 * f + 2], s1);
      for (int q = 0; q < SGH_NSUM; q++) lane[q][f % 64] += s1[q];
    }
    for (int q = 0; q < SGH_NSUM; q++) sum[q] = sgh_host_wave_sum(lane[q]);
    sgh_finish(sum, V.data(), shape);
  }
  for (int j = 0; j < n_dirs; j++) {
    double dhat[3], og[3], bl = 0, bh = 0;
    int il = -1, ih = -1;
    sgh_direction(rec.data(), dir + 3 * j, dir_body ? dir_body[j] : -1, dhat, og);
    for (int v = 0; v < h.nvert; v++) {
      const double x = sgh_height(dhat, og, &V[SGH_VREC * v]);
      if (sgh_lower(x, v, bl, il)) { bl = x; il = v; }
      if (sgh_upper(x, v, bh, ih)) { bh = x; ih = v; }
    }
    if (lo) lo[j] = bl;
    if (hi) hi[j] = bh;
    if (lo_vert) lo_vert[j] = il;
    if (hi_vert) hi_vert[j] = ih;
  }
  if (com || linvel || angmom) {
    for (int i = 0; i < o.nbody; i++) sgh_body_share(DD, d, &rec[SGD_REC * i], i, &sh[SGH_SHARE * i]);
    for (int i = 0; i < o.nbody; i++) {
      double c3[3], l3[3], a3[3];
      const int s0 = HI[h.sstart + i];
      sgh_subtree(DD, d, sh.data(), HI + h.slist + s0, HI[h.sstart + i + 1] - s0, HD[h.smass + i], i, c3, l3, a3);
      for (int c = 0; c < 3; c++) {
        if (com) com[3 * i + c] = c3[c];
        if (linvel) linvel[3 * i + c] = l3[c];
        if (angmom) angmom[3 * i + c] = a3[c];
      }
    }
  }
  return 0;
}
#endif
