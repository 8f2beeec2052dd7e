// sg_readout.h -- what the read-outs (sg_get_poses, sg_render, sg_get_contacts, sg_ray) keep per model and per batch: the kinematics table
// with mj_kinematics' per-body / per-geom routines, the contact read-out's pair table and the skin's device tables.  The builders are
// defined in sg_tables.cpp (host C++, no HIP); sg_tables_build (sg_tables.h) calls them for sg_model_create (sg_api.hip) and for the host
// twins alike, sg_model and sg_batch (sg_batch.h) hold the results.
#pragma once
#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif
#include <cmath>
#include <string>
#include <vector>

#include "sg_contacts.h"   // SGC_MAXCON; the joint and geom type codes of softgrip_model.h
#include "sg_plan.h"
#include "sg_render.h"     // the geom categories and types in gmeta (SGR_CAT_*, SGR_PLANE ..), uint32_t

// ---- the kinematics table: one double and one int array, sections at the offsets below ----
struct SgKinOff {
  int nbody, ngeom, njnt, nq, nlevel;
  // doubles
  int bpos, bquat, jpos, jaxis, jq0, gpos, gmat, gsize;
  // ints
  int bpar, bjadr, bjnum, jtype, jqadr, gbody, gmeta, lstart, lbody;
};

struct SgKinHost {
  bool ok = false;
  std::string err;
  int bad_type = -1;           // first geom type the renderer has no intersection for (-1: none)
  SgKinOff o;
  std::vector<double> dbl;
  std::vector<int> ints;
  std::vector<double> qpos0, rbound;
};

// the one writer of every read-out table (this one, sg_dyn.h, sg_smooth.h, sg_point.h, sg_solve.h): appends a section to a table's array
// and returns the offset it starts at
template <class T>
inline int sg_put(std::vector<T>& to, const T* p, size_t n) {
  const int at = (int)to.size();
  to.insert(to.end(), p, p + n);
  return at;
}
template <class T>
inline int sg_put(std::vector<T>& to, const std::vector<T>& section) { return sg_put(to, section.data(), section.size()); }

// mj_kinematics for one body, as mjcf.Model.kinematics() does it (parent pose in px / pq, parent quaternion normalised)
__host__ __device__ inline void sgk_quat_mul(double* r, const double* a, const double* b) {
  const double w = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
  const double x = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
  const double y = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
  const double z = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
  r[0] = w; r[1] = x; r[2] = y; r[3] = z;
}
__host__ __device__ inline void sgk_quat_mat(double* M, const double* q) {
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  M[0] = w * w + x * x - y * y - z * z; M[1] = 2 * (x * y - w * z); M[2] = 2 * (x * z + w * y);
  M[3] = 2 * (x * y + w * z); M[4] = w * w - x * x + y * y - z * z; M[5] = 2 * (y * z - w * x);
  M[6] = 2 * (x * z - w * y); M[7] = 2 * (y * z + w * x); M[8] = w * w - x * x - y * y + z * z;
}
__host__ __device__ inline void sgk_quat_normalize(double* q) {
  const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  if (n < 1e-15) { q[0] = 1; q[1] = q[2] = q[3] = 0; return; }
  for (int k = 0; k < 4; k++) q[k] /= n;
}
__host__ __device__ inline void sgk_mv(double* r, const double* M, const double* v) {
  const double x = M[0] * v[0] + M[1] * v[1] + M[2] * v[2], y = M[3] * v[0] + M[4] * v[1] + M[5] * v[2], z = M[6] * v[0] + M[7] * v[1] + M[8] * v[2];
  r[0] = x; r[1] = y; r[2] = z;
}

// body i from its parent's pose (pp, pq) -> out[7] = xpos, xquat
__host__ __device__ inline void sgk_body(const double* D, const int* I, const SgKinOff& o, const double* qpos, int i, const double* pp, const double* pq,
                                         double* out) {
  double R[9], t[3], pos[3], quat[4];
  sgk_quat_mat(R, pq);
  sgk_mv(t, R, D + o.bpos + 3 * i);
  for (int k = 0; k < 3; k++) pos[k] = pp[k] + t[k];
  sgk_quat_mul(quat, pq, D + o.bquat + 4 * i);
  const int j0 = I[o.bjadr + i], nj = I[o.bjnum + i];
  for (int j = j0; j < j0 + nj; j++) {
    const int type = I[o.jtype + j], qa = I[o.jqadr + j];
    if (type == SG_JNT_FREE) {
      for (int k = 0; k < 3; k++) pos[k] = qpos[qa + k];
      for (int k = 0; k < 4; k++) quat[k] = qpos[qa + 3 + k];
      sgk_quat_normalize(quat);
      continue;
    }
    const double* jp = D + o.jpos + 3 * j;
    const double* ja = D + o.jaxis + 3 * j;
    double anchor[3], axis[3];
    sgk_quat_mat(R, quat);
    sgk_mv(t, R, jp);
    for (int k = 0; k < 3; k++) anchor[k] = pos[k] + t[k];
    sgk_mv(axis, R, ja);
    const double dq = qpos[qa] - D[o.jq0 + j];
    if (type == SG_JNT_SLIDE) {
      for (int k = 0; k < 3; k++) pos[k] = pos[k] + axis[k] * dq;
    } else {
      const double s = sin(dq / 2);
      const double ql[4] = {cos(dq / 2), ja[0] * s, ja[1] * s, ja[2] * s};
      double qn[4];
      sgk_quat_mul(qn, quat, ql);
      for (int k = 0; k < 4; k++) quat[k] = qn[k];
      sgk_quat_mat(R, quat);
      sgk_mv(t, R, jp);
      for (int k = 0; k < 3; k++) pos[k] = anchor[k] - t[k];
    }
  }
  sgk_quat_normalize(quat);
  for (int k = 0; k < 3; k++) out[k] = pos[k];
  for (int k = 0; k < 4; k++) out[3 + k] = quat[k];
}

// geom g from its body's pose: world position and orientation (row-major)
__host__ __device__ inline void sgk_geom(const double* D, const int* I, const SgKinOff& o, const double* body7, int g, double* gx, double* gm) {
  double R[9], t[3];
  sgk_quat_mat(R, body7 + 3);
  sgk_mv(t, R, D + o.gpos + 3 * g);
  for (int k = 0; k < 3; k++) gx[k] = body7[k] + t[k];
  const double* L = D + o.gmat + 9 * g;
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) gm[3 * r + c] = R[3 * r] * L[c] + R[3 * r + 1] * L[3 + c] + R[3 * r + 2] * L[6 + c];
}

// the table from the blob and the plan (geom categories, finger geoms); K->ok says whether the read-outs can run the model
void sgk_build(const void* blob, size_t nbytes, const SgPlan& plan, const SgTreeDev* tree, bool fast, SgKinHost* K);
// mj_kinematics on the host at qpos0: body poses [nbody][7]
void sgk_host_fk(const SgKinHost& K, std::vector<double>* body);
// the default free camera (sg_model_default_camera): cam[7] = lookat xyz, distance, azimuth, elevation, fovy
void sgk_default_camera(const SgKinHost& K, double* cam);

// ---- the contact read-out's tables ----
struct SgConHost {
  bool ok = false;
  std::string err;
  int cap = SGC_MAXCON;
  std::vector<int> pairs;     // [npair][2]
  std::vector<double> gaux;   // [ngeom][2]: geom_margin, geom_rbound
};

// the pair table and the per-geom margins / bounding radii from the blob
void sgc_from_blob(const void* blob, size_t nbytes, const SgKinHost& K, SgConHost* C);

// ---- the skin's tables on a batch's device (sg_skin.h builds them on the host) ----
struct SgSkinDev {
  const int* vert_body;      // [nvert]
  const double* vert_pos;    // [nvert][3]
  const uint32_t* faces;     // [nface] sgr_pack_face
  const int* adj_start;      // [nvert + 1]
  const int* adj;            // [3 nface]
  const int* hidden;         // [ngeom] 1: a geom the skin replaces
  int nvert, nface;
  float rgb[3];
};
