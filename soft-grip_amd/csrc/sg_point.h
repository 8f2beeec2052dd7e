// sg_point.h -- the per-env, per-point arithmetic of the point read-outs (sg_get_point_motion, sg_get_jacobians): pose, velocity and
// acceleration of a point fixed on a body, what a gyro and an accelerometer there would read, and the point's Jacobians.  Pure
// functions of their arguments, compiled for gfx950 (sg_point_kernel.h, inside sg_readout.hip) and by g++ for the CPU tests
// (tests/point_ref.py), which drive the same text point by point through sgp_host_env (sg_readout_host.h).
//
// The forward walk is sg_smooth.h's: sgs_world / sgs_body leave in every body's record its pose (0 .. 6), its twist (7 .. 12: angular
// velocity, linear velocity of the frame's origin xpos) and its acceleration (13 .. 18: angular, and that of xpos WITH THE WORLD
// ACCELERATING AT -gravity, which is what an accelerometer measures), and per dof its twist (u, the linear velocity at the world origin).
// Only those 19 slots of a record are read or written here, so the records are kept at 19 doubles (SGP_REC), not sg_smooth.h's 29.
// A dof's record is 7 doubles: the twist and a stamp -- the number of the last point whose body the dof moves (sgp_mark).
#pragma once
#include "sg_smooth.h"

#define SGP_REC 19
#define SGP_DOF 7
#define SGP_STAMP 6   // a dof record's stamp slot
// The kernel's LDS block: nbody records, nv dof records and nv ints (the dof-parent chain) beside its static LDS (SGP_STATIC_LDS bytes:
// the block-wide __syncthreads_or; the kept assembly's figure, held by tests/test_point_host.py).  Of the 160 KB a gfx950 workgroup can
// have, 1024 dofs leave room for 672 bodies.
#define SGP_STATIC_LDS 256
#define SGP_LDS_MAX 163840
#define SGP_MAXDOF 1024
#define SGP_MAXBODY ((SGP_LDS_MAX - SGP_STATIC_LDS - (8 * SGP_DOF + 4) * SGP_MAXDOF) / (SGP_REC * 8))
static_assert(SGP_REC == SGS_ACC + 6, "a point record ends with sgs_body's acceleration slots");
static_assert(SGP_DOF == SGS_DOF && SGP_STAMP == 6, "sgs_body lays the dof records out at SGS_DOF and writes their slots 0 .. 5 only");

// ---- the point table: one int array, sections at the offsets below ----
struct SgPointOff {
  int bdof;   // [nbody] where a body enters the dof-parent chain: the last dof of the nearest ancestor-or-self that has dofs, else -1
  int dpar;   // [nv] a dof's parent dof: the dof before it on the same body, else bdof of the body's parent
};

struct SgPointHost {
  bool ok = false;
  std::string err;
  SgPointOff o;
  std::vector<int> ints;
  // the model's sites (sg_model_sites): host side only
  std::vector<int> site_body;
  std::vector<double> site_pos, site_quat;
};

// the table from the blob (K, Dn: the model's kinematics and dynamics tables, whose bodies, joints and dofs it indexes).  P->ok says
// whether the point read-outs can run the model
void sgp_build(const void* blob, size_t nbytes, const SgKinHost& K, const SgDynHost& Dn, SgPointHost* P);

// the world's record (sgs_world's, cut to SGP_REC)
__host__ __device__ inline void sgp_world(const double* DD, const SgDynOff& d, double* rec) {
  double w[SGS_REC];
  sgs_world(DD, d, w);
  for (int k = 0; k < SGP_REC; k++) rec[k] = w[k];
}

// the world position of the point at `local` in the frame of the body with record rec
__host__ __device__ inline void sgp_pos(const double* rec, const double* local, double* P) {
  double R[9], t[3];
  sgk_quat_mat(R, rec + 3);
  sgk_mv(t, R, local);
  for (int k = 0; k < 3; k++) P[k] = rec[k] + t[k];
}

// everything sg_get_point_motion reports of one point: local[3] its place and quat[4] its frame (NULL: the body's; normalised here) in
// the frame of the body with record rec.  pos[3]; mat[9] = R(xquat) R(quat), row-major; vel[6] = (w, v + w x r), r = pos - xpos;
// acc[6] = (al, a + al x r + w x (w x r) + gravity): the record's acceleration has the world falling upwards, the kinematic one has
// not; gyro[3] = mat' w; accel[3] = mat' (acc - gravity)
__host__ __device__ inline void sgp_motion(const double* DD, const SgDynOff& d, const double* rec, const double* local, const double* quat, double* pos, double* mat,
                                           double* vel, double* acc, double* gyro, double* accel) {
  const double *w = rec + 7, *v = rec + 10, *al = rec + SGS_ACC, *a = rec + SGS_ACC + 3, *g = DD + d.grav;
  double R[9], r[3], c[3], c1[3], c2[3], f[3];
  sgk_quat_mat(R, rec + 3);
  sgk_mv(r, R, local);
  for (int k = 0; k < 3; k++) pos[k] = rec[k] + r[k];
  if (quat) {
    double q[4] = {quat[0], quat[1], quat[2], quat[3]}, Q[9];
    sgk_quat_normalize(q);
    sgk_quat_mat(Q, q);
    for (int i = 0; i < 3; i++)
      for (int k = 0; k < 3; k++) mat[3 * i + k] = R[3 * i] * Q[k] + R[3 * i + 1] * Q[3 + k] + R[3 * i + 2] * Q[6 + k];
  } else {
    for (int k = 0; k < 9; k++) mat[k] = R[k];
  }
  sgd_cross(c, w, r);
  sgd_cross(c1, al, r);
  sgd_cross(c2, w, c);
  for (int k = 0; k < 3; k++) {
    vel[k] = w[k]; vel[3 + k] = v[k] + c[k];
    acc[k] = al[k]; acc[3 + k] = a[k] + c1[k] + c2[k] + g[k];
    f[k] = acc[3 + k] - g[k];
  }
  for (int k = 0; k < 3; k++) {   // mat' w, mat' f
    gyro[k] = mat[k] * w[0] + mat[3 + k] * w[1] + mat[6 + k] * w[2];
    accel[k] = mat[k] * f[0] + mat[3 + k] * f[1] + mat[6 + k] * f[2];
  }
}

// the dofs that move `body` get `stamp` in their records: the walk up the dof-parent chain from the body's entry.  dpar: the chain
// (the table's section, or a copy of it)
__host__ __device__ inline void sgp_mark(const int* PI, const SgPointOff& p, const int* dpar, int body, double* S, double stamp) {
  for (int i = PI[p.bdof + body]; i >= 0; i = dpar[i]) S[SGP_DOF * i + SGP_STAMP] = stamp;
}

// column d of the Jacobians of the world point P on the body whose dofs carry `stamp`: jp[3] = lin + u x P (a slider's axis; a hinge's
// u x (P - anchor); a free joint's world axis or body axis x (P - xpos)) and jr[3] = u; zeros for a dof that does not move the body
__host__ __device__ inline void sgp_jac_col(const double* Sd, double stamp, const double* P, double* jp, double* jr) {
  for (int k = 0; k < 3; k++) jp[k] = jr[k] = 0.0;
  if (Sd[SGP_STAMP] == stamp) {
    double c[3];
    sgd_cross(c, Sd, P);
    for (int k = 0; k < 3; k++) { jp[k] = Sd[3 + k] + c[k]; jr[k] = Sd[k]; }
  }
}
