// sg_dyn.h -- the per-env arithmetic of the velocity, tendon and energy read-outs (sg_get_velocities, sg_get_tendons, sg_get_energy):
// the dynamics table beside the kinematics table of sg_readout.h, and what one lane does for one body, one tendon segment, one joint.
// Pure functions of their arguments, compiled for gfx950 (sg_dyn_kernel.h, inside sg_readout.hip) and by g++ for the CPU tests
// (tests/dyn_ref.py), which drive the same text body by body through sgd_host_env (sg_readout_host.h).
//
// Definitions.  A body's record is 13 doubles: xpos, xquat (exactly what sgk_body gives), then its twist in world axes: the angular
// velocity and the linear velocity of the body frame's origin.  The twist is the time derivative of the pose when qpos moves as qvel says
// (mj_integratePos): slide and hinge joints at rate qvel; a free joint's position at its three linear components (world frame) and its
// quaternion at 1/2 q (0, w), w the three angular components in the BODY frame.  Joints of one body are taken in joint order, each hinge
// about its anchor in the frame the joints before it have left (sgk_body's anchors), which is mj_jac's convention: xaxis and xanchor.
#pragma once
#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif
#include "sg_readout.h"

#define SGD_REC 13        // doubles per body: xpos 3, xquat 4, angular velocity 3, linear velocity of the origin 3
// 13 doubles per body of dynamic LDS beside the kernel's static LDS (SGD_STATIC_LDS bytes: the block-wide __syncthreads_or; the kept
// assembly's figure, held by tests/test_dyn_host.py): 627 bodies are 65 208 + 256 bytes, within the 65 536 a workgroup gets without asking
#define SGD_STATIC_LDS 256
#define SGD_MAXBODY ((65536 - SGD_STATIC_LDS) / (SGD_REC * 8))

// ---- the dynamics table: one double and one int array, sections at the offsets below ----
struct SgDynOff {
  int nv, nsite, ntendon, nwrap;
  // doubles
  int bmass, bipos, bimat, jspring, jstiff, arm, spos, wprm, tstiff, tspring, grav;
  // ints
  int jdof, sbody, tadr, tnum, wtype, wobj;
};

struct SgDynHost {
  bool ok = false;
  std::string err;
  SgDynOff o;
  std::vector<double> dbl;
  std::vector<int> ints;
};

// the table from the blob (K: the model's kinematics table, whose joints and bodies it indexes); D->ok says whether the three read-outs
// can run the model
void sgd_build(const void* blob, size_t nbytes, const SgKinHost& K, SgDynHost* D);

__host__ __device__ inline void sgd_cross(double* r, const double* a, const double* b) {
  const double x = a[1] * b[2] - a[2] * b[1], y = a[2] * b[0] - a[0] * b[2], z = a[0] * b[1] - a[1] * b[0];
  r[0] = x; r[1] = y; r[2] = z;
}

// body i from its parent's record par[13] -> out[13].  The pose half is sgk_body's walk, operation by operation; the twist rides along:
// it starts as the parent's twist carried to this body's origin and gains every joint's share as the joint is passed.
__host__ __device__ inline void sgd_body(const double* D, const int* I, const SgKinOff& o, const int* jdof, const double* qpos, const double* qvel, int i,
                                         const double* par, double* out) {
  const double *pp = par, *pq = par + 3;
  double R[9], t[3], pos[3], quat[4], w[3], v[3], c[3];
  sgk_quat_mat(R, pq);
  sgk_mv(t, R, D + o.bpos + 3 * i);
  for (int k = 0; k < 3; k++) pos[k] = pp[k] + t[k];
  sgk_quat_mul(quat, pq, D + o.bquat + 4 * i);
  sgd_cross(c, par + 7, t);   // the parent's twist at pos
  for (int k = 0; k < 3; k++) { w[k] = par[7 + k]; v[k] = par[10 + k] + c[k]; }
  const int j0 = I[o.bjadr + i], nj = I[o.bjnum + i];
  for (int j = j0; j < j0 + nj; j++) {
    const int type = I[o.jtype + j], qa = I[o.jqadr + j], da = jdof[j];
    if (type == SG_JNT_FREE) {   // the pose IS the seven positions; the six velocities: linear in the world frame, angular in the body's
      for (int k = 0; k < 3; k++) pos[k] = qpos[qa + k];
      for (int k = 0; k < 4; k++) quat[k] = qpos[qa + 3 + k];
      sgk_quat_normalize(quat);
      sgk_quat_mat(R, quat);
      sgk_mv(w, R, qvel + da + 3);
      for (int k = 0; k < 3; k++) v[k] = qvel[da + k];
      continue;
    }
    const double* jp = D + o.jpos + 3 * j;
    const double* ja = D + o.jaxis + 3 * j;
    double anchor[3], axis[3];
    sgk_quat_mat(R, quat);
    sgk_mv(t, R, jp);
    for (int k = 0; k < 3; k++) anchor[k] = pos[k] + t[k];
    sgk_mv(axis, R, ja);
    const double dq = qpos[qa] - D[o.jq0 + j], qd = qvel[da];
    if (type == SG_JNT_SLIDE) {
      // the origin slides along an axis that turns with the body: d/dt (axis dq) = axis qd + (w x axis) dq
      sgd_cross(c, w, axis);
      for (int k = 0; k < 3; k++) { pos[k] = pos[k] + axis[k] * dq; v[k] += axis[k] * qd + c[k] * dq; }
    } else {
      // the anchor's velocity as a point of the body before this hinge; behind the hinge the origin turns about it at w + axis qd
      sgd_cross(c, w, t);
      for (int k = 0; k < 3; k++) { v[k] += c[k]; w[k] += axis[k] * qd; }
      const double s = sin(dq / 2);
      const double ql[4] = {cos(dq / 2), ja[0] * s, ja[1] * s, ja[2] * s};
      double qn[4];
      sgk_quat_mul(qn, quat, ql);
      for (int k = 0; k < 4; k++) quat[k] = qn[k];
      sgk_quat_mat(R, quat);
      sgk_mv(t, R, jp);
      for (int k = 0; k < 3; k++) pos[k] = anchor[k] - t[k];
      sgd_cross(c, w, t);
      for (int k = 0; k < 3; k++) v[k] -= c[k];
    }
  }
  sgk_quat_normalize(quat);
  for (int k = 0; k < 3; k++) out[k] = pos[k];
  for (int k = 0; k < 4; k++) out[3 + k] = quat[k];
  for (int k = 0; k < 3; k++) { out[7 + k] = w[k]; out[10 + k] = v[k]; }
}

// a point fixed on a body, local[3] in the body's frame: its world position and velocity from the body's record
__host__ __device__ inline void sgd_point(const double* rec, const double* local, double* x, double* xd) {
  double R[9], t[3], c[3];
  sgk_quat_mat(R, rec + 3);
  sgk_mv(t, R, local);
  sgd_cross(c, rec + 7, t);
  for (int k = 0; k < 3; k++) { x[k] = rec[k] + t[k]; xd[k] = rec[10 + k] + c[k]; }
}

// wrap w of a tendon and, for a spatial tendon, the one behind it: their share of the tendon's length and velocity.
// Fixed tendon (a joint wrap): coef q, coef qvel.  Spatial tendon (site wraps): the segment site w -> site w + 1, its length and
// unit . (v1 - v0); a segment shorter than 1e-15 counts its length and no velocity (the oracle's tendon stage skips its Jacobian).
__host__ __device__ inline void sgd_wrap(const double* D, const int* I, const SgKinOff& o, const double* DD, const int* DI, const SgDynOff& d, const double* qpos,
                                         const double* qvel, const double* recs, int w, double* len, double* vel) {
  const int obj = DI[d.wobj + w];
  if (DI[d.wtype + w] == SG_WRAP_JOINT) {
    const double coef = DD[d.wprm + w];
    *len = coef * qpos[I[o.jqadr + obj]];
    *vel = coef * qvel[DI[d.jdof + obj]];
    return;
  }
  const int s1 = DI[d.wobj + w + 1];
  double p0[3], v0[3], p1[3], v1[3];
  sgd_point(recs + SGD_REC * DI[d.sbody + obj], DD + d.spos + 3 * obj, p0, v0);
  sgd_point(recs + SGD_REC * DI[d.sbody + s1], DD + d.spos + 3 * s1, p1, v1);
  const double dx[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};
  const double L = sqrt(dx[0] * dx[0] + dx[1] * dx[1] + dx[2] * dx[2]);
  *len = L;
  *vel = L < 1e-15 ? 0.0 : (dx[0] * (v1[0] - v0[0]) + dx[1] * (v1[1] - v0[1]) + dx[2] * (v1[2] - v0[2])) / L;
}
// how many shares tendon t has: its joint wraps, or its sites less one
__host__ __device__ inline int sgd_nshare(const int* DI, const SgDynOff& d, int t) {
  const int a = DI[d.tadr + t], n = DI[d.tnum + t];
  return DI[d.wtype + a] == SG_WRAP_JOINT ? n : n - 1;
}

// body i's centre of mass xipos = xpos + R body_ipos and its velocity
__host__ __device__ inline void sgd_com(const double* DD, const SgDynOff& d, const double* rec, int i, double* xi, double* vc) {
  sgd_point(rec, DD + d.bipos + 3 * i, xi, vc);
}
// body i's shares of the gravity term, -m g . xipos, and of the kinetic term, 1/2 (m |vc|^2 + w' R I R' w), I = body_imat about the centre of mass
__host__ __device__ inline void sgd_body_energy(const double* DD, const SgDynOff& d, const double* rec, int i, double* egrav, double* ekin) {
  double xi[3], vc[3], R[9], wl[3], Iw[3];
  sgd_com(DD, d, rec, i, xi, vc);
  const double m = DD[d.bmass + i];
  const double* g = DD + d.grav;
  *egrav = -m * (g[0] * xi[0] + g[1] * xi[1] + g[2] * xi[2]);
  sgk_quat_mat(R, rec + 3);
  const double* w = rec + 7;
  for (int k = 0; k < 3; k++) wl[k] = R[k] * w[0] + R[3 + k] * w[1] + R[6 + k] * w[2];   // R' w: the angular velocity in the body's frame
  sgk_mv(Iw, DD + d.bimat + 9 * i, wl);
  *ekin = 0.5 * (m * (vc[0] * vc[0] + vc[1] * vc[1] + vc[2] * vc[2]) + (wl[0] * Iw[0] + wl[1] * Iw[1] + wl[2] * Iw[2]));
}
// joint j's spring potential 1/2 k (q - qpos_spring)^2 (slide and hinge; a free joint has no spring), k the stiffness this env's next step uses
__host__ __device__ inline double sgd_joint_spring(const int* I, const SgKinOff& o, const double* DD, const SgDynOff& d, const double* qpos, int j, int masked,
                                                   double kenv) {
  if (I[o.jtype + j] == SG_JNT_FREE) return 0.0;
  const double k = masked ? kenv : DD[d.jstiff + j], x = qpos[I[o.jqadr + j]] - DD[d.jspring + j];
  return 0.5 * k * x * x;
}
// tendon t's spring potential 1/2 k (L - tendon_lengthspring)^2
__host__ __device__ inline double sgd_tendon_spring(const double* DD, const SgDynOff& d, int t, double L, int masked, double kenv) {
  const double k = masked ? kenv : DD[d.tstiff + t], x = L - DD[d.tspring + t];
  return 0.5 * k * x * x;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- the host twins' walk (sgd_host_env in sg_readout_host.h, sgh_host_env in sg_shape.h): the records [nbody][SGD_REC] of one env, the
// world at rest, then the bodies by index (parents precede children) -- the kernels' order, stated once ----
inline void sgd_host_walk(const SgKinHost& K, const SgDynHost& Dn, const double* qpos, const double* qvel, std::vector<double>* rec) {
  const SgKinOff& o = K.o;
  rec->assign((size_t)SGD_REC * o.nbody, 0.0);
  (*rec)[3] = 1.0;
  for (int i = 1; i < o.nbody; i++)
    sgd_body(K.dbl.data(), K.ints.data(), o, Dn.ints.data() + Dn.o.jdof, qpos, qvel, i, &(*rec)[SGD_REC * K.ints[o.bpar + i]], &(*rec)[SGD_REC * i]);
}
#endif
