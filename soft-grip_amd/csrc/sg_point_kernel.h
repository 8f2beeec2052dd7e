// sg_point_kernel.h -- the point read-outs' kernel (sg_get_point_motion / sg_get_jacobians), fp64.
//
// A kernel of sg_readout.hip's translation unit: its device assembly is in sg_readout.device.s and under the build's assembly check.
// It only READS the batch's canonical qpos and qvel (or the rows the caller passes in their place), so every pipeline is served without
// touching its kernels.
//
//   sg_point_kernel   one wavefront per listed env, sg_smooth_kernel's shape.  LDS holds every body's record (nbody x 19 doubles), every
//                     dof's twist and stamp (nv x 7 doubles) and the dof-parent chain (nv ints) (sg_point.h).
//                     1. forward: bodies level by level through the kinematics table's depth schedule, a lane per body of the level
//                        (sgs_body): pose, twist and acceleration at the given qacc, or at none, and the dofs' twists.
//                     2. motion: a lane per point, in 64-strides (sgp_motion); each output a point's own 3, 6 or 9 doubles.
//                     3. Jacobians, point by point: lane 0 walks the dof-parent chain up from the point's body and stamps the dofs
//                        on it with the point's number (sgp_mark: no clearing between points); then the lanes run ACROSS the dofs,
//                        a lane per column in 64-strides, so each of the point's six rows leaves as runs of 64 consecutive doubles.
//                        A dof without the stamp writes its zeros: every entry of jacp and jacr is written.
//                     ONE launch serves both entry points: a NULL output's section is skipped.
// No sums across lanes and no atomics: two calls give the same bits, an env's bits depend neither on the envs listed beside it nor on
// which outputs are NULL, a point's neither on n_pts nor on its place in the list.
// An env whose qpos, qvel or qacc row (those in use: the Jacobians use qpos alone, and walk at a row of zeros for qvel) holds a NaN or
// inf gets NaN in every output; nothing is indexed by a state value.
#pragma once
#include "sg_point.h"

struct SgPointArgs {
  const double* D;    // the kinematics table (sg_readout.h)
  const int* I;
  SgKinOff o;
  const double* DD;   // the dynamics table (sg_dyn.h)
  const int* DI;
  SgDynOff d;
  const int* PI;      // the point table (sg_point.h)
  SgPointOff p;
  const double *qpos, *qvel;   // the batch's [n][nq], [n][nv] (row = env id), or with `given` bit 0 / 1 set the caller's [n_ids][..] (row = k)
  const double* qacc;          // [n_ids][nv] or NULL: zero
  int given;                   // bit 2: no velocity is asked for (sg_get_jacobians) -- qvel is ONE row of nv zeros that every env walks at, unchecked
  const int* env_ids;   // device, n_ids entries (NULL: env k = k)
  int n_ids, n_pts;
  const int* pt_body;       // device [n_pts]
  const double* pt_pos;     // device [n_pts][3]
  const double* pt_quat;    // device [n_pts][4] or NULL: identity
  double *pos, *mat, *vel, *acc, *gyro, *accel;   // [n_ids][n_pts][3 | 9 | 6 | 6 | 3 | 3]; any output may be NULL
  double *jacp, *jacr;                            // [n_ids][n_pts][3][nv]
};

__device__ __forceinline__ void sgp_put(double* out, size_t at, int n, const double* v, bool bad, double qnan) {
  if (!out) return;
  for (int c = 0; c < n; c++) out[at * n + c] = bad ? qnan : v[c];
}

__global__ __launch_bounds__(64) void sg_point_kernel(SgPointArgs a) {
  extern __shared__ double sp_lds[];   // [nbody][SGP_REC], [nv][SGP_DOF], then nv ints
  const SgKinOff& o = a.o;
  const SgDynOff& d = a.d;
  double* recs = sp_lds;
  double* S = recs + (size_t)SGP_REC * o.nbody;
  int* dpar = (int*)(S + (size_t)SGP_DOF * d.nv);
  const int k = blockIdx.x, lane = threadIdx.x;
  const int env = a.env_ids ? a.env_ids[k] : k;
  const double* q = a.qpos + (size_t)((a.given & 1) ? k : env) * o.nq;
  const double* qd = (a.given & 4) ? a.qvel : a.qvel + (size_t)((a.given & 2) ? k : env) * d.nv;
  const double* qdd = a.qacc ? a.qacc + (size_t)k * d.nv : nullptr;
  bool bad = false;
  for (int i = lane; i < o.nq; i += 64) bad |= !isfinite(q[i]);
  if (!(a.given & 4))
    for (int i = lane; i < d.nv; i += 64) bad |= !isfinite(qd[i]);
  if (qdd)
    for (int i = lane; i < d.nv; i += 64) bad |= !isfinite(qdd[i]);
  bad = __syncthreads_or(bad);
  const double qnan = __longlong_as_double(0x7ff8000000000000ll);
  const size_t nv = d.nv, prow = (size_t)k * a.n_pts;
  const bool motion = a.pos || a.mat || a.vel || a.acc || a.gyro || a.accel;
  if (!bad) {
    // 1. forward
    for (int i = lane; i < d.nv; i += 64) { S[SGP_DOF * i + SGP_STAMP] = 0.0; dpar[i] = a.PI[a.p.dpar + i]; }
    if (lane == 0) sgp_world(a.DD, d, recs);
    __syncthreads();
    for (int L = 1; L < o.nlevel; L++) {
      const int b0 = a.I[o.lstart + L], b1 = a.I[o.lstart + L + 1];
      for (int s = b0 + lane; s < b1; s += 64) {
        const int i = a.I[o.lbody + s], p = a.I[o.bpar + i];
        sgs_body(a.D, a.I, o, a.DD, d, a.DI + d.jdof, q, qd, qdd, i, recs + SGP_REC * p, recs + SGP_REC * i, S);
      }
      __syncthreads();
    }
  }
  // 2. motion: a lane per point
  if (motion)
    for (int p = lane; p < a.n_pts; p += 64) {
      double pos[3], mat[9], vel[6], acc[6], gyro[3], accel[3];
      if (!bad)
        sgp_motion(a.DD, d, recs + SGP_REC * a.pt_body[p], a.pt_pos + 3 * p, a.pt_quat ? a.pt_quat + 4 * p : nullptr, pos, mat, vel, acc, gyro, accel);
      sgp_put(a.pos, prow + p, 3, pos, bad, qnan);
      sgp_put(a.mat, prow + p, 9, mat, bad, qnan);
      sgp_put(a.vel, prow + p, 6, vel, bad, qnan);
      sgp_put(a.acc, prow + p, 6, acc, bad, qnan);
      sgp_put(a.gyro, prow + p, 3, gyro, bad, qnan);
      sgp_put(a.accel, prow + p, 3, accel, bad, qnan);
    }
  // 3. Jacobians: point by point, the lanes across the dofs
  if (!a.jacp && !a.jacr) return;
  if (bad) {
    const size_t at = prow * 3 * nv, n = (size_t)a.n_pts * 3 * nv;
    for (size_t i = lane; i < n; i += 64) {
      if (a.jacp) a.jacp[at + i] = qnan;
      if (a.jacr) a.jacr[at + i] = qnan;
    }
    return;
  }
  for (int p = 0; p < a.n_pts; p++) {
    const size_t at = (prow + p) * 3 * nv;
    const int body = a.pt_body[p];
    const double stamp = (double)(p + 1);
    double P[3];
    sgp_pos(recs + SGP_REC * body, a.pt_pos + 3 * p, P);
    if (lane == 0) sgp_mark(a.PI, a.p, dpar, body, S, stamp);
    __syncthreads();
    for (int i = lane; i < d.nv; i += 64) {
      double jp[3], jr[3];
      sgp_jac_col(S + SGP_DOF * i, stamp, P, jp, jr);
      for (int r = 0; r < 3; r++) {
        if (a.jacp) a.jacp[at + r * nv + i] = jp[r];
        if (a.jacr) a.jacr[at + r * nv + i] = jr[r];
      }
    }
    __syncthreads();   // (every lane is past its reads of the stamps before the next point's walk writes them)
  }
}
