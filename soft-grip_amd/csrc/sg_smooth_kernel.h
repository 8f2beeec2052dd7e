// sg_smooth_kernel.h -- the mass-matrix, joint-force and inverse-dynamics read-outs' kernel (sg_get_mass_matrix / sg_get_joint_forces /
// sg_inverse_dynamics), fp64.
//
// A kernel of sg_readout.hip's translation unit: its device assembly is in sg_readout.device.s and under the build's assembly check.
// It only READS the batch's canonical qpos, qvel and act and its per-env stiffness, so every pipeline is served without touching its kernels.
//
//   sg_smooth_kernel   one wavefront per listed env, sg_dyn_kernel's shape.  LDS holds every body's record (nbody x 29 doubles), every
//                      dof's (nv x 7) and two forces per tendon (sg_smooth.h).
//                      1. forward: bodies level by level through the kinematics table's depth schedule, a lane per body of the level:
//                         pose, twist and acceleration (the given qacc, or none), and the dofs' twists.
//                      2. a lane per body turns its acceleration into its Newton-Euler force and its inertia about the world origin;
//                         then the levels in reverse, a lane per body adding its children's sums in the child list's order.
//                      3. a lane per dof projects its body's gathered force on its twist: qfrc_bias (qacc = 0) or the Newton-Euler part
//                         of qfrc_inverse.
//                      4. a lane per dof writes row and column i of M up to the diagonal from its body's composite inertia, walking
//                         its ancestor dofs (sgs_mass_row): every entry once, no cleared buffer needed.
//                      5. tendon by tendon the lanes take the shares in 64-strides and a wavefront sum gives length and velocity, hence
//                         the tendon's two scalar forces; with spatial tendons a lane per body collects their pulls and the reverse
//                         walk runs once more; a lane per dof adds springs, dampers and the tendons' shares.
//                      ONE launch serves whichever outputs an entry point passes: a NULL output's section is skipped.
// Sums: gathers in child order, a lane's own terms in ascending order, the tendon sums by wave_sum2's butterfly.  No atomics: two calls
// give the same bits, and an env's bits depend neither on the envs listed beside it nor on which outputs are NULL.
// An env whose qpos or qvel (or qacc row, where one is read) holds a NaN or inf gets NaN in every output; nothing is indexed by a state value.
#pragma once
#include "sg_smooth.h"

struct SgSmoothArgs {
  const double* D;    // the kinematics table (sg_readout.h)
  const int* I;
  SgKinOff o;
  const double* DD;   // the dynamics table (sg_dyn.h)
  const int* DI;
  SgDynOff d;
  const double* SD;   // the smooth table (sg_smooth.h)
  const int* SI;
  SgSmoothOff s;
  const double *qpos, *qvel, *act, *kenv;
  const int *kmask_jnt, *kmask_ten;
  const int* env_ids;   // device, n_ids entries (NULL: env k = k)
  int n_ids;
  double* M;                          // [n_ids][nv][nv]; any output may be NULL
  double *bias, *passive, *actuator;  // [n_ids][nv]
  const double* qacc;                 // [n_ids][nv], read when inverse is asked
  double* inverse;                    // [n_ids][nv]
};

// the levels from the leaves up: every body of a level adds its children's slots [from, from + count)
__device__ __forceinline__ void sgs_gather_levels(const SgSmoothArgs& a, double* recs, int lane, int from, int count) {
  const SgKinOff& o = a.o;
  for (int L = o.nlevel - 2; L >= 1; L--) {
    const int b0 = a.I[o.lstart + L], b1 = a.I[o.lstart + L + 1];
    for (int s = b0 + lane; s < b1; s += 64) sgs_gather(a.SI, a.s, recs, a.I[o.lbody + s], from, count);
    __syncthreads();
  }
}

__global__ __launch_bounds__(64) void sg_smooth_kernel(SgSmoothArgs a) {
  extern __shared__ double ss_lds[];   // [nbody][SGS_REC], [nv][SGS_DOF], [ntendon][2]
  const SgKinOff& o = a.o;
  const SgDynOff& d = a.d;
  const SgSmoothOff& sm = a.s;
  double* recs = ss_lds;
  double* S = recs + (size_t)SGS_REC * o.nbody;
  double* ften = S + (size_t)SGS_DOF * d.nv;
  const int k = blockIdx.x, lane = threadIdx.x;
  const int env = a.env_ids ? a.env_ids[k] : k;
  const double* q = a.qpos + (size_t)env * o.nq;
  const double* qd = a.qvel + (size_t)env * d.nv;
  const double* qdd = a.inverse ? a.qacc + (size_t)k * d.nv : nullptr;
  bool bad = false;
  for (int i = lane; i < o.nq; i += 64) bad |= !isfinite(q[i]);
  for (int i = lane; i < d.nv; i += 64) bad |= !isfinite(qd[i]);
  if (qdd)
    for (int i = lane; i < d.nv; i += 64) bad |= !isfinite(qdd[i]);
  bad = __syncthreads_or(bad);
  const double qnan = __longlong_as_double(0x7ff8000000000000ll);
  const size_t row = (size_t)k * d.nv;
  if (bad) {
    for (int i = lane; i < d.nv; i += 64) {
      if (a.bias) a.bias[row + i] = qnan;
      if (a.passive) a.passive[row + i] = qnan;
      if (a.actuator) a.actuator[row + i] = qnan;
      if (a.inverse) a.inverse[row + i] = qnan;
    }
    if (a.M)
      for (size_t i = lane; i < (size_t)d.nv * d.nv; i += 64) a.M[row * d.nv + i] = qnan;
    return;
  }
  // 1. forward
  if (lane == 0) sgs_world(a.DD, d, recs);
  __syncthreads();
  for (int L = 1; L < o.nlevel; L++) {
    const int b0 = a.I[o.lstart + L], b1 = a.I[o.lstart + L + 1];
    for (int s = b0 + lane; s < b1; s += 64) {
      const int i = a.I[o.lbody + s], p = a.I[o.bpar + i];
      sgs_body(a.D, a.I, o, a.DD, d, a.DI + d.jdof, q, qd, qdd, i, recs + SGS_REC * p, recs + SGS_REC * i, S);
    }
    __syncthreads();
  }
  // 2. - 4. Newton-Euler forces and composite inertias, gathered; the dofs' forces; the mass matrix
  if (a.M || a.bias || a.inverse) {
    for (int i = 1 + lane; i < o.nbody; i += 64) sgs_body_force(a.DD, d, recs + SGS_REC * i, i);
    __syncthreads();
    sgs_gather_levels(a, recs, lane, SGS_ACC, SGS_REC - SGS_ACC);
    for (int i = lane; i < d.nv; i += 64) {
      const double f = sgs_project(S + SGS_DOF * i, recs + SGS_REC * a.SI[sm.dbody + i] + SGS_ACC);
      S[SGS_DOF * i + 6] = f;
      if (a.bias) a.bias[row + i] = f;
    }
    if (a.M)
      for (int i = lane; i < d.nv; i += 64) sgs_mass_row(a.SI, sm, a.DD, d, recs, S, i, a.M + row * d.nv);
  }
  // 5. springs, dampers, tendons and actuators
  if (a.passive || a.actuator || a.inverse) {
    const double kenv = a.kenv[env];
    for (int t = 0; t < d.ntendon; t++) {
      double len = 0.0, vel = 0.0;
      const int w0 = a.DI[d.tadr + t], n = sgd_nshare(a.DI, d, t);
      for (int s = lane; s < n; s += 64) {
        double l1, v1;
        sgs_wrap(a.I, o, a.DD, a.DI, d, q, qd, recs, w0 + s, &l1, &v1);
        len += l1; vel += v1;
      }
      len = wave_sum2(len);
      vel = wave_sum2(vel);
      double ft[2];
      sgs_tendon_force(a.SD, a.SI, sm, a.DD, d, a.act + (size_t)env * sm.nu, t, len, vel, a.kmask_ten[t], kenv, ft);
      if (lane == 0) { ften[2 * t] = ft[0]; ften[2 * t + 1] = ft[1]; }
    }
    __syncthreads();   // (ften; and every lane is past its reads of the records' force and inertia slots)
    if (sm.nspatial) {
      for (int i = lane; i < o.nbody; i += 64) sgs_body_tendons(a.DD, a.DI, d, ften, recs, i);
      __syncthreads();
      sgs_gather_levels(a, recs, lane, SGS_ACC, 12);
    }
    for (int i = lane; i < d.nv; i += 64) {
      double f[2];
      sgs_dof_applied(a.SD, a.SI, sm, a.I, o, a.DD, a.DI, d, q, qd, recs, S, ften, a.kmask_jnt, kenv, i, f);
      if (a.passive) a.passive[row + i] = f[0];
      if (a.actuator) a.actuator[row + i] = f[1];
      if (a.inverse) a.inverse[row + i] = S[SGS_DOF * i + 6] + a.DD[d.arm + i] * qdd[i] - f[0];
    }
  }
}
