// sg_dyn_kernel.h -- the velocity, tendon and energy read-outs' kernel (sg_get_velocities / sg_get_tendons / sg_get_energy), fp64.
//
// A kernel of sg_readout.hip's translation unit: its device assembly is in sg_readout.device.s and under the build's assembly check.
// It only READS the batch's canonical qpos and qvel and its per-env stiffness, so every pipeline is served without touching its kernels.
//
//   sg_dyn_kernel   one wavefront per listed env, sg_kin_kernel's shape.  Bodies go level by level through the kinematics table's depth
//                   schedule (a lane per body of the level, 64-body strides); every body's pose and twist stay in LDS (nbody x 13 doubles,
//                   sg_dyn.h).  Then, as the outputs ask: a lane per body writes the velocities; per tendon the lanes take its wraps /
//                   segments in 64-strides and a wavefront sum gives length and velocity; lanes over bodies, joints and dofs give the four
//                   energy terms.  ONE launch serves whichever outputs an entry point passes: a NULL output's section is skipped.
// Sums: every lane adds its 64-strided shares in ascending order, then the xor butterfly of wave_sum2 (sg_work.h).  No atomics: two calls
// give the same bits, and an env's bits do not depend on which envs are listed beside it.
// An env whose qpos or qvel holds a NaN or inf gets NaN in every output; nothing is indexed by a state value.
#pragma once
#include "sg_dyn.h"

struct SgDynArgs {
  const double* D;    // the kinematics table (sg_readout.h)
  const int* I;
  SgKinOff o;
  const double* DD;   // the dynamics table (sg_dyn.h)
  const int* DI;
  SgDynOff d;
  const double *qpos, *qvel, *kenv;
  const int *kmask_jnt, *kmask_ten;
  const int* env_ids;   // device, n_ids entries (NULL: env k = k)
  int n_ids;
  double *ang, *lin, *com_lin;   // [n_ids][nbody][3]; any may be NULL
  double *ten_len, *ten_vel;     // [n_ids][ntendon]
  double* energy;                // [n_ids][4]: gravity, joint springs, tendon springs, kinetic
};

__global__ __launch_bounds__(64) void sg_dyn_kernel(SgDynArgs a) {
  extern __shared__ double sd_body[];   // [nbody][SGD_REC]
  const SgKinOff& o = a.o;
  const SgDynOff& d = a.d;
  const int k = blockIdx.x, lane = threadIdx.x;
  const int env = a.env_ids ? a.env_ids[k] : k;
  const double* q = a.qpos + (size_t)env * o.nq;
  const double* qd = a.qvel + (size_t)env * d.nv;
  bool bad = false;
  for (int i = lane; i < o.nq; i += 64) bad |= !isfinite(q[i]);
  for (int i = lane; i < d.nv; i += 64) bad |= !isfinite(qd[i]);
  bad = __syncthreads_or(bad);
  const double qnan = __longlong_as_double(0x7ff8000000000000ll);
  if (lane < SGD_REC) sd_body[lane] = lane == 3 ? 1.0 : 0.0;   // the world: at rest at the origin
  __syncthreads();
  if (!bad) {
    for (int L = 1; L < o.nlevel; L++) {
      const int b0 = a.I[o.lstart + L], b1 = a.I[o.lstart + L + 1];
      for (int s = b0 + lane; s < b1; s += 64) {
        const int i = a.I[o.lbody + s], p = a.I[o.bpar + i];
        sgd_body(a.D, a.I, o, a.DI + d.jdof, q, qd, i, sd_body + SGD_REC * p, sd_body + SGD_REC * i);
      }
      __syncthreads();
    }
  }
  // 1. velocities: a lane per body
  if (a.ang || a.lin || a.com_lin) {
    for (int i = lane; i < o.nbody; i += 64) {
      const double* rec = sd_body + SGD_REC * i;
      const size_t at = ((size_t)k * o.nbody + i) * 3;
      if (a.ang)
        for (int c = 0; c < 3; c++) a.ang[at + c] = bad ? qnan : rec[7 + c];
      if (a.lin)
        for (int c = 0; c < 3; c++) a.lin[at + c] = bad ? qnan : rec[10 + c];
      if (a.com_lin) {
        double xi[3], vc[3] = {qnan, qnan, qnan};
        if (!bad) sgd_com(a.DD, d, rec, i, xi, vc);
        for (int c = 0; c < 3; c++) a.com_lin[at + c] = vc[c];
      }
    }
  }
  // 2. tendons: lanes over a tendon's shares, one tendon after the other (the energy's tendon term needs the lengths too)
  const double kenv = a.kenv[env];
  double e_ten = 0.0;
  if (a.ten_len || a.ten_vel || a.energy) {
    for (int t = 0; t < d.ntendon; t++) {
      double len = 0.0, vel = 0.0;
      if (!bad) {
        const int w0 = a.DI[d.tadr + t], n = sgd_nshare(a.DI, d, t);
        for (int s = lane; s < n; s += 64) {
          double l1, v1;
          sgd_wrap(a.D, a.I, o, a.DD, a.DI, d, q, qd, sd_body, w0 + s, &l1, &v1);
          len += l1; vel += v1;
        }
        len = wave_sum2(len);
        vel = wave_sum2(vel);
        e_ten += sgd_tendon_spring(a.DD, d, t, len, a.kmask_ten[t], kenv);
      }
      if (lane == 0) {
        if (a.ten_len) a.ten_len[(size_t)k * d.ntendon + t] = bad ? qnan : len;
        if (a.ten_vel) a.ten_vel[(size_t)k * d.ntendon + t] = bad ? qnan : vel;
      }
    }
  }
  // 3. energy: lanes over bodies (gravity, kinetic), joints (springs) and dofs (armature)
  if (a.energy) {
    double e_grav = 0.0, e_jnt = 0.0, e_kin = 0.0;
    if (!bad) {
      for (int i = 1 + lane; i < o.nbody; i += 64) {
        double g1, k1;
        sgd_body_energy(a.DD, d, sd_body + SGD_REC * i, i, &g1, &k1);
        e_grav += g1; e_kin += k1;
      }
      for (int j = lane; j < o.njnt; j += 64) e_jnt += sgd_joint_spring(a.I, o, a.DD, d, q, j, a.kmask_jnt[j], kenv);
      for (int i = lane; i < d.nv; i += 64) e_kin += 0.5 * a.DD[d.arm + i] * qd[i] * qd[i];
      e_grav = wave_sum2(e_grav);
      e_jnt = wave_sum2(e_jnt);
      e_kin = wave_sum2(e_kin);
    }
    if (lane == 0) {
      double* out = a.energy + (size_t)k * 4;
      out[0] = bad ? qnan : e_grav; out[1] = bad ? qnan : e_jnt; out[2] = bad ? qnan : e_ten; out[3] = bad ? qnan : e_kin;
    }
  }
}
