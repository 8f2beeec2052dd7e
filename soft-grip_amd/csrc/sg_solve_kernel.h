// sg_solve_kernel.h -- the kernel of the read-outs that start with the inverse of the mass matrix (sg_solve_mass / sg_forward_smooth /
// sg_get_point_inertia), fp64.
//
// A kernel of sg_readout.hip's translation unit: its device assembly is in sg_readout.device.s and under the build's assembly check.
// It only READS the batch's canonical qpos, qvel and act and its per-env stiffness, so every pipeline is served without touching its kernels.
//
//   sg_solve_kernel   one wavefront per listed env, sg_smooth_kernel's shape.  LDS holds sg_smooth_kernel's records, the packed factor of
//                     M with M's diagonal (nM + nv doubles) and a tile of right-hand sides (sg_solve.h).
//                     1. the NaN check of the rows the call uses.
//                     2. forward: bodies level by level (sgs_body, qacc = none); sg_solve_mass and sg_get_point_inertia walk at a row
//                        of zeros for qvel, M being a function of qpos alone.
//                     3. a lane per body: Newton-Euler force and inertia (sgs_body_force), then the reverse gather.
//                     4. a lane per packed entry of M (sgv_mass_entry).
//                     5. the factor, levels from the deepest: a lane per packed entry of the level's rows gathers its descendants'
//                        terms serially in ascending order (sgv_factor_entry), then the off-diagonal entries are divided by the diagonal.
//                     6. the pivot figure min D / M_ii; an env with a D that is not finite or not positive ends here, in NaN.
//                     7. the right-hand sides, tile by tile: rows of y; or passive + actuator + applied - bias, formed as stage 5 of
//                        sg_smooth_kernel forms them; or the six rows of J of every point of the tile.
//                     8. the solve: lanes over (right-hand side of the tile) x (dof of the level) -- up sweep, scaling, down sweep.
//                     9. the store: x; or qacc_smooth; or W, a lane per pair (a <= b) of a point, stored twice.
//                     ONE kernel serves the three entry points (mode); a NULL output's section is skipped.
// The gathers of the factor and of the up sweep run serially in a lane, up to 223 terms under the free ball's root dofs: the order is
// the table's and the g++ build's.  Measured against an experiment build that spread the gathers of more than 64 terms over the lanes
// and summed with wave_sum2: 2.5 x faster on the free ball's one right-hand side, nothing to gain on the grippers,
// whose gathers have at most 15 terms; it wants its own list of long entries in the table and was not taken into this kernel.
// No sums across lanes and no atomics: two calls give the same bits; an env's bits depend neither on the envs listed beside it nor on
// which outputs are NULL; a right-hand side's or a point's neither on how many stand beside it nor on its place -- the tile size cannot
// change bits.  An env whose qpos (or qvel, y rows, qfrc_applied row, where the call reads them) holds a NaN or inf gets NaN in every
// output; nothing is indexed by a state value.
#pragma once
#include "sg_solve.h"
#include "sg_point.h"   // sgp_pos

#define SGV_MODE_SOLVE 0
#define SGV_MODE_FORWARD 1
#define SGV_MODE_POINT 2

struct SgSolveArgs {
  const double* D;    // the kinematics table (sg_readout.h)
  const int* I;
  SgKinOff o;
  const double* DD;   // the dynamics table (sg_dyn.h)
  const int* DI;
  SgDynOff d;
  const double* SD;   // the smooth table (sg_smooth.h)
  const int* SI;
  SgSmoothOff s;
  const int* VI;      // the solve table (sg_solve.h)
  SgSolveOff v;
  const double *qpos, *qvel, *act, *kenv;
  const double* zero;   // [nv] zeros: the qvel sg_solve_mass and sg_get_point_inertia walk at
  const int *kmask_jnt, *kmask_ten;
  const int* env_ids;   // device, n_ids entries (NULL: env k = k)
  int n_ids, mode;
  int n_rhs, tile;      // right-hand sides (SOLVE) or points (POINT) of an env, and how many of them a tile holds
  const int* rhs_count; // SOLVE: [n_ids] how many of an env's n_rhs rows are there, or NULL: all.  The others are not read, and not written
                        // either EXCEPT for an env that ends in NaN (sgv_fill): x must have room for all n_rhs rows of every env
  const double* y;      // SOLVE: [n_ids][n_rhs][nv]
  double* x;            //        [n_ids][n_rhs][nv] or NULL; may be y
  const double* applied;   // FORWARD: [n_ids][nv] or NULL: zero
  double *qacc, *qfrc;     //          [n_ids][nv]; any may be NULL
  const int* pt_body;      // POINT: device [n_rhs]
  const double* pt_pos;    //        device [n_rhs][3]
  double* W;               //        [n_ids][n_rhs][6][6] or NULL
  double* pivot;           // [n_ids] or NULL
};

__device__ __forceinline__ double sgv_wave_min(double x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x = fmin(x, __shfl_xor(x, o));
  return x;
}

// every output of env k but the pivot figure becomes `val`
__device__ __forceinline__ void sgv_fill(const SgSolveArgs& a, int k, int lane, double val) {
  const size_t nv = a.d.nv;
  if (a.mode == SGV_MODE_SOLVE && a.x)
    for (size_t i = lane; i < (size_t)a.n_rhs * nv; i += 64) a.x[(size_t)k * a.n_rhs * nv + i] = val;
  if (a.mode == SGV_MODE_FORWARD)
    for (size_t i = lane; i < nv; i += 64) {
      if (a.qacc) a.qacc[(size_t)k * nv + i] = val;
      if (a.qfrc) a.qfrc[(size_t)k * nv + i] = val;
    }
  if (a.mode == SGV_MODE_POINT && a.W)
    for (size_t i = lane; i < (size_t)a.n_rhs * 36; i += 64) a.W[(size_t)k * a.n_rhs * 36 + i] = val;
}

// the levels from the leaves up: every body of a level adds its children's slots [from, from + count)
__device__ __forceinline__ void sgv_gather_levels(const SgSolveArgs& a, double* recs, int lane, int from, int count) {
  const SgKinOff& o = a.o;
  for (int L = o.nlevel - 2; L >= 1; L--) {
    const int b0 = a.I[o.lstart + L], b1 = a.I[o.lstart + L + 1];
    for (int s = b0 + lane; s < b1; s += 64) sgs_gather(a.SI, a.s, recs, a.I[o.lbody + s], from, count);
    __syncthreads();
  }
}

// X[nr][nv] <- M^-1 X: lanes over (right-hand side) x (dof of the level).  Ends synchronised
__device__ __forceinline__ void sgv_solve_tile(const SgSolveArgs& a, const double* F, double* X, int nr, int lane) {
  const SgSolveOff& v = a.v;
  const int nv = a.d.nv;
  for (int L = v.nlevel - 2; L >= 0; L--) {   // (the deepest level has no descendants)
    const int l0 = a.VI[v.lstart + L], n = a.VI[v.lstart + L + 1] - l0;
    for (int w = lane; w < nr * n; w += 64) {
      const int r = w / n, j = a.VI[v.ldof + l0 + w % n];
      X[r * nv + j] = sgv_up(a.VI, v, F, X + r * nv, j);
    }
    __syncthreads();
  }
  for (int w = lane; w < nr * nv; w += 64) {
    const int r = w / nv, i = w % nv;
    X[w] = sgv_scale(a.VI, v, F, X + r * nv, i);
  }
  __syncthreads();
  for (int L = 1; L < v.nlevel; L++) {
    const int l0 = a.VI[v.lstart + L], n = a.VI[v.lstart + L + 1] - l0;
    for (int w = lane; w < nr * n; w += 64) {
      const int r = w / n, i = a.VI[v.ldof + l0 + w % n];
      X[r * nv + i] = sgv_down(a.VI, v, F, X + r * nv, i);
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(64) void sg_solve_kernel(SgSolveArgs a) {
  extern __shared__ __attribute__((aligned(16))) double sv_lds[];   // [nbody][SGS_REC], [nv][SGS_DOF], [ntendon][2], [nM], [nv], [tile][nv]
  const SgKinOff& o = a.o;
  const SgDynOff& d = a.d;
  const SgSmoothOff& sm = a.s;
  const SgSolveOff& v = a.v;
  double* recs = sv_lds;
  double* S = recs + (size_t)SGS_REC * o.nbody;
  double* ften = S + (size_t)SGS_DOF * d.nv;
  double* F = ften + 2 * (size_t)d.ntendon;
  double* mdiag = F + v.nM;
  double* X = mdiag + d.nv;
  const int k = blockIdx.x, lane = threadIdx.x;
  const int env = a.env_ids ? a.env_ids[k] : k;
  const int nv = d.nv;
  const double* q = a.qpos + (size_t)env * o.nq;
  const double* qd = a.mode == SGV_MODE_FORWARD ? a.qvel + (size_t)env * nv : a.zero;
  const double qnan = __longlong_as_double(0x7ff8000000000000ll);
  const int n_rhs = a.rhs_count ? max(0, min(a.n_rhs, a.rhs_count[k])) : a.n_rhs;   // (the rows' stride stays a.n_rhs)
  // 1. the NaN check
  bool bad = false;
  for (int i = lane; i < o.nq; i += 64) bad |= !isfinite(q[i]);
  if (a.mode == SGV_MODE_FORWARD) {
    for (int i = lane; i < nv; i += 64) bad |= !isfinite(qd[i]);
    if (a.applied)
      for (int i = lane; i < nv; i += 64) bad |= !isfinite(a.applied[(size_t)k * nv + i]);
  }
  if (a.mode == SGV_MODE_SOLVE)
    for (size_t i = lane; i < (size_t)n_rhs * nv; i += 64) bad |= !isfinite(a.y[(size_t)k * a.n_rhs * nv + i]);
  bad = __syncthreads_or(bad);
  if (bad) {
    sgv_fill(a, k, lane, qnan);
    if (a.pivot && lane == 0) a.pivot[k] = qnan;
    return;
  }
  // 2. forward
  if (lane == 0) sgs_world(a.DD, d, recs);
  __syncthreads();
  for (int L = 1; L < o.nlevel; L++) {
    const int b0 = a.I[o.lstart + L], b1 = a.I[o.lstart + L + 1];
    for (int s = b0 + lane; s < b1; s += 64) {
      const int i = a.I[o.lbody + s], p = a.I[o.bpar + i];
      sgs_body(a.D, a.I, o, a.DD, d, a.DI + d.jdof, q, qd, nullptr, i, recs + SGS_REC * p, recs + SGS_REC * i, S);
    }
    __syncthreads();
  }
  // 3. Newton-Euler forces and composite inertias, gathered; the dofs' bias forces
  for (int i = 1 + lane; i < o.nbody; i += 64) sgs_body_force(a.DD, d, recs + SGS_REC * i, i);
  __syncthreads();
  sgv_gather_levels(a, recs, lane, SGS_ACC, SGS_REC - SGS_ACC);
  if (a.mode == SGV_MODE_FORWARD)
    for (int i = lane; i < nv; i += 64) S[SGS_DOF * i + 6] = sgs_project(S + SGS_DOF * i, recs + SGS_REC * a.SI[sm.dbody + i] + SGS_ACC);
  // 4. the packed M
  for (int e = lane; e < v.nM; e += 64) {
    const double val = sgv_mass_entry(a.VI, v, a.SI, sm, a.DD, d, recs, S, e);
    F[e] = val;
    if (a.VI[v.anc + e] == a.VI[v.erow + e]) mdiag[a.VI[v.erow + e]] = val;
  }
  __syncthreads();
  // 5. the factor
  for (int L = v.nlevel - 1; L >= 0; L--) {
    const int e0 = a.VI[v.elstart + L], e1 = a.VI[v.elstart + L + 1];
    if (L < v.nlevel - 1) {   // (the deepest level has no descendants)
      for (int s = e0 + lane; s < e1; s += 64) {
        const int e = a.VI[v.eidx + s];
        F[e] = sgv_factor_entry(a.VI, v, F, e);
      }
      __syncthreads();
    }
    if (L > 0) {
      for (int s = e0 + lane; s < e1; s += 64) {
        const int e = a.VI[v.eidx + s];
        if (a.VI[v.anc + e] != a.VI[v.erow + e]) F[e] = sgv_factor_scale(a.VI, v, F, e);
      }
      __syncthreads();
    }
  }
  // 6. the pivot figure
  double pmin = INFINITY;
  bool pbad = false, pnan = false;
  for (int i = lane; i < nv; i += 64) {
    const double Di = F[a.VI[v.rstart + i]], r = sgv_pivot_ratio(a.VI, v, F, mdiag, i);
    pbad |= !isfinite(Di) || !(Di > 0.0);
    pnan |= r != r;
    pmin = fmin(pmin, r);
  }
  pbad = __syncthreads_or(pbad);
  pnan = __syncthreads_or(pnan);
  pmin = sgv_wave_min(pmin);
  if (a.pivot && lane == 0) a.pivot[k] = pnan ? qnan : pmin;
  if (pbad) {
    sgv_fill(a, k, lane, qnan);
    return;
  }
  // 7. - 9. right-hand sides, solve, store
  if (a.mode == SGV_MODE_SOLVE) {
    if (!a.x) return;
    const size_t at = (size_t)k * a.n_rhs * nv;
    for (int r0 = 0; r0 < n_rhs; r0 += a.tile) {
      const int nr = min(a.tile, n_rhs - r0);
      for (int w = lane; w < nr * nv; w += 64) X[w] = a.y[at + (size_t)r0 * nv + w];
      __syncthreads();
      sgv_solve_tile(a, F, X, nr, lane);
      for (int w = lane; w < nr * nv; w += 64) a.x[at + (size_t)r0 * nv + w] = X[w];
      __syncthreads();   // (every lane is past its reads of the tile before the next one is loaded)
    }
    return;
  }
  if (a.mode == SGV_MODE_FORWARD) {
    if (!a.qacc && !a.qfrc) return;
    // sg_smooth_kernel's stage 5: springs, dampers, tendons and actuators
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
    __syncthreads();
    if (sm.nspatial) {
      for (int i = lane; i < o.nbody; i += 64) sgs_body_tendons(a.DD, a.DI, d, ften, recs, i);
      __syncthreads();
      sgv_gather_levels(a, recs, lane, SGS_ACC, 12);
    }
    const size_t row = (size_t)k * nv;
    for (int i = lane; i < nv; i += 64) {
      double f[2];
      sgs_dof_applied(a.SD, a.SI, sm, a.I, o, a.DD, a.DI, d, q, qd, recs, S, ften, a.kmask_jnt, kenv, i, f);
      const double fs = f[0] + f[1] + (a.applied ? a.applied[row + i] : 0.0) - S[SGS_DOF * i + 6];
      X[i] = fs;
      if (a.qfrc) a.qfrc[row + i] = fs;
    }
    __syncthreads();
    if (!a.qacc) return;
    sgv_solve_tile(a, F, X, 1, lane);
    for (int i = lane; i < nv; i += 64) a.qacc[row + i] = X[i];
    return;
  }
  // the point inertias: a.tile points, six right-hand sides each
  if (!a.W) return;
  for (int p0 = 0; p0 < a.n_rhs; p0 += a.tile) {
    const int np = min(a.tile, a.n_rhs - p0);
    for (int w = lane; w < np * 6 * nv; w += 64) X[w] = 0.0;
    __syncthreads();
    for (int pp = 0; pp < np; pp++) {   // the six rows of J: a lane per dof of the chain from the point's body up
      const int body = a.pt_body[p0 + pp], e0 = a.VI[v.bdof + body];
      if (e0 < 0) continue;
      const int r = a.VI[v.rstart + e0], n = a.VI[v.depth + e0];
      double P[3];
      sgp_pos(recs + SGS_REC * body, a.pt_pos + 3 * (p0 + pp), P);
      for (int t = lane; t <= n; t += 64) {
        const int dof = a.VI[v.anc + r + t];
        double c6[6];
        sgv_jcol(S + SGS_DOF * dof, P, c6);
        for (int c = 0; c < 6; c++) X[(pp * 6 + c) * nv + dof] = c6[c];
      }
    }
    __syncthreads();
    sgv_solve_tile(a, F, X, 6 * np, lane);
    for (int w = lane; w < np * 21; w += 64) {   // a lane per pair a <= b of a point
      const int pp = w / 21;
      int b = 0, c = w % 21;
      while (c > b) { c -= b + 1; b++; }   // pair c <= b of the upper triangle, row by row of its transpose
      const int body = a.pt_body[p0 + pp];
      double P[3];
      sgp_pos(recs + SGS_REC * body, a.pt_pos + 3 * (p0 + pp), P);
      const double w6 = sgv_w_entry(a.VI, v, S, X + (size_t)pp * 6 * nv, nv, a.VI[v.bdof + body], P, c, b);
      double* out = a.W + ((size_t)k * a.n_rhs + p0 + pp) * 36;
      out[6 * c + b] = w6;
      out[6 * b + c] = w6;
    }
    __syncthreads();   // (every lane is past its reads of the tile before the next one is cleared)
  }
}
