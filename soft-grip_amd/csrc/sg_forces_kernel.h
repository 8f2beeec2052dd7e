// sg_forces_kernel.h -- the two kernels of the constraint-force read-out (sg_get_forces), fp64.
//
// Kernels of sg_readout.hip's translation unit: their device assembly is in sg_readout.device.s and under the build's assembly check.
// They only READ the batch's canonical qpos, qvel and qacc_warmstart (and, through the kernels launched before them, act and the per-env
// stiffness), so every pipeline is served without touching its kernels.  The per-env arithmetic is sg_forces.h's, which g++ compiles too.
//
// A chunk of listed envs goes through five launches in stream order, all on one work space (sg_get_forces in sg_readout.hip):
//   sg_contacts_kernel      the contact list, at the list's capacity                                  (sg_contacts_kernel.h, as it is)
//   sg_solve_kernel         forward mode: qacc_smooth                                                  (sg_solve_kernel.h, as it is)
//   sg_forces_rows_kernel   one wavefront per env: the forward walk (sgs_body), the row list (lane 0, serially: the oracle's order),
//                           then row by row -- a cone's three rows together -- the lanes across the dofs write the DENSE row of J and
//                           take its products with qvel, qacc_smooth and qacc_warmstart (lane-strided partial sums, a fixed butterfly);
//                           impedance, R, aref, b and the warm start's force of the row go to its scalar record
//   sg_solve_kernel         solve mode with a per-env count: W = M^-1 J', nefc right-hand sides of the env's J
//   sg_forces_pgs_kernel    one wavefront per env, the hot path.  LDS: f [nrows] and the running acceleration a = M^-1 J' f [nv].
//                           Prologue: the diagonal blocks J_i . W_k + R, a of the warm start, its cost and the gate.  Sweeps: a row's
//                           residual is b + R f + J_i . a; the update is wavefront-uniform (every lane computes it), then each lane
//                           adds W_i df to ITS columns of a -- a lane reads and writes only the columns it owns, so a sweep needs no
//                           barrier.  A cone's three rows go in one pass.  Epilogue: qfrc_constraint = J' f (a lane per dof, rows in
//                           ascending order), qacc = qacc_smooth + a, the row and contact outputs.
// No atomics; every sum has a fixed shape: two calls give the same bits, and an env's bits depend neither on the chunking nor on the
// envs listed beside it nor on which outputs are NULL.  An env whose state holds a NaN or inf (or whose M has a bad pivot) reports
// nefc = ncon = -1 and NaN in every double output; nothing is indexed by a state value.
#pragma once
#include "sg_forces.h"

struct SgForcesArgs {
  const double* D;    // the kinematics table
  const int* I;
  SgKinOff o;
  const double* DD;   // the dynamics table
  const int* DI;
  SgDynOff d;
  const int* VI;      // the solve table
  SgSolveOff v;
  const double* FD;   // the forces table
  const int* FI;
  SgForceOff f;
  const double *qpos, *qvel, *warm, *zero;
  const int* env_ids;   // device, the chunk's entries
  int n_ids;
  // the chunk's work space, env k of the chunk at k times the array's stride
  double *J, *W, *sc, *qs, *cdist, *cpos, *cframe;   // [nrows][nv] x 2, [nrows][SGF_SC], [nv], [cap], [cap][3], [cap][9]
  int *rows, *cgeom, *caddr, *ncon_ws, *nefc_ws;      // [3][nrows], [cap][2], [cap], 1, 1
  // the call's outputs, at the chunk's first env; any may be NULL
  int max_rows, max_contacts;
  int32_t *nefc, *iters, *efc_type, *efc_id, *ncon;
  double *efc_force, *contact_force, *qfrc, *qacc;
};

__device__ __forceinline__ double sgf_wave_sum(double p) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) p += __shfl_xor(p, o);
  return p;
}
__device__ __forceinline__ double sgf_wave_dot(const double* x, const double* y, int n, int lane) { return sgf_wave_sum(sgf_dot_lane(x, y, n, lane)); }

__global__ __launch_bounds__(64) void sg_forces_rows_kernel(SgForcesArgs a) {
  extern __shared__ __attribute__((aligned(16))) double sf_lds[];   // [nbody][SGS_REC], [nv][SGS_DOF], then 3 nrows + cap ints
  __shared__ int s_nefc;
  const SgKinOff& o = a.o;
  const SgDynOff& d = a.d;
  const SgForceOff& f = a.f;
  const int nv = d.nv, nrows = f.nrows, cap = f.cap;
  double* recs = sf_lds;
  double* S = recs + (size_t)SGS_REC * o.nbody;
  int* rtype = (int*)(S + (size_t)SGS_DOF * nv);
  int* rid = rtype + nrows;
  int* raux = rid + nrows;
  int* caddr = raux + nrows;
  const int k = blockIdx.x, lane = threadIdx.x;
  const int env = a.env_ids[k];
  const double* q = a.qpos + (size_t)env * o.nq;
  const double* qd = a.qvel + (size_t)env * nv;
  const double* wm = a.warm + (size_t)env * nv;
  const double* qs = a.qs + (size_t)k * nv;
  const int ncon = a.ncon_ws[k];
  bool bad = ncon < 0 || ncon > cap;
  for (int i = lane; i < o.nq; i += 64) bad |= !isfinite(q[i]);
  for (int i = lane; i < nv; i += 64) bad |= !isfinite(qd[i]) || !isfinite(wm[i]) || !isfinite(qs[i]);
  bad = __syncthreads_or(bad);
  if (bad) {
    if (lane == 0) a.nefc_ws[k] = -1;
    return;
  }
  // the forward walk: poses and dof twists, the stamp slots at zero
  for (int i = lane; i < nv; i += 64) S[SGS_DOF * i + 6] = 0.0;
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
  SgfEnv E;
  E.I = a.I; E.o = o; E.DD = a.DD; E.DI = a.DI; E.d = d; E.VI = a.VI; E.v = a.v; E.FD = a.FD; E.FI = a.FI; E.f = f;
  E.qpos = q; E.zero = a.zero; E.recs = recs; E.S = S;
  E.cgeom = a.cgeom + (size_t)k * 2 * cap; E.cdist = a.cdist + (size_t)k * cap; E.cpos = a.cpos + (size_t)k * 3 * cap; E.cframe = a.cframe + (size_t)k * 9 * cap;
  // the row list
  if (lane == 0) s_nefc = sgf_row_list(a.FD, a.FI, f, a.I, o, q, ncon, E.cgeom, E.cdist, rtype, rid, raux, caddr);
  __syncthreads();
  const int ne = s_nefc;
  int* rows = a.rows + (size_t)k * 3 * nrows;
  for (int i = lane; i < ne; i += 64) { rows[i] = rtype[i]; rows[nrows + i] = rid[i]; rows[2 * nrows + i] = raux[i]; }
  for (int c = lane; c < ncon; c += 64) a.caddr[(size_t)k * cap + c] = caddr[c];
  if (lane == 0) a.nefc_ws[k] = ne;
  double* J = a.J + (size_t)k * nrows * nv;
  double* sc = a.sc + (size_t)k * nrows * SGF_SC;
  const double *opt = a.FD + f.opt, timestep = opt[0], impratio = opt[2];
  // row by row; a cone's three rows together
  for (int i = 0; i < ne;) {
    const int dim = rtype[i] == SGF_ELLIPTIC ? 3 : 1;
    double R[3], jar[3], b[3], fric[2] = {0.0, 0.0};
    for (int r = 0; r < dim; r++) {
      const int ty = rtype[i + r], id = rid[i + r], aux = raux[i + r];
      double* Jr = J + (size_t)(i + r) * nv;
      double pv = 0.0, ps = 0.0, pw = 0.0;
      for (int c = lane; c < nv; c += 64) {
        const double val = sgf_row_j(E, ty, id, aux, c);
        Jr[c] = val;
        pv += val * qd[c];
        ps += val * qs[c];
        pw += val * wm[c];
      }
      pv = sgf_wave_sum(pv); ps = sgf_wave_sum(ps); pw = sgf_wave_sum(pw);
      double pos, margin, dA, solref[2], solimp[5], K1, B1;
      sgf_row_params(E, ty, id, aux, &pos, &margin, &dA, solref, solimp);
      const double imp = sgf_impedance(solimp, pos, margin);
      sgf_kb(solref, solimp, imp, dA, timestep, &R[r], &K1, &B1);
      const double aref = sgf_aref(K1, B1, imp, pos, margin, pv);
      b[r] = ps - aref;
      jar[r] = pw - aref;
    }
    if (dim == 3) {
      int cd;
      double solref[2], solimp[5], inc;
      sgf_contact_params(a.FD, a.FI, f, E.cgeom[2 * rid[i]], E.cgeom[2 * rid[i] + 1], &cd, fric, solref, solimp, &inc);
      const double mu = sgf_cone_r(impratio, fric, R);
      const double Dd[3] = {1 / R[0], 1 / R[1], 1 / R[2]};
      double fw[3];
      sgf_warm_cone(mu, fric, Dd, jar, fw);
      if (lane == 0)
#pragma unroll
        for (int r = 0; r < 3; r++) {
          double* s = sc + (size_t)(i + r) * SGF_SC;
          s[SGF_B] = b[r]; s[SGF_R] = R[r]; s[SGF_F0] = fw[r]; s[SGF_FRIC] = fric[0]; s[SGF_FRIC + 1] = fric[1];
          s[SGF_A] = s[SGF_A + 1] = s[SGF_A + 2] = 0.0;
        }
    } else if (lane == 0) {
      double* s = sc + (size_t)i * SGF_SC;
      const double Dd = 1 / R[0];
      s[SGF_B] = b[0]; s[SGF_R] = R[0]; s[SGF_F0] = sgf_warm_scalar(rtype[i], Dd, jar[0]);
      s[SGF_A] = s[SGF_A + 1] = s[SGF_A + 2] = 0.0; s[SGF_FRIC] = s[SGF_FRIC + 1] = 0.0;
    }
    i += dim;
  }
}

// every double output of env k becomes NaN, its counts -1 (iters 0)
__device__ __forceinline__ void sgf_fill_nan(const SgForcesArgs& a, int k, int lane) {
  const double qnan = __longlong_as_double(0x7ff8000000000000ll);
  const size_t nv = a.d.nv;
  if (a.efc_force)
    for (int i = lane; i < a.max_rows; i += 64) a.efc_force[(size_t)k * a.max_rows + i] = qnan;
  if (a.contact_force)
    for (int i = lane; i < 3 * a.max_contacts; i += 64) a.contact_force[(size_t)k * 3 * a.max_contacts + i] = qnan;
  for (size_t i = lane; i < nv; i += 64) {
    if (a.qfrc) a.qfrc[(size_t)k * nv + i] = qnan;
    if (a.qacc) a.qacc[(size_t)k * nv + i] = qnan;
  }
  if (lane == 0) {
    if (a.nefc) a.nefc[k] = -1;
    if (a.ncon) a.ncon[k] = -1;
    if (a.iters) a.iters[k] = 0;
  }
}

__global__ __launch_bounds__(64) void sg_forces_pgs_kernel(SgForcesArgs a) {
  extern __shared__ __attribute__((aligned(16))) double sp_lds2[];   // f [nrows], a [nv]
  const SgForceOff& fo = a.f;
  const int nv = a.d.nv, nrows = fo.nrows, cap = fo.cap;
  double* f = sp_lds2;
  double* acc = f + nrows;
  const int k = blockIdx.x, lane = threadIdx.x;
  const int ne = a.nefc_ws[k], ncon = a.ncon_ws[k];
  if (ne < 0 || ne > nrows || ncon < 0 || ncon > cap) {
    sgf_fill_nan(a, k, lane);
    return;
  }
  const int* rtype = a.rows + (size_t)k * 3 * nrows;
  const int* rid = rtype + nrows;
  const double* J = a.J + (size_t)k * nrows * nv;
  const double* W = a.W + (size_t)k * nrows * nv;
  double* sc = a.sc + (size_t)k * nrows * SGF_SC;
  const double* qs = a.qs + (size_t)k * nv;
  const double *opt = a.FD + fo.opt, tolerance = opt[1], meaninertia = opt[3];
  // the diagonal blocks of A + R
  for (int i = 0; i < ne;) {
    const int dim = rtype[i] == SGF_ELLIPTIC ? 3 : 1;
    for (int j = 0; j < dim; j++)
      for (int c = 0; c < dim; c++) {
        const double val = sgf_wave_dot(J + (size_t)(i + j) * nv, W + (size_t)(i + c) * nv, nv, lane) + (j == c ? sc[(size_t)(i + j) * SGF_SC + SGF_R] : 0.0);
        if (lane == 0) sc[(size_t)(i + j) * SGF_SC + SGF_A + c] = val;
      }
    i += dim;
  }
  // the warm start, its acceleration, its cost and the gate
  for (int i = lane; i < ne; i += 64) f[i] = sc[(size_t)i * SGF_SC + SGF_F0];
  __syncthreads();   // (with it the blocks written above are visible to every lane)
  for (int c = lane; c < nv; c += 64) {
    double s = 0.0;
    for (int i = 0; i < ne; i++) s += W[(size_t)i * nv + c] * f[i];
    acc[c] = s;
  }
  __syncthreads();
  double cost = 0.0;
  for (int i = 0; i < ne; i++) {
    const double* s = sc + (size_t)i * SGF_SC;
    cost += sgf_warm_cost(f[i], s[SGF_R], sgf_wave_dot(J + (size_t)i * nv, acc, nv, lane), s[SGF_B]);
  }
  if (!sgf_warm_keep(cost)) {
    for (int i = lane; i < ne; i += 64) f[i] = 0.0;
    for (int c = lane; c < nv; c += 64) acc[c] = 0.0;
  }
  __syncthreads();
  // the sweeps: every lane computes the (uniform) update and writes it to f; a lane owns the columns lane, lane + 64, .. of a
  const double scale = sgf_scale(meaninertia, nv);
  int iters = 0;
  for (int iter = 0; iter < fo.iterations; iter++) {
    double improvement = 0.0;
    for (int i = 0; i < ne;) {
      const int dim = rtype[i] == SGF_ELLIPTIC ? 3 : 1;
      double res[3], old[3], fn[3], A[9];
      for (int j = 0; j < dim; j++) {
        const double* s = sc + (size_t)(i + j) * SGF_SC;
        old[j] = fn[j] = f[i + j];
        res[j] = s[SGF_B] + s[SGF_R] * old[j] + sgf_wave_dot(J + (size_t)(i + j) * nv, acc, nv, lane);
        for (int c = 0; c < dim; c++) A[j * dim + c] = s[SGF_A + c];
      }
      if (dim == 1) fn[0] = sgf_pgs_scalar(rtype[i], res[0], A[0], fn[0]);
      else sgf_pgs_cone(A, res, sc + (size_t)i * SGF_SC + SGF_FRIC, fn);
      improvement -= sgf_cost_change(A, fn, old, res, dim);
      for (int j = 0; j < dim; j++) {
        const double df = fn[j] - old[j];
        f[i + j] = fn[j];
        if (df != 0.0) {
          const double* Wr = W + (size_t)(i + j) * nv;
          for (int c = lane; c < nv; c += 64) acc[c] += Wr[c] * df;
        }
      }
      i += dim;
    }
    iters = iter + 1;
    if (sgf_sweep_done(improvement, scale, tolerance)) break;
  }
  __syncthreads();
  // the outputs
  for (int c = lane; c < nv; c += 64) {
    double s = 0.0;
    for (int i = 0; i < ne; i++) s += J[(size_t)i * nv + c] * f[i];
    if (a.qfrc) a.qfrc[(size_t)k * nv + c] = s;
    if (a.qacc) a.qacc[(size_t)k * nv + c] = qs[c] + acc[c];
  }
  const int nw = ne < a.max_rows ? ne : a.max_rows;
  for (int i = lane; i < nw; i += 64) {
    const size_t at = (size_t)k * a.max_rows + i;
    if (a.efc_type) a.efc_type[at] = rtype[i];
    if (a.efc_id) a.efc_id[at] = rid[i];
    if (a.efc_force) a.efc_force[at] = f[i];
  }
  if (a.contact_force) {
    const int nc = ncon < a.max_contacts ? ncon : a.max_contacts;
    for (int c = lane; c < nc; c += 64) {
      const int at = a.caddr[(size_t)k * cap + c];
      double* out = a.contact_force + ((size_t)k * a.max_contacts + c) * 3;
      out[0] = at < 0 ? 0.0 : f[at];
      const bool cone = at >= 0 && rtype[at] == SGF_ELLIPTIC;
      out[1] = cone ? f[at + 1] : 0.0;
      out[2] = cone ? f[at + 2] : 0.0;
    }
  }
  if (lane == 0) {
    if (a.nefc) a.nefc[k] = ne;
    if (a.ncon) a.ncon[k] = ncon;
    if (a.iters) a.iters[k] = iters;
  }
}
