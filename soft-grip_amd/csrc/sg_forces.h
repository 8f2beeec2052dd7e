// sg_forces.h -- the per-env arithmetic of the constraint-force read-out (sg_get_forces): mj_forward's constraint stage as the oracle
// restates it (make_constraint, project_constraint, the warm start of sgo_forward, sol_pgs), at the batch's CURRENT state.  Pure functions
// of their arguments, compiled for gfx950 (sg_forces_kernel.h, inside sg_readout.hip) and by g++ for the CPU tests (sg_forces_host.h,
// tests/forces_ref.py), which drive the same text row by row as the kernel's lanes run it.
//
// Kinematics, the factor of M with its sweeps and qacc_smooth are sg_smooth.h's and sg_solve.h's, the contact list is sg_contacts.h's, a
// contact's Jacobian column is sg_point.h's sgp_jac_col: reused, not restated.  What is here:
//   the forces table      equality records, limited joints, per-geom solver parameters, the three *_invweight0 arrays, opt's numbers
//   sgf_row_list          the row list in the oracle's order: equalities by id, limits by joint (lower side first, dist < margin),
//                         contacts in sg_get_contacts' order (dist < includemargin; 1 row for condim 1, 3 for condim 3), njmax's cut
//   sgf_row_j             entry (row, dof) of the DENSE Jacobian: a row is nv doubles, one column per dof, the common dofs of a
//                         contact's two chains merged in add_row's order (geom2's share, then minus geom1's)
//   sgf_row_params        pos, margin, diagApprox, solref, solimp of a row; sgf_impedance, sgf_kb, sgf_cone_r: mj_makeImpedance
//   sgf_warm_*            mj_constraintUpdate, the warm start's forces; sgf_warm_keep: its cost gate
//   sgf_pgs_scalar / sgf_pgs_cone / sgf_qcqp2 / sgf_cost_change   one PGS row update; sgf_sweep_done: the sweep's early exit
// A + R is never formed: a row's residual is b_i + R_i f_i + J_i . a with a = M^-1 J' f kept up to date by a += W_i df, W = M^-1 J'.
// Sums over the dofs of a row are taken as the wavefront takes them -- lane l adds the columns l, l + 64, .. in ascending order, the 64
// partial sums meet in a fixed butterfly (sgf_fold) -- so the result depends on nothing but the row.
#pragma once
#ifndef SG_FORCES_H   // (beside #pragma once: the host tests build from a patched COPY of this file, which sg_forces_host.h and sg_tables.cpp
#define SG_FORCES_H   // include first; sg_tables.h's include of the file in this directory must then add nothing)
#include "sg_solve.h"
#include "sg_point.h"

#define SGF_EQUALITY 0   // the oracle's type codes (sg_oracle.c)
#define SGF_LIMIT 3
#define SGF_FRICTIONLESS 5
#define SGF_ELLIPTIC 7
#define SGF_MINVAL 1e-15
#define SGF_MINIMP 1e-4
#define SGF_MAXIMP 0.9999
#define SGF_SC 8         // doubles of a row's scalar record (below)
// a row's scalar record in the work space: b, R, the force the solve starts from, the row's entries of the diagonal block of A + R
// (one for a scalar row, three for a row of a cone), the cone's two friction coefficients
enum { SGF_B = 0, SGF_R = 1, SGF_F0 = 2, SGF_A = 3, SGF_FRIC = 6 };
// The kernels' LDS: the rows kernel holds sg_smooth_kernel's records and the row directory (3 ints a row); the solver f (R doubles) and
// a (nv doubles); each beside SGF_STATIC_LDS bytes of static LDS
#define SGF_STATIC_LDS 1024
#define SGF_LDS_MAX 163840

// ---- the forces table: one double and one int array, sections at the offsets below ----
struct SgForceOff {
  int neq, nlim, cap, njmax, iterations, nrows;   // equalities, limited joints, contacts kept at most, opt's njmax and iterations, row capacity
  // doubles
  int eqdata, eqsolref, eqsolimp, tlen0, jrange, jmargin, jsolref, jsolimp, gfric, gsolref, gsolimp, gsolmix, ggap, gmargin, dofinvw, bodyinvw, teninvw, q0, opt;
  // ints
  int eqtype, eqobj1, eqobj2, limj, gcondim;
};

struct SgForceHost {
  bool ok = false;
  std::string err;
  SgForceOff o;
  std::vector<double> dbl;
  std::vector<int> ints;
};

// the table from the blob (the model's other tables index the same bodies, joints, dofs, geoms and tendons).  F->ok says whether
// sg_get_forces can run the model; a refusal names the limit
void sgf_build(const void* blob, size_t nbytes, const SgKinHost& K, const SgConHost& C, const SgDynHost& Dn, const SgSolveHost& V, SgForceHost* F);

// the rows the call reserves per env: every equality, both sides of every limited joint, three rows of every contact the list can hold;
// a positive njmax cuts the contacts' share as make_constraint cuts it
inline int sgf_row_capacity(int neq, int nlim, int cap, int njmax) {
  const int fixed = neq + 2 * nlim, all = fixed + 3 * cap;
  if (njmax > 0 && all > njmax) return fixed > njmax ? fixed : njmax;
  return all;
}
// doubles and ints of one env's slice of the work space: J and W (nrows x nv each), the scalar records, qacc_smooth, the contact list
// (dist, pos, frame; geoms), the row directory (type, id, aux) and the three counts (nefc, ncon, spare)
inline size_t sgf_env_doubles(const SgForceOff& f, int nv) { return 2 * (size_t)f.nrows * nv + (size_t)SGF_SC * f.nrows + nv + 13 * (size_t)f.cap; }
inline size_t sgf_env_ints(const SgForceOff& f) { return 3 * (size_t)f.nrows + 3 * (size_t)f.cap + 4; }
inline size_t sgf_env_bytes(const SgForceOff& f, int nv) { return 8 * sgf_env_doubles(f, nv) + 4 * sgf_env_ints(f); }

// ---- sums over the dofs, as the wavefront takes them ----
// the butterfly over the 64 lanes' partial sums: lane l meets lane l ^ 32, then ^ 16, .. ^ 1; p[0] ends as what every lane ends with
__host__ __device__ inline double sgf_fold(double* p) {
  for (int o = 32; o > 0; o >>= 1)
    for (int l = 0; l < o; l++) p[l] = p[l] + p[l + o];
  return p[0];
}
// lane `lane`'s share of x . y over n columns
__host__ __device__ inline double sgf_dot_lane(const double* x, const double* y, int n, int lane) {
  double p = 0.0;
  for (int c = lane; c < n; c += 64) p += x[c] * y[c];
  return p;
}
// x . y as the wavefront computes it (the host's form; the kernel's lanes call sgf_dot_lane and fold with __shfl_xor)
inline double sgf_dot(const double* x, const double* y, int n) {
  double p[64];
  for (int l = 0; l < 64; l++) p[l] = sgf_dot_lane(x, y, n, l);
  return sgf_fold(p);
}

// ---- the row list ----
// does dof `dof` move the body that enters the dof-parent chain at dof e0 (-1: the world)?
__host__ __device__ inline bool sgf_moves(const int* VI, const SgSolveOff& v, int e0, int dof) {
  if (e0 < 0) return false;
  const int up = VI[v.depth + e0] - VI[v.depth + dof];
  return up >= 0 && VI[v.anc + VI[v.rstart + e0] + up] == dof;
}

// the mixed parameters of a contact between geoms g1 and g2 (add_contact, equal priority): condim max, friction max, solref and solimp
// weighted by solmix, margin max - gap max.  fric[2]: the two tangential coefficients of an elliptic cone
__host__ __device__ inline void sgf_contact_params(const double* FD, const int* FI, const SgForceOff& f, int g1, int g2, int* dim, double* fric, double* solref,
                                                   double* solimp, double* includemargin) {
  const int d1 = FI[f.gcondim + g1], d2 = FI[f.gcondim + g2];
  *dim = d1 > d2 ? d1 : d2;
  const double *f1 = FD + f.gfric + 3 * g1, *f2 = FD + f.gfric + 3 * g2;
  fric[0] = fric[1] = f1[0] > f2[0] ? f1[0] : f2[0];
  double mix;
  const double s1 = FD[f.gsolmix + g1], s2 = FD[f.gsolmix + g2];
  if (s1 >= SGF_MINVAL && s2 >= SGF_MINVAL) mix = s1 / (s1 + s2);
  else if (s1 < SGF_MINVAL && s2 < SGF_MINVAL) mix = 0.5;
  else mix = s1 < SGF_MINVAL ? 0.0 : 1.0;
  const double *r1 = FD + f.gsolref + 2 * g1, *r2 = FD + f.gsolref + 2 * g2;
  if (r1[0] > 0 && r2[0] > 0)
    for (int k = 0; k < 2; k++) solref[k] = mix * r1[k] + (1 - mix) * r2[k];
  else
    for (int k = 0; k < 2; k++) solref[k] = r1[k] < r2[k] ? r1[k] : r2[k];
  for (int k = 0; k < 5; k++) solimp[k] = mix * FD[f.gsolimp + 5 * g1 + k] + (1 - mix) * FD[f.gsolimp + 5 * g2 + k];
  *includemargin = fmax(FD[f.gmargin + g1], FD[f.gmargin + g2]) - fmax(FD[f.ggap + g1], FD[f.ggap + g2]);
}

// the distance of limited joint j from the `side` end of its range (-1: the lower one, +1: the upper one)
__host__ __device__ inline double sgf_limit_dist(const double* FD, const SgForceOff& f, const int* I, const SgKinOff& o, const double* qpos, int j, int side) {
  return side * (FD[f.jrange + 2 * j + (side + 1) / 2] - qpos[I[o.jqadr + j]]);
}

// the row list of one env, serially in the oracle's order: rtype / rid / raux [nrows] (aux: a limit row's side, a contact row's index in
// its cone), caddr [ncon] a contact's first row or -1.  ncon, cgeom, cdist: sg_get_contacts' list.  Returns nefc (<= f.nrows)
__host__ __device__ inline int sgf_row_list(const double* FD, const int* FI, const SgForceOff& f, const int* I, const SgKinOff& o, const double* qpos, int ncon,
                                            const int* cgeom, const double* cdist, int* rtype, int* rid, int* raux, int* caddr) {
  int n = 0;
  for (int e = 0; e < f.neq; e++) { rtype[n] = SGF_EQUALITY; rid[n] = e; raux[n] = 0; n++; }
  for (int l = 0; l < f.nlim; l++) {
    const int j = FI[f.limj + l];
    for (int side = -1; side <= 1; side += 2)
      if (sgf_limit_dist(FD, f, I, o, qpos, j, side) < FD[f.jmargin + j]) { rtype[n] = SGF_LIMIT; rid[n] = j; raux[n] = side; n++; }
  }
  int c = 0;
  for (; c < ncon; c++) {
    int dim;
    double fric[2], solref[2], solimp[5], inc;
    sgf_contact_params(FD, FI, f, cgeom[2 * c], cgeom[2 * c + 1], &dim, fric, solref, solimp, &inc);
    caddr[c] = -1;
    if (cdist[c] >= inc) continue;
    if (f.njmax > 0 && n + dim > f.njmax) break;
    caddr[c] = n;
    for (int r = 0; r < dim; r++) { rtype[n] = dim == 1 ? SGF_FRICTIONLESS : SGF_ELLIPTIC; rid[n] = c; raux[n] = r; n++; }
  }
  for (; c < ncon; c++) caddr[c] = -1;
  return n;
}

// ---- the rows' Jacobian and parameters ----
// the length of tendon t, its shares summed serially in ascending order (sgs_wrap at a qvel of zeros: `zero`)
__host__ __device__ inline double sgf_tendon_length(const int* I, const SgKinOff& o, const double* DD, const int* DI, const SgDynOff& d, const double* qpos,
                                                    const double* zero, const double* recs, int t) {
  double L = 0.0;
  const int w0 = DI[d.tadr + t], n = sgd_nshare(DI, d, t);
  for (int s = 0; s < n; s++) {
    double l1, v1;
    sgs_wrap(I, o, DD, DI, d, qpos, zero, recs, w0 + s, &l1, &v1);
    L += l1;
  }
  return L;
}

// column `dof` of the translational Jacobian of world point P on the body entering the chain at e0, along the unit vector e (zero for a
// dof that does not move the body): sgp_jac_col's column.  The dof records' stamp slots hold zero
__host__ __device__ inline double sgf_point_j(const int* VI, const SgSolveOff& v, const double* S, int e0, const double* P, const double* e, int dof) {
  if (!sgf_moves(VI, v, e0, dof)) return 0.0;
  double jp[3], jr[3];
  sgp_jac_col(S + SGS_DOF * dof, 0.0, P, jp, jr);
  return e[0] * jp[0] + e[1] * jp[1] + e[2] * jp[2];
}

// entry `dof` of tendon t's Jacobian (tendons() of the oracle): a fixed tendon's coefficient at its joints' dofs; a spatial tendon's
// segments in ascending order, the far site's share added, the near site's subtracted, a segment shorter than 1e-15 skipped
__host__ __device__ inline double sgf_tendon_j(const int* VI, const SgSolveOff& v, const double* DD, const int* DI, const SgDynOff& d, const double* recs,
                                               const double* S, int t, int dof) {
  const int w0 = DI[d.tadr + t], n = DI[d.tnum + t];
  double val = 0.0;
  if (DI[d.wtype + w0] == SG_WRAP_JOINT) {
    for (int w = w0; w < w0 + n; w++)
      if (DI[d.jdof + DI[d.wobj + w]] == dof) val = DD[d.wprm + w];
    return val;
  }
  for (int w = w0; w < w0 + n - 1; w++) {
    const int s0 = DI[d.wobj + w], s1 = DI[d.wobj + w + 1], b0 = DI[d.sbody + s0], b1 = DI[d.sbody + s1];
    double p0[3], p1[3];
    sgp_pos(recs + SGS_REC * b0, DD + d.spos + 3 * s0, p0);
    sgp_pos(recs + SGS_REC * b1, DD + d.spos + 3 * s1, p1);
    double e[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};
    const double len = sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
    if (len < SGF_MINVAL) continue;
    for (int k = 0; k < 3; k++) e[k] /= len;
    val += sgf_point_j(VI, v, S, VI[v.bdof + b1], p1, e, dof);
    val -= sgf_point_j(VI, v, S, VI[v.bdof + b0], p0, e, dof);
  }
  return val;
}

// what the walk over the rows hands every row function: the tables, the env's state and records, its contact list
struct SgfEnv {
  const int* I; SgKinOff o;                        // kinematics (its int section; the walk that leaves recs and S reads the doubles)
  const double* DD; const int* DI; SgDynOff d;     // dynamics
  const int* VI; SgSolveOff v;                     // solve
  const double* FD; const int* FI; SgForceOff f;   // forces
  const double *qpos, *zero;
  const double *recs, *S;                          // [nbody][SGS_REC], [nv][SGS_DOF] with the stamp slots at zero
  const int* cgeom; const double *cdist, *cpos, *cframe;
};

// entry (row, dof) of the dense Jacobian.  type, id, aux: the row's entry of the list
__host__ __device__ inline double sgf_row_j(const SgfEnv& E, int type, int id, int aux, int dof) {
  if (type == SGF_EQUALITY) {
    if (E.FI[E.f.eqtype + id] != SG_EQ_JOINT) return sgf_tendon_j(E.VI, E.v, E.DD, E.DI, E.d, E.recs, E.S, E.FI[E.f.eqobj1 + id], dof);
    const int j = E.FI[E.f.eqobj1 + id], j2 = E.FI[E.f.eqobj2 + id];
    double val = 0.0;
    if (E.DI[E.d.jdof + j] == dof) val = 1.0;
    if (j2 >= 0 && E.DI[E.d.jdof + j2] == dof) {
      const double* pc = E.FD + E.f.eqdata + 5 * id;
      const int q2 = E.I[E.o.jqadr + j2];
      const double dif = E.qpos[q2] - E.FD[E.f.q0 + q2];
      const double der = pc[1] + dif * (2 * pc[2] + dif * (3 * pc[3] + dif * 4 * pc[4]));
      val += -der;
    }
    return val;
  }
  if (type == SGF_LIMIT) return E.DI[E.d.jdof + id] == dof ? (double)-aux : 0.0;
  const double *P = E.cpos + 3 * id, *e = E.cframe + 9 * id + 3 * aux;
  const int b1 = E.I[E.o.gbody + E.cgeom[2 * id]], b2 = E.I[E.o.gbody + E.cgeom[2 * id + 1]];
  double val = sgf_point_j(E.VI, E.v, E.S, E.VI[E.v.bdof + b2], P, e, dof);
  val += -sgf_point_j(E.VI, E.v, E.S, E.VI[E.v.bdof + b1], P, e, dof);
  return val;
}

// a row's pos, margin, diagApprox, solref[2] and solimp[5] (make_constraint)
__host__ __device__ inline void sgf_row_params(const SgfEnv& E, int type, int id, int aux, double* pos, double* margin, double* dA, double* solref, double* solimp) {
  const SgForceOff& f = E.f;
  *margin = 0.0;
  if (type == SGF_EQUALITY) {
    const int j = E.FI[f.eqobj1 + id], j2 = E.FI[f.eqobj2 + id];
    const double* pc = E.FD + f.eqdata + 5 * id;
    if (E.FI[f.eqtype + id] == SG_EQ_JOINT) {
      const int q1 = E.I[E.o.jqadr + j];
      if (j2 < 0) {
        *pos = E.qpos[q1] - E.FD[f.q0 + q1] - pc[0];
        *dA = E.FD[f.dofinvw + E.DI[E.d.jdof + j]] + 0.0;
      } else {
        const int q2 = E.I[E.o.jqadr + j2];
        const double dif = E.qpos[q2] - E.FD[f.q0 + q2];
        const double poly = pc[0] + dif * (pc[1] + dif * (pc[2] + dif * (pc[3] + dif * pc[4])));
        *pos = E.qpos[q1] - E.FD[f.q0 + q1] - poly;
        *dA = E.FD[f.dofinvw + E.DI[E.d.jdof + j]] + E.FD[f.dofinvw + E.DI[E.d.jdof + j2]];
      }
    } else {
      *pos = sgf_tendon_length(E.I, E.o, E.DD, E.DI, E.d, E.qpos, E.zero, E.recs, j) - E.FD[f.tlen0 + j] - pc[0];
      *dA = E.FD[f.teninvw + j];
    }
    for (int k = 0; k < 2; k++) solref[k] = E.FD[f.eqsolref + 2 * id + k];
    for (int k = 0; k < 5; k++) solimp[k] = E.FD[f.eqsolimp + 5 * id + k];
    return;
  }
  if (type == SGF_LIMIT) {
    *pos = sgf_limit_dist(E.FD, f, E.I, E.o, E.qpos, id, aux);
    *margin = E.FD[f.jmargin + id];
    *dA = E.FD[f.dofinvw + E.DI[E.d.jdof + id]];
    for (int k = 0; k < 2; k++) solref[k] = E.FD[f.jsolref + 2 * id + k];
    for (int k = 0; k < 5; k++) solimp[k] = E.FD[f.jsolimp + 5 * id + k];
    return;
  }
  int dim;
  double fric[2], inc;
  const int g1 = E.cgeom[2 * id], g2 = E.cgeom[2 * id + 1];
  sgf_contact_params(E.FD, E.FI, f, g1, g2, &dim, fric, solref, solimp, &inc);
  *pos = aux == 0 ? E.cdist[id] : 0.0;
  *margin = aux == 0 ? inc : 0.0;
  *dA = E.FD[f.bodyinvw + E.I[E.o.gbody + g1]] + E.FD[f.bodyinvw + E.I[E.o.gbody + g2]];
}

// the impedance d(pos - margin) of mj_makeImpedance
__host__ __device__ inline double sgf_impedance(const double* solimp, double pos, double margin) {
  double s[5];
  s[0] = fmin(SGF_MAXIMP, fmax(SGF_MINIMP, solimp[0])); s[1] = fmin(SGF_MAXIMP, fmax(SGF_MINIMP, solimp[1]));
  s[2] = fmax(0.0, solimp[2]); s[3] = fmin(SGF_MAXIMP, fmax(SGF_MINIMP, solimp[3])); s[4] = fmax(1.0, solimp[4]);
  if (s[0] == s[1] || s[2] <= SGF_MINVAL) return 0.5 * (s[0] + s[1]);
  const double x = fabs((pos - margin) / s[2]);
  if (x >= 1 || x <= 0) return x >= 1 ? s[1] : s[0];
  double y;
  if (s[4] == 1) y = x;
  else if (x <= s[3]) y = pow(x, s[4]) / pow(s[3], s[4] - 1);
  else y = 1 - pow(1 - x, s[4]) / pow(1 - s[3], s[4] - 1);
  return s[0] + y * (s[1] - s[0]);
}

// a row's own R = max(1e-15, (1 - d) / d diagApprox) and the stiffness and damping of its reference acceleration: (timeconst, dampratio)
// with timeconst >= 2 timestep (refsafe), or the direct (-stiffness, -damping) form
__host__ __device__ inline void sgf_kb(const double* solref, const double* solimp, double imp, double dA, double timestep, double* R, double* K, double* B) {
  const double dmax = fmin(SGF_MAXIMP, fmax(SGF_MINIMP, solimp[1]));
  *R = fmax(SGF_MINVAL, (1 - imp) / imp * dA);
  if (solref[0] > 0 && solref[1] > 0) {
    const double tc = fmax(solref[0], 2 * timestep);
    *K = 1 / fmax(SGF_MINVAL, dmax * dmax * tc * tc * solref[1] * solref[1]);
    *B = 2 / fmax(SGF_MINVAL, dmax * tc);
  } else {
    *K = -solref[0] / fmax(SGF_MINVAL, dmax * dmax);
    *B = -solref[1] / fmax(SGF_MINVAL, dmax);
  }
}
// the reference acceleration of a row with velocity vel
__host__ __device__ inline double sgf_aref(double K, double B, double imp, double pos, double margin, double vel) { return -B * vel - K * imp * (pos - margin); }

// an elliptic cone's friction rows: R[1], R[2] from the normal row's R[0] through impratio, and the regularised mu
__host__ __device__ inline double sgf_cone_r(double impratio, const double* fric, double* R) {
  R[1] = R[0] / fmax(SGF_MINVAL, impratio);
  R[2] = R[1] * fric[0] * fric[0] / (fric[1] * fric[1]);
  return fric[0] * sqrt(R[1] / R[0]);
}

// ---- the warm start (mj_constraintUpdate on jar = J qacc_warmstart - aref) ----
__host__ __device__ inline double sgf_warm_scalar(int type, double D, double jar) {
  if (type == SGF_EQUALITY) return -D * jar;
  return jar < 0 ? -D * jar : 0.0;
}
__host__ __device__ inline void sgf_warm_cone(double mu, const double* fric, const double* D, const double* jar, double* f) {
  const double U[3] = {jar[0] * mu, jar[1] * fric[0], jar[2] * fric[1]};
  const double N = U[0], T = sqrt(U[1] * U[1] + U[2] * U[2]);
  if (N >= mu * T || (T <= 0 && N >= 0)) { f[0] = f[1] = f[2] = 0.0; return; }
  if (mu * N + T <= 0 || (T <= 0 && N < 0)) {
    for (int j = 0; j < 3; j++) f[j] = -D[j] * jar[j];
    return;
  }
  const double Dm = D[0] / (mu * mu * (1 + mu * mu)), NmT = N - mu * T;
  f[0] = -Dm * NmT * mu;
  f[1] = -f[0] / T * U[1] * fric[0];
  f[2] = -f[0] / T * U[2] * fric[1];
}
// row i's share of the warm start's cost, f_i (1/2 ((A + R) f)_i + b_i), with ((A + R) f)_i = R_i f_i + J_i . a
__host__ __device__ inline double sgf_warm_cost(double f, double R, double ja, double b) { return f * (0.5 * (R * f + ja) + b); }
// the cost gate: the warm start is kept only if it beats f = 0
__host__ __device__ inline bool sgf_warm_keep(double cost) { return !(cost > 0.0); }

// ---- one PGS row update (sol_pgs) ----
__host__ __device__ inline double sgf_pgs_scalar(int type, double res, double A, double f) {
  f -= res / A;
  if (type != SGF_EQUALITY && f < 0) f = 0.0;
  return f;
}

__host__ __device__ inline int sgf_qcqp2(double* res, const double* Ain, const double* bin, const double* dd, double r) {
  const double b1 = bin[0] * dd[0], b2 = bin[1] * dd[1];
  const double A11 = Ain[0] * dd[0] * dd[0], A22 = Ain[3] * dd[1] * dd[1], A12 = Ain[1] * dd[0] * dd[1];
  double la = 0, v1 = 0, v2 = 0;
  for (int it = 0; it < 20; it++) {
    const double det = (A11 + la) * (A22 + la) - A12 * A12;
    if (det < 1e-10) { res[0] = res[1] = 0; return 0; }
    const double di = 1 / det, P11 = (A22 + la) * di, P22 = (A11 + la) * di, P12 = -A12 * di;
    v1 = -P11 * b1 - P12 * b2; v2 = -P12 * b1 - P22 * b2;
    const double val = v1 * v1 + v2 * v2 - r * r;
    if (val < 1e-10) break;
    const double deriv = -2 * (P11 * v1 * v1 + 2 * P12 * v1 * v2 + P22 * v2 * v2), delta = -val / deriv;
    if (delta < 1e-10) break;
    la += delta;
  }
  res[0] = v1 * dd[0]; res[1] = v2 * dd[1];
  return la != 0;
}

// the three rows of an elliptic cone in one pass: A[9] the diagonal block of A + R, res[3] the residuals, f[3] updated in place
__host__ __device__ inline void sgf_pgs_cone(const double* A, const double* res, const double* fric, double* f) {
  const double old[3] = {f[0], f[1], f[2]};
  if (f[0] < SGF_MINVAL) {   // normal update
    f[0] -= res[0] / A[0];
    if (f[0] < 0) f[0] = 0.0;
    f[1] = f[2] = 0.0;
  } else {                   // ray update
    const double v[3] = {f[0], f[1], f[2]};
    double v1[3], denom = 0;
    for (int j = 0; j < 3; j++) { v1[j] = A[3 * j] * v[0] + A[3 * j + 1] * v[1] + A[3 * j + 2] * v[2]; denom += v[j] * v1[j]; }
    if (denom >= SGF_MINVAL) {
      double x = -(v[0] * res[0] + v[1] * res[1] + v[2] * res[2]) / denom;
      if (f[0] + x * v[0] < 0) x = -f[0] / v[0];
      for (int j = 0; j < 3; j++) f[j] += x * v[j];
    }
  }
  if (f[0] < SGF_MINVAL) {   // friction update with the normal force fixed
    f[1] = f[2] = 0.0;
  } else {
    const double Ac[4] = {A[4], A[5], A[7], A[8]};
    double bc[2], v[2];
    for (int j = 0; j < 2; j++) {
      bc[j] = res[j + 1];
      for (int k = 0; k < 2; k++) bc[j] -= Ac[2 * j + k] * old[1 + k];
      bc[j] += A[3 * (j + 1)] * (f[0] - old[0]);
    }
    if (sgf_qcqp2(v, Ac, bc, fric, f[0])) {
      double s = v[0] * v[0] / (fric[0] * fric[0]) + v[1] * v[1] / (fric[1] * fric[1]);
      s = sqrt(f[0] * f[0] / fmax(SGF_MINVAL, s));
      v[0] *= s; v[1] *= s;
    }
    f[1] = v[0]; f[2] = v[1];
  }
}

// the change of the cost under the update old -> f of dim rows; an update that raises it by more than 1e-10 is taken back
__host__ __device__ inline double sgf_cost_change(const double* A, double* f, const double* old, const double* res, int dim) {
  double delta[3], change = 0;
  for (int j = 0; j < dim; j++) delta[j] = f[j] - old[j];
  for (int j = 0; j < dim; j++) {
    double s = 0;
    for (int k = 0; k < dim; k++) s += A[j * dim + k] * delta[k];
    change += 0.5 * delta[j] * s + delta[j] * res[j];
  }
  if (change > 1e-10) { for (int j = 0; j < dim; j++) f[j] = old[j]; change = 0; }
  return change;
}

// the sweep's early exit: the scaled improvement of a whole sweep below the tolerance
__host__ __device__ inline double sgf_scale(double meaninertia, int nv) { return 1 / (meaninertia * (nv > 1 ? nv : 1)); }
__host__ __device__ inline bool sgf_sweep_done(double improvement, double scale, double tolerance) { return improvement * scale < tolerance; }
#endif   // SG_FORCES_H
