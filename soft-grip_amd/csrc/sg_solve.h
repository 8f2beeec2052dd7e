// sg_solve.h -- the per-env arithmetic of the read-outs that start with the inverse of the mass matrix (sg_solve_mass, sg_forward_smooth,
// sg_get_point_inertia): the solve table beside the smooth table, and what one lane does for one packed entry of M, one entry of its
// factor, one dof of a sweep.  Pure functions of their arguments, compiled for gfx950 (sg_solve_kernel.h, inside sg_readout.hip) and by
// g++ for the CPU tests (tests/solve_ref.py), which drive the same text entry by entry and dof by dof through sgv_host_env (sg_readout_host.h).
//
// Definitions.  M is sg_smooth.h's: entry (i, j) is nonzero only where dof j is dof i or one of its ancestors on the dof-parent chain
// (SgSmoothOff::dpar), so M is kept PACKED, row by row: row i holds depth(i) + 1 doubles, slot 0 the diagonal, slot t the entry with
// the t-th ancestor, nearest first.  nM is the number of packed entries.  The factor is mj_factorM's, M = L' D L with L unit lower
// triangular and L[k][j] != 0 only where j is an ancestor of k; it overwrites the packed M in place: slot 0 of row k becomes D[k], slot t
// becomes L[k][ancestor t].  No pivoting and no clamping of small pivots.
// Every elimination is a GATHER: an entry (i, j) of the factor takes M[i][j] - sum over the descendants k of i, ascending, of
// L[k][i] D[k] L[k][j], all of them rows of deeper levels and final by then; a dof of the up sweep takes its descendants' x, a dof of the
// down sweep its ancestors'.  Who owns a value and in which order it is summed is fixed by the table: no atomics, and a right-hand side
// is one lane's work per dof, so its bits depend on nothing beside it.
#pragma once
#include <algorithm>

#include "sg_smooth.h"

// The kernel's LDS block: sg_smooth_kernel's records (nbody x 29, nv x 7 and two doubles per tendon), the packed factor and M's diagonal
// (nM + nv doubles) and a tile of right-hand sides, nv doubles each, beside its static LDS (SGV_STATIC_LDS bytes: the block-wide
// __syncthreads_or; the kept assembly's figure, held by tests/test_solve_host.py).  A model runs when a tile of SGV_MINRHS right-hand
// sides -- one point of sg_get_point_inertia -- fits the 160 KB a gfx950 workgroup gets when the launch asks for it.
#define SGV_STATIC_LDS 256
#define SGV_LDS_MAX 163840
#define SGV_MINRHS 6

// ---- the solve table: one int array, sections at the offsets below ----
struct SgSolveOff {
  int nM, nlevel;   // packed entries; depth levels of the dofs
  int depth;        // [nv] ancestors of the dof on the dof-parent chain
  int rstart;       // [nv + 1] where dof i's row starts in the packed factor
  int anc;          // [nM] the column of every packed entry: slot t of row i is i's t-th ancestor (t = 0: i itself)
  int erow;         // [nM] the row of every packed entry
  int lstart, ldof;     // [nlevel + 1], [nv] the level schedule: the dofs of depth L, ascending
  int elstart, eidx;    // [nlevel + 1], [nM] the packed entries of the rows of depth L
  int dstart, desc;     // [nv + 1], [nM - nv] every dof's descendants, ascending
  int doff, drow;       // [nM - nv] beside desc: for descendant k of dof i where L[k][i] and where D[k] sit in the packed factor, so a
                        // gather's next address never waits for a table entry that depends on the one before
  int bdof;         // [nbody] where a body enters the dof-parent chain: the last dof of the nearest ancestor-or-self that has dofs, else -1
};

struct SgSolveHost {
  bool ok = false;
  std::string err;
  SgSolveOff o;
  std::vector<int> ints;
};

// the doubles of the LDS block that do not depend on the call, and the right-hand sides a tile can hold beside them (<= 0: none)
inline long long sgv_fixed_doubles(long long nbody, long long nv, long long ntendon, long long nM) {
  return SGS_REC * nbody + SGS_DOF * nv + 2 * ntendon + nM + nv;
}
inline long long sgv_tile(long long nbody, long long nv, long long ntendon, long long nM) {
  return (SGV_LDS_MAX - SGV_STATIC_LDS - 8 * sgv_fixed_doubles(nbody, nv, ntendon, nM)) / (8 * (nv > 0 ? nv : 1));
}

// the table from the dof-parent chain (dpar [nv], parents before children) and the dofs' bodies (dbody [nv]; bpar [nbody] the bodies'
// parents).  V->ok says whether the three read-outs can run the model; the size check comes before anything of size nM is built
inline void sgv_build(int nbody, const int* bpar, int nv, const int* dbody, const int* dpar, int ntendon, SgSolveHost* V) {
  V->ok = false;
  V->ints.clear();
  if (nv < 1) { V->err = "a model without dofs"; return; }
  std::vector<int> depth(nv), rstart(nv + 1, 0);
  long long nM = 0;
  int nlevel = 0;
  for (int i = 0; i < nv; i++) {
    if (dpar[i] >= i || dpar[i] < -1) { V->err = "dof parents must precede their children"; return; }
    depth[i] = dpar[i] < 0 ? 0 : depth[dpar[i]] + 1;
    nlevel = std::max(nlevel, depth[i] + 1);
    nM += depth[i] + 1;
  }
  if (sgv_tile(nbody, nv, ntendon, nM) < SGV_MINRHS) {
    V->err = "the factor of the mass matrix (" + std::to_string(nM) + " entries) and " + std::to_string(SGV_MINRHS) +
             " right-hand sides do not fit the " + std::to_string(SGV_LDS_MAX / 1024) + " KB of LDS";
    return;
  }
  for (int i = 0; i < nv; i++) rstart[i + 1] = rstart[i] + depth[i] + 1;
  std::vector<int> anc(nM), erow(nM), dcount(nv, 0);
  for (int i = 0; i < nv; i++) {
    int j = i;
    for (int t = 0; t <= depth[i]; t++, j = dpar[j]) {
      anc[rstart[i] + t] = j;
      erow[rstart[i] + t] = i;
      if (t) dcount[j]++;
    }
  }
  std::vector<int> lstart(nlevel + 1, 0), ldof, elstart(nlevel + 1, 0), eidx;
  for (int L = 0; L < nlevel; L++) {
    lstart[L] = (int)ldof.size();
    elstart[L] = (int)eidx.size();
    for (int i = 0; i < nv; i++)
      if (depth[i] == L) {
        ldof.push_back(i);
        for (int t = 0; t <= L; t++) eidx.push_back(rstart[i] + t);
      }
  }
  lstart[nlevel] = (int)ldof.size();
  elstart[nlevel] = (int)eidx.size();
  std::vector<int> dstart(nv + 1, 0), desc(nM - nv), doff(nM - nv), drow(nM - nv), fill(nv);
  for (int i = 0; i < nv; i++) dstart[i + 1] = dstart[i] + dcount[i];
  for (int i = 0; i < nv; i++) fill[i] = dstart[i];
  for (int k = 0; k < nv; k++)   // (k ascending: every list comes out ascending)
    for (int t = 1; t <= depth[k]; t++) {
      const int at = fill[anc[rstart[k] + t]]++;
      desc[at] = k; doff[at] = rstart[k] + t; drow[at] = rstart[k];
    }
  std::vector<int> bdof(nbody, -1);
  for (int i = 0; i < nv; i++)
    if (dbody[i] < 0 || dbody[i] >= nbody) { V->err = "dof body out of range"; return; }
  for (int b = 1; b < nbody; b++) {
    if (bpar[b] < 0 || bpar[b] >= b) { V->err = "body parents must precede their children"; return; }
    bdof[b] = bdof[bpar[b]];
    for (int i = 0; i < nv; i++)
      if (dbody[i] == b) bdof[b] = i;
  }
  SgSolveOff& o = V->o;
  o.nM = (int)nM; o.nlevel = nlevel;
  std::vector<int>& I = V->ints;
  o.depth = sg_put(I, depth); o.rstart = sg_put(I, rstart); o.anc = sg_put(I, anc); o.erow = sg_put(I, erow); o.lstart = sg_put(I, lstart);
  o.ldof = sg_put(I, ldof); o.elstart = sg_put(I, elstart); o.eidx = sg_put(I, eidx); o.dstart = sg_put(I, dstart); o.desc = sg_put(I, desc);
  o.doff = sg_put(I, doff); o.drow = sg_put(I, drow); o.bdof = sg_put(I, bdof);
  V->ok = true;
}

// the table of a model (K, Dn, Sm: its kinematics, dynamics and smooth tables): a model sg_get_mass_matrix cannot run is refused with
// that read-out's reason
inline void sgv_build(const SgKinHost& K, const SgDynHost& Dn, const SgSmoothHost& Sm, SgSolveHost* V) {
  if (!K.ok) { V->err = K.err; return; }
  if (!Sm.ok) { V->err = Sm.err; return; }
  sgv_build(K.o.nbody, K.ints.data() + K.o.bpar, Dn.o.nv, Sm.ints.data() + Sm.o.dbody, Sm.ints.data() + Sm.o.dpar, Dn.o.ntendon, V);
}

// where dof i's descendant list ends
__host__ __device__ inline int sgv_desc_end(const int* VI, const SgSolveOff& v, int i) { return VI[v.dstart + i + 1]; }

// packed entry e of M, sgs_mass_row's arithmetic: the twist of the entry's column on the momentum that the composite inertia of the
// row's body has under the row's twist, plus the armature on the diagonal
__host__ __device__ inline double sgv_mass_entry(const int* VI, const SgSolveOff& v, const int* SI, const SgSmoothOff& s, const double* DD, const SgDynOff& d,
                                                 const double* recs, const double* S, int e) {
  const int i = VI[v.erow + e], j = VI[v.anc + e];
  double F[6];
  sgs_momentum(recs + SGS_REC * SI[s.dbody + i] + SGS_INR, S + SGS_DOF * i, F);
  double val = sgs_project(S + SGS_DOF * j, F);
  if (j == i) val += DD[d.arm + i];
  return val;
}

// packed entry e = (i, j) of the factor before its scaling: M[i][j] - sum over the descendants k of i, ascending, of L[k][i] D[k] L[k][j].
// F holds M in the rows of i's level and above and the finished factor in the deeper ones
__host__ __device__ inline double sgv_factor_entry(const int* VI, const SgSolveOff& v, const double* F, int e) {
  const int i = VI[v.erow + e], j = VI[v.anc + e];
  const int up = VI[v.depth + i] - VI[v.depth + j];   // L[k][j] sits that many slots behind L[k][i]
  double val = F[e];
  for (int c = VI[v.dstart + i]; c < sgv_desc_end(VI, v, i); c++) {
    const int at = VI[v.doff + c];
    val -= F[at] * F[VI[v.drow + c]] * F[at + up];
  }
  return val;
}

// the scaling of packed entry e = (i, j), j an ancestor of i, once row i's diagonal holds D[i]: L[i][j] = entry / D[i]
__host__ __device__ inline double sgv_factor_scale(const int* VI, const SgSolveOff& v, const double* F, int e) { return F[e] / F[VI[v.rstart + VI[v.erow + e]]]; }

// dof i's share of the pivot figure: D[i] / M[i][i]
__host__ __device__ inline double sgv_pivot_ratio(const int* VI, const SgSolveOff& v, const double* F, const double* mdiag, int i) {
  return F[VI[v.rstart + i]] / mdiag[i];
}

// ---- x = L^-1 D^-1 L^-T y on one right-hand side x[nv], in place ----
// up sweep, levels from the deepest: dof j loses its descendants' L[k][j] x[k], ascending; their x is final
__host__ __device__ inline double sgv_up(const int* VI, const SgSolveOff& v, const double* F, const double* x, int j) {
  double acc = x[j];
  for (int c = VI[v.dstart + j]; c < sgv_desc_end(VI, v, j); c++) acc -= F[VI[v.doff + c]] * x[VI[v.desc + c]];
  return acc;
}

// the scaling of dof i
__host__ __device__ inline double sgv_scale(const int* VI, const SgSolveOff& v, const double* F, const double* x, int i) { return x[i] / F[VI[v.rstart + i]]; }

// down sweep, levels from the roots: dof i loses its ancestors' L[i][j] x[j], nearest first; their x is final
__host__ __device__ inline double sgv_down(const int* VI, const SgSolveOff& v, const double* F, const double* x, int i) {
  const int r = VI[v.rstart + i], n = VI[v.depth + i];
  double acc = x[i];
  for (int t = 1; t <= n; t++) acc -= F[r + t] * x[VI[v.anc + r + t]];
  return acc;
}

// ---- the point inertia W = J M^-1 J' ----
// column d of the 6 x nv Jacobian of the world point P for a dof that moves the point's body: (jacr, jacp) = (u, lin + u x P),
// sgp_jac_col's arithmetic in sg_get_point_motion's angular-then-linear order
__host__ __device__ inline void sgv_jcol(const double* Sd, const double* P, double* c6) {
  double c[3];
  sgd_cross(c, Sd, P);
  for (int k = 0; k < 3; k++) { c6[k] = Sd[k]; c6[3 + k] = Sd[3 + k] + c[k]; }
}

// W[a][b] of the point P whose body enters the dof-parent chain at dof e0 (-1: the world, all zeros): row a of J on the solved column
// X[b] = M^-1 J[b]' (X: six right-hand sides of nv doubles), summed over the chain from e0 up, nearest first
__host__ __device__ inline double sgv_w_entry(const int* VI, const SgSolveOff& v, const double* S, const double* X, int nv, int e0, const double* P, int a, int b) {
  double w = 0.0;
  if (e0 < 0) return w;
  const int r = VI[v.rstart + e0], n = VI[v.depth + e0];
  for (int t = 0; t <= n; t++) {
    const int dof = VI[v.anc + r + t];
    double c6[6];
    sgv_jcol(S + SGS_DOF * dof, P, c6);
    w += c6[a] * X[(size_t)b * nv + dof];
  }
  return w;
}
