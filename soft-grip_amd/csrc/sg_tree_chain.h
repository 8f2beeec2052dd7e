// sg_tree_chain.h -- small dense math of the tree pipeline (part of sg_tree.h): a serial chain's L'DL and its solves, the scalar row
// update, the free object's 6 x 6 block.
#pragma once

namespace sgt {

// solve (L'DL) x = x for one chain block (MuJoCo's mj_solveLD on a serial chain: dof_parentid[k] = k - 1); Lc: nd x nd, row-major,
// L[k][i] (i < k) below the diagonal, D on it
SG_HD void chain_solve(const double* Lc, int nd, double* x) {
  for (int k = nd - 1; k >= 1; k--) {
    const double xk = x[k];
    for (int i = k - 1; i >= 0; i--) x[i] -= Lc[k * nd + i] * xk;
  }
  for (int k = 0; k < nd; k++) x[k] /= Lc[k * nd + k];
  for (int k = 1; k < nd; k++) {
    double s = x[k];
    for (int i = k - 1; i >= 0; i--) s -= Lc[k * nd + i] * x[i];
    x[k] = s;
  }
}
// the same solve with x in registers: fully unrolled over the SGT_CHD capacity, guarded by nd (LDS reads of L only, no dependent
// read-modify-write chain through LDS: 9 k instead of 100 k cycles for the M^-1 columns).  Same operations in the same order.
// Lc: a padded block [P][P] (identity beyond the chain's dofs), xmem: a padded vector [P]; P is the same on every lane, so the guards
// are scalar branches around straight-line blocks
template <int CHD>
SG_HD void chain_solve_reg(const double* Lc, int P, double* xmem) {
  double x[CHD];
#pragma unroll
  for (int k = 0; k < CHD; k += 4)
    if (k < P) { x[k] = xmem[k]; x[k + 1] = xmem[k + 1]; x[k + 2] = xmem[k + 2]; x[k + 3] = xmem[k + 3]; }
#pragma unroll
  for (int k = CHD - 1; k >= 1; k--)
    if (k < P) {
      const double xk = x[k];
#pragma unroll
      for (int i = k - 1; i >= 0; i--) x[i] -= Lc[k * P + i] * xk;
    }
#pragma unroll
  for (int k = 0; k < CHD; k += 4)
    if (k < P) { x[k] /= Lc[k * P + k]; x[k + 1] /= Lc[(k + 1) * P + k + 1]; x[k + 2] /= Lc[(k + 2) * P + k + 2]; x[k + 3] /= Lc[(k + 3) * P + k + 3]; }
#pragma unroll
  for (int k = 1; k < CHD; k++)
    if (k < P) {
      double s = x[k];
#pragma unroll
      for (int i = k - 1; i >= 0; i--) s -= Lc[k * P + i] * x[i];
      x[k] = s;
    }
#pragma unroll
  for (int k = 0; k < CHD; k += 4)
    if (k < P) { xmem[k] = x[k]; xmem[k + 1] = x[k + 1]; xmem[k + 2] = x[k + 2]; xmem[k + 3] = x[k + 3]; }
}
// scalar row update with the reciprocal of the row's diagonal A + R precomputed (as the fast kernels' equality rows)
SG_HD double scalar_update_rcp(double& f, double b, double Ja, double R, double Adiag, double Ainv, bool inequality) {
  const double res = b + Ja + R * f, old = f;
  double fn = f - res * Ainv;
  if (inequality && fn < 0) fn = 0;
  const double d = fn - old;
  double change = 0.5 * d * d * Adiag + d * res;
  if (change > 1e-10) { fn = old; change = 0; }
  f = fn;
  return change;
}
// inverse of a symmetric positive definite 6 x 6 matrix (Gauss-Jordan without pivoting: the free object's Schur complement)
SG_HD_HEAVY void spd_inverse6(const double* Sm, double* Si) {
  double a[6][12];
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < 6; j++) { a[i][j] = Sm[6 * i + j]; a[i][6 + j] = i == j ? 1.0 : 0.0; }
  for (int k = 0; k < 6; k++) {
    const double pv = 1.0 / a[k][k];
    for (int j = 0; j < 12; j++) a[k][j] *= pv;
    for (int i = 0; i < 6; i++) {
      if (i == k) continue;
      const double f = a[i][k];
      for (int j = 0; j < 12; j++) a[i][j] -= f * a[k][j];
    }
  }
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < 6; j++) Si[6 * i + j] = a[i][6 + j];
}
SG_HD double dot6(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3] + a[4] * b[4] + a[5] * b[5]; }
SG_HD void mat6vec(double* r, const double* M, const double* v) {
  for (int i = 0; i < 6; i++) r[i] = dot6(M + 6 * i, v);
}
// in-place L'DL of a chain block (mj_factorM restricted to a serial chain)
SG_HD void chain_factor(double* Lc, int nd) {
  for (int k = nd - 1; k >= 1; k--) {
    const double dk = Lc[k * nd + k];
    for (int i = k - 1; i >= 0; i--) {
      const double a = Lc[k * nd + i] / dk;
      for (int j = i; j >= 0; j--) Lc[i * nd + j] -= a * Lc[k * nd + j];
      Lc[k * nd + i] = a;
    }
  }
}

}  // namespace sgt
