// The solve table and the per-lane functions of sg_solve_mass / sg_forward_smooth / sg_get_point_inertia (csrc/sg_solve.h: the text the
// kernel compiles) under AddressSanitizer and UBSan: a stand-alone program, nothing of it is loaded into python.
// tests/test_solve_host.py builds and runs it:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I soft-grip_amd/csrc scripts/sanitize/solve_main.cpp
// Dof trees: one dof, a serial chain, a fan under a chain (the free ball's shape), seeded random forests, and a chain past the LDS
// limit (refused).  Every array has exactly the size the functions may read, so one element past an end is a report.  On each tree a
// matrix M = L' D L of the tree's sparsity is packed, factorised in the kernel's order and solved: the factor must give L and D back
// and solve(M v) = v, both to 1e-9 of the largest value.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sg_readout_host.h"   // sgv_host_factor_levels, sgv_host_sweep: the kernel's order, stated once

static unsigned long long g_seed = 88172645463325252ull;
static double rnd() {   // xorshift, U(0, 1)
  g_seed ^= g_seed << 13; g_seed ^= g_seed >> 7; g_seed ^= g_seed << 17;
  return (double)(g_seed >> 11) / 9007199254740992.0;
}

static int run(const char* name, const std::vector<int>& dpar, bool expect_ok) {
  const int nv = (int)dpar.size(), nbody = nv + 1;
  std::vector<int> bpar(nbody, 0), dbody(nv);
  for (int i = 0; i < nv; i++) { dbody[i] = i + 1; bpar[i + 1] = dpar[i] < 0 ? 0 : dpar[i] + 1; }   // a body per dof
  SgSolveHost V;
  sgv_build(nbody, bpar.data(), nv, dbody.data(), dpar.data(), 0, &V);
  if (!V.ok) {
    printf("%-28s refused: %s\n", name, V.err.c_str());
    return expect_ok ? 1 : 0;
  }
  if (!expect_ok) { printf("%-28s accepted, but must be refused\n", name); return 1; }
  const SgSolveOff& v = V.o;
  V.ints = std::vector<int>(V.ints);   // (a fresh allocation of exactly the table's size: one element past its end is a report)
  const std::vector<int>& VI = V.ints;
  // L and D of the tree's sparsity, then the packed M = L' D L from the definition
  std::vector<double> Lp(v.nM), M(v.nM, 0.0);
  for (int e = 0; e < v.nM; e++) Lp[e] = VI[v.anc + e] == VI[v.erow + e] ? 0.5 + rnd() : rnd() - 0.5;   // slot 0: D
  for (int i = 0; i < nv; i++)
    for (int t = 0; t <= VI[v.depth + i]; t++) {
      const int j = VI[v.anc + VI[v.rstart + i] + t];
      double s = 0.0;
      for (int k = 0; k < nv; k++) {   // k = i or a descendant of i: L[k][i] D[k] L[k][j]
        const int up = VI[v.depth + k] - VI[v.depth + i];
        if (up < 0 || VI[v.anc + VI[v.rstart + k] + up] != i) continue;
        const double* row = Lp.data() + VI[v.rstart + k];
        s += (up ? row[up] : 1.0) * row[0] * (up + t ? row[up + t] : 1.0);
      }
      M[VI[v.rstart + i] + t] = s;
    }
  std::vector<double> F(M), mdiag(nv);
  for (int i = 0; i < nv; i++) mdiag[i] = M[VI[v.rstart + i]];
  sgv_host_factor_levels(V, F.data());
  double worst = 0.0, pivot = INFINITY;
  for (int e = 0; e < v.nM; e++) worst = fmax(worst, fabs(F[e] - Lp[e]));
  for (int i = 0; i < nv; i++) pivot = fmin(pivot, sgv_pivot_ratio(VI.data(), v, F.data(), mdiag.data(), i));
  // solve(M v) = v
  std::vector<double> want(nv), x(nv, 0.0);
  for (int i = 0; i < nv; i++) want[i] = rnd() - 0.5;
  for (int i = 0; i < nv; i++)
    for (int t = 0; t <= VI[v.depth + i]; t++) {
      const int j = VI[v.anc + VI[v.rstart + i] + t];
      x[i] += M[VI[v.rstart + i] + t] * want[j];
      if (t) x[j] += M[VI[v.rstart + i] + t] * want[i];
    }
  sgv_host_sweep(V, nv, F.data(), x.data());
  double werr = 0.0;
  for (int i = 0; i < nv; i++) werr = fmax(werr, fabs(x[i] - want[i]));
  // a point inertia's pairs on random twists: every body's chain, and the world's
  std::vector<double> S((size_t)SGS_DOF * nv), X(6 * (size_t)nv);
  for (double& s : S) s = rnd() - 0.5;
  for (double& s : X) s = rnd() - 0.5;
  const double P[3] = {0.1, -0.2, 0.3};
  double wsum = 0.0;
  for (int b = 0; b < nbody; b++)
    for (int c = 0; c < 6; c++)
      for (int a = 0; a <= c; a++) wsum += sgv_w_entry(VI.data(), v, S.data(), X.data(), nv, VI[v.bdof + b], P, a, c);
  printf("%-28s nv %4d  nM %6d  levels %4d  tile %5lld  |factor - L, D| %.1e  |solve(M v) - v| %.1e  pivot %.3f  (w %.3f)\n", name, nv, v.nM, v.nlevel,
         sgv_tile(nbody, nv, 0, v.nM), worst, werr, pivot, wsum);
  return !(worst <= 1e-9 && werr <= 1e-9 && pivot > 0.0);
}

int main() {
  int bad = 0;
  bad += run("one dof", {-1}, true);
  std::vector<int> chain(60), fan(224, 5), big(1024);
  for (int i = 0; i < 60; i++) chain[i] = i - 1;
  for (int i = 0; i < 6; i++) fan[i] = i - 1;   // six free dofs in a chain, 218 sliders under the last
  for (int i = 0; i < 1024; i++) big[i] = i - 1;
  bad += run("serial chain of 60", chain, true);
  bad += run("218-wide fan under a 6-chain", fan, true);
  for (int f = 0; f < 4; f++) {
    std::vector<int> forest(20 + 40 * f);
    for (int i = 0; i < (int)forest.size(); i++) forest[i] = i == 0 || rnd() < 0.1 * (f + 1) ? -1 : (int)(rnd() * i);   // a root, or any earlier dof
    char name[32];
    snprintf(name, sizeof name, "random forest %d", f);
    bad += run(name, forest, true);
  }
  bad += run("serial chain of 1024", big, false);
  printf(bad ? "FAILED\n" : "ok\n");
  return bad ? 1 : 0;
}
