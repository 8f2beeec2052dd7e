// The row builder and a full solve of sg_get_forces (csrc/sg_forces.h through csrc/sg_forces_host.h, and through it the smooth walk, the
// factor and the sweep of csrc/sg_readout_host.h: the text the kernels compile) under
// AddressSanitizer and UBSan: a stand-alone program, nothing of it is loaded into python.  tests/test_forces_host.py builds and runs it:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I soft-grip_amd/csrc scripts/sanitize/forces_main.cpp
//       soft-grip_amd/csrc/sg_tables.cpp
//   usage: forces_main BLOB STATE ...     pairs of files: a model blob, and a state of nq + 2 nv + nu + 1 doubles -- qpos, qvel,
//                                         qacc_warmstart, act (one double where nu = 0), the stiffness k of every joint and tendon listed
// The test hands it mini_gripper a squeeze in (equalities, limits, elliptic contacts) and a one-dof slider pushed past its range (one
// limit row).  Every vector has exactly the size the functions may read.  Per model one line: rows, contacts, sweeps, the largest force
// and the largest residual b + R f + J . a left on an equality row beside the largest |b|.
#include <cmath>
#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "sg_forces_host.h"

static std::string slurp(const char* path) {
  std::ifstream f(path, std::ios::binary);
  return std::string(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

static int run(const char* blob_path, const char* state_path) {
  const std::string blob = slurp(blob_path), raw = slurp(state_path);
  SgHostTables T;
  sg_host_tables(blob.data(), blob.size(), &T);
  const SgKinHost& K = T.kin;
  const SgDynHost& D = T.dyn;
  const SgSmoothHost& S = T.smooth;
  const SgForceHost& F = T.forces;
  if (!F.ok) { printf("%s refused: %s\n", blob_path, F.err.c_str()); return 1; }
  const int nq = K.o.nq, nv = D.o.nv, nu = S.o.nu > 0 ? S.o.nu : 1;
  if (raw.size() != sizeof(double) * (size_t)(nq + 2 * nv + nu + 1)) { printf("%s: state of %zu bytes\n", state_path, raw.size()); return 1; }
  const double* p = (const double*)raw.data();
  const std::vector<double> qpos(p, p + nq), qvel(p + nq, p + nq + nv), warm(p + nq + nv, p + nq + 2 * nv), act(p + nq + 2 * nv, p + nq + 2 * nv + nu);
  const double k = p[nq + 2 * nv + nu];
  const std::vector<int> kmj(K.o.njnt + 1, 0), kmt(D.o.ntendon + 1, 0);   // (no joint or tendon takes the per-env stiffness: k rides along unused)
  SgfHostOut o;
  if (sgf_host_env(T, qpos.data(), qvel.data(), act.data(), warm.data(), k, kmj.data(), kmt.data(), &o)) { printf("%s: a state that is not finite\n", state_path); return 1; }
  double fmax_ = 0.0, bmax = 0.0, worst = 0.0;
  std::vector<double> a(nv, 0.0);
  for (int i = 0; i < o.nefc; i++)
    for (int c = 0; c < nv; c++) a[c] += o.W[(size_t)i * nv + c] * o.f[i];
  for (int i = 0; i < o.nefc; i++) {
    fmax_ = fmax(fmax_, fabs(o.f[i]));
    bmax = fmax(bmax, fabs(o.sc[(size_t)i * SGF_SC + SGF_B]));
  }
  int neq = 0;
  for (int i = 0; i < o.nefc; i++)
    if (o.rtype[i] == SGF_EQUALITY) {
      neq++;
      const double* s = &o.sc[(size_t)i * SGF_SC];
      worst = fmax(worst, fabs(s[SGF_B] + s[SGF_R] * o.f[i] + sgf_dot(&o.J[(size_t)i * nv], a.data(), nv)));
    }
  printf("%s: nv %d rows %d (capacity %d, %d equalities) contacts %d sweeps %d max |f| %.6g equality residual %.3g of max |b| %.3g\n", blob_path, nv, o.nefc, F.o.nrows,
         neq, o.ncon, o.iters, fmax_, worst, bmax);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 3 || (argc - 1) % 2) { printf("usage: forces_main BLOB STATE ...\n"); return 2; }
  for (int i = 1; i + 1 < argc; i += 2)
    if (run(argv[i], argv[i + 1])) return 1;
  printf("ok\n");
  return 0;
}
