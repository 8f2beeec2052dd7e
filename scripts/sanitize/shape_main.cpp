// The shape table's builder and the per-lane functions of sg_get_skin_vertices / sg_get_shape / sg_get_subtree (csrc/sg_shape.h: the text
// the kernel compiles, driven by sgh_host_env in the kernel's order) under AddressSanitizer and UBSan: a stand-alone program, nothing of
// it is loaded into python.  tests/test_shape_host.py builds and runs it:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I soft-grip_amd/csrc scripts/sanitize/shape_main.cpp
//       soft-grip_amd/csrc/sg_tables.cpp
//   usage: shape_main BLOB INTS DOUBLES ...   triples of files: a model blob; int32 nvert, nface, vert_body [nvert], face [nface][3]; doubles
//                                             vert_pos [nvert][3], qpos [nq], qvel [nv]
// Every vector has exactly the size the functions may read.  Per model: the skin as given, with every output and seven directions (one
// per body frame among them); the same skin with its last face dropped (open: the extents still run); a tetrahedron on the world body;
// no skin at all (the subtree rows alone); and the builder's refusal of an LDS block past the limit.
#include <cmath>
#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "sg_readout_host.h"   // sg_host_tables
#include "sg_shape.h"

static std::string slurp(const char* path) {
  std::ifstream f(path, std::ios::binary);
  return std::string(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

// every output of one env in vectors of exactly the sizes the call may write -> the volume (NaN without shape)
static double run_env(const SgKinHost& K, const SgDynHost& D, const SgSkinHost& S, const double* qpos, const double* qvel, int frame, bool want_shape, int* closed) {
  SgShapeHost T;
  sgh_build(K, D, S, &T);
  if (!T.ok) { printf("refused: %s\n", T.err.c_str()); return NAN; }
  *closed = T.o.closed;
  const int nb = K.o.nbody, nv = S.nvert;
  std::vector<double> dir, pos(3 * (size_t)nv), vel(3 * (size_t)nv), local(3 * (size_t)nv), shape(SGH_SHAPE_N), com(3 * (size_t)nb), lin(3 * (size_t)nb), ang(3 * (size_t)nb);
  std::vector<int> dir_body;
  const double base[4][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {0.3, -2, 0.7}};
  for (int j = 0; j < 7; j++) {
    for (int c = 0; c < 3; c++) dir.push_back(base[j % 4][c]);
    dir_body.push_back(j < 4 ? -1 : (j * 37) % nb);
  }
  const int nd = nv ? 7 : 0;
  std::vector<double> lo(nd), hi(nd);
  std::vector<int> lov(nd), hiv(nd);
  if (sgh_host_env(K, D, T, qpos, qvel, frame, nd, dir.data(), dir_body.data(), nv ? pos.data() : nullptr, nv ? vel.data() : nullptr, nv ? local.data() : nullptr,
                   want_shape ? shape.data() : nullptr, lo.data(), hi.data(), lov.data(), hiv.data(), com.data(), lin.data(), ang.data())) {
    printf("a state that is not finite\n");
    return NAN;
  }
  for (int j = 0; j < nd; j++)
    if (!(lo[j] <= hi[j]) || lov[j] < 0 || hiv[j] >= nv) { printf("extent %d out of order\n", j); return NAN; }
  std::vector<double> rest(3 * (size_t)nv);
  if (nv) sgh_rest(K, S, frame, rest.data());
  return want_shape ? shape[0] : NAN;
}

static int run(const char* blob_path, const char* int_path, const char* dbl_path) {
  const std::string blob = slurp(blob_path), ri = slurp(int_path), rd = slurp(dbl_path);
  SgHostTables T;
  sg_host_tables(blob.data(), blob.size(), &T);
  const SgKinHost& K = T.kin;
  const SgDynHost& D = T.dyn;
  if (!D.ok) { printf("%s refused: %s\n", blob_path, D.err.c_str()); return 1; }
  const int* pi = (const int*)ri.data();
  if (ri.size() < 8) { printf("%s: too short\n", int_path); return 1; }
  SgSkinHost S;
  S.nvert = pi[0]; S.nface = pi[1];
  const size_t nq = K.o.nq, nv = D.o.nv;
  if (ri.size() != 4 * (2 + (size_t)S.nvert + 3 * (size_t)S.nface) || rd.size() != 8 * (3 * (size_t)S.nvert + nq + nv)) { printf("%s: sizes do not match\n", int_path); return 1; }
  S.vert_body.assign(pi + 2, pi + 2 + S.nvert);
  S.face.assign(pi + 2 + S.nvert, pi + 2 + S.nvert + 3 * S.nface);
  const double* pd = (const double*)rd.data();
  S.vert_pos.assign(pd, pd + 3 * (size_t)S.nvert);
  const std::vector<double> qpos(pd + 3 * (size_t)S.nvert, pd + 3 * (size_t)S.nvert + nq), qvel(pd + 3 * (size_t)S.nvert + nq, pd + 3 * (size_t)S.nvert + nq + nv);
  int closed = -2, open_closed = -2, tet_closed = -2, none_closed = -2;
  const double V = run_env(K, D, S, qpos.data(), qvel.data(), S.vert_body[0], true, &closed);
  SgSkinHost Open = S;
  Open.nface--;
  Open.face.resize(3 * (size_t)Open.nface);
  run_env(K, D, Open, qpos.data(), qvel.data(), -1, false, &open_closed);
  SgSkinHost Tet;
  Tet.nvert = 4; Tet.nface = 4;
  Tet.vert_body.assign(4, 0);
  Tet.vert_pos = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1};
  Tet.face = {0, 2, 1, 0, 1, 3, 0, 3, 2, 1, 2, 3};
  const double Vt = run_env(K, D, Tet, qpos.data(), qvel.data(), -1, true, &tet_closed);
  SgSkinHost None;
  run_env(K, D, None, qpos.data(), qvel.data(), -1, false, &none_closed);
  printf("%s: %d vertices %d faces closed %d volume %.9g; open %d; tetrahedron closed %d volume %.9g; no skin %d\n", blob_path, S.nvert, S.nface, closed, V, open_closed,
         tet_closed, Vt, none_closed);
  if (!(closed == 1 && open_closed == 0 && tet_closed == 1 && none_closed == -1 && V > 0 && std::fabs(Vt - 1.0 / 6.0) < 1e-15)) return 1;
  // an LDS block past the limit: refused before any array is read
  SgKinHost Kb;
  SgDynHost Db;
  SgSkinHost Sb;
  SgShapeHost Tb;
  Kb.ok = Db.ok = true;
  Kb.o = SgKinOff();
  Kb.o.nbody = 1000;
  sgh_build(Kb, Db, Sb, &Tb);
  if (Tb.ok) return 1;
  printf("refused: %s\n", Tb.err.c_str());
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 4 || (argc - 1) % 3) { printf("usage: shape_main BLOB INTS DOUBLES ...\n"); return 2; }
  for (int i = 1; i + 2 < argc; i += 3)
    if (run(argv[i], argv[i + 1], argv[i + 2])) return 1;
  printf("ok\n");
  return 0;
}
