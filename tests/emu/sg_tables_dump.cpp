// sg_tables_dump.cpp -- digests of the read-out tables csrc/sg_tables.cpp and sg_solve.h build of a model (tests/test_tables_host.py holds
// them against tests/golden/readout_table_digests.json, so an edit of a builder cannot change a table unnoticed).
//   usage: sg_tables_dump FILE...    FILE = a model blob, or an .xml scene (compiled by sg_mjcf_compile_file in both composite variants)
// Per input the tables are built on the plans as sg_model_create builds them (sg_host_tables_planned: a scene both plan builders refuse
// gets a plan that names no geom, the table builders take any blob).  Per table -- the forces table is not among them -- one line: the ok flag, the err text, and
// an FNV-1a hash (64 bits) over the raw bytes of the offset block and of every vector with its element count, and the scalars.  The
// tables are zero-initialised before the builder fills them (as `new sg_model()` leaves them), so the bytes are deterministic.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>

#include "../../soft-grip_amd/csrc/sg_mjcf.h"
#include "../../soft-grip_amd/csrc/sg_readout_host.h"   // sg_host_tables_planned

static uint64_t fnv1a(const void* p, size_t n) {
  uint64_t h = 0xcbf29ce484222325ull;
  for (size_t i = 0; i < n; i++) h = (h ^ ((const unsigned char*)p)[i]) * 0x100000001b3ull;
  return h;
}
template <class V>
static void part(const char* name, const V& v) {
  printf(" %s=%016llx/%zu", name, (unsigned long long)fnv1a(v.data(), v.size() * sizeof(v[0])), v.size());
}
template <class T>
static void head(const std::string& label, const char* table, const T& t) {
  printf("%s %s: ok=%d err='%s'", label.c_str(), table, (int)t.ok, t.err.c_str());
}
template <class O>
static void off(const O& o) {
  printf(" off=%016llx", (unsigned long long)fnv1a(&o, sizeof o));
}

static void dump(const std::string& label, const std::string& blob) {
  SgHostTables T{};
  bool has_fast, has_tree;
  sg_host_tables_planned(blob.data(), blob.size(), &T, &has_fast, &has_tree);
  printf("%s plans: fast=%d tree=%d\n", label.c_str(), (int)has_fast, (int)has_tree);
  const SgKinHost& K = T.kin;
  const SgConHost& C = T.con;
  const SgDynHost& D = T.dyn;
  const SgSmoothHost& S = T.smooth;
  const SgPointHost& P = T.point;
  const SgSolveHost& V = T.solve;
  head(label, "kin", K); off(K.o); part("dbl", K.dbl); part("ints", K.ints); part("qpos0", K.qpos0); part("rbound", K.rbound);
  printf(" bad_type=%d\n", K.bad_type);
  head(label, "con", C); part("pairs", C.pairs); part("gaux", C.gaux);
  printf(" cap=%d\n", C.cap);
  head(label, "dyn", D); off(D.o); part("dbl", D.dbl); part("ints", D.ints);
  printf("\n");
  head(label, "smooth", S); off(S.o); part("dbl", S.dbl); part("ints", S.ints);
  printf("\n");
  head(label, "point", P); off(P.o); part("ints", P.ints); part("site_body", P.site_body); part("site_pos", P.site_pos); part("site_quat", P.site_quat);
  printf("\n");
  head(label, "solve", V); off(V.o); part("ints", V.ints);
  printf("\n");
}

int main(int argc, char** argv) {
  for (int i = 1; i < argc; i++) {
    const std::string path = argv[i], base = path.substr(path.find_last_of('/') + 1);
    if (path.size() > 4 && path.compare(path.size() - 4, 4, ".xml") == 0) {
      for (int nb = 0; nb < 2; nb++) {
        std::string blob, err;
        const std::string label = base + " nb=" + std::to_string(nb);
        if (!sg_mjcf_compile_file(path.c_str(), nb != 0, false, &blob, &err)) { printf("%s compile error: %s\n", label.c_str(), err.c_str()); continue; }
        dump(label, blob);
      }
    } else {
      std::ifstream f(path, std::ios::binary);
      if (!f) { printf("%s cannot be read\n", base.c_str()); return 1; }
      dump(base, std::string(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>()));
    }
  }
  return 0;
}
