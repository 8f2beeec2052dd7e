// Host test of the element table the rows pipeline uploads (sg_rows_elem_table, soft-grip_amd/csrc/sg_rows_host.h): the plan's fields
// followed by the fields the host derives once per model, which the phase kernel used to recompute for every element in every substep.
// tests/test_phase_table_host.py builds this with the host sanitizers (address, undefined) and runs it over every committed model.
//   usage: sg_phase_table_test MODEL.sgmodel...
// Per model the two-finger plan accepts: the table is built through the product's host code and held, bit for bit (memcmp), against the
// expressions the kernel evaluated -- the same IEEE operations on the same table words in the same order:
//   SGD_MSUM      m = EL(SGE_MASS, e) + EL(SGE_ARMATURE, e)                           (FINISH)
//   SGD_INVM      1.0 / (EL(SGE_MASS, e) + EL(SGE_ARMATURE, e))                       (BEGIN's element stage, the contact rows; element 0's: im0)
//   SGD_NBINVW+d  EL(SGE_INVW, e) + EL(SGE_INVW, e2), e2 = nbtab[d * N + e] >= 0      (the neighbour rows' regulariser)
// Each operand is read through a volatile so that the compiler evaluates exactly these operations at run time.  The table's size and every
// field's place are sg_rows_layout.h's constants, the ones the kernel indexes by (enum SgElemDerived, sg_elem_table_index): asserted below.
// A model the two-finger plan refuses (the tree pipeline's scenes) has no such table: it is reported as "refused" and not counted.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../../soft-grip_amd/csrc/sg_rows_host.h"

// one set of constants: the derived fields follow the plan's, dense and in the order the kernel names them, and a field is nelem doubles
static_assert(SGD_MSUM == SGE_NFIELD && SGD_INVM == SGE_NFIELD + 1 && SGD_NBINVW == SGE_NFIELD + 2 && SGD_NFIELD == SGE_NFIELD + 5,
              "the derived fields lie behind the plan's fields, one after the other");
static_assert(sg_elem_table_index(0, 0, 7) == 0 && sg_elem_table_index(SGE_MASS, 3, 110) == (size_t)SGE_MASS * 110 + 3 &&
              sg_elem_table_index(SGD_NBINVW + 2, 109, 110) + 1 == sg_elem_table_doubles(110) && sg_elem_table_doubles(1) == (size_t)SGD_NFIELD,
              "field f of element e is word f * nelem + e; the last word of the last field ends the table");

static int fails = 0;
#define CHECK(c, ...)                                       \
  do {                                                      \
    if (!(c)) {                                             \
      if (fails++ < 20) { std::printf("FAIL %s: ", #c); std::printf(__VA_ARGS__); std::printf("\n"); } \
    }                                                       \
  } while (0)

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

int main(int argc, char** argv) {
  int checked = 0;
  for (int a = 1; a < argc; a++) {
    const std::string path = argv[a], label = path.substr(path.find_last_of('/') + 1);
    std::ifstream f(path, std::ios::binary);
    if (!f) { std::printf("%s cannot be read\n", label.c_str()); return 1; }
    const std::string blob((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    SgPlan P;
    std::string err;
    if (!sg_plan_build(blob.data(), blob.size(), &P, &err)) { std::printf("refused %s: %s\n", label.c_str(), err.c_str()); continue; }
    const int N = P.h.nelem;
    const std::vector<double> t = sg_rows_elem_table(P);
    CHECK(t.size() == sg_elem_table_doubles(N) && t.size() == (size_t)SGD_NFIELD * N, "%s: %zu words", label.c_str(), t.size());
    CHECK(P.elem.size() == (size_t)SGE_NFIELD * N && std::memcmp(t.data(), P.elem.data(), P.elem.size() * sizeof(double)) == 0,
          "%s: the plan's fields lead the table unchanged", label.c_str());
    CHECK((P.h.nnb > 0) == (P.nbtab.size() >= (size_t)9 * N), "%s: nbtab of %zu ints", label.c_str(), P.nbtab.size());
    auto EL = [&](int fld, int e) { volatile double v = t[sg_elem_table_index(fld, e, N)]; return (double)v; };   // what the kernel's EL(f, e) reads
    int rows = 0;
    for (int e = 0; e < N && fails == 0; e++) {
      const double m = EL(SGE_MASS, e) + EL(SGE_ARMATURE, e);
      CHECK(same_bits(EL(SGD_MSUM, e), m), "%s: msum of element %d", label.c_str(), e);
      const double im = 1.0 / (EL(SGE_MASS, e) + EL(SGE_ARMATURE, e));
      CHECK(same_bits(EL(SGD_INVM, e), im), "%s: invm of element %d", label.c_str(), e);
      for (int d = 0; d < 3; d++) {
        const int e2 = P.h.nnb > 0 ? P.nbtab[(size_t)d * N + e] : -1;
        CHECK(e2 >= -1 && e2 < N, "%s: partner %d of element %d", label.c_str(), e2, e);
        const double w = e2 >= 0 ? EL(SGE_INVW, e) + EL(SGE_INVW, e2) : 0.0;
        CHECK(same_bits(EL(SGD_NBINVW + d, e), w), "%s: neighbour weight %d of element %d", label.c_str(), d, e);
        rows += e2 >= 0;
      }
    }
    CHECK(rows == P.h.nnb, "%s: %d rows with a summed weight, %d neighbour rows", label.c_str(), rows, P.h.nnb);
    // the step factors' im0 (the neighbour rows' block of the phase kernel): element 0's inverse mass, as the kernel formed it
    const double im0 = 1.0 / (EL(SGE_MASS, 0) + EL(SGE_ARMATURE, 0));
    CHECK(same_bits(EL(SGD_INVM, 0), im0), "%s: im0", label.c_str());
    std::printf("checked %s: %d elements, %d neighbour rows, %zu words\n", label.c_str(), N, P.h.nnb, t.size());
    checked++;
  }
  std::printf(fails ? "FAILED (%d)\n" : "PASS %d models\n", fails ? fails : checked);
  return fails ? 1 : 0;
}
