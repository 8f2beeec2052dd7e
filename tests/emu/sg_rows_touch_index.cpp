// Host check of the solver's look-ahead index rule (soft-grip_amd/csrc/sg_work.h: sg_rows_load_slot), exhaustively over every slot i and
// stream length nsmax in [0, SG_CAP], the look-ahead distances given on the command line and 4 and 8 envs per wavefront.  The row blocks
// are a real allocation of the size the library makes (sg_rows_host.h: [SG_CAP + 2][nwb + 2] blocks of 8 KB) and every requested row word is READ from
// it at the addresses the kernel forms, so built with the host sanitizers (address, undefined) an index outside it stops the program.
// tests/test_rows_touch_index.py builds and runs this; it prints one line per (epw, distance) and "PASS".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../soft-grip_amd/csrc/sg_rows_host.h"

static int fails = 0;
#define CHECK(c, ...)                                       \
  do {                                                      \
    if (!(c)) {                                             \
      if (fails++ < 20) { std::printf("FAIL %s: ", #c); std::printf(__VA_ARGS__); std::printf("\n"); } \
    }                                                       \
  } while (0)

int main(int argc, char** argv) {
  const int nenv = 9, nwb = (nenv + 7) / 8;
  size_t crow_count = 0;   // the size the library makes: sg_rows_work_each (crow's does not depend on the model)
  SgWork w = {};
  sg_rows_work_each(w, SgPlanHeader{}, 1, (size_t)nenv, false, [&](auto** p, size_t count) {
    if ((void*)p == (void*)&w.crow) crow_count = count;
    return true;
  });
  CHECK(crow_count > 0, "crow is not enumerated");
  std::vector<double> crow(crow_count, 1.0);
  unsigned long long reads = 0;
  double sum = 0;
  for (int a = 1; a < argc; a++) {
    const int D = std::atoi(argv[a]);
    for (int epw : {4, 8}) {
      for (int nsmax = 0; nsmax <= SG_CAP; nsmax++) {
        for (int i = 0; i <= SG_CAP; i++)
          for (int ahead = 1; ahead <= D; ahead++) {
            const int s = sg_rows_load_slot(i, ahead, nsmax);
            CHECK(s == -1 || (s == i + ahead && s >= 0 && s <= nsmax - 1 && s < SG_CAP + 2), "load i %d ahead %d nsmax %d -> %d", i, ahead, nsmax, s);
            CHECK((s == -1) == (i + ahead >= nsmax), "load i %d ahead %d nsmax %d -> %d", i, ahead, nsmax, s);
            if (s < 0) continue;
            for (int env = 0; env < nenv; env++)      // the 16 fields of every row lane of every env, as load_row forms them (SG_ROW_INDEX)
              for (int g = 0; g < 8; g++)
                for (int k = 0; k < SG_RK; k++) { sum += crow[SG_ROW_INDEX(s, env >> 3, k, 8 * (env & 7) + g, nwb)]; reads++; }
          }
        // a whole pass as the kernel runs it: trips of two while a slot two ahead exists, then the last one or two slots; the slots it
        // loads are 0 .. nsmax - 1, each once, in order (nsmax = 0: the kernel skips the pass)
        if (nsmax > 0) {
          std::vector<int> loaded{0};
          int i = 0;
          for (; sg_rows_load_slot(i, 2, nsmax) >= 0; i += 2) { loaded.push_back(sg_rows_load_slot(i, 1, nsmax)); loaded.push_back(sg_rows_load_slot(i, 2, nsmax)); }
          if (sg_rows_load_slot(i, 1, nsmax) >= 0) loaded.push_back(sg_rows_load_slot(i, 1, nsmax));
          CHECK((int)loaded.size() == nsmax, "nsmax %d: %zu slots loaded", nsmax, loaded.size());
          for (size_t k = 0; k < loaded.size(); k++) CHECK(loaded[k] == (int)k, "nsmax %d: load %zu is slot %d", nsmax, k, loaded[k]);
          CHECK(i < nsmax && i + 2 >= nsmax, "nsmax %d: the pass ends at slot %d", nsmax, i);
        }
      }
      std::printf("epw %d distance %d: %llu words read\n", epw, D, reads);
    }
  }
  CHECK(sum == (double)reads, "read words");
  std::printf(fails ? "FAILED (%d)\n" : "PASS\n", fails);
  return fails ? 1 : 0;
}
