// Host check of the index rules by which the phase kernel hands the equality block to the rows solver (soft-grip_amd/csrc/sg_rows_layout.h:
// sg_eq_fix_index, sg_eq_nb_index for the writer; sg_eq_rec_trips, sg_eq_rec_row, sg_eq_rec_stored, sg_eq_rec_live, sg_eq_rec_index for the
// solver's staging trips), over the committed two-finger models at 1, 5 and 9 envs.
//   usage: sg_rows_staging_index MODEL.sgmodel...
// The work space is heap blocks of exactly the counts sg_rows_work_each enumerates, and every word a kernel would request is READ from
// them, so built with the host sanitizers (address, undefined) an index outside a block stops the program.  Checked per model and n:
//   * every (env, e) and (env, e, d) index of the writer lies inside its array's count, and the indices are distinct;
//   * the solver's lanes over its trips reach each of the 4 (N + 1) row records of an env exactly once, group N and nothing behind it is
//     read from memory, and a live row u = 4 e + d is read from where the writer put (e, d);
//   * the env slots of the ragged last wavefront (env >= n) and the lanes past the records still form addresses inside the arrays.
// tests/test_rows_staging_host.py builds and runs this; it prints one line per model and "PASS <models>".
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../../soft-grip_amd/csrc/sg_rows_host.h"

static int fails = 0;
#define CHECK(c, ...)                                       \
  do {                                                      \
    if (!(c)) {                                             \
      if (fails++ < 20) { std::printf("FAIL %s: ", #c); std::printf(__VA_ARGS__); std::printf("\n"); } \
    }                                                       \
  } while (0)

// heap blocks of exact size, every word 1.0 (a read word is counted by its value); a count of 0 gives one element
struct Heap {
  std::vector<void*> blocks;
  std::vector<size_t> counts;
  ~Heap() { for (void* p : blocks) std::free(p); }
  template <class T>
  bool operator()(T** out, size_t count) {
    counts.push_back(count);
    blocks.push_back(std::malloc((count ? count : 1) * sizeof(T)));
    *out = (T*)blocks.back();
    for (size_t i = 0; i < (count ? count : 1); i++) (*out)[i] = (T)1;
    return true;
  }
  size_t count_of(const void* p) const {
    for (size_t i = 0; i < blocks.size(); i++)
      if (blocks[i] == p) return counts[i];
    return 0;
  }
};

static void check_model(const std::string& label, const SgPlanHeader& H, int rounds, int n) {
  const int N = H.nelem;
  Heap heap;
  SgWork w = {};
  CHECK(sg_rows_work_each(w, H, rounds, (size_t)n, false, heap), "%s n %d: enumeration", label.c_str(), n);
  const size_t fix_n = heap.count_of(w.eqb), nb_n = heap.count_of(w.nbb);
  CHECK(fix_n == heap.count_of(w.eqR) && nb_n == heap.count_of(w.nbR), "%s n %d: g and c arrays of different counts", label.c_str(), n);
  double sum = 0;
  unsigned long long reads = 0;
  // ---- the writer: element-major, dense, inside the counts, distinct
  std::vector<char> fix_seen(fix_n, 0), nb_seen(nb_n, 0);
  for (int env = 0; env < n; env++)
    for (int e = 0; e < N; e++) {
      const size_t o = sg_eq_fix_index((size_t)env, e, N);
      CHECK(o < fix_n, "%s n %d: fix row (%d, %d) at %zu of %zu", label.c_str(), n, env, e, o, fix_n);
      if (o >= fix_n) continue;
      CHECK(!fix_seen[o], "%s n %d: fix row (%d, %d) shares word %zu", label.c_str(), n, env, e, o);
      fix_seen[o] = 1;
      sum += w.eqb[o] + w.eqR[o]; reads += 2;
      if (H.nnb == 0) continue;
      for (int d = 0; d < 3; d++) {
        const size_t q = sg_eq_nb_index((size_t)env, e, d, N);
        CHECK(q < nb_n, "%s n %d: neighbour row (%d, %d, %d) at %zu of %zu", label.c_str(), n, env, e, d, q, nb_n);
        if (q >= nb_n) continue;
        CHECK(!nb_seen[q], "%s n %d: neighbour row (%d, %d, %d) shares word %zu", label.c_str(), n, env, e, d, q);
        nb_seen[q] = 1;
        sum += w.nbb[q] + w.nbR[q]; reads += 2;
      }
    }
  for (size_t o = 0; o < (size_t)n * N && o < fix_n; o++) CHECK(fix_seen[o], "%s n %d: fix word %zu is nobody's (not dense)", label.c_str(), n, o);
  if (H.nnb > 0)
    for (size_t q = 0; q < (size_t)n * 3 * N && q < nb_n; q++) CHECK(nb_seen[q], "%s n %d: neighbour word %zu is nobody's (not dense)", label.c_str(), n, q);
  if (H.nnb == 0) { CHECK(sum == (double)reads, "%s n %d: read words", label.c_str(), n); return; }
  // ---- the solver: four env slots per wavefront, trips of 64 lanes over the padded row count of its instantiation
  const int NR = 8 * sg_rows_nsl(N), trips = sg_eq_rec_trips(NR);
  CHECK(NR >= N && 64 * trips >= 4 * (N + 1), "%s: %d trips for %d elements", label.c_str(), trips, N);
  for (int wave = 0; wave < (n + 3) / 4; wave++)
    for (int e2 = 0; e2 < 4; e2++) {
      const size_t env = (size_t)wave * 4 + e2;     // may be past the batch: loaded like the others, from a clamped address
      std::vector<int> stored(4 * (N + 1), 0);
      for (int t = 0; t < trips; t++)
        for (int lane = 0; lane < 64; lane++) {
          const int u = sg_eq_rec_row(lane, t);
          const size_t o = sg_eq_rec_index(env, u, N, (size_t)n);
          const int uc = u < 4 * N ? u : 4 * N - 1, d = uc & 3;
          CHECK(o < (d == 0 ? fix_n : nb_n), "%s n %d: env slot %zu row %d reads word %zu", label.c_str(), n, env, u, o);
          if (o >= (d == 0 ? fix_n : nb_n)) continue;
          sum += (d == 0 ? w.eqb : w.nbb)[o] + (d == 0 ? w.eqR : w.nbR)[o]; reads += 2;    // every lane of every trip loads
          if (sg_eq_rec_stored(u, N)) {
            CHECK(u >= 0 && u < 4 * (N + 1), "%s: row %d stored", label.c_str(), u);
            stored[u]++;
          }
          CHECK(sg_eq_rec_live(u, N) == (u < 4 * N) && (!sg_eq_rec_live(u, N) || sg_eq_rec_stored(u, N)), "%s: row %d live", label.c_str(), u);
          if (sg_eq_rec_live(u, N) && env < (size_t)n) {   // ... from where the writer put it
            const int e = u >> 2;
            const size_t want = (u & 3) == 0 ? sg_eq_fix_index(env, e, N) : sg_eq_nb_index(env, e, (u & 3) - 1, N);
            CHECK(o == want, "%s n %d: env %zu row %d read at %zu, written at %zu", label.c_str(), n, env, u, o, want);
          }
        }
      for (int u = 0; u < 4 * (N + 1); u++) CHECK(stored[u] == 1, "%s n %d: env slot %zu row %d staged %d times", label.c_str(), n, env, u, stored[u]);
      for (int u = 4 * N; u < 4 * (N + 1); u++) CHECK(!sg_eq_rec_live(u, N), "%s: group N row %d is not zero", label.c_str(), u);
    }
  CHECK(sum == (double)reads, "%s n %d: read words", label.c_str(), n);
}

int main(int argc, char** argv) {
  int models = 0;
  for (int a = 1; a < argc; a++) {
    const std::string path = argv[a], label = path.substr(path.find_last_of('/') + 1);
    std::ifstream f(path, std::ios::binary);
    if (!f) { std::printf("%s cannot be read\n", label.c_str()); return 1; }
    const std::string blob((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    SgPlan P;
    std::string err;
    if (!sg_plan_build(blob.data(), blob.size(), &P, &err)) { std::printf("%s: refused: %s\n", label.c_str(), err.c_str()); return 1; }
    const int rounds = (P.h.nelem + 63) / 64;
    for (int n : {1, 5, 9}) check_model(label, P.h, rounds, n);
    std::printf("checked %s: %d elements, %d neighbour rows, %d trips\n", label.c_str(), P.h.nelem, P.h.nnb, P.h.nnb > 0 ? sg_eq_rec_trips(8 * sg_rows_nsl(P.h.nelem)) : 0);
    models++;
  }
  std::printf(fails ? "FAILED (%d)\n" : "PASS %d models\n", fails ? fails : models);
  return fails ? 1 : 0;
}
