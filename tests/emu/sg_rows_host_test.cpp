// Host test of the rows pipeline's host side (soft-grip_amd/csrc/sg_rows_host.h) by the rules by which the KERNELS index what it
// makes; tests/test_rows_host.py builds this with the host sanitizers (address, undefined), runs it over the committed two-finger
// models and holds its digest lines against tests/golden/rows_host_digests.json.
//   usage: sg_rows_host_test MODEL.sgmodel...
// Per model one digest line -- FNV-1a hashes and lengths of the padded schedule, the table and cpos, and every work-space count at
// 1, 9 and 4096 envs -- then the checks, at 1, 3, 4, 5, 8 and 9 envs (where (n + 3) / 4, (n + 7) / 8 and the ragged last wavefront
// differ).  The table, the solver's LDS block and every work-space buffer are heap blocks of exactly the size sg_rows_host.h gives, and
// every address a kernel forms is READ from them: under the sanitizer an index outside a block stops the program.  The index rules are
// sg_rows_layout.h's functions, the ones the kernels call (adr_of, row0 and load_row of sg_rows.hip, the exports of sg_phase.hip); what is
// stated here on its own is what the kernels NEED of each region -- how many words of which size they put there.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <memory>
#include <set>
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

static uint64_t fnv1a(const void* p, size_t n) {
  uint64_t h = 0xcbf29ce484222325ull;
  for (size_t i = 0; i < n; i++) h = (h ^ ((const unsigned char*)p)[i]) * 0x100000001b3ull;
  return h;
}
template <class V>
static void part(const char* name, const V& v) {
  std::printf(" %s=%016llx/%zu", name, (unsigned long long)fnv1a(v.data(), v.size() * sizeof(v[0])), v.size());
}

// heap blocks of exact size, zero-filled; a count of 0 gives one element (SgArena::zeros)
struct Heap {
  std::vector<void*> blocks;
  std::vector<size_t> counts;
  ~Heap() { for (void* p : blocks) std::free(p); }
  template <class T>
  bool operator()(T** out, size_t count) {
    counts.push_back(count);
    blocks.push_back(std::calloc(count ? count : 1, sizeof(T)));
    *out = (T*)blocks.back();
    return true;
  }
  template <class T>
  T* copy(const std::vector<T>& v) {
    T* p = nullptr;
    (*this)(&p, v.size());
    for (size_t i = 0; i < v.size(); i++) p[i] = v[i];
    return p;
  }
};

static const char* const WORK_NAMES[] = {"crec", "ns", "crow", "cdummy", "envh", "shared", "pending", "status", "iters", "ncon", "nefc", "touch", "sMinv", "saF",
                                         "lim_active", "lim", "as", "eqf", "eqb", "eqR", "asme", "fsm", "chh", "nbf", "nbb", "nbR", "cst", "gcon", "gen", "gen_count",
                                         "gen_list", "gpairs16", "gcval"};
static const size_t NWORK = sizeof WORK_NAMES / sizeof WORK_NAMES[0];
static_assert(sizeof(SgWork) == (NWORK + 1) * sizeof(void*), "a member of SgWork without a name here (secprof is the batch's)");

static std::vector<size_t> work_counts(const SgPlanHeader& H, int rounds, size_t n, bool legacy) {
  SgWork w = {};
  std::vector<size_t> c;
  sg_rows_work_each(w, H, rounds, n, legacy, [&](auto**, size_t count) { c.push_back(count); return true; });
  return c;
}

static void digest_line(const std::string& label, const SgPlan& P, int rounds) {
  std::printf("%s:", label.c_str());
  if (P.h.nnb > 0) {
    SgRowsTables T;
    sg_rows_tables(P, &T);
    part("sched", T.sched); part("tab", T.tab); part("cpos", T.cpos);
  } else std::printf(" no tables");
  for (size_t n : {(size_t)1, (size_t)9, (size_t)4096}) {
    const std::vector<size_t> c = work_counts(P.h, rounds, n, false);
    CHECK(c.size() == NWORK, "%zu buffers enumerated", c.size());
    std::printf(" work%zu:", n);
    for (size_t k = 0; k < c.size() && k < NWORK; k++) std::printf("%s%s=%zu", k ? "," : "", WORK_NAMES[k], c[k]);
  }
  for (size_t n : {(size_t)1, (size_t)9, (size_t)4096}) std::printf(" legacy%zu:crec=%zu", n, work_counts(P.h, rounds, n, true)[0]);
  std::printf("\n");
}

// 0. layouts that depend on no model: the contact row's fields and the chain hand-off record
static void check_static_layouts() {
  int slot[SG_RK] = {};
  for (int k = 0; k < SG_RK; k++) {
    const int pr = sg_row_pair(k), h = sg_row_half(k);
    CHECK(pr >= 0 && pr < SG_RK / 2 && (h == 0 || h == 1), "field %d: pair %d half %d", k, pr, h);
    if (pr >= 0 && pr < SG_RK / 2 && (h == 0 || h == 1)) slot[2 * pr + h]++;
    CHECK(sg_row_imm(k) == (pr - SG_ROW_BASE_PAIR) * 64 && SG_ROW_INDEX(0, 0, k, 0, 1) == (size_t)(128 * pr + h), "field %d: immediate %d", k, sg_row_imm(k));
  }
  for (int q = 0; q < SG_RK; q++) CHECK(slot[q] == 1, "slot %d of a contact row holds %d fields", q, slot[q]);
  int cell[SG_CHW] = {};
  for (const SgHandoffField& f : SG_HANDOFF_FIELDS)
    for (int j = f.off; j < f.off + f.len; j++) {
      CHECK(j >= 0 && j < SG_CHW, "hand-off field at %d leaves the record", f.off);
      if (j >= 0 && j < SG_CHW) cell[j]++;
    }
  static_assert(SGH_END == SGH_LIMF + SG_MAXLIM, "the limit rows' forces end the record");
  for (int j = 0; j < SG_CHW; j++) CHECK(cell[j] == (j < SGH_END ? 1 : 0), "hand-off word %d belongs to %d fields", j, cell[j]);
}

// 1. the solver's LDS block: the regions' starts off[0 .. nregion - 1] in order, what the kernel puts into each (`need`) ending before the next
// begins, the last region's end off[nregion] at lds_doubles.  Returns a block of exactly that size.
static double* lds_block(Heap& heap, const std::string& label, int nregion, const size_t* off, const size_t* need, size_t total) {
  CHECK(off[0] == 0 && off[nregion] == total, "%s: the LDS regions end at %zu of %zu doubles", label.c_str(), off[nregion], total);
  for (int r = 0; r < nregion; r++)
    CHECK(need[r] > 0 && off[r] + need[r] <= off[r + 1], "%s: LDS region %d at %zu, the kernel needs %zu, next at %zu", label.c_str(), r, off[r], need[r], off[r + 1]);
  double* lds = nullptr;
  heap(&lds, total);
  double sum = 0;
  for (int r = 0; r < nregion; r++) sum += lds[off[r]] + lds[off[r] + need[r] - 1];
  CHECK(sum == 0.0, "read words");
  return lds;
}
static void check_lds_fix(const std::string& label, const SgRowsShape& sh, int epw, int nsl) {
  const int NR = 8 * nsl;
  const size_t z = 0, oBR = SG_LDS_FIX_BR(z, epw, NR), oRI = SG_LDS_FIX_RI(oBR, epw, NR), oIC = SG_LDS_FIX_IC(oRI, epw, NR), oZ = SG_LDS_FIX_ZERO(oIC, NR);
  const size_t off[6] = {z, oBR, oRI, oIC, oZ, SG_LDS_FIX_END(oZ)};
  // AF, BR: a pair per env and row; RI: a word; IC: a pair per row; the zero word and 64 sink words
  const size_t need[5] = {(size_t)2 * epw * NR, (size_t)2 * epw * NR, (size_t)epw * NR, (size_t)2 * NR, 65};
  Heap heap;
  lds_block(heap, label + " epw " + std::to_string(epw), 5, off, need, sh.lds_doubles(epw, nsl));
  CHECK(NR >= sh.nelem, "%s: %d rows for %d elements", label.c_str(), NR, sh.nelem);
}

// ... of a neighbour-row model, and 2. the table decodes back to the schedule, by the kernel's rule, into that block
static void check_tables(const std::string& label, const SgPlan& P, const SgRowsShape& sh, const SgRowsTables& T, int epw) {
  const SgPlanHeader& H = P.h;
  const int N = H.nelem, R = H.eq_rounds;
  const bool cst = sh.nb_mode == 2;
  CHECK(T.sched.size() == (size_t)(R + 8) * SG_EQ_SLOTS && P.sched.size() == (size_t)R * SG_EQ_SLOTS, "%s: %zu slots", label.c_str(), T.sched.size());
  CHECK(T.tab.size() == sh.tab_words, "%s: %zu table words, the kernel stages %zu", label.c_str(), T.tab.size(), sh.tab_words);
  const size_t z = 0, oGS = SG_LDS_NB_GS(z, epw, N), oTAB = SG_LDS_NB_TAB(oGS, epw, N, cst), oZ = SG_LDS_NB_ZERO(oTAB, R, cst), oENV = SG_LDS_NB_ENV(oZ);
  const size_t off[6] = {z, oGS, oTAB, oZ, oENV, SG_LDS_NB_END(oENV, epw)};
  // per env N sliders and the zero word | per env N + 1 groups of four states (8 bytes) or records (16) | the table | the zero word and 64 sink
  // words | two words per env
  const size_t NA = SG_ROWS_NA_NB(N), GW = SG_ROWS_GW_NB(N, cst);
  const size_t need[5] = {(epw - 1) * NA + N + 1, (size_t)epw * (cst ? 4 : 8) * (N + 1), T.tab.size() * sizeof(unsigned) / sizeof(double), 65, (size_t)2 * epw};
  CHECK(NA >= (size_t)N + 1 && NA % 2 == 0 && sizeof(unsigned) * T.tab.size() == sizeof(double) * (oZ - oTAB), "%s: slider words %zu, table region %zu", label.c_str(), NA, oZ - oTAB);
  CHECK(sizeof(double) * sh.lds_doubles(epw, 0) <= 160 * 1024, "%s: LDS", label.c_str());
  Heap heap;
  double* const lds = lds_block(heap, label + " epw " + std::to_string(epw), 5, off, need, sh.lds_doubles(epw, 0));
  const unsigned* tab = heap.copy(T.tab);
  double sum = 0;
  for (int le = 0; le < epw; le += epw - 1) {   // the first and the last env of the wavefront
    const char* const Ae = (const char*)(lds + (size_t)le * NA);
    const char* const GS = (const char*)(lds + oGS + (size_t)le * GW);
    for (size_t i = 0; i < T.sched.size(); i++) {
      const SgEqSlot& sl = T.sched[i];
      const size_t round = i / SG_EQ_SLOTS, b = i % SG_EQ_SLOTS;
      if (i >= P.sched.size()) CHECK(sl.e == N && sl.p[0] == N && sl.p[1] == N && sl.p[2] == N, "%s: spare slot %zu is not idle", label.c_str(), i);
      CHECK(sl.e >= 0 && sl.e <= N, "%s: slot %zu element %d", label.c_str(), i, sl.e);
      for (int h = 0; h < 2; h++) {
        const size_t g = 2 * b + h, t = round * 16 + g;   // the lane's word (pair) of the round: TAB + g, + 16 per round
        unsigned px, py, rec;
        if (cst) { const unsigned tt = tab[t]; px = sg_tab1_x(tt); py = sg_tab1_y(tt); rec = sg_tab1_rec(tt); }
        else { const unsigned x = tab[2 * t], y = tab[2 * t + 1]; px = sg_tab2_x(x); py = sg_tab2_y(x); rec = y; }
        const int want_x = h ? sl.p[1] : sl.e, want_y = h ? sl.p[2] : sl.p[0];
        CHECK(px == 8u * want_x && py == 8u * want_y, "%s: slot %zu h %d decodes to sliders %u %u, wanted %d %d", label.c_str(), i, h, px / 8, py / 8, want_x, want_y);
        // the lane's rows 2 h, 2 h + 1 of group e: states of 8 bytes (streamed factors) or records (g, c) of 16
        const unsigned want_rec = (cst ? 8u : 16u) * (4u * sl.e + 2u * h);
        CHECK(rec == want_rec && rec % 16 == 0, "%s: slot %zu h %d row states at byte %u, wanted %u", label.c_str(), i, h, rec, want_rec);
        CHECK(px % 8 == 0 && py % 8 == 0 && px + 8 <= 8 * NA && py + 8 <= 8 * NA && rec + (cst ? 16 : 32) <= 8 * GW, "%s: slot %zu h %d leaves its LDS region", label.c_str(), i, h);
        sum += *(const double*)(Ae + px) + *(const double*)(Ae + py);
        for (unsigned k = 0; k < (cst ? 2u : 4u); k++) sum += ((const double*)(GS + rec))[k];
      }
    }
  }
  // the deepest words the solver fetches: two rounds past its padded round count (trips of 4 rounds, of 2 with the factors in LDS)
  const int trip = cst ? 4 : 2, padded = (R + trip - 1) & ~(trip - 1);
  CHECK(padded + 1 < R + 8, "%s: look-ahead past the spare rounds", label.c_str());
  for (size_t w = 0; w < (cst ? 1u : 2u); w++) sum += tab[(cst ? 1 : 2) * ((size_t)(padded + 1) * 16 + 15) + w];
  CHECK(sum >= 0, "read words");
  // 3. cpos: one place per scheduled element, inside the scheduled rounds
  CHECK(T.cpos.size() == (size_t)N, "%s: cpos of %zu", label.c_str(), T.cpos.size());
  std::set<int> seen, elems;
  for (size_t i = 0; i < P.sched.size(); i++) {
    const int e = P.sched[i].e;
    if (e >= N) continue;
    CHECK(elems.insert(e).second, "%s: element %d scheduled twice", label.c_str(), e);
    CHECK(seen.insert(T.cpos[e]).second && T.cpos[e] >= 0 && T.cpos[e] + 4 <= 128 * R && T.cpos[e] % 4 == 0, "%s: cpos[%d] = %d", label.c_str(), e, T.cpos[e]);
  }
  CHECK((int)elems.size() == N, "%s: %zu of %d elements scheduled", label.c_str(), elems.size(), N);
}

// 3 (per env) and 4: the kernels' addresses into the work space of an n-env batch
static void check_work(const std::string& label, const SgPlan& P, int rounds, const SgRowsShape& sh, const SgRowsTables& T, int n) {
  const SgPlanHeader& H = P.h;
  const int R = H.eq_rounds, nwb = (n + 7) / 8;
  Heap heap;
  SgWork w = {};
  CHECK(sg_rows_work_each(w, H, rounds, (size_t)n, false, heap) && heap.counts.size() == NWORK, "%s n %d: enumeration", label.c_str(), n);
  const std::vector<size_t>& c = heap.counts;
  const size_t crow_n = c[2], cdummy_n = c[3], cst_n = c[26];
  CHECK(heap.blocks[2] == (void*)w.crow && heap.blocks[3] == (void*)w.cdummy && heap.blocks[26] == (void*)w.cst, "%s: the order of WORK_NAMES", label.c_str());
  double sum = 0;
  // contact rows: every slot, block (the dummies nwb, nwb + 1 included), field and lane; the last word is the buffer's last
  for (int slot = 0; slot < SG_CAP + 2; slot++)
    for (int wave = 0; wave < nwb + 2; wave++)
      for (int k = 0; k < SG_RK; k++)
        for (int lane = 0; lane < 64; lane += (slot == 0 || slot == SG_CAP + 1 || wave >= nwb - 1) ? 1 : 63) sum += w.crow[SG_ROW_INDEX(slot, wave, k, lane, nwb)];
  CHECK(SG_ROW_INDEX(SG_CAP + 1, nwb + 1, SG_RK - 1, 63, nwb) + 1 == crow_n, "%s n %d: crow of %zu", label.c_str(), n, crow_n);
  // a lane's column as the solver forms it: row0 (biased to SG_ROW_BASE_PAIR), a slot stride in 16-byte units, the field pairs by their
  // immediates -- every slot of the buffer, SG_CAP + 1 included, at 4 envs per wavefront and, where the model has no neighbour rows, at 8.
  // The env slots of the ragged last wavefront and the lanes outside the finger quads stay on their wavefront's private zero block
  for (int epw : {4, 8}) {
    if (epw == 8 && sh.nb_mode) continue;
    const int lpe = sh.nb_mode ? 16 : 8;   // lanes per env
    for (int blk = 0; blk < (n + epw - 1) / epw; blk++)
      for (int lane = 0; lane < 64; lane++) {
        const int le = lane / lpe, g = lane % lpe, env = blk * epw + le;
        const bool has_row = le < epw && env < n && g < 8;
        const size_t row0 = has_row ? SG_ROW_INDEX(0, env >> 3, 2 * SG_ROW_BASE_PAIR, 8 * (env & 7) + g, nwb) : sg_row_dummy_index((size_t)blk, SG_ROW_BASE_PAIR) + 2 * lane;
        const size_t stride = has_row ? 2 * sg_row_slot_stride(nwb) : 0, count = has_row ? crow_n : cdummy_n;
        const double* const base = has_row ? w.crow : w.cdummy;
        for (int slot = 0; slot < SG_CAP + 2; slot++)
          for (int k = 0; k < SG_RK; k++) {
            const ptrdiff_t at = (ptrdiff_t)(row0 + slot * stride) + 2 * sg_row_imm(k) + sg_row_half(k);
            CHECK(at >= 0 && (size_t)at < count, "%s n %d epw %d block %d lane %d slot %d field %d: word %td of %zu", label.c_str(), n, epw, blk, lane, slot, k, at, count);
            if (at >= 0 && (size_t)at < count) sum += base[at];
            if (has_row) CHECK((size_t)at == SG_ROW_INDEX(slot, env >> 3, k, 8 * (env & 7) + g, nwb), "%s n %d: the solver's field %d of slot %d is not the exporter's", label.c_str(), n, k, slot);
          }
      }
  }
  CHECK(sg_row_dummy_index((size_t)((n + 3) / 4 - 1), SG_RK / 2 - 1) + 2 * 63 + 2 == cdummy_n, "%s n %d: cdummy of %zu", label.c_str(), n, cdummy_n);
  if (sh.nb_mode == 2) {
    // the stream of step factors: what the solver's lanes read, up to its deepest prefetched round (the first four rounds, then four ahead
    // inside the padded round count)
    const int padded = (R + 3) & ~3, deepest = padded - 1 > 3 ? padded - 1 : 3;
    CHECK(deepest < sh.cst_rounds && sh.cst_rounds == R + 8, "%s: %d rounds of step factors", label.c_str(), sh.cst_rounds);
    for (int wv = 0; wv < (n + 3) / 4; wv++)
      for (int k = 0; k <= deepest; k++)
        for (int lane = 0; lane < 64; lane++) { const double* const q = w.cst + SG_CST_INDEX(wv, k, lane, R + 8); sum += q[0] + q[1]; }
    CHECK(SG_CST_INDEX((n + 3) / 4 - 1, sh.cst_rounds - 1, 63, sh.cst_rounds) + 2 == cst_n, "%s n %d: cst of %zu", label.c_str(), n, cst_n);
    // ... and where the phase kernel writes them: the four doubles of element e's block are the words of lanes 2 g, 2 g + 1 of the env's
    // group in the block's round
    for (int env = 0; env < n; env++)
      for (size_t i = 0; i < P.sched.size(); i++) {
        const int e = P.sched[i].e;
        if (e >= H.nelem) continue;
        const size_t round = i / SG_EQ_SLOTS, g = i % SG_EQ_SLOTS;
        const size_t dst = SG_CST_INDEX(env >> 2, 0, 16 * (env & 3), sh.cst_rounds) + T.cpos[e];
        const size_t rd0 = SG_CST_INDEX(env >> 2, round, 16 * (env & 3) + 2 * g, R + 8), rd1 = SG_CST_INDEX(env >> 2, round, 16 * (env & 3) + 2 * g + 1, R + 8);
        CHECK(dst == rd0 && dst + 2 == rd1 && dst % 2 == 0, "%s n %d env %d element %d: written at %zu, read at %zu and %zu", label.c_str(), n, env, e, dst, rd0, rd1);
        sum += w.cst[dst] + w.cst[dst + 1] + w.cst[dst + 2] + w.cst[dst + 3];
      }
  } else CHECK(cst_n == 0 && sh.cst_rounds == 0, "%s: a stream of %zu without streamed factors", label.c_str(), cst_n);
  CHECK((c[31] > 0) == (rounds >= 4) && (c[32] > 0) == (rounds >= 4), "%s: the slim phase kernel's lists", label.c_str());
  if (rounds >= 4) CHECK(c[31] == (size_t)n * SG_MAXCH * SG_CG * (4 * 64 + 2) && c[32] == (size_t)n * SG_MAXCH * 64, "%s n %d: gpairs16 %zu gcval %zu", label.c_str(), n, c[31], c[32]);
  CHECK(sum == 0.0, "%s n %d: read words", label.c_str(), n);
}

int main(int argc, char** argv) {
  int accepted = 0;
  check_static_layouts();
  for (int a = 1; a < argc; a++) {
    const std::string path = argv[a], label = path.substr(path.find_last_of('/') + 1);
    std::ifstream f(path, std::ios::binary);
    if (!f) { std::printf("%s cannot be read\n", label.c_str()); return 1; }
    const std::string blob((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    SgPlan P;
    std::string err;
    if (!sg_plan_build(blob.data(), blob.size(), &P, &err)) { std::printf("%s: refused: %s\n", label.c_str(), err.c_str()); return 1; }
    const int rounds = (P.h.nelem + 63) / 64;
    digest_line(label, P, rounds);
    CHECK(sg_rows_admits(P.h, &err), "%s: %s", label.c_str(), err.c_str());
    accepted++;
    const SgRowsShape sh = sg_rows_shape(P.h);
    CHECK(sh.nb_mode == (P.h.nnb > 0 ? SG_ROWS_NB_MODE(P.h.nelem, P.h.eq_rounds) : 0) && sh.two_words == (sh.nb_mode == 1), "%s: mode %d", label.c_str(), sh.nb_mode);
    SgRowsTables T;
    if (sh.nb_mode) sg_rows_tables(P, &T);
    else CHECK(sh.tab_words == 0 && sh.cst_rounds == 0, "%s: shape without neighbour rows", label.c_str());
    for (int epw : {4, 8}) {   // (the kernel runs a neighbour-row model at 4 only; its carve holds at 8 all the same)
      if (sh.nb_mode) check_tables(label, P, sh, T, epw);
      else check_lds_fix(label, sh, epw, sg_rows_nsl(P.h.nelem));
    }
    for (int n : {1, 3, 4, 5, 8, 9}) check_work(label, P, rounds, sh, T, n);
    std::printf("checked %s: mode %d, %d elements, %d rounds\n", label.c_str(), sh.nb_mode, P.h.nelem, P.h.eq_rounds);
  }
  // 4. admission: 255 elements do not fit the table's fields, and a schedule whose table alone outgrows the LDS
  {
    SgPlanHeader H = {};
    std::string err;
    H.nnb = 1; H.nelem = 254; H.eq_rounds = 100;
    CHECK(sg_rows_admits(H, &err), "254 elements: %s", err.c_str());
    H.nelem = 255;
    CHECK(!sg_rows_admits(H, &err) && err == "too many neighbour equality rows for the PGS kernel's LDS", "255 elements: %s", err.c_str());
    H.nelem = 200; H.eq_rounds = 3000; err.clear();
    CHECK(sizeof(double) * SG_ROWS_LDS_NB(4, 200, 3000, 1) > 160 * 1024, "the header's LDS");
    CHECK(!sg_rows_admits(H, &err) && err == "too many neighbour equality rows for the PGS kernel's LDS", "LDS over 160 KB: %s", err.c_str());
    H.nnb = 0;
    CHECK(sg_rows_admits(H, &err), "no neighbour rows");
  }
  std::printf(fails ? "FAILED (%d)\n" : "PASS %d models\n", fails ? fails : accepted);
  return fails ? 1 : 0;
}
