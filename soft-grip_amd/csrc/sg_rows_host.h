// sg_rows_host.h -- the host side of the rows pipeline (sg_phase.hip, sg_rows.hip), in one place and free of device calls: which models
// the solver admits, the shape of its launch, the solver's tables as the kernels decode them, and the size of every buffer of SgWork.
// sg_api.hip's rows_alloc and launch_split are its users in the library.  Every layout rule it sizes and packs by is sg_rows_layout.h's, the
// kernels' own; tests/emu/sg_rows_host_test.cpp runs those rules over blocks of the sizes made here.
#pragma once
#include <string>
#include <vector>

#include "sg_plan.h"
#include "sg_work.h"

// does the rows solver run a two-finger model?  (neighbour-row models: the kernel keeps every equality row of its envs in LDS)
inline bool sg_rows_admits(const SgPlanHeader& H, std::string* err) {
  if (H.nnb > 0 && (H.nelem > SG_ROWS_MAX_NELEM || sizeof(double) * SG_ROWS_LDS_NB(4, H.nelem, H.eq_rounds, 1) > 160 * 1024)) {
    if (err) *err = "too many neighbour equality rows for the PGS kernel's LDS";
    return false;
  }
  return true;
}

// what a model fixes of the solver's launch
struct SgRowsShape {
  int nelem = 0, eq_rounds = 0;
  int nb_mode = 0;         // template parameter NB of sg_pgs_rows_kernel: 0 no neighbour rows, 1 their step factors in LDS, 2 streamed (SgWork::cst)
  bool two_words = false;  // the table has two words per lane and round (nb_mode 1)
  int cst_rounds = 0;      // rounds of SgWork::cst per solver wavefront: eq_rounds + 8 (nb_mode 2), else 0 -- nothing to stream
  size_t tab_words = 0;    // the table: 16 lanes x (1 | 2) words x (eq_rounds + 8) rounds, 0 without neighbour rows
  // the kernel's LDS block in doubles: epw envs per wavefront; nsl (sg_rows_nsl) pads the joint-fix rows of a model without neighbour rows
  size_t lds_doubles(int epw, int nsl) const {
    return nb_mode ? SG_ROWS_LDS_NB(epw, nelem, eq_rounds, nb_mode == 2) : SG_ROWS_LDS_FIX(epw, 8 * nsl);
  }
};
inline SgRowsShape sg_rows_shape(const SgPlanHeader& H) {
  SgRowsShape s;
  s.nelem = H.nelem; s.eq_rounds = H.eq_rounds;
  s.nb_mode = H.nnb > 0 ? SG_ROWS_NB_MODE(H.nelem, H.eq_rounds) : 0;
  s.two_words = s.nb_mode == 1;
  s.cst_rounds = s.nb_mode == 2 ? H.eq_rounds + 8 : 0;
  s.tab_words = s.nb_mode ? sizeof(double) / sizeof(unsigned) * SG_LDS_NB_ZERO((size_t)0, H.eq_rounds, s.nb_mode == 2) : 0;
  return s;
}

// the tables of a neighbour-row model, as the batch uploads them
struct SgRowsTables {
  std::vector<SgEqSlot> sched;  // SgPlan::sched + eight spare rounds of idle slots (the kernel fetches slots a few rounds ahead)
  std::vector<unsigned> tab;    // the same schedule as the solver's table words (above)
  std::vector<int> cpos;        // per element: where the phase kernel puts its block's four step factors (SgPhaseArgs::cpos)
};
inline void sg_rows_tables(const SgPlan& P, SgRowsTables* T) {
  const SgPlanHeader& H = P.h;
  T->sched = P.sched;
  SgEqSlot idle;
  idle.e = idle.p[0] = idle.p[1] = idle.p[2] = H.nelem;
  for (int g = 0; g < 8 * SG_EQ_SLOTS; g++) T->sched.push_back(idle);
  const std::vector<SgEqSlot>& sch = T->sched;
  const bool two_words = sg_rows_shape(H).two_words;
  T->tab.assign((two_words ? 4 : 2) * sch.size(), 0u);
  for (size_t i = 0; i < 2 * sch.size(); i++) {
    const SgEqSlot& sl = sch[i >> 1];
    const int h = (int)(i & 1);
    const unsigned x = h ? sl.p[1] : sl.e, y = h ? sl.p[2] : sl.p[0];
    if (two_words) { T->tab[2 * i] = sg_tab2_pack(x, y); T->tab[2 * i + 1] = sg_tab2_rec((unsigned)sl.e, (unsigned)h); }
    else T->tab[i] = sg_tab1_pack(x, y, (unsigned)sl.e, (unsigned)h);
  }
  // round r, slot g of the schedule = lanes 2 g, 2 g + 1 of the env's 16-lane group, two doubles each (SG_CST_INDEX): doubles from the
  // start of the env's group in round 0
  T->cpos.assign(H.nelem, 0);
  for (size_t i = 0; i < P.sched.size(); i++)
    if (P.sched[i].e < H.nelem) T->cpos[P.sched[i].e] = (int)(i / SG_EQ_SLOTS) * 128 + 4 * (int)(i % SG_EQ_SLOTS);
}

// The element table as the batch uploads it (SgPhaseArgs::elem): the plan's fields and the derived ones behind them (enum SgElemDerived,
// sg_rows_layout.h).  The model blob and SgPlan::elem stay as they are; every kernel that indexes the plan's fields by f * nelem + e reads
// the same words as before.  Each derived value is one operation on doubles held in variables -- nothing a compiler could contract.
inline std::vector<double> sg_rows_elem_table(const SgPlan& P) {
  const int N = P.h.nelem;
  std::vector<double> t(P.elem);
  t.resize(sg_elem_table_doubles(N), 0.0);
  for (int e = 0; e < N; e++) {
    const double m = t[sg_elem_table_index(SGE_MASS, e, N)], arm = t[sg_elem_table_index(SGE_ARMATURE, e, N)];
    const double msum = m + arm;
    t[sg_elem_table_index(SGD_MSUM, e, N)] = msum;
    t[sg_elem_table_index(SGD_INVM, e, N)] = 1.0 / msum;
    if (P.h.nnb > 0)
      for (int d = 0; d < 3; d++) {
        const int e2 = P.nbtab[(size_t)d * N + e];   // out_e2[d][e], -1: no such row
        if (e2 >= 0) t[sg_elem_table_index(SGD_NBINVW + d, e, N)] = t[sg_elem_table_index(SGE_INVW, e, N)] + t[sg_elem_table_index(SGE_INVW, e2, N)];
      }
  }
  return t;
}

// Every buffer of SgWork with its element count, in one place: f(&w.member, count) for each, until one call returns false.  rounds =
// ceil(nelem / 64); legacy: the build has the split pipeline's solver (its contact records, 126 MB at 4096 envs, are otherwise not
// allocated).  SgWork::secprof is not here: it belongs to the batch, whichever pipeline runs.  A count of 0 is a buffer no kernel of
// this model touches (it still gets a pointer of its own).
template <class F>
bool sg_rows_work_each(SgWork& w, const SgPlanHeader& H, int rounds, size_t n, bool legacy, F&& f) {
  const size_t S = 2 * n, N = H.nelem;   // finger streams, elements
  const bool slim = SG_PHASE_SLIM(rounds);
  return f(&w.crec, legacy ? SG_CAP * ((n + SG_EPW - 1) / SG_EPW + 1) * SG_RF * SG_SPW : 0) &&   // [SG_CAP][nwb + 1][SG_RF][16]
         f(&w.ns, S) &&                                                       // [S]
         f(&w.crow, SG_ROW_INDEX(SG_CAP + 2, 0, 0, 0, (n + 7) / 8)) &&       // [SG_CAP + 2][nwb + 2][SG_RK / 2][64][2]
         f(&w.cdummy, sg_row_dummy_index((n + 3) / 4, 0)) &&               // [ceil(n / 4)][SG_RK / 2][64][2]
         f(&w.envh, SG_ENVH_ROWS * n) &&                                      // [SG_ENVH_ROWS][n]
         f(&w.shared, n) && f(&w.pending, n) && f(&w.status, n) && f(&w.iters, n) && f(&w.ncon, n) && f(&w.nefc, n) && f(&w.touch, n) &&   // [n]
         f(&w.sMinv, SGH_N_M * S) &&                                          // [16][S]
         f(&w.saF, SG_CD * S) &&                                              // [4][S]
         f(&w.lim_active, S) &&                                               // [S]
         f(&w.lim, SGH_N_LIM * S) &&                                          // [SG_LIM_ROWS][SG_MAXLIM][S]
         f(&w.as, n * N) && f(&w.eqf, n * N) && f(&w.eqb, n * N) && f(&w.eqR, n * N) && f(&w.asme, n * N) && f(&w.fsm, n * N) &&   // [n][N]
         f(&w.chh, n * 2 * SG_CHW) &&                                         // [n][2][SG_CHW]
         f(&w.nbf, n * (3 * N + 1)) && f(&w.nbb, n * (3 * N + 1)) && f(&w.nbR, n * (3 * N + 1)) &&   // [n][3 N] (+ 1 each)
         f(&w.cst, sg_rows_shape(H).cst_rounds ? SG_CST_INDEX((n + 3) / 4, 0, 0, H.eq_rounds + 8) : 0) &&   // [ceil(n / 4)][eq_rounds + 8][64][2]
         f(&w.gcon, n * SG_GEN_MAXCON * SG_GEN_W) &&                          // [n][SG_GEN_MAXCON][SG_GEN_W]
         f(&w.gen, n) &&                                                      // [n]
         f(&w.gen_count, 4) &&                                                // [1] (+ 3)
         f(&w.gen_list, n) &&                                                 // [n]
         f(&w.gpairs16, slim ? n * SG_PAIRS_CAP(4) : 0) &&                    // [n][SG_MAXCH * SG_CG * (4 * 64 + 2)]
         f(&w.gcval, slim ? n * SG_MAXCH * 64 : 0);                           // [n][SG_MAXCH][64]
}
