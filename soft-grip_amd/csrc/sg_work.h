// sg_work.h -- what the kernels of the two-finger class share: the batch's device work space (SgWork), the kernel argument blocks
// and the LAUNCHERS; the layouts of what the kernels pass each other through that work space are sg_rows_layout.h's.
//
// One translation unit per kernel family -- sg_phase.hip (sg_chain_kernel, sg_phase_kernel), sg_rows.hip (sg_pgs_rows_kernel: the
// solver), sg_tree.hip (the tree pipeline) and, in test builds only (-DSG_LEGACY_PIPELINES), sg_legacy.hip (r01's fused and split
// pipelines, kept as cross-checks) -- compiled side by side; sg_api.hip (the C ABI) sees the launchers below and nothing else, and sizes and fills what they take through sg_rows_host.h.
// A substep of the rows pipeline is the chain   chain -> phase(finish + begin) -> [general pass] -> pgs_rows.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/softgrip.h"
#include "sg_math.h"
#include "sg_general.h"
#include "sg_rows_layout.h"

using namespace sgm;

#define SG_CAP 64        // contact capacity per stream in the split pipeline
#define SG_NF 26         // constant fields of a contact record
#define SG_RF 30         // record fields: 26 constants, 3 force components, slider index (as an int in a double slot)
// Contact records are blocked for the PGS kernel: one block per (slot, PGS wavefront) holds SG_RF fields x SG_SPW streams,
// so a wavefront reads a whole record with ONE vector address plus immediate offsets (field stride 128 B), and its 16
// stream lanes use every byte of the 128-B lines they touch.  Block index nwb (one past the last wave) is a dummy
// target for the unconditional stores of idle lanes.
#define SG_REC_INDEX(slot, wave, field, pos, nwb) (((((size_t)(slot)) * ((nwb) + 1) + (wave)) * SG_RF + (field)) * SG_SPW + (pos))
#define SG_G 8           // lanes per env in the PGS kernel (8 measured best: 16 -> 1.35x slower PGS, 4 -> 1.07x slower)
#define SG_EPW (64 / SG_G)   // envs per PGS wavefront
#define SG_SPW (2 * SG_EPW)  // finger streams per PGS wavefront
#define SG_GEN_GRID 256  // blocks of the general contact pass (they stride over the listed envs: no limit on how many there are)

struct SgWork {          // device workspace of one batch (all pointers device memory; every member's element count: sg_rows_work_each, sg_rows_host.h)
  double* crec;          // [SG_CAP][nwb + 1][SG_RF][16]   nwb = ceil(nenv / 8) PGS wavefronts (+1 dummy block)
  unsigned long long* secprof;  // [32] cycle sums per kernel section (only written when built with -DSG_SECTION_PROF)
  double* crow;          // [SG_CAP + 2][nwb + 2][SG_RK / 2][64][2]   row layout (sg_pgs_rows_kernel), +2 dummy blocks
  double* cdummy;        // [ceil(nenv / 4)][SG_RK / 2][64][2]  one private all-zero block per PGS wavefront for its lanes without an env
  int* ns;               // [S]
  double* envh;          // [4][nenv]: tb, tR, tA, tf
  int *shared, *pending, *status, *iters, *ncon, *nefc, *touch;  // [nenv]
  double *sMinv, *saF;   // [16][S], [4][S]
  int* lim_active;       // [S]
  double* lim;           // [4][SG_MAXLIM][S]: sign, R, b, f
  double *as, *eqf, *eqb, *eqR;  // [nenv][N]  slider accelerations; the fix rows' force, right-hand side b, regulariser R.  Neighbour-row models on the
                         // rows pipeline (SgPhaseArgs::rowlayout, H.nnb > 0) hand the solver its rows READY instead (sg_eq_fix_index): eqb = the row's
                         // state g0 = b + R f of the final warm-start force, eqR = its step factor c0 = (1/m) / (1/m + R) -- eqR only where the solver
                         // keeps the factors in LDS (SG_ROWS_NB_MODE 1; mode 2 streams them from cst and eqR is not written) -- and eqf is not written
  double *asme, *fsm;    // [nenv][N]  begin -> finish hand-off
  double* chh;           // [nenv][2][SG_CHW]  chain hand-off (enum SGH_*)
  double *nbf, *nbb, *nbR;  // [nenv][3 N]  neighbour equality rows (models with H.nnb > 0) by slot (SgPlan::nbtab): force, right-hand side, regulariser.
                         // Rows pipeline: nbf as said (the phase kernel gathers from it by row id); nbb and nbR are element-major and dense,
                         // [nenv][N][3] (sg_eq_nb_index): nbb = g_d = b + R f of element e's d-th neighbour row, nbR = c_d = (1/m) / (2/m + R)
                         // (mode 1 only, as eqR); a row that does not exist holds 0 in both
  double* cst;           // [ceil(nenv / 4)][eq_rounds + 8][64][2]  step factors c = (1/m) / (A + R) of the equality rows in the SOLVER's order: what lane l of
                         // wavefront w reads in round k of its equality block (SG_CST_INDEX); written by the phase kernel, zero where a slot / row is idle
  double* gcon;          // [nenv][SG_GEN_MAXCON][SG_GEN_W]  contacts of envs on the general contact path (sg_general.h), in mj_collision's order
  int* gen;              // [nenv]  number of general contacts of the pending substep (0: the env is on the fast path)
  int* gen_count;        // [1]  envs the main phase pass has put on gen_list in this substep (reset by sg_chain_kernel)
  int* gen_list;         // [nenv]
  // models of four element rounds (193 .. 256 sliders: the ball): the phase kernel's pair list and per-slot slider pushes, which its smaller
  // instantiations keep in LDS (Smem2): without them its block is 19.5 KB instead of 22.6 -- EIGHT workgroups per CU, the 4096 wavefronts in two rounds
  // instead of three (a round is ~60 us whatever its size: profiles/r05s_phase_kernel_occupancy.txt)
  unsigned short* gpairs16;  // [nenv][SG_MAXCH * SG_CG * (4 * 64 + 2)]   (2 entries otherwise)
  double* gcval;             // [nenv][SG_MAXCH][64]                       (2 entries otherwise)
};

struct SgPhaseArgs {
  const SgPlanHeader* H;
  const double* elem;
  double *qpos, *qvel, *warm, *act, *ctrl;
  const double* kenv;
  const int *kmask_jnt, *kmask_ten;
  const unsigned char* mask;
  double* sens;
  long long sens_stride;
  SgWork w;
  int nenv;
  int do_reset, do_finish, finish_integrate, do_begin, first;
  int rowlayout;  // 1: export contact records in the row layout of sg_pgs_rows_kernel
  const int* nbtab;  // SgPlan::nbtab (neighbour rows per element), nullptr when H.nnb == 0
  const int* cpos;   // neighbour-row models: per element, where the four step factors of its equality block sit in a wavefront's round-major
                     // stream W.cst (doubles: round * 128 + 4 * block slot); the host derives it from SgPlan::sched (sg_rows_tables)
  int cst_rounds;    // eq_rounds + 8: rounds of W.cst per solver wavefront; 0: the solver keeps the factors in LDS (SG_ROWS_NB_MODE 1), nothing to write
  const SgGenPair* gpairs;  // SgPlan::gpairs (the general contact path's candidate pairs)
  // copies of the plan header's sizes, by value: the kernels' first addresses then do not wait for a load from *H
  int nelem, nv, nu, elem_dof0, nchain, t0_id;
  double timestep;
};

// The solver's look-ahead over a wavefront's contact slots 0 .. nsmax - 1 (sg_rows.hip, the contact pass): while slot i is updated the rows
// of slot i + ahead are loaded into registers -- or nothing is (-1) where that slot is past the end of the wavefront's longest stream.
// Whatever (i, ahead) a caller passes, a slot that comes back lies in [0, nsmax - 1] (tests/test_rows_touch_index.py).
__host__ __device__ constexpr int sg_rows_load_slot(int i, int ahead, int nsmax) { return i + ahead < nsmax ? i + ahead : -1; }

struct StageRec2 {
  double dist, pos[3], n[3];
  int sl, box;
};

struct ChainLds2 {  // what the phase kernel needs of a finger chain (imported from sg_chain_kernel's hand-off record)
  double v[SG_CD], w[SG_CD], qacc_smooth[SG_CD], Minv[16];
  int lim_active, pad;
  double lim_sign[SG_MAXLIM], lim_R[SG_MAXLIM], lim_b[SG_MAXLIM], lim_f[SG_MAXLIM];  // contiguous, in the hand-off record's order
};
// (the phase kernel imports SGH_LIMSIGN .. and exports SgWork::lim as ONE run of SGH_N_LIM doubles from lim_sign on)
static_assert(offsetof(ChainLds2, lim_R) - offsetof(ChainLds2, lim_sign) == (SGH_LIMR - SGH_LIMSIGN) * sizeof(double) &&
              offsetof(ChainLds2, lim_b) - offsetof(ChainLds2, lim_sign) == (SGH_LIMB - SGH_LIMSIGN) * sizeof(double) &&
              offsetof(ChainLds2, lim_f) - offsetof(ChainLds2, lim_sign) == (SGH_LIMF - SGH_LIMSIGN) * sizeof(double), "ChainLds2's limit rows lie as the hand-off record's");

#define SG_PHASE_SLIM(R) ((R) >= 4)   // the pair list and the slot pushes live in the work space (SgWork::gpairs16, gcval), not in LDS
#define SG_PAIRS_CAP(R) (SG_MAXCH * SG_CG * ((R) * 64 + 2))
#define SG_PHASE_LDS_BUDGET (160 * 1024 / 8)   // bytes of LDS per workgroup at eight workgroups per CU (two wavefronts per SIMD)
// the neighbour rows' warm-start forces by row id (< 3 nelem) also live in LDS, for the gather of recompute_a: where the block stays within the
// budget with them -- one and two element rounds (the box: 20 064 bytes); three and four (cylinder, ball) gather from the work space
#define SG_PHASE_NBF_LDS(R, NB) ((NB) && (R) <= 2)
template <int R, int CPL, bool NB>
struct Smem2 {
  ChainKin K[SG_MAXCH];
  ChainLds2 cs[SG_MAXCH];
  double boxp[SG_MAXCH * SG_CG][3], boxm[SG_MAXCH * SG_CG][9];
  double ve[R * 64], asme[R * 64], we[R * 64], as[R * 64];
  StageRec2 stage[SG_MAXCH][32 * CPL];
  unsigned short pairs[SG_PHASE_SLIM(R) ? 4 : SG_PAIRS_CAP(R)];  // broadphase survivors, (box << 12) | element, in contact order
  unsigned char eslot[R * 64][SG_MAXCH * SG_CG];          // per element and box: first contact slot (< 64) | (contact count << 6)
  double cval[SG_PHASE_SLIM(R) ? 1 : SG_MAXCH * 32 * CPL];   // per contact slot [chain][32 CPL]: invm * Js' f (its push on the slider)
  double nbf[SG_PHASE_NBF_LDS(R, NB) ? 3 * R * 64 : 1];      // neighbour rows' warm-start forces by row id (SG_PHASE_NBF_LDS)
};
#define SG_PAIR_CENTER 0xFFF  // element code of the object's centre sphere

__device__ __forceinline__ double wave_sum2(double x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
  return x;
}
__device__ __forceinline__ int lanes_below2(unsigned long long m) {
  return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0));
}

#if defined(__HIP_DEVICE_COMPILE__)
#define SG_CONSTAS __attribute__((address_space(4)))   // (the host pass of the same source has no address spaces to convert between)
#else
#define SG_CONSTAS
#endif

// section timing for scripts/section_profile.py (build_native.py --prof): every wavefront sums the cycles between stamps per
// section in registers and adds them to W.secprof[] once, at its end.  Compiled out of the product library.
#ifdef SG_SECTION_PROF
#define SG_T0() unsigned long long t_prev_ = __builtin_readcyclecounter(), t_acc_[26] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}
#define SG_T(k)                                                   \
  do {                                                            \
    unsigned long long t_now_ = __builtin_readcyclecounter();     \
    t_acc_[k] += t_now_ - t_prev_;                                \
    t_prev_ = __builtin_readcyclecounter();                       \
  } while (0)
#define SG_TEND()                                                 \
  do {                                                            \
    if (threadIdx.x == 0)                                         \
      for (int k_ = 0; k_ < 26; k_++)                             \
        if (t_acc_[k_]) atomicAdd(&a.w.secprof[k_], t_acc_[k_]);  \
  } while (0)
#else
#define SG_T0()
#define SG_T(k)
#define SG_TEND()
#endif


struct SgPgsArgs {
  const unsigned* tab;       // the schedule as the solver's LDS table words (lane 2 b + h of a 16-lane group, block slot b; sg_rows_tables)
  const SgEqSlot* sched;  // SgPlan::sched (equality-row schedule of neighbour-row models), nullptr when H.nnb == 0
  const int* nbtab;       // SgPlan::nbtab
  const SgPlanHeader* H;
  const double* elem;
  SgWork w;
  int nenv;
};

// ---- launchers (defined next to their kernels) ----
hipError_t sg_launch_chain(const SgPhaseArgs& p, int nenv, hipStream_t s);
// the main pass over all envs and, when genpass, the general contact pass behind it (SG_GEN_GRID blocks striding over the listed envs; sg_general.h)
hipError_t sg_launch_phase(const SgPhaseArgs& p, int rounds, bool nb, bool genpass, int nenv, hipStream_t s);
hipError_t sg_rows_prepare();                 // once per device: dynamic-LDS limits of every solver instantiation
hipError_t sg_launch_rows(const SgPgsArgs& a, int nsl, int nb /* 0 | 1 | 2: template parameter NB of sg_pgs_rows_kernel */, int epw, int nenv, size_t lds_bytes, hipStream_t s);
#ifdef SG_LEGACY_PIPELINES   // test builds only (build_native.py --legacy): r01's fused kernel and the split pipeline's stream-per-lane solver
struct SgKArgs;
hipError_t sg_legacy_prepare();
hipError_t sg_launch_pgs_split(const SgPgsArgs& a, int nenv, size_t lds_bytes, hipStream_t s);
hipError_t sg_launch_fused(const SgKArgs& a, int rounds, int nenv, hipStream_t s);
#endif
