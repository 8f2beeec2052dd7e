// sg_rows_layout.h -- every layout the kernels of the rows pipeline share THROUGH MEMORY (sg_chain_kernel -> sg_phase_kernel -> sg_pgs_rows_kernel),
// written once: the contact-row block, the solver's LDS block, its table words, the equality block's export, the stream of step factors, the
// chain hand-off record and the per-stream / per-env arrays.  The kernels index by these functions and constants, sg_rows_host.h sizes and packs
// by them, and tests/emu/sg_rows_host_test.cpp runs the same functions over heap blocks of the host's sizes under the host sanitizers.
// Index functions and constants only -- no kernel code lives here, and a change of a rule here moves writer, reader, host and test together.
#pragma once
#include <cstddef>
#include <hip/hip_runtime.h>

#include "sg_math.h"

// ---- contact rows (SgWork::crow, written by the phase kernel's export, read and written by the solver's contact pass) ----
// A finger stream is a QUAD of lanes: lane r < 3 holds row r (normal, tangent 1, tangent 2) of every contact, lane 3 what the rows share;
// lane q also OWNS finger acceleration aF[q].  Block per (slot, wavefront): SG_RK / 2 field PAIRS x 64 lanes x 2 doubles, lane =
// 8 * env_in_wave + 4 * chain + r, so a lane fetches two fields with one 16-byte load.  Blocks nwb and nwb + 1 of every slot are dummies:
// lanes of envs that do not exist read block nwb (all zero, never written) and write to block nwb + 1.
#define SG_RK 16
enum SgRowField : int {     // of a row lane r < 3
  SGR_JF0 = 0, SGR_JF1, SGR_JF2, SGR_JF3,   // Jf[r][0..3]
  SGR_JS = 4, SGR_B = 5,                    // Js[r], b[r]
  SGR_F = 6, SGR_AF = 7,                    // f[r], (A f)[r]: one pair, the only fields the solver writes
  SGR_A0 = 8, SGR_A1, SGR_A2,               // A[r][0..2]
  SGR_IMJS = 11,                            // invm * Js[r]
  // W_k = M^-1 J_F[k]' (4 values per row k; lane q of the quad, the fourth included, keeps the q-th of each): the finger update
  // aF[q] += sum_k W_k[q] df_k is three multiply-adds on lane q after broadcasting the three force changes, instead of four more quad sums
  // and a 4 x 4 product on every lane
  SGR_W0 = 12, SGR_W1, SGR_W2,
  SGR_R = 15,                               // R, replicated on the row lanes (0 on the fourth)
};
enum SgQuadField : int {    // of the quad's fourth lane; every field not named here (and SGR_W0 .. SGR_W2, which it shares) is zero
  SGQ_P11 = 0, SGQ_P12, SGQ_P22,            // inverse friction block
  SGQ_SLIDER = 4,                           // slider index (an int in the double's low word)
  SGQ_E1 = 8, SGQ_E2, SGQ_COS, SGQ_SIN,     // the friction-scaled block S = Q diag(e1, e2) Q' (for the QCQP Newton iteration)
};
// (macros where a kernel passes a constant: the compiler folds them where they stand, a call it would fold a few passes later)
#define SG_ROW_PAIR(k) ((k) / 2)
#define SG_ROW_HALF(k) ((k) & 1)
__host__ __device__ constexpr int sg_row_pair(int field) { return SG_ROW_PAIR(field); }
__host__ __device__ constexpr int sg_row_half(int field) { return SG_ROW_HALF(field); }
#define SG_ROW_INDEX(slot, wave, k, lane, nwb) \
  ((((((size_t)(slot)) * ((nwb) + 2) + (wave)) * (SG_RK / 2) + SG_ROW_PAIR(k)) * 64 + (lane)) * 2 + SG_ROW_HALF(k))
// The solver walks a lane's column with ONE pointer per slot, biased to this pair, and reaches the eight pairs by immediate offsets
// (in 16-byte units from that pointer; a slot further on is sg_row_slot_stride)
constexpr int SG_ROW_BASE_PAIR = 4;
#define SG_ROW_IMM(k) ((SG_ROW_PAIR(k) - SG_ROW_BASE_PAIR) * 64)
__host__ __device__ constexpr int sg_row_imm(int field) { return SG_ROW_IMM(field); }
__host__ __device__ constexpr size_t sg_row_slot_stride(int nwb) { return (size_t)(nwb + 2) * (SG_RK / 2) * 64; }
// lanes without a contact stream read and write the private all-zero block of their wavefront (SgWork::cdummy, [wavefronts][SG_RK / 2][64][2])
__host__ __device__ constexpr size_t sg_row_dummy_index(size_t wave, int pair) { return (wave * (SG_RK / 2) + pair) * 128; }   // + 2 * lane
static_assert(sg_row_pair(SGR_F) == sg_row_pair(SGR_AF) && sg_row_half(SGR_F) == 0, "f and A f are one pair: the solver's one 16-byte write-back");
static_assert(SG_RK % 2 == 0 && sg_row_pair(0) == 0 && sg_row_pair(SG_RK - 1) == SG_RK / 2 - 1 && SGR_R == SG_RK - 1, "16 fields, pairs 0 .. SG_RK / 2 - 1");
static_assert(sg_row_imm(0) * 16 >= -4096 && sg_row_imm(SG_RK - 1) * 16 <= 4095, "every pair within a global load's 13-bit signed immediate offset");

// ---- the solver's instantiations: joint-fix rows per lane (template parameter NSL of sg_pgs_rows_kernel), ascending ----
#define SG_NSL_LIST(X) X(8) X(14) X(20) X(26) X(29) X(32)
__host__ __device__ constexpr int sg_rows_nsl(int nelem) {   // the instantiated NSL that holds nelem rows over an env's 8 lanes
#define SG_NSL_HOLDS(v) if (v * 8 >= nelem) return v;
  SG_NSL_LIST(SG_NSL_HOLDS)
#undef SG_NSL_HOLDS
  return 32;
}

// ---- the solver's LDS block, in doubles: regions in order, each one's offset the sum of the lengths before it ----
// Fix-only models, EPW envs per wavefront, joint-fix rows padded to NR = 8 * NSL per env (padding rows are neutral: b = 0, R = 1, 1 / (A + R) = 0):
//   AF [EPW][NR] pairs (a_s, f) -- the only pair written | BR [EPW][NR] pairs (b, R) | RI [EPW][NR] 1 / (A_jj + R_j) | IC [NR] pairs (1/m, tendon
//   coefficient), shared by the envs | ZERO: word 0 stays 0 (reads of "no slider"), word 1 + lane is that lane's write sink
// Neighbour-row models (EPW = 4), N elements, ROUNDS = H.eq_rounds, CST: the step factors stream from memory (SG_ROWS_NB_MODE 2):
//   AE [EPW][NA] slider accelerations (word N stays 0: "no partner"; padded to a 16-byte multiple) | GS [EPW][GW] row records: N + 1 groups of four
//   states g (CST) or four pairs (g, c) | TAB the schedule's table words, 16 lanes x (1 | 2) words per round, ROUNDS + 8 rounds | ZERO as above |
//   ENV [2][EPW]: the sum of an env's slider accelerations at the start, then its final offset aoff
// (Until r04 the step factors always sat beside g -- 70 KB for the ball's 218 elements, two workgroups per CU, i.e. the 1024 wavefronts of a
//  4096-env batch in TWO rounds; streamed in round-major order, SgWork::cst: 38 KB, four per CU, one round.)
// Each region starts where the one before it ends: its macro takes that region's start -- a pointer to doubles in the kernel (one 32-bit
// addition per region, as written out by hand before), a count of doubles on the host, from 0.
constexpr int SG_ROWS_LDS_SINK = 72;   // the ZERO region: 1 + 64 words, padded
#define SG_LDS_FIX_BR(AF, EPW, NR) ((AF) + (size_t)2 * (EPW) * (NR))
#define SG_LDS_FIX_RI(BR, EPW, NR) ((BR) + (size_t)2 * (EPW) * (NR))
#define SG_LDS_FIX_IC(RI, EPW, NR) ((RI) + (size_t)(EPW) * (NR))
#define SG_LDS_FIX_ZERO(IC, NR) ((IC) + (size_t)2 * (NR))
#define SG_LDS_FIX_END(ZERO) ((ZERO) + SG_ROWS_LDS_SINK)
#define SG_ROWS_NA_NB(N) (((N) + 2) & ~1)                         // words of an env's slider array
#define SG_ROWS_GW_NB(N, CST) (((CST) ? 4 : 8) * ((N) + 1))       // doubles of an env's row records
#define SG_LDS_NB_GS(AE, EPW, N) ((AE) + (size_t)(EPW) * SG_ROWS_NA_NB(N))
#define SG_LDS_NB_TAB(GS, EPW, N, CST) ((GS) + (size_t)(EPW) * SG_ROWS_GW_NB(N, CST))
#define SG_LDS_NB_ZERO(TAB, ROUNDS, CST) ((TAB) + (size_t)8 * ((CST) ? 1 : 2) * ((ROUNDS) + 8))
#define SG_LDS_NB_ENV(ZERO) ((ZERO) + SG_ROWS_LDS_SINK)
#define SG_LDS_NB_END(ENV, EPW) ((ENV) + (size_t)2 * (EPW))
#define SG_ROWS_LDS_FIX(EPW, NR) SG_LDS_FIX_END(SG_LDS_FIX_ZERO(SG_LDS_FIX_IC(SG_LDS_FIX_RI(SG_LDS_FIX_BR((size_t)0, EPW, NR), EPW, NR), EPW, NR), NR))
#define SG_ROWS_LDS_NB(EPW, N, ROUNDS, CST) SG_LDS_NB_END(SG_LDS_NB_ENV(SG_LDS_NB_ZERO(SG_LDS_NB_TAB(SG_LDS_NB_GS((size_t)0, EPW, N), EPW, N, CST), ROUNDS, CST)), EPW)
// the step factors stay in LDS beside the states (NB = 1) while four workgroups of the solver still share a CU's 160 KB that way
#define SG_ROWS_NB_MODE(N, ROUNDS) (sizeof(double) * SG_ROWS_LDS_NB(4, N, ROUNDS, 0) <= 40 * 1024 ? 1 : 2)

// ---- the solver's table words (SgPgsArgs::tab, staged into the TAB region) ----
// Lane 2 b + h of an env's 16-lane group holds, for the block e in slot b of a round, the byte offsets (x, y) of two slider words in the
// env's AE array -- sliders (e, p0) for h = 0 and (p1, p2) for h = 1 -- and where the lane's pair of row states sits in the env's GS array:
//   streamed step factors (NB = 2): ONE word   x | y << SG_TAB1_YSH | (2 e + h) << SG_TAB1_RSH    the pair of states in 16-byte units
//   step factors in LDS   (NB = 1): TWO words  x | y << SG_TAB2_YSH,  64 e + 32 h                   the byte offset of two 32-byte records
// (two words: halves and a plain word decode inside the address additions; the packed word costs four more integer instructions per round,
//  the 8 us per launch that r04 lost against r03 on one box, profiles/r05_ab_rounds.txt.  NB = 2 keeps it: its LDS block has no 2.5 KB to spare)
constexpr int SG_TAB1_YSH = 11, SG_TAB1_RSH = 22, SG_TAB2_YSH = 16;
__host__ __device__ constexpr unsigned sg_tab1_pack(unsigned sx, unsigned sy, unsigned e, unsigned h) { return (8u * sx) | ((8u * sy) << SG_TAB1_YSH) | ((2u * e + h) << SG_TAB1_RSH); }
__host__ __device__ constexpr unsigned sg_tab1_x(unsigned w) { return w & ((1u << SG_TAB1_YSH) - 1u); }
__host__ __device__ constexpr unsigned sg_tab1_y(unsigned w) { return (w >> SG_TAB1_YSH) & ((1u << (SG_TAB1_RSH - SG_TAB1_YSH)) - 1u); }
__host__ __device__ constexpr unsigned sg_tab1_rec(unsigned w) { return (w >> SG_TAB1_RSH) << 4; }
__host__ __device__ constexpr unsigned sg_tab2_pack(unsigned sx, unsigned sy) { return (8u * sx) | ((8u * sy) << SG_TAB2_YSH); }
__host__ __device__ constexpr unsigned sg_tab2_rec(unsigned e, unsigned h) { return 64u * e + 32u * h; }
__host__ __device__ constexpr unsigned sg_tab2_x(unsigned w) { return w & ((1u << SG_TAB2_YSH) - 1u); }
__host__ __device__ constexpr unsigned sg_tab2_y(unsigned w) { return w >> SG_TAB2_YSH; }
// what the narrowest field admits: an env's slider array -- nelem sliders, the zero word and a word of padding -- within reach of an
// 11-bit byte offset
constexpr int SG_ROWS_MAX_NELEM = (1 << SG_TAB1_YSH) / 8 - 2;
static_assert(SG_ROWS_MAX_NELEM == 254 && 2 * SG_ROWS_MAX_NELEM + 1 < (1 << (32 - SG_TAB1_RSH)) && SG_TAB1_RSH - SG_TAB1_YSH >= SG_TAB1_YSH &&
              8 * (SG_ROWS_MAX_NELEM + 2) <= (1 << SG_TAB2_YSH), "every field of a table word holds its largest value");

// ---- the solver's stream of step factors (SgWork::cst), in doubles: wavefront w (four envs), round k of its equality block, lane l ----
#define SG_CST_INDEX(w, k, l, rounds) ((((size_t)(w) * (rounds) + (k)) * 64 + (l)) * 2)

// ---- the equality block as the phase kernel exports it to the solver (neighbour-row models): element-major and dense, no look-up by row id ----
// Fix row of element e: SgWork::eqb / eqR [nenv][N]; its neighbour row d = 0 .. 2: SgWork::nbb / nbR [nenv][N][3]
__host__ __device__ constexpr size_t sg_eq_fix_index(size_t env, int e, int N) { return env * (size_t)N + (size_t)e; }
__host__ __device__ constexpr size_t sg_eq_nb_index(size_t env, int e, int d, int N) { return (env * (size_t)N + (size_t)e) * 3 + (size_t)d; }
// The solver stages an env's 4 (N + 1) row records in trips of 64 lanes: lane l of trip t holds row u = 4 e + d -- d = 0 the fix row of
// element e, d = 1 .. 3 its neighbour rows; group e = N is the idle slots' and stays zero, as does the padding behind it
__host__ __device__ constexpr int sg_eq_rec_trips(int nr) { return (4 * (nr + 1) + 63) / 64; }   // nr >= N: the instantiation's padded row count
__host__ __device__ constexpr int sg_eq_rec_row(int lane, int trip) { return lane + 64 * trip; }
__host__ __device__ constexpr bool sg_eq_rec_stored(int u, int N) { return u < 4 * (N + 1); }      // the row has a record in LDS
__host__ __device__ constexpr bool sg_eq_rec_live(int u, int N) { return u < 4 * N; }              // ... and is read from memory (else it is zero)
// where row u of an env is read from: the fix rows' array (d = 0) or the neighbour rows' -- clamped, so that every lane of every trip and
// every env slot of a ragged last wavefront forms an address inside the batch's arrays and the loads need no predicate
__host__ __device__ constexpr size_t sg_eq_rec_index(size_t env, int u, int N, size_t nenv) {
  const size_t envc = env < nenv ? env : nenv - 1;
  const int uc = u < 4 * N ? u : 4 * N - 1, e = uc >> 2, d = uc & 3;
  return d == 0 ? sg_eq_fix_index(envc, e, N) : sg_eq_nb_index(envc, e, d - 1, N);
}

// ---- the element table on the device (SgPhaseArgs::elem, SgPgsArgs::elem): SgPlan::elem's SGE_NFIELD fields of nelem doubles each, then the
// fields the HOST derives from them once per model (sg_rows_elem_table, sg_rows_host.h) -- per-model arithmetic the phase kernel redid for
// every element in every substep.  Each is ONE IEEE operation on table values, the operation the kernel performed: the bits are the kernel's
// (tests/emu/sg_phase_table_test.cpp).  Field f of element e is at f * nelem + e, as in SgPlan::elem.
enum SgElemDerived : int {
  SGD_MSUM = SGE_NFIELD,   // SGE_MASS + SGE_ARMATURE: the slider's 1 x 1 mass-matrix block
  SGD_INVM,                // 1 / SGD_MSUM (element 0's is the step factors' im0: equal masses, sg_plan_build)
  SGD_NBINVW,              // + d, d = 0 .. 2: SGE_INVW of e + SGE_INVW of the partner of e's d-th neighbour row; 0 where there is no such row
  SGD_NFIELD = SGD_NBINVW + 3
};
__host__ __device__ constexpr size_t sg_elem_table_index(int f, int e, int N) { return (size_t)f * (size_t)N + (size_t)e; }
__host__ __device__ constexpr size_t sg_elem_table_doubles(int N) { return (size_t)SGD_NFIELD * (size_t)N; }

// ---- chain hand-off record (SgWork::chh, SG_CHW doubles per stream): written by sg_chain_kernel's BEGIN, read by its FINISH and by the phase kernel ----
#define SG_CHW 160
enum { SGH_QSM = 0, SGH_QFRC = 4, SGH_ACTDOT = 8, SGH_M = 9, SGH_K = 25, SGH_MINV = 73, SGH_V = 89, SGH_W = 93, SGH_BOX = 97,
       SGH_LIMACT = 121, SGH_LIMSIGN = 122, SGH_LIMR = 130, SGH_LIMB = 138, SGH_LIMF = 146, SGH_END = 154 };
constexpr int SGH_N_M = SG_CD * SG_CD;                            // M, M^-1: the chain's 4 x 4 blocks
constexpr int SGH_N_K = (int)(sizeof(sgm::ChainKin) / sizeof(double));   // the chain's kinematics, as the struct lies in memory
constexpr int SGH_N_BOX1 = 3 + 9, SGH_N_BOX = SGH_N_BOX1 * SG_CG;        // per finger box: position, rotation
constexpr int SGH_N_LIM = 4 * SG_MAXLIM;                                 // sign | R | b | f of the limit rows, SG_MAXLIM each (enum SgLimRow)
struct SgHandoffField { int off, len; };
constexpr SgHandoffField SG_HANDOFF_FIELDS[] = {{SGH_QSM, SG_CD}, {SGH_QFRC, SG_CD}, {SGH_ACTDOT, 1}, {SGH_M, SGH_N_M}, {SGH_K, SGH_N_K}, {SGH_MINV, SGH_N_M},
                                                {SGH_V, SG_CD}, {SGH_W, SG_CD}, {SGH_BOX, SGH_N_BOX}, {SGH_LIMACT, 1}, {SGH_LIMSIGN, SG_MAXLIM},
                                                {SGH_LIMR, SG_MAXLIM}, {SGH_LIMB, SG_MAXLIM}, {SGH_LIMF, SG_MAXLIM}};
constexpr bool sg_handoff_tiles() {   // every field starts where the one before it ends, the last ends at SGH_END
  int at = 0;
  for (const SgHandoffField& f : SG_HANDOFF_FIELDS) {
    if (f.off != at || f.len <= 0) return false;
    at += f.len;
  }
  return at == SGH_END;
}
static_assert(SGH_N_K == 48 && sizeof(sgm::ChainKin) % sizeof(double) == 0, "ChainKin is 48 doubles: axes, anchors, body positions and rotations");
static_assert(sg_handoff_tiles() && SGH_END <= SG_CHW && SG_CHW % 2 == 0, "the hand-off fields tile [0, SGH_END) inside a record of 16-byte pairs");

// ---- per-stream and per-env arrays of SgWork: stream st = SG_STREAM(env, chain) of S = 2 nenv ----
enum SgEnvhRow : int { SG_ENVH_TB, SG_ENVH_TR, SG_ENVH_TA, SG_ENVH_TF, SG_ENVH_ROWS };   // the tendon row: b, R, A, f
enum SgLimRow : int { SG_LIM_SIGN, SG_LIM_R, SG_LIM_B, SG_LIM_F, SG_LIM_ROWS };          // in the hand-off record's order
static_assert(SGH_LIMSIGN + SG_LIM_R * SG_MAXLIM == SGH_LIMR && SGH_LIMSIGN + SG_LIM_B * SG_MAXLIM == SGH_LIMB && SGH_LIMSIGN + SG_LIM_F * SG_MAXLIM == SGH_LIMF &&
              SG_LIM_ROWS * SG_MAXLIM == SGH_N_LIM, "SgWork::lim is the hand-off record's limit block, value by value");
// (macros: a kernel's index expression stands where it is used, as it did when it was written out by hand)
#define SG_STREAM(env, chain) (2 * (size_t)(env) + (chain))                                   // ns, lim_active: [S]
#define SG_ENVH_INDEX(row, env, nenv) ((size_t)(row) * (nenv) + (env))                        // envh: [SG_ENVH_ROWS][nenv]
#define SG_MINV_INDEX(i, st, S) ((size_t)(i) * (S) + (st))                                    // sMinv: [SGH_N_M][S], i = 4 row + column
#define SG_SAF_INDEX(d, st, S) ((size_t)(d) * (S) + (st))                                     // saF: [SG_CD][S]
#define SG_LIM_INDEX(row, k, st, S) (((size_t)(row) * SG_MAXLIM + (k)) * (S) + (st))          // lim: [SG_LIM_ROWS][SG_MAXLIM][S]
#define SG_LIM_FLAT_INDEX(i, st, S) ((size_t)(i) * (S) + (st))                                // ... by i = SG_MAXLIM row + k
static_assert(SG_LIM_INDEX(SG_LIM_F, SG_MAXLIM - 1, 5, 7) == SG_LIM_FLAT_INDEX(SGH_N_LIM - 1, 5, 7), "the two views of SgWork::lim");
