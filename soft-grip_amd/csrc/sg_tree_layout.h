// sg_tree_layout.h -- what the tree pipeline keeps where (part of sg_tree.h): capacities, the launch arguments, the records' field
// names, the env's LDS block and work space (lds_carve) and the sizes and offsets everything else derives from them.
#pragma once
#if defined(SGT_EMU_SEPARATE)
#include <stdlib.h>

#include <utility>
#include <vector>
#endif

namespace sgt {
using namespace sgm;

#ifndef SGT_DIET
#define SGT_DIET 0x1ff   // which groups of arrays live in the env's work space instead of LDS (lds_carve): bits 0 - 5 the build-only groups,
                         // 6 M^-1, 7 the sliders' 1 / m (scenes without a free object), 8 the capsule centres of a free object's scene.
                         // All set: 37 KB of LDS for the four-finger scene, FOUR workgroups per CU (129 against 94 k env-steps/s with
                         // M^-1 and 1 / m in LDS, r04v profile)
#endif
#define SGT_MAXCON 128   // contacts of an env
#define SGT_MAXHIT 256   // candidate pairs that pass the bounding tests
#define SGT_HITREC 8     // contacts one pair can produce (box - box)
#define SGT_RECW 10      // doubles of a staged narrowphase record: dist, pos[3], n[3], tangent hint[3]
#define SGT_LDS_HEADER 2   // doubles at the head of the env's LDS block (lds_carve)
#define SGT_CSC 56       // scalar doubles of a contact record in the work space
#define SGT_LROW 6       // doubles of a chain limit row: dof, sign, R, b, f, 1 / (A + R)
#ifndef SGT_LROW_AHEAD
#define SGT_LROW_AHEAD 4 // register sets of the sweep's chain-limit-row pass (lookahead + 1).  8 measured: four-finger 196.6 -> 193.0 k, free ball 51.7 -> 49.8 k (r05 t9)
#endif

struct TreeArgs {
  const SgPlanHeader* H;
  const SgTreeDev* T;
  const double* elem;        // SgPlan::elem (SoA over elements)
  const SgGenPair* gpairs;
  const SgEqSlot* sched;     // neighbour-row models: SgPlan::sched (eq_rounds x 64 blocks) and SgPlan::nbtab (out_e2 | out_slot | in_slot, [3][N] each)
  const int* nbtab;
  double *qpos, *qvel, *warm, *act, *ctrl;   // [n][nq] / [n][nv], [n][nu]
  const double* kenv;
  const int *kmask_jnt, *kmask_ten;
  const unsigned char* mask;  // mode 1: envs to reset (nullptr = all)
  double* sens;
  long long sens_stride;
  int *flags, *touch, *touch_words, *ncon, *nefc, *iters;   // touch_words: [n][2], bit g = finger box g touches an object geom
  double* cws;               // per-env work space, cws_stride doubles each
  long long cws_stride;
  int nenv, nsub, mode;      // mode 1: reset + one forward without integration, then nsub steps
  unsigned long long* secprof;   // profiling build (-DSG_SECTION_PROF) only: cycle sums per section, else unused
};

// work-space layout (doubles): staged narrowphase records | contact rows | the chains' mass-matrix blocks | the arrays lds_carve backs with
// global memory.  Where the parts begin, from `at` = the env's first double (a pointer) or 0 (an offset): for the stage frame, the sweep,
// cws_doubles and the emulation's layout dump alike.  (Macros: as forced-inline functions they changed the code of tree_sweep and of
// the finish stage -- the compiler folds the sums into its addresses differently -- and this kernel's code is not moved, sg_tree_frame.inc)
SG_HD long long cws_row_doubles(int CS) { return 12LL * CS + SGT_CSC; }   // 2 blocks x (J, W) x 3 rows x CS + scalars
#define SGT_CWS_ROWS(at) ((at) + (size_t)SGT_MAXHIT * SGT_HITREC * SGT_RECW)                          // the contact rows [SGT_MAXCON][cws_row_doubles]
#define SGT_CWS_MASS(rows, CW) ((rows) + (size_t)SGT_MAXCON * (CW))                                   // from the contact rows on: the mass-matrix blocks [K][CS][CS], identity-padded; CW = cws_row_doubles(CS)
#define SGT_CWS_CARVE(at, CW, NMAT) (SGT_CWS_MASS(SGT_CWS_ROWS(at), CW) + (NMAT))                      // lds_carve's gbase

// scalar part of a contact record
enum { CS_A = 0, CS_B = 6, CS_F0 = 9, CS_R = 12, CS_INVM = 13, CS_JS = 14, CS_SL = 17, CS_C1 = 18, CS_N1 = 19, CS_C2 = 20, CS_N2 = 21,
       CS_ROWS = 22, CS_TOUCH = 23, CS_OBJ = 24 /* the contact touches the free object */, CS_JO = 25 /* [3][6]: its rows on the object's free dofs, body frame */,
       CS_TMP = 43 /* [12]: between the phases of the rows' build: J v, J a_smooth, J a_warm, body invweights, blocks, distance */,
       CS_PE = 43 /* [7], once the rows are built (the temporaries are done with): the friction block's inverse and eigen-decomposition, contact_block_constants */ };
// the free object's block in LDS (S.of[..]); body frame unless said otherwise
enum { OF_P = 0, OF_Q = 3, OF_R = 7, OF_VW = 16 /* world */, OF_VL = 19, OF_WL = 22 /* (v, w) contiguous */, OF_WARM = 25, OF_ASM = 31, OF_AF = 37, OF_GF = 43, OF_SINV = 49,
       OF_CEN = 85 /* world */, OF_GL = 88, OF_CTEN = 91, OF_BIAS = 97, OF_X = 103, OF_Y = 109, OF_WB = 115 /* OF_WARM: dof coordinates (world translations), kept
       across substeps; OF_WB: the same in the body frame of this substep */, OF_MFF = 121 /* upper triangle of M_ff, 21 */, OF_TMP = 142, OF_N = 160 };

struct Lds {
  double *q, *v, *warm, *asm_, *aF, *fs, *fc, *bias, *tenJ, *kd, *qacc;
  double *xpos, *xmat, *xipos, *ximat, *bw, *bal, *ba, *bf, *bn;
  double *anchor, *axis, *gpos, *gmat, *gsz, *spos;
  double *L, *Minv, *tmpP;
  double *qe, *ve, *we, *asme, *ae, *fse, *ffix, *bfix, *Rfix, *flim, *blim, *Rlim, *ke;
  double *einvm, *ecoef, *ecen, *Ifix, *Ilim;   // 1 / (m + armature), tendon coefficient, capsule centres [3][N], 1 / (A + R) of the fix / limit rows
  double *lrow, *seg, *chs, *cf, *red, *swc, *ctx;   // swc: the step's scalars for the sweep function (SWC_*); ctx: those the stage functions hand on (CTX_*)
  double *nbf, *nbb, *nbR, *nbI, *nbA;   // neighbour equality rows by slot d * N + e (the d-th row registered for element e): force, b, R, 1 / (A + R); free object: A + R
  double *nbq, *fixq;   // grippers with neighbour rows (no free object): the rows' sweep constants PACKED for the pipelined equality rounds of tree_sweep -- nbq[4 k] = R, b, 1 / (A + R), 1 / m of the partner; fixq[4 e] = b, R, 1 / (A + R), 1 / m of the fix row
  double *frow;   // free object: the joint-fix rows' constants for the serial sweep, [N][5]: b, R, A + R, 1 / (A + R), 1 / D
  double *of, *Be, *Ce, *Afix;   // free object (plans with has_free): scalars (OF_*), B_e [N][6], C_e = -S^-1 B_e / D_e [N][6], the fix rows' diagonals A + R
  int *hit_pair, *hit_sorted, *hit_cnt, *hit_off, *con_src, *con_chain, *icnt;
  double* csc;   // LDS copies of the first `ncache` contacts' scalar records (the sweeps read them 30 times; the rest stay in the work space)
  int ncache;
};
enum { IC_NHIT = 0, IC_NCON, IC_SERIAL, IC_NLIVE, IC_NPURE, IC_NLIM0 /* + chain */, IC_NLEV = IC_NLIM0 + SGT_MAXCH /* levels of the contact schedule */, IC_N };
static_assert(IC_N <= 32, "S.icnt holds 32 counters");
// per-chain scalars in LDS (chs[c * CHS_N + ..])
enum { CHS_TLEN = 0, CHS_TVEL, CHS_TFRC, CHS_AFRC, CHS_ACTDOT, CHS_ACT, CHS_CTRL, CHS_KT, CHS_N };

// scalars the sweep takes from / hands back to the step (S.swc, in LDS: uniform reads)
enum { SWC_TEN_R = 0, SWC_TEN_B, SWC_TEN_F, SWC_TJ_A, SWC_TEN_I, SWC_CTEN, SWC_NCON = SWC_CTEN + 6, SWC_SERIAL, SWC_ITERS, SWC_N = 16 };
// the step's scalars the stage functions hand on (S.ctx)
enum { CTX_FLAGS = 0, CTX_NCON, CTX_NEFC, CTX_ITERS, CTX_TLO, CTX_THI, CTX_STOP, CTX_LAST, CTX_INTEGRATE, CTX_SUB, CTX_N = 16 };

// The env's arrays.  base: its LDS block; gbase: the part of its work space that backs the arrays only their own lane (or a later
// phase behind a barrier) touches -- the L'DL blocks, the sliders' sweep constants and build-only state: 35 KB of the four-finger
// scene's 113 KB, which is what lets two workgroups share a CU's LDS (the loads are coalesced and L2-resident).  Returns the LDS
// bytes; *gdoubles the doubles taken from gbase.
#if !SGT_DEVICE && defined(SGT_EMU_SEPARATE)
// Host emulation, checking build (tests/emu, `make sep`): every array of the carve is a heap block of its own, EXACT in size, so that
// AddressSanitizer sees an access one element past ANY array -- inside the env's one LDS block / work space such an access lands in the
// neighbouring array and shows, if at all, as a wrong number on some other layout.  The driver owns the pool (blocks are handed out in
// the carve's order, the same on every call) and poisons the LDS-class blocks before a launch.
struct SepPool { std::vector<std::pair<void*, size_t>> lds, glob; size_t il = 0, ig = 0; double* part[3] = {nullptr, nullptr, nullptr}; };   // part: staged records, contact rows, mass-matrix blocks
inline SepPool*& sep_pool() { static SepPool* p = nullptr; return p; }
inline double* sep_part(int k, size_t n) { SepPool* sp = sep_pool(); if (!sp->part[k]) sp->part[k] = (double*)calloc(n ? n : 1, sizeof(double)); return sp->part[k]; }
inline void* sep_take(std::vector<std::pair<void*, size_t>>& v, size_t& i, size_t bytes) {
  if (i == v.size()) v.push_back({calloc(bytes ? bytes : 1, 1), bytes});
  if (v[i].second != bytes) abort();   // (the carve's order and sizes are a function of the model alone)
  return v[i++].first;
}
#endif
SG_HD size_t lds_carve(Lds& L, double* base, const SgTreeDev& T, int N, int has_free, double* gbase, size_t* gdoubles, int nnb = 0, size_t* used_out = nullptr) {
  L = Lds();   // (every pointer null until assigned: an array the carve forgets faults on the host emulation instead of reading the stack's leftovers)
  double *p = base + SGT_LDS_HEADER, *g = gbase;   // (the block's first words: the launch's argument segment for the called stages, sg_tree_frame.inc)
#if !SGT_DEVICE && defined(SGT_EMU_SEPARATE)
  SepPool* const sp = (base != reinterpret_cast<double*>((uintptr_t)4096)) ? sep_pool() : nullptr;   // (the sizing calls carve from address 4096)
  if (sp) sp->il = sp->ig = 0;
  auto take = [&](size_t n) { double* r = p; p += (n + 1) & ~(size_t)1; return sp ? (double*)sep_take(sp->lds, sp->il, n * sizeof(double)) : r; };
  auto takeg = [&](size_t n) { double* r = g; g += (n + 1) & ~(size_t)1; return sp ? (double*)sep_take(sp->glob, sp->ig, n * sizeof(double)) : r; };
#else
  auto take = [&](size_t n) { double* r = p; p += (n + 1) & ~(size_t)1; return r; };
  auto takeg = [&](size_t n) { double* r = g; g += (n + 1) & ~(size_t)1; return r; };
#endif
  const int ND = T.ND, NB = T.NB;
  // r04: LDS holds what the SWEEP touches (accelerations, forces, limit rows) and what the PAIR WALK touches (capsule centres, box poses);
  // everything only the once-per-substep build stages read or write -- kinematics, body poses and RNE temporaries, the sliders' state,
  // tendon segments, M^-1 (whose rows the sweep prefetches) -- sits in the env's work space (coalesced, L2 / Infinity-Cache resident):
  // 37.5 KB instead of 76 for the four-finger scene, i.e. FOUR workgroups per CU (one per SIMD) instead of two
  auto tk = [&](int bit, size_t n) { return (SGT_DIET >> bit) & 1 ? takeg(n) : take(n); };   // (SGT_DIET: which groups live in the work space)
  L.q = take(ND); L.v = take(ND); L.warm = take(ND); L.asm_ = take(ND); L.aF = take(T.K * T.CS);   // (read joint by joint by the one-lane-per-chain stages: LDS)
  L.fs = tk(0, ND); L.fc = tk(0, ND); L.bias = tk(0, ND); L.tenJ = tk(0, ND); L.kd = tk(0, ND); L.qacc = tk(0, ND);
  L.xpos = tk(1, 3 * NB); L.xmat = tk(1, 9 * NB); L.xipos = tk(1, 3 * NB); L.ximat = tk(1, 9 * NB); L.bw = tk(1, 3 * NB);
  L.bal = tk(1, 3 * NB); L.ba = tk(1, 3 * NB); L.bf = tk(1, 3 * NB); L.bn = tk(1, 3 * NB);
  L.anchor = tk(2, 3 * ND); L.axis = tk(2, 3 * ND); L.gpos = take(3 * T.NG); L.gmat = take(9 * T.NG); L.gsz = take(3 * T.NG); L.spos = tk(2, 3 * T.NS);
  L.L = takeg(T.NMAT); L.Minv = tk(6, T.NMAT); L.tmpP = tk(3, T.K * T.CS);   // (M^-1: the sweep's limit rows prefetch its rows, W = J M^-1 reads it lane = word)
  L.qe = takeg(N); L.ve = tk(4, N); L.we = tk(4, N); L.asme = tk(4, N); L.ae = take(N); L.fse = takeg(N); L.ffix = take(N);
  L.bfix = takeg(N); L.Rfix = takeg(N); L.flim = take(2 * N); L.blim = takeg(2 * N); L.Rlim = takeg(2 * N); L.ke = takeg(N);
  // 1 / m: in registers for the sweeps (the free object's serial rows read it per contact: LDS there).  The capsule centres: LDS for the pair
  // walk -- but a free object's scene has few candidate pairs and its own LDS arrays (B_e, C_e, the rows' constants): work space there
  L.einvm = has_free ? take(N) : tk(7, N); L.ecoef = takeg(N);
  L.ecen = (has_free && ((SGT_DIET >> 8) & 1)) ? takeg(3 * N) : take(3 * N);
  L.Ifix = takeg(N); L.Ilim = takeg(2 * N);
  L.lrow = take(SGT_LROW * 2 * ND); L.seg = tk(5, 4 * T.K * SGT_MAXTS); L.chs = tk(5, CHS_N * SGT_MAXCH); L.cf = take(3 * SGT_MAXCON);
  L.red = take(16); L.swc = take(16); L.ctx = take(16);
  L.of = take(has_free ? OF_N : 0); L.Be = take(has_free ? 6 * N : 0); L.Ce = take((has_free && nnb) ? 6 * N : 0); L.Afix = takeg(has_free ? N : 0);   // (C_e: kept for the neighbour-row blocks only -- the plain rows recompute it, free_fix_rows)
  L.frow = take(has_free ? 4 * N : 0);
  L.nbf = takeg(nnb ? 3 * N : 0); L.nbb = takeg(nnb ? 3 * N : 0); L.nbR = takeg(nnb ? 3 * N : 0); L.nbI = takeg(nnb ? 3 * N : 0);
  L.nbA = takeg((nnb && has_free) ? 3 * N : 0);
  L.nbq = takeg((nnb && !has_free) ? 12 * N : 0); L.fixq = takeg((nnb && !has_free) ? 4 * N : 0);
  if (gdoubles) *gdoubles = (size_t)(g - gbase);
  int* ip = (int*)p;
  L.hit_pair = ip; ip += SGT_MAXHIT;
  L.hit_sorted = ip; ip += SGT_MAXHIT;
  L.hit_cnt = ip; ip += SGT_MAXHIT;
  L.hit_off = ip; ip += SGT_MAXHIT;
  L.con_src = ip; ip += SGT_MAXCON;
  L.con_chain = ip; ip += SGT_MAXCON;
  L.icnt = ip; ip += 32;
#if !SGT_DEVICE && defined(SGT_EMU_SEPARATE)
  if (sp) {
    auto takei = [&](size_t n) { return (int*)sep_take(sp->lds, sp->il, n * sizeof(int)); };
    L.hit_pair = takei(SGT_MAXHIT); L.hit_sorted = takei(2 * SGT_MAXHIT); L.hit_cnt = L.hit_sorted + SGT_MAXHIT; L.hit_off = takei(SGT_MAXHIT);   // (hit_sorted + hit_cnt: ONE array to the pair walk's block lists)
    L.con_src = takei(SGT_MAXCON); L.con_chain = takei(SGT_MAXCON); L.icnt = takei(32);
  }
#endif
  // what is left of the LDS up to the next occupancy step (160 KB / k workgroups per CU) caches contact scalars
  // (the hardware hands LDS out in granules -- a workgroup's request is rounded up -- so a share is taken a granule short of 160 KB / k:
  //  r04 measured 53 920 B per workgroup, 3 x which is under 160 KB, still running TWO per CU)
  const size_t used = (size_t)((char*)ip - (char*)base), total = 160 * 1024;
  if (used_out) *used_out = used;
  const size_t kper = used + 2560 < total ? total / (used + 2560) : 1, share = (total / (kper ? kper : 1)) / 2560 * 2560 - 2560;
  const size_t room = share > used ? share - used : 0;
  size_t nc = room / (SGT_CSC * sizeof(double));
  if (nc > SGT_MAXCON) nc = SGT_MAXCON;
  L.ncache = (int)nc;
  L.csc = (double*)ip;
#if !SGT_DEVICE && defined(SGT_EMU_SEPARATE)
  if (sp) L.csc = (double*)sep_take(sp->lds, sp->il, nc * SGT_CSC * sizeof(double));
#endif
  return used + nc * SGT_CSC * sizeof(double);
}
SG_HD size_t lds_bytes(const SgTreeDev& T, int N, int has_free = 0, int nnb = 0) {
  Lds L;
  return lds_carve(L, reinterpret_cast<double*>((uintptr_t)4096), T, N, has_free, reinterpret_cast<double*>((uintptr_t)4096), nullptr, nnb);
}
SG_HD size_t lds_used_bytes(const SgTreeDev& T, int N, int has_free = 0, int nnb = 0) {   // without the contact-scalar cache that fills the share
  Lds L;
  size_t u = 0;
  lds_carve(L, reinterpret_cast<double*>((uintptr_t)4096), T, N, has_free, reinterpret_cast<double*>((uintptr_t)4096), nullptr, nnb, &u);
  return u;
}
SG_HD size_t gws_doubles(const SgTreeDev& T, int N, int has_free, int nnb);
SG_HD long long cws_doubles(const SgTreeDev& T, int N, int has_free, int nnb = 0) {
  long long n = (long long)SGT_CWS_CARVE((size_t)0, cws_row_doubles(T.CS), T.NMAT) + (long long)gws_doubles(T, N, has_free, nnb);
#ifdef SG_DEBUG_WORK   // (debugging build: the env's LDS block is copied behind its work space when a launch ends, scripts/dev/work_diff.py)
  n += (long long)(lds_bytes(T, N, has_free, nnb) / sizeof(double));
#endif
  return n;
}
SG_HD size_t gws_doubles(const SgTreeDev& T, int N, int has_free, int nnb) {   // the work-space doubles behind the global-backed arrays
  Lds L;
  size_t n = 0;
  lds_carve(L, reinterpret_cast<double*>((uintptr_t)4096), T, N, has_free, reinterpret_cast<double*>((uintptr_t)4096), &n, nnb);
  return n;
}

// the address space of the arrays whose home SGT_DIET decides (lds_carve): M^-1 (bit 6), the sliders' 1 / m without a free object (bit 7)
#if (SGT_DIET >> 6) & 1
#define SGT_MINV_AS SGT_GLOBP
#else
#define SGT_MINV_AS SGT_LDSP
#endif
#if (SGT_DIET >> 7) & 1
#define SGT_EINVM_AS SGT_GLOBP
#else
#define SGT_EINVM_AS SGT_LDSP
#endif

}  // namespace sgt
