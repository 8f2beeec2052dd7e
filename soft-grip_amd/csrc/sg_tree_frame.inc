// sg_tree_frame.inc -- the STAGE FRAME: the names every stage function of the tree pipeline (sg_tree_stage_*.h) and its driver
// (sg_tree_env.h) work with, defined once and included AS TEXT inside their bodies:
//
//   #define SGT_FRAME SGT_FRAME_STAGE_HEAD      first thing in a stage function: everything below up to the step's scalars
//   #define SGT_FRAME SGT_FRAME_STAGE_TAIL      last thing in it: the label stage_done, the step's scalars back into S.ctx
//   #define SGT_FRAME SGT_FRAME_TABLES          tree_env: tables, carve and offsets ...
//   #define SGT_FRAME SGT_FRAME_STATE           ... and, after its masked-reset return, the env's state pointers
//   #include "sg_tree_frame.inc"                (which undefines SGT_FRAME again)
//
// Text and not a struct ON PURPOSE.  With the same locals as members of a StageEnv<CHD> object (the bodies moved verbatim into member
// templates) all twelve stage instantiations compiled to different code -- the collision stage 3 370 -> 3 586 instructions, the
// constraint stage + 270 -- and two of the three kernels with them: the optimiser does not see through the object what it sees in
// locals.  This kernel has a record of builds that differ in unrelated places disagreeing about single stores (DESIGN.md 4.10), so its
// generated code is not moved for tidiness: one function per stage over this shared text gives the instruction streams of the one
// four-way function it replaces, label for label (profiles/r08_tree_split_asm_same.txt; scripts/dev/asm_same.py checks a build).
//
// Names it puts in scope:
//   tables and carve   A env lds_base (device: recovered from the LDS header word; host: parameters) | H T N ND NB K nv nu CS h | S (Lds) |
//                      elemc gpairs nbtab sched E(f, e) | cw CW stage crow0 Mg crow(c) cscal(c) cscr(c) pidx(d)
//   state              FR gq gv gw gact gctrl kenv kt0
//   shared by stages   maxnd factor_all() tree_motion(qacc) (dynamics, finish) | slider_acc(e) (constraints, finish)
//   step scalars       flags ncon nefc iters stop touch_lo touch_hi last integrate sub (from S.ctx; the tail writes the first seven back)
//   (the work space's offsets come from sg_tree_layout.h's SGT_CWS_* -- macros for the same reason)
//   tail               stage_done: (a stage leaves early by `goto stage_done`, which is why its body sits in a block of its own)
#define SGT_FRAME_TABLES 1
#define SGT_FRAME_STATE 2
#define SGT_FRAME_STAGE_HEAD 3
#define SGT_FRAME_STAGE_TAIL 4
#if SGT_FRAME == SGT_FRAME_STAGE_HEAD && SGT_DEVICE
  // (the launch arguments: the kernel left the address of its argument segment in the first word of the LDS block -- a called function
  //  has no register for it -- and the segment is read through the constant address space: uniform, scalar loads)
  lds_ = (SGT_LDSP double*)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(unsigned long long)lds_);
  const unsigned long long ka_ = *(const SGT_LDSP unsigned long long*)lds_;
  const SGT_CONST TreeArgs& A = *(const SGT_CONST TreeArgs*)(((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(ka_ >> 32)) << 32) |
                                                               (unsigned)__builtin_amdgcn_readfirstlane((int)ka_));
  const int env = (int)blockIdx.x;
  double* const lds_base = (double*)lds_;
#endif
#if SGT_FRAME == SGT_FRAME_STAGE_HEAD || SGT_FRAME == SGT_FRAME_TABLES
  // The plan tables are read-only for the kernel's lifetime: read through the constant address space, a uniform index is a scalar load
  // (K$) that the compiler may hoist and keep, not a vector load behind a full vmcnt wait after every store
  const SGT_CONST SgPlanHeader& H = *(const SGT_CONST SgPlanHeader*)A.H;
  const SGT_CONST SgTreeDev& T = *(const SGT_CONST SgTreeDev*)A.T;
  const int N = H.nelem, ND = T.ND, NB = T.NB, K = T.K, nv = H.nv, nu = H.nu;
  constexpr int CS = CHD;   // (= T.CS: the plan pads the chains' stride to the instantiation's capacity, sg_plan.cpp)
  const double h = H.timestep;
  Lds S;
  lds_carve(S, lds_base, T, N, H.has_free, SGT_CWS_CARVE(A.cws + (size_t)env * A.cws_stride, cws_row_doubles(T.CS), T.NMAT), nullptr, H.nnb);
  const SGT_CONST double* const elemc = (const SGT_CONST double*)A.elem;
  const SGT_CONST SgGenPair* const gpairs = (const SGT_CONST SgGenPair*)A.gpairs;
  const SGT_CONST int* const nbtab = (const SGT_CONST int*)A.nbtab;
  const SGT_CONST SgEqSlot* const sched = (const SGT_CONST SgEqSlot*)A.sched;
  auto E = [&](int f, int e) { return elemc[(size_t)f * N + e]; };
  double* const cw = A.cws + (size_t)env * A.cws_stride;
  const long long CW = cws_row_doubles(CS);
#if !SGT_DEVICE && defined(SGT_EMU_SEPARATE)
  double* const stage = sep_pool() ? sep_part(0, SGT_CWS_ROWS((size_t)0)) : cw;
  double* const crow0 = sep_pool() ? sep_part(1, (size_t)SGT_MAXCON * CW) : SGT_CWS_ROWS(cw);
#else
  double* const stage = cw;
  double* const crow0 = SGT_CWS_ROWS(cw);
#endif
  auto crow = [&](int c) { return crow0 + (size_t)c * CW; };                 // J1[3][CS] | W1[3][CS] | J2[3][CS] | W2[3][CS] | scalars
  auto cscal = [&](int c) { return crow0 + (size_t)c * CW + 12 * CS; };
  auto cscr = [&](int c) -> const double* { return c < S.ncache ? S.csc + (size_t)c * SGT_CSC : crow0 + (size_t)c * CW + 12 * CS; };   // for the sweeps: the LDS copy when there is one
#if !SGT_DEVICE && defined(SGT_EMU_SEPARATE)
  double* const Mg = sep_pool() ? sep_part(2, (size_t)T.NMAT) : SGT_CWS_MASS(crow0, CW);
#else
  double* const Mg = SGT_CWS_MASS(crow0, CW);    // the chains' mass-matrix blocks [K][CS][CS], identity-padded
#endif
  auto pidx = [&](int d) { const int c = T.d_chain[d]; return c * CS + d - T.c_dof0[c]; };   // flat chain dof -> index in a padded [K][CS] vector
  (void)ND; (void)NB; (void)K; (void)nv; (void)h; (void)elemc; (void)E; (void)CW; (void)crow; (void)cscal; (void)cscr; (void)pidx;   // (no includer uses every name)

#endif
#if SGT_FRAME == SGT_FRAME_STAGE_HEAD || SGT_FRAME == SGT_FRAME_STATE
  const bool FR = H.has_free != 0;   // the composite's elements hang off a free body (6 dofs): the "object block" below
  double* const gq = A.qpos + (size_t)env * H.nq;
  double* const gv = A.qvel + (size_t)env * nv;
  double* const gw = A.warm + (size_t)env * nv;
  double* const gact = A.act + (size_t)env * (nu > 0 ? nu : 1);
  double* const gctrl = A.ctrl + (size_t)env * (nu > 0 ? nu : 1);

  const double kenv = A.kenv[env];
  const double kt0 = A.kmask_ten[H.t0_id] ? kenv : H.t0_k0;
  (void)kenv; (void)gq; (void)gv; (void)gw; (void)gact; (void)gctrl; (void)kt0; (void)stage; (void)Mg; (void)nu; (void)sched; (void)nbtab; (void)gpairs;
#endif
#if SGT_FRAME == SGT_FRAME_STAGE_HEAD
  // L'DL of every chain block in S.L at once (mj_factorM on serial chains): step s eliminates dof k = nd - 1 - s of each chain, one lane
  // per row i < k: L[i][j] -= (L[k][i] / L[k][k]) L[k][j] for j <= i, then row k is scaled.  Same operations as chain_factor.
  // The blocks are padded to [CS][CS]; a row's update runs over the whole row (the entries right of the diagonal are never read), so
  // that every lane's loop has the same count.
  int maxnd = 0;
  for (int c = 0; c < K; c++) maxnd = T.c_ndof[c] > maxnd ? T.c_ndof[c] : maxnd;
  auto factor_all = [&]() {
#if SGT_DEVICE && !defined(SGT_X_NOREGLDL)
    // L'DL IN REGISTERS (r04), chains of up to 17 dofs: a lane group per chain, lane i holds row i of the (symmetric) block.  Pivot k
    // (from the last dof down, mj_factorM's order): every lane i < k needs a = M[i][k] / D_k -- its own word and one broadcast -- and
    // row k's words M[k][j] = M[j][k], j < k: the SAME register of the lanes j, k shuffles; then M[i][j] -= a M[k][j] in registers
    // (both triangles are kept, so that the words a lane needs of row k are the column words of the other lanes) and U[i][k] = a is
    // L[k][i].  Row 16 -- the 17th dof of the four-finger gripper's long chains, one more than a group has lanes -- is eliminated
    // first and is never updated: its words are read by every lane of the group.  ~400 shuffles + 140 multiply-adds for all chains
    // at once; step by step through the work space with two barriers a pivot it took 100 k cycles, and it runs twice a substep
    // (M and M + h B: 40 % of a contact-free substep).
    constexpr int NC = CHD < 17 ? CHD : 17;
    if (maxnd <= NC && CS <= 20) {
      const int grp = (int)threadIdx.x >> 4, l = (int)threadIdx.x & 15, gb = (int)threadIdx.x & 48;
      for (int c0 = 0; c0 < K; c0 += 4) {
        const int c = c0 + grp, cc = c < K ? c : 0;
        double* Lc = S.L + cc * CS * CS;
        const bool row = c < K && l < CS;   // the lane holds a row of a chain (else a virtual identity row: every step a no-op)
        double m[NC];
#pragma unroll
        for (int j = 0; j < NC; j++) m[j] = (row && j < CS) ? Lc[l * CS + j] : (j == l ? 1.0 : 0.0);
        if constexpr (NC == 17) {
          if (CS > 16) {   // (uniform)
            const double a = m[16] / Lc[16 * CS + 16];
#pragma unroll
            for (int j = 0; j < 16; j++) m[j] -= a * Lc[16 * CS + j];
            m[16] = a;
          }
        }
#pragma unroll
        for (int k = (NC == 17 ? 15 : NC - 1); k >= 1; k--) {
          const double Dk = __shfl(m[k], gb + k, 64);
          double v[16];
#pragma unroll
          for (int j = 0; j < k; j++) v[j] = __shfl(m[k], gb + j, 64);
          if (l < k) {
            const double a = m[k] / Dk;
#pragma unroll
            for (int j = 0; j < k; j++) m[j] -= a * v[j];
            m[k] = a;
          }
        }
        // back to the work space in chain_solve's layout: D on the diagonal, L[k][i] (i < k) below it -- lane i writes column i
        if (row) {
          double dd = m[0];
#pragma unroll
          for (int j = 1; j < NC; j++) dd = j == l ? m[j] : dd;
          Lc[l * CS + l] = dd;
#pragma unroll
          for (int k = 1; k < NC; k++)
            if (l < k && k < CS) Lc[k * CS + l] = m[k];
        }
      }
      SGT_SYNC();
      return;
    }
#endif
    for (int st = 0; st + 1 < CS; st++) {
      SGT_PAR(idx, K * CS) {
        const int c = idx / CS, i = idx % CS, k = T.c_ndof[c] - 1 - st;
        if (k >= 1 && i < k) {
          double* Lc = S.L + c * CS * CS;
          const double a = Lc[k * CS + i] / Lc[k * CS + k];
          for (int j = 0; j < CS; j += 4) {
            const double l0 = Lc[k * CS + j], l1 = Lc[k * CS + j + 1], l2 = Lc[k * CS + j + 2], l3 = Lc[k * CS + j + 3];
            const double r0 = Lc[i * CS + j], r1 = Lc[i * CS + j + 1], r2 = Lc[i * CS + j + 2], r3 = Lc[i * CS + j + 3];
            Lc[i * CS + j] = r0 - a * l0; Lc[i * CS + j + 1] = r1 - a * l1; Lc[i * CS + j + 2] = r2 - a * l2; Lc[i * CS + j + 3] = r3 - a * l3;
          }
        }
      }
      SGT_SYNC();
      SGT_PAR(idx, K * CS) {
        const int c = idx / CS, i = idx % CS, k = T.c_ndof[c] - 1 - st;
        if (k >= 1 && i < k) {
          double* Lc = S.L + c * CS * CS;
          Lc[k * CS + i] = Lc[k * CS + i] / Lc[k * CS + k];
        }
      }
      SGT_SYNC();
    }
  };
  auto tree_motion = [&](const double* qacc) {
    SGT_PAR(c, K) {
      double w[3] = {0, 0, 0}, al[3] = {0, 0, 0}, a[3] = {-H.gravity[0], -H.gravity[1], -H.gravity[2]}, P[3], r[3], t[3], t2[3];
      for (int k = 0; k < 3; k++) P[k] = T.c_root_pos[c][k];
      for (int bi = 0; bi < T.c_nbody[c]; bi++) {
        const int tb = T.c_body0[c] + bi;
        for (int kj = 0; kj <= T.b_njnt[tb]; kj++) {
          const bool lastj = kj == T.b_njnt[tb];
          const int d = T.b_dof0[tb] + kj;
          const double* Q = lastj ? S.xpos + 3 * tb : S.anchor + 3 * d;
          for (int k = 0; k < 3; k++) r[k] = Q[k] - P[k];
          cross3(t, w, r);
          cross3(t2, al, r); addscl3(a, t2, 1);
          cross3(t2, w, t); addscl3(a, t2, 1);
          for (int k = 0; k < 3; k++) P[k] = Q[k];
          if (lastj) break;
          const double* u = S.axis + 3 * d;
          const double qd = S.v[d], qdd = qacc ? qacc[d] : 0.0;
          cross3(t, w, u);
          addscl3(al, u, qdd); addscl3(al, t, qd);
          addscl3(w, u, qd);
        }
        for (int k = 0; k < 3; k++) { S.bw[3 * tb + k] = w[k]; S.bal[3 * tb + k] = al[k]; S.ba[3 * tb + k] = a[k]; }
      }
    }
  };
  auto slider_acc = [&](int e) {   // a slider's constraint acceleration: with a free object its local part minus the body's share
    return FR ? S.ae[e] - dot6(S.Be + 6 * e, S.of + OF_AF) * S.einvm[e] : S.ae[e];
  };
  (void)maxnd; (void)factor_all; (void)tree_motion; (void)slider_acc;
  int flags = (int)S.ctx[CTX_FLAGS], ncon = (int)S.ctx[CTX_NCON], nefc = (int)S.ctx[CTX_NEFC], iters = (int)S.ctx[CTX_ITERS], stop = 0;
  unsigned touch_lo = (unsigned)S.ctx[CTX_TLO], touch_hi = (unsigned)S.ctx[CTX_THI];
  const bool last = S.ctx[CTX_LAST] != 0.0, integrate = S.ctx[CTX_INTEGRATE] != 0.0;
  const int sub = (int)S.ctx[CTX_SUB];
  (void)last; (void)integrate; (void)sub; (void)nefc; (void)iters; (void)touch_lo; (void)touch_hi; (void)ncon;
  SGT_SYNC();   // (every lane has the step's scalars before lane 0 writes them back)
  SGT_STAMP_INIT();
#endif
#if SGT_FRAME == SGT_FRAME_STAGE_TAIL
stage_done: __attribute__((unused));
  SGT_SYNC();
  SGT_ONE {
    S.ctx[CTX_FLAGS] = flags; S.ctx[CTX_NCON] = ncon; S.ctx[CTX_NEFC] = nefc; S.ctx[CTX_ITERS] = iters;
    S.ctx[CTX_TLO] = touch_lo; S.ctx[CTX_THI] = touch_hi; S.ctx[CTX_STOP] = stop;
  }
  SGT_SYNC();
#endif
#undef SGT_FRAME
