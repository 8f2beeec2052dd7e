// sg_tree_sweep.h -- the PGS sweeps of one forward pass (part of sg_tree.h)
#pragma once

namespace sgt {

// ---------------------------------------------------------------- stage 10b: the PGS sweeps (mj_solPGS) of one forward pass, one env
// Everything the rows need was laid out by tree_env: the sliders' rows (S.ffix, S.flim, constants in the work space), the chains' limit
// rows (S.lrow), the contacts' J / W rows and scalars (work space), the accelerations a = M^-1 J' f of the current forces (S.aF, S.ae).
// A function of its own ON PURPOSE (see the call site).  Pointers come typed by address space, uniform values are made scalar again.
template <int CHD, bool FRT, bool NBT>   // FRT: the scene has a free object, NBT: the composite's neighbour rows -- compile-time facts of the instantiation, so that a sweep carries only its own scene class's code (r04: 355 -> 190 spill instructions for the four-finger gripper's)
static SGT_NOINLINE void tree_sweep(const SGT_CONST SgPlanHeader* Hp, const SGT_CONST SgTreeDev* Tp, const SGT_CONST int* nbtab, const SGT_CONST SgEqSlot* sched,
                                    const int* nbtab_generic, SGT_GLOBP double* cw_, SGT_LDSP double* lds_, unsigned long long* secprof) {
#if SGT_DEVICE
  // (arguments of a called function arrive in vector registers: back to scalar ones, so that the plan tables are scalar loads again)
  auto uni = [](auto* q) { return (decltype(q))(((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)((unsigned long long)q >> 32)) << 32) |
                                                 (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned long long)q)); };
  Hp = uni(Hp); Tp = uni(Tp); nbtab = uni(nbtab); sched = uni(sched); nbtab_generic = uni(nbtab_generic); secprof = uni(secprof);
  cw_ = (SGT_GLOBP double*)(((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)((unsigned long long)cw_ >> 32)) << 32) |
                            (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned long long)cw_));
  lds_ = (SGT_LDSP double*)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(unsigned long long)lds_);
#endif
  const SGT_CONST SgPlanHeader& H = *Hp;
  const SGT_CONST SgTreeDev& T = *Tp;
  double* const cw = (double*)cw_;
  const int N = H.nelem, K = T.K;
  constexpr int CS = CHD;   // (= T.CS: the plan pads the chains' stride to the instantiation's capacity)
  constexpr bool FR = FRT, NB = NBT;
  Lds S;
  lds_carve(S, (double*)lds_, T, N, H.has_free, SGT_CWS_CARVE(cw, cws_row_doubles(T.CS), T.NMAT), nullptr, H.nnb);
  const long long CW = cws_row_doubles(CS);
#if !SGT_DEVICE && defined(SGT_EMU_SEPARATE)
  double* const crow0 = sep_pool() ? sep_part(1, (size_t)SGT_MAXCON * CW) : SGT_CWS_ROWS(cw);
#else
  double* const crow0 = SGT_CWS_ROWS(cw);
#endif
  auto crow = [&](int c) { return crow0 + (size_t)c * CW; };
  auto cscr = [&](int c) -> const double* { return c < S.ncache ? S.csc + (size_t)c * SGT_CSC : crow0 + (size_t)c * CW + 12 * CS; };
  // The sweeps' arrays once more, TYPED BY ADDRESS SPACE (r05).  Through the carve's generic pointers every access is a FLAT instruction,
  // which counts on both memory counters: the wait for an LDS word (a contact's force, a slider's acceleration) then also waits for
  // every global load in flight -- the NEXT contact's record, requested one update ahead precisely so that its latency is hidden.  The
  // r04 ISA had `flat_load_dwordx4 (S.cf)` + `s_waitcnt vmcnt(0)` in the middle of every update: ~8 k cycles an update, two exposed
  // round trips.  Typed, the LDS words are ds_read / ds_write (lgkmcnt only) and the prefetch stays in flight.
  SGT_LDSP double* const aeL = (SGT_LDSP double*)S.ae;
  SGT_LDSP double* const aFL = (SGT_LDSP double*)S.aF;
  SGT_LDSP double* const cfL = (SGT_LDSP double*)S.cf;
  SGT_LDSP double* const ffixL = (SGT_LDSP double*)S.ffix;
  SGT_LDSP double* const flimL = (SGT_LDSP double*)S.flim;
  SGT_LDSP double* const lrowL = (SGT_LDSP double*)S.lrow;
  SGT_LDSP double* const ofL = (SGT_LDSP double*)S.of;
  SGT_LDSP double* const BeL = (SGT_LDSP double*)S.Be;
  const SGT_LDSP int* const icntL = (const SGT_LDSP int*)S.icnt;
  const SGT_LDSP int* const hitpairL = (const SGT_LDSP int*)S.hit_pair;
  const SGT_LDSP int* const hitcntL = (const SGT_LDSP int*)S.hit_cnt;
  const SGT_MINV_AS double* const MinvT = (const SGT_MINV_AS double*)S.Minv;
  const SGT_GLOBP double* const bfixG = (const SGT_GLOBP double*)S.bfix;
  const SGT_GLOBP double* const RfixG = (const SGT_GLOBP double*)S.Rfix;
  const SGT_GLOBP double* const IfixG = (const SGT_GLOBP double*)S.Ifix;
  const SGT_GLOBP double* const nbbG = (const SGT_GLOBP double*)S.nbb;
  const SGT_GLOBP double* const nbRG = (const SGT_GLOBP double*)S.nbR;
  const SGT_GLOBP double* const nbIG = (const SGT_GLOBP double*)S.nbI;
  SGT_GLOBP double* const nbfG = (SGT_GLOBP double*)S.nbf;
  [[maybe_unused]] const SGT_GLOBP double* const nbqG = (const SGT_GLOBP double*)S.nbq;
  [[maybe_unused]] const SGT_GLOBP double* const fixqG = (const SGT_GLOBP double*)S.fixq;
  const SGT_EINVM_AS double* const einvmNF = (const SGT_EINVM_AS double*)S.einvm;   // scenes WITHOUT a free object only (with one: LDS, lds_carve)
  (void)aeL; (void)aFL; (void)cfL; (void)ffixL; (void)flimL; (void)lrowL; (void)ofL; (void)BeL; (void)icntL; (void)hitpairL; (void)hitcntL; (void)MinvT;
  (void)bfixG; (void)RfixG; (void)IfixG; (void)nbbG; (void)nbRG; (void)nbIG; (void)nbfG; (void)einvmNF;
  struct { unsigned long long* secprof; const int* nbtab; } A = {secprof, nbtab_generic};   // (what SGT_STAMP and the free object's row functions name)
  (void)A;
  SGT_STAMP_INIT();
  const double con_mu[2] = {H.con_mu[0], H.con_mu[1]};
  const int ncon = (int)S.swc[SWC_NCON];
  const bool serial_contacts = S.swc[SWC_SERIAL] != 0.0;
  const double ten_R = S.swc[SWC_TEN_R], ten_b = S.swc[SWC_TEN_B], tj_A = S.swc[SWC_TJ_A], ten_I = S.swc[SWC_TEN_I];
  double ten_f = S.swc[SWC_TEN_F];
  const double cten[6] = {S.swc[SWC_CTEN], S.swc[SWC_CTEN + 1], S.swc[SWC_CTEN + 2], S.swc[SWC_CTEN + 3], S.swc[SWC_CTEN + 4], S.swc[SWC_CTEN + 5]};
  auto slider_acc = [&](int e) {   // a slider's constraint acceleration: with a free object its local part minus the body's share
    return FR ? S.ae[e] - dot6(S.Be + 6 * e, S.of + OF_AF) * S.einvm[e] : S.ae[e];
  };
  int iters = 0;
  // the sliders' row constants, per lane for the whole solve (r04): b, R, 1 / (A + R) of the joint-fix row, R, b, 1 / (A + R) of the two
  // limit rows, 1 / m and the tendon coefficient.  They sit in the work space (not in LDS); every sweep used to fetch
  // them again -- four dependent trips of the wavefront to L2 per pass, 6 % + 3 % of a substep at the squeeze
  double kfb[SGT_NSLOT], kfR[SGT_NSLOT], kfI[SGT_NSLOT], kim[SGT_NSLOT], kco[SGT_NSLOT], klR[SGT_NSLOT][2], klb[SGT_NSLOT][2], klI[SGT_NSLOT][2];
  SGT_PAR_SLOT(e, t, N) {
    kfb[t] = S.bfix[e]; kfR[t] = S.Rfix[e]; kfI[t] = S.Ifix[e]; kim[t] = S.einvm[e]; kco[t] = S.ecoef[e];
    for (int sd = 0; sd < 2; sd++) { klR[t][sd] = S.Rlim[2 * e + sd]; klb[t][sd] = S.blim[2 * e + sd]; klI[t][sd] = S.Ilim[2 * e + sd]; }
  }
  for (int it = 0; it < H.iterations; it++) {
    double imp_par = 0, imp_uni = 0;
    // joint-fix rows: each on its own slider
    double S_ae = 0;
    if (FR) {
      // with a free object a joint-fix row moves the body and through it every slider: the rows run one after the other (mj_solPGS's
      // order), the body's acceleration a_f in registers, a row's own slider from its local part and a_f
      if (NB) SGT_ONE {
        S.red[0] = free_eq_blocks((const SGT_LDSP double*)S.frow, (const SGT_LDSP double*)S.Be, (const SGT_LDSP double*)S.Ce, (const SGT_LDSP double*)S.einvm, (SGT_LDSP double*)S.ffix,
                                  (SGT_LDSP double*)S.ae, (SGT_LDSP double*)(S.of + OF_AF), N, A.nbtab, S.nbf, S.nbb, S.nbR, S.nbA, S.nbI);
      }
#ifdef SGT_FIXROWS_BLOCKED
      if (!NB) {   // (device: every lane a block of the rows, free_fix_rows_blocked; each lane's share of the cost change goes into the wavefront sum)
        imp_par += free_fix_rows_blocked((const SGT_LDSP double*)S.frow, (const SGT_LDSP double*)S.Be, (const SGT_LDSP double*)S.einvm, (const SGT_LDSP double*)(S.of + OF_SINV),
                                         (SGT_LDSP double*)S.ffix, (SGT_LDSP double*)S.ae, (SGT_LDSP double*)(S.of + OF_AF), N);
        SGT_ONE { S.red[0] = 0.0; }
      }
#else
      if (!NB) SGT_ROW_LANES {   // (device: lanes 0 .. 7, the six components of the body's acceleration a lane each)
        const double r_ = free_fix_rows((const SGT_LDSP double*)S.frow, (const SGT_LDSP double*)S.Be, (const SGT_LDSP double*)S.einvm, (const SGT_LDSP double*)(S.of + OF_SINV),
                                        (SGT_LDSP double*)S.ffix, (SGT_LDSP double*)S.ae, (SGT_LDSP double*)(S.of + OF_AF), N);
        SGT_ONE { S.red[0] = r_; }
      }
#endif
      SGT_SYNC();
      imp_uni += S.red[0];
      SGT_PAR(e, N) S_ae += S.ecoef[e] * S.ae[e];
      S_ae = wsum(S_ae) - dot6(H.obj_tenB, S.of + OF_AF);   // sum coef_e a_e, a_e = local part - B_e . a_f / D_e
    } else if (NB) {
      // equality BLOCKS [fix_e, e's neighbour rows] in the plan's list schedule: the blocks of a round share no slider (they
      // commute exactly), every block sits in a later round than the blocks it depends on -- the rounds in order ARE mj_solPGS's
      // sequential sweep (sg_plan.h); 64 blocks per round, a lane each
#if SGT_DEVICE && !defined(SGT_X_EQSYNC)
      // (r05s) The rounds PIPELINED: a round's table words (its slot) and its rows' constants and forces -- two dependent trips to the work
      // space -- do not depend on the rounds before it, only the sliders' accelerations (LDS) do.  As written for the emulation below, every
      // round paid both trips and then a barrier that drains the rows' force stores: ~2.5 us a round, 55 us a sweep, three quarters of a
      // substep of the four-finger gripper's default model.  Here a round's constants are requested two rounds ahead and its slot five (three
      // register sets), and nothing in the loop waits at a barrier: the wavefront's LDS instructions execute in order, so a lane's read of a
      // slider sees the write another lane made a round earlier.  Same rows, same order, same arithmetic: same bits.
      {
        const int lane = (int)threadIdx.x;
        const int nr = H.eq_rounds;
        struct ERec { int e, pe[3]; double invm, Rf, bf, If, ipm[3], R[3], b[3], I[3], f[3]; };
        auto load_rec = [&](ERec& q, const SgEqSlot slot) {
          q.e = slot.e;
          const int e = slot.e < N ? slot.e : 0;
          // (the rows' constants packed by the build stage, S.fixq / S.nbq: one 32-byte record per row -- two loads behind ONE address
          //  instead of four or five words from as many arrays behind as many 64-bit address computations)
          {
            const SGT_GLOBP double2* const fq = (const SGT_GLOBP double2*)(fixqG + 4 * e);
            const double2 u = fq[0], w = fq[1];
            q.bf = u.x; q.Rf = u.y; q.If = w.x; q.invm = w.y;
          }
#pragma unroll
          for (int d = 0; d < 3; d++) {
            const int pe = slot.e < N ? slot.p[d] : N;
            const int k = d * N + e;
            q.pe[d] = pe;
            const SGT_GLOBP double2* const nq = (const SGT_GLOBP double2*)(nbqG + 4 * k);   // (row k's words exist whether the block has the row or not)
            const double2 u = nq[0], w = nq[1];
            q.R[d] = u.x; q.b[d] = u.y; q.I[d] = w.x; q.ipm[d] = w.y;
            q.f[d] = nbfG[k];
          }
        };
        // A block straight through: the slider's and its partners' accelerations are read TOGETHER at the top (one LDS latency, not four in
        // a row behind each other's stores), the four rows run in registers, the stores follow.  A row the block does not have is a no-op
        // by its record (R = b = 1 / (A + R) = 1 / m_p = f = 0: the step is exactly 0) on the block's own slider as stand-in partner, so no
        // lane branches inside a block; the own slider's store comes last.
        auto run = [&](const ERec& q) {
          const int e = q.e;
          if (e < N) {
            const double invm = q.invm;
            const int pc0 = q.pe[0] < N ? q.pe[0] : e, pc1 = q.pe[1] < N ? q.pe[1] : e, pc2 = q.pe[2] < N ? q.pe[2] : e;
            double ae_ = aeL[e], f0 = ffixL[e];
            const double ap0 = aeL[pc0], ap1 = aeL[pc1], ap2 = aeL[pc2];
            double old = f0;
            imp_par -= scalar_update_rcp(f0, q.bf, ae_, q.Rf, invm + q.Rf, q.If, false);
            ae_ += invm * (f0 - old);
            double f1 = q.f[0];
            old = f1;
            imp_par -= scalar_update_rcp(f1, q.b[0], ae_ - ap0, q.R[0], invm + q.ipm[0] + q.R[0], q.I[0], false);
            const double d1 = f1 - old;
            ae_ += invm * d1;
            double f2 = q.f[1];
            old = f2;
            imp_par -= scalar_update_rcp(f2, q.b[1], ae_ - ap1, q.R[1], invm + q.ipm[1] + q.R[1], q.I[1], false);
            const double d2 = f2 - old;
            ae_ += invm * d2;
            double f3 = q.f[2];
            old = f3;
            imp_par -= scalar_update_rcp(f3, q.b[2], ae_ - ap2, q.R[2], invm + q.ipm[2] + q.R[2], q.I[2], false);
            const double d3 = f3 - old;
            ae_ += invm * d3;
            ffixL[e] = f0;
            nbfG[e] = f1; nbfG[N + e] = f2; nbfG[2 * N + e] = f3;
            aeL[pc0] = ap0 - q.ipm[0] * d1;
            aeL[pc1] = ap1 - q.ipm[1] * d2;
            aeL[pc2] = ap2 - q.ipm[2] * d3;
            aeL[e] = ae_;
          }
        };
        if (nr > 0) {
          // three register sets: a round's record is requested TWO rounds before it runs, its slot three rounds before that
          auto slot_of = [&](int r) { return sched[(r < nr ? r : 0) * 64 + lane]; };   // (past the end: round 0's words, read and not used)
          ERec q0, q1, q2;
          SgEqSlot t0 = slot_of(0), t1 = slot_of(1), t2 = slot_of(2);
          load_rec(q0, t0); load_rec(q1, t1);
          t0 = slot_of(3); t1 = slot_of(4);
          for (int r = 0; r < nr; r += 3) {
            load_rec(q2, t2); t2 = slot_of(r + 5);
            run(q0);
            __builtin_amdgcn_wave_barrier();
            load_rec(q0, t0); t0 = slot_of(r + 6);
            if (r + 1 < nr) run(q1);
            __builtin_amdgcn_wave_barrier();
            load_rec(q1, t1); t1 = slot_of(r + 7);
            if (r + 2 < nr) run(q2);
            __builtin_amdgcn_wave_barrier();
          }
        }
        SGT_SYNC();
      }
#else
      for (int r = 0; r < H.eq_rounds; r++) {
        SGT_PAR(sl, 64) {
          const SgEqSlot slot = sched[r * 64 + sl];
          const int e = slot.e;
          if (e < N) {
            const double invm = einvmNF[e];
            double ae_ = aeL[e], f = ffixL[e];
            double old = f;
            const double Rf = RfixG[e];
            imp_par -= scalar_update_rcp(f, bfixG[e], ae_, Rf, invm + Rf, IfixG[e], false);
            ffixL[e] = f;
            ae_ += invm * (f - old);
            for (int d = 0; d < 3; d++) {
              const int pe = slot.p[d];
              if (pe >= N) continue;
              const int k = d * N + e;
              const double ap = aeL[pe], ipm = einvmNF[pe], R = nbRG[k];
              f = nbfG[k]; old = f;
              imp_par -= scalar_update_rcp(f, nbbG[k], ae_ - ap, R, invm + ipm + R, nbIG[k], false);
              nbfG[k] = f;
              ae_ += invm * (f - old);
              aeL[pe] = ap - ipm * (f - old);
            }
            aeL[e] = ae_;
          }
        }
        SGT_SYNC();
      }
#endif
      SGT_PAR_SLOT(e, t, N) S_ae += kco[t] * aeL[e];
      S_ae = wsum(S_ae);
    } else {
      SGT_PAR_SLOT(e, t, N) {
        const double invm = kim[t];
        double f = ffixL[e];
        const double old = f, ael = aeL[e];
        imp_par -= scalar_update_rcp(f, kfb[t], ael, kfR[t], invm + kfR[t], kfI[t], false);
        ffixL[e] = f;
        const double an = ael + invm * (f - old);
        aeL[e] = an;
        S_ae += kco[t] * an;
      }
      S_ae = wsum(S_ae);
    }
    SGT_STAMP(17);
    {  // the tendon-fix row over all sliders
      const double old = ten_f;
      imp_uni -= scalar_update_rcp(ten_f, ten_b, S_ae, ten_R, tj_A + ten_R, ten_I, false);
      const double dfl = ten_f - old;
      SGT_PAR_SLOT(e, t, N) aeL[e] += kco[t] * dfl * kim[t];
      if (FR) {
        SGT_SYNC();
        SGT_ONE { for (int q = 0; q < 6; q++) S.of[OF_AF + q] += cten[q] * dfl; }
        SGT_SYNC();
      }
    }
    SGT_STAMP(18);
    // chain limit rows: serial within a chain, the chains side by side
#if SGT_DEVICE && !defined(SGT_X_NOLG)
    // A LANE GROUP per chain (r04): the 16 lanes of a DPP row hold the chain's accelerations -- lane l dofs l and l + 16 -- in registers
    // for the whole pass; a row's J a = +-a[dof] is a masked row sum (rotations, no LDS), its scalar update runs on all 16 lanes
    // alike, its push a += M^-1[dof][.] df is one multiply-add per lane and word.  (One lane per chain -- 4 of 64 -- read and wrote
    // all CS words through LDS per row: 1 900 cycles a row, 13 % of a substep at the squeeze.)  Four chains per pass.
    {
      const int grp = (int)threadIdx.x >> 4, l = (int)threadIdx.x & 15;
      const bool lo_w = l < CS, hi_w = l + 16 < CS;   // (short chains: CS < 16 -- the lanes beyond the stride hold no word)
      const int ll = lo_w ? l : 0;
      for (int c0 = 0; c0 < K; c0 += 4) {
        const int c = c0 + grp, cc = c < K ? c : 0;
        SGT_LDSP double* rows = lrowL + SGT_LROW * 2 * T.c_dof0[cc];
        const SGT_MINV_AS double* Mi = MinvT + cc * CS * CS;
        double a0 = lo_w ? aFL[cc * CS + l] : 0.0, a1 = hi_w ? aFL[cc * CS + l + 16] : 0.0;
        const int nrow = c < K ? icntL[IC_NLIM0 + cc] : 0;
        int nmax = __builtin_amdgcn_readlane(nrow, 0);
        for (int g2 = 16; g2 < 64; g2 += 16) { const int o = __builtin_amdgcn_readlane(nrow, g2); nmax = o > nmax ? o : nmax; }
#if defined(SG_SECTION_PROF)
        if (threadIdx.x == 0) { atomicAdd(&A.secprof[44], (unsigned long long)nmax); atomicAdd(&A.secprof[45], 1ull); }   // chain limit rows: row slots per pass
#endif
        // (two register sets: the next row's record and its row of M^-1 -- two dependent LDS round trips -- are on their way during a row's update)
        struct LRec { double sg, R, b, f, Ainv, mdd, m0, m1; int dl; };
        auto load_row = [&](LRec& q, int i) {
          // (a group past its own list -- or without one -- reads row 0's words and dof 0's row of M^-1: both exist, nothing is applied.
          //  The dof index MUST be a valid one: M^-1 sits in the work space, and a stale LDS word as an index into it is a memory fault)
          const bool have = i < nrow;
          const SGT_LDSP double* r = rows + SGT_LROW * (have ? i : 0);
          int dl = have ? (int)r[0] : 0;
          dl = dl < 0 ? 0 : (dl >= CS ? CS - 1 : dl);
          q.dl = dl; q.sg = r[1]; q.R = r[2]; q.b = r[3]; q.f = r[4]; q.Ainv = r[5];
          q.mdd = Mi[dl * CS + dl]; q.m0 = Mi[dl * CS + ll]; q.m1 = Mi[dl * CS + (hi_w ? l + 16 : ll)];
        };
        auto update_row = [&](const LRec& q, int i) {
          const bool act = i < nrow;
          double f = q.f;
          const double adl = rowsum16(l == (q.dl & 15) ? (q.dl < 16 ? a0 : a1) : 0.0);
          const double ch = scalar_update_rcp(f, q.b, q.sg * adl, q.R, q.mdd + q.R, q.Ainv, true);
          const double dfl = act ? q.sg * (f - q.f) : 0.0;
          if (lo_w) a0 += q.m0 * dfl;
          if (hi_w) a1 += q.m1 * dfl;
          if (act && l == 0) { imp_par -= ch; rows[SGT_LROW * i + 4] = f; }
        };
        // SGT_LROW_AHEAD register sets: a row's words and its row of M^-1 -- two dependent round trips away: the row's dof index from LDS, then
        // the work space -- are requested SGT_LROW_AHEAD - 1 rows ahead.  Seven ahead instead of three measured SLOWER (r05): the wait is
        // not the loads' latency
        constexpr int AH = SGT_LROW_AHEAD;
        LRec q[AH];
        if (nmax > 0) {
#pragma unroll
          for (int k = 0; k < AH - 1; k++) load_row(q[k], k);
        }
        for (int i = 0; i < nmax; i += AH) {
#pragma unroll
          for (int k = 0; k < AH; k++) {
            load_row(q[(k + AH - 1) % AH], i + k + AH - 1);
            update_row(q[k], i + k);
          }
        }
        if (c < K) {
          if (lo_w) aFL[cc * CS + l] = a0;
          if (hi_w) aFL[cc * CS + l + 16] = a1;
        }
      }
    }
#else
    SGT_PAR(c, K) {
      double* rows = S.lrow + SGT_LROW * 2 * T.c_dof0[c];
      const double* Mi = S.Minv + c * CS * CS;
      double* aFc = S.aF + c * CS;
      const int nrow = S.icnt[IC_NLIM0 + c];
      for (int i = 0; i < nrow; i++) {
        double* r = rows + SGT_LROW * i;
        const int dl = (int)r[0];
        double f = r[4];
        const double old = f;
        imp_par -= scalar_update_rcp(f, r[3], r[1] * aFc[dl], r[2], Mi[dl * CS + dl] + r[2], r[5], true);
        r[4] = f;
        const double dfl = r[1] * (f - old);
        // every load before the first store (a load-store chain through LDS costs a round trip per element): unrolled over the
        // capacity, the loads unguarded (beyond the padded stride CS they hit other LDS words and are dropped), the stores behind
        // scalar branches on CS, which is the same on every lane
        double an[CHD];
#pragma unroll
        for (int k = 0; k < CHD; k++) an[k] = aFc[k] + Mi[dl * CS + k] * dfl;
#pragma unroll
        for (int k = 0; k < CHD; k += 4)
          if (k < CS) { aFc[k] = an[k]; aFc[k + 1] = an[k + 1]; aFc[k + 2] = an[k + 2]; aFc[k + 3] = an[k + 3]; }
      }
    }
#endif
    SGT_STAMP(19);
    // slider limit rows
    SGT_PAR_SLOT(e, t, N) {
      const double invm = kim[t];
#pragma unroll
      for (int sd = 0; sd < 2; sd++) {
        const double R = klR[t][sd];
        if (R == 0.0) continue;
        const double sg = sd ? -1.0 : 1.0;
        double f = flimL[2 * e + sd];
        const double old = f;
        imp_par -= scalar_update_rcp(f, klb[t][sd], sg * aeL[e], R, invm + R, klI[t][sd], true);
        flimL[2 * e + sd] = f;
        aeL[e] += invm * sg * (f - old);
      }
    }
    SGT_SYNC();
    SGT_STAMP(12);
    // contacts: one stream per chain ...
    if (!serial_contacts) {
#if SGT_DEVICE && !defined(SGT_X_NOSTREAM)
      // One STREAM PER CHAIN on a lane group (r04): the chain's accelerations in registers as in the limit-row pass (lane l: dofs l,
      // l + 16), a contact's J and W rows read one word per lane and row (coalesced 128-byte pieces from the work space, the NEXT
      // contact's on their way during this one's update), J a as three row sums, the 3 x 3 block update on all 16 lanes alike, the
      // push a += W' df as three multiply-adds per lane and word.  The streams' contact lists (S.hit_pair: contact ids by chain,
      // offsets behind them) are built with the rows.  One lane per chain cost ~14 k cycles an update: 120 loads and the whole
      // chain vector through LDS per contact, 47 % of a substep at the squeeze.
      {
        const int grp = (int)threadIdx.x >> 4, l = (int)threadIdx.x & 15;
        const bool lo_w = l < CS, hi_w = l + 16 < CS;   // (short chains: CS < 16 -- the lanes beyond the stride hold no word)
        const int ll = lo_w ? l : 0;
        const SGT_LDSP int* const lvl = hitpairL;       // [nlev][K]: the contact of chain c in level L, or -1 (tree_stage_constraints)
        const int nlev = icntL[IC_NLEV], nb = (K + 3) >> 2, nslot = nlev * nb;   // a slot = (level, batch of four chains): one update per lane group
        // a contact as the sweep needs it: J and W rows, word l (j, w) and word l + 16 (k, x), and the scalars of its record -- all from the
        // work space (one address space: the loads of the NEXT contact, requested before this one's update, stay in flight across it;
        // through a pointer that may be LDS or global every use waited for every load issued before it)
        struct CRec { double j0, j1, j2, k0, k1, k2, w0, w1, w2, x0, x1, x2, A[6], Pe[7], B[3], R, invm, Js[3], slf; int ci; };
        auto load_rec = [&](CRec& q, int ci) {
          const double* J = crow(ci);
          const double* W = J + 3 * CS;
          const double* sc = J + 12 * CS;
          const int lh = hi_w ? l + 16 : ll;   // (a lane without a word reads word 0 / word ll again: its product is zeroed below)
          q.ci = ci;
          q.j0 = J[ll]; q.j1 = J[CS + ll]; q.j2 = J[2 * CS + ll]; q.k0 = J[lh]; q.k1 = J[CS + lh]; q.k2 = J[2 * CS + lh];
          q.w0 = W[ll]; q.w1 = W[CS + ll]; q.w2 = W[2 * CS + ll]; q.x0 = W[lh]; q.x1 = W[CS + lh]; q.x2 = W[2 * CS + lh];
#pragma unroll
          for (int k = 0; k < 6; k++) q.A[k] = sc[CS_A + k];
#pragma unroll
          for (int k = 0; k < 3; k++) { q.B[k] = sc[CS_B + k]; q.Js[k] = sc[CS_JS + k]; }
          q.R = sc[CS_R]; q.invm = sc[CS_INVM]; q.slf = sc[CS_SL];
#pragma unroll
          for (int k = 0; k < 7; k++) q.Pe[k] = sc[CS_PE + k];
        };
        if (nslot > 0) {
#if defined(SG_SECTION_PROF)
          if (threadIdx.x == 0) { atomicAdd(&A.secprof[40], (unsigned long long)nslot); atomicAdd(&A.secprof[41], 1ull); }   // update slots per pass
#endif
          const bool one_batch = nb == 1;   // (K <= 4: a group keeps ITS chain's accelerations in registers over the whole pass)
          int ci_safe = 0;   // (level 0 holds a contact: what a group without one in a slot reads; nothing of it is applied)
          for (int c = K - 1; c >= 0; c--) { const int x = lvl[c]; ci_safe = x >= 0 ? x : ci_safe; }
          // (K <= 4, every reference scene: slot = level, the group's chain is fixed -- no divisions by the batch count in the loop)
          auto chain_of = [&](int sl_) { return one_batch ? grp : 4 * (sl_ % nb) + grp; };
          auto contact_of = [&](int sl_) {
            if (one_batch) return (sl_ < nslot && grp < K) ? lvl[sl_ * K + grp] : -1;
            const int c = chain_of(sl_);
            return (sl_ < nslot && c < K) ? lvl[(sl_ / nb) * K + c] : -1;
          };
          int cc = grp < K ? grp : 0;
          double a0 = lo_w ? aFL[cc * CS + l] : 0.0, a1 = hi_w ? aFL[cc * CS + l + 16] : 0.0;   // (0 on a lane without a word: its J a terms vanish)
#if defined(SG_SECTION_PROF)
          long long tpa = 0, tpb = 0, tpc = 0, tpn = 0;   // cycles of an update's three parts (registers; added up once per pass, below)
#define SGT_TP(x) const long long x = clock64()
#else
#define SGT_TP(x) ((void)0)
#endif
          auto update = [&](const CRec& q, const bool act) {
            SGT_TP(t0_);
            const int ci = q.ci, sl = (int)q.slf;
            const double p0 = rowsum16(q.j0 * a0 + q.k0 * a1), p1 = rowsum16(q.j1 * a0 + q.k1 * a1), p2 = rowsum16(q.j2 * a0 + q.k2 * a1);
            const double as_ = sl >= 0 ? aeL[sl] : 0.0;
            double f[3] = {cfL[3 * ci], cfL[3 * ci + 1], cfL[3 * ci + 2]}, df[3];
            const double res[3] = {q.B[0] + q.Js[0] * as_ + p0 + q.R * f[0], q.B[1] + q.Js[1] * as_ + p1 + q.R * f[1], q.B[2] + q.Js[2] * as_ + p2 + q.R * f[2]};
#if defined(SG_SECTION_PROF)
            asm volatile("" :: "v"(res[0]), "v"(res[1]), "v"(res[2]));
#endif
            SGT_TP(t1_);
            const double ch = contact_block_update_pre(q.A, q.Pe, res, f, con_mu, df);
#if defined(SG_SECTION_PROF)
            asm volatile("" :: "v"(df[0]), "v"(df[1]), "v"(df[2]), "v"(ch));
#endif
            SGT_TP(t2_);
            if (act) {
              if (lo_w) a0 += q.w0 * df[0] + q.w1 * df[1] + q.w2 * df[2];
              if (hi_w) a1 += q.x0 * df[0] + q.x1 * df[1] + q.x2 * df[2];
              if (l == 0) {
                imp_par -= ch;
                cfL[3 * ci] = f[0]; cfL[3 * ci + 1] = f[1]; cfL[3 * ci + 2] = f[2];
                if (sl >= 0) aeL[sl] += q.invm * (q.Js[0] * df[0] + q.Js[1] * df[1] + q.Js[2] * df[2]);
              }
            }
#if defined(SG_SECTION_PROF)
            asm volatile("" :: "v"(a0), "v"(a1));
            { const long long t3_ = clock64(); tpa += t1_ - t0_; tpb += t2_ - t1_; tpc += t3_ - t2_; tpn++; }
#endif
          };
          // one slot: more than four chains -> the group's chain changes from slot to slot, its accelerations go through LDS
          auto slot = [&](const CRec& q, int sl_, int ci) {
            if (!one_batch) {
              const int c = chain_of(sl_);
              cc = c < K ? c : 0;
              a0 = lo_w ? aFL[cc * CS + l] : 0.0; a1 = hi_w ? aFL[cc * CS + l + 16] : 0.0;
            }
            update(q, ci >= 0);
            if (!one_batch && ci >= 0) {
              if (lo_w) aFL[cc * CS + l] = a0;
              if (hi_w) aFL[cc * CS + l + 16] = a1;
            }
          };
          CRec ra, rb;   // two register sets: no copies, the other set's loads in flight during an update
          int cia = contact_of(0), cib;
          load_rec(ra, cia >= 0 ? cia : ci_safe);
          for (int j = 0; j < nslot; j += 2) {
            cib = contact_of(j + 1);
            load_rec(rb, cib >= 0 ? cib : ci_safe);
            slot(ra, j, cia);
            cia = contact_of(j + 2);
            load_rec(ra, cia >= 0 ? cia : ci_safe);
            slot(rb, j + 1, cib);
          }
          if (one_batch && grp < K) {
            if (lo_w) aFL[cc * CS + l] = a0;
            if (hi_w) aFL[cc * CS + l + 16] = a1;
          }
#if defined(SG_SECTION_PROF)
          if (threadIdx.x == 0) { atomicAdd(&A.secprof[42], (unsigned long long)tpa); atomicAdd(&A.secprof[43], (unsigned long long)tpn); atomicAdd(&A.secprof[46], (unsigned long long)tpb); atomicAdd(&A.secprof[47], (unsigned long long)tpc); }
#endif
#undef SGT_TP
        }
      }
#else
      for (int Lv = 0; Lv < S.icnt[IC_NLEV]; Lv++) {   // the levels in sequence, a level's contacts (one per chain at most) side by side
        SGT_PAR(c, K) {
          double* aFc = S.aF + c * CS;
          const int ci = S.hit_pair[Lv * K + c];
          if (ci < 0) continue;
          const double* sc = cscr(ci);
          const double* J = crow(ci);
          const double* W = J + 3 * CS;
          const int sl = (int)sc[CS_SL];
          double p0 = 0, p1 = 0, p2 = 0;
          // whole padded rows (J is zero beyond the body's dofs), unrolled over the capacity with every load issued up front: the rows
          // sit in global memory (L2), and a loop would pay that latency once per trip.  Beyond the padded stride CS (uniform) the
          // loads hit the record's other words (finite), against a zero.
#pragma unroll
          for (int k = 0; k < CHD; k++) {   // (one select, not three)
            const double a = k < CS ? aFc[k] : 0.0, j0 = J[k], j1 = J[CS + k], j2 = J[2 * CS + k];
            p0 += j0 * a; p1 += j1 * a; p2 += j2 * a;
          }
          double w0[CHD], w1[CHD], w2[CHD];   // the W rows are on their way while the block update runs
#pragma unroll
          for (int k = 0; k < CHD; k++) { w0[k] = W[k]; w1[k] = W[CS + k]; w2[k] = W[2 * CS + k]; }
          const double as_ = sl >= 0 ? S.ae[sl] : 0.0;
          double f[3] = {S.cf[3 * ci], S.cf[3 * ci + 1], S.cf[3 * ci + 2]}, df[3];
          const double res[3] = {sc[CS_B] + sc[CS_JS] * as_ + p0 + sc[CS_R] * f[0], sc[CS_B + 1] + sc[CS_JS + 1] * as_ + p1 + sc[CS_R] * f[1],
                                 sc[CS_B + 2] + sc[CS_JS + 2] * as_ + p2 + sc[CS_R] * f[2]};
          imp_par -= contact_block_update_pre(sc + CS_A, sc + CS_PE, res, f, con_mu, df);
          double an[CHD];
#pragma unroll
          for (int k = 0; k < CHD; k++) an[k] = aFc[k] + (w0[k] * df[0] + w1[k] * df[1] + w2[k] * df[2]);
#pragma unroll
          for (int k = 0; k < CHD; k += 4)
            if (k < CS) { aFc[k] = an[k]; aFc[k + 1] = an[k + 1]; aFc[k + 2] = an[k + 2]; aFc[k + 3] = an[k + 3]; }
          S.cf[3 * ci] = f[0]; S.cf[3 * ci + 1] = f[1]; S.cf[3 * ci + 2] = f[2];
          if (sl >= 0) S.ae[sl] += sc[CS_INVM] * (sc[CS_JS] * df[0] + sc[CS_JS + 1] * df[1] + sc[CS_JS + 2] * df[2]);
        }
        SGT_SYNC();
      }
#endif
      SGT_SYNC();
    }
    // ... or one serial list, the lanes spread over the dofs of a contact's chain block(s)
#if SGT_DEVICE
    // (r04) WAVE-SYNCHRONOUS when all chain words fit the wavefront (K CS <= 64: the free ball's two-finger gripper): lane c CS + d
    // keeps chain word d of chain c in a register for the whole pass, the free body's acceleration and S^-1 sit in registers on every
    // lane alike, a contact's J / W words, scalars and object columns come from the work space one contact AHEAD (two register
    // sets), J a is three wavefront sums (DPP), and nothing in the loop waits at a barrier.  Per contact the bulk-synchronous
    // version below pays two barriers -- each draining every outstanding load -- and two exposed round trips to the work space:
    // 7.6 k cycles an update, 70 % of a free-ball substep.
#ifdef SGT_X_NOSF
    const bool serial_fast = false;
#else
    const bool serial_fast = serial_contacts && K * CS <= 64;
#endif
    if (serial_fast) {
      const int lane = (int)threadIdx.x;
      const bool dofl = lane < K * CS;
      const int mc = dofl ? lane / CS : -1, mdl = dofl ? lane % CS : 0;
      // (with a free object its LDS arrays -- B_e, 1 / m, C_e -- are read through typed pointers too: FR is a fact of the instantiation)
      const SGT_LDSP double* const einvmL = (const SGT_LDSP double*)S.einvm;
      const SGT_LDSP double* const CeL = (const SGT_LDSP double*)S.Ce;
      double a = dofl ? aFL[lane] : 0.0;
      // (r05) The body's push a_f += S^-1 w is spread over six lanes: lane q < 6 keeps ROW q of S^-1 and computes component q, six scalar
      // reads hand the result to every lane.  All 36 words on every lane -- parked in accumulation registers and fetched back for each
      // product -- were 108 instructions per contact, and the slider's share C_sl dg_e = -S^-1 B_sl dg_e / D_sl a second such product:
      // now ONE product, S^-1 (J_o' df - B_sl dg_e / D_sl).  ~900 instructions per contact before, a wavefront alone on its SIMD pays ~7
      // cycles for each.
      double af[6] = {0, 0, 0, 0, 0, 0}, gf[6] = {0, 0, 0, 0, 0, 0}, Siq[6] = {0, 0, 0, 0, 0, 0};
      if (FR) {
        const int qr = (lane & 7) < 6 ? (lane & 7) : 5;
#pragma unroll
        for (int q = 0; q < 6; q++) { af[q] = ofL[OF_AF + q]; gf[q] = ofL[OF_GF + q]; Siq[q] = ofL[OF_SINV + 6 * qr + q]; }
      }
      // J a: sums over the lanes that hold chain words, the first K CS of the wavefront -- 8 for a two-finger gripper: a butterfly inside
      // every group of eight lanes (the three rows' sums side by side: each step's DPP moves wait two cycles for the add in front of them),
      // then one scalar read per group in use (a loop over a scalar count: a branch the compiler cannot turn into "do all and select")
      const int ngrp = __builtin_amdgcn_readfirstlane((K * CS + 7) >> 3);
      auto chain_sums = [&](double& x0, double& x1, double& x2) {
        { const double t0 = dpp64<0xB1>(x0), t1 = dpp64<0xB1>(x1), t2 = dpp64<0xB1>(x2); x0 += t0; x1 += t1; x2 += t2; }
        { const double t0 = dpp64<0x4E>(x0), t1 = dpp64<0x4E>(x1), t2 = dpp64<0x4E>(x2); x0 += t0; x1 += t1; x2 += t2; }
        { const double t0 = dpp64<0x141>(x0), t1 = dpp64<0x141>(x1), t2 = dpp64<0x141>(x2); x0 += t0; x1 += t1; x2 += t2; }
        double s0 = readlane64(x0, 0), s1 = readlane64(x1, 0), s2 = readlane64(x2, 0);
        for (int gq = 1; gq < ngrp; gq++) { s0 += readlane64(x0, 8 * gq); s1 += readlane64(x1, 8 * gq); s2 += readlane64(x2, 8 * gq); }
        x0 = s0; x1 = s1; x2 = s2;
      };
      struct SRec { double j0, j1, j2, w0, w1, w2, A[6], Pe[7], B[3], R, invm, Js[3], slf, rowsf, objf, Jo[18]; int ci; };
      auto load_srec = [&](SRec& q, int ci) {
        const double* J = crow(ci);
        const double* sc = J + 12 * CS;
        const int cc12 = hitcntL[ci];   // (c1 + 1) | (c2 + 1) << 8, packed with the rows
        const int c1 = (cc12 & 0xff) - 1, c2 = ((cc12 >> 8) & 0xff) - 1;
        const int blk = (dofl && mc == c1) ? 0 : ((dofl && mc == c2) ? 1 : -1);
        const double* Jb = J + (blk == 1 ? 6 * CS : 0) + (blk >= 0 ? mdl : 0);
        const double z = blk >= 0 ? 1.0 : 0.0;
        q.ci = ci;
        q.j0 = z * Jb[0]; q.j1 = z * Jb[CS]; q.j2 = z * Jb[2 * CS];
        q.w0 = z * Jb[3 * CS]; q.w1 = z * Jb[4 * CS]; q.w2 = z * Jb[5 * CS];
#pragma unroll
        for (int k = 0; k < 6; k++) q.A[k] = sc[CS_A + k];
#pragma unroll
        for (int k = 0; k < 3; k++) { q.B[k] = sc[CS_B + k]; q.Js[k] = sc[CS_JS + k]; }
        q.R = sc[CS_R]; q.invm = sc[CS_INVM]; q.slf = sc[CS_SL]; q.rowsf = sc[CS_ROWS]; q.objf = sc[CS_OBJ];
#pragma unroll
        for (int k = 0; k < 7; k++) q.Pe[k] = sc[CS_PE + k];
        if (FR) {
#pragma unroll
          for (int k = 0; k < 18; k++) q.Jo[k] = sc[CS_JO + k];
        }
      };
      auto update = [&](const SRec& q, const bool have) {
        // (the record's words are the same on every lane: as scalars, the branches on them are real branches, not masked regions)
        const int ci = q.ci, sl = __builtin_amdgcn_readfirstlane((int)q.slf);
        const bool act = have && __builtin_amdgcn_readfirstlane((int)(q.rowsf != 0.0)) != 0, ob = FR && __builtin_amdgcn_readfirstlane((int)(q.objf != 0.0)) != 0;
        double p0 = q.j0 * a, p1 = q.j1 * a, p2 = q.j2 * a;
        chain_sums(p0, p1, p2);
        if (ob) { p0 += dot6(q.Jo, af); p1 += dot6(q.Jo + 6, af); p2 += dot6(q.Jo + 12, af); }
        double as_ = 0.0;
        // (r05) the slider's B_sl and 1 / D_sl are read ONCE, for the slider's acceleration here and for its share of the body's push below:
        // read again there (the stores in between may alias them, as far as the compiler knows) they were six more LDS reads and a wait
        // in every update's dependency chain -- free ball +1.5 %
        double Bs_[6] = {0, 0, 0, 0, 0, 0}, eim = 0.0;
        if (sl >= 0) {
          if (FR) {
#pragma unroll
            for (int k = 0; k < 6; k++) Bs_[k] = BeL[6 * sl + k];
            eim = einvmL[sl];
            as_ = aeL[sl] - (Bs_[0] * af[0] + Bs_[1] * af[1] + Bs_[2] * af[2] + Bs_[3] * af[3] + Bs_[4] * af[4] + Bs_[5] * af[5]) * eim;
          } else as_ = aeL[sl];
        }
        double f[3] = {cfL[3 * ci], cfL[3 * ci + 1], cfL[3 * ci + 2]}, df[3];
        const double res[3] = {q.B[0] + q.Js[0] * as_ + p0 + q.R * f[0], q.B[1] + q.Js[1] * as_ + p1 + q.R * f[1], q.B[2] + q.Js[2] * as_ + p2 + q.R * f[2]};
        const double ch = contact_block_update_pre(q.A, q.Pe, res, f, con_mu, df);
        if (act) {
          imp_uni -= ch;
          a += q.w0 * df[0] + q.w1 * df[1] + q.w2 * df[2];
          const double dge = sl >= 0 ? q.Js[0] * df[0] + q.Js[1] * df[1] + q.Js[2] * df[2] : 0.0;
          if (lane == 0) {
            cfL[3 * ci] = f[0]; cfL[3 * ci + 1] = f[1]; cfL[3 * ci + 2] = f[2];
            if (sl >= 0) aeL[sl] += q.invm * dge;
          }
          if (ob) {   // the push on the body: g_f += J_o' df; a_f += S^-1 J_o' df + C_sl dg_e, C_sl = -S^-1 B_sl / D_sl
            double dg[6], w6[6];
#pragma unroll
            for (int k = 0; k < 6; k++) { dg[k] = q.Jo[k] * df[0] + q.Jo[6 + k] * df[1] + q.Jo[12 + k] * df[2]; w6[k] = dg[k]; }
            double Cs[6] = {0, 0, 0, 0, 0, 0};   // the neighbour-row models keep C_sl (S.Ce); the others fold the slider's share into the one product
            if (sl >= 0) {
              if (NB) {
#pragma unroll
                for (int k = 0; k < 6; k++) Cs[k] = CeL[6 * sl + k];
              } else {
                const double sh = dge * eim;
#pragma unroll
                for (int k = 0; k < 6; k++) w6[k] -= Bs_[k] * sh;
              }
            }
            const double daq = dot6(Siq, w6);   // lane q < 6: component q of S^-1 w
#pragma unroll
            for (int k = 0; k < 6; k++) { gf[k] += dg[k]; af[k] += NB ? readlane64(daq, k) + Cs[k] * dge : readlane64(daq, k); }
          }
        }
      };
      if (ncon > 0) {
        SRec ra, rb;
        load_srec(ra, 0);
        for (int j = 0; j < ncon; j += 2) {
          load_srec(rb, j + 1 < ncon ? j + 1 : 0);
          update(ra, true);
          load_srec(ra, j + 2 < ncon ? j + 2 : 0);
          update(rb, j + 1 < ncon);
        }
      }
      if (dofl) aFL[lane] = a;
      if (FR && lane == 0) {
#pragma unroll
        for (int q = 0; q < 6; q++) { ofL[OF_AF + q] = af[q]; ofL[OF_GF + q] = gf[q]; }
      }
      SGT_SYNC();
    }
    for (int ci = 0; serial_contacts && !serial_fast && ci < ncon; ci++) {
#else
    for (int ci = 0; serial_contacts && ci < ncon; ci++) {
#endif
      const double* sc = cscr(ci);
      if (sc[CS_ROWS] == 0.0) continue;
      const int c1 = (int)sc[CS_C1], c2 = (int)sc[CS_C2], n1 = (int)sc[CS_N1], n2 = (int)sc[CS_N2], sl = (int)sc[CS_SL];
      double p0 = 0, p1 = 0, p2 = 0;
      SGT_PAR(i, n1 + n2) {
        const bool second = i >= n1;
        const int dl = second ? i - n1 : i;
        const double* J = crow(ci) + (second ? 6 * CS : 0);
        const double a = S.aF[(second ? c2 : c1) * CS + dl];
        p0 += J[dl] * a; p1 += J[CS + dl] * a; p2 += J[2 * CS + dl] * a;
      }
      p0 = wsum(p0); p1 = wsum(p1); p2 = wsum(p2);
      const bool ob = FR && sc[CS_OBJ] != 0.0;
      if (ob) { p0 += dot6(sc + CS_JO, S.of + OF_AF); p1 += dot6(sc + CS_JO + 6, S.of + OF_AF); p2 += dot6(sc + CS_JO + 12, S.of + OF_AF); }
      const double as_ = sl >= 0 ? slider_acc(sl) : 0.0;
      double f[3] = {S.cf[3 * ci], S.cf[3 * ci + 1], S.cf[3 * ci + 2]}, df[3];
      const double res[3] = {sc[CS_B] + sc[CS_JS] * as_ + p0 + sc[CS_R] * f[0], sc[CS_B + 1] + sc[CS_JS + 1] * as_ + p1 + sc[CS_R] * f[1],
                             sc[CS_B + 2] + sc[CS_JS + 2] * as_ + p2 + sc[CS_R] * f[2]};
      imp_uni -= contact_block_update_pre(sc + CS_A, sc + CS_PE, res, f, con_mu, df);
      SGT_SYNC();   // every lane has read the old forces and accelerations
      const int n1c = c1 >= 0 ? CS : 0, n2c = c2 >= 0 ? CS : 0;
      SGT_PAR(i, n1c + n2c) {
        const bool second = i >= n1c;
        const int dl = second ? i - n1c : i;
        const double* W = crow(ci) + (second ? 9 * CS : 3 * CS);
        S.aF[(second ? c2 : c1) * CS + dl] += W[dl] * df[0] + W[CS + dl] * df[1] + W[2 * CS + dl] * df[2];
      }
      SGT_ONE {
        S.cf[3 * ci] = f[0]; S.cf[3 * ci + 1] = f[1]; S.cf[3 * ci + 2] = f[2];
        const double dge = sl >= 0 ? sc[CS_JS] * df[0] + sc[CS_JS + 1] * df[1] + sc[CS_JS + 2] * df[2] : 0.0;
        if (sl >= 0) S.ae[sl] += sc[CS_INVM] * dge;
        if (ob) {   // the push on the body: g_f += J_o' df; a_f += S^-1 J_o' df + C_sl dg_e
          double dg[6], da[6];
          for (int q = 0; q < 6; q++) dg[q] = sc[CS_JO + q] * df[0] + sc[CS_JO + 6 + q] * df[1] + sc[CS_JO + 12 + q] * df[2];
          mat6vec(da, S.of + OF_SINV, dg);
          double Cs[6] = {0, 0, 0, 0, 0, 0};
          if (sl >= 0) {
            if (NB) { for (int q = 0; q < 6; q++) Cs[q] = S.Ce[6 * sl + q]; }
            else {
              double Bs[6];
              mat6vec(Bs, S.of + OF_SINV, S.Be + 6 * sl);
              for (int q = 0; q < 6; q++) Cs[q] = -Bs[q] * S.einvm[sl];
            }
          }
          for (int q = 0; q < 6; q++) { S.of[OF_GF + q] += dg[q]; S.of[OF_AF + q] += da[q] + Cs[q] * dge; }
        }
      }
      SGT_SYNC();
    }
    SGT_STAMP(13);
    const double improvement = (wsum(imp_par) + imp_uni) * H.pgs_scale;
    iters = it + 1;
    if (improvement < H.tolerance) break;
  }

  SGT_ONE { S.swc[SWC_ITERS] = iters; S.swc[SWC_TEN_F] = ten_f; }
}

}  // namespace sgt
