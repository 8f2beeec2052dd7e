// sg_tree_free.h -- the free object's equality rows in the PGS sweep (part of sg_tree.h): every joint-fix row moves the body, so they run
// in mj_solPGS's order -- one after the other, in blocks over the wavefront, or as equality blocks with the neighbour rows.
#pragma once

namespace sgt {

// The free object's joint-fix rows, one after the other (one lane).  A function of its own ON PURPOSE: inlined into the step kernel --
// 256 + 256 registers and spilling -- the loop's 40 live values went to scratch memory and a row cost 600 cycles; called, it gets a
// register allocation of its own.  The next row's 19 words are loaded before this row's dependent arithmetic.
static SGT_NOINLINE double free_fix_rows(const SGT_LDSP double* frow, const SGT_LDSP double* Be, const SGT_LDSP double* einvm, const SGT_LDSP double* Sinv,
                                         SGT_LDSP double* ffix, SGT_LDSP double* ae, SGT_LDSP double* af, int N) {
#if SGT_DEVICE && !defined(SGT_X_ROWS1LANE)
  // EIGHT LANES (r05; the caller enters with lanes 0 .. 7): lane q < 6 owns component q of the body's acceleration a_f, of B_e and of
  // C_e = -S^-1 B_e / D_e.  A row on one lane cost ~66 instructions -- 6 for B_e . a_f, 36 for C_e (recomputed per row since r04: the
  // array would not fit the LDS share of four workgroups per CU), 6 for a_f += C_e df -- and a wavefront alone on its SIMD pays ~7
  // cycles for each, whatever it is and however few lanes it feeds: 500 cycles a row, 40 % of a free-ball substep.  Here the dot product
  // is one multiply and an 8-lane DPP sum, C_e six multiply-adds per lane (row q of S^-1 in registers), the push one: ~40 instructions.
  // The scalar part of a row (residual, force, cost) runs on all eight lanes alike.  The next row's words are read one row ahead.
  const int q = (int)threadIdx.x & 7;
  const bool own = q < 6;
  const int qq = own ? q : 0;
  double afq = own ? af[qq] : 0.0, imp = 0;
  double Sq[6];
#pragma unroll
  for (int k = 0; k < 6; k++) Sq[k] = Sinv[6 * qq + k];
  double nr[4], nB[6], nBq = Be[qq], nf = ffix[0], na = ae[0], ni = einvm[0];
#pragma unroll
  for (int k = 0; k < 4; k++) nr[k] = frow[k];
#pragma unroll
  for (int k = 0; k < 6; k++) nB[k] = Be[k];
  for (int e = 0; e < N; e++) {
    double r4[4], B6[6];
    const double Bq = nBq, f = nf, ael = na, invm = ni;
#pragma unroll
    for (int k = 0; k < 4; k++) r4[k] = nr[k];
#pragma unroll
    for (int k = 0; k < 6; k++) B6[k] = nB[k];
    {  // (the row behind the last one is read too: the arrays are followed by other words of the LDS block, and the values are dropped)
      const int en = e + 1;
#pragma unroll
      for (int k = 0; k < 4; k++) nr[k] = frow[4 * en + k];
#pragma unroll
      for (int k = 0; k < 6; k++) nB[k] = Be[6 * en + k];
      nBq = Be[6 * en + qq]; nf = ffix[en]; na = ae[en]; ni = einvm[en];
    }
    double dot = own ? Bq * afq : 0.0;          // B_e . a_f over the six owner lanes (lanes 6, 7 add nothing)
    dot += dpp64<0xB1>(dot);                    // quad_perm [1,0,3,2]
    dot += dpp64<0x4E>(dot);                    // quad_perm [2,3,0,1]
    dot += dpp64<0x141>(dot);                   // row_half_mirror: the other quad of the eight
    double fn = f;
    imp -= scalar_update_rcp(fn, r4[0], ael - dot * invm, r4[1], r4[2], r4[3], false);
    const double dfl = fn - f;
    const double Cq = -(((Sq[0] * B6[0] + Sq[1] * B6[1]) + (Sq[2] * B6[2] + Sq[3] * B6[3])) + (Sq[4] * B6[4] + Sq[5] * B6[5])) * invm;
    afq += Cq * dfl;                            // (lanes 6, 7 carry a dummy: never stored)
    if (q == 0) { ffix[e] = fn; ae[e] = ael + invm * dfl; }
  }
  if (own) af[qq] = afq;
  return imp;
#else
  // C_e = -S^-1 B_e / D_e is RECOMPUTED per row (r04: 36 multiply-adds that do not depend on the previous row -- they run in the shadow
  // of its dependent chain) instead of read from a [N][6] array: without that array and the rows' copy of 1 / D the free ball's
  // LDS block is 37.8 KB instead of 50 -- four workgroups per CU instead of three.  Same expressions as the rows' build (tree_stage_constraints).
  double af6[6], imp = 0, Si[36];
  for (int q = 0; q < 6; q++) af6[q] = af[q];
  for (int q = 0; q < 36; q++) Si[q] = Sinv[q];
  double nr[4], nB[6], nC[6], nf = ffix[0], na = ae[0], ni = einvm[0];
  for (int q = 0; q < 4; q++) nr[q] = frow[q];
  for (int q = 0; q < 6; q++) nB[q] = Be[q];
  {
    double Bs[6];
    mat6vec(Bs, Si, nB);
    for (int q = 0; q < 6; q++) nC[q] = -Bs[q] * ni;
  }
#pragma unroll 2
  for (int e = 0; e < N; e++) {
    double r4[4], B6[6], C6[6], f = nf;
    const double ael = na, invm = ni;
    for (int q = 0; q < 4; q++) r4[q] = nr[q];
    for (int q = 0; q < 6; q++) { B6[q] = nB[q]; C6[q] = nC[q]; }
    {  // (on the device the row behind the last one is read too: the arrays are followed by other words of the LDS block, and the values
       //  are dropped; the host build reads the last row again -- its checking layout gives every array a heap block of its own)
      const int en = (SGT_DEVICE || e + 1 < N) ? e + 1 : e;
      for (int q = 0; q < 4; q++) nr[q] = frow[4 * en + q];
      for (int q = 0; q < 6; q++) nB[q] = Be[6 * en + q];
      nf = ffix[en]; na = ae[en]; ni = einvm[en];
      double Bs[6];
      mat6vec(Bs, Si, nB);
      for (int q = 0; q < 6; q++) nC[q] = -Bs[q] * ni;
    }
    const double old = f;
    imp -= scalar_update_rcp(f, r4[0], ael - dot6(B6, af6) * invm, r4[1], r4[2], r4[3], false);
    const double dfl = f - old;
    ffix[e] = f;
    ae[e] = ael + invm * dfl;
    for (int q = 0; q < 6; q++) af6[q] += C6[q] * dfl;
  }
  for (int q = 0; q < 6; q++) af[q] = af6[q];
  return imp;
#endif
}
#if SGT_DEVICE && !defined(SGT_X_ROWS8LANE) && !defined(SGT_X_ROWS1LANE)
#define SGT_FIXROWS_BLOCKED 1
// The free object's joint-fix rows IN BLOCKS (r05).  A row's update is affine in the body's acceleration a_f -- with u = B_e . a_f its force
// step is d = alpha_e + beta_e u (alpha_e = -(b + a_e + R f) / (A + R) from the row's own state, beta_e = (1 / D_e) / (A + R)) and
// a_f' = a_f + C_e d = (I + beta_e C_e B_e') a_f + alpha_e C_e -- and an equality row is never clamped or reverted (its step always lowers the
// cost: scalar_update_rcp's test cannot fire), so the sweep over the N rows is a chain of N affine maps of a 6-vector.  One after the other
// on eight lanes it was 500 cycles a row, 218 rows, 30 sweeps: 40 - 48 % of a free-ball substep (profiles/r05_tree_sections_freeball.txt).
// Here lane b < 32 owns a BLOCK of L consecutive rows (L = ceil(N / 32), made odd: the lanes' LDS addresses then fall into different banks):
//   1. every lane runs its block from a_f = 0 (-> c_b) and, beside it, the six unit vectors without the rows' alpha (-> M_b, 6 x 6):
//      the block as ONE affine map a_f -> M_b a_f + c_b.  M_b is constant over a substep's sweeps, but 36 values per lane have nowhere to
//      stay between two calls (the env's LDS block is full), so they are rebuilt: 78 instructions a row;
//   2. the scan: a_f at the start of block b + 1 = M_b (a_f at the start of block b) + c_b, block after block, the running a_f in scalar
//      registers (one matrix-vector product on every lane, lane b's result read back: ~57 instructions a block);
//   3. every lane runs its block again from its true start, now as the serial code does -- residual, force, cost, the slider's local part.
// ~3 300 instructions a sweep instead of 218 x 70.  Same mathematics as mj_solPGS's row-after-row sweep; the rounding differs (a block's
// successors see M_b a + c_b, not the sum its own rows accumulate: relative 1e-16 per block), as it already did between the oracle's serial
// dot product and the eight-lane tree sum.  Host builds (the emulation) keep the serial loop above.
// (INLINED into the sweep: as a called function -- 248 registers -- it saved 44 callee-saved registers to scratch memory on every call, 30
//  calls a substep: the free ball's fabric traffic went from 13.2 to 27.5 GB per sg_step call, profiles/r05_freeball_fix_hbm_traffic.json)
#if defined(SGT_X_BLOCKED_CALL)
#define SGT_BLOCKED_ATTR SGT_NOINLINE
#else
#define SGT_BLOCKED_ATTR __device__ __forceinline__
#endif
static SGT_BLOCKED_ATTR double free_fix_rows_blocked(const SGT_LDSP double* frow, const SGT_LDSP double* Be, const SGT_LDSP double* einvm, const SGT_LDSP double* Sinv,
                                                 SGT_LDSP double* ffix, SGT_LDSP double* ae, SGT_LDSP double* af, int N) {
  const int lane = (int)threadIdx.x;
  if (N <= 0) return 0.0;   // (a free body without sliders: no rows, a_f stays; uniform)
  const int L = ((N + 31) >> 5) | 1, nblk = (N + L - 1) / L;      // (uniform)
  const bool act = lane < nblk;
  const int e0 = act ? lane * L : 0;
  double Si[36];
#pragma unroll
  for (int k = 0; k < 36; k++) Si[k] = Sinv[k];
  struct Row { double b, R, A, I, B[6], C[6], f, al, im, z; int e; };
  auto load = [&](Row& w, int r) {
    const int e = e0 + r;
    const bool ok = act && e < N;
    const int ec = ok ? e : 0;
    w.e = ec; w.z = ok ? 1.0 : 0.0;
    w.b = frow[4 * ec]; w.R = frow[4 * ec + 1]; w.A = frow[4 * ec + 2]; w.I = frow[4 * ec + 3];
#pragma unroll
    for (int k = 0; k < 6; k++) w.B[k] = Be[6 * ec + k];
    w.f = ffix[ec]; w.al = ae[ec]; w.im = einvm[ec];
  };
  auto cvec = [&](Row& w) {   // C_e = -S^-1 B_e / D_e (same expressions as the rows' build and the serial loop)
#pragma unroll
    for (int q = 0; q < 6; q++)
      w.C[q] = -(((Si[6 * q] * w.B[0] + Si[6 * q + 1] * w.B[1]) + (Si[6 * q + 2] * w.B[2] + Si[6 * q + 3] * w.B[3])) + (Si[6 * q + 4] * w.B[4] + Si[6 * q + 5] * w.B[5])) * w.im;
  };
  // ---- 1. my block as an affine map
  double c[6] = {0, 0, 0, 0, 0, 0}, M[36];
#pragma unroll
  for (int k = 0; k < 36; k++) M[k] = (k % 7 == 0) ? 1.0 : 0.0;
  {
    Row w, wn;
    load(wn, 0);
    for (int r = 0; r < L; r++) {
      w = wn;
      load(wn, r + 1 < L ? r + 1 : r);
      cvec(w);
      const double beta = w.z * w.I * w.im, alpha = -(w.z * w.I) * ((w.b + w.al) + w.R * w.f);
      const double d = alpha + beta * dot6(w.B, c);
#pragma unroll
      for (int q = 0; q < 6; q++) c[q] += w.C[q] * d;
#pragma unroll
      for (int k = 0; k < 6; k++) {   // column k of M
        const double uk = beta * (((w.B[0] * M[k] + w.B[1] * M[6 + k]) + (w.B[2] * M[12 + k] + w.B[3] * M[18 + k])) + (w.B[4] * M[24 + k] + w.B[5] * M[30 + k]));
#pragma unroll
        for (int q = 0; q < 6; q++) M[6 * q + k] += w.C[q] * uk;
      }
    }
  }
  // ---- 2. the scan over the blocks: the running a_f is uniform (scalar registers), lane b keeps the value it had in front of block b
  // (lanes below b sit the step out: lane b's t is then final -- the a_f behind ITS block -- and block b + 1 starts from its left neighbour's t)
  double au[6], ain[6], t[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int q = 0; q < 6; q++) au[q] = af[q];
  for (int b = 0; b < nblk; b++) {
    if (lane >= b) {
#pragma unroll
      for (int q = 0; q < 6; q++)
        t[q] = ((c[q] + M[6 * q] * au[0]) + (M[6 * q + 1] * au[1] + M[6 * q + 2] * au[2])) + ((M[6 * q + 3] * au[3] + M[6 * q + 4] * au[4]) + M[6 * q + 5] * au[5]);
    }
#pragma unroll
    for (int q = 0; q < 6; q++) au[q] = readlane64(t[q], b);
  }
#pragma unroll
  for (int q = 0; q < 6; q++) {
    const double left = dpp64<0x138>(t[q]);   // wave_shr:1 -- lane l receives lane l - 1's word
    ain[q] = lane == 0 ? af[q] : left;
  }
  // ---- 3. my block's rows from their true start, as the serial sweep runs them
  double imp = 0;
  {
    Row w, wn;
    load(wn, 0);
    for (int r = 0; r < L; r++) {
      w = wn;
      load(wn, r + 1 < L ? r + 1 : r);
      cvec(w);
      const double Ja = w.al - dot6(w.B, ain) * w.im;
      const double res = w.b + Ja + w.R * w.f, fn = w.f - res * w.I, d = w.z * (fn - w.f);
      imp -= 0.5 * d * d * w.A + d * res;
      if (w.z != 0.0) { ffix[w.e] = fn; ae[w.e] = w.al + w.im * d; }
#pragma unroll
      for (int q = 0; q < 6; q++) ain[q] += w.C[q] * d;
    }
  }
  // the body's acceleration behind the last block
#pragma unroll
  for (int q = 0; q < 6; q++) {
    const double last = readlane64(ain[q], nblk - 1);
    if (lane == 0) af[q] = last;
  }
  return imp;
}
#endif
// The same with the composite's neighbour equalities: the equality BLOCKS [fix_e, e's neighbour rows (partner p: J = +1 on e, -1 on p)] in
// mj_solPGS's order.  A neighbour row moves two sliders and, through both, the body: a_f += (C_e - C_p) df.  (The neighbour rows' words
// sit in the work space: generic pointers.)
static SGT_NOINLINE double free_eq_blocks(const SGT_LDSP double* frow, const SGT_LDSP double* Be, const SGT_LDSP double* Ce, const SGT_LDSP double* einvm, SGT_LDSP double* ffix, SGT_LDSP double* ae,
                                          SGT_LDSP double* af, int N, const int* nbtab, double* nbf, const double* nbb, const double* nbR, const double* nbA,
                                          const double* nbI) {
  double af6[6], imp = 0;
  for (int q = 0; q < 6; q++) af6[q] = af[q];
  for (int e = 0; e < N; e++) {
    double B6[6], C6[6];
    for (int q = 0; q < 6; q++) { B6[q] = Be[6 * e + q]; C6[q] = Ce[6 * e + q]; }
    const double invm = einvm[e];
    double f = ffix[e], old = f, ael = ae[e];
    imp -= scalar_update_rcp(f, frow[4 * e], ael - dot6(B6, af6) * invm, frow[4 * e + 1], frow[4 * e + 2], frow[4 * e + 3], false);
    double dfl = f - old;
    ffix[e] = f;
    ael += invm * dfl;
    for (int q = 0; q < 6; q++) af6[q] += C6[q] * dfl;
    for (int d = 0; d < 3; d++) {
      const int k = d * N + e, pe = nbtab[k];
      if (pe < 0) continue;
      double Bp[6], Cp[6];
      for (int q = 0; q < 6; q++) { Bp[q] = Be[6 * pe + q]; Cp[q] = Ce[6 * pe + q]; }
      const double ipm = einvm[pe], apl = ae[pe];
      f = nbf[k]; old = f;
      imp -= scalar_update_rcp(f, nbb[k], (ael - dot6(B6, af6) * invm) - (apl - dot6(Bp, af6) * ipm), nbR[k], nbA[k], nbI[k], false);
      dfl = f - old;
      nbf[k] = f;
      ael += invm * dfl;
      ae[pe] = apl - ipm * dfl;
      for (int q = 0; q < 6; q++) af6[q] += (C6[q] - Cp[q]) * dfl;
    }
    ae[e] = ael;
  }
  for (int q = 0; q < 6; q++) af[q] = af6[q];
  return imp;
}

}  // namespace sgt
