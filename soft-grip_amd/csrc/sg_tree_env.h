// sg_tree_env.h -- the tree pipeline's driver (part of sg_tree.h): state in, the substeps as calls of the four stage functions, state
// and outputs back
#pragma once

namespace sgt {

// the whole call for one env.  lane: threadIdx.x on the device, 0 on the host
// CHD: the unroll capacity of the per-chain loops (>= the plan's padded stride CS): the kernel is instantiated for 8, 20 and 24
template <int CHD = SGT_CHD>
SG_HD void tree_env(const TreeArgs& A, const int env, double* lds_base) {
#define SGT_FRAME SGT_FRAME_TABLES
#include "sg_tree_frame.inc"

  if (A.mode == 1 && A.mask && !A.mask[env]) return;   // masked reset: the other envs keep everything
#define SGT_FRAME SGT_FRAME_STATE
#include "sg_tree_frame.inc"

  // ---------------------------------------------------------------- state in
  SGT_PAR(d, ND) {
    const int j = T.d_gid[d];
    const bool rs = A.mode == 1;
    S.q[d] = rs ? T.d_qpos0[d] : gq[j];
    S.v[d] = rs ? 0.0 : gv[j];
    S.warm[d] = rs ? 0.0 : gw[j];
    S.kd[d] = A.kmask_jnt[j] ? kenv : T.d_stiffness[d];
    S.qacc[d] = 0;
  }
  SGT_PAR(e, N) {
    const int jd = H.elem_dof0 + e, jq = H.elem_qpos0 + e;
    const bool rs = A.mode == 1;
    S.qe[e] = rs ? E(SGE_QPOS0, e) : gq[jq];
    S.ve[e] = rs ? 0.0 : gv[jd];
    S.we[e] = rs ? 0.0 : gw[jd];
    S.ke[e] = A.kmask_jnt[H.elem_jnt0 + e] ? kenv : E(SGE_K0, e);
    S.einvm[e] = 1.0 / (E(SGE_MASS, e) + E(SGE_ARMATURE, e));
    S.ecoef[e] = E(SGE_COEF, e);
    if (FR) {   // B_e = m_e (a_e ; k_e x a_e): the slider's column of the object's mass matrix, body frame (constant)
      const double m = E(SGE_MASS, e), a[3] = {E(SGE_AX, e), E(SGE_AY, e), E(SGE_AZ, e)}, k0[3] = {E(SGE_KX, e), E(SGE_KY, e), E(SGE_KZ, e)};
      double kxa[3];
      cross3(kxa, k0, a);
      for (int c = 0; c < 3; c++) { S.Be[6 * e + c] = m * a[c]; S.Be[6 * e + 3 + c] = m * kxa[c]; }
    }
  }
  if (FR) {
    SGT_ONE {
      const bool rs = A.mode == 1;
      for (int c = 0; c < 7; c++) S.of[OF_P + c] = rs ? H.free_q0[c] : gq[H.free_qadr + c];
      for (int c = 0; c < 3; c++) { S.of[OF_VW + c] = rs ? 0.0 : gv[H.free_dadr + c]; S.of[OF_WL + c] = rs ? 0.0 : gv[H.free_dadr + 3 + c]; }
      for (int c = 0; c < 6; c++) S.of[OF_WARM + c] = rs ? 0.0 : gw[H.free_dadr + c];   // warmstart in dof coordinates (world translations)
    }
  }
  SGT_PAR(c, K) {
    double* cs = S.chs + c * CHS_N;
    const bool rs = A.mode == 1;
    cs[CHS_ACT] = (T.a_has[c] && !rs) ? gact[T.a_id[c]] : 0.0;
    cs[CHS_CTRL] = (T.a_has[c] && !rs) ? gctrl[T.a_id[c]] : 0.0;
    cs[CHS_KT] = T.t_has[c] ? (A.kmask_ten[T.t_id[c]] ? kenv : T.t_k0[c]) : 0.0;
  }
  SGT_ONE {
    for (int i = 0; i < 32; i++) S.icnt[i] = 0;
    if (A.mode == 1)
      for (int u = 0; u < nu; u++) gctrl[u] = 0.0;   // mj_resetData clears ctrl
  }
  SGT_ONE { for (int i = 0; i < CTX_N; i++) S.ctx[i] = 0; }
  SGT_SYNC();

  const int nfwd = A.nsub + (A.mode == 1 ? 1 : 0);
  SGT_PAR(i, 3 * T.NG) S.gsz[i] = T.g_size[i / 3][i % 3];   // the boxes' half sizes next to their poses (the pair walk's tight test)
  for (int sub = 0; sub < nfwd; sub++) {
    SGT_ONE { S.ctx[CTX_SUB] = sub; S.ctx[CTX_LAST] = sub == nfwd - 1 ? 1.0 : 0.0; S.ctx[CTX_INTEGRATE] = (A.mode == 1 && sub == 0) ? 0.0 : 1.0; }
    SGT_SYNC();
    SGT_STAGE_CALL(dynamics);
    if (S.ctx[CTX_STOP] != 0.0) break;   // (uniform: bad positions / velocities -- the env stops integrating for the rest of the call)
    SGT_STAGE_CALL(collision);
    SGT_STAGE_CALL(constraints);
    SGT_STAGE_CALL(finish);
    if (S.ctx[CTX_STOP] != 0.0) break;   // (bad accelerations)
  }
  const int flags = (int)S.ctx[CTX_FLAGS], ncon = (int)S.ctx[CTX_NCON], nefc = (int)S.ctx[CTX_NEFC], iters = (int)S.ctx[CTX_ITERS];
  const unsigned touch_lo = (unsigned)S.ctx[CTX_TLO], touch_hi = (unsigned)S.ctx[CTX_THI];

  // ---------------------------------------------------------------- state and outputs back
  SGT_SYNC();
  SGT_PAR(d, ND) {
    const int j = T.d_gid[d];
    gq[j] = S.q[d]; gv[j] = S.v[d]; gw[j] = S.warm[d];
  }
  SGT_PAR(e, N) {
    const int jd = H.elem_dof0 + e;
    gq[H.elem_qpos0 + e] = S.qe[e]; gv[jd] = S.ve[e]; gw[jd] = S.we[e];
  }
  if (FR) SGT_ONE {
    for (int c = 0; c < 7; c++) gq[H.free_qadr + c] = S.of[OF_P + c];
    for (int c = 0; c < 3; c++) { gv[H.free_dadr + c] = S.of[OF_VW + c]; gv[H.free_dadr + 3 + c] = S.of[OF_WL + c]; }
    for (int c = 0; c < 6; c++) gw[H.free_dadr + c] = S.of[OF_WARM + c];
  }
  SGT_PAR(c, K)
    if (T.a_has[c]) gact[T.a_id[c]] = S.chs[c * CHS_N + CHS_ACT];
#ifdef SG_DEBUG_WORK
  {
    SGT_SYNC();
    const long long nl = (long long)(lds_bytes(T, N, H.has_free, H.nnb) / sizeof(double)), at = cws_doubles(T, N, H.has_free, H.nnb) - nl;
    SGT_PAR(i, nl) cw[at + i] = lds_base[i];
  }
#endif
  SGT_ONE {
    A.flags[env] = flags; A.ncon[env] = ncon; A.nefc[env] = nefc; A.iters[env] = iters;
    A.touch[env] = (int)touch_lo;
    A.touch_words[2 * env] = (int)touch_lo; A.touch_words[2 * env + 1] = (int)touch_hi;
  }
}

}  // namespace sgt
