// sg_tree_stage_finish.h -- the last stage of a substep: qacc, sensors, Euler with implicit joint damping (part of sg_tree.h)
#pragma once

namespace sgt {

template <int CHD>
static SGT_STAGE_ATTR void tree_stage_finish(SGT_STAGE_PARAMS) {
#define SGT_FRAME SGT_FRAME_STAGE_HEAD
#include "sg_tree_frame.inc"
  {
    // ---------------------------------------------------------------- qacc, qfrc_constraint, warmstart, sensors
    SGT_PAR(d, ND) {
      const int c = T.d_chain[d], dl = d - T.c_dof0[c];
      double s = 0;
      const double* rows = S.lrow + SGT_LROW * 2 * T.c_dof0[c];
      for (int i = 0; i < S.icnt[IC_NLIM0 + c]; i++)
        if ((int)rows[SGT_LROW * i] == dl) s += rows[SGT_LROW * i + 1] * rows[SGT_LROW * i + 4];
      for (int ci = 0; ci < ncon; ci++) {
        const double* sc = cscr(ci);
        if (sc[CS_ROWS] == 0.0) continue;
        for (int b = 0; b < 2; b++)
          if ((int)sc[b ? CS_C2 : CS_C1] == c && dl < (int)sc[b ? CS_N2 : CS_N1]) {
            const double* J = crow(ci) + (b ? 6 * CS : 0);
            s += J[dl] * S.cf[3 * ci] + J[CS + dl] * S.cf[3 * ci + 1] + J[2 * CS + dl] * S.cf[3 * ci + 2];
          }
      }
      S.fc[d] = s;
      S.qacc[d] = S.asm_[d] + S.aF[pidx(d)];
      S.warm[d] = S.qacc[d];
    }
    double badacc = 0;
    SGT_PAR(d, ND) badacc += isbad(S.qacc[d]) ? 1.0 : 0.0;
    SGT_PAR(e, N) {
      const double qa = S.asme[e] + slider_acc(e);
      S.we[e] = qa;
      badacc += isbad(qa) ? 1.0 : 0.0;
    }
    if (FR) {   // the body: qacc in dof coordinates (translations along the world axes) is what the next solve warmstarts from
      double qf[6], tw[3];
      for (int q = 0; q < 6; q++) { qf[q] = S.of[OF_ASM + q] + S.of[OF_AF + q]; badacc += isbad(qf[q]) ? 1.0 / 64 : 0.0; }
      mulmat3(tw, S.of + OF_R, qf);
      SGT_SYNC();
      SGT_ONE { for (int q = 0; q < 3; q++) { S.of[OF_WARM + q] = tw[q]; S.of[OF_WARM + 3 + q] = qf[3 + q]; } }
    }
    badacc = wsum(badacc);
    SGT_SYNC();
    if (last && A.sens) {   // sensordata of the call = that of the last forward pass
      tree_motion(S.qacc);
      SGT_SYNC();
      SGT_PAR(i, T.NSENS) {
        const int s = T.sn_site[i], tb = T.s_body[s];
        double sm[9], out[3];
        mulmat33(sm, S.xmat + 9 * tb, T.s_mat[s]);
        if (T.sn_type[i] == SG_SENS_GYRO) {
          mulmatT3(out, sm, S.bw + 3 * tb);
        } else {
          const double *w = S.bw + 3 * tb, *al = S.bal + 3 * tb;
          double r[3], a[3], t[3], t2[3];
          for (int k = 0; k < 3; k++) { r[k] = S.spos[3 * s + k] - S.xpos[3 * tb + k]; a[k] = S.ba[3 * tb + k]; }
          cross3(t, al, r); addscl3(a, t, 1);
          cross3(t, w, r); cross3(t2, w, t); addscl3(a, t2, 1);
          mulmatT3(out, sm, a);
        }
        double* so = A.sens + (size_t)env * A.sens_stride + T.sn_adr[i];
        so[0] = out[0]; so[1] = out[1]; so[2] = out[2];
      }
    }
    if (badacc > 0) { flags |= SG_FLAG_BADQACC; stop = 1; goto stage_done; }
    if (!integrate) goto stage_done;
    SGT_STAMP(15);
    // ---------------------------------------------------------------- stage 12: Euler with implicit joint damping
    SGT_PAR(i, T.NMAT) {
      const int c = i / (CS * CS), a = (i % (CS * CS)) / CS, b = i % CS;
      S.L[i] = Mg[i] + ((a == b && a < T.c_ndof[c]) ? h * T.d_damping[T.c_dof0[c] + a] : 0.0);
    }
    SGT_PAR(i, K * CS) S.tmpP[i] = 0;
    SGT_SYNC();
    SGT_PAR(d, ND) S.tmpP[pidx(d)] = S.fs[d] + S.fc[d];   // right-hand side, padded
    factor_all();
    SGT_PAR(c, K) {
      chain_solve_reg<CHD>(S.L + c * CS * CS, CS, S.tmpP + c * CS);
      double* cs = S.chs + c * CHS_N;
      cs[CHS_ACT] += h * cs[CHS_ACTDOT];
    }
    double Jx = 0, Jy = 0;
    if (FR) {
      // (M + h B) x = f for the arrow matrix: D' = D + h d, S' = M_ff - sum B B' / D' (the sum is a plan constant); the same solve for
      // y = (M + h B)^-1 J' of the volume tendon (D5: Sherman-Morrison on top of it)
      double Sh[36], Shi[36], rf[6] = {0, 0, 0, 0, 0, 0}, xf[6], yf[6], t6[6];
      {
        int qq = 0;
        for (int r = 0; r < 6; r++)
          for (int q = r; q < 6; q++) { Sh[6 * r + q] = Sh[6 * q + r] = S.of[OF_MFF + qq] - H.obj_BBDh[qq]; qq++; }
      }
      spd_inverse6(Sh, Shi);
      SGT_PAR(e, N) {
        const double D = E(SGE_MASS, e) + E(SGE_ARMATURE, e), den = D + h * E(SGE_DAMPING, e), r = (S.fse[e] + D * S.ae[e]) / den;   // (g_e = D x the local part)
        for (int q = 0; q < 6; q++) rf[q] += S.Be[6 * e + q] * r;
      }
      for (int q = 0; q < 6; q++) t6[q] = -S.of[OF_BIAS + q] + S.of[OF_GF + q] - wsum(rf[q]);
      mat6vec(xf, Shi, t6);
      for (int q = 0; q < 6; q++) t6[q] = -H.obj_tenBh[q];
      mat6vec(yf, Shi, t6);
      SGT_PAR(e, N) {
        const double D = E(SGE_MASS, e) + E(SGE_ARMATURE, e), den = D + h * E(SGE_DAMPING, e), co = S.ecoef[e];
        const double x = (S.fse[e] + D * S.ae[e] - dot6(S.Be + 6 * e, xf)) / den, y = (co - dot6(S.Be + 6 * e, yf)) / den;
        S.asme[e] = x; S.Ifix[e] = y;   // (both arrays are rebuilt by the next forward pass)
        Jx += co * x; Jy += co * y;
      }
      Jx = wsum(Jx); Jy = wsum(Jy);
      const double kf = H.t0_implicit ? h * H.t0_damping * Jx / (1 + h * H.t0_damping * Jy) : 0.0;
      SGT_SYNC();
      SGT_PAR(e, N) {
        S.ve[e] += h * (S.asme[e] - kf * S.Ifix[e]);
        S.qe[e] += h * S.ve[e];
      }
      SGT_ONE {   // the body: velocities (world translations, body-frame rotations), then mj_integratePos with the new velocity
        double* o = S.of;
        double xw[3], xb[3] = {xf[0] - kf * yf[0], xf[1] - kf * yf[1], xf[2] - kf * yf[2]};
        mulmat3(xw, o + OF_R, xb);
        for (int q = 0; q < 3; q++) {
          o[OF_VW + q] += h * xw[q];
          o[OF_WL + q] += h * (xf[3 + q] - kf * yf[3 + q]);
          o[OF_P + q] += h * o[OF_VW + q];
        }
        const double* wl = o + OF_WL;
        const double nw = sqrt(dot3(wl, wl)), ang = h * nw;
        if (nw > SG_MINVAL) {   // mju_quatIntegrate: q <- q * (cos, axis sin), the axis in the body frame
          const double sn = sin(0.5 * ang), qr[4] = {cos(0.5 * ang), wl[0] / nw * sn, wl[1] / nw * sn, wl[2] / nw * sn};
          const double nq0 = sqrt(o[OF_Q] * o[OF_Q] + o[OF_Q + 1] * o[OF_Q + 1] + o[OF_Q + 2] * o[OF_Q + 2] + o[OF_Q + 3] * o[OF_Q + 3]);
          (void)nq0;
          quatmul(o + OF_Q, o + OF_Q, qr);
          const double nq = sqrt(o[OF_Q] * o[OF_Q] + o[OF_Q + 1] * o[OF_Q + 1] + o[OF_Q + 2] * o[OF_Q + 2] + o[OF_Q + 3] * o[OF_Q + 3]);
          for (int q = 0; q < 4; q++) o[OF_Q + q] /= nq;
        }
      }
    } else {
      SGT_PAR(e, N) {
        const double m = E(SGE_MASS, e) + E(SGE_ARMATURE, e), fce = m * S.ae[e], den = m + h * E(SGE_DAMPING, e), co = S.ecoef[e];
        const double x = (S.fse[e] + fce) / den;
        S.asme[e] = x;   // (asme is rebuilt by the next forward pass)
        Jx += co * x; Jy += co * co / den;
      }
      Jx = wsum(Jx); Jy = wsum(Jy);
      const double kk = H.t0_implicit ? h * H.t0_damping * Jx / (1 + h * H.t0_damping * Jy) : 0.0;   // D5: Sherman-Morrison
      SGT_SYNC();
      SGT_PAR(e, N) {
        const double den = E(SGE_MASS, e) + E(SGE_ARMATURE, e) + h * E(SGE_DAMPING, e);
        const double x = S.asme[e] - kk * E(SGE_COEF, e) / den;
        S.ve[e] += h * x;
        S.qe[e] += h * S.ve[e];
      }
    }
    SGT_PAR(d, ND) {
      S.v[d] += h * S.tmpP[pidx(d)];
      S.q[d] += h * S.v[d];
    }
    SGT_SYNC();
    SGT_STAMP(16);
  }
#define SGT_FRAME SGT_FRAME_STAGE_TAIL
#include "sg_tree_frame.inc"
}

}  // namespace sgt
