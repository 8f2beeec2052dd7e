// sg_tree_stage_constraints.h -- the third stage of a substep: constraint rows (equality, limits, contacts), warmstart, the PGS sweeps (sg_tree_sweep.h) (part of sg_tree.h)
#pragma once

namespace sgt {

template <int CHD>
static SGT_STAGE_ATTR void tree_stage_constraints(SGT_STAGE_PARAMS) {
#define SGT_FRAME SGT_FRAME_STAGE_HEAD
#include "sg_tree_frame.inc"
  {
    // ---------------------------------------------------------------- stage 6: constraint rows
    // (a) equality rows: one joint-fix row per element, the tendon-fix row over all sliders
    double tj_pos = 0, tj_vel = 0, tj_asm = 0, tj_warm = 0, tj_A = 0;
    SGT_PAR(e, N) {
      const double pos = S.qe[e] - E(SGE_QPOS0, e), imp = impedance(H.eqj_solimp, pos, 0.0);
      const double R = fmax(SG_MINVAL, (1 - imp) / imp * E(SGE_INVW, e));
      const double aref = -H.eqj_B * S.ve[e] - H.eqj_K * imp * pos;
      S.Rfix[e] = R; S.bfix[e] = S.asme[e] - aref;
      S.ffix[e] = -(S.we[e] - aref) / R;
      const double co = S.ecoef[e], invm = S.einvm[e];
      double Aee = invm;
      if (FR) {   // the row reaches every slider through the body: [M^-1]_ee = 1/D + B' S^-1 B / D^2; C_e = -S^-1 B_e / D
        double Bs[6];
        mat6vec(Bs, S.of + OF_SINV, S.Be + 6 * e);
        Aee = invm + dot6(S.Be + 6 * e, Bs) * invm * invm;
        if (H.nnb > 0) for (int q = 0; q < 6; q++) S.Ce[6 * e + q] = -Bs[q] * invm;   // (kept for the neighbour-row blocks only: lds_carve)
        S.Afix[e] = Aee + R;
        double* fr4 = S.frow + 4 * e;
        fr4[0] = S.bfix[e]; fr4[1] = R; fr4[2] = Aee + R; fr4[3] = 1.0 / (Aee + R);
      }
      S.Ifix[e] = 1.0 / (Aee + R);
      if (!FR && H.nnb > 0) { double* const fq = S.fixq + 4 * e; fq[0] = S.bfix[e]; fq[1] = R; fq[2] = S.Ifix[e]; fq[3] = invm; }
      tj_pos += co * S.qe[e]; tj_vel += co * S.ve[e]; tj_asm += co * S.asme[e]; tj_warm += co * S.we[e]; tj_A += co * co * invm;
      // (d) limit rows of the slider: slot 0 lower side, slot 1 upper side (MuJoCo's order)
      for (int sd = 0; sd < 2; sd++) {
        const int side = 2 * sd - 1;
        double Rl = 0, bl = 0, fl = 0;   // R = 0 marks an inactive slot
        if (E(SGE_LIMITED, e) != 0.0) {
          const double dist = side * ((sd ? E(SGE_RHI, e) : E(SGE_RLO, e)) - S.qe[e]);
          if (dist < H.lime_margin) {
            const double sg = -side, impl = impedance(H.lime_solimp, dist, H.lime_margin);
            Rl = fmax(SG_MINVAL, (1 - impl) / impl * E(SGE_INVW, e));
            const double arefl = -H.lime_B * sg * S.ve[e] - H.lime_K * impl * (dist - H.lime_margin);
            const double jar = sg * S.we[e] - arefl;
            bl = sg * S.asme[e] - arefl;
            fl = jar < 0 ? -jar / Rl : 0.0;
          }
        }
        S.Rlim[2 * e + sd] = Rl; S.blim[2 * e + sd] = bl; S.flim[2 * e + sd] = fl;
        S.Ilim[2 * e + sd] = 1.0 / (invm + Rl);
      }
    }
    tj_pos = wsum(tj_pos); tj_vel = wsum(tj_vel); tj_asm = wsum(tj_asm); tj_warm = wsum(tj_warm); tj_A = wsum(tj_A);
    double cten[6] = {0, 0, 0, 0, 0, 0};   // free object: the tendon row's push on the body, C_ten = -S^-1 sum_e coef_e B_e / D_e
    if (FR) {
      double Bs[6];
      mat6vec(Bs, S.of + OF_SINV, H.obj_tenB);
      tj_A += dot6(H.obj_tenB, Bs);
      for (int q = 0; q < 6; q++) cten[q] = -Bs[q];
    }
    double ten_R, ten_b, ten_f;
    {
      const double pos = tj_pos - H.t0_L0, imp = impedance(H.eqt_solimp, pos, 0.0);
      ten_R = fmax(SG_MINVAL, (1 - imp) / imp * H.eqt_invw);
      const double aref = -H.eqt_B * tj_vel - H.eqt_K * imp * pos;
      ten_b = tj_asm - aref;
      ten_f = -(tj_warm - aref) / ten_R;
    }
    const double ten_I = 1.0 / (tj_A + ten_R);
#ifdef SGT_X_TAP   // (scripts/repro/tree_mono: the tendon row's intermediates into spare words of S.red, for a word-by-word comparison with the emulation)
    SGT_ONE { S.red[8] = tj_pos; S.red[9] = tj_vel; S.red[10] = tj_asm; S.red[11] = tj_warm; S.red[12] = tj_A; S.red[13] = ten_R; S.red[14] = ten_b; S.red[15] = H.t0_L0; }
#endif
    // (a') the composite's neighbour equalities q_e1 - q0_e1 = q_e2 - q0_e2 (MuJoCo's documented composite): slot
    //      d * N + e = the d-th row registered for element e (its partner: nbtab's out_e2); J = +1 on e, -1 on the partner
    const bool NB = H.nnb > 0;
    if (NB) {
      SGT_SYNC();   // (asme / we of other lanes' elements)
      SGT_PAR(k, 3 * N) {
        const int e = k % N, pe = nbtab[k];
        double R = 0, b = 0, f = 0, I = 0;   // R = 0 marks an empty slot
        if (pe >= 0) {
          const double pos = (S.qe[e] - E(SGE_QPOS0, e)) - (S.qe[pe] - E(SGE_QPOS0, pe)), imp = impedance(H.eqj_solimp, pos, 0.0);
          R = fmax(SG_MINVAL, (1 - imp) / imp * (E(SGE_INVW, e) + E(SGE_INVW, pe)));
          const double aref = -H.eqj_B * (S.ve[e] - S.ve[pe]) - H.eqj_K * imp * pos;
          b = (S.asme[e] - S.asme[pe]) - aref;
          f = -((S.we[e] - S.we[pe]) - aref) / R;
          double Arow = S.einvm[e] + S.einvm[pe];
          if (FR) {   // through the body too: [M^-1]_ee + [M^-1]_pp - 2 [M^-1]_ep, [M^-1]_xy = delta_xy / D_x + B_x' S^-1 B_y / (D_x D_y)
            double Se[6], Sp[6];
            mat6vec(Se, S.of + OF_SINV, S.Be + 6 * e);
            mat6vec(Sp, S.of + OF_SINV, S.Be + 6 * pe);
            const double ie = S.einvm[e], ip = S.einvm[pe];
            Arow += dot6(S.Be + 6 * e, Se) * ie * ie + dot6(S.Be + 6 * pe, Sp) * ip * ip - 2 * dot6(S.Be + 6 * e, Sp) * ie * ip;
            S.nbA[k] = Arow + R;
          }
          I = 1.0 / (Arow + R);
        }
        S.nbR[k] = R; S.nbb[k] = b; S.nbf[k] = f; S.nbI[k] = I;
        if (!FR) { double* const nq = S.nbq + 4 * k; nq[0] = R; nq[1] = b; nq[2] = I; nq[3] = pe >= 0 ? S.einvm[pe] : 0.0; }
      }
    }
    // (c) limit rows of the chain dofs, one lane per chain: compact list in dof order, lower side first
    SGT_PAR(c, K) {
      int n = 0;
      double* rows = S.lrow + SGT_LROW * 2 * T.c_dof0[c];
      for (int dl = 0; dl < T.c_ndof[c]; dl++) {
        const int d = T.c_dof0[c] + dl;
        if (!T.d_limited[d]) continue;
        for (int sd = 0; sd < 2; sd++) {
          const int side = 2 * sd - 1;
          const double dist = side * (T.d_range[d][sd] - S.q[d]);
          if (!(dist < T.d_margin[d])) continue;
          const double sg = -side, imp = impedance(T.d_solimp[d], dist, T.d_margin[d]);
          const double R = fmax(SG_MINVAL, (1 - imp) / imp * T.d_invw[d]);
          const double aref = -T.d_limB[d] * sg * S.v[d] - T.d_limK[d] * imp * (dist - T.d_margin[d]);
          const double jar = sg * S.warm[d] - aref;
          double* r = rows + SGT_LROW * n++;
          r[0] = dl; r[1] = sg; r[2] = R; r[3] = sg * S.asm_[d] - aref; r[4] = jar < 0 ? -jar / R : 0.0;
          r[5] = 1.0 / (S.Minv[c * CS * CS + dl * CS + dl] + R);
        }
      }
      S.icnt[IC_NLIM0 + c] = n;
    }
    SGT_STAMP(9);
    // (e) contact rows, one lane per contact
    SGT_PAR(ci, ncon) {
      const int src = S.con_src[ci], hi = src / SGT_HITREC;
      const double* rec = stage + (size_t)src * SGT_RECW;
      const SgGenPair gp = gpairs[S.hit_sorted[hi]];
      double* J1 = crow(ci);
      double *W1 = J1 + 3 * CS, *J2 = J1 + 6 * CS, *W2 = J1 + 9 * CS, *sc = cscal(ci);
      double fr[9];
      const double hint[3] = {rec[7], rec[8], rec[9]};
      make_frame_hint(rec + 4, (hint[0] != 0 || hint[1] != 0 || hint[2] != 0) ? hint : nullptr, fr);
      // the two sides: geom1's body enters the row with -, geom2's with +
      int ch[2] = {-1, -1}, nd[2] = {0, 0}, sl = -1, touchbit = -1;
      double binvw = 0, Js[3] = {0, 0, 0}, invm = 0;
      bool obj = false, onfree = false;
      int nblk = 0;
      double Jo[3][6] = {{0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0}}, fl[9], xl[3];   // free object: frame rows and contact point in the body's frame
      if (FR) {
        const double d3[3] = {rec[1] - S.of[OF_P], rec[2] - S.of[OF_P + 1], rec[3] - S.of[OF_P + 2]};
        mulmatT3(xl, S.of + OF_R, d3);
        for (int rr = 0; rr < 3; rr++) mulmatT3(fl + 3 * rr, S.of + OF_R, fr + 3 * rr);
      }
      auto object_side = [&](double sg) {   // a point of the free body (or of one of its leaves): translation n, rotation x x n
        onfree = true;
        for (int rr = 0; rr < 3; rr++) {
          double xn[3];
          cross3(xn, xl, fl + 3 * rr);
          for (int c = 0; c < 3; c++) { Jo[rr][c] += sg * fl[3 * rr + c]; Jo[rr][3 + c] += sg * xn[c]; }
        }
      };
      for (int side = 0; side < 2; side++) {
        const int ref = side ? gp.g2 : gp.g1, kind = sgg_kind(ref), idx = sgg_index(ref);
        const double sg = side ? 1.0 : -1.0;
        if (kind == SGG_BOX) {
          const int tb = T.g_body[idx], c = T.b_chain[tb], n = T.b_nabove[tb], d0 = T.c_dof0[c];
          binvw += T.b_invw[tb];
          touchbit = idx;
          int blk = -1;
          for (int b = 0; b < nblk; b++)
            if (ch[b] == c) blk = b;
          const bool fresh = blk < 0;
          if (fresh) { blk = nblk++; ch[blk] = c; nd[blk] = 0; }
          double* J = blk ? J2 : J1;
          const int nold = nd[blk];
          if (fresh)
            for (int k = 0; k < 3 * CS; k++) J[k] = 0.0;   // the sweep reads whole padded rows
          for (int dl = 0; dl < (n > nold ? n : nold); dl++) {
            double jp[3] = {0, 0, 0};
            if (dl < n) {
              double r[3];
              for (int k = 0; k < 3; k++) r[k] = rec[1 + k] - S.anchor[3 * (d0 + dl) + k];
              cross3(jp, S.axis + 3 * (d0 + dl), r);
            }
            for (int rr = 0; rr < 3; rr++) {
              const double add = sg * dot3(fr + 3 * rr, jp);
              J[rr * CS + dl] = (dl < nold ? J[rr * CS + dl] : 0.0) + add;
            }
          }
          if (n > nold) nd[blk] = n;
        } else if (kind == SGG_ELEM) {
          sl = idx; obj = true;
          binvw += E(SGE_BINVW, idx);
          invm = 1.0 / (E(SGE_MASS, idx) + E(SGE_ARMATURE, idx));
          const double ax[3] = {E(SGE_AX, idx), E(SGE_AY, idx), E(SGE_AZ, idx)};   // (local to the free body when there is one)
          for (int rr = 0; rr < 3; rr++) Js[rr] += sg * dot3((FR ? fl : fr) + 3 * rr, ax);
          if (FR) object_side(sg);
        } else if (kind == SGG_CENTER) {
          obj = true;
          if (FR) { object_side(sg); binvw += H.free_binvw; }
        }
      }
      // J v, J a_smooth, J a_warmstart (the rows' reference accelerations need them); W = J M^-1 and A = J M^-1 J' + R follow in the next two
      // phases.  What this lane knows about the contact travels in its scalar record (the final A, b, f overwrite the temporaries).
      double vel[3], js[3], jw[3];
      for (int rr = 0; rr < 3; rr++) {
        vel[rr] = sl >= 0 ? Js[rr] * S.ve[sl] : 0.0;
        js[rr] = sl >= 0 ? Js[rr] * S.asme[sl] : 0.0;
        jw[rr] = sl >= 0 ? Js[rr] * S.we[sl] : 0.0;
        if (onfree) { vel[rr] += dot6(Jo[rr], S.of + OF_VL); js[rr] += dot6(Jo[rr], S.of + OF_ASM); jw[rr] += dot6(Jo[rr], S.of + OF_WB); }
      }
      for (int b = 0; b < nblk; b++) {
        const int c = ch[b], d0 = T.c_dof0[c], n = nd[b];
        const double* J = b ? J2 : J1;
        for (int rr = 0; rr < 3; rr++)
          for (int dl = 0; dl < n; dl++) {
            vel[rr] += J[rr * CS + dl] * S.v[d0 + dl];
            js[rr] += J[rr * CS + dl] * S.asm_[d0 + dl];
            jw[rr] += J[rr * CS + dl] * S.warm[d0 + dl];
          }
      }
      for (int k = 0; k < 3; k++) { sc[CS_TMP + k] = vel[k]; sc[CS_TMP + 3 + k] = js[k]; sc[CS_TMP + 6 + k] = jw[k]; sc[CS_JS + k] = Js[k]; }
      sc[CS_TMP + 9] = binvw; sc[CS_TMP + 10] = nblk; sc[CS_TMP + 11] = rec[0];
      sc[CS_INVM] = invm; sc[CS_SL] = sl;
      sc[CS_C1] = ch[0]; sc[CS_N1] = nd[0]; sc[CS_C2] = ch[1]; sc[CS_N2] = nd[1];
      sc[CS_TOUCH] = (obj && touchbit >= 0) ? touchbit : -1;
      sc[CS_OBJ] = onfree ? 1.0 : 0.0;
      for (int rr = 0; rr < 3; rr++)
        for (int q = 0; q < 6; q++) sc[CS_JO + 6 * rr + q] = Jo[rr][q];
    }
    SGT_SYNC();
    // (e2) W = J M^-1, one lane per WORD of a W row (r04: contact, chain block, row, dof -- 780 items for 13 contacts; a contact's own lane
    //      used to run the 3 x CS x n products alone, out of an LDS copy of M^-1: with M^-1 in the work space the lanes of a row read
    //      consecutive words of its rows)
    SGT_PAR(i, ncon * 6 * CS) {
      const int ci = i / (6 * CS), rem = i % (6 * CS), b = rem / (3 * CS), rr = (rem / CS) % 3, dl = rem % CS;
      const double* sc = cscal(ci);
      const int c = (int)sc[b ? CS_C2 : CS_C1];
      if (c >= 0) {
        const double* J = crow(ci) + (b ? 6 * CS : 0) + rr * CS;
        const double* Mi = S.Minv + c * CS * CS;
        double s = 0;
#pragma unroll
        for (int e2 = 0; e2 < CS; e2++) s += J[e2] * Mi[e2 * CS + dl];   // (J is zero beyond the body's dofs: the same sum as over them)
        crow(ci)[(b ? 9 * CS : 3 * CS) + rr * CS + dl] = s;
      }
    }
    SGT_SYNC();
    // (e3) A, the reference accelerations, the warmstart force: the contact's lane again
    SGT_PAR(ci, ncon) {
      double* J1 = crow(ci);
      double *W1 = J1 + 3 * CS, *J2 = J1 + 6 * CS, *W2 = J1 + 9 * CS, *sc = cscal(ci);
      int ch[2] = {(int)sc[CS_C1], (int)sc[CS_C2]}, nd[2] = {(int)sc[CS_N1], (int)sc[CS_N2]};
      const int sl = (int)sc[CS_SL], nblk = (int)sc[CS_TMP + 10];
      const bool onfree = sc[CS_OBJ] != 0.0;
      const double invm = sc[CS_INVM], binvw = sc[CS_TMP + 9];
      double Js[3], vel[3], js[3], jw[3], Jo[3][6];
      for (int k = 0; k < 3; k++) { Js[k] = sc[CS_JS + k]; vel[k] = sc[CS_TMP + k]; js[k] = sc[CS_TMP + 3 + k]; jw[k] = sc[CS_TMP + 6 + k]; }
      for (int rr = 0; rr < 3; rr++)
        for (int q = 0; q < 6; q++) Jo[rr][q] = sc[CS_JO + 6 * rr + q];
      const double rec0 = sc[CS_TMP + 11];
      const double* rec = &rec0;
      double Am[6] = {0, 0, 0, 0, 0, 0};
      for (int b = 0; b < nblk; b++) {
        const int n = nd[b];
        const double* J = b ? J2 : J1;
        const double* W = b ? W2 : W1;
        int k = 0;
        for (int rr = 0; rr < 3; rr++)
          for (int s2 = rr; s2 < 3; s2++) {
            double s = 0;
            for (int dl = 0; dl < n; dl++) s += W[rr * CS + dl] * J[s2 * CS + dl];
            Am[k++] += s;
          }
      }
      const double dist = rec[0], imp = impedance(H.con_solimp, dist, H.con_margin);
      const double R = fmax(SG_MINVAL, (1 - imp) / imp * binvw), D = 1 / R;
      if (onfree) {   // the object's share of J M^-1 J' through the arrow matrix: y = M^-1 J_r' = (y_f ; y_e)
        double yf[3][6], ye[3];
        for (int rr = 0; rr < 3; rr++) {
          double t6[6];
          for (int q = 0; q < 6; q++) t6[q] = Jo[rr][q] - (sl >= 0 ? S.Be[6 * sl + q] * Js[rr] * invm : 0.0);
          mat6vec(yf[rr], S.of + OF_SINV, t6);
          ye[rr] = sl >= 0 ? (Js[rr] - dot6(S.Be + 6 * sl, yf[rr])) * invm : 0.0;
        }
        int k = 0;
        for (int rr = 0; rr < 3; rr++)
          for (int s2 = rr; s2 < 3; s2++) { Am[k] += dot6(Jo[s2], yf[rr]) + Js[s2] * ye[rr] + (rr == s2 ? R : 0.0); k++; }
      } else {
        int k = 0;
        for (int rr = 0; rr < 3; rr++)
          for (int s2 = rr; s2 < 3; s2++) { Am[k] += Js[rr] * Js[s2] * invm + (rr == s2 ? R : 0.0); k++; }
      }
      double bb[3], jar[3];
      for (int rr = 0; rr < 3; rr++) {
        const double aref = -H.con_B * vel[rr] - (rr == 0 ? H.con_K * imp * (dist - H.con_margin) : 0.0);
        bb[rr] = js[rr] - aref;
        jar[rr] = jw[rr] - aref;
      }
      double f[3];
      {  // warmstart force: primal -> dual map of the elliptic cone (mj_constraintUpdate)
        const double mu = H.con_mu[0], U0 = jar[0] * mu, U1 = jar[1] * H.con_mu[0], U2 = jar[2] * H.con_mu[1];
        const double Nn = U0, Tt = sqrt(U1 * U1 + U2 * U2);
        if (Nn >= mu * Tt || (Tt <= 0 && Nn >= 0)) { f[0] = f[1] = f[2] = 0; }
        else if (mu * Nn + Tt <= 0 || (Tt <= 0 && Nn < 0)) { for (int rr = 0; rr < 3; rr++) f[rr] = -D * jar[rr]; }
        else {
          const double Dm = D / (mu * mu * (1 + mu * mu)), NmT = Nn - mu * Tt;
          f[0] = -Dm * NmT * mu;
          f[1] = -f[0] / Tt * U1 * H.con_mu[0];
          f[2] = -f[0] / Tt * U2 * H.con_mu[1];
        }
      }
      const bool rows = dist < H.con_margin;   // mj_makeConstraint: a contact at dist >= margin - gap is listed but gets no rows
      for (int k = 0; k < 6; k++) sc[CS_A + k] = Am[k];
      for (int k = 0; k < 3; k++) { sc[CS_B + k] = bb[k]; sc[CS_F0 + k] = rows ? f[k] : 0.0; S.cf[3 * ci + k] = rows ? f[k] : 0.0; }
      sc[CS_R] = R;
      sc[CS_ROWS] = rows ? 1.0 : 0.0;
      {
        const double mu2[2] = {H.con_mu[0], H.con_mu[1]};
        double pe[7];
        contact_block_constants(Am, mu2, pe);
        for (int k = 0; k < 7; k++) sc[CS_PE + k] = pe[k];   // (every temporary of this record has been read above)
      }
      // the contact's stream in the sweep: its one chain; -1 = no rows; -2 = not exactly one chain block (both fingers, or a slider
      // against a static geom): such a list is swept serially
      S.con_chain[ci] = !rows ? -1 : ((nblk == 1 && !onfree) ? ch[0] : -2);   // (a free object couples every contact on it: serial list)
    }
    SGT_ONE { S.icnt[IC_SERIAL] = 0; }
    SGT_SYNC();
    {
      const int ncc = ncon < S.ncache ? ncon : S.ncache;
      SGT_PAR(i, ncc * SGT_CSC) S.csc[i] = cscal(i / SGT_CSC)[i % SGT_CSC];
    }
    // THE CONTACTS' LEVEL SCHEDULE (r05).  Two contacts commute exactly unless they share a dof: the same chain, or the same slider
    // (two fingers on one capsule).  Level(i) = 1 + the highest level of an EARLIER contact that shares a dof with i: contacts of one level are
    // mutually independent, and every pair that does not commute keeps mj_solPGS's order -- the levels in sequence ARE the
    // sequential sweep.  A level holds at most one contact per chain: the sweep runs it on the chains' lane groups side by side.
    // (Until r04 a slider under two fingers sent the WHOLE list to the one-after-the-other fallback: the four-finger scene at
    // the squeeze -- 13 contacts, always a shared capsule somewhere -- ran 13 serial updates per sweep with two barriers each, 55 % of
    // a substep; its levels: 4 - 5.)  Table S.hit_pair[level][chain] = contact id or -1 (the pair walk's hit list is done with); a
    // contact with two chain blocks, without one, or on a free object still makes the list serial, as does a table overflow.
    SGT_PAR(ci, ncon) {
      if (S.con_chain[ci] == -2) S.icnt[IC_SERIAL] = 1;
      S.hit_sorted[ci] = (int)cscal(ci)[CS_SL];      // (staged for the one lane that builds the schedule: a word of LDS instead of a trip to the work space per contact)
    }
    SGT_PAR(i, SGT_MAXHIT) S.hit_pair[i] = -1;
    SGT_PAR(e, N) S.hit_off[e] = 0;                  // last level + 1 of slider e (N <= SGT_MAXHIT: four elements a lane)
    SGT_PAR(c, K) S.hit_sorted[SGT_MAXCON + c] = 0;  // ... of chain c
    SGT_SYNC();
    SGT_ONE {
      int nlev = 0;
      if (S.icnt[IC_SERIAL] == 0) {
        const int cap = SGT_MAXHIT / K;
        for (int ci = 0; ci < ncon; ci++) {
          const int c = S.con_chain[ci];
          if (c < 0) continue;
          const int sl = S.hit_sorted[ci];
          int L = S.hit_sorted[SGT_MAXCON + c];
          if (sl >= 0 && S.hit_off[sl] > L) L = S.hit_off[sl];
          if (L >= cap) { S.icnt[IC_SERIAL] = 1; break; }
          S.hit_pair[L * K + c] = ci;
          S.hit_sorted[SGT_MAXCON + c] = L + 1;
          if (sl >= 0) S.hit_off[sl] = L + 1;
          nlev = nlev > L + 1 ? nlev : L + 1;
        }
      }
      S.icnt[IC_NLEV] = nlev;
    }
    SGT_SYNC();
    const bool serial_contacts = S.icnt[IC_SERIAL] != 0;
#if SGT_DEVICE
    // the serial list's wave-synchronous pass reads a contact's chains from LDS (S.hit_cnt: the narrowphase counts are done with)
    if (serial_contacts) {
      SGT_PAR(ci, ncon) S.hit_cnt[ci] = (((int)cscal(ci)[CS_C1] + 1) & 0xff) | ((((int)cscal(ci)[CS_C2] + 1) & 0xff) << 8);
      SGT_SYNC();
    }
#endif
    const double con_mu[2] = {H.con_mu[0], H.con_mu[1]};
    SGT_STAMP(10);
    // row count (nefc) and the touch bits of this contact list
    {
      int nl = 0;
      for (int c = 0; c < K; c++) nl += S.icnt[IC_NLIM0 + c];
      double cnt = 0;
      SGT_PAR(e, N) cnt += (S.Rlim[2 * e] != 0.0 ? 1.0 : 0.0) + (S.Rlim[2 * e + 1] != 0.0 ? 1.0 : 0.0);
      SGT_PAR(ci, ncon) cnt += cscal(ci)[CS_ROWS] != 0.0 ? 3.0 : 0.0;
      nefc = N + 1 + nl + H.nnb + (int)wsum(cnt);
      touch_lo = touch_hi = 0;
      for (int ci = 0; ci < ncon; ci++) {   // uniform loop: every lane ends up with the same words
        const int tbit = (int)cscal(ci)[CS_TOUCH];
        if (tbit >= 0 && tbit < 32) touch_lo |= 1u << tbit;
        else if (tbit >= 32 && tbit < 64) touch_hi |= 1u << (tbit - 32);
      }
    }

    // ---------------------------------------------------------------- stage 10: warmstart (kept only if it beats f = 0), PGS
    // a = M^-1 J' f of the current forces: chains in aF, sliders in ae
    auto apply_all = [&]() {
      SGT_PAR(e, N) {
        double g = S.ffix[e] + S.ecoef[e] * ten_f + S.flim[2 * e] - S.flim[2 * e + 1];
        if (NB)
          for (int d = 0; d < 3; d++) {   // its own rows push it with +f, the rows that have it as partner (nbtab's in_slot) with -f
            if (nbtab[d * N + e] >= 0) g += S.nbf[d * N + e];
            const int in = nbtab[6 * N + d * N + e];
            if (in >= 0) g -= S.nbf[in];
          }
        S.ae[e] = S.einvm[e] * g;
      }
      SGT_PAR(idx, K * CS) {
        const int c = idx / CS, dl = idx % CS;
        const double* rows = S.lrow + SGT_LROW * 2 * T.c_dof0[c];
        double s = 0;
        // (r05s: eight rows' words of M^-1 -- work space, behind the row's dof index from LDS -- requested together, then added in the rows'
        //  order: row by row the loop paid a trip to the work space per row, 14 in a row for a finger of the four-finger gripper)
        const int nl = S.icnt[IC_NLIM0 + c];
        for (int i0 = 0; i0 < nl; i0 += 8) {
          double mw[8];
          for (int k = 0; k < 8; k++) {
            const int ii = i0 + k < nl ? i0 + k : 0;   // (past the list: row 0's word, read and not used -- the dof index must be a valid one)
            mw[k] = S.Minv[c * CS * CS + (int)rows[SGT_LROW * ii] * CS + dl];
          }
          for (int k = 0; k < 8; k++) {
            const int i = i0 + k;
            if (i < nl) s += mw[k] * rows[SGT_LROW * i + 1] * rows[SGT_LROW * i + 4];
          }
        }
        S.aF[idx] = s;
      }
      SGT_SYNC();
      // The contacts add their pushes in the list's order (a slider or a chain may carry several).  Every chain word has its lane, which walks
      // the list and adds what is its own -- the same sums in the same order as contact after contact between barriers (two per contact
      // until r05: 4 % of a free-ball substep), without a barrier; the sliders' and the object's words go through one lane meanwhile.
#if SGT_DEVICE && !defined(SGT_X_WSSERIAL)
      // (r05s) a list of at most 64 contacts: a contact's chains come from the lane that holds
      // its record (scalar reads: no trip to the work space per contact and lane), and the next contact's W words are requested while the
      // current one's are added -- the same sums in the same order
      if (ncon <= 64) {
        const int lane = (int)threadIdx.x, cl = lane < ncon ? lane : 0;
        const double* scl = cscr(cl);
        const bool rows_l = lane < ncon && scl[CS_ROWS] != 0.0;
        const int c1_l = rows_l ? (int)scl[CS_C1] : -1, c2_l = rows_l ? (int)scl[CS_C2] : -1;
        for (int w0 = 0; w0 < K * CS; w0 += 64) {   // (the four-finger gripper's 80 chain words: two passes)
        const int wi = w0 + lane;
        const bool word = wi < K * CS;
        const int c = word ? wi / CS : -2, dl = word ? wi % CS : 0;   // (-2: a lane without a word matches no chain)
        double a = word ? S.aF[wi] : 0.0;
        struct WR { double w0, w1, w2, w3, w4, w5; bool m1, m2; };
        auto ldw = [&](WR& q, const int ci) {   // ci uniform
          q.m1 = __builtin_amdgcn_readlane(c1_l, ci) == c; q.m2 = __builtin_amdgcn_readlane(c2_l, ci) == c;
          const double* W1 = crow(ci) + 3 * CS + dl;
          const double* W2 = crow(ci) + 9 * CS + dl;
          q.w0 = q.w1 = q.w2 = q.w3 = q.w4 = q.w5 = 0.0;
          if (q.m1) { q.w0 = W1[0]; q.w1 = W1[CS]; q.w2 = W1[2 * CS]; }
          if (q.m2) { q.w3 = W2[0]; q.w4 = W2[CS]; q.w5 = W2[2 * CS]; }
        };
        auto acc = [&](const WR& q, const int ci) {
          const double* f = S.cf + 3 * ci;
          if (q.m1) a += q.w0 * f[0] + q.w1 * f[1] + q.w2 * f[2];
          if (q.m2) a += q.w3 * f[0] + q.w4 * f[1] + q.w5 * f[2];
        };
        if (ncon > 0) {
          WR qa, qb;
          ldw(qa, 0);
          for (int ci = 0; ci < ncon; ci += 2) {
            ldw(qb, ci + 1 < ncon ? ci + 1 : 0);
            acc(qa, ci);
            ldw(qa, ci + 2 < ncon ? ci + 2 : 0);
            if (ci + 1 < ncon) acc(qb, ci + 1);
          }
        }
        if (word) S.aF[wi] = a;
        }
      } else
#endif
      SGT_PAR(idx, K * CS) {
        const int c = idx / CS, dl = idx % CS;
        double a = S.aF[idx];
        for (int ci = 0; ci < ncon; ci++) {
          const double* sc = cscr(ci);
          if (sc[CS_ROWS] == 0.0) continue;
          const int c1 = (int)sc[CS_C1], c2 = (int)sc[CS_C2];
          if (c1 != c && c2 != c) continue;
          const double* f = S.cf + 3 * ci;
          const double* W1 = crow(ci) + 3 * CS;
          const double* W2 = crow(ci) + 9 * CS;
          if (c1 == c) a += W1[dl] * f[0] + W1[CS + dl] * f[1] + W1[2 * CS + dl] * f[2];
          if (c2 == c) a += W2[dl] * f[0] + W2[CS + dl] * f[1] + W2[2 * CS + dl] * f[2];
        }
        S.aF[idx] = a;
      }
#if SGT_DEVICE && !defined(SGT_X_WSSERIAL)
      // (r05s) the sliders' and the free body's words: every contact's TERMS on a lane of their own (its record's loads side by side with the
      // other contacts'), then the sums in the list's order by scalar reads of the lanes -- the same terms added in the same order as the
      // one-lane walk below, which paid a record's round trip to the work space per contact: ~1.5 us each, 3 % of a free-ball substep
      if (ncon <= 64) {
        const int lane = (int)threadIdx.x, cl = lane < ncon ? lane : 0;
        const double* sc = cscr(cl);
        const bool rows = lane < ncon && sc[CS_ROWS] != 0.0;
        const double* f = S.cf + 3 * cl;
        const double f0 = f[0], f1 = f[1], f2 = f[2];
        const int sl = rows ? (int)sc[CS_SL] : -1;
        const double ts = sl >= 0 ? sc[CS_INVM] * (sc[CS_JS] * f0 + sc[CS_JS + 1] * f1 + sc[CS_JS + 2] * f2) : 0.0;
        const int ob = (FR && rows && sc[CS_OBJ] != 0.0) ? 1 : 0;
        double tq[6] = {0, 0, 0, 0, 0, 0};
        if (FR && ob)
          for (int q = 0; q < 6; q++) tq[q] = sc[CS_JO + q] * f0 + sc[CS_JO + 6 + q] * f1 + sc[CS_JO + 12 + q] * f2;
        double gf[6] = {0, 0, 0, 0, 0, 0};
        if (FR)
          for (int q = 0; q < 6; q++) gf[q] = S.of[OF_GF + q];
        for (int c = 0; c < ncon; c++) {   // (uniform)
          const int slc = __builtin_amdgcn_readlane(sl, c);
          if (slc >= 0) {
            const double t = readlane64(ts, c);
            SGT_ONE { S.ae[slc] += t; }
          }
          if (FR && __builtin_amdgcn_readlane(ob, c))
            for (int q = 0; q < 6; q++) gf[q] += readlane64(tq[q], c);
        }
        if (FR) SGT_ONE { for (int q = 0; q < 6; q++) S.of[OF_GF + q] = gf[q]; }
      } else
#endif
      SGT_ONE {
        for (int ci = 0; ci < ncon; ci++) {
          const double* sc = cscr(ci);
          if (sc[CS_ROWS] == 0.0) continue;
          const double* f = S.cf + 3 * ci;
          const int sl = (int)sc[CS_SL];
          if (sl >= 0) S.ae[sl] += sc[CS_INVM] * (sc[CS_JS] * f[0] + sc[CS_JS + 1] * f[1] + sc[CS_JS + 2] * f[2]);
          if (FR && sc[CS_OBJ] != 0.0)
            for (int q = 0; q < 6; q++) S.of[OF_GF + q] += sc[CS_JO + q] * f[0] + sc[CS_JO + 6 + q] * f[1] + sc[CS_JO + 12 + q] * f[2];
        }
      }
      SGT_SYNC();
      if (FR) {   // S.ae holds the sliders' LOCAL part g_e / D_e; the body: a_f = S^-1 (g_f - sum_e B_e g_e / D_e)
        double red[6] = {0, 0, 0, 0, 0, 0}, rhs[6], af6[6];
        SGT_PAR(e, N)
          for (int q = 0; q < 6; q++) red[q] += S.Be[6 * e + q] * S.ae[e];
        for (int q = 0; q < 6; q++) rhs[q] = S.of[OF_GF + q] - wsum(red[q]);
        mat6vec(af6, S.of + OF_SINV, rhs);
        SGT_SYNC();
        SGT_ONE { for (int q = 0; q < 6; q++) S.of[OF_AF + q] = af6[q]; }
        SGT_SYNC();
      }
    };
    if (FR) { SGT_ONE { for (int q = 0; q < 6; q++) S.of[OF_GF + q] = 0; } }
    apply_all();
    {
      double cost = 0, S_ae = 0;
      SGT_PAR(e, N) {
        const double ae_ = slider_acc(e);
        S_ae += S.ecoef[e] * ae_;
        cost += S.ffix[e] * (0.5 * (ae_ + S.Rfix[e] * S.ffix[e]) + S.bfix[e]);
        cost += S.flim[2 * e] * (0.5 * (ae_ + S.Rlim[2 * e] * S.flim[2 * e]) + S.blim[2 * e]);
        cost += S.flim[2 * e + 1] * (0.5 * (-ae_ + S.Rlim[2 * e + 1] * S.flim[2 * e + 1]) + S.blim[2 * e + 1]);
      }
      if (NB) SGT_PAR(k, 3 * N) {
        const int pe = nbtab[k];
        if (pe >= 0) cost += S.nbf[k] * (0.5 * ((slider_acc(k % N) - slider_acc(pe)) + S.nbR[k] * S.nbf[k]) + S.nbb[k]);
      }
      SGT_PAR(c, K) {
        const double* rows = S.lrow + SGT_LROW * 2 * T.c_dof0[c];
        for (int i = 0; i < S.icnt[IC_NLIM0 + c]; i++) {
          const double* r = rows + SGT_LROW * i;
          cost += r[4] * (0.5 * (r[1] * S.aF[c * CS + (int)r[0]] + r[2] * r[4]) + r[3]);
        }
      }
      SGT_PAR(ci, ncon) {
        const double* sc = cscr(ci);
        if (sc[CS_ROWS] == 0.0) continue;
        const double* f = S.cf + 3 * ci;
        const int sl = (int)sc[CS_SL];
        for (int rr = 0; rr < 3; rr++) {
          double ja = sl >= 0 ? sc[CS_JS + rr] * slider_acc(sl) : 0.0;
          if (FR && sc[CS_OBJ] != 0.0) ja += dot6(sc + CS_JO + 6 * rr, S.of + OF_AF);
          for (int b = 0; b < 2; b++) {
            const int c = (int)sc[b ? CS_C2 : CS_C1], n = (int)sc[b ? CS_N2 : CS_N1];
            if (c < 0) continue;
            const double* J = crow(ci) + (b ? 6 * CS : 0) + rr * CS;
            for (int dl = 0; dl < n; dl++) ja += J[dl] * S.aF[c * CS + dl];
          }
          cost += f[rr] * (0.5 * (ja + sc[CS_R] * f[rr]) + sc[CS_B + rr]);
        }
      }
      S_ae = wsum(S_ae);
      cost = wsum(cost) + ten_f * (0.5 * (S_ae + ten_R * ten_f) + ten_b);
      if (cost > 0) {   // uniform
        ten_f = 0;
        SGT_PAR(e, N) { S.ffix[e] = 0; S.flim[2 * e] = 0; S.flim[2 * e + 1] = 0; S.ae[e] = 0; }
        if (NB) SGT_PAR(k, 3 * N) S.nbf[k] = 0;
        SGT_PAR(i, K * CS) S.aF[i] = 0;
        if (FR) SGT_ONE { for (int q = 0; q < 6; q++) S.of[OF_AF + q] = S.of[OF_GF + q] = 0; }
        SGT_PAR(c, K)
          for (int i = 0; i < S.icnt[IC_NLIM0 + c]; i++) S.lrow[SGT_LROW * (2 * T.c_dof0[c] + i) + 4] = 0;
        SGT_PAR(i, 3 * ncon) S.cf[i] = 0;
      }
      SGT_SYNC();
    }
    iters = 0;
    SGT_STAMP(11);
    // the PGS sweeps run in a function of their own (tree_sweep, above tree_env): its register allocation is not the monolith's --
    // the step's ~40 stages in one function left the sweep's loops 249 spilled registers and 2.3 KB of scratch memory per lane
    SGT_ONE {
      double* w = S.swc;
      w[SWC_TEN_R] = ten_R; w[SWC_TEN_B] = ten_b; w[SWC_TEN_F] = ten_f; w[SWC_TJ_A] = tj_A; w[SWC_TEN_I] = ten_I;
      for (int q = 0; q < 6; q++) w[SWC_CTEN + q] = cten[q];
      w[SWC_NCON] = ncon; w[SWC_SERIAL] = serial_contacts ? 1.0 : 0.0;
    }
    SGT_SYNC();
    {   // (uniform branches: one instantiation of the sweep per scene class)
      const SGT_CONST SgPlanHeader* const hp = (const SGT_CONST SgPlanHeader*)A.H;
      const SGT_CONST SgTreeDev* const tp = (const SGT_CONST SgTreeDev*)A.T;
      const SGT_CONST int* const nbc = (const SGT_CONST int*)A.nbtab;
      const SGT_CONST SgEqSlot* const sc = (const SGT_CONST SgEqSlot*)A.sched;
      SGT_GLOBP double* const cwp = (SGT_GLOBP double*)(A.cws + (size_t)env * A.cws_stride);
      SGT_LDSP double* const lp = (SGT_LDSP double*)lds_base;
      if (FR && NB) tree_sweep<CHD, true, true>(hp, tp, nbc, sc, A.nbtab, cwp, lp, A.secprof);
      else if (FR) tree_sweep<CHD, true, false>(hp, tp, nbc, sc, A.nbtab, cwp, lp, A.secprof);
      else if (NB) tree_sweep<CHD, false, true>(hp, tp, nbc, sc, A.nbtab, cwp, lp, A.secprof);
      else tree_sweep<CHD, false, false>(hp, tp, nbc, sc, A.nbtab, cwp, lp, A.secprof);
    }
    SGT_SYNC();
    SGT_STAMP_RESET();
    iters = (int)S.swc[SWC_ITERS];

    SGT_STAMP(14);
  }
#define SGT_FRAME SGT_FRAME_STAGE_TAIL
#include "sg_tree_frame.inc"
}

}  // namespace sgt
