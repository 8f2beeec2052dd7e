// sg_tree_stage_dynamics.h -- the first stage of a substep: checks, kinematics, tendons, mass matrix, L'DL + M^-1, bias and smooth accelerations (part of sg_tree.h)
#pragma once

namespace sgt {

template <int CHD>
static SGT_STAGE_ATTR void tree_stage_dynamics(SGT_STAGE_PARAMS) {
#define SGT_FRAME SGT_FRAME_STAGE_HEAD
#include "sg_tree_frame.inc"
  {
    // ---------------------------------------------------------------- mj_checkPos / mj_checkVel
    {
      double bad = 0;
      SGT_PAR(d, ND) bad += (isbad(S.q[d]) ? 1.0 : 0.0) + (isbad(S.v[d]) ? 1024.0 : 0.0);
      SGT_PAR(e, N) bad += (isbad(S.qe[e]) ? 1.0 : 0.0) + (isbad(S.ve[e]) ? 1024.0 : 0.0);
      if (FR) SGT_PAR(c, 7) bad += (isbad(S.of[OF_P + c]) ? 1.0 : 0.0) + ((c < 3 && (isbad(S.of[OF_VW + c]) || isbad(S.of[OF_WL + c]))) ? 1024.0 : 0.0);
      bad = wsum(bad);
      if (bad > 0) {
        const int nb = (int)bad;
        if (nb % 1024) flags |= SG_FLAG_BADQPOS;
        if (nb / 1024) flags |= SG_FLAG_BADQVEL;
        { stop = 1; goto stage_done; }   // uniform: the env stops integrating for the rest of the call
      }
    }
    SGT_STAMP(0);
    // ---------------------------------------------------------------- stage 1: kinematics, one lane per chain
    SGT_PAR(c, K) {
      double pos[3], quat[4], mat[9], ppos[3], pquat[4], pmat[9], t[3];
      for (int k = 0; k < 3; k++) ppos[k] = T.c_root_pos[c][k];
      for (int k = 0; k < 4; k++) pquat[k] = T.c_root_quat[c][k];
      quat2mat(pmat, pquat);
      for (int bi = 0; bi < T.c_nbody[c]; bi++) {
        const int tb = T.c_body0[c] + bi;
        mulmat3(t, pmat, T.b_pos[tb]);
        for (int k = 0; k < 3; k++) pos[k] = ppos[k] + t[k];
        quatmul(quat, pquat, T.b_quat[tb]);
        for (int kj = 0; kj < T.b_njnt[tb]; kj++) {
          const int d = T.b_dof0[tb] + kj;
          quat2mat(mat, quat);
          mulmat3(t, mat, T.d_pos[d]);
          for (int k = 0; k < 3; k++) S.anchor[3 * d + k] = pos[k] + t[k];
          mulmat3(S.axis + 3 * d, mat, T.d_axis[d]);
          const double dq = S.q[d] - T.d_qpos0[d], sn = sin(0.5 * dq);
          const double ql[4] = {cos(0.5 * dq), T.d_axis[d][0] * sn, T.d_axis[d][1] * sn, T.d_axis[d][2] * sn};
          quatmul(quat, quat, ql);
          quat2mat(mat, quat);
          mulmat3(t, mat, T.d_pos[d]);
          for (int k = 0; k < 3; k++) pos[k] = S.anchor[3 * d + k] - t[k];
        }
        const double nq = sqrt(quat[0] * quat[0] + quat[1] * quat[1] + quat[2] * quat[2] + quat[3] * quat[3]);
        for (int k = 0; k < 4; k++) quat[k] /= nq;
        quat2mat(mat, quat);
        for (int k = 0; k < 3; k++) S.xpos[3 * tb + k] = pos[k];
        for (int k = 0; k < 9; k++) S.xmat[9 * tb + k] = mat[k];
        mulmat3(t, mat, T.b_ipos[tb]);
        for (int k = 0; k < 3; k++) S.xipos[3 * tb + k] = pos[k] + t[k];
        double RI[9], Rt[9];
        mulmat33(RI, mat, T.b_imat[tb]);
        for (int a = 0; a < 3; a++)
          for (int b = 0; b < 3; b++) Rt[3 * a + b] = mat[3 * b + a];
        mulmat33(S.ximat + 9 * tb, RI, Rt);
        for (int k = 0; k < 3; k++) ppos[k] = pos[k];
        for (int k = 0; k < 4; k++) pquat[k] = quat[k];
        for (int k = 0; k < 9; k++) pmat[k] = mat[k];
      }
    }
    if (FR) SGT_ONE {   // the free body's pose IS its 7 positions; velocities, gravity and the warmstart in its frame
      double* o = S.of;
      const double nq = sqrt(o[OF_Q] * o[OF_Q] + o[OF_Q + 1] * o[OF_Q + 1] + o[OF_Q + 2] * o[OF_Q + 2] + o[OF_Q + 3] * o[OF_Q + 3]);
      double qn[4] = {o[OF_Q] / nq, o[OF_Q + 1] / nq, o[OF_Q + 2] / nq, o[OF_Q + 3] / nq};
      quat2mat(o + OF_R, qn);
      mulmatT3(o + OF_VL, o + OF_R, o + OF_VW);
      mulmatT3(o + OF_GL, o + OF_R, H.gravity);
      mulmatT3(o + OF_WB, o + OF_R, o + OF_WARM);
      for (int c = 0; c < 3; c++) o[OF_WB + 3 + c] = o[OF_WARM + 3 + c];
      double t[3];
      mulmat3(t, o + OF_R, H.center_pos);
      for (int c = 0; c < 3; c++) o[OF_CEN + c] = o[OF_P + c] + t[c];
    }
    SGT_SYNC();
    SGT_PAR(g, T.NG) {
      const int tb = T.g_body[g];
      double t[3];
      mulmat3(t, S.xmat + 9 * tb, T.g_pos[g]);
      for (int k = 0; k < 3; k++) S.gpos[3 * g + k] = S.xpos[3 * tb + k] + t[k];
      mulmat33(S.gmat + 9 * g, S.xmat + 9 * tb, T.g_mat[g]);
    }
    SGT_PAR(s, T.NS) {
      const int tb = T.s_body[s];
      double t[3];
      mulmat3(t, S.xmat + 9 * tb, T.s_pos[s]);
      for (int k = 0; k < 3; k++) S.spos[3 * s + k] = S.xpos[3 * tb + k] + t[k];
    }
    SGT_SYNC();
    SGT_STAMP(1);
    // ---------------------------------------------------------------- stage 3: tendons.  segments, then one lane per dof
    SGT_PAR(i, K * SGT_MAXTS) {
      const int c = i / SGT_MAXTS, w = i % SGT_MAXTS;
      if (T.t_has[c] && w + 1 < T.t_nsite[c]) {
        const int s0 = T.t_site[c][w], s1 = T.t_site[c][w + 1];
        const double* p0 = s0 >= 0 ? S.spos + 3 * s0 : T.t_fixed[c][w];
        const double* p1 = s1 >= 0 ? S.spos + 3 * s1 : T.t_fixed[c][w + 1];
        double dif[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};
        const double len = sqrt(dot3(dif, dif));
        double* sg = S.seg + 4 * i;
        sg[3] = len;
        for (int k = 0; k < 3; k++) sg[k] = len < SG_MINVAL ? 0.0 : dif[k] / len;
      }
    }
    SGT_SYNC();
    SGT_PAR(d, ND) {
      const int c = T.d_chain[d], dl = d - T.c_dof0[c];
      double J = 0;
      if (T.t_has[c])
        for (int w = 0; w + 1 < T.t_nsite[c]; w++) {
          const double* sg = S.seg + 4 * (c * SGT_MAXTS + w);
          if (sg[3] < SG_MINVAL) continue;
          const int s0 = T.t_site[c][w], s1 = T.t_site[c][w + 1];
          double r[3], jp[3];
          if (s1 >= 0 && T.b_nabove[T.s_body[s1]] > dl) {
            for (int k = 0; k < 3; k++) r[k] = S.spos[3 * s1 + k] - S.anchor[3 * d + k];
            cross3(jp, S.axis + 3 * d, r);
            J += dot3(sg, jp);
          }
          if (s0 >= 0 && T.b_nabove[T.s_body[s0]] > dl) {
            for (int k = 0; k < 3; k++) r[k] = S.spos[3 * s0 + k] - S.anchor[3 * d + k];
            cross3(jp, S.axis + 3 * d, r);
            J -= dot3(sg, jp);
          }
        }
      S.tenJ[d] = J;
    }
    SGT_SYNC();
    // tendon length / velocity, spring-damper and actuator force (stages 3, 7, 8), one lane per chain
    SGT_PAR(c, K) {
      double* cs = S.chs + c * CHS_N;
      double Lt = 0, vel = 0;
      if (T.t_has[c]) {
        for (int w = 0; w + 1 < T.t_nsite[c]; w++) Lt += S.seg[4 * (c * SGT_MAXTS + w) + 3];
        for (int dl = 0; dl < T.c_ndof[c]; dl++) vel += S.tenJ[T.c_dof0[c] + dl] * S.v[T.c_dof0[c] + dl];
      }
      cs[CHS_TLEN] = Lt; cs[CHS_TVEL] = vel;
      cs[CHS_TFRC] = T.t_has[c] ? -cs[CHS_KT] * (Lt - T.t_lspring[c]) - T.t_damping[c] * vel : 0.0;
      double afrc = 0, adot = 0;
      if (T.a_has[c]) {
        const double g = T.a_gear[c];
        adot = (cs[CHS_CTRL] - cs[CHS_ACT]) / fmax(SG_MINVAL, T.a_tc[c]);
        afrc = T.a_gain[c] * cs[CHS_ACT] + T.a_bias[c][0] + T.a_bias[c][1] * (g * Lt) + T.a_bias[c][2] * (g * vel);
        afrc *= g;   // qfrc_actuator = gear * J * force
      }
      cs[CHS_AFRC] = afrc; cs[CHS_ACTDOT] = adot;
    }
    SGT_STAMP(2);
    // ---------------------------------------------------------------- stage 4: mass matrix, one lane per entry of the lower triangles
    // (the identity padding of the blocks never changes: written by the first forward pass of a call)
    if (sub == 0) SGT_PAR(i, T.NMAT) {
      const int c = i / (CS * CS), a = (i % (CS * CS)) / CS, b = i % CS, nd = T.c_ndof[c];
      if (a >= nd || b >= nd) Mg[i] = a == b ? 1.0 : 0.0;
    }
    // one lane per entry of the LOWER TRIANGLES only (r04: 840 items for the four-finger gripper's four 20 x 20 blocks instead of 1 600,
    // of which the upper ones idled through the trips of their wavefront): item = (chain, triangular index)
    const int TRI = CS * (CS + 1) / 2;
    SGT_PAR(i, K * TRI) {
      const int c = i / TRI, tt = i % TRI, nd = T.c_ndof[c];
      int a = (int)((sqrt(8.0 * tt + 1.0) - 1.0) * 0.5);
      while (a * (a + 1) / 2 > tt) a--;
      while ((a + 1) * (a + 2) / 2 <= tt) a++;
      const int b = tt - a * (a + 1) / 2;
      if (a < nd) {
        const int da = T.c_dof0[c] + a, db = T.c_dof0[c] + b;
        double s = a == b ? T.d_armature[da] : 0.0;
        for (int tb = T.d_body[da]; tb < T.c_body0[c] + T.c_nbody[c]; tb++) {
          const double mass = T.b_mass[tb];
          if (mass <= 0) continue;
          double ra[3], rb[3], ja[3], jb[3], Ir[3];
          for (int k = 0; k < 3; k++) { ra[k] = S.xipos[3 * tb + k] - S.anchor[3 * da + k]; rb[k] = S.xipos[3 * tb + k] - S.anchor[3 * db + k]; }
          cross3(ja, S.axis + 3 * da, ra);
          cross3(jb, S.axis + 3 * db, rb);
          mulmat3(Ir, S.ximat + 9 * tb, S.axis + 3 * da);
          s += mass * dot3(ja, jb) + dot3(Ir, S.axis + 3 * db);
        }
        Mg[c * CS * CS + a * CS + b] = s;
        Mg[c * CS * CS + b * CS + a] = s;
      }
    }
    SGT_SYNC();
    SGT_STAMP(3);
    SGT_PAR(i, T.NMAT) S.L[i] = Mg[i];
    SGT_SYNC();
    factor_all();
    SGT_PAR(idx, K * CS) {   // M^-1 by columns (= rows): solve for the unit vectors (the padding rows come out as unit vectors too)
      const int c = idx / CS, dl = idx % CS;
      double* x = S.Minv + c * CS * CS + dl * CS;
      for (int k = 0; k < CS; k++) x[k] = k == dl ? 1.0 : 0.0;
      chain_solve_reg<CHD>(S.L + c * CS * CS, CS, x);
    }
    SGT_STAMP(4);
    // ---------------------------------------------------------------- stage 7: bias forces (RNE with qacc = 0), body velocities
    tree_motion(nullptr);
    SGT_SYNC();
    SGT_PAR(tb, NB) {
      const double *w = S.bw + 3 * tb, *al = S.bal + 3 * tb;
      double c[3], t[3], t2[3], f[3], n[3], Iw[3];
      for (int k = 0; k < 3; k++) { c[k] = S.xipos[3 * tb + k] - S.xpos[3 * tb + k]; f[k] = S.ba[3 * tb + k]; }
      cross3(t, al, c); addscl3(f, t, 1);
      cross3(t, w, c); cross3(t2, w, t); addscl3(f, t2, 1);
      for (int k = 0; k < 3; k++) f[k] *= T.b_mass[tb];
      mulmat3(n, S.ximat + 9 * tb, al);
      mulmat3(Iw, S.ximat + 9 * tb, w);
      cross3(t, w, Iw); addscl3(n, t, 1);
      for (int k = 0; k < 3; k++) { S.bf[3 * tb + k] = f[k]; S.bn[3 * tb + k] = n[k]; }
    }
    SGT_SYNC();
    SGT_PAR(d, ND) {
      const int c = T.d_chain[d];
      double s = 0;
      for (int tb = T.d_body[d]; tb < T.c_body0[c] + T.c_nbody[c]; tb++) {
        if (T.b_mass[tb] <= 0) continue;
        double r[3], jp[3];
        for (int k = 0; k < 3; k++) r[k] = S.xipos[3 * tb + k] - S.anchor[3 * d + k];
        cross3(jp, S.axis + 3 * d, r);
        s += dot3(jp, S.bf + 3 * tb) + dot3(S.axis + 3 * d, S.bn + 3 * tb);
      }
      S.bias[d] = s;
      // passive (joint spring / damper, tendon spring / damper) - bias + actuator
      const double* cs = S.chs + c * CHS_N;
      const double pas = -S.kd[d] * (S.q[d] - T.d_springref[d]) - T.d_damping[d] * S.v[d] + S.tenJ[d] * cs[CHS_TFRC];
      S.fs[d] = pas - s + S.tenJ[d] * cs[CHS_AFRC];
    }
    SGT_PAR(i, K * CS) S.tmpP[i] = 0;
    SGT_SYNC();
    SGT_PAR(d, ND) S.tmpP[pidx(d)] = S.fs[d];
    SGT_SYNC();
    SGT_PAR(c, K) chain_solve_reg<CHD>(S.L + c * CS * CS, CS, S.tmpP + c * CS);
    SGT_SYNC();
    SGT_PAR(d, ND) S.asm_[d] = S.tmpP[pidx(d)];
    SGT_STAMP(5);
    // ---------------------------------------------------------------- the composite's sliders: smooth forces (stages 7 - 9)
    double t0_len = 0, t0_vel = 0;
    SGT_PAR(e, N) { t0_len += E(SGE_COEF, e) * S.qe[e]; t0_vel += E(SGE_COEF, e) * S.ve[e]; }
    t0_len = wsum(t0_len); t0_vel = wsum(t0_vel);
    const double t0_frc = -kt0 * (t0_len - H.t0_lspring) - H.t0_damping * t0_vel;
    if (FR) {
      // ---- the free object, everything in the body's frame.  Dofs: (v, w) of the body -- v turned into its frame --
      // and the sliders.  Mass matrix [[M_ff, B], [B', D]]: M_ff from the total mass, first moment and inertia about the body's
      // origin (they move with the sliders: three reductions), B_e constant, D diagonal.  Bias: RNE over a star -- the body
      // and its leaves (oracle tree_motion / rne_bias): a leaf's centre of mass accelerates with -g + 2 (w x a_e) s'_e + w x (w x k_e).
      const double* o = S.of;
      const double w[3] = {o[OF_WL], o[OF_WL + 1], o[OF_WL + 2]}, gl[3] = {o[OF_GL], o[OF_GL + 1], o[OF_GL + 2]};
      double acc[15];   // force (3), torque about the origin (3), first moment (3), inertia about the origin (6: 00 01 02 11 12 22)
      for (int k = 0; k < 15; k++) acc[k] = 0;
      SGT_PAR(e, N) {
        const double m = E(SGE_MASS, e), sd = S.qe[e] - E(SGE_QPOS0, e), a[3] = {E(SGE_AX, e), E(SGE_AY, e), E(SGE_AZ, e)};
        const double k[3] = {E(SGE_KX, e) + a[0] * sd, E(SGE_KY, e) + a[1] * sd, E(SGE_KZ, e) + a[2] * sd};
        const double Ie[9] = {E(SGE_I00, e), E(SGE_I01, e), E(SGE_I02, e), E(SGE_I01, e), E(SGE_I11, e), E(SGE_I12, e), E(SGE_I02, e), E(SGE_I12, e), E(SGE_I22, e)};
        double t[3], t2[3], f[3], n[3], Iw[3], kxf[3];
        cross3(t, w, a);
        cross3(t2, w, k); cross3(f, w, t2);
        for (int c = 0; c < 3; c++) f[c] = m * (f[c] - gl[c] + 2 * t[c] * S.ve[e]);
        mulmat3(Iw, Ie, w);
        cross3(n, w, Iw);
        cross3(kxf, k, f);
        const double pas = -S.ke[e] * (S.qe[e] - E(SGE_SPRINGREF, e)) - E(SGE_DAMPING, e) * S.ve[e] + E(SGE_COEF, e) * t0_frc;
        S.fse[e] = pas - dot3(a, f);
        const double kk = dot3(k, k);
        for (int c = 0; c < 3; c++) { acc[c] += f[c]; acc[3 + c] += kxf[c] + n[c]; acc[6 + c] += m * k[c]; }
        acc[9] += Ie[0] + m * (kk - k[0] * k[0]); acc[10] += Ie[1] - m * k[0] * k[1]; acc[11] += Ie[2] - m * k[0] * k[2];
        acc[12] += Ie[4] + m * (kk - k[1] * k[1]); acc[13] += Ie[5] - m * k[1] * k[2]; acc[14] += Ie[8] + m * (kk - k[2] * k[2]);
        double cl[3] = {E(SGE_GX, e) + a[0] * sd, E(SGE_GY, e) + a[1] * sd, E(SGE_GZ, e) + a[2] * sd}, cw[3];   // the capsule's centre, world
        mulmat3(cw, o + OF_R, cl);
        for (int c = 0; c < 3; c++) S.ecen[3 * e + c] = o[OF_P + c] + cw[c];
      }
      for (int k = 0; k < 15; k++) acc[k] = wsum(acc[k]);
      SGT_SYNC();
      SGT_ONE {
        double* ow = S.of;
        const double mF = H.free_mass, *c = H.free_com;
        double t2[3], f[3], n[3], Iw[3], cxf[3];
        cross3(t2, w, c); cross3(f, w, t2);
        for (int q = 0; q < 3; q++) f[q] = mF * (f[q] - gl[q]);
        mulmat3(Iw, H.free_inertia, w);
        cross3(n, w, Iw);
        cross3(cxf, c, f);
        const double cc = dot3(c, c);
        double F6[6], mk[3], I6[6];
        for (int q = 0; q < 3; q++) { F6[q] = acc[q] + f[q]; F6[3 + q] = acc[3 + q] + cxf[q] + n[q]; mk[q] = acc[6 + q] + mF * c[q]; }
        I6[0] = acc[9] + H.free_inertia[0] + mF * (cc - c[0] * c[0]); I6[1] = acc[10] + H.free_inertia[1] - mF * c[0] * c[1];
        I6[2] = acc[11] + H.free_inertia[2] - mF * c[0] * c[2]; I6[3] = acc[12] + H.free_inertia[4] + mF * (cc - c[1] * c[1]);
        I6[4] = acc[13] + H.free_inertia[5] - mF * c[1] * c[2]; I6[5] = acc[14] + H.free_inertia[8] + mF * (cc - c[2] * c[2]);
        for (int q = 0; q < 6; q++) ow[OF_BIAS + q] = F6[q];
        // M_ff = [[m I, -[mk]x], [[mk]x, I_o]]; kept (21 numbers) for the Euler step's S' = M_ff - sum B B' / (D + h d)
        double Mff[36];
        for (int q = 0; q < 36; q++) Mff[q] = 0;
        Mff[0] = Mff[7] = Mff[14] = H.obj_msum;
        Mff[0 * 6 + 4] = mk[2]; Mff[0 * 6 + 5] = -mk[1]; Mff[1 * 6 + 3] = -mk[2]; Mff[1 * 6 + 5] = mk[0]; Mff[2 * 6 + 3] = mk[1]; Mff[2 * 6 + 4] = -mk[0];
        Mff[21] = I6[0]; Mff[22] = I6[1]; Mff[23] = I6[2]; Mff[28] = I6[3]; Mff[29] = I6[4]; Mff[35] = I6[5];
        for (int r = 0; r < 6; r++)
          for (int q = 0; q < r; q++) Mff[6 * r + q] = Mff[6 * q + r];
        double Sm[36];
        int qq = 0;
        for (int r = 0; r < 6; r++)
          for (int q = r; q < 6; q++) { Sm[6 * r + q] = Sm[6 * q + r] = Mff[6 * r + q] - H.obj_BBD[qq]; ow[OF_MFF + qq] = Mff[6 * r + q]; qq++; }
        spd_inverse6(Sm, ow + OF_SINV);
      }
      SGT_SYNC();
      double red[6] = {0, 0, 0, 0, 0, 0};
      SGT_PAR(e, N)
        for (int q = 0; q < 6; q++) red[q] += S.Be[6 * e + q] * S.fse[e] * S.einvm[e];
      for (int q = 0; q < 6; q++) red[q] = wsum(red[q]);
      double rhs[6], af6[6];
      for (int q = 0; q < 6; q++) rhs[q] = -o[OF_BIAS + q] - red[q];
      mat6vec(af6, o + OF_SINV, rhs);
      SGT_SYNC();
      SGT_ONE { for (int q = 0; q < 6; q++) S.of[OF_ASM + q] = af6[q]; }
      SGT_PAR(e, N) S.asme[e] = (S.fse[e] - dot6(S.Be + 6 * e, af6)) * S.einvm[e];
    }
    if (!FR) SGT_PAR(e, N) {
      const double m = E(SGE_MASS, e), ga = H.gravity[0] * E(SGE_AX, e) + H.gravity[1] * E(SGE_AY, e) + H.gravity[2] * E(SGE_AZ, e);
      const double pas = -S.ke[e] * (S.qe[e] - E(SGE_SPRINGREF, e)) - E(SGE_DAMPING, e) * S.ve[e] + E(SGE_COEF, e) * t0_frc;
      S.fse[e] = pas + m * ga;   // - bias, bias = -m g . axis
      S.asme[e] = S.fse[e] / (m + E(SGE_ARMATURE, e));
      const double dq = S.qe[e] - E(SGE_QPOS0, e);   // the capsule's centre (the pair walk reads it from LDS)
      S.ecen[3 * e] = E(SGE_GX, e) + E(SGE_AX, e) * dq; S.ecen[3 * e + 1] = E(SGE_GY, e) + E(SGE_AY, e) * dq; S.ecen[3 * e + 2] = E(SGE_GZ, e) + E(SGE_AZ, e) * dq;
    }
    SGT_SYNC();

    SGT_STAMP(6);
  }
#define SGT_FRAME SGT_FRAME_STAGE_TAIL
#include "sg_tree_frame.inc"
}

}  // namespace sgt
