// sg_tree_stage_collision.h -- the second stage of a substep: collision over the candidate-pair table -- block culling, the pair walks, rank, narrowphase (part of sg_tree.h)
#pragma once

namespace sgt {

template <int CHD>
static SGT_STAGE_ATTR void tree_stage_collision(SGT_STAGE_PARAMS) {
#define SGT_FRAME SGT_FRAME_STAGE_HEAD
#include "sg_tree_frame.inc"
  {
    // ---------------------------------------------------------------- stage 5: collision over the candidate-pair table
    SGT_ONE { S.icnt[IC_NHIT] = 0; S.icnt[IC_NLIVE] = 0; S.icnt[IC_NPURE] = 0; }
    SGT_SYNC();
    auto elem_center = [&](int e, double* c) { c[0] = S.ecen[3 * e]; c[1] = S.ecen[3 * e + 1]; c[2] = S.ecen[3 * e + 2]; };
    // The table is walked a BLOCK (64 consecutive pairs: one trip of the wavefront) at a time.  A block of (capsule | centre sphere) x
    // finger-box pairs only -- most of the table: a finger body's boxes against 32 elements -- is skipped while every box in it is out
    // of reach of the bounding box of the object (element centres and the centre sphere): no pair of it can pass its own bounding
    // test, let alone produce a contact.  The plan lists a block's boxes behind the table (sg_plan.cpp); the live blocks are
    // gathered in parallel (in any order: the hits are ranked by pair index afterwards), then walked.
    const int ngpair = H.ngpair, nblk = (ngpair + 63) / 64;
    const bool cull = nblk <= 2 * SGT_MAXHIT && T.NG <= SGT_MAXHIT;   // the list lives in hit_sorted + hit_cnt, the boxes' flags in hit_off
    int* const live = S.hit_sorted;
    if (cull) {
      double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
      SGT_PAR(e, N)
        for (int k = 0; k < 3; k++) { lo[k] = fmin(lo[k], S.ecen[3 * e + k]); hi[k] = fmax(hi[k], S.ecen[3 * e + k]); }
      for (int k = 0; k < 3; k++) { lo[k] = -wmax(-lo[k]); hi[k] = wmax(hi[k]); }
      if (H.has_center) {
        const double* cenw = FR ? S.of + OF_CEN : H.center_pos;
        const double ex = fmax(0.0, H.center_radius - H.cap_rbound);
        for (int k = 0; k < 3; k++) { lo[k] = fmin(lo[k], cenw[k] - ex); hi[k] = fmax(hi[k], cenw[k] + ex); }
      }
      SGT_PAR(g, T.NG) {
        double d2 = 0;
        for (int k = 0; k < 3; k++) {
          const double x = S.gpos[3 * g + k], d = fmax(fmax(lo[k] - x, x - hi[k]), 0.0);
          d2 += d * d;
        }
        const double reach = (T.g_rbound[g] + H.cap_rbound + H.con_margin) * 1.000001 + 1e-9;   // (the pairs' own bounds are floats rounded up)
        S.hit_off[g] = d2 > reach * reach ? 1 : 0;
      }
      SGT_SYNC();
      SGT_PAR(b, nblk) {
        const SgGenPair d = gpairs[ngpair + 1 + b];
        bool far = d.kind > 0;
        for (int j = 0; j < d.kind; j++) far = far && S.hit_off[(d.g1 >> (8 * j)) & 0xFF] != 0;
        if (far) continue;
        if (d.kind != 0) live[2 * SGT_MAXHIT - 1 - lds_inc(&S.icnt[IC_NPURE])] = b;   // blocks of the common kind: their own list, from the far end
        else live[lds_inc(&S.icnt[IC_NLIVE])] = b;
      }
      SGT_SYNC();
    }
    SGT_STAMP(20);
    const int nlive = cull ? S.icnt[IC_NLIVE] : nblk;
    {  // blocks of (capsule | centre sphere) x finger box pairs: no kinds to tell apart, everything in LDS -- a trip is ~40 instructions,
       // a fraction of the latency of its table words, so the words of 8 trips are fetched together
      const int npure = cull ? S.icnt[IC_NPURE] : 0;
      const double* const cen0 = FR ? S.of + OF_CEN : H.center_pos;
      const double cen[3] = {cen0[0], cen0[1], cen0[2]};
      constexpr int G = SGT_DEVICE ? 8 : 1;
      const double reach2 = (H.cap_rbound + H.con_margin) * (H.cap_rbound + H.con_margin) * (1.0 + 1e-12);
      for (int b0 = 0; b0 < npure; b0 += G) {
        SgGenPair buf[G];
        int blks[G];
#pragma unroll
        for (int g = 0; g < G; g++) {
          buf[g].kind = SGP_UNSUPPORTED; buf[g].g1 = buf[g].g2 = buf[g].pad = 0;
          blks[g] = b0 + g < npure ? live[2 * SGT_MAXHIT - 1 - (b0 + g)] : -1;
          const int p = blks[g] * 64 + SGT_FIRST;
          // (unconditional loads, all eight in flight together: a trip beyond the list or the table reads the sentinel entry at [ngpair])
          if (SGT_DEVICE) buf[g] = gpairs[blks[g] >= 0 && p < ngpair ? p : ngpair];
        }
#pragma unroll
        for (int g = 0; g < G; g++) {
          if (blks[g] < 0) continue;
          SGT_PAR(j, 64) {
            const int p = blks[g] * 64 + j;
            if (p >= ngpair) continue;
            if (!SGT_DEVICE) buf[g] = gpairs[p];
            const SgGenPair gp = buf[g];
            if (gp.kind == SGP_UNSUPPORTED) continue;
            const int i2 = sgg_index(gp.g2), i1 = sgg_index(gp.g1), k1 = sgg_kind(gp.g1);
            const bool el = k1 == SGG_ELEM, ctr = k1 == SGG_CENTER;
            const double* const c1 = (el ? S.ecen : S.gpos) + (ctr ? 0 : 3 * i1);   // (both in LDS)
            float bf;
            memcpy(&bf, &gp.pad, 4);
            const double bound = (double)bf;
            const double dif[3] = {S.gpos[3 * i2] - (ctr ? cen[0] : c1[0]), S.gpos[3 * i2 + 1] - (ctr ? cen[1] : c1[1]), S.gpos[3 * i2 + 2] - (ctr ? cen[2] : c1[2])};
            if (dot3(dif, dif) > bound * bound) continue;
            if (el) {   // tighter: the capsule's bounding sphere against the box itself
              const double t[3] = {-dif[0], -dif[1], -dif[2]};
              double loc[3];
              mulmatT3(loc, S.gmat + 9 * i2, t);
              // (box_sdist(loc, size) - cap_rbound > margin, without the root: the distance to the box squared against the reach
              //  squared, a hair more permissive -- a filter; the narrowphase decides)
              double q = 0;
              for (int k = 0; k < 3; k++) { const double d = fmax(fabs(loc[k]) - S.gsz[3 * i2 + k], 0.0); q += d * d; }
              if (q > reach2) continue;
            }
            const int idx = lds_inc(&S.icnt[IC_NHIT]);
            if (idx < SGT_MAXHIT) S.hit_pair[idx] = p;
          }
        }
      }
    }
    SGT_STAMP(21);
    {  // 64 pairs at a time; the next trip's table words are fetched before this trip's tests.  The bounding distance of a pair
       // (sum of the bounding radii + margin; plane pairs: rbound + margin) travels in the table as a float rounded up: a filter
       // that passes every pair the exact test passes -- the narrowphase decides
      SgGenPair nxt;
      nxt.kind = SGP_PLANE_CAP; nxt.g1 = nxt.g2 = 0; nxt.pad = (int)0xff800000u;   // (a pair that never hits: bound = -inf)
      if (SGT_DEVICE && nlive > 0) {
        const int p0 = (cull ? live[0] : 0) * 64 + SGT_FIRST;
        nxt = gpairs[p0 < ngpair ? p0 : ngpair];
      }
      for (int bi = 0; bi < nlive; bi++) {
        const int blk = cull ? live[bi] : bi;
        SgGenPair cur = nxt;
        if (SGT_DEVICE) {
          const int p1 = (bi + 1 < nlive ? (cull ? live[bi + 1] : bi + 1) : nblk) * 64 + SGT_FIRST;
          nxt = gpairs[p1 < ngpair ? p1 : ngpair];
        }
        SGT_PAR(j, 64) {
        const int p = blk * 64 + j;
        if (p >= ngpair) continue;
        if (!SGT_DEVICE) cur = gpairs[p];
        const SgGenPair gp = cur;
        const int i1 = sgg_index(gp.g1), i2 = sgg_index(gp.g2), k2 = sgg_kind(gp.g2);
        // (a pair with other contact parameters than the plan's one set, SGP_UNSUPPORTED, is walked like any pair of its geometry:
        //  the narrowphase below turns what would be its contact into the unsupported-pair flag)
        const int gk = gp.kind == SGP_UNSUPPORTED ? sgp_geometry(gp.g1, gp.g2) : gp.kind;
        float bf;
        memcpy(&bf, &gp.pad, 4);
        const double bound = (double)bf;
        bool hit = false;
        const double* cenw = FR ? S.of + OF_CEN : H.center_pos;   // the centre sphere (on the free body when there is one)
        if (gk == SGP_PLANE_CAP || gk == SGP_PLANE_BOX || gk == SGP_PLANE_SPH) {
          const double* c = gk == SGP_PLANE_SPH ? cenw : gk == SGP_PLANE_CAP ? S.ecen + 3 * i2 : (k2 == SGG_BOX ? S.gpos + 3 * i2 : H.st_pos[i2]);
          const double dif[3] = {c[0] - H.plane_pos[0], c[1] - H.plane_pos[1], c[2] - H.plane_pos[2]};
          hit = !(dot3(dif, H.plane_normal) > bound);
        } else {
          // geom2 is a box (finger or static); geom1 the centre sphere, an element capsule or a box
          const double* bp = k2 == SGG_BOX ? S.gpos + 3 * i2 : H.st_pos[i2];
          const int k1 = sgg_kind(gp.g1);
          const double* c = k1 == SGG_CENTER ? cenw : (k1 == SGG_ELEM ? S.ecen + 3 * i1 : (k1 == SGG_BOX ? S.gpos + 3 * i1 : H.st_pos[i1]));
          const double dif[3] = {bp[0] - c[0], bp[1] - c[1], bp[2] - c[2]};
          hit = !(dot3(dif, dif) > bound * bound);
          if (hit && k1 == SGG_ELEM) {   // tighter: the capsule's bounding sphere against the box itself
            const double* bm = k2 == SGG_BOX ? S.gmat + 9 * i2 : H.st_mat[i2];
            const double* sz = k2 == SGG_BOX ? T.g_size[i2] : H.st_size[i2];
            const double t[3] = {-dif[0], -dif[1], -dif[2]};
            double loc[3];
            mulmatT3(loc, bm, t);
            hit = !(box_sdist(loc, sz) - H.cap_rbound > H.con_margin);
          }
        }
        if (hit) {
          const int idx = lds_inc(&S.icnt[IC_NHIT]);
          if (idx < SGT_MAXHIT) S.hit_pair[idx] = p;
        }
        }
      }
    }
    SGT_SYNC();
    SGT_STAMP(7);
    int nhit = S.icnt[IC_NHIT];
    if (nhit > SGT_MAXHIT) { nhit = SGT_MAXHIT; flags |= SG_FLAG_CONTACTFULL; }
    SGT_PAR(i, nhit) {   // rank by pair index = mj_collision's order
      const int p = S.hit_pair[i];
      int r = 0;
      for (int j = 0; j < nhit; j++) r += S.hit_pair[j] < p ? 1 : 0;
      S.hit_sorted[r] = p;
    }
    SGT_SYNC();
    int unsup = 0;
    SGT_PAR(i, nhit) {   // narrowphase, one lane per hit
      SgGenPair gp = gpairs[S.hit_sorted[i]];
      const bool unsupported = gp.kind == SGP_UNSUPPORTED;
      if (unsupported) gp.kind = sgp_geometry(gp.g1, gp.g2);
      const int i1 = sgg_index(gp.g1), i2 = sgg_index(gp.g2), k1 = sgg_kind(gp.g1), k2 = sgg_kind(gp.g2);
      double* out = stage + (size_t)i * SGT_HITREC * SGT_RECW;
      int n = 0;
      auto put = [&](const ConRec& r, const double* hint) {
        double* o = out + n * SGT_RECW;
        o[0] = r.dist;
        for (int k = 0; k < 3; k++) { o[1 + k] = r.pos[k]; o[4 + k] = r.n[k]; o[7 + k] = hint ? hint[k] : 0.0; }
        n++;
      };
      const int st2 = k2 == SGG_STATIC ? i2 : 0;   // (a plane pair's geom2 is an element or a box: no static geom is named, none is read)
      const double* bp = k2 == SGG_BOX ? S.gpos + 3 * i2 : H.st_pos[st2];
      const double* bm = k2 == SGG_BOX ? S.gmat + 9 * i2 : H.st_mat[st2];
      const double* sz = k2 == SGG_BOX ? T.g_size[i2] : H.st_size[st2];
      const double* cenw = FR ? S.of + OF_CEN : H.center_pos;
      auto elem_axis = [&](int e, double* cax) {   // the capsule's axis in the world (it turns with a free body)
        const double cl[3] = {E(SGE_CX, e), E(SGE_CY, e), E(SGE_CZ, e)};
        if (FR) mulmat3(cax, S.of + OF_R, cl);
        else { cax[0] = cl[0]; cax[1] = cl[1]; cax[2] = cl[2]; }
      };
      if (gp.kind == SGP_PLANE_SPH) {   // oracle collision(), plane - sphere branch
        const double e3[3] = {cenw[0] - H.plane_pos[0], cenw[1] - H.plane_pos[1], cenw[2] - H.plane_pos[2]};
        const double dist = dot3(e3, H.plane_normal) - H.center_radius;
        if (!(dist > H.con_margin)) {
          ConRec r0;
          r0.dist = dist;
          for (int k = 0; k < 3; k++) { r0.pos[k] = cenw[k] - H.plane_normal[k] * (H.center_radius + 0.5 * dist); r0.n[k] = H.plane_normal[k]; }
          put(r0, nullptr);
        }
      } else if (gp.kind == SGP_PLANE_CAP) {
        double c[3], cax[3];
        elem_center(i2, c);
        elem_axis(i2, cax);
        ConRec r0, r1;
        const int m = gen_plane_capsule(H.plane_pos, H.plane_normal, c, cax, H.cap_radius, H.cap_hl, H.con_margin, r0, r1);
        if (m > 0) put(r0, cax);
        if (m > 1) put(r1, cax);
      } else if (gp.kind == SGP_PLANE_BOX) {
        ConRec r[4];
        const int m = gen_plane_box(H.plane_pos, H.plane_normal, bp, bm, sz, H.con_margin, r);
        for (int k = 0; k < m; k++) put(r[k], nullptr);
      } else if (gp.kind == SGP_SPH_BOX) {
        ConRec r0;
        if (sphere_box(cenw, H.center_radius, bp, bm, sz, H.con_margin, r0)) put(r0, nullptr);
      } else if (gp.kind == SGP_CAP_BOX) {
        double c[3], cax[3];
        elem_center(i1, c);
        elem_axis(i1, cax);
        ConRec r0, r1;
        const int m = capsule_box(c, cax, H.cap_radius, H.cap_hl, bp, bm, sz, H.con_margin, r0, r1);
        if (m & 1) put(r0, nullptr);
        if (m & 2) put(r1, nullptr);
      } else if (gp.kind == SGP_BOX_BOX) {
        const double* p1 = k1 == SGG_BOX ? S.gpos + 3 * i1 : H.st_pos[i1];
        const double* R1 = k1 == SGG_BOX ? S.gmat + 9 * i1 : H.st_mat[i1];
        const double* s1 = k1 == SGG_BOX ? T.g_size[i1] : H.st_size[i1];
        ConRec r[8];
        double poly[16][3], tmp[16][3];
        const int m = gen_box_box(p1, R1, s1, bp, bm, sz, H.con_margin, r, poly, tmp);
        for (int k = 0; k < m; k++) put(r[k], nullptr);
      }
      if (unsupported) {
        // A pair whose mixed contact parameters differ from the finger / object pairs' (the plan keeps ONE set) cannot become rows.
        // It must not vanish either: what would be its contact raises the unsupported-pair flag -- data, as on the rows pipeline's
        // general path (sg_phase.hip sg_gen_phase) -- and the host resets the env, instead of a finger passing through the geom.
        for (int k = 0; k < n; k++)
          if (out[k * SGT_RECW] < H.con_margin) unsup = 1;
        n = 0;
      }
      S.hit_cnt[i] = n;
    }
    if (wmax((double)unsup) > 0) flags |= SG_FLAG_UNSUPPORTED_PAIR;
    SGT_SYNC();
    SGT_ONE {
      int off = 0;
      for (int i = 0; i < nhit; i++) { S.hit_off[i] = off; off += S.hit_cnt[i]; }
      S.icnt[IC_NCON] = off;
    }
    SGT_SYNC();
    ncon = S.icnt[IC_NCON];
    if (ncon > SGT_MAXCON) { ncon = SGT_MAXCON; flags |= SG_FLAG_CONTACTFULL; }
    SGT_PAR(i, nhit)
      for (int k = 0; k < S.hit_cnt[i]; k++)
        if (S.hit_off[i] + k < SGT_MAXCON) S.con_src[S.hit_off[i] + k] = i * SGT_HITREC + k;
    SGT_SYNC();

    SGT_STAMP(8);
  }
#define SGT_FRAME SGT_FRAME_STAGE_TAIL
#include "sg_tree_frame.inc"
}

}  // namespace sgt
