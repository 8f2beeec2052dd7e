// sg_forces_host.h -- sg_get_forces for ONE env on the host, serially and in the kernels' order: the g++ build of sg_forces.h that the CPU
// tests hold against the oracle (tests/forces_ref.py) and the sanitizer program runs (scripts/sanitize/forces_main.cpp).  Host C++ only;
// no part of the library.  Every sum over the dofs of a row goes through sgf_dot, which adds as the wavefront adds; every stage is the
// kernel's stage: the contact list (sg_contacts_kernel), qacc_smooth and the factor (sg_solve_kernel), the rows (sg_forces_rows_kernel),
// W = M^-1 J' (sg_solve_kernel again), the solve (sg_forces_pgs_kernel).
#pragma once
#include <cmath>
#include <cstring>
#include <vector>

#include "sg_forces.h"         // (first: a test that builds from a patched copy beside this file gets the copy, sg_forces.h's SG_FORCES_H)
#include "sg_readout_host.h"   // the smooth walk, the factor and the sweep

struct SgfHostOut {
  int nefc = 0, ncon = 0, iters = 0, warm_kept = 0;
  std::vector<int> rtype, rid, raux, caddr, cgeom;
  std::vector<double> cdist, cpos, cframe;
  std::vector<double> J, W, sc, f, qfrc, qacc, qacc_smooth;   // J, W [nefc][nv]; sc [nefc][SGF_SC]
};

// sg_contacts_kernel's flow on the records' poses: the list at cap slots.  Returns ncon, or -1 where a pose leaves the oracle's range
inline int sgf_host_contacts(const SgKinHost& K, const SgConHost& C, const double* recs, std::vector<int>* geom, std::vector<double>* dist, std::vector<double>* pos,
                             std::vector<double>* frame) {
  const SgKinOff& o = K.o;
  const double* D = K.dbl.data();
  const int* I = K.ints.data();
  std::vector<double> gx(3 * (size_t)o.ngeom + 1), gm(9 * (size_t)o.ngeom + 1);
  for (int g = 0; g < o.ngeom; g++) {
    sgk_geom(D, I, o, recs + SGS_REC * I[o.gbody + g], g, &gx[3 * g], &gm[9 * g]);
    for (int c = 0; c < 3; c++)
      if (!(fabs(gx[3 * g + c]) <= SG_MAXVAL)) return -1;
  }
  const int cap = C.cap;
  geom->assign(2 * (size_t)cap, 0); dist->assign(cap, 0.0); pos->assign(3 * (size_t)cap, 0.0); frame->assign(9 * (size_t)cap, 0.0);
  int total = 0;
  for (size_t p = 0; p < C.pairs.size() / 2 && total < cap; p++) {
    const int g1 = C.pairs[2 * p], g2 = C.pairs[2 * p + 1], t1 = I[o.gmeta + g1] & 0xFF, t2 = I[o.gmeta + g2] & 0xFF;
    const double margin = fmax(C.gaux[2 * g1], C.gaux[2 * g2]);
    if (!sgc_broad(t1, &gx[3 * g1], &gm[9 * g1], &gx[3 * g2], C.gaux[2 * g1 + 1], C.gaux[2 * g2 + 1], margin)) continue;
    sgm::ConRec rec[SGC_MAXREC];
    double poly[16][3], tmp[16][3];
    int n;
    if (t1 == SG_GEOM_BOX) n = sgm::gen_box_box(&gx[3 * g1], &gm[9 * g1], D + o.gsize + 3 * g1, &gx[3 * g2], &gm[9 * g2], D + o.gsize + 3 * g2, margin, rec, poly, tmp);
    else n = sgc_narrow(t1, t2, &gx[3 * g1], &gm[9 * g1], D + o.gsize + 3 * g1, &gx[3 * g2], &gm[9 * g2], D + o.gsize + 3 * g2, margin, rec);
    for (int c = 0; c < n; c++, total++) {
      if (total >= cap) continue;
      (*geom)[2 * total] = g1; (*geom)[2 * total + 1] = g2;
      (*dist)[total] = rec[c].dist;
      memcpy(&(*pos)[3 * total], rec[c].pos, 24);
      double nn[3] = {rec[c].n[0], rec[c].n[1], rec[c].n[2]};
      sgc_frame(t1, t2, &gm[9 * g2], nn, &(*frame)[9 * total]);
    }
  }
  return total < cap ? total : cap;
}

// one env.  Returns 0, or -1 for an env the kernels end in NaN (a state value that is not finite, a pose out of range, a bad pivot)
inline int sgf_host_env(const SgKinHost& K, const SgConHost& C, const SgDynHost& Dn, const SgSmoothHost& Sm, const SgSolveHost& V, const SgForceHost& Fo,
                        const double* qpos, const double* qvel, const double* act, const double* warm, double kenv, const int* kmask_jnt, const int* kmask_ten,
                        SgfHostOut* out) {
  const SgHostView T(K, Dn, Sm, V);
  const SgKinOff& o = K.o;
  const SgDynOff& d = Dn.o;
  const SgSolveOff& v = V.o;
  const SgForceOff& f = Fo.o;
  const int nv = d.nv;
  const int* VI = V.ints.data();
  for (int i = 0; i < o.nq; i++)
    if (!std::isfinite(qpos[i])) return -1;
  for (int i = 0; i < nv; i++)
    if (!std::isfinite(qvel[i]) || !std::isfinite(warm[i])) return -1;
  // sg_solve_kernel's forward mode: the factor and qacc_smooth
  SgvHostFactor fac;
  {
    std::vector<double> rec((size_t)SGS_REC * o.nbody), S((size_t)SGS_DOF * nv + 1), qfrc_smooth(nv + 1);
    sgs_host_walk(T, qpos, qvel, nullptr, rec.data(), S.data());
    sgv_host_factor(T, rec.data(), S.data(), &fac);
    if (fac.bad) return -1;
    out->qacc_smooth.assign(nv, 0.0);
    sgv_host_forward_smooth(T, qpos, qvel, act, nullptr, kenv, kmask_jnt, kmask_ten, rec.data(), S.data(), fac.F.data(), qfrc_smooth.data(), out->qacc_smooth.data());
  }
  const std::vector<double>& F = fac.F;
  for (int i = 0; i < nv; i++)
    if (!std::isfinite(out->qacc_smooth[i])) return -1;
  // the rows kernel's walk: poses and dof twists, the stamp slots at zero
  std::vector<double> recs((size_t)SGS_REC * o.nbody), S((size_t)SGS_DOF * nv, 0.0), zero(nv + 1, 0.0);
  sgs_host_forward(T, qpos, qvel, nullptr, SGS_REC, recs.data(), S.data());
  out->ncon = sgf_host_contacts(K, C, recs.data(), &out->cgeom, &out->cdist, &out->cpos, &out->cframe);
  if (out->ncon < 0) return -1;
  SgfEnv E;
  E.I = K.ints.data(); E.o = o; E.DD = Dn.dbl.data(); E.DI = Dn.ints.data(); E.d = d; E.VI = VI; E.v = v;
  E.FD = Fo.dbl.data(); E.FI = Fo.ints.data(); E.f = f; E.qpos = qpos; E.zero = zero.data(); E.recs = recs.data(); E.S = S.data();
  E.cgeom = out->cgeom.data(); E.cdist = out->cdist.data(); E.cpos = out->cpos.data(); E.cframe = out->cframe.data();
  out->rtype.assign(f.nrows + 1, 0); out->rid.assign(f.nrows + 1, 0); out->raux.assign(f.nrows + 1, 0); out->caddr.assign(f.cap + 1, -1);
  const int ne = out->nefc = sgf_row_list(E.FD, E.FI, f, E.I, o, qpos, out->ncon, E.cgeom, E.cdist, out->rtype.data(), out->rid.data(), out->raux.data(), out->caddr.data());
  const int *rtype = out->rtype.data(), *rid = out->rid.data(), *raux = out->raux.data();
  out->J.assign((size_t)ne * nv, 0.0); out->W.assign((size_t)ne * nv, 0.0); out->sc.assign((size_t)ne * SGF_SC, 0.0); out->f.assign(ne, 0.0);
  out->qfrc.assign(nv, 0.0); out->qacc = out->qacc_smooth; out->iters = 0; out->warm_kept = 0;
  if (!ne) return 0;
  double *J = out->J.data(), *W = out->W.data(), *sc = out->sc.data(), *fr = out->f.data();
  const double *opt = E.FD + f.opt, timestep = opt[0], tolerance = opt[1], impratio = opt[2], meaninertia = opt[3];
  // the rows stage: a scalar row alone, the rows of a cone together
  for (int i = 0; i < ne;) {
    const int dim = rtype[i] == SGF_ELLIPTIC ? 3 : 1;
    double R[3], jar[3], fric[2] = {0.0, 0.0};
    for (int r = 0; r < dim; r++) {
      double* Jr = J + (size_t)(i + r) * nv;
      for (int c = 0; c < nv; c++) Jr[c] = sgf_row_j(E, rtype[i + r], rid[i + r], raux[i + r], c);
      double pos, margin, dA, solref[2], solimp[5], K1, B1;
      sgf_row_params(E, rtype[i + r], rid[i + r], raux[i + r], &pos, &margin, &dA, solref, solimp);
      const double imp = sgf_impedance(solimp, pos, margin);
      sgf_kb(solref, solimp, imp, dA, timestep, &R[r], &K1, &B1);
      const double aref = sgf_aref(K1, B1, imp, pos, margin, sgf_dot(Jr, qvel, nv));
      sc[(size_t)(i + r) * SGF_SC + SGF_B] = sgf_dot(Jr, out->qacc_smooth.data(), nv) - aref;
      jar[r] = sgf_dot(Jr, warm, nv) - aref;
    }
    if (dim == 3) {
      int cd;
      double solref[2], solimp[5], inc;
      sgf_contact_params(E.FD, E.FI, f, E.cgeom[2 * rid[i]], E.cgeom[2 * rid[i] + 1], &cd, fric, solref, solimp, &inc);
      const double mu = sgf_cone_r(impratio, fric, R);
      const double Dd[3] = {1 / R[0], 1 / R[1], 1 / R[2]};
      double fw[3];
      sgf_warm_cone(mu, fric, Dd, jar, fw);
      for (int r = 0; r < 3; r++) {
        double* s = sc + (size_t)(i + r) * SGF_SC;
        s[SGF_R] = R[r]; s[SGF_F0] = fw[r]; s[SGF_FRIC] = fric[0]; s[SGF_FRIC + 1] = fric[1];
      }
    } else {
      double* s = sc + (size_t)i * SGF_SC;
      s[SGF_R] = R[0]; s[SGF_F0] = sgf_warm_scalar(rtype[i], 1 / R[0], jar[0]);
    }
    i += dim;
  }
  // W = M^-1 J'
  for (int i = 0; i < ne; i++) {
    memcpy(W + (size_t)i * nv, J + (size_t)i * nv, sizeof(double) * nv);
    sgv_host_sweep(V, nv, F.data(), W + (size_t)i * nv);
  }
  // the solver's prologue: the diagonal blocks, the warm start and its gate
  std::vector<double> a(nv, 0.0);
  for (int i = 0; i < ne;) {
    const int dim = rtype[i] == SGF_ELLIPTIC ? 3 : 1;
    for (int j = 0; j < dim; j++)
      for (int k = 0; k < dim; k++)
        sc[(size_t)(i + j) * SGF_SC + SGF_A + k] = sgf_dot(J + (size_t)(i + j) * nv, W + (size_t)(i + k) * nv, nv) + (j == k ? sc[(size_t)(i + j) * SGF_SC + SGF_R] : 0.0);
    i += dim;
  }
  for (int i = 0; i < ne; i++) fr[i] = sc[(size_t)i * SGF_SC + SGF_F0];
  for (int c = 0; c < nv; c++) {
    double s = 0.0;
    for (int i = 0; i < ne; i++) s += W[(size_t)i * nv + c] * fr[i];
    a[c] = s;
  }
  double cost = 0.0;
  for (int i = 0; i < ne; i++) {
    const double* s = sc + (size_t)i * SGF_SC;
    cost += sgf_warm_cost(fr[i], s[SGF_R], sgf_dot(J + (size_t)i * nv, a.data(), nv), s[SGF_B]);
  }
  out->warm_kept = sgf_warm_keep(cost);
  if (!out->warm_kept) {
    for (int i = 0; i < ne; i++) fr[i] = 0.0;
    for (int c = 0; c < nv; c++) a[c] = 0.0;
  }
  // the sweeps
  const double scale = sgf_scale(meaninertia, nv);
  for (int iter = 0; iter < f.iterations; iter++) {
    double improvement = 0.0;
    for (int i = 0; i < ne;) {
      const int dim = rtype[i] == SGF_ELLIPTIC ? 3 : 1;
      double res[3], old[3], A[9];
      for (int j = 0; j < dim; j++) {
        const double* s = sc + (size_t)(i + j) * SGF_SC;
        res[j] = s[SGF_B] + s[SGF_R] * fr[i + j] + sgf_dot(J + (size_t)(i + j) * nv, a.data(), nv);
        old[j] = fr[i + j];
        for (int k = 0; k < dim; k++) A[j * dim + k] = s[SGF_A + k];
      }
      if (dim == 1) fr[i] = sgf_pgs_scalar(rtype[i], res[0], A[0], fr[i]);
      else sgf_pgs_cone(A, res, sc + (size_t)i * SGF_SC + SGF_FRIC, fr + i);
      improvement -= sgf_cost_change(A, fr + i, old, res, dim);
      for (int j = 0; j < dim; j++) {
        const double df = fr[i + j] - old[j];
        if (df != 0.0)
          for (int c = 0; c < nv; c++) a[c] += W[(size_t)(i + j) * nv + c] * df;
      }
      i += dim;
    }
    out->iters = iter + 1;
    if (sgf_sweep_done(improvement, scale, tolerance)) break;
  }
  for (int c = 0; c < nv; c++) {
    double s = 0.0;
    for (int i = 0; i < ne; i++) s += J[(size_t)i * nv + c] * fr[i];
    out->qfrc[c] = s;
    out->qacc[c] = out->qacc_smooth[c] + a[c];
  }
  return 0;
}
// ... on a model's tables
inline int sgf_host_env(const SgHostTables& T, const double* qpos, const double* qvel, const double* act, const double* warm, double kenv, const int* kmask_jnt,
                        const int* kmask_ten, SgfHostOut* out) {
  return sgf_host_env(T.kin, T.con, T.dyn, T.smooth, T.solve, T.forces, qpos, qvel, act, warm, kenv, kmask_jnt, kmask_ten, out);
}
