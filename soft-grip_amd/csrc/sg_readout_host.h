// sg_readout_host.h -- the read-out families' host twins: ONE env on the host, serially and in the kernels' order, on the tables
// sg_tables_build makes of a blob.  The g++ build of each family's arithmetic header (sg_dyn.h, sg_smooth.h, sg_point.h, sg_solve.h,
// sg_forces_host.h adds sg_forces.h on top of the pieces here; sg_shape.h has its own driver beside its arithmetic) that the CPU tests hold against the NumPy references and the
// oracle (tests/*_ref.py) and the sanitizer programs run (scripts/sanitize/*_main.cpp).  Host C++ only; no part of the library.
//
// The env drivers (sgd_host_env, sgs_host_env, sgp_host_env, sgv_host_env) are composed from pieces that each stand once:
//   sgd_host_walk      sg_dyn.h's records, bodies by index (in sg_dyn.h, host only: sg_shape.h's sgh_host_env walks with it too)
//   sgs_host_forward   sg_smooth.h's forward walk: the world's record, then the bodies by index
//   sgs_host_walk      ... and back: the bodies' forces, gathered rootwards by descending index, projected on the dofs
//   sgs_host_applied   the tendons, the bodies' tendon pulls gathered rootwards, the dofs' passive and actuator forces
//   sgv_host_factor    the packed M entry by entry, its factor by levels from the deepest, the pivot test
//   sgv_host_sweep     one right-hand side: up sweep by levels, scaling, down sweep
// A change of a kernel's order of operations is mirrored in the one piece that states it.
#pragma once
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/softgrip.h"
#include "../../include/softgrip_model.h"
#include "sg_general.h"
#include "sg_tree_lanes.h"
#include "sg_tree_layout.h"   // sgt::lds_bytes: the tree pipeline's size check of sg_model_create
#include "sg_tables.h"

// ---- a model's tables ----
// the plan that names no geom: the table builders take any blob, and only the geoms' categories (the renderer's) come from the plans
inline std::unique_ptr<SgPlan> sg_host_empty_plan() {
  auto plan = std::make_unique<SgPlan>();
  *plan = SgPlan{};
  plan->h.plane_geom = plan->h.center_geom = -1;
  return plan;
}
// the tables on the empty plan: what every twin runs on
inline void sg_host_tables(const void* blob, size_t n, SgHostTables* T) { sg_tables_build(blob, n, *sg_host_empty_plan(), nullptr, false, T); }
// the tables on the plans as sg_model_create builds them (has_fast / has_tree: which of them took the blob), else -- a blob both refuse,
// where sg_model_create stops -- on the empty plan.  Links sg_plan.cpp
inline void sg_host_tables_planned(const void* blob, size_t n, SgHostTables* T, bool* has_fast, bool* has_tree) {
  auto plan = std::make_unique<SgPlan>(), tplan = std::make_unique<SgPlan>();
  auto tree = std::make_unique<SgTreeDev>();
  memset(tree.get(), 0, sizeof(SgTreeDev));
  std::string err, terr;
  *has_fast = sg_plan_build(blob, n, plan.get(), &err);
  *has_tree = sg_tree_plan_build(blob, n, tplan.get(), tree.get(), &terr);
  if (*has_tree && sgt::lds_bytes(*tree, tplan->h.nelem, tplan->h.has_free, tplan->h.nnb) > 160 * 1024) *has_tree = false;
  if (!*has_fast && !*has_tree) tplan = sg_host_empty_plan();
  sg_tables_build(blob, n, *has_fast ? *plan : *tplan, *has_tree ? tree.get() : nullptr, *has_fast, T);
}

// what the pieces below run on: the kinematics, dynamics, smooth and solve tables -- a model's SgHostTables, or the four by themselves
// (sg_forces_host.h) -- with their offset blocks and arrays under the names the arithmetic headers' parameters have
struct SgHostView {
  const SgSolveHost& solve;
  const SgKinOff& o; const double* D; const int* I;
  const SgDynOff& d; const double* DD; const int* DI;
  const SgSmoothOff& s; const double* SD; const int* SI;
  const SgSolveOff& v; const int* VI;
  SgHostView(const SgKinHost& K, const SgDynHost& Dn, const SgSmoothHost& Sm, const SgSolveHost& V)
      : solve(V), o(K.o), D(K.dbl.data()), I(K.ints.data()), d(Dn.o), DD(Dn.dbl.data()), DI(Dn.ints.data()), s(Sm.o), SD(Sm.dbl.data()), SI(Sm.ints.data()), v(V.o),
        VI(V.ints.data()) {}
  SgHostView(const SgHostTables& T) : SgHostView(T.kin, T.dyn, T.smooth, T.solve) {}
};

// ---- the pieces ----
// sg_smooth.h's forward walk: poses, twists and accelerations in the records, the dofs' twists in S.  qacc NULL: zero.  stride: the
// doubles per record -- SGS_REC, or SGP_REC for the point read-outs, which keep the records' first 19 slots only (sgp_world)
inline void sgs_host_forward(const SgHostView& t, const double* qpos, const double* qvel, const double* qacc, int stride, double* rec, double* S) {
  if (stride == SGP_REC) sgp_world(t.DD, t.d, rec);
  else sgs_world(t.DD, t.d, rec);
  for (int i = 1; i < t.o.nbody; i++) sgs_body(t.D, t.I, t.o, t.DD, t.d, t.DI + t.d.jdof, qpos, qvel, qacc, i, &rec[stride * t.I[t.o.bpar + i]], &rec[stride * i], S);
}

// the whole smooth walk: forward, every body's force, the forces gathered rootwards, slot 6 of a dof's record their projection on it
inline void sgs_host_walk(const SgHostView& t, const double* qpos, const double* qvel, const double* qacc, double* rec, double* S) {
  sgs_host_forward(t, qpos, qvel, qacc, SGS_REC, rec, S);
  for (int i = 1; i < t.o.nbody; i++) sgs_body_force(t.DD, t.d, &rec[SGS_REC * i], i);
  for (int i = t.o.nbody - 1; i >= 1; i--) sgs_gather(t.SI, t.s, rec, i, SGS_ACC, SGS_REC - SGS_ACC);
  for (int i = 0; i < t.d.nv; i++) S[SGS_DOF * i + 6] = sgs_project(&S[SGS_DOF * i], &rec[SGS_REC * t.SI[t.s.dbody + i] + SGS_ACC]);
}

// after the walk: every tendon's length and velocity share by share and its forces, the bodies' tendon pulls gathered rootwards (they
// overwrite the records' force slots; the poses stay), then per dof f[2 i] the passive and f[2 i + 1] the actuator force
inline void sgs_host_applied(const SgHostView& t, const double* qpos, const double* qvel, const double* act, double kenv, const int* kmask_jnt, const int* kmask_ten,
                             double* rec, const double* S, double* f) {
  std::vector<double> ften(2 * (size_t)t.d.ntendon + 1);
  for (int n = 0; n < t.d.ntendon; n++) {
    double L = 0, V = 0;
    const int w0 = t.DI[t.d.tadr + n], ns = sgd_nshare(t.DI, t.d, n);
    for (int k = 0; k < ns; k++) {
      double l1, v1;
      sgs_wrap(t.I, t.o, t.DD, t.DI, t.d, qpos, qvel, rec, w0 + k, &l1, &v1);
      L += l1; V += v1;
    }
    sgs_tendon_force(t.SD, t.SI, t.s, t.DD, t.d, act, n, L, V, kmask_ten[n], kenv, &ften[2 * n]);
  }
  if (t.s.nspatial) {
    for (int i = 0; i < t.o.nbody; i++) sgs_body_tendons(t.DD, t.DI, t.d, ften.data(), rec, i);
    for (int i = t.o.nbody - 1; i >= 1; i--) sgs_gather(t.SI, t.s, rec, i, SGS_ACC, 12);
  }
  for (int i = 0; i < t.d.nv; i++) sgs_dof_applied(t.SD, t.SI, t.s, t.I, t.o, t.DD, t.DI, t.d, qpos, qvel, rec, S, ften.data(), kmask_jnt, kenv, i, f + 2 * i);
}

// the factor by levels from the deepest, in place on a packed M: a level's entries are all read before any is written, then scaled by
// their row's D
inline void sgv_host_factor_levels(const SgSolveHost& V, double* F) {
  const SgSolveOff& v = V.o;
  const int* VI = V.ints.data();
  for (int L = v.nlevel - 1; L >= 0; L--) {
    const int e0 = VI[v.elstart + L], e1 = VI[v.elstart + L + 1];
    std::vector<double> val(e1 - e0);
    for (int q = e0; q < e1; q++) val[q - e0] = sgv_factor_entry(VI, v, F, VI[v.eidx + q]);
    for (int q = e0; q < e1; q++) F[VI[v.eidx + q]] = val[q - e0];
    for (int q = e0; q < e1; q++) {
      const int e = VI[v.eidx + q];
      if (VI[v.anc + e] != VI[v.erow + e]) F[e] = sgv_factor_scale(VI, v, F, e);
    }
  }
}

// after the walk: the packed M, its packed factor, and the pivot test -- bad: some D is not finite or not positive (the kernels end
// such an env in NaN); pivot: min D_i / M_ii, NaN if any ratio is
struct SgvHostFactor {
  std::vector<double> M, F;
  double pivot = 0;
  bool bad = false;
};
inline void sgv_host_factor(const SgHostView& t, const double* rec, const double* S, SgvHostFactor* out) {
  const int nv = t.d.nv;
  std::vector<double> mdiag(nv);
  std::vector<double>& F = out->F;
  F.assign(t.v.nM, 0.0);
  for (int e = 0; e < t.v.nM; e++) {
    F[e] = sgv_mass_entry(t.VI, t.v, t.SI, t.s, t.DD, t.d, rec, S, e);
    if (t.VI[t.v.anc + e] == t.VI[t.v.erow + e]) mdiag[t.VI[t.v.erow + e]] = F[e];
  }
  out->M = F;
  sgv_host_factor_levels(t.solve, F.data());
  double pmin = INFINITY;
  bool pnan = false;
  out->bad = false;
  for (int i = 0; i < nv; i++) {
    const double Di = F[t.VI[t.v.rstart + i]], r = sgv_pivot_ratio(t.VI, t.v, F.data(), mdiag.data(), i);
    out->bad |= !std::isfinite(Di) || !(Di > 0.0);
    pnan |= r != r;
    pmin = fmin(pmin, r);
  }
  out->pivot = pnan ? (double)NAN : pmin;
}

// x <- M^-1 x with the packed factor F: up sweep by levels from the deepest, scaling, down sweep by levels from the roots
inline void sgv_host_sweep(const SgSolveHost& V, int nv, const double* F, double* x) {
  const SgSolveOff& v = V.o;
  const int* VI = V.ints.data();
  for (int L = v.nlevel - 2; L >= 0; L--)
    for (int s = VI[v.lstart + L]; s < VI[v.lstart + L + 1]; s++) { const int j = VI[v.ldof + s]; x[j] = sgv_up(VI, v, F, x, j); }
  for (int i = 0; i < nv; i++) x[i] = sgv_scale(VI, v, F, x, i);
  for (int L = 1; L < v.nlevel; L++)
    for (int s = VI[v.lstart + L]; s < VI[v.lstart + L + 1]; s++) { const int i = VI[v.ldof + s]; x[i] = sgv_down(VI, v, F, x, i); }
}

// sg_solve_kernel's forward mode after the walk and the factor: qfrc_smooth = passive + actuator + applied - bias per dof and
// qacc_smooth = M^-1 qfrc_smooth.  applied NULL: the term is a literal 0.0, which is what sg_get_forces' twin has always added
inline void sgv_host_forward_smooth(const SgHostView& t, const double* qpos, const double* qvel, const double* act, const double* applied, double kenv,
                                    const int* kmask_jnt, const int* kmask_ten, double* rec, const double* S, const double* F, double* qfrc_s, double* qacc_s) {
  const int nv = t.d.nv;
  std::vector<double> f(2 * (size_t)nv + 1);
  sgs_host_applied(t, qpos, qvel, act, kenv, kmask_jnt, kmask_ten, rec, S, f.data());
  for (int i = 0; i < nv; i++) qfrc_s[i] = qacc_s[i] = f[2 * i] + f[2 * i + 1] + (applied ? applied[i] : 0.0) - S[SGS_DOF * i + 6];
  sgv_host_sweep(t.solve, nv, F, qacc_s);
}

// ---- sg_get_velocities / sg_get_tendons / sg_get_energy: bodies by index, then per tendon its shares, then the energy terms ----
struct SgdHostOut {
  std::vector<double> ang, lin, com_lin, poses;   // [nbody][3 | 3 | 3 | 7]
  std::vector<double> ten_len, ten_vel;           // [ntendon]
  double energy[4];                               // gravity, joint springs, tendon springs, kinetic
};
inline void sgd_host_env(const SgHostTables& T, const double* qpos, const double* qvel, double kenv, const int* kmask_jnt, const int* kmask_ten, SgdHostOut* out) {
  const SgHostView t(T);
  const int nb = t.o.nbody;
  std::vector<double> rec;
  sgd_host_walk(T.kin, T.dyn, qpos, qvel, &rec);
  out->ang.assign(3 * (size_t)nb, 0.0); out->lin.assign(3 * (size_t)nb, 0.0); out->com_lin.assign(3 * (size_t)nb, 0.0); out->poses.assign(7 * (size_t)nb, 0.0);
  out->ten_len.assign(t.d.ntendon, 0.0); out->ten_vel.assign(t.d.ntendon, 0.0);
  double e[4] = {0, 0, 0, 0};
  for (int i = 0; i < nb; i++) {
    double xi[3], vc[3];
    sgd_com(t.DD, t.d, &rec[SGD_REC * i], i, xi, vc);
    for (int c = 0; c < 3; c++) { out->ang[3 * i + c] = rec[SGD_REC * i + 7 + c]; out->lin[3 * i + c] = rec[SGD_REC * i + 10 + c]; out->com_lin[3 * i + c] = vc[c]; }
    for (int c = 0; c < 7; c++) out->poses[7 * i + c] = rec[SGD_REC * i + c];
    if (i > 0) {
      double g1, k1;
      sgd_body_energy(t.DD, t.d, &rec[SGD_REC * i], i, &g1, &k1);
      e[0] += g1; e[3] += k1;
    }
  }
  for (int n = 0; n < t.d.ntendon; n++) {
    double L = 0, V = 0;
    const int w0 = t.DI[t.d.tadr + n], ns = sgd_nshare(t.DI, t.d, n);
    for (int k = 0; k < ns; k++) {
      double l1, v1;
      sgd_wrap(t.D, t.I, t.o, t.DD, t.DI, t.d, qpos, qvel, rec.data(), w0 + k, &l1, &v1);
      L += l1; V += v1;
    }
    out->ten_len[n] = L; out->ten_vel[n] = V;
    e[2] += sgd_tendon_spring(t.DD, t.d, n, L, kmask_ten[n], kenv);
  }
  for (int j = 0; j < t.o.njnt; j++) e[1] += sgd_joint_spring(t.I, t.o, t.DD, t.d, qpos, j, kmask_jnt[j], kenv);
  for (int i = 0; i < t.d.nv; i++) e[3] += 0.5 * t.DD[t.d.arm + i] * qvel[i] * qvel[i];
  memcpy(out->energy, e, sizeof e);
}

// ---- sg_get_mass_matrix / sg_get_joint_forces / sg_inverse_dynamics: the walk once at qacc = 0 and, where qacc is given, once before
// that with it; then the tendons, the bodies' tendon pulls, the dofs again ----
struct SgsHostOut {
  std::vector<double> M;                                  // [nv][nv], NaN where sgs_mass_row writes nothing
  std::vector<double> bias, passive, actuator, inverse;   // [nv]; inverse with qacc only
};
inline void sgs_host_env(const SgHostTables& T, const double* qpos, const double* qvel, const double* act, const double* qacc, double kenv, const int* kmask_jnt,
                         const int* kmask_ten, SgsHostOut* out) {
  const SgHostView t(T);
  const int nv = t.d.nv;
  std::vector<double> rec((size_t)SGS_REC * t.o.nbody), S((size_t)SGS_DOF * nv + 1), tau(nv + 1), f(2 * (size_t)nv + 1);
  out->M.assign((size_t)nv * nv, (double)NAN); out->bias.assign(nv, 0.0); out->passive.assign(nv, 0.0); out->actuator.assign(nv, 0.0);
  out->inverse.assign(qacc ? nv : 0, 0.0);
  if (qacc) {
    sgs_host_walk(T, qpos, qvel, qacc, rec.data(), S.data());
    for (int i = 0; i < nv; i++) tau[i] = S[SGS_DOF * i + 6];
  }
  sgs_host_walk(T, qpos, qvel, nullptr, rec.data(), S.data());
  for (int i = 0; i < nv; i++) out->bias[i] = S[SGS_DOF * i + 6];
  for (int i = 0; i < nv; i++) sgs_mass_row(t.SI, t.s, t.DD, t.d, rec.data(), S.data(), i, out->M.data());
  sgs_host_applied(T, qpos, qvel, act, kenv, kmask_jnt, kmask_ten, rec.data(), S.data(), f.data());
  for (int i = 0; i < nv; i++) {
    out->passive[i] = f[2 * i]; out->actuator[i] = f[2 * i + 1];
    if (qacc) out->inverse[i] = tau[i] + t.DD[t.d.arm + i] * qacc[i] - f[2 * i];
  }
}

// ---- sg_get_point_motion / sg_get_jacobians: the forward walk on SGP_REC records, then the points' motion, then the Jacobians point by
// point: the chain walk that stamps the dofs, then column by column.  qacc, pt_quat NULL: zero, the body's frame ----
struct SgpHostOut {
  std::vector<double> pos, mat, vel, acc, gyro, accel;   // [n_pts][3 | 9 | 6 | 6 | 3 | 3]
  std::vector<double> jacp, jacr;                        // [n_pts][3][nv]
};
inline void sgp_host_env(const SgHostTables& T, const double* qpos, const double* qvel, const double* qacc, int n_pts, const int* pt_body, const double* pt_pos,
                         const double* pt_quat, SgpHostOut* out) {
  const SgHostView t(T);
  const SgPointOff& pt = T.point.o;
  const int* PI = T.point.ints.data();
  const size_t nv = t.d.nv, P = n_pts;
  std::vector<double> rec((size_t)SGP_REC * t.o.nbody), S((size_t)SGP_DOF * nv + 1, 0.0);
  sgs_host_forward(T, qpos, qvel, qacc, SGP_REC, rec.data(), S.data());
  out->pos.assign(3 * P, 0.0); out->mat.assign(9 * P, 0.0); out->vel.assign(6 * P, 0.0); out->acc.assign(6 * P, 0.0); out->gyro.assign(3 * P, 0.0);
  out->accel.assign(3 * P, 0.0); out->jacp.assign(3 * P * nv, 0.0); out->jacr.assign(3 * P * nv, 0.0);
  for (int p = 0; p < n_pts; p++) {
    const double* r = &rec[SGP_REC * pt_body[p]];
    sgp_motion(t.DD, t.d, r, pt_pos + 3 * p, pt_quat ? pt_quat + 4 * p : nullptr, &out->pos[3 * p], &out->mat[9 * p], &out->vel[6 * p], &out->acc[6 * p],
               &out->gyro[3 * p], &out->accel[3 * p]);
    double X[3];
    sgp_pos(r, pt_pos + 3 * p, X);
    sgp_mark(PI, pt, PI + pt.dpar, pt_body[p], S.data(), (double)(p + 1));
    for (size_t i = 0; i < nv; i++) {
      double jp[3], jr[3];
      sgp_jac_col(&S[SGP_DOF * i], (double)(p + 1), X, jp, jr);
      for (int c = 0; c < 3; c++) { out->jacp[(3 * p + c) * nv + i] = jp[c]; out->jacr[(3 * p + c) * nv + i] = jr[c]; }
    }
  }
}

// ---- sg_solve_mass / sg_forward_smooth / sg_get_point_inertia, all three modes on one walk and one factor: the right-hand sides y
// [n_rhs][nv]; the points' W = J M^-1 J' (before the tendons' pulls overwrite the records' force slots); qacc_smooth with applied (NULL:
// none) added to qfrc_smooth, which sg_forward_smooth alone takes.  An env with a bad pivot ends in NaN, as the kernels end it ----
struct SgvHostOut {
  std::vector<double> x, qacc_smooth, qfrc_smooth, W;   // [n_rhs][nv], [nv], [nv], [n_pts][6][6]
  SgvHostFactor fac;                                    // the packed M and factor, the pivot figure, the pivot-bad flag
  long long tile = 0;                                   // right-hand sides per tile
  std::vector<int> levels;                              // dofs per depth
};
inline void sgv_host_env(const SgHostTables& T, const double* qpos, const double* qvel, const double* act, double kenv, const int* kmask_jnt, const int* kmask_ten,
                         int n_rhs, const double* y, const double* applied, int n_pts, const int* pt_body, const double* pt_pos, SgvHostOut* out) {
  const SgHostView t(T);
  const SgSolveOff& v = t.v;
  const int* VI = t.VI;
  const int nv = t.d.nv;
  out->tile = sgv_tile(t.o.nbody, nv, t.d.ntendon, v.nM);
  out->levels.resize(v.nlevel);
  for (int L = 0; L < v.nlevel; L++) out->levels[L] = VI[v.lstart + L + 1] - VI[v.lstart + L];
  std::vector<double> rec((size_t)SGS_REC * t.o.nbody), S((size_t)SGS_DOF * nv + 1), X(6 * (size_t)nv);
  sgs_host_walk(T, qpos, qvel, nullptr, rec.data(), S.data());
  sgv_host_factor(T, rec.data(), S.data(), &out->fac);
  const double fill = out->fac.bad ? (double)NAN : 0.0;
  out->x.assign((size_t)n_rhs * nv, fill); out->qacc_smooth.assign(nv, fill); out->qfrc_smooth.assign(nv, fill); out->W.assign(36 * (size_t)n_pts, fill);
  if (out->fac.bad) return;
  const double* F = out->fac.F.data();
  for (int r = 0; r < n_rhs; r++) {
    memcpy(&out->x[(size_t)r * nv], y + (size_t)r * nv, sizeof(double) * nv);
    sgv_host_sweep(T.solve, nv, F, &out->x[(size_t)r * nv]);
  }
  for (int p = 0; p < n_pts; p++) {
    const int body = pt_body[p], e0 = VI[v.bdof + body];
    double P[3], *W = &out->W[36 * (size_t)p];
    sgp_pos(&rec[SGS_REC * body], pt_pos + 3 * p, P);
    std::fill(X.begin(), X.end(), 0.0);
    if (e0 >= 0)
      for (int k = 0; k <= VI[v.depth + e0]; k++) {
        const int dd = VI[v.anc + VI[v.rstart + e0] + k];
        double c6[6];
        sgv_jcol(&S[SGS_DOF * dd], P, c6);
        for (int c = 0; c < 6; c++) X[(size_t)c * nv + dd] = c6[c];
      }
    for (int c = 0; c < 6; c++) sgv_host_sweep(T.solve, nv, F, &X[(size_t)c * nv]);
    for (int b = 0; b < 6; b++)
      for (int c = 0; c <= b; c++) W[6 * c + b] = W[6 * b + c] = sgv_w_entry(VI, v, S.data(), X.data(), nv, e0, P, c, b);
  }
  sgv_host_forward_smooth(T, qpos, qvel, act, applied, kenv, kmask_jnt, kmask_ten, rec.data(), S.data(), F, out->qfrc_smooth.data(), out->qacc_smooth.data());
}
