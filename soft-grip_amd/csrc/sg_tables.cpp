// sg_tables.cpp -- the host builders of the read-outs' per-model tables: kinematics and contact pairs (sg_readout.h), dynamics (sg_dyn.h),
// smooth (sg_smooth.h), point (sg_point.h), forces (sg_forces.h) and -- per skin, at the first call after sg_model_set_skin -- shape
// (sg_shape.h); sg_solve.h builds its own.  sg_tables_build (sg_tables.h) runs them in their one order: sg_model_create (sg_api.hip) calls
// it, and so does everything on the host that wants a model's tables (sg_readout_host.h).  Plain host C++ without a HIP call: every
// variant of the library links it, and the host tests and sanitizer programs compile it with g++.  Every builder either sets ok or
// leaves a message in err.
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>   // (the library's build compiles every source as HIP: the shared headers' __forceinline__)
#endif
#include <algorithm>
#include <cmath>
#include <string>
#include <type_traits>
#include <vector>

#include "sg_blob.h"   // sg_blob_find: the one (bounds-checked) reader of the model blob
#include "sg_point.h"  // (sg_smooth.h, sg_dyn.h, sg_readout.h)
#include "sg_forces.h" // (sg_solve.h; before sg_tables.h: a patched copy beside this file wins, SG_FORCES_H)
#include "sg_tables.h"
#include "sg_shape.h"  // (sg_skin.h)

// ---- the builders sg_model_create calls (sg_readout.h) ----
// an array of the blob as `var`, its length in c (want >= 0: that many elements), or the builder ends with T->err set
#define SG_FIELD(T, var, name, dt, want)                                                                                 \
  const auto* var = (const std::conditional<dt == SG_DT_F64, double, int>::type*)sg_blob_find(blob, nbytes, name, dt, &c); \
  if (!var || (want >= 0 && c != want)) { T->err = std::string("model blob lacks ") + name; return; }

// the kinematics table: per body its parent, body_pos, body_quat and joints; per joint type, jnt_pos, jnt_axis, qposadr, qpos0; per geom body,
// geom_pos, geom_quat (as a matrix), geom_size, geom_type, geom_rbound and a category from the plan; the bodies' depth-level schedule
void sgk_build(const void* blob, size_t nbytes, const SgPlan& plan, const SgTreeDev* tree, bool fast, SgKinHost* K) {
  long long nb = 0, nj = 0, ng = 0, nq = 0, c = 0;
  SG_FIELD(K, par, "body_parentid", SG_DT_I32, -1);
  nb = c;
  SG_FIELD(K, bpos, "body_pos", SG_DT_F64, 3 * nb);
  SG_FIELD(K, bquat, "body_quat", SG_DT_F64, 4 * nb);
  SG_FIELD(K, jadr, "body_jntadr", SG_DT_I32, nb);
  SG_FIELD(K, jnum, "body_jntnum", SG_DT_I32, nb);
  SG_FIELD(K, jtype, "jnt_type", SG_DT_I32, -1);
  nj = c;
  SG_FIELD(K, jpos, "jnt_pos", SG_DT_F64, 3 * nj);
  SG_FIELD(K, jaxis, "jnt_axis", SG_DT_F64, 3 * nj);
  SG_FIELD(K, q0, "qpos0", SG_DT_F64, -1);
  nq = c;
  SG_FIELD(K, gtype, "geom_type", SG_DT_I32, -1);
  ng = c;
  SG_FIELD(K, gbody, "geom_bodyid", SG_DT_I32, ng);
  SG_FIELD(K, gpos, "geom_pos", SG_DT_F64, 3 * ng);
  SG_FIELD(K, gquat, "geom_quat", SG_DT_F64, 4 * ng);
  SG_FIELD(K, gsize, "geom_size", SG_DT_F64, 3 * ng);
  SG_FIELD(K, grb, "geom_rbound", SG_DT_F64, ng);
  long long ca = 0;
  const int* qadr = (const int*)sg_blob_find(blob, nbytes, "jnt_qposadr", SG_DT_I32, &ca);   // (only blobs with a free joint carry it)
  if (qadr && ca != nj) qadr = nullptr;
  if (nb < 1 || nb > 1024) { K->err = "the kinematic tree has more than 1024 bodies"; return; }
  // checks: parents before children, joint / position addresses in range
  std::vector<int> depth(nb, 0);
  for (int i = 1; i < nb; i++) {
    if (par[i] < 0 || par[i] >= i) { K->err = "body parents must precede their children"; return; }
    depth[i] = depth[par[i]] + 1;
    if (jnum[i] < 0 || (jnum[i] > 0 && (jadr[i] < 0 || jadr[i] + jnum[i] > nj))) { K->err = "joint address out of range"; return; }
  }
  for (int j = 0; j < nj; j++) {
    const int qa = qadr ? qadr[j] : j;
    if (qa < 0 || qa + (jtype[j] == SG_JNT_FREE ? 7 : 1) > nq) { K->err = "joint position address out of range"; return; }
    if (jtype[j] != SG_JNT_FREE && jtype[j] != SG_JNT_SLIDE && jtype[j] != SG_JNT_HINGE) { K->err = "unsupported joint type"; return; }
  }
  for (int g = 0; g < ng; g++)
    if (gbody[g] < 0 || gbody[g] >= nb) { K->err = "geom body out of range"; return; }
  // categories from the plan
  std::vector<int> cat(ng, SGR_CAT_STATIC);
  if (plan.h.plane_geom >= 0 && plan.h.plane_geom < ng) cat[plan.h.plane_geom] = SGR_CAT_GROUND;
  for (int g : plan.elem_geom)
    if (g >= 0 && g < ng) cat[g] = SGR_CAT_ELEM;
  if (fast)
    for (int ch = 0; ch < plan.h.nchain; ch++)
      for (int k = 0; k < plan.h.chain[ch].ngeom; k++) cat[plan.h.chain[ch].g_id[k]] = SGR_CAT_FINGER;
  if (tree)
    for (int k = 0; k < tree->NG; k++) cat[tree->g_id[k]] = SGR_CAT_FINGER;
  if (plan.h.has_center && plan.h.center_geom >= 0 && plan.h.center_geom < ng) cat[plan.h.center_geom] = SGR_CAT_CENTER;
  // level schedule (level 0 = the world body)
  int nlevel = 0;
  for (int i = 0; i < nb; i++) nlevel = std::max(nlevel, depth[i] + 1);
  std::vector<int> lstart(nlevel + 1, 0), lbody;
  for (int L = 0; L < nlevel; L++) {
    lstart[L] = (int)lbody.size();
    for (int i = 0; i < nb; i++)
      if (depth[i] == L) lbody.push_back(i);
  }
  lstart[nlevel] = (int)lbody.size();
  SgKinOff& o = K->o;
  o.nbody = (int)nb; o.ngeom = (int)ng; o.njnt = (int)nj; o.nq = (int)nq; o.nlevel = nlevel;
  std::vector<double>& D = K->dbl;
  o.bpos = sg_put(D, bpos, 3 * nb); o.bquat = sg_put(D, bquat, 4 * nb); o.jpos = sg_put(D, jpos, 3 * nj); o.jaxis = sg_put(D, jaxis, 3 * nj);
  std::vector<double> jq0(nj);
  for (int j = 0; j < nj; j++) jq0[j] = q0[qadr ? qadr[j] : j];
  o.jq0 = sg_put(D, jq0);
  o.gpos = sg_put(D, gpos, 3 * ng);
  std::vector<double> gm(9 * ng);
  for (int g = 0; g < ng; g++) sgk_quat_mat(&gm[9 * g], gquat + 4 * g);
  o.gmat = sg_put(D, gm);
  o.gsize = sg_put(D, gsize, 3 * ng);
  std::vector<int>& I = K->ints;
  o.bpar = sg_put(I, par, nb); o.bjadr = sg_put(I, jadr, nb); o.bjnum = sg_put(I, jnum, nb); o.jtype = sg_put(I, jtype, nj);
  std::vector<int> qa(nj), meta(ng);
  for (int j = 0; j < nj; j++) qa[j] = qadr ? qadr[j] : j;
  o.jqadr = sg_put(I, qa);
  o.gbody = sg_put(I, gbody, ng);
  for (int g = 0; g < ng; g++) {
    meta[g] = (gtype[g] & 0xFF) | (cat[g] << 8);
    if (K->bad_type < 0 && gtype[g] != SGR_PLANE && gtype[g] != SGR_SPHERE && gtype[g] != SGR_CAPSULE && gtype[g] != SGR_BOX) K->bad_type = gtype[g];
  }
  o.gmeta = sg_put(I, meta);
  o.lstart = sg_put(I, lstart);
  o.lbody = sg_put(I, lbody);
  K->qpos0.assign(q0, q0 + nq);
  K->rbound.assign(grb, grb + ng);
  K->ok = true;
}

void sgk_host_fk(const SgKinHost& K, std::vector<double>* body) {
  const SgKinOff& o = K.o;
  body->assign((size_t)o.nbody * 7, 0.0);
  (*body)[3] = 1.0;
  for (int i = 1; i < o.nbody; i++) {   // (parents precede children)
    const int p = K.ints[o.bpar + i];
    sgk_body(K.dbl.data(), K.ints.data(), o, K.qpos0.data(), i, &(*body)[7 * p], &(*body)[7 * p + 3], &(*body)[7 * i]);
  }
}

// the default free camera: lookat = centre of the bounding box of the non-plane geoms' centres at qpos0, distance = 2 x (its
// half-diagonal + the largest bounding radius of those geoms), azimuth 90, elevation -30, fovy 45.  (1.5 x half-diagonal + radius cuts
// the near finger off at the image border in every committed scene: the gripper's base box alone has a 1.36 m bounding radius.)
void sgk_default_camera(const SgKinHost& K, double* cam) {
  std::vector<double> body;
  sgk_host_fk(K, &body);
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY}, rb = 0;
  for (int g = 0; g < K.o.ngeom; g++) {
    if ((K.ints[K.o.gmeta + g] & 0xFF) == SGR_PLANE) continue;   // (rb too: a plane's bounding radius is 0 or infinite)
    double gx[3], gm[9];
    sgk_geom(K.dbl.data(), K.ints.data(), K.o, &body[7 * K.ints[K.o.gbody + g]], g, gx, gm);
    for (int k = 0; k < 3; k++) { lo[k] = std::min(lo[k], gx[k]); hi[k] = std::max(hi[k], gx[k]); }
    rb = std::max(rb, K.rbound[g]);
  }
  if (!(lo[0] <= hi[0])) { lo[0] = lo[1] = lo[2] = hi[0] = hi[1] = hi[2] = 0; }
  double hd = 0;
  for (int k = 0; k < 3; k++) { cam[k] = 0.5 * (lo[k] + hi[k]); hd += 0.25 * (hi[k] - lo[k]) * (hi[k] - lo[k]); }
  cam[3] = 2.0 * (sqrt(hd) + rb);
  if (!(cam[3] > 0)) cam[3] = 1.0;
  cam[4] = 90.0; cam[5] = -30.0; cam[6] = 45.0;
}

void sgc_from_blob(const void* blob, size_t nbytes, const SgKinHost& K, SgConHost* C) {
  if (!K.ok) { C->err = K.err; return; }
  long long c = 0;
  const long long nb = K.o.nbody, ng = K.o.ngeom;
  SG_FIELD(C, par, "body_parentid", SG_DT_I32, nb);
  SG_FIELD(C, weld, "body_weldid", SG_DT_I32, nb);
  SG_FIELD(C, gadr, "body_geomadr", SG_DT_I32, nb);
  SG_FIELD(C, gnum, "body_geomnum", SG_DT_I32, nb);
  SG_FIELD(C, gbody, "geom_bodyid", SG_DT_I32, ng);
  SG_FIELD(C, gtype, "geom_type", SG_DT_I32, ng);
  SG_FIELD(C, ctype, "geom_contype", SG_DT_I32, ng);
  SG_FIELD(C, caff, "geom_conaffinity", SG_DT_I32, ng);
  SG_FIELD(C, gmargin, "geom_margin", SG_DT_F64, ng);
  SG_FIELD(C, grb, "geom_rbound", SG_DT_F64, ng);
  const int* oi = (const int*)sg_blob_find(blob, nbytes, "opt_i", SG_DT_I32, &c);
  if (!oi || c < 2) { C->err = "model blob lacks opt_i"; return; }
  C->cap = sgc_cap(oi[1]);
  if (!sgc_build_pairs((int)nb, (int)ng, par, weld, gadr, gnum, gbody, gtype, ctype, caff, &C->pairs, &C->err)) return;
  C->gaux.resize(2 * ng);
  for (int g = 0; g < ng; g++) { C->gaux[2 * g] = gmargin[g]; C->gaux[2 * g + 1] = grb[g]; }
  C->ok = true;
}

// the dynamics table (sg_dyn.h): per body mass, body_ipos, body_imat; per joint its dof, qpos_spring and stiffness; per dof the armature;
// the sites, the tendons and their wraps; gravity.  Tendons of joint wraps only or of site wraps only: the class the blob allows
void sgd_build(const void* blob, size_t nbytes, const SgKinHost& K, SgDynHost* T) {
  if (!K.ok) { T->err = K.err; return; }
  const long long nb = K.o.nbody, nj = K.o.njnt, nq = K.o.nq;
  long long c = 0, nv = 0, ns = 0, nt = 0, nw = 0;
  if (nb > SGD_MAXBODY) { T->err = "more than " + std::to_string(SGD_MAXBODY) + " bodies"; return; }
  SG_FIELD(T, mass, "body_mass", SG_DT_F64, nb);
  SG_FIELD(T, ipos, "body_ipos", SG_DT_F64, 3 * nb);
  SG_FIELD(T, imat, "body_imat", SG_DT_F64, 9 * nb);
  SG_FIELD(T, jstiff, "jnt_stiffness", SG_DT_F64, nj);
  SG_FIELD(T, qspring, "qpos_spring", SG_DT_F64, nq);
  SG_FIELD(T, arm, "dof_armature", SG_DT_F64, -1);
  nv = c;
  SG_FIELD(T, sbody, "site_bodyid", SG_DT_I32, -1);
  ns = c;
  SG_FIELD(T, spos, "site_pos", SG_DT_F64, 3 * ns);
  SG_FIELD(T, tadr, "tendon_adr", SG_DT_I32, -1);
  nt = c;
  SG_FIELD(T, tnum, "tendon_num", SG_DT_I32, nt);
  SG_FIELD(T, tstiff, "tendon_stiffness", SG_DT_F64, nt);
  SG_FIELD(T, tspring, "tendon_lengthspring", SG_DT_F64, nt);
  SG_FIELD(T, wtype, "wrap_type", SG_DT_I32, -1);
  nw = c;
  SG_FIELD(T, wobj, "wrap_objid", SG_DT_I32, nw);
  SG_FIELD(T, wprm, "wrap_prm", SG_DT_F64, nw);
  SG_FIELD(T, optd, "opt_d", SG_DT_F64, -1);
  if (c < 4) { T->err = "model blob lacks opt_d"; return; }
  long long ca = 0;
  const int* dadr = (const int*)sg_blob_find(blob, nbytes, "jnt_dofadr", SG_DT_I32, &ca);   // (only blobs with a free joint carry it)
  if (dadr && ca != nj) dadr = nullptr;
  const int* jtype = K.ints.data() + K.o.jtype;
  std::vector<int> jd(nj);
  std::vector<double> jspring(nj);
  for (int j = 0; j < nj; j++) {
    jd[j] = dadr ? dadr[j] : j;
    if (jd[j] < 0 || jd[j] + (jtype[j] == SG_JNT_FREE ? 6 : 1) > nv) { T->err = "joint dof address out of range"; return; }
    jspring[j] = qspring[K.ints[K.o.jqadr + j]];
  }
  for (int s = 0; s < ns; s++)
    if (sbody[s] < 0 || sbody[s] >= nb) { T->err = "site body out of range"; return; }
  for (int t = 0; t < nt; t++) {
    if (tadr[t] < 0 || tnum[t] < 1 || (long long)tadr[t] + tnum[t] > nw) { T->err = "tendon wrap address out of range"; return; }
    const int type = wtype[tadr[t]];
    if (type != SG_WRAP_JOINT && type != SG_WRAP_SITE) { T->err = "tendon wraps other than joints and sites"; return; }
    for (int w = tadr[t]; w < tadr[t] + tnum[t]; w++) {
      if (wtype[w] != type) { T->err = "a tendon that mixes joint and site wraps"; return; }
      if (wobj[w] < 0 || wobj[w] >= (type == SG_WRAP_JOINT ? nj : ns)) { T->err = "tendon wrap object out of range"; return; }
      if (type == SG_WRAP_JOINT && jtype[wobj[w]] == SG_JNT_FREE) { T->err = "a fixed tendon over a free joint"; return; }
    }
  }
  SgDynOff& o = T->o;
  o.nv = (int)nv; o.nsite = (int)ns; o.ntendon = (int)nt; o.nwrap = (int)nw;
  std::vector<double>& D = T->dbl;
  o.bmass = sg_put(D, mass, nb); o.bipos = sg_put(D, ipos, 3 * nb); o.bimat = sg_put(D, imat, 9 * nb); o.jspring = sg_put(D, jspring);
  o.jstiff = sg_put(D, jstiff, nj); o.arm = sg_put(D, arm, nv); o.spos = sg_put(D, spos, 3 * ns); o.wprm = sg_put(D, wprm, nw); o.tstiff = sg_put(D, tstiff, nt);
  o.tspring = sg_put(D, tspring, nt); o.grav = sg_put(D, optd + 1, 3);
  std::vector<int>& I = T->ints;
  o.jdof = sg_put(I, jd); o.sbody = sg_put(I, sbody, ns); o.tadr = sg_put(I, tadr, nt); o.tnum = sg_put(I, tnum, nt); o.wtype = sg_put(I, wtype, nw);
  o.wobj = sg_put(I, wobj, nw);
  if (I.empty()) I.push_back(0);   // (a model without joints, sites and tendons: the upload still has something to hold)
  T->ok = true;
}

// the dof-parent chain of a model, from the bodies (bpar, bjadr, bjnum), their joints (jtype) and the joints' dofs (jdof): per dof its body
// and its parent dof (the dof before it on the same body, else the last dof of the nearest ancestor that has one, else -1), per body the
// last dof at or above it (-1: none).  The smooth and the point table are both cut from it.  false: *err says what the dofs break
struct SgDofChain {
  std::vector<int> dbody, dpar, last;
};
static bool sg_dof_chain(const SgKinHost& K, const SgDynHost& Dn, SgDofChain* C, std::string* err) {
  const int nb = K.o.nbody, nv = Dn.o.nv;
  const int *par = K.ints.data() + K.o.bpar, *jadr = K.ints.data() + K.o.bjadr, *jnum = K.ints.data() + K.o.bjnum, *jtype = K.ints.data() + K.o.jtype;
  const int* jdof = Dn.ints.data() + Dn.o.jdof;
  std::vector<int>&dbody = C->dbody, &dpar = C->dpar, &last = C->last;
  dbody.assign(nv, -1); dpar.assign(nv, -1); last.assign(nb, -1);
  for (int i = 1; i < nb; i++) {
    last[i] = last[par[i]];
    for (int j = jadr[i]; j < jadr[i] + jnum[i]; j++)
      for (int e = 0; e < (jtype[j] == SG_JNT_FREE ? 6 : 1); e++) {
        const int dof = jdof[j] + e;
        if (dbody[dof] >= 0) { *err = "two joints share a dof"; return false; }
        if (last[i] >= dof) { *err = "dofs must follow the order of the bodies and their joints"; return false; }
        dbody[dof] = i; dpar[dof] = last[i]; last[i] = dof;
      }
  }
  for (int i = 0; i < nv; i++)
    if (dbody[i] < 0) { *err = "a dof without a joint"; return false; }
  return true;
}

// the smooth table (sg_smooth.h): per dof its damping, its body and its parent dof (the dof before it on the same body, else the last dof
// of the nearest ancestor that has one, else -1); per tendon its damping; the actuators on their tendons; the bodies' child lists
void sgs_build(const void* blob, size_t nbytes, const SgKinHost& K, const SgDynHost& Dn, SgSmoothHost* T) {
  if (!K.ok) { T->err = K.err; return; }
  if (K.o.nbody > SGS_MAXBODY) { T->err = "more than " + std::to_string(SGS_MAXBODY) + " bodies"; return; }
  if (!Dn.ok) { T->err = Dn.err; return; }
  const long long nb = K.o.nbody, nv = Dn.o.nv, nt = Dn.o.ntendon;
  if (nv > SGS_MAXDOF) { T->err = "more than " + std::to_string(SGS_MAXDOF) + " dofs"; return; }
  if (nt > SGS_MAXTENDON) { T->err = "more than " + std::to_string(SGS_MAXTENDON) + " tendons"; return; }
  long long c = 0, nu = 0;
  SG_FIELD(T, ddamp, "dof_damping", SG_DT_F64, nv);
  SG_FIELD(T, tdamp, "tendon_damping", SG_DT_F64, nt);
  SG_FIELD(T, atrn, "actuator_trnid", SG_DT_I32, -1);
  nu = c;
  SG_FIELD(T, again, "actuator_gain", SG_DT_F64, nu);
  SG_FIELD(T, abias, "actuator_bias", SG_DT_F64, 3 * nu);
  SG_FIELD(T, agear, "actuator_gear", SG_DT_F64, nu);
  for (int u = 0; u < nu; u++)
    if (atrn[u] < 0 || atrn[u] >= nt) { T->err = "actuator tendon out of range"; return; }
  SgDofChain ch;
  if (!sg_dof_chain(K, Dn, &ch, &T->err)) return;
  const int* par = K.ints.data() + K.o.bpar;
  std::vector<int> cstart(nb + 1, 0), child;
  for (int i = 0; i < nb; i++) {
    cstart[i] = (int)child.size();
    for (int k = i + 1; k < nb; k++)
      if (par[k] == i) child.push_back(k);
  }
  cstart[nb] = (int)child.size();
  SgSmoothOff& o = T->o;
  o.nu = (int)nu; o.nspatial = 0;
  for (int t = 0; t < nt; t++) o.nspatial += Dn.ints[Dn.o.wtype + Dn.ints[Dn.o.tadr + t]] == SG_WRAP_SITE;
  std::vector<double>& D = T->dbl;
  o.ddamp = sg_put(D, ddamp, nv); o.tdamp = sg_put(D, tdamp, nt); o.again = sg_put(D, again, nu); o.abias = sg_put(D, abias, 3 * nu); o.agear = sg_put(D, agear, nu);
  if (D.empty()) D.push_back(0.0);
  std::vector<int>& I = T->ints;
  o.dbody = sg_put(I, ch.dbody); o.dpar = sg_put(I, ch.dpar); o.atrn = sg_put(I, atrn, nu); o.cstart = sg_put(I, cstart);
  o.child = sg_put(I, child);
  T->ok = true;
}

// the point table (sg_point.h): per body where it enters the dof-parent chain, per dof its parent dof; and the model's sites for
// sg_model_sites.  The walk is the smooth table's (sg_dof_chain), the limits before it are its own: the smooth table's (bodies, tendons)
// are not the point read-outs', so a model sgs_build refuses for its size can still have a point table
void sgp_build(const void* blob, size_t nbytes, const SgKinHost& K, const SgDynHost& Dn, SgPointHost* T) {
  if (!K.ok) { T->err = K.err; return; }
  if (!Dn.ok) { T->err = Dn.err; return; }
  const long long nb = K.o.nbody, nv = Dn.o.nv, ns = Dn.o.nsite;
  if (nb > SGP_MAXBODY) { T->err = "more than " + std::to_string(SGP_MAXBODY) + " bodies"; return; }
  if (nv > SGP_MAXDOF) { T->err = "more than " + std::to_string(SGP_MAXDOF) + " dofs"; return; }
  long long c = 0;
  SG_FIELD(T, squat, "site_quat", SG_DT_F64, 4 * ns);
  SgDofChain ch;
  if (!sg_dof_chain(K, Dn, &ch, &T->err)) return;
  std::vector<int>& I = T->ints;
  T->o.bdof = sg_put(I, ch.last); T->o.dpar = sg_put(I, ch.dpar);
  T->site_body.assign(Dn.ints.begin() + Dn.o.sbody, Dn.ints.begin() + Dn.o.sbody + ns);
  T->site_pos.assign(Dn.dbl.begin() + Dn.o.spos, Dn.dbl.begin() + Dn.o.spos + 3 * ns);
  T->site_quat.assign(squat, squat + 4 * ns);
  T->ok = true;
}

// the forces table (sg_forces.h): the equality records, the limited joints, the per-geom solver parameters, the three *_invweight0
// arrays and opt's tolerance, iterations, impratio, meaninertia and njmax.  A model sg_solve_mass refuses is refused with that
// read-out's reason; a condim other than 1 or 3 and an LDS block that does not fit are refused by name
void sgf_build(const void* blob, size_t nbytes, const SgKinHost& K, const SgConHost& C, const SgDynHost& Dn, const SgSolveHost& V, SgForceHost* T) {
  if (!K.ok) { T->err = K.err; return; }
  if (!C.ok) { T->err = C.err; return; }
  if (!V.ok) { T->err = V.err; return; }
  const long long nb = K.o.nbody, nj = K.o.njnt, ng = K.o.ngeom, nq = K.o.nq, nv = Dn.o.nv, nt = Dn.o.ntendon;
  long long c = 0, ne = 0;
  SG_FIELD(T, eqtype, "eq_type", SG_DT_I32, -1);
  ne = c;
  SG_FIELD(T, eqo1, "eq_obj1id", SG_DT_I32, ne);
  SG_FIELD(T, eqo2, "eq_obj2id", SG_DT_I32, ne);
  SG_FIELD(T, eqdata, "eq_data", SG_DT_F64, 5 * ne);
  SG_FIELD(T, eqsolref, "eq_solref", SG_DT_F64, 2 * ne);
  SG_FIELD(T, eqsolimp, "eq_solimp", SG_DT_F64, 5 * ne);
  SG_FIELD(T, tlen0, "tendon_length0", SG_DT_F64, nt);
  SG_FIELD(T, teninvw, "tendon_invweight0", SG_DT_F64, nt);
  SG_FIELD(T, jlimited, "jnt_limited", SG_DT_I32, nj);
  SG_FIELD(T, jrange, "jnt_range", SG_DT_F64, 2 * nj);
  SG_FIELD(T, jmargin, "jnt_margin", SG_DT_F64, nj);
  SG_FIELD(T, jsolref, "jnt_solref", SG_DT_F64, 2 * nj);
  SG_FIELD(T, jsolimp, "jnt_solimp", SG_DT_F64, 5 * nj);
  SG_FIELD(T, gfric, "geom_friction", SG_DT_F64, 3 * ng);
  SG_FIELD(T, gsolref, "geom_solref", SG_DT_F64, 2 * ng);
  SG_FIELD(T, gsolimp, "geom_solimp", SG_DT_F64, 5 * ng);
  SG_FIELD(T, gsolmix, "geom_solmix", SG_DT_F64, ng);
  SG_FIELD(T, ggap, "geom_gap", SG_DT_F64, ng);
  SG_FIELD(T, gmargin, "geom_margin", SG_DT_F64, ng);
  SG_FIELD(T, gcondim, "geom_condim", SG_DT_I32, ng);
  SG_FIELD(T, dofinvw, "dof_invweight0", SG_DT_F64, nv);
  SG_FIELD(T, binvw, "body_invweight0", SG_DT_F64, 2 * nb);
  SG_FIELD(T, q0, "qpos0", SG_DT_F64, nq);
  SG_FIELD(T, optd, "opt_d", SG_DT_F64, -1);
  if (c < 7) { T->err = "model blob lacks opt_d"; return; }
  SG_FIELD(T, opti, "opt_i", SG_DT_I32, -1);
  if (c < 3) { T->err = "model blob lacks opt_i"; return; }
  const int* jtype = K.ints.data() + K.o.jtype;
  for (int e = 0; e < ne; e++) {
    if (eqtype[e] == SG_EQ_JOINT) {
      if (eqo1[e] < 0 || eqo1[e] >= nj || eqo2[e] >= nj || jtype[eqo1[e]] == SG_JNT_FREE || (eqo2[e] >= 0 && jtype[eqo2[e]] == SG_JNT_FREE)) {
        T->err = "joint equality " + std::to_string(e) + " names no scalar joint";
        return;
      }
    } else if (eqtype[e] == SG_EQ_TENDON) {
      if (eqo1[e] < 0 || eqo1[e] >= nt) { T->err = "tendon equality " + std::to_string(e) + " names no tendon"; return; }
    } else {
      T->err = "equality type " + std::to_string(eqtype[e]) + " (joint and tendon equalities only)";
      return;
    }
  }
  // every candidate pair's condim (the larger of its geoms') must be 1 or 3
  for (size_t p = 0; p + 1 < C.pairs.size(); p += 2) {
    const int cd = std::max(gcondim[C.pairs[p]], gcondim[C.pairs[p + 1]]);
    if (cd != 1 && cd != 3) { T->err = "condim " + std::to_string(cd) + " of geoms " + std::to_string(C.pairs[p]) + " and " + std::to_string(C.pairs[p + 1]) + " (1 and 3 only)"; return; }
  }
  std::vector<int> limj;
  for (int j = 0; j < nj; j++)
    if (jlimited[j] && jtype[j] != SG_JNT_FREE) limj.push_back(j);
  SgForceOff& o = T->o;
  o.neq = (int)ne; o.nlim = (int)limj.size(); o.cap = C.cap; o.njmax = opti[2]; o.iterations = opti[0];
  o.nrows = sgf_row_capacity(o.neq, o.nlim, o.cap, o.njmax);
  const long long rows_lds = 8ll * (SGS_REC * nb + SGS_DOF * nv) + 4ll * (3ll * o.nrows + o.cap), pgs_lds = 8ll * (o.nrows + nv);
  if (std::max(rows_lds, pgs_lds) > SGF_LDS_MAX - SGF_STATIC_LDS) {
    T->err = "the row list of " + std::to_string(o.nrows) + " rows beside the bodies' records (" + std::to_string(std::max(rows_lds, pgs_lds)) + " bytes) does not fit the " +
             std::to_string(SGF_LDS_MAX / 1024) + " KB of LDS";
    return;
  }
  std::vector<double>& D = T->dbl;
  o.eqdata = sg_put(D, eqdata, 5 * ne); o.eqsolref = sg_put(D, eqsolref, 2 * ne); o.eqsolimp = sg_put(D, eqsolimp, 5 * ne); o.tlen0 = sg_put(D, tlen0, nt);
  o.jrange = sg_put(D, jrange, 2 * nj); o.jmargin = sg_put(D, jmargin, nj); o.jsolref = sg_put(D, jsolref, 2 * nj); o.jsolimp = sg_put(D, jsolimp, 5 * nj);
  o.gfric = sg_put(D, gfric, 3 * ng); o.gsolref = sg_put(D, gsolref, 2 * ng); o.gsolimp = sg_put(D, gsolimp, 5 * ng); o.gsolmix = sg_put(D, gsolmix, ng);
  o.ggap = sg_put(D, ggap, ng); o.gmargin = sg_put(D, gmargin, ng); o.dofinvw = sg_put(D, dofinvw, nv);
  std::vector<double> bw(nb);
  for (int b = 0; b < nb; b++) bw[b] = binvw[2 * b];
  o.bodyinvw = sg_put(D, bw); o.teninvw = sg_put(D, teninvw, nt); o.q0 = sg_put(D, q0, nq);
  const double opt4[4] = {optd[0], optd[4], optd[5], optd[6]};   // timestep, tolerance, impratio, meaninertia
  o.opt = sg_put(D, opt4, 4);
  std::vector<int>& I = T->ints;
  o.eqtype = sg_put(I, eqtype, ne); o.eqobj1 = sg_put(I, eqo1, ne); o.eqobj2 = sg_put(I, eqo2, ne); o.limj = sg_put(I, limj); o.gcondim = sg_put(I, gcondim, ng);
  if (I.empty()) I.push_back(0);
  T->ok = true;
}

void sg_tables_build(const void* blob, size_t nbytes, const SgPlan& plan, const SgTreeDev* tree, bool fast, SgHostTables* T) {
  sgk_build(blob, nbytes, plan, tree, fast, &T->kin);
  sgc_from_blob(blob, nbytes, T->kin, &T->con);
  sgd_build(blob, nbytes, T->kin, &T->dyn);
  sgs_build(blob, nbytes, T->kin, T->dyn, &T->smooth);
  sgp_build(blob, nbytes, T->kin, T->dyn, &T->point);
  sgv_build(T->kin, T->dyn, T->smooth, &T->solve);
  sgf_build(blob, nbytes, T->kin, T->con, T->dyn, T->solve, &T->forces);
}

// the shape table (sg_shape.h): the skin's vertices (body, position) and faces, whether it is closed -- every directed edge (a, b) of
// its faces once, and (b, a) once --, the deepest body that is an ancestor of every body a vertex is bound to ("the object"), and per
// body its subtree (itself and its descendants, ascending) with the subtree's mass, summed in that order.  The masses, body_ipos and
// body_imat are the dynamics table's.  The skin is no part of the blob and may be empty: the subtree read-out needs none
void sgh_build(const SgKinHost& K, const SgDynHost& Dn, const SgSkinHost& S, SgShapeHost* T) {
  if (!K.ok) { T->err = K.err; return; }
  if (!Dn.ok) { T->err = Dn.err; return; }
  const int nb = K.o.nbody, nvert = S.nvert, nface = S.nface;
  const int* par = K.ints.data() + K.o.bpar;
  const long long lds = sgh_lds_bytes(nb, nvert);
  if (lds > SGH_LDS_MAX - SGH_STATIC_LDS) {
    T->err = "the records of " + std::to_string(nb) + " bodies and " + std::to_string(nvert) + " skin vertices (" + std::to_string(lds) + " bytes) do not fit the " +
             std::to_string(SGH_LDS_MAX / 1024) + " KB of LDS";
    return;
  }
  for (int v = 0; v < nvert; v++)
    if (S.vert_body[v] < 0 || S.vert_body[v] >= nb) { T->err = "skin vertex body out of range"; return; }
  for (int f = 0; f < 3 * nface; f++)
    if (S.face[f] < 0 || S.face[f] >= nvert) { T->err = "skin face vertex out of range"; return; }
  SgShapeOff& o = T->o;
  o.nvert = nvert; o.nface = nface; o.closed = -1; o.root = -1;
  if (nvert > 0) {
    std::vector<std::pair<int, int>> edge;
    edge.reserve(3 * (size_t)nface);
    for (int f = 0; f < nface; f++)
      for (int e = 0; e < 3; e++) edge.push_back({S.face[3 * f + e], S.face[3 * f + (e + 1) % 3]});
    std::sort(edge.begin(), edge.end());
    bool closed = nface > 0 && std::adjacent_find(edge.begin(), edge.end()) == edge.end();
    for (size_t e = 0; closed && e < edge.size(); e++) closed = std::binary_search(edge.begin(), edge.end(), std::make_pair(edge[e].second, edge[e].first));
    o.closed = closed ? 1 : 0;
    int root = S.vert_body[0];
    for (int v = 1; v < nvert; v++) {
      int other = S.vert_body[v];
      while (root != other) {   // (parents precede their children: the larger id climbs)
        if (root > other) root = par[root];
        else other = par[other];
      }
    }
    o.root = root;
  }
  std::vector<std::vector<int>> sub(nb);
  for (int j = 0; j < nb; j++)
    for (int i = j;; i = par[i]) {
      sub[i].push_back(j);
      if (i == 0) break;
    }
  std::vector<int> sstart(nb + 1, 0), slist;
  std::vector<double> smass(nb, 0.0);
  for (int i = 0; i < nb; i++) {
    sstart[i] = (int)slist.size();
    for (int j : sub[i]) { slist.push_back(j); smass[i] += Dn.dbl[Dn.o.bmass + j]; }
  }
  sstart[nb] = (int)slist.size();
  o.nlist = (int)slist.size();
  std::vector<double>& D = T->dbl;
  o.vpos = sg_put(D, S.vert_pos.data(), 3 * (size_t)nvert); o.smass = sg_put(D, smass);
  std::vector<int>& I = T->ints;
  o.vbody = sg_put(I, (const int*)S.vert_body.data(), (size_t)nvert); o.face = sg_put(I, (const int*)S.face.data(), 3 * (size_t)nface);
  o.sstart = sg_put(I, sstart); o.slist = sg_put(I, slist);
  T->ok = true;
}

void sgh_rest(const SgKinHost& K, const SgSkinHost& S, int frame_body, double* rest) {
  std::vector<double> body;
  sgk_host_fk(K, &body);
  double rec[SGD_REC] = {0}, frec[SGD_REC] = {0};
  if (frame_body >= 0)
    for (int c = 0; c < 7; c++) frec[c] = body[7 * (size_t)frame_body + c];
  for (int v = 0; v < S.nvert; v++) {
    for (int c = 0; c < 7; c++) rec[c] = body[7 * (size_t)S.vert_body[v] + c];
    double pv[SGH_VREC];
    sgh_vertex(rec, &S.vert_pos[3 * (size_t)v], pv);
    if (frame_body < 0)
      for (int c = 0; c < 3; c++) rest[3 * v + c] = pv[c];
    else
      sgh_local(frec, pv, rest + 3 * v);
  }
}
