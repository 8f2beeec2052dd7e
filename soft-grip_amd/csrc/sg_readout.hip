// sg_readout.hip -- the read-out half of the C ABI (include/softgrip.h): sg_get_poses, sg_render / sg_render_ex and the skin,
// sg_get_contacts, sg_ray, sg_get_velocities / sg_get_tendons / sg_get_energy, sg_get_mass_matrix / sg_get_joint_forces /
// sg_inverse_dynamics, sg_get_point_motion / sg_get_jacobians, sg_solve_mass / sg_forward_smooth / sg_get_point_inertia, with the kernels
// they launch (the *_kernel*.h files, whose device assembly is sg_readout.device.s) and the host builders of their per-model tables
// (sg_readout.h, sg_dyn.h, sg_smooth.h, sg_point.h; sg_solve.h builds its own).  None of them writes the state: every pipeline is served.  No CPU fallback.
#include <algorithm>
#include <cstring>
#include <type_traits>

#include "sg_batch.h"
#include "sg_blob.h"   // sg_blob_find: the one (bounds-checked) reader of the model blob
#include "sg_kin_kernels.h"
#include "sg_contacts_kernel.h"
#include "sg_ray_kernels.h"
#include "sg_ray_skin_kernels.h"
#include "sg_dyn_kernel.h"
#include "sg_smooth_kernel.h"
#include "sg_point_kernel.h"
#include "sg_solve_kernel.h"

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
  auto putd = [&](const double* p, size_t n) { int at = (int)D.size(); D.insert(D.end(), p, p + n); return at; };
  o.bpos = putd(bpos, 3 * nb); o.bquat = putd(bquat, 4 * nb); o.jpos = putd(jpos, 3 * nj); o.jaxis = putd(jaxis, 3 * nj);
  std::vector<double> jq0(nj);
  for (int j = 0; j < nj; j++) jq0[j] = q0[qadr ? qadr[j] : j];
  o.jq0 = putd(jq0.data(), nj);
  o.gpos = putd(gpos, 3 * ng);
  std::vector<double> gm(9 * ng);
  for (int g = 0; g < ng; g++) sgk_quat_mat(&gm[9 * g], gquat + 4 * g);
  o.gmat = putd(gm.data(), 9 * ng);
  o.gsize = putd(gsize, 3 * ng);
  std::vector<int>& I = K->ints;
  auto puti = [&](const int* p, size_t n) { int at = (int)I.size(); I.insert(I.end(), p, p + n); return at; };
  o.bpar = puti(par, nb); o.bjadr = puti(jadr, nb); o.bjnum = puti(jnum, nb); o.jtype = puti(jtype, nj);
  std::vector<int> qa(nj), meta(ng);
  for (int j = 0; j < nj; j++) qa[j] = qadr ? qadr[j] : j;
  o.jqadr = puti(qa.data(), nj);
  o.gbody = puti(gbody, ng);
  for (int g = 0; g < ng; g++) {
    meta[g] = (gtype[g] & 0xFF) | (cat[g] << 8);
    if (K->bad_type < 0 && gtype[g] != SGR_PLANE && gtype[g] != SGR_SPHERE && gtype[g] != SGR_CAPSULE && gtype[g] != SGR_BOX) K->bad_type = gtype[g];
  }
  o.gmeta = puti(meta.data(), ng);
  o.lstart = puti(lstart.data(), lstart.size());
  o.lbody = puti(lbody.data(), lbody.size());
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
  auto putd = [&](const double* p, size_t n) { int at = (int)D.size(); D.insert(D.end(), p, p + n); return at; };
  o.bmass = putd(mass, nb); o.bipos = putd(ipos, 3 * nb); o.bimat = putd(imat, 9 * nb); o.jspring = putd(jspring.data(), nj);
  o.jstiff = putd(jstiff, nj); o.arm = putd(arm, nv); o.spos = putd(spos, 3 * ns); o.wprm = putd(wprm, nw); o.tstiff = putd(tstiff, nt);
  o.tspring = putd(tspring, nt); o.grav = putd(optd + 1, 3);
  std::vector<int>& I = T->ints;
  auto puti = [&](const int* p, size_t n) { int at = (int)I.size(); I.insert(I.end(), p, p + n); return at; };
  o.jdof = puti(jd.data(), nj); o.sbody = puti(sbody, ns); o.tadr = puti(tadr, nt); o.tnum = puti(tnum, nt); o.wtype = puti(wtype, nw);
  o.wobj = puti(wobj, nw);
  if (I.empty()) I.push_back(0);   // (a model without joints, sites and tendons: the upload still has something to hold)
  T->ok = true;
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
  const int *par = K.ints.data() + K.o.bpar, *jadr = K.ints.data() + K.o.bjadr, *jnum = K.ints.data() + K.o.bjnum, *jtype = K.ints.data() + K.o.jtype;
  const int* jdof = Dn.ints.data() + Dn.o.jdof;
  std::vector<int> dbody(nv, -1), dpar(nv, -1), last(nb, -1);   // last[i]: the last dof of body i or of its nearest ancestor with one
  for (int i = 1; i < nb; i++) {
    last[i] = last[par[i]];
    for (int j = jadr[i]; j < jadr[i] + jnum[i]; j++)
      for (int e = 0; e < (jtype[j] == SG_JNT_FREE ? 6 : 1); e++) {
        const int dof = jdof[j] + e;
        if (dbody[dof] >= 0) { T->err = "two joints share a dof"; return; }
        if (last[i] >= dof) { T->err = "dofs must follow the order of the bodies and their joints"; return; }
        dbody[dof] = i; dpar[dof] = last[i]; last[i] = dof;
      }
  }
  for (int i = 0; i < nv; i++)
    if (dbody[i] < 0) { T->err = "a dof without a joint"; return; }
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
  auto putd = [&](const double* p, size_t n) { int at = (int)D.size(); D.insert(D.end(), p, p + n); return at; };
  o.ddamp = putd(ddamp, nv); o.tdamp = putd(tdamp, nt); o.again = putd(again, nu); o.abias = putd(abias, 3 * nu); o.agear = putd(agear, nu);
  if (D.empty()) D.push_back(0.0);
  std::vector<int>& I = T->ints;
  auto puti = [&](const int* p, size_t n) { int at = (int)I.size(); I.insert(I.end(), p, p + n); return at; };
  o.dbody = puti(dbody.data(), nv); o.dpar = puti(dpar.data(), nv); o.atrn = puti(atrn, nu); o.cstart = puti(cstart.data(), nb + 1);
  o.child = puti(child.data(), child.size());
  T->ok = true;
}

// the point table (sg_point.h): per body where it enters the dof-parent chain, per dof its parent dof; and the model's sites for
// sg_model_sites.  Its own walk over the bodies, as the smooth table's limits (bodies, tendons) are not the point read-outs'
void sgp_build(const void* blob, size_t nbytes, const SgKinHost& K, const SgDynHost& Dn, SgPointHost* T) {
  if (!K.ok) { T->err = K.err; return; }
  if (!Dn.ok) { T->err = Dn.err; return; }
  const long long nb = K.o.nbody, nv = Dn.o.nv, ns = Dn.o.nsite;
  if (nb > SGP_MAXBODY) { T->err = "more than " + std::to_string(SGP_MAXBODY) + " bodies"; return; }
  if (nv > SGP_MAXDOF) { T->err = "more than " + std::to_string(SGP_MAXDOF) + " dofs"; return; }
  long long c = 0;
  SG_FIELD(T, squat, "site_quat", SG_DT_F64, 4 * ns);
  const int *par = K.ints.data() + K.o.bpar, *jadr = K.ints.data() + K.o.bjadr, *jnum = K.ints.data() + K.o.bjnum, *jtype = K.ints.data() + K.o.jtype;
  const int* jdof = Dn.ints.data() + Dn.o.jdof;
  std::vector<int> bdof(nb, -1), dpar(nv, -2);
  for (int i = 1; i < nb; i++) {
    bdof[i] = bdof[par[i]];
    for (int j = jadr[i]; j < jadr[i] + jnum[i]; j++)
      for (int e = 0; e < (jtype[j] == SG_JNT_FREE ? 6 : 1); e++) {
        const int dof = jdof[j] + e;
        if (dpar[dof] != -2) { T->err = "two joints share a dof"; return; }
        if (bdof[i] >= dof) { T->err = "dofs must follow the order of the bodies and their joints"; return; }
        dpar[dof] = bdof[i]; bdof[i] = dof;
      }
  }
  for (int i = 0; i < nv; i++)
    if (dpar[i] == -2) { T->err = "a dof without a joint"; return; }
  std::vector<int>& I = T->ints;
  auto puti = [&](const int* p, size_t n) { int at = (int)I.size(); I.insert(I.end(), p, p + n); return at; };
  T->o.bdof = puti(bdof.data(), nb); T->o.dpar = puti(dpar.data(), nv);
  T->site_body.assign(Dn.ints.begin() + Dn.o.sbody, Dn.ints.begin() + Dn.o.sbody + ns);
  T->site_pos.assign(Dn.dbl.begin() + Dn.o.spos, Dn.dbl.begin() + Dn.o.spos + 3 * ns);
  T->site_quat.assign(squat, squat + 4 * ns);
  T->ok = true;
}

// ---- the entry points' common prologue ----
// One read-out call on stream s: prepare() puts the kinematics table on the batch's device and the listed env ids (host array,
// range-checked here) in a device buffer, reserve() grows a scratch buffer of the batch, kin() launches sg_kin_kernel over the listed envs.
// Every message carries fn, the calling entry point's name.
struct Readout {
  sg_batch* b;
  const char* fn;
  hipStream_t s;
  const int* dids = nullptr;   // the env ids on the device (NULL: env k = k)
  int n_ids = 0;

  int prepare(const int32_t* env_ids, int n) {
    const SgKinHost& K = b->m->kin;
    if (!K.ok) return fail(SG_ERR_MODEL, std::string(fn) + ": " + K.err);
    if (n <= 0) return fail(SG_ERR_INVALID, std::string(fn) + ": n_ids must be positive");
    if (!env_ids && n != b->n) return fail(SG_ERR_INVALID, std::string(fn) + ": env_ids == NULL needs n_ids == the batch's env count");
    if (env_ids)
      for (int i = 0; i < n; i++)
        if (env_ids[i] < 0 || env_ids[i] >= b->n)
          return fail(SG_ERR_INVALID, std::string(fn) + ": env id " + std::to_string(env_ids[i]) + " out of range [0, " + std::to_string(b->n) + ")");
    HIPCHK(hipSetDevice(b->device));
    if (!b->kin_d) {   // built on the side: the batch sees the tables only once both are filled
      SgArena A;
      double* d = nullptr;
      int* ip = nullptr;
      if (!(A.upload(&d, K.dbl) && A.upload(&ip, K.ints))) return devmem_fail(A.nomem, std::string(fn) + " (pose tables)");
      A.give_to(b->mem);
      b->kin_d = d; b->kin_i = ip;
    }
    n_ids = n;
    if (env_ids) {
      if (int rc = reserve(b->kin_ids, n, "env ids")) return rc;
      HIPCHK(hipMemcpyAsync(b->kin_ids.p, env_ids, sizeof(int) * n, hipMemcpyHostToDevice, s));
      dids = b->kin_ids.p;
    }
    return SG_OK;
  }

  template <class T>
  int reserve(SgScratch<T>& buf, size_t count, const char* what) {
    return buf.reserve(count, s) ? SG_OK : devmem_fail(buf.nomem, std::string(fn) + " (" + what + ")");
  }

  int kin(double* xpos, double* xquat, double* gxpos, double* gxmat, float* recs, const double* eye) {
    const SgKinHost& K = b->m->kin;
    SgKinArgs a;
    a.D = b->kin_d; a.I = b->kin_i; a.o = K.o; a.qpos = b->qpos; a.env_ids = dids; a.n_ids = n_ids;
    a.xpos = xpos; a.xquat = xquat; a.gxpos = gxpos; a.gxmat = gxmat; a.recs = recs;
    for (int c = 0; c < 3; c++) a.eye[c] = eye ? eye[c] : 0.0;
    hipLaunchKernelGGL(sg_kin_kernel, dim3(n_ids), dim3(64), sizeof(double) * 7 * K.o.nbody, s, a);
    HIPCHK(hipGetLastError());
    return SG_OK;
  }
};

// the skin's tables on the batch's device, uploaded again when the model's skin has changed since (an earlier skin render, on whatever
// stream it went out, may still read the old ones: the device is waited for first -- once per sg_model_set_skin, not per render).  fn: the
// calling entry point's name (sg_render_ex, sg_ray)
static int skin_prepare(sg_batch* b, const char* fn) {
  const SgSkinHost& S = b->m->skin;
  if (b->skin_version == S.version) return SG_OK;
  const SgKinHost& K = b->m->kin;
  SgSkinTables T;
  sg_skin_tables(S, K.ints.data() + K.o.gbody, K.o.ngeom, K.o.nbody, &T);
  HIPCHK(hipDeviceSynchronize());
  b->skin_version = 0;
  b->skin_mem.release();
  SgArena& A = b->skin_mem;
  int *vb = nullptr, *as = nullptr, *ad = nullptr, *hid = nullptr, *vis = nullptr;
  std::vector<int> visible;   // (sg_ray with SG_RAY_SKIN stages these alone)
  for (int g = 0; g < K.o.ngeom; g++)
    if (!T.hidden[g]) visible.push_back(g);
  double* vp = nullptr;
  uint32_t* fc = nullptr;
  if (!(A.upload(&vb, S.vert_body) && A.upload(&vp, S.vert_pos) && A.upload(&fc, T.faces) && A.upload(&as, T.adj_start) && A.upload(&ad, T.adj) &&
        A.upload(&hid, T.hidden) && A.upload(&vis, visible))) {
    const bool nomem = A.nomem;
    A.release();
    return devmem_fail(nomem, std::string(fn) + " (skin tables)");
  }
  b->skin_vis = vis; b->skin_nvis = (int)visible.size();
  SgSkinDev& d = b->skin_dev;
  d.vert_body = vb; d.vert_pos = vp; d.faces = fc; d.adj_start = as; d.adj = ad; d.hidden = hid;
  d.nvert = S.nvert; d.nface = S.nface;
  for (int c = 0; c < 3; c++) d.rgb[c] = S.rgba[c];
  b->skin_version = S.version;
  return SG_OK;
}

// sg_render (skin == false, fn "sg_render") and sg_render_ex with the skin drawn (fn "sg_render_ex"): argument and model checks before
// anything touches the device, the geoms' records (and the skin's vertex records) of the listed envs, then a workgroup per tile and env
static int render(const char* fn, bool skin, sg_batch* b, const double* cam, const int32_t* env_ids, int n_ids, int width, int height, uint8_t* rgba,
                  float* depth, int32_t* segid, void* stream) {
  const std::string f = std::string(fn) + ": ";
  if (!b || !cam) return fail(SG_ERR_INVALID, f + "null batch or camera");
  if (width <= 0 || height <= 0 || width > 16384 || height > 16384) return fail(SG_ERR_INVALID, f + "image size out of range (1 .. 16384)");
  for (int c = 0; c < 7; c++)
    if (!std::isfinite(cam[c])) return fail(SG_ERR_INVALID, f + "camera values must be finite");
  if (!(cam[3] > 0) || !(cam[6] > 0 && cam[6] < 180)) return fail(SG_ERR_INVALID, f + "camera distance must be > 0 and fovy in (0, 180)");
  const SgKinHost& K = b->m->kin;
  if (K.ok && K.bad_type >= 0)
    return fail(SG_ERR_MODEL, f + "geom type " + std::to_string(K.bad_type) + " has no ray intersection (plane, sphere, capsule and box only)");
  if (K.ok && K.o.ngeom > SGR_MAXGEOM) return fail(SG_ERR_MODEL, f + "more than " + std::to_string(SGR_MAXGEOM) + " geoms");
  Readout r{b, fn, (hipStream_t)stream};
  if (int rc = r.prepare(env_ids, n_ids)) return rc;
  if (skin)
    if (int rc = skin_prepare(b, fn)) return rc;
  if (int rc = r.reserve(b->rrecs, (size_t)n_ids * K.o.ngeom * SGR_REC, "geom records")) return rc;
  if (skin) {
    if (int rc = r.reserve(b->skin_xpos, (size_t)n_ids * K.o.nbody * 3, "body poses")) return rc;
    if (int rc = r.reserve(b->skin_xquat, (size_t)n_ids * K.o.nbody * 4, "body poses")) return rc;
    if (int rc = r.reserve(b->skin_vrec, (size_t)n_ids * b->m->skin.nvert * SGR_VREC, "vertex records")) return rc;
  }
  SgSkinRenderArgs A;   // (A.r alone is the plain renderer's argument)
  SgRenderArgs& a = A.r;
  double eye[3];
  sgr_camera(cam, width, height, eye, &a.cam);
  if (int rc = r.kin(skin ? b->skin_xpos.p : nullptr, skin ? b->skin_xquat.p : nullptr, nullptr, nullptr, b->rrecs.p, eye)) return rc;
  if (skin) {
    SgSkinVertArgs V;
    V.s = b->skin_dev; V.xpos = b->skin_xpos.p; V.xquat = b->skin_xquat.p; V.nbody = K.o.nbody; V.vrec = b->skin_vrec.p;
    for (int c = 0; c < 3; c++) V.eye[c] = eye[c];
    hipLaunchKernelGGL(sg_skin_vert_kernel, dim3(n_ids), dim3(256), 0, r.s, V);
    HIPCHK(hipGetLastError());
    A.s = b->skin_dev; A.vrec = b->skin_vrec.p;
  }
  a.recs = b->rrecs.p; a.ngeom = K.o.ngeom; a.n_ids = n_ids;
  a.tiles_x = (width + SGR_TILE - 1) / SGR_TILE;
  a.ntiles = a.tiles_x * ((height + SGR_TILE - 1) / SGR_TILE);
  a.rgba = rgba; a.depth = depth; a.segid = segid;
  if (!rgba && !depth && !segid) return SG_OK;
  if ((long long)a.ntiles * n_ids > 0x7fffffffll) return fail(SG_ERR_INVALID, f + "too many tiles x envs for one launch");
  if (skin) hipLaunchKernelGGL(sg_rskin_kernel, dim3((unsigned)(a.ntiles * n_ids)), dim3(256), 0, r.s, A);
  else hipLaunchKernelGGL(sg_render_kernel, dim3((unsigned)(a.ntiles * n_ids)), dim3(256), 0, r.s, a);
  HIPCHK(hipGetLastError());
  return SG_OK;
}

extern "C" {

int sg_model_default_camera(const sg_model* m, double* cam) {
  if (!m || !cam) return fail(SG_ERR_INVALID, "sg_model_default_camera: null argument");
  if (!m->kin.ok) return fail(SG_ERR_MODEL, "sg_model_default_camera: " + m->kin.err);
  sgk_default_camera(m->kin, cam);
  return SG_OK;
}

int sg_get_poses(sg_batch* b, const int32_t* env_ids, int n_ids, double* xpos, double* xquat, double* geom_xpos, double* geom_xmat, void* stream) {
  if (!b) return fail(SG_ERR_INVALID, "sg_get_poses: null batch");
  Readout r{b, "sg_get_poses", (hipStream_t)stream};
  if (int rc = r.prepare(env_ids, n_ids)) return rc;
  if (!xpos && !xquat && !geom_xpos && !geom_xmat) return SG_OK;
  return r.kin(xpos, xquat, geom_xpos, geom_xmat, nullptr, nullptr);
}

int sg_render(sg_batch* b, const double* cam, const int32_t* env_ids, int n_ids, int width, int height, uint8_t* rgba, float* depth, int32_t* segid,
              void* stream) {
  return render("sg_render", false, b, cam, env_ids, n_ids, width, height, rgba, depth, segid, stream);
}

// (flags zero, or a model without a skin: the plain renderer, under its name)
int sg_render_ex(sg_batch* b, const double* cam, const int32_t* env_ids, int n_ids, int width, int height, int flags, uint8_t* rgba, float* depth,
                 int32_t* segid, void* stream) {
  if (flags & ~SG_RENDER_SKIN) return fail(SG_ERR_INVALID, "sg_render_ex: unknown flag bits");
  if (!b || !cam) return fail(SG_ERR_INVALID, "sg_render_ex: null batch or camera");
  const bool skin = (flags & SG_RENDER_SKIN) && b->m->skin.nvert != 0;
  return render(skin ? "sg_render_ex" : "sg_render", skin, b, cam, env_ids, n_ids, width, height, rgba, depth, segid, stream);
}

// ---- the skin (sg_skin.h) ----
int sg_model_set_skin(sg_model* m, int nvert, const int32_t* vert_body, const double* vert_pos, int nface, const int32_t* face, const float* rgba) {
  if (!m) return fail(SG_ERR_INVALID, "sg_model_set_skin: null model");
  if (nvert < 0 || nface < 0) return fail(SG_ERR_INVALID, "sg_model_set_skin: negative count");
  if (nvert == 0) {   // removes the skin
    m->skin.nvert = m->skin.nface = 0;
    m->skin.vert_body.clear(); m->skin.vert_pos.clear(); m->skin.face.clear();
    m->skin.version++;
    return SG_OK;
  }
  if (!m->kin.ok) return fail(SG_ERR_MODEL, "sg_model_set_skin: " + m->kin.err);
  if (nvert > SGR_MAXVERT || nface > SGR_MAXFACE)
    return fail(SG_ERR_MODEL, "sg_model_set_skin: more than " + std::to_string(SGR_MAXVERT) + " vertices or " + std::to_string(SGR_MAXFACE) + " faces");
  if (!vert_body || !vert_pos || !rgba || (nface > 0 && !face)) return fail(SG_ERR_INVALID, "sg_model_set_skin: null array with a positive count");
  for (int v = 0; v < nvert; v++) {
    if (vert_body[v] < 0 || vert_body[v] >= m->kin.o.nbody)
      return fail(SG_ERR_INVALID, "sg_model_set_skin: vertex " + std::to_string(v) + " is bound to body " + std::to_string(vert_body[v]) + ", outside [0, nbody)");
    for (int c = 0; c < 3; c++)
      if (!std::isfinite(vert_pos[3 * v + c])) return fail(SG_ERR_INVALID, "sg_model_set_skin: vertex positions must be finite");
  }
  for (int f = 0; f < nface; f++) {
    const int32_t* q = face + 3 * f;
    for (int c = 0; c < 3; c++)
      if (q[c] < 0 || q[c] >= nvert) return fail(SG_ERR_INVALID, "sg_model_set_skin: face " + std::to_string(f) + " has a vertex index outside [0, nvert)");
    if (q[0] == q[1] || q[1] == q[2] || q[0] == q[2]) return fail(SG_ERR_INVALID, "sg_model_set_skin: face " + std::to_string(f) + " repeats a vertex");
  }
  for (int c = 0; c < 4; c++)
    if (!std::isfinite(rgba[c])) return fail(SG_ERR_INVALID, "sg_model_set_skin: rgba must be finite");
  SgSkinHost& S = m->skin;
  S.nvert = nvert; S.nface = nface;
  S.vert_body.assign(vert_body, vert_body + nvert);
  S.vert_pos.assign(vert_pos, vert_pos + 3 * (size_t)nvert);
  S.face.assign(face, face + 3 * (size_t)nface);
  for (int c = 0; c < 4; c++) S.rgba[c] = rgba[c];
  S.version++;
  return SG_OK;
}

int sg_model_skin(const sg_model* m, int* nvert, int* nface, int32_t* vert_body, double* vert_pos, int32_t* face, float* rgba) {
  if (!m) return fail(SG_ERR_INVALID, "sg_model_skin: null model");
  const SgSkinHost& S = m->skin;
  if (nvert) *nvert = S.nvert;
  if (nface) *nface = S.nface;
  if (vert_body) std::copy(S.vert_body.begin(), S.vert_body.end(), vert_body);
  if (vert_pos) std::copy(S.vert_pos.begin(), S.vert_pos.end(), vert_pos);
  if (face) std::copy(S.face.begin(), S.face.end(), face);
  if (rgba)
    for (int c = 0; c < 4; c++) rgba[c] = S.rgba[c];
  return SG_OK;
}

// ---- contact read-out ----
int sg_model_ncollision_pairs(const sg_model* m) {
  if (!m) return 0;
  if (!m->con.ok) return fail(SG_ERR_MODEL, "sg_model_ncollision_pairs: " + m->con.err);
  return (int)(m->con.pairs.size() / 2);
}

int sg_get_contacts(sg_batch* b, const int32_t* env_ids, int n_ids, int max_contacts, int32_t* ncon, int32_t* geom, double* dist, double* pos,
                    double* frame, void* stream) {
  // (argument checks first, in an order that lets each be reached without a device)
  if (n_ids <= 0) return fail(SG_ERR_INVALID, "sg_get_contacts: n_ids must be positive");
  if (max_contacts <= 0 && (geom || dist || pos || frame)) return fail(SG_ERR_INVALID, "sg_get_contacts: max_contacts must be positive when a contact array is given");
  if (!b) return fail(SG_ERR_INVALID, "sg_get_contacts: null batch");
  const SgConHost& Cn = b->m->con;
  const SgKinHost& K = b->m->kin;
  if (K.ok && !Cn.ok) return fail(SG_ERR_MODEL, "sg_get_contacts: " + Cn.err);
  Readout r{b, "sg_get_contacts", (hipStream_t)stream};
  if (int rc = r.prepare(env_ids, n_ids)) return rc;
  if (!ncon && !geom && !dist && !pos && !frame) return SG_OK;
  if (!b->con_pairs) {   // (on the side, as the pose tables)
    SgArena A;
    int* dp = nullptr;
    double* dg = nullptr;
    if (!(A.upload(&dp, Cn.pairs) && A.upload(&dg, Cn.gaux))) return devmem_fail(A.nomem, "sg_get_contacts (pair tables)");
    A.give_to(b->mem);
    b->con_pairs = dp; b->con_gaux = dg;
  }
  const size_t npose = sgc_pose_doubles(K.o);
  const size_t lds = sizeof(double) * (SGC_FIXED_DBL + npose);
  const bool in_lds = lds <= 159 * 1024;   // (the kernel has 256 B of static LDS besides; the CU has 160 KB)
  if (!in_lds)
    if (int rc = r.reserve(b->con_scratch, (size_t)n_ids * npose, "pose blocks")) return rc;
  if (in_lds && !b->con_attr_set) {   // per device, as the solver kernels' attribute; what this model's launches ask for (above 64 KB it must be granted)
    HIPCHK(hipFuncSetAttribute((const void*)sg_contacts_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    b->con_attr_set = true;
  }
  SgConArgs a;
  a.D = b->kin_d; a.I = b->kin_i; a.o = K.o; a.gaux = b->con_gaux; a.pairs = b->con_pairs; a.npair = (int)(Cn.pairs.size() / 2); a.cap = Cn.cap;
  a.qpos = b->qpos; a.env_ids = r.dids; a.n_ids = n_ids; a.max_contacts = max_contacts;
  a.ncon = ncon; a.geom = geom; a.dist = dist; a.pos = pos; a.frame = frame; a.scratch = in_lds ? nullptr : b->con_scratch.p;
  if (in_lds) hipLaunchKernelGGL(sg_contacts_kernel<true>, dim3(n_ids), dim3(64), lds, r.s, a);
  else hipLaunchKernelGGL(sg_contacts_kernel<false>, dim3(n_ids), dim3(64), sizeof(double) * SGC_FIXED_DBL, r.s, a);
  HIPCHK(hipGetLastError());
  return SG_OK;
}

// ---- ray queries ----
// Which layout a call gets: lanes over geoms below SG_RAY_CROSSOVER rays per env, lane per ray from there on.  Measured (DESIGN.md 8.3,
// profiles/r08_ray_bench.json; 4096 envs, softbox): lanes over geoms wins at 16 rays per env (0.18 against 0.33 ms) and loses at 64 (0.55
// against 0.40 ms); the two lines cross near 34.  SG_RAY_LAYOUT=rays|geoms, read per call, forces one (the tests run both at every shape).
// With SG_RAY_SKIN on a model that has a skin the siblings of sg_ray_skin_kernels.h run: sg_kin_kernel, the vertex kernel, one
// of the two layouts, chosen by the same constant.
#define SG_RAY_CROSSOVER 32
int sg_ray(sg_batch* b, const int32_t* env_ids, int n_ids, int n_rays, const double* origin, const double* dir, const int32_t* ray_body,
           const int32_t* ray_exclude, int cat_mask, double max_dist, int flags, double* dist, int32_t* geomid, double* normal, void* stream) {
  // (argument checks first, in an order that lets most be reached without a device)
  if (n_ids <= 0 || n_rays <= 0) return fail(SG_ERR_INVALID, "sg_ray: n_ids and n_rays must be positive");
  if (cat_mask < 1 || cat_mask > SG_RAY_ALL) return fail(SG_ERR_INVALID, "sg_ray: cat_mask outside [1, 31]");
  if (flags & ~(SG_RAY_PER_ENV | SG_RAY_SKIN)) return fail(SG_ERR_INVALID, "sg_ray: unknown flag bits");
  if (!std::isfinite(max_dist)) return fail(SG_ERR_INVALID, "sg_ray: max_dist must be finite (<= 0: unlimited)");
  if (!b || !origin || !dir) return fail(SG_ERR_INVALID, "sg_ray: null batch, origin or dir");
  const SgKinHost& K = b->m->kin;
  if (K.ok)
    for (const int32_t* ids : {ray_body, ray_exclude})
      for (int r = 0; ids && r < n_rays; r++)
        if (ids[r] < -1 || ids[r] >= K.o.nbody)
          return fail(SG_ERR_INVALID, "sg_ray: body id " + std::to_string(ids[r]) + " of ray " + std::to_string(r) + " outside [-1, " + std::to_string(K.o.nbody) + ")");
  if (K.ok && K.bad_type >= 0)
    return fail(SG_ERR_MODEL, "sg_ray: geom type " + std::to_string(K.bad_type) + " has no ray intersection (plane, sphere, capsule and box only)");
  if (K.ok && K.o.ngeom > SGY_MAXGEOM) return fail(SG_ERR_MODEL, "sg_ray: more than " + std::to_string(SGY_MAXGEOM) + " geoms");
  if ((long long)n_ids * n_rays > 0x7fffffffll) return fail(SG_ERR_INVALID, "sg_ray: too many envs x rays for one launch");
  const bool skin = (flags & SG_RAY_SKIN) && b->m->skin.nvert != 0;   // (a model without a skin: the plain call)
  Readout r{b, "sg_ray", (hipStream_t)stream};
  if (int rc = r.prepare(env_ids, n_ids)) return rc;
  if (!dist && !geomid && !normal) return SG_OK;
  const size_t nb = K.o.nbody, ng = K.o.ngeom;
  if (skin) {
    if (int rc = skin_prepare(b, "sg_ray")) return rc;
    if (int rc = r.reserve(b->ray_vtx, (size_t)n_ids * b->skin_dev.nvert * 3, "skin vertices")) return rc;
  }
  if (int rc = r.reserve(b->ray_xpos, (size_t)n_ids * nb * 3, "body poses")) return rc;
  if (int rc = r.reserve(b->ray_xquat, (size_t)n_ids * nb * 4, "body poses")) return rc;
  if (int rc = r.reserve(b->ray_gxpos, (size_t)n_ids * (ng ? ng : 1) * 3, "geom poses")) return rc;
  if (int rc = r.reserve(b->ray_gxmat, (size_t)n_ids * (ng ? ng : 1) * 9, "geom poses")) return rc;
  if (int rc = r.reserve(b->ray_ids, 2 * (size_t)n_rays, "ray body ids")) return rc;
  if (ray_body) HIPCHK(hipMemcpyAsync(b->ray_ids.p, ray_body, sizeof(int) * n_rays, hipMemcpyHostToDevice, r.s));
  if (ray_exclude) HIPCHK(hipMemcpyAsync(b->ray_ids.p + n_rays, ray_exclude, sizeof(int) * n_rays, hipMemcpyHostToDevice, r.s));
  if (int rc = r.kin(b->ray_xpos.p, b->ray_xquat.p, b->ray_gxpos.p, b->ray_gxmat.p, nullptr, nullptr)) return rc;
  SgRayArgs a;
  a.D = b->kin_d; a.I = b->kin_i; a.gsize = K.o.gsize; a.gmeta = K.o.gmeta; a.gbody = K.o.gbody; a.ngeom = K.o.ngeom; a.nbody = K.o.nbody;
  a.xpos = b->ray_xpos.p; a.xquat = b->ray_xquat.p; a.gxpos = b->ray_gxpos.p; a.gxmat = b->ray_gxmat.p;
  a.origin = origin; a.dir = dir;
  a.ray_body = ray_body ? b->ray_ids.p : nullptr; a.ray_exclude = ray_exclude ? b->ray_ids.p + n_rays : nullptr;
  a.n_ids = n_ids; a.n_rays = n_rays; a.per_env = (flags & SG_RAY_PER_ENV) ? 1 : 0; a.cat_mask = cat_mask;
  a.limit = max_dist > 0 ? max_dist : INFINITY;
  a.dist = dist; a.geomid = geomid; a.normal = normal;
  bool by_geoms = n_rays < SG_RAY_CROSSOVER;
  if (const char* forced = getenv("SG_RAY_LAYOUT")) {
    if (!strcmp(forced, "rays")) by_geoms = false;
    else if (!strcmp(forced, "geoms")) by_geoms = true;
    else if (*forced) return fail(SG_ERR_INVALID, "sg_ray: SG_RAY_LAYOUT must be rays or geoms");
  }
  if (skin) {
    const SgSkinDev& S = b->skin_dev;
    SgSkinRayVertArgs V;
    V.vert_body = S.vert_body; V.vert_pos = S.vert_pos; V.xpos = a.xpos; V.xquat = a.xquat; V.nvert = S.nvert; V.nbody = K.o.nbody; V.vtx = b->ray_vtx.p;
    hipLaunchKernelGGL(sg_skinray_vert_kernel, dim3(n_ids), dim3(256), 0, r.s, V);
    HIPCHK(hipGetLastError());
    SgSkinRayArgs A;
    A.r = a; A.vtx = b->ray_vtx.p; A.faces = S.faces; A.vert_body = S.vert_body; A.hidden = S.hidden; A.vis = b->skin_vis;
    A.nvert = S.nvert; A.nface = S.nface; A.nvis = b->skin_nvis;
    if (by_geoms) {
      hipLaunchKernelGGL(sg_skinray_geoms_kernel, dim3((unsigned)((long long)n_ids * n_rays)), dim3(64), 0, r.s, A);
    } else {
      const int nblk = (n_rays + 255) / 256;
      hipLaunchKernelGGL(sg_skinray_rays_kernel, dim3((unsigned)((long long)n_ids * nblk)), dim3(256), sg_skinray_lds(A.nvis, A.nvert, A.nface), r.s, A, nblk);
    }
  } else if (by_geoms) {
    hipLaunchKernelGGL(sg_ray_geoms_kernel, dim3((unsigned)((long long)n_ids * n_rays)), dim3(64), 0, r.s, a);
  } else {
    const int nblk = (n_rays + 255) / 256;
    hipLaunchKernelGGL(sg_ray_rays_kernel, dim3((unsigned)((long long)n_ids * nblk)), dim3(256), sizeof(double) * SGY_REC * (ng ? ng : 1), r.s, a, nblk);
  }
  HIPCHK(hipGetLastError());
  return SG_OK;
}

// ---- velocity, tendon and energy read-outs: one walk (sg_dyn_kernel), whichever outputs the entry point fn passes ----
static int dyn(const char* fn, sg_batch* b, const int32_t* env_ids, int n_ids, double* ang, double* lin, double* com_lin, double* ten_len, double* ten_vel,
               double* energy, void* stream) {
  // (argument checks first, in an order that lets each be reached without a device)
  if (n_ids <= 0) return fail(SG_ERR_INVALID, std::string(fn) + ": n_ids must be positive");
  if (!b) return fail(SG_ERR_INVALID, std::string(fn) + ": null batch");
  const SgKinHost& K = b->m->kin;
  const SgDynHost& Dn = b->m->dyn;
  const SgPlanHeader& H = b->m->plan.h;
  if (K.ok && !Dn.ok) return fail(SG_ERR_MODEL, std::string(fn) + ": " + Dn.err);
  if (K.ok && (Dn.o.nv != H.nv || K.o.nq != H.nq || K.o.njnt != H.njnt || Dn.o.ntendon != H.ntendon))   // (the strides of qpos / qvel and the masks' lengths)
    return fail(SG_ERR_MODEL, std::string(fn) + ": the blob's joint, dof or tendon counts differ from the plan's");
  Readout r{b, fn, (hipStream_t)stream};
  if (int rc = r.prepare(env_ids, n_ids)) return rc;
  if (!ang && !lin && !com_lin && !ten_len && !ten_vel && !energy) return SG_OK;
  if (!b->dyn_d) {   // (on the side, as the pose tables)
    SgArena A;
    double* dd = nullptr;
    int* di = nullptr;
    if (!(A.upload(&dd, Dn.dbl) && A.upload(&di, Dn.ints))) return devmem_fail(A.nomem, std::string(fn) + " (dynamics tables)");
    A.give_to(b->mem);
    b->dyn_d = dd; b->dyn_i = di;
  }
  SgDynArgs a;
  a.D = b->kin_d; a.I = b->kin_i; a.o = K.o; a.DD = b->dyn_d; a.DI = b->dyn_i; a.d = Dn.o;
  a.qpos = b->qpos; a.qvel = b->qvel; a.kenv = b->kenv; a.kmask_jnt = b->kmask_jnt; a.kmask_ten = b->kmask_ten;
  a.env_ids = r.dids; a.n_ids = n_ids;
  a.ang = ang; a.lin = lin; a.com_lin = com_lin; a.ten_len = ten_len; a.ten_vel = ten_vel; a.energy = energy;
  hipLaunchKernelGGL(sg_dyn_kernel, dim3(n_ids), dim3(64), sizeof(double) * SGD_REC * K.o.nbody, r.s, a);   // (<= 64 KB: SGD_MAXBODY)
  HIPCHK(hipGetLastError());
  return SG_OK;
}

int sg_get_velocities(sg_batch* b, const int32_t* env_ids, int n_ids, double* ang, double* lin, double* com_lin, void* stream) {
  return dyn("sg_get_velocities", b, env_ids, n_ids, ang, lin, com_lin, nullptr, nullptr, nullptr, stream);
}
int sg_get_tendons(sg_batch* b, const int32_t* env_ids, int n_ids, double* length, double* velocity, void* stream) {
  return dyn("sg_get_tendons", b, env_ids, n_ids, nullptr, nullptr, nullptr, length, velocity, nullptr, stream);
}
int sg_get_energy(sg_batch* b, const int32_t* env_ids, int n_ids, double* energy, void* stream) {
  return dyn("sg_get_energy", b, env_ids, n_ids, nullptr, nullptr, nullptr, nullptr, nullptr, energy, stream);
}

// ---- mass matrix, joint forces and inverse dynamics: one kernel (sg_smooth_kernel), whichever outputs the entry point fn passes ----
static int smooth(const char* fn, sg_batch* b, const int32_t* env_ids, int n_ids, double* M, double* bias, double* passive, double* actuator,
                  const double* qacc, bool need_qacc, double* inverse, void* stream) {
  // (argument checks first, in an order that lets each be reached without a device)
  if (n_ids <= 0) return fail(SG_ERR_INVALID, std::string(fn) + ": n_ids must be positive");
  if (!b) return fail(SG_ERR_INVALID, std::string(fn) + ": null batch");
  if (need_qacc && !qacc) return fail(SG_ERR_INVALID, std::string(fn) + ": null qacc");
  const SgKinHost& K = b->m->kin;
  const SgDynHost& Dn = b->m->dyn;
  const SgSmoothHost& Sm = b->m->smooth;
  const SgPlanHeader& H = b->m->plan.h;
  if (K.ok && !Sm.ok) return fail(SG_ERR_MODEL, std::string(fn) + ": " + Sm.err);
  if (K.ok && (Dn.o.nv != H.nv || K.o.nq != H.nq || K.o.njnt != H.njnt || Dn.o.ntendon != H.ntendon || Sm.o.nu != H.nu))   // (the strides of qpos / qvel / act and the masks' lengths)
    return fail(SG_ERR_MODEL, std::string(fn) + ": the blob's joint, dof, tendon or actuator counts differ from the plan's");
  Readout r{b, fn, (hipStream_t)stream};
  if (int rc = r.prepare(env_ids, n_ids)) return rc;
  if (!M && !bias && !passive && !actuator && !inverse) return SG_OK;
  if (!b->dyn_d) {   // (on the side, as the pose tables)
    SgArena A;
    double* dd = nullptr;
    int* di = nullptr;
    if (!(A.upload(&dd, Dn.dbl) && A.upload(&di, Dn.ints))) return devmem_fail(A.nomem, std::string(fn) + " (dynamics tables)");
    A.give_to(b->mem);
    b->dyn_d = dd; b->dyn_i = di;
  }
  if (!b->smooth_d) {
    SgArena A;
    double* sd = nullptr;
    int* si = nullptr;
    if (!(A.upload(&sd, Sm.dbl) && A.upload(&si, Sm.ints))) return devmem_fail(A.nomem, std::string(fn) + " (smooth tables)");
    A.give_to(b->mem);
    b->smooth_d = sd; b->smooth_i = si;
  }
  // nbody <= SGS_MAXBODY, nv <= SGS_MAXDOF, ntendon <= SGS_MAXTENDON (sgs_build): with the kernel's static LDS within SGS_LDS_MAX
  const size_t lds = sizeof(double) * ((size_t)SGS_REC * K.o.nbody + (size_t)SGS_DOF * Dn.o.nv + 2 * (size_t)Dn.o.ntendon);
  if (!b->smooth_attr_set) {   // per device, as the contact read-out's attribute: above 64 KB the launch's dynamic LDS must be granted
    HIPCHK(hipFuncSetAttribute((const void*)sg_smooth_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, SGS_LDS_MAX - SGS_STATIC_LDS));
    b->smooth_attr_set = true;
  }
  SgSmoothArgs a;
  a.D = b->kin_d; a.I = b->kin_i; a.o = K.o; a.DD = b->dyn_d; a.DI = b->dyn_i; a.d = Dn.o; a.SD = b->smooth_d; a.SI = b->smooth_i; a.s = Sm.o;
  a.qpos = b->qpos; a.qvel = b->qvel; a.act = b->act; a.kenv = b->kenv; a.kmask_jnt = b->kmask_jnt; a.kmask_ten = b->kmask_ten;
  a.env_ids = r.dids; a.n_ids = n_ids;
  a.M = M; a.bias = bias; a.passive = passive; a.actuator = actuator; a.qacc = qacc; a.inverse = inverse;
  hipLaunchKernelGGL(sg_smooth_kernel, dim3(n_ids), dim3(64), lds, r.s, a);
  HIPCHK(hipGetLastError());
  return SG_OK;
}

int sg_get_mass_matrix(sg_batch* b, const int32_t* env_ids, int n_ids, double* M, void* stream) {
  return smooth("sg_get_mass_matrix", b, env_ids, n_ids, M, nullptr, nullptr, nullptr, nullptr, false, nullptr, stream);
}
int sg_get_joint_forces(sg_batch* b, const int32_t* env_ids, int n_ids, double* bias, double* passive, double* actuator, void* stream) {
  return smooth("sg_get_joint_forces", b, env_ids, n_ids, nullptr, bias, passive, actuator, nullptr, false, nullptr, stream);
}
int sg_inverse_dynamics(sg_batch* b, const int32_t* env_ids, int n_ids, const double* qacc, double* qfrc_inverse, void* stream) {
  return smooth("sg_inverse_dynamics", b, env_ids, n_ids, nullptr, nullptr, nullptr, nullptr, qacc, true, qfrc_inverse, stream);
}

// ---- point motion and point Jacobians: one kernel (sg_point_kernel), whichever outputs the entry point fn passes ----
static int point(const char* fn, sg_batch* b, const int32_t* env_ids, int n_ids, int n_pts, const int32_t* pt_body, const double* pt_pos, const double* pt_quat,
                 const double* qpos, const double* qvel, const double* qacc, double* pos, double* mat, double* vel, double* acc, double* gyro, double* accel,
                 double* jacp, double* jacr, bool use_qvel, void* stream) {
  // (argument checks first, in an order that lets each be reached without a device)
  const std::string f = std::string(fn) + ": ";
  if (n_ids <= 0) return fail(SG_ERR_INVALID, f + "n_ids must be positive");
  if (n_pts <= 0) return fail(SG_ERR_INVALID, f + "n_pts must be positive");
  if (!b) return fail(SG_ERR_INVALID, f + "null batch");
  if (!pt_body || !pt_pos) return fail(SG_ERR_INVALID, f + "null pt_body or pt_pos");
  const SgKinHost& K = b->m->kin;
  const SgDynHost& Dn = b->m->dyn;
  const SgPointHost& Pt = b->m->point;
  const SgPlanHeader& H = b->m->plan.h;
  for (int p = 0; p < n_pts; p++) {
    if (K.ok && (pt_body[p] < 0 || pt_body[p] >= K.o.nbody))
      return fail(SG_ERR_INVALID, f + "body id " + std::to_string(pt_body[p]) + " of point " + std::to_string(p) + " outside [0, " + std::to_string(K.o.nbody) + ")");
    for (int c = 0; c < 3; c++)
      if (!std::isfinite(pt_pos[3 * p + c])) return fail(SG_ERR_INVALID, f + "pt_pos of point " + std::to_string(p) + " is not finite");
    if (pt_quat) {
      double n2 = 0.0;
      for (int c = 0; c < 4; c++) {
        if (!std::isfinite(pt_quat[4 * p + c])) return fail(SG_ERR_INVALID, f + "pt_quat of point " + std::to_string(p) + " is not finite");
        n2 += pt_quat[4 * p + c] * pt_quat[4 * p + c];
      }
      if (!(n2 > 0.0) || !std::isfinite(n2)) return fail(SG_ERR_INVALID, f + "pt_quat of point " + std::to_string(p) + " has zero length (or overflows)");
    }
  }
  if (K.ok && !Pt.ok) return fail(SG_ERR_MODEL, f + Pt.err);
  if (K.ok && (Dn.o.nv != H.nv || K.o.nq != H.nq))   // (the strides of qpos / qvel)
    return fail(SG_ERR_MODEL, f + "the blob's position or dof counts differ from the plan's");
  if ((long long)n_ids * n_pts > 0x7fffffffll) return fail(SG_ERR_INVALID, f + "too many envs x points for one launch");
  Readout r{b, fn, (hipStream_t)stream};
  if (int rc = r.prepare(env_ids, n_ids)) return rc;
  if (!pos && !mat && !vel && !acc && !gyro && !accel && !jacp && !jacr) return SG_OK;
  if (!b->dyn_d) {   // (on the side, as the pose tables)
    SgArena A;
    double* dd = nullptr;
    int* di = nullptr;
    if (!(A.upload(&dd, Dn.dbl) && A.upload(&di, Dn.ints))) return devmem_fail(A.nomem, std::string(fn) + " (dynamics tables)");
    A.give_to(b->mem);
    b->dyn_d = dd; b->dyn_i = di;
  }
  if (!b->point_i) {   // the point table, and a row of nv zeros: the qvel the Jacobian-only call walks at
    SgArena A;
    int* pi = nullptr;
    double* z = nullptr;
    if (!(A.upload(&pi, Pt.ints) && A.upload(&z, std::vector<double>(Dn.o.nv > 0 ? Dn.o.nv : 1, 0.0)))) return devmem_fail(A.nomem, std::string(fn) + " (point table)");
    A.give_to(b->mem);
    b->point_i = pi; b->point_zero = z;
  }
  // nbody <= SGP_MAXBODY, nv <= SGP_MAXDOF (sgp_build): with the kernel's static LDS within SGP_LDS_MAX
  const size_t lds = sizeof(double) * ((size_t)SGP_REC * K.o.nbody + (size_t)SGP_DOF * Dn.o.nv) + sizeof(int) * (size_t)Dn.o.nv;
  if (!b->point_attr_set) {   // per device, as the smooth read-out's attribute: above 64 KB the launch's dynamic LDS must be granted
    HIPCHK(hipFuncSetAttribute((const void*)sg_point_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, SGP_LDS_MAX - SGP_STATIC_LDS));
    b->point_attr_set = true;
  }
  // the points: host arrays, read here and copied on the stream
  if (int rc = r.reserve(b->pt_ids, (size_t)n_pts, "point body ids")) return rc;
  if (int rc = r.reserve(b->pt_d, 7 * (size_t)n_pts, "points")) return rc;
  HIPCHK(hipMemcpyAsync(b->pt_ids.p, pt_body, sizeof(int) * n_pts, hipMemcpyHostToDevice, r.s));
  HIPCHK(hipMemcpyAsync(b->pt_d.p, pt_pos, sizeof(double) * 3 * n_pts, hipMemcpyHostToDevice, r.s));
  if (pt_quat) HIPCHK(hipMemcpyAsync(b->pt_d.p + 3 * (size_t)n_pts, pt_quat, sizeof(double) * 4 * n_pts, hipMemcpyHostToDevice, r.s));
  SgPointArgs a;
  a.D = b->kin_d; a.I = b->kin_i; a.o = K.o; a.DD = b->dyn_d; a.DI = b->dyn_i; a.d = Dn.o; a.PI = b->point_i; a.p = Pt.o;
  a.qpos = qpos ? qpos : b->qpos; a.qvel = !use_qvel ? b->point_zero : qvel ? qvel : b->qvel; a.qacc = qacc;
  a.given = (qpos ? 1 : 0) | (use_qvel ? (qvel ? 2 : 0) : 4);
  a.env_ids = r.dids; a.n_ids = n_ids; a.n_pts = n_pts;
  a.pt_body = b->pt_ids.p; a.pt_pos = b->pt_d.p; a.pt_quat = pt_quat ? b->pt_d.p + 3 * (size_t)n_pts : nullptr;
  a.pos = pos; a.mat = mat; a.vel = vel; a.acc = acc; a.gyro = gyro; a.accel = accel; a.jacp = jacp; a.jacr = jacr;
  hipLaunchKernelGGL(sg_point_kernel, dim3(n_ids), dim3(64), lds, r.s, a);
  HIPCHK(hipGetLastError());
  return SG_OK;
}

int sg_get_point_motion(sg_batch* b, const int32_t* env_ids, int n_ids, int n_pts, const int32_t* pt_body, const double* pt_pos, const double* pt_quat,
                        const double* qpos, const double* qvel, const double* qacc, double* pos, double* mat, double* vel, double* acc, double* gyro,
                        double* accel, void* stream) {
  return point("sg_get_point_motion", b, env_ids, n_ids, n_pts, pt_body, pt_pos, pt_quat, qpos, qvel, qacc, pos, mat, vel, acc, gyro, accel, nullptr, nullptr, true, stream);
}
int sg_get_jacobians(sg_batch* b, const int32_t* env_ids, int n_ids, int n_pts, const int32_t* pt_body, const double* pt_pos, const double* qpos, double* jacp,
                     double* jacr, void* stream) {
  return point("sg_get_jacobians", b, env_ids, n_ids, n_pts, pt_body, pt_pos, nullptr, qpos, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
               jacp, jacr, false, stream);
}

// ---- mass-matrix solves, smooth forward dynamics and point inertias: one kernel (sg_solve_kernel), in the mode of the entry point fn ----
static int solve(const char* fn, int mode, sg_batch* b, const int32_t* env_ids, int n_ids, int n_rhs, const double* y, double* x, const double* applied,
                 double* qacc, double* qfrc, const int32_t* pt_body, const double* pt_pos, double* W, double* pivot, void* stream) {
  // (argument checks first, in an order that lets each be reached without a device)
  const std::string f = std::string(fn) + ": ";
  if (n_ids <= 0) return fail(SG_ERR_INVALID, f + "n_ids must be positive");
  if (mode == SGV_MODE_SOLVE && n_rhs <= 0) return fail(SG_ERR_INVALID, f + "n_rhs must be positive");
  if (mode == SGV_MODE_POINT && n_rhs <= 0) return fail(SG_ERR_INVALID, f + "n_pts must be positive");
  if (!b) return fail(SG_ERR_INVALID, f + "null batch");
  if (mode == SGV_MODE_SOLVE && !y) return fail(SG_ERR_INVALID, f + "null y");
  if (mode == SGV_MODE_SOLVE && !x && !pivot) return fail(SG_ERR_INVALID, f + "x and pivot are both null");
  if (mode == SGV_MODE_POINT && (!pt_body || !pt_pos)) return fail(SG_ERR_INVALID, f + "null pt_body or pt_pos");
  const SgKinHost& K = b->m->kin;
  const SgDynHost& Dn = b->m->dyn;
  const SgSmoothHost& Sm = b->m->smooth;
  const SgSolveHost& Sv = b->m->solve;
  const SgPlanHeader& H = b->m->plan.h;
  if (mode == SGV_MODE_POINT)
    for (int p = 0; p < n_rhs; p++) {
      if (K.ok && (pt_body[p] < 0 || pt_body[p] >= K.o.nbody))
        return fail(SG_ERR_INVALID, f + "body id " + std::to_string(pt_body[p]) + " of point " + std::to_string(p) + " outside [0, " + std::to_string(K.o.nbody) + ")");
      for (int c = 0; c < 3; c++)
        if (!std::isfinite(pt_pos[3 * p + c])) return fail(SG_ERR_INVALID, f + "pt_pos of point " + std::to_string(p) + " is not finite");
    }
  if (K.ok && !Sv.ok) return fail(SG_ERR_MODEL, f + Sv.err);
  if (K.ok && (Dn.o.nv != H.nv || K.o.nq != H.nq || K.o.njnt != H.njnt || Dn.o.ntendon != H.ntendon || Sm.o.nu != H.nu))   // (the strides of qpos / qvel / act and the masks' lengths)
    return fail(SG_ERR_MODEL, f + "the blob's joint, dof, tendon or actuator counts differ from the plan's");
  if ((long long)n_ids * n_rhs > 0x7fffffffll / 36) return fail(SG_ERR_INVALID, f + "too many envs x right-hand sides or points for one launch");
  Readout r{b, fn, (hipStream_t)stream};
  if (int rc = r.prepare(env_ids, n_ids)) return rc;
  if (!x && !qacc && !qfrc && !W && !pivot) return SG_OK;
  if (!b->dyn_d) {   // (on the side, as the pose tables)
    SgArena A;
    double* dd = nullptr;
    int* di = nullptr;
    if (!(A.upload(&dd, Dn.dbl) && A.upload(&di, Dn.ints))) return devmem_fail(A.nomem, std::string(fn) + " (dynamics tables)");
    A.give_to(b->mem);
    b->dyn_d = dd; b->dyn_i = di;
  }
  if (!b->smooth_d) {
    SgArena A;
    double* sd = nullptr;
    int* si = nullptr;
    if (!(A.upload(&sd, Sm.dbl) && A.upload(&si, Sm.ints))) return devmem_fail(A.nomem, std::string(fn) + " (smooth tables)");
    A.give_to(b->mem);
    b->smooth_d = sd; b->smooth_i = si;
  }
  if (!b->solve_i) {   // the solve table, and a row of nv zeros: the qvel the calls that need M alone walk at
    SgArena A;
    int* vi = nullptr;
    double* z = nullptr;
    if (!(A.upload(&vi, Sv.ints) && A.upload(&z, std::vector<double>(Dn.o.nv, 0.0)))) return devmem_fail(A.nomem, std::string(fn) + " (solve table)");
    A.give_to(b->mem);
    b->solve_i = vi; b->solve_zero = z;
  }
  // a tile of SGV_MINRHS right-hand sides fits beside the fixed block (sgv_build); the launch asks for the tile it uses, no more
  const long long fixed = sgv_fixed_doubles(K.o.nbody, Dn.o.nv, Dn.o.ntendon, Sv.o.nM), room = sgv_tile(K.o.nbody, Dn.o.nv, Dn.o.ntendon, Sv.o.nM);
  const int tile = mode == SGV_MODE_FORWARD ? 1 : (int)std::min<long long>(n_rhs, mode == SGV_MODE_POINT ? room / 6 : room);
  const size_t lds = sizeof(double) * ((size_t)fixed + (size_t)tile * (mode == SGV_MODE_POINT ? 6 : 1) * Dn.o.nv);
  if (!b->solve_attr_set) {   // per device, as the smooth read-out's attribute: above 64 KB the launch's dynamic LDS must be granted
    HIPCHK(hipFuncSetAttribute((const void*)sg_solve_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, SGV_LDS_MAX - SGV_STATIC_LDS));
    b->solve_attr_set = true;
  }
  if (mode == SGV_MODE_POINT) {   // the points: host arrays, read here and copied on the stream
    if (int rc = r.reserve(b->sv_ids, (size_t)n_rhs, "point body ids")) return rc;
    if (int rc = r.reserve(b->sv_pos, 3 * (size_t)n_rhs, "points")) return rc;
    HIPCHK(hipMemcpyAsync(b->sv_ids.p, pt_body, sizeof(int) * n_rhs, hipMemcpyHostToDevice, r.s));
    HIPCHK(hipMemcpyAsync(b->sv_pos.p, pt_pos, sizeof(double) * 3 * n_rhs, hipMemcpyHostToDevice, r.s));
  }
  SgSolveArgs a;
  a.D = b->kin_d; a.I = b->kin_i; a.o = K.o; a.DD = b->dyn_d; a.DI = b->dyn_i; a.d = Dn.o; a.SD = b->smooth_d; a.SI = b->smooth_i; a.s = Sm.o;
  a.VI = b->solve_i; a.v = Sv.o;
  a.qpos = b->qpos; a.qvel = b->qvel; a.act = b->act; a.kenv = b->kenv; a.zero = b->solve_zero; a.kmask_jnt = b->kmask_jnt; a.kmask_ten = b->kmask_ten;
  a.env_ids = r.dids; a.n_ids = n_ids; a.mode = mode; a.n_rhs = mode == SGV_MODE_FORWARD ? 1 : n_rhs; a.tile = tile;
  a.y = y; a.x = x; a.applied = applied; a.qacc = qacc; a.qfrc = qfrc;
  a.pt_body = mode == SGV_MODE_POINT ? b->sv_ids.p : nullptr; a.pt_pos = mode == SGV_MODE_POINT ? b->sv_pos.p : nullptr; a.W = W; a.pivot = pivot;
  hipLaunchKernelGGL(sg_solve_kernel, dim3(n_ids), dim3(64), lds, r.s, a);
  HIPCHK(hipGetLastError());
  return SG_OK;
}

int sg_solve_mass(sg_batch* b, const int32_t* env_ids, int n_ids, int n_rhs, const double* y, double* x, double* pivot, void* stream) {
  return solve("sg_solve_mass", SGV_MODE_SOLVE, b, env_ids, n_ids, n_rhs, y, x, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, pivot, stream);
}
int sg_forward_smooth(sg_batch* b, const int32_t* env_ids, int n_ids, const double* qfrc_applied, double* qacc_smooth, double* qfrc_smooth, double* pivot,
                      void* stream) {
  return solve("sg_forward_smooth", SGV_MODE_FORWARD, b, env_ids, n_ids, 1, nullptr, nullptr, qfrc_applied, qacc_smooth, qfrc_smooth, nullptr, nullptr, nullptr,
               pivot, stream);
}
int sg_get_point_inertia(sg_batch* b, const int32_t* env_ids, int n_ids, int n_pts, const int32_t* pt_body, const double* pt_pos, double* W, double* pivot,
                         void* stream) {
  return solve("sg_get_point_inertia", SGV_MODE_POINT, b, env_ids, n_ids, n_pts, nullptr, nullptr, nullptr, nullptr, nullptr, pt_body, pt_pos, W, pivot, stream);
}

int sg_model_nsite(const sg_model* m) { return m ? (int)m->point.site_body.size() : 0; }
// the model's sites as points of the two calls above (host arrays, any may be NULL)
int sg_model_sites(const sg_model* m, int32_t* body, double* pos, double* quat) {
  if (!m) return fail(SG_ERR_INVALID, "sg_model_sites: null model");
  const SgPointHost& P = m->point;
  if (!P.ok) return fail(SG_ERR_MODEL, "sg_model_sites: " + P.err);
  if (body) std::copy(P.site_body.begin(), P.site_body.end(), body);
  if (pos) std::copy(P.site_pos.begin(), P.site_pos.end(), pos);
  if (quat) std::copy(P.site_quat.begin(), P.site_quat.end(), quat);
  return SG_OK;
}

}  // extern "C"
