// sg_readout.hip -- the read-out half of the C ABI (include/softgrip.h): sg_get_poses, sg_render / sg_render_ex and the skin,
// sg_get_contacts, sg_ray, sg_get_velocities / sg_get_tendons / sg_get_energy, sg_get_mass_matrix / sg_get_joint_forces /
// sg_inverse_dynamics, sg_get_point_motion / sg_get_jacobians, sg_solve_mass / sg_forward_smooth / sg_get_point_inertia, sg_get_forces,
// sg_get_skin_vertices / sg_get_shape / sg_get_subtree, with the kernels
// they launch (the *_kernel*.h files, whose device assembly is sg_readout.device.s).  Entry points and launches only: the host builders of
// the per-model tables are in sg_tables.cpp (sg_solve.h builds its own), what brings a table to a batch's device is SgDevTable
// (sg_devmem.h) under Readout::need_*.  None of them writes the state: every pipeline is served.  No CPU fallback.
#include <algorithm>
#include <cstring>

#include "sg_batch.h"
#include "sg_kin_kernels.h"
#include "sg_contacts_kernel.h"
#include "sg_ray_kernels.h"
#include "sg_ray_skin_kernels.h"
#include "sg_dyn_kernel.h"
#include "sg_smooth_kernel.h"
#include "sg_point_kernel.h"
#include "sg_solve_kernel.h"
#include "sg_forces_kernel.h"
#include "sg_shape_kernel.h"

// ---- the entry points' common prologue ----
// One read-out call on stream s: prepare() puts the kinematics table on the batch's device and the listed env ids (host array,
// range-checked here) in a device buffer, need_*() the further tables the call's kernel reads -- each with the tables it is built on, so a
// new read-out family declares what it needs in one line --, reserve() grows a scratch buffer of the batch, grant_lds() lets a kernel ask
// for more than 64 KB of LDS, tables_*() fill the table part of an argument struct, kin() launches sg_kin_kernel over the listed envs.
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
    if (int rc = need(b->kin, &K.dbl, &K.ints, "pose tables")) return rc;
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

  // a table on the batch's device, uploaded at its first use (on the side: the batch sees it only once every section is up)
  int need(SgDevTable& t, const std::vector<double>* dbl, const std::vector<int>* ints, const char* what) {
    return t.ensure(b->mem, dbl, ints) ? SG_OK : devmem_fail(t.nomem, std::string(fn) + " (" + what + ")");
  }
  int need_con() { return need(b->con, &b->m->con.gaux, &b->m->con.pairs, "pair tables"); }
  int need_dyn() { return need(b->dyn, &b->m->dyn.dbl, &b->m->dyn.ints, "dynamics tables"); }
  int need_smooth() {
    if (int rc = need_dyn()) return rc;
    return need(b->smooth, &b->m->smooth.dbl, &b->m->smooth.ints, "smooth tables");
  }
  // (the row of zeros counts as part of the table that asks for it)
  int need_zero(const char* what) {
    if (b->zero.d) return SG_OK;
    const std::vector<double> zeros(std::max(b->m->dyn.o.nv, 1), 0.0);
    return need(b->zero, &zeros, nullptr, what);
  }
  int need_point() {
    if (int rc = need_dyn()) return rc;
    if (int rc = need(b->point, nullptr, &b->m->point.ints, "point table")) return rc;
    return need_zero("point table");
  }
  int need_solve() {
    if (int rc = need_smooth()) return rc;
    if (int rc = need(b->solve, nullptr, &b->m->solve.ints, "solve table")) return rc;
    return need_zero("solve table");
  }

  // once per batch (so per device): a launch's dynamic LDS above 64 KB must be granted to the kernel first
  template <class Kernel>
  int grant_lds(bool& granted, Kernel kernel, size_t bytes) {
    if (granted) return SG_OK;
    HIPCHK(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    granted = true;
    return SG_OK;
  }

  // the table part of a kernel's argument struct, one level per table the struct is built on
  template <class Args>
  void tables_kin(Args& a) const { a.D = b->kin.d; a.I = b->kin.i; a.o = b->m->kin.o; }
  template <class Args>
  void tables_dyn(Args& a) const { tables_kin(a); a.DD = b->dyn.d; a.DI = b->dyn.i; a.d = b->m->dyn.o; }
  template <class Args>
  void tables_smooth(Args& a) const { tables_dyn(a); a.SD = b->smooth.d; a.SI = b->smooth.i; a.s = b->m->smooth.o; }

  // the points of a call (host arrays: body ids, positions, with quat quaternions) on the device, copied on the stream: ids holds the
  // body ids, d the positions [n][3] and, from 3 n on, the quaternions [n][4]; room: doubles of d per point
  int stage_points(SgScratch<int>& ids, SgScratch<double>& d, int room, int n, const int32_t* body, const double* pos, const double* quat) {
    if (int rc = reserve(ids, (size_t)n, "point body ids")) return rc;
    if (int rc = reserve(d, (size_t)room * n, "points")) return rc;
    HIPCHK(hipMemcpyAsync(ids.p, body, sizeof(int) * n, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d.p, pos, sizeof(double) * 3 * n, hipMemcpyHostToDevice, s));
    if (quat) HIPCHK(hipMemcpyAsync(d.p + 3 * (size_t)n, quat, sizeof(double) * 4 * n, hipMemcpyHostToDevice, s));
    return SG_OK;
  }

  int kin(double* xpos, double* xquat, double* gxpos, double* gxmat, float* recs, const double* eye) {
    const SgKinHost& K = b->m->kin;
    SgKinArgs a;
    tables_kin(a);
    a.qpos = b->qpos; a.env_ids = dids; a.n_ids = n_ids;
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

// the launch of sg_contacts_kernel over r's listed envs (sg_get_contacts; sg_get_forces for a chunk's list in its work space)
static int contacts_launch(Readout& r, int max_contacts, int32_t* ncon, int32_t* geom, double* dist, double* pos, double* frame) {
  sg_batch* b = r.b;
  const SgConHost& Cn = b->m->con;
  const SgKinHost& K = b->m->kin;
  const int n_ids = r.n_ids;
  if (int rc = r.need_con()) return rc;
  const size_t npose = sgc_pose_doubles(K.o);
  const size_t lds = sizeof(double) * (SGC_FIXED_DBL + npose);
  const bool in_lds = lds <= 159 * 1024;   // (the kernel has 256 B of static LDS besides; the CU has 160 KB)
  if (!in_lds)
    if (int rc = r.reserve(b->con_scratch, (size_t)n_ids * npose, "pose blocks")) return rc;
  if (in_lds)   // (what this model's launches ask for)
    if (int rc = r.grant_lds(b->con_attr_set, sg_contacts_kernel<true>, lds)) return rc;
  SgConArgs a;
  r.tables_kin(a);
  a.gaux = b->con.d; a.pairs = b->con.i; a.npair = (int)(Cn.pairs.size() / 2); a.cap = Cn.cap;
  a.qpos = b->qpos; a.env_ids = r.dids; a.n_ids = n_ids; a.max_contacts = max_contacts;
  a.ncon = ncon; a.geom = geom; a.dist = dist; a.pos = pos; a.frame = frame; a.scratch = in_lds ? nullptr : b->con_scratch.p;
  if (in_lds) hipLaunchKernelGGL(sg_contacts_kernel<true>, dim3(n_ids), dim3(64), lds, r.s, a);
  else hipLaunchKernelGGL(sg_contacts_kernel<false>, dim3(n_ids), dim3(64), sizeof(double) * SGC_FIXED_DBL, r.s, a);
  HIPCHK(hipGetLastError());
  return SG_OK;
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
  return contacts_launch(r, max_contacts, ncon, geom, dist, pos, frame);
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
  a.D = b->kin.d; a.I = b->kin.i; a.gsize = K.o.gsize; a.gmeta = K.o.gmeta; a.gbody = K.o.gbody; a.ngeom = K.o.ngeom; a.nbody = K.o.nbody;
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

// ---- checks the dyn, smooth, point and solve read-outs share ----
// the blob's counts against the plan header's, which the batch's state is laid out by: COUNTS_POINT the strides of qpos / qvel; COUNTS_DYN
// the masks' lengths too; COUNTS_SMOOTH the stride of act too -> what differs, in the words of that level, or NULL
enum { COUNTS_POINT, COUNTS_DYN, COUNTS_SMOOTH };
static const char* counts_differ(const sg_model* m, int level) {
  const SgPlanHeader& H = m->plan.h;
  bool differ = m->dyn.o.nv != H.nv || m->kin.o.nq != H.nq;
  if (level >= COUNTS_DYN) differ = differ || m->kin.o.njnt != H.njnt || m->dyn.o.ntendon != H.ntendon;
  if (level >= COUNTS_SMOOTH) differ = differ || m->smooth.o.nu != H.nu;
  static const char* const words[] = {"the blob's position or dof counts differ from the plan's", "the blob's joint, dof or tendon counts differ from the plan's",
                                      "the blob's joint, dof, tendon or actuator counts differ from the plan's"};
  return differ ? words[level] : nullptr;
}

// the points of a call, point by point: the body id in range (where the model has a kinematics table), pt_pos finite, then pt_quat
// (NULL: the call takes none) finite and of a length that can be normalised -> SG_OK, or the first fault under the prefix f
static int check_points(const std::string& f, const SgKinHost& K, int n_pts, const int32_t* pt_body, const double* pt_pos, const double* pt_quat) {
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
  if (K.ok && !Dn.ok) return fail(SG_ERR_MODEL, std::string(fn) + ": " + Dn.err);
  if (const char* what = K.ok ? counts_differ(b->m, COUNTS_DYN) : nullptr) return fail(SG_ERR_MODEL, std::string(fn) + ": " + what);
  Readout r{b, fn, (hipStream_t)stream};
  if (int rc = r.prepare(env_ids, n_ids)) return rc;
  if (!ang && !lin && !com_lin && !ten_len && !ten_vel && !energy) return SG_OK;
  if (int rc = r.need_dyn()) return rc;
  SgDynArgs a;
  r.tables_dyn(a);
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
  if (K.ok && !Sm.ok) return fail(SG_ERR_MODEL, std::string(fn) + ": " + Sm.err);
  if (const char* what = K.ok ? counts_differ(b->m, COUNTS_SMOOTH) : nullptr) return fail(SG_ERR_MODEL, std::string(fn) + ": " + what);
  Readout r{b, fn, (hipStream_t)stream};
  if (int rc = r.prepare(env_ids, n_ids)) return rc;
  if (!M && !bias && !passive && !actuator && !inverse) return SG_OK;
  if (int rc = r.need_smooth()) return rc;
  // nbody <= SGS_MAXBODY, nv <= SGS_MAXDOF, ntendon <= SGS_MAXTENDON (sgs_build): with the kernel's static LDS within SGS_LDS_MAX
  const size_t lds = sizeof(double) * ((size_t)SGS_REC * K.o.nbody + (size_t)SGS_DOF * Dn.o.nv + 2 * (size_t)Dn.o.ntendon);
  if (int rc = r.grant_lds(b->smooth_attr_set, sg_smooth_kernel, SGS_LDS_MAX - SGS_STATIC_LDS)) return rc;
  SgSmoothArgs a;
  r.tables_smooth(a);
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
  if (int rc = check_points(f, K, n_pts, pt_body, pt_pos, pt_quat)) return rc;
  if (K.ok && !Pt.ok) return fail(SG_ERR_MODEL, f + Pt.err);
  if (const char* what = K.ok ? counts_differ(b->m, COUNTS_POINT) : nullptr) return fail(SG_ERR_MODEL, f + what);
  if ((long long)n_ids * n_pts > 0x7fffffffll) return fail(SG_ERR_INVALID, f + "too many envs x points for one launch");
  Readout r{b, fn, (hipStream_t)stream};
  if (int rc = r.prepare(env_ids, n_ids)) return rc;
  if (!pos && !mat && !vel && !acc && !gyro && !accel && !jacp && !jacr) return SG_OK;
  if (int rc = r.need_point()) return rc;   // (with the row of zeros: the qvel the Jacobian-only call walks at)
  // nbody <= SGP_MAXBODY, nv <= SGP_MAXDOF (sgp_build): with the kernel's static LDS within SGP_LDS_MAX
  const size_t lds = sizeof(double) * ((size_t)SGP_REC * K.o.nbody + (size_t)SGP_DOF * Dn.o.nv) + sizeof(int) * (size_t)Dn.o.nv;
  if (int rc = r.grant_lds(b->point_attr_set, sg_point_kernel, SGP_LDS_MAX - SGP_STATIC_LDS)) return rc;
  if (int rc = r.stage_points(b->pt_ids, b->pt_d, 7, n_pts, pt_body, pt_pos, pt_quat)) return rc;
  SgPointArgs a;
  r.tables_dyn(a);
  a.PI = b->point.i; a.p = Pt.o;
  a.qpos = qpos ? qpos : b->qpos; a.qvel = !use_qvel ? b->zero.d : qvel ? qvel : b->qvel; a.qacc = qacc;
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

// the launch of sg_solve_kernel over r's listed envs in one of its modes (the three entry points below; sg_get_forces for qacc_smooth and
// for W = M^-1 J' with rhs_count rows per env).  pt_body, pt_pos: the points on the device
static int solve_launch(Readout& r, int mode, int n_rhs, const double* y, double* x, const int* rhs_count, const double* applied, double* qacc, double* qfrc,
                        const int* pt_body, const double* pt_pos, double* W, double* pivot) {
  sg_batch* b = r.b;
  const SgKinHost& K = b->m->kin;
  const SgDynHost& Dn = b->m->dyn;
  const SgSolveHost& Sv = b->m->solve;
  if (int rc = r.need_solve()) return rc;   // (with the row of zeros: the qvel the calls that need M alone walk at)
  // a tile of SGV_MINRHS right-hand sides fits beside the fixed block (sgv_build); the launch asks for the tile it uses, no more
  const long long fixed = sgv_fixed_doubles(K.o.nbody, Dn.o.nv, Dn.o.ntendon, Sv.o.nM), room = sgv_tile(K.o.nbody, Dn.o.nv, Dn.o.ntendon, Sv.o.nM);
  const int tile = mode == SGV_MODE_FORWARD ? 1 : (int)std::min<long long>(n_rhs, mode == SGV_MODE_POINT ? room / 6 : room);
  const size_t lds = sizeof(double) * ((size_t)fixed + (size_t)tile * (mode == SGV_MODE_POINT ? 6 : 1) * Dn.o.nv);
  if (int rc = r.grant_lds(b->solve_attr_set, sg_solve_kernel, SGV_LDS_MAX - SGV_STATIC_LDS)) return rc;
  SgSolveArgs a;
  r.tables_smooth(a);
  a.VI = b->solve.i; a.v = Sv.o;
  a.qpos = b->qpos; a.qvel = b->qvel; a.act = b->act; a.kenv = b->kenv; a.zero = b->zero.d; a.kmask_jnt = b->kmask_jnt; a.kmask_ten = b->kmask_ten;
  a.env_ids = r.dids; a.n_ids = r.n_ids; a.mode = mode; a.n_rhs = mode == SGV_MODE_FORWARD ? 1 : n_rhs; a.tile = tile; a.rhs_count = rhs_count;
  a.y = y; a.x = x; a.applied = applied; a.qacc = qacc; a.qfrc = qfrc;
  a.pt_body = pt_body; a.pt_pos = pt_pos; a.W = W; a.pivot = pivot;
  hipLaunchKernelGGL(sg_solve_kernel, dim3(r.n_ids), dim3(64), lds, r.s, a);
  HIPCHK(hipGetLastError());
  return SG_OK;
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
  const SgSolveHost& Sv = b->m->solve;
  if (mode == SGV_MODE_POINT)
    if (int rc = check_points(f, K, n_rhs, pt_body, pt_pos, nullptr)) return rc;
  if (K.ok && !Sv.ok) return fail(SG_ERR_MODEL, f + Sv.err);
  if (const char* what = K.ok ? counts_differ(b->m, COUNTS_SMOOTH) : nullptr) return fail(SG_ERR_MODEL, f + what);
  if ((long long)n_ids * n_rhs > 0x7fffffffll / 36) return fail(SG_ERR_INVALID, f + "too many envs x right-hand sides or points for one launch");
  Readout r{b, fn, (hipStream_t)stream};
  if (int rc = r.prepare(env_ids, n_ids)) return rc;
  if (!x && !qacc && !qfrc && !W && !pivot) return SG_OK;
  if (mode == SGV_MODE_POINT)
    if (int rc = r.stage_points(b->sv_ids, b->sv_pos, 3, n_rhs, pt_body, pt_pos, nullptr)) return rc;
  return solve_launch(r, mode, n_rhs, y, x, nullptr, applied, qacc, qfrc, mode == SGV_MODE_POINT ? b->sv_ids.p : nullptr, mode == SGV_MODE_POINT ? b->sv_pos.p : nullptr, W,
                      pivot);
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

// ---- constraint and contact forces: the chunked launch chain of sg_forces_kernel.h ----
int sg_model_max_rows(const sg_model* m) {
  if (!m) return fail(SG_ERR_INVALID, "sg_model_max_rows: null model");
  if (!m->forces.ok) return fail(SG_ERR_MODEL, "sg_model_max_rows: " + m->forces.err);
  return m->forces.o.nrows;
}

// one env's share of the work space in bytes (its doubles, then its ints rounded up to whole doubles)
static size_t forces_env_bytes(const sg_model* m) {
  return 8 * (sgf_env_doubles(m->forces.o, m->dyn.o.nv) + (sgf_env_ints(m->forces.o) + 1) / 2);
}

int sg_set_forces_workspace(sg_batch* b, size_t bytes) {
  if (!b) return fail(SG_ERR_INVALID, "sg_set_forces_workspace: null batch");
  if (!b->m->forces.ok) return fail(SG_ERR_MODEL, "sg_set_forces_workspace: " + b->m->forces.err);
  const size_t need = forces_env_bytes(b->m);
  if (bytes < need) return fail(SG_ERR_INVALID, "sg_set_forces_workspace: " + std::to_string(bytes) + " bytes are below one env's need of " + std::to_string(need));
  b->forces_cap = bytes;
  return SG_OK;
}

int sg_get_forces(sg_batch* b, const int32_t* env_ids, int n_ids, int max_rows, int max_contacts, int32_t* nefc, int32_t* iters, int32_t* efc_type, int32_t* efc_id,
                  double* efc_force, int32_t* ncon, double* contact_force, double* qfrc_constraint, double* qacc, void* stream) {
  // (argument checks first, in an order that lets each be reached without a device)
  const std::string fn = "sg_get_forces: ";
  if (!b) return fail(SG_ERR_INVALID, fn + "null batch");
  if (n_ids <= 0) return fail(SG_ERR_INVALID, fn + "n_ids must be positive");
  if (max_rows <= 0 && (efc_type || efc_id || efc_force)) return fail(SG_ERR_INVALID, fn + "max_rows must be positive when a row array is given");
  if (max_contacts <= 0 && contact_force) return fail(SG_ERR_INVALID, fn + "max_contacts must be positive when contact_force is given");
  if (!env_ids && n_ids != b->n) return fail(SG_ERR_INVALID, fn + "env_ids == NULL needs n_ids == the batch's env count");
  if (env_ids)
    for (int i = 0; i < n_ids; i++)
      if (env_ids[i] < 0 || env_ids[i] >= b->n)
        return fail(SG_ERR_INVALID, fn + "env id " + std::to_string(env_ids[i]) + " out of range [0, " + std::to_string(b->n) + ")");
  const sg_model* m = b->m;
  const SgKinHost& K = m->kin;
  const SgForceHost& Fo = m->forces;
  if (K.ok && !Fo.ok) return fail(SG_ERR_MODEL, fn + Fo.err);
  if (const char* what = K.ok ? counts_differ(m, COUNTS_SMOOTH) : nullptr) return fail(SG_ERR_MODEL, fn + what);
  // (the kernels index the list: every env gets an id, also where the caller lists none)
  std::vector<int32_t> all;
  if (!env_ids) {
    all.resize(n_ids);
    for (int i = 0; i < n_ids; i++) all[i] = i;
    env_ids = all.data();
  }
  Readout r{b, "sg_get_forces", (hipStream_t)stream};
  if (int rc = r.prepare(env_ids, n_ids)) return rc;
  if (!nefc && !iters && !efc_type && !efc_id && !efc_force && !ncon && !contact_force && !qfrc_constraint && !qacc) return SG_OK;
  if (int rc = r.need_solve()) return rc;
  if (int rc = r.need_con()) return rc;
  if (int rc = r.need(b->forces, &Fo.dbl, &Fo.ints, "forces table")) return rc;
  const SgForceOff& f = Fo.o;
  const int nv = m->dyn.o.nv;
  const size_t nrows = f.nrows, cap = f.cap, per_env = forces_env_bytes(m);
  const int chunk = (int)std::min<size_t>((size_t)n_ids, std::max<size_t>(b->forces_cap / per_env, 1));
  if (int rc = r.reserve(b->forces_ws, (size_t)chunk * (per_env / 8), "work space")) return rc;
  const size_t lds_rows = sizeof(double) * ((size_t)SGS_REC * K.o.nbody + (size_t)SGS_DOF * nv) + sizeof(int) * (3 * nrows + cap);
  const size_t lds_pgs = sizeof(double) * (nrows + nv);
  if (int rc = r.grant_lds(b->forces_rows_attr_set, sg_forces_rows_kernel, SGF_LDS_MAX - SGF_STATIC_LDS)) return rc;
  if (int rc = r.grant_lds(b->forces_pgs_attr_set, sg_forces_pgs_kernel, SGF_LDS_MAX - SGF_STATIC_LDS)) return rc;
  // the work space of a chunk: every array for `chunk` envs, the doubles first
  SgForcesArgs a;
  r.tables_dyn(a);
  a.VI = b->solve.i; a.v = m->solve.o; a.FD = b->forces.d; a.FI = b->forces.i; a.f = f;
  a.qpos = b->qpos; a.qvel = b->qvel; a.warm = b->warm; a.zero = b->zero.d;
  double* wd = b->forces_ws.p;
  a.J = wd; wd += (size_t)chunk * nrows * nv;
  a.W = wd; wd += (size_t)chunk * nrows * nv;
  a.sc = wd; wd += (size_t)chunk * nrows * SGF_SC;
  a.qs = wd; wd += (size_t)chunk * nv;
  a.cdist = wd; wd += (size_t)chunk * cap;
  a.cpos = wd; wd += (size_t)chunk * 3 * cap;
  a.cframe = wd; wd += (size_t)chunk * 9 * cap;
  int* wi = (int*)wd;
  a.rows = wi; wi += (size_t)chunk * 3 * nrows;
  a.cgeom = wi; wi += (size_t)chunk * 2 * cap;
  a.caddr = wi; wi += (size_t)chunk * cap;
  a.ncon_ws = wi; wi += chunk;
  a.nefc_ws = wi;
  a.max_rows = max_rows; a.max_contacts = max_contacts;
  const int* ids = r.dids;
  for (int c0 = 0; c0 < n_ids; c0 += chunk) {
    const int nc = std::min(chunk, n_ids - c0);
    r.dids = ids + c0; r.n_ids = nc;
    if (int rc = contacts_launch(r, (int)cap, a.ncon_ws, a.cgeom, a.cdist, a.cpos, a.cframe)) return rc;
    if (int rc = solve_launch(r, SGV_MODE_FORWARD, 1, nullptr, nullptr, nullptr, nullptr, a.qs, nullptr, nullptr, nullptr, nullptr, nullptr)) return rc;
    a.env_ids = r.dids; a.n_ids = nc;
    const size_t at = (size_t)c0;
    a.nefc = nefc ? nefc + at : nullptr; a.iters = iters ? iters + at : nullptr; a.ncon = ncon ? ncon + at : nullptr;
    a.efc_type = efc_type ? efc_type + at * max_rows : nullptr; a.efc_id = efc_id ? efc_id + at * max_rows : nullptr;
    a.efc_force = efc_force ? efc_force + at * max_rows : nullptr;
    a.contact_force = contact_force ? contact_force + at * 3 * max_contacts : nullptr;
    a.qfrc = qfrc_constraint ? qfrc_constraint + at * nv : nullptr; a.qacc = qacc ? qacc + at * nv : nullptr;
    hipLaunchKernelGGL(sg_forces_rows_kernel, dim3(nc), dim3(64), lds_rows, r.s, a);
    HIPCHK(hipGetLastError());
    if (int rc = solve_launch(r, SGV_MODE_SOLVE, (int)nrows, a.J, a.W, a.nefc_ws, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr)) return rc;
    hipLaunchKernelGGL(sg_forces_pgs_kernel, dim3(nc), dim3(64), lds_pgs, r.s, a);
    HIPCHK(hipGetLastError());
  }
  return SG_OK;
}

// ---- the soft object: skin vertices, shape and subtrees, one kernel (sg_shape_kernel), whichever outputs the entry point fn passes ----
// the shape table of the model's current skin, built for a host query (fn: its name) -> SG_OK or SG_ERR_MODEL
static int shape_table(const char* fn, const sg_model* m, SgShapeHost* T) {
  sgh_build(m->kin, m->dyn, m->skin, T);
  return T->ok ? SG_OK : fail(SG_ERR_MODEL, std::string(fn) + ": " + T->err);
}

int sg_model_skin_closed(const sg_model* m) {
  if (!m) return fail(SG_ERR_INVALID, "sg_model_skin_closed: null model");
  SgShapeHost T;
  if (int rc = shape_table("sg_model_skin_closed", m, &T)) return rc;
  return T.o.closed;
}
int sg_model_skin_root(const sg_model* m) {
  if (!m) return fail(SG_ERR_INVALID, "sg_model_skin_root: null model");
  SgShapeHost T;
  if (int rc = shape_table("sg_model_skin_root", m, &T)) return rc;
  return T.o.root;
}
int sg_model_skin_rest(const sg_model* m, int frame_body, double* rest) {
  if (!m || !rest) return fail(SG_ERR_INVALID, "sg_model_skin_rest: null argument");
  if (!m->kin.ok) return fail(SG_ERR_MODEL, "sg_model_skin_rest: " + m->kin.err);
  if (frame_body < -1 || frame_body >= m->kin.o.nbody) return fail(SG_ERR_INVALID, "sg_model_skin_rest: frame_body outside [-1, nbody)");
  if (m->skin.nvert == 0) return fail(SG_ERR_MODEL, "sg_model_skin_rest: the model has no skin");
  sgh_rest(m->kin, m->skin, frame_body, rest);
  return SG_OK;
}
int sg_model_subtree_mass(const sg_model* m, double* mass) {
  if (!m || !mass) return fail(SG_ERR_INVALID, "sg_model_subtree_mass: null argument");
  SgShapeHost T;
  if (int rc = shape_table("sg_model_subtree_mass", m, &T)) return rc;
  std::copy(T.dbl.begin() + T.o.smass, T.dbl.begin() + T.o.smass + m->kin.o.nbody, mass);
  return SG_OK;
}

// the shape table on the batch's device, uploaded again when the model's skin has changed since (an earlier call, on whatever stream it
// went out, may still read the old one: the device is waited for first -- once per sg_model_set_skin, not per call)
static int shape_prepare(sg_batch* b, const char* fn, const SgShapeHost& T) {
  if (b->shape_up && b->shape_version == b->m->skin.version) return SG_OK;
  HIPCHK(hipDeviceSynchronize());
  b->shape_up = false;
  b->shape_mem.release();
  SgArena& A = b->shape_mem;
  double* d = nullptr;
  int* i = nullptr;
  if (!(A.upload(&d, T.dbl) && A.upload(&i, T.ints))) {
    const bool nomem = A.nomem;
    A.release();
    return devmem_fail(nomem, std::string(fn) + " (shape table)");
  }
  b->shape_d = d; b->shape_i = i; b->shape_off = T.o;
  b->shape_version = b->m->skin.version;
  b->shape_up = true;
  return SG_OK;
}

static int shape(const char* fn, bool need_skin, sg_batch* b, const int32_t* env_ids, int n_ids, int frame_body, int n_dirs, const double* dir,
                 const int32_t* dir_body, double* pos, double* vel, double* local, double* shp, double* lo, double* hi, int32_t* lo_vert, int32_t* hi_vert,
                 double* com, double* linvel, double* angmom, void* stream) {
  // (argument checks first, in an order that lets each be reached without a device)
  const std::string f = std::string(fn) + ": ";
  if (!b) return fail(SG_ERR_INVALID, f + "null batch");
  if (n_ids <= 0) return fail(SG_ERR_INVALID, f + "n_ids must be positive");
  if (n_dirs < 0 || n_dirs > SGH_MAXDIR) return fail(SG_ERR_INVALID, f + "n_dirs outside [0, " + std::to_string(SGH_MAXDIR) + "]");
  if (n_dirs > 0 && !dir) return fail(SG_ERR_INVALID, f + "null dir with n_dirs > 0");
  for (int j = 0; j < n_dirs; j++) {
    double n2 = 0.0;
    for (int c = 0; c < 3; c++) {
      if (!std::isfinite(dir[3 * j + c])) return fail(SG_ERR_INVALID, f + "direction " + std::to_string(j) + " is not finite");
      n2 += dir[3 * j + c] * dir[3 * j + c];
    }
    if (!(n2 > 0.0) || !std::isfinite(n2)) return fail(SG_ERR_INVALID, f + "direction " + std::to_string(j) + " has zero length (or overflows)");
  }
  const sg_model* m = b->m;
  const SgKinHost& K = m->kin;
  if (K.ok) {
    if (frame_body < -1 || frame_body >= K.o.nbody)
      return fail(SG_ERR_INVALID, f + "frame_body " + std::to_string(frame_body) + " outside [-1, " + std::to_string(K.o.nbody) + ")");
    for (int j = 0; dir_body && j < n_dirs; j++)
      if (dir_body[j] < -1 || dir_body[j] >= K.o.nbody)
        return fail(SG_ERR_INVALID, f + "body id " + std::to_string(dir_body[j]) + " of direction " + std::to_string(j) + " outside [-1, " + std::to_string(K.o.nbody) + ")");
  }
  if (!env_ids && n_ids != b->n) return fail(SG_ERR_INVALID, f + "env_ids == NULL needs n_ids == the batch's env count");
  if (env_ids)
    for (int i = 0; i < n_ids; i++)
      if (env_ids[i] < 0 || env_ids[i] >= b->n)
        return fail(SG_ERR_INVALID, f + "env id " + std::to_string(env_ids[i]) + " out of range [0, " + std::to_string(b->n) + ")");
  if (K.ok && !m->dyn.ok) return fail(SG_ERR_MODEL, f + m->dyn.err);
  if (const char* what = K.ok ? counts_differ(m, COUNTS_DYN) : nullptr) return fail(SG_ERR_MODEL, f + what);
  if (K.ok && need_skin && m->skin.nvert == 0) return fail(SG_ERR_MODEL, f + "the model has no skin (sg_model_set_skin)");
  SgShapeHost T;
  const bool stale = !(b->shape_up && b->shape_version == m->skin.version);
  if (K.ok && stale) {
    sgh_build(K, m->dyn, m->skin, &T);
    if (!T.ok) return fail(SG_ERR_MODEL, f + T.err);
  }
  const SgShapeOff& h = stale ? T.o : b->shape_off;
  if (K.ok && shp && h.closed != 1) return fail(SG_ERR_MODEL, f + "the skin is not closed: some directed edge of its faces lacks its reverse, or occurs twice");
  if (K.ok && (long long)n_ids * std::max(std::max(h.nvert, K.o.nbody), std::max(n_dirs, SGH_SHAPE_N)) > 0x7fffffffll / 3)
    return fail(SG_ERR_INVALID, f + "too many envs x vertices, bodies or directions for one launch");
  Readout r{b, fn, (hipStream_t)stream};
  if (int rc = r.prepare(env_ids, n_ids)) return rc;
  const bool ext = n_dirs > 0 && (lo || hi || lo_vert || hi_vert);
  if (!pos && !vel && !local && !shp && !ext && !com && !linvel && !angmom) return SG_OK;
  if (int rc = r.need_dyn()) return rc;
  if (int rc = shape_prepare(b, fn, T)) return rc;
  if (ext) {
    if (int rc = r.reserve(b->shape_dir, 3 * (size_t)n_dirs, "directions")) return rc;
    HIPCHK(hipMemcpyAsync(b->shape_dir.p, dir, sizeof(double) * 3 * n_dirs, hipMemcpyHostToDevice, r.s));
    if (dir_body) {
      if (int rc = r.reserve(b->shape_dir_body, (size_t)n_dirs, "direction body ids")) return rc;
      HIPCHK(hipMemcpyAsync(b->shape_dir_body.p, dir_body, sizeof(int) * n_dirs, hipMemcpyHostToDevice, r.s));
    }
  }
  // (sgh_build: the block fits SGH_LDS_MAX beside the kernel's static LDS)
  const size_t lds = (size_t)sgh_lds_bytes(K.o.nbody, b->shape_off.nvert);
  if (int rc = r.grant_lds(b->shape_attr_set, sg_shape_kernel, SGH_LDS_MAX - SGH_STATIC_LDS)) return rc;
  SgShapeArgs a;
  r.tables_dyn(a);
  a.HD = b->shape_d; a.HI = b->shape_i; a.h = b->shape_off;
  a.qpos = b->qpos; a.qvel = b->qvel; a.env_ids = r.dids; a.n_ids = n_ids; a.frame_body = frame_body;
  a.n_dirs = ext ? n_dirs : 0; a.dir = ext ? b->shape_dir.p : nullptr; a.dir_body = ext && dir_body ? b->shape_dir_body.p : nullptr;
  a.pos = pos; a.vel = vel; a.local = local; a.shape = shp; a.lo = lo; a.hi = hi; a.lo_vert = lo_vert; a.hi_vert = hi_vert;
  a.com = com; a.linvel = linvel; a.angmom = angmom;
  hipLaunchKernelGGL(sg_shape_kernel, dim3(n_ids), dim3(64), lds, r.s, a);
  HIPCHK(hipGetLastError());
  return SG_OK;
}

int sg_get_skin_vertices(sg_batch* b, const int32_t* env_ids, int n_ids, int frame_body, double* pos, double* vel, double* local, void* stream) {
  return shape("sg_get_skin_vertices", true, b, env_ids, n_ids, frame_body, 0, nullptr, nullptr, pos, vel, local, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
               nullptr, nullptr, stream);
}
int sg_get_shape(sg_batch* b, const int32_t* env_ids, int n_ids, int n_dirs, const double* dir, const int32_t* dir_body, double* shp, double* lo, double* hi,
                 int32_t* lo_vert, int32_t* hi_vert, void* stream) {
  return shape("sg_get_shape", true, b, env_ids, n_ids, -1, n_dirs, dir, dir_body, nullptr, nullptr, nullptr, shp, lo, hi, lo_vert, hi_vert, nullptr, nullptr, nullptr,
               stream);
}
int sg_get_subtree(sg_batch* b, const int32_t* env_ids, int n_ids, double* com, double* linvel, double* angmom, void* stream) {
  return shape("sg_get_subtree", false, b, env_ids, n_ids, -1, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, com, linvel,
               angmom, stream);
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
