// sg_kin.hip -- pose read-out (mj_kinematics, fp64) and the headless renderer (fp32 ray casting) for sg_get_poses / sg_render.
//
// Compiled inside sg_api.hip's translation unit (it includes this file), so its device assembly is part of sg_api.device.s and of the
// build's assembly check.  Both kernels only READ the batch's canonical qpos ([n_envs][nq], what sg_get_state copies out), so every
// pipeline (rows, tree, the legacy ones) is served without touching its kernels.
//
//   sg_kin_kernel     one wavefront per listed env.  Bodies go level by level through a depth schedule built on the host (a lane per body
//                     of the level, 64-body strides), their poses stay in LDS (nbody x 7 doubles); then a lane per geom.  Writes any of
//                     xpos / xquat / geom_xpos / geom_xmat and, for the renderer, the geoms' fp32 records relative to the camera eye.
//   sg_render_kernel  256 lanes = one 16 x 16 pixel tile of one env.  Stages the env's records in LDS, culls their bounding spheres
//                     against the tile's ray cone (ballot + prefix count into an LDS list, planes always kept), then a lane per pixel
//                     traces its ray through the list only (sg_render.h).
// An env whose qpos holds a NaN or inf gets NaN poses and renders as background; nothing is indexed by a state value.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "sg_blob.h"   // sg_blob_find: the one (bounds-checked) reader of the model blob
#include "sg_plan.h"
#include "sg_render.h"
#include "sg_skin.h"
#include "../../include/softgrip_model.h"

// ---- the kinematics table: one double and one int array, sections at the offsets below ----
struct SgKinOff {
  int nbody, ngeom, njnt, nq, nlevel;
  // doubles
  int bpos, bquat, jpos, jaxis, jq0, gpos, gmat, gsize;
  // ints
  int bpar, bjadr, bjnum, jtype, jqadr, gbody, gmeta, lstart, lbody;
};

struct SgKinHost {
  bool ok = false;
  std::string err;
  int bad_type = -1;           // first geom type the renderer has no intersection for (-1: none)
  SgKinOff o;
  std::vector<double> dbl;
  std::vector<int> ints;
  std::vector<double> qpos0, rbound;
};

// mj_kinematics for one body, as mjcf.Model.kinematics() does it (parent pose in px / pq, parent quaternion normalised)
__host__ __device__ inline void sgk_quat_mul(double* r, const double* a, const double* b) {
  const double w = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
  const double x = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
  const double y = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
  const double z = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
  r[0] = w; r[1] = x; r[2] = y; r[3] = z;
}
__host__ __device__ inline void sgk_quat_mat(double* M, const double* q) {
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  M[0] = w * w + x * x - y * y - z * z; M[1] = 2 * (x * y - w * z); M[2] = 2 * (x * z + w * y);
  M[3] = 2 * (x * y + w * z); M[4] = w * w - x * x + y * y - z * z; M[5] = 2 * (y * z - w * x);
  M[6] = 2 * (x * z - w * y); M[7] = 2 * (y * z + w * x); M[8] = w * w - x * x - y * y + z * z;
}
__host__ __device__ inline void sgk_quat_normalize(double* q) {
  const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  if (n < 1e-15) { q[0] = 1; q[1] = q[2] = q[3] = 0; return; }
  for (int k = 0; k < 4; k++) q[k] /= n;
}
__host__ __device__ inline void sgk_mv(double* r, const double* M, const double* v) {
  const double x = M[0] * v[0] + M[1] * v[1] + M[2] * v[2], y = M[3] * v[0] + M[4] * v[1] + M[5] * v[2], z = M[6] * v[0] + M[7] * v[1] + M[8] * v[2];
  r[0] = x; r[1] = y; r[2] = z;
}

// body i from its parent's pose (pp, pq) -> out[7] = xpos, xquat
__host__ __device__ inline void sgk_body(const double* D, const int* I, const SgKinOff& o, const double* qpos, int i, const double* pp, const double* pq,
                                         double* out) {
  double R[9], t[3], pos[3], quat[4];
  sgk_quat_mat(R, pq);
  sgk_mv(t, R, D + o.bpos + 3 * i);
  for (int k = 0; k < 3; k++) pos[k] = pp[k] + t[k];
  sgk_quat_mul(quat, pq, D + o.bquat + 4 * i);
  const int j0 = I[o.bjadr + i], nj = I[o.bjnum + i];
  for (int j = j0; j < j0 + nj; j++) {
    const int type = I[o.jtype + j], qa = I[o.jqadr + j];
    if (type == SG_JNT_FREE) {
      for (int k = 0; k < 3; k++) pos[k] = qpos[qa + k];
      for (int k = 0; k < 4; k++) quat[k] = qpos[qa + 3 + k];
      sgk_quat_normalize(quat);
      continue;
    }
    const double* jp = D + o.jpos + 3 * j;
    const double* ja = D + o.jaxis + 3 * j;
    double anchor[3], axis[3];
    sgk_quat_mat(R, quat);
    sgk_mv(t, R, jp);
    for (int k = 0; k < 3; k++) anchor[k] = pos[k] + t[k];
    sgk_mv(axis, R, ja);
    const double dq = qpos[qa] - D[o.jq0 + j];
    if (type == SG_JNT_SLIDE) {
      for (int k = 0; k < 3; k++) pos[k] = pos[k] + axis[k] * dq;
    } else {
      const double s = sin(dq / 2);
      const double ql[4] = {cos(dq / 2), ja[0] * s, ja[1] * s, ja[2] * s};
      double qn[4];
      sgk_quat_mul(qn, quat, ql);
      for (int k = 0; k < 4; k++) quat[k] = qn[k];
      sgk_quat_mat(R, quat);
      sgk_mv(t, R, jp);
      for (int k = 0; k < 3; k++) pos[k] = anchor[k] - t[k];
    }
  }
  sgk_quat_normalize(quat);
  for (int k = 0; k < 3; k++) out[k] = pos[k];
  for (int k = 0; k < 4; k++) out[3 + k] = quat[k];
}

// geom g from its body's pose: world position and orientation (row-major)
__host__ __device__ inline void sgk_geom(const double* D, const int* I, const SgKinOff& o, const double* body7, int g, double* gx, double* gm) {
  double R[9], t[3];
  sgk_quat_mat(R, body7 + 3);
  sgk_mv(t, R, D + o.gpos + 3 * g);
  for (int k = 0; k < 3; k++) gx[k] = body7[k] + t[k];
  const double* L = D + o.gmat + 9 * g;
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) gm[3 * r + c] = R[3 * r] * L[c] + R[3 * r + 1] * L[3 + c] + R[3 * r + 2] * L[6 + c];
}

// ---- host: the table from the blob and the plan ----
// per body: parent, body_pos, body_quat, its joints; per joint: type, jnt_pos, jnt_axis, qposadr, qpos0; per geom: body, geom_pos, geom_quat
// (as a matrix), geom_size, geom_type, geom_rbound and a category from the plan; the bodies' depth-level schedule
static void sgk_build(const void* blob, size_t nbytes, const SgPlan& plan, const SgTreeDev* tree, bool fast, SgKinHost* K) {
  long long nb = 0, nj = 0, ng = 0, nq = 0, c = 0;
#define KF(var, name, dt, want)                                                               \
  const auto* var = (const std::conditional<dt == SG_DT_F64, double, int>::type*)sg_blob_find(blob, nbytes, name, dt, &c); \
  if (!var || (want >= 0 && c != want)) { K->err = std::string("model blob lacks ") + name; return; }
  KF(par, "body_parentid", SG_DT_I32, -1);
  nb = c;
  KF(bpos, "body_pos", SG_DT_F64, 3 * nb);
  KF(bquat, "body_quat", SG_DT_F64, 4 * nb);
  KF(jadr, "body_jntadr", SG_DT_I32, nb);
  KF(jnum, "body_jntnum", SG_DT_I32, nb);
  KF(jtype, "jnt_type", SG_DT_I32, -1);
  nj = c;
  KF(jpos, "jnt_pos", SG_DT_F64, 3 * nj);
  KF(jaxis, "jnt_axis", SG_DT_F64, 3 * nj);
  KF(q0, "qpos0", SG_DT_F64, -1);
  nq = c;
  KF(gtype, "geom_type", SG_DT_I32, -1);
  ng = c;
  KF(gbody, "geom_bodyid", SG_DT_I32, ng);
  KF(gpos, "geom_pos", SG_DT_F64, 3 * ng);
  KF(gquat, "geom_quat", SG_DT_F64, 4 * ng);
  KF(gsize, "geom_size", SG_DT_F64, 3 * ng);
  KF(grb, "geom_rbound", SG_DT_F64, ng);
#undef KF
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

// mj_kinematics on the host at qpos0: body poses [nbody][7]
static void sgk_host_fk(const SgKinHost& K, std::vector<double>* body) {
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
static void sgk_default_camera(const SgKinHost& K, double* cam) {
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

// ---- device ----
struct SgKinArgs {
  const double* D;
  const int* I;
  SgKinOff o;
  const double* qpos;
  const int* env_ids;   // device, n_ids entries (NULL: env k = k)
  int n_ids;
  double *xpos, *xquat, *gxpos, *gxmat;   // any may be NULL
  float* recs;                             // [n_ids][ngeom][SGR_REC] (NULL: no records)
  double eye[3];
};

__global__ __launch_bounds__(64) void sg_kin_kernel(SgKinArgs a) {
  extern __shared__ double sk_body[];   // [nbody][7]
  const SgKinOff& o = a.o;
  const int k = blockIdx.x, lane = threadIdx.x;
  const int env = a.env_ids ? a.env_ids[k] : k;
  const double* q = a.qpos + (size_t)env * o.nq;
  bool bad = false;
  for (int i = lane; i < o.nq; i += 64) bad |= !isfinite(q[i]);
  bad = __syncthreads_or(bad);
  const double qnan = __longlong_as_double(0x7ff8000000000000ll);
  if (lane == 0) {
    for (int c = 0; c < 7; c++) sk_body[c] = c == 3 ? 1.0 : 0.0;
  }
  __syncthreads();
  if (!bad) {
    for (int L = 1; L < o.nlevel; L++) {
      const int b0 = a.I[o.lstart + L], b1 = a.I[o.lstart + L + 1];
      for (int s = b0 + lane; s < b1; s += 64) {
        const int i = a.I[o.lbody + s], p = a.I[o.bpar + i];
        sgk_body(a.D, a.I, o, q, i, sk_body + 7 * p, sk_body + 7 * p + 3, sk_body + 7 * i);
      }
      __syncthreads();
    }
  }
  if (a.xpos || a.xquat) {
    for (int i = lane; i < o.nbody; i += 64) {
      if (a.xpos)
        for (int c = 0; c < 3; c++) a.xpos[((size_t)k * o.nbody + i) * 3 + c] = bad ? qnan : sk_body[7 * i + c];
      if (a.xquat)
        for (int c = 0; c < 4; c++) a.xquat[((size_t)k * o.nbody + i) * 4 + c] = bad ? qnan : sk_body[7 * i + 3 + c];
    }
  }
  for (int g = lane; g < o.ngeom; g += 64) {
    double gx[3], gm[9];
    if (bad) {
      for (int c = 0; c < 3; c++) gx[c] = qnan;
      for (int c = 0; c < 9; c++) gm[c] = qnan;
    } else {
      sgk_geom(a.D, a.I, o, sk_body + 7 * a.I[o.gbody + g], g, gx, gm);
    }
    const size_t kg = (size_t)k * o.ngeom + g;
    if (a.gxpos)
      for (int c = 0; c < 3; c++) a.gxpos[kg * 3 + c] = gx[c];
    if (a.gxmat)
      for (int c = 0; c < 9; c++) a.gxmat[kg * 9 + c] = gm[c];
    if (a.recs) {
      const int meta = a.I[o.gmeta + g];
      float rec[SGR_REC];
      sgr_make_record(gx, gm, a.D + o.gsize + 3 * g, meta & 0xFF, meta >> 8, a.eye, rec);
      float4* dst = (float4*)(a.recs + kg * SGR_REC);
      for (int c = 0; c < 4; c++) dst[c] = make_float4(rec[4 * c], rec[4 * c + 1], rec[4 * c + 2], rec[4 * c + 3]);
    }
  }
}

struct SgRenderArgs {
  const float* recs;   // [n_ids][ngeom][SGR_REC]
  int ngeom, n_ids, tiles_x, ntiles;
  SgrCam cam;
  uint8_t* rgba;       // [n_ids][H][W][4]
  float* depth;        // [n_ids][H][W]
  int32_t* segid;      // [n_ids][H][W]
};

__global__ __launch_bounds__(256) void sg_render_kernel(SgRenderArgs a) {
  __shared__ float4 srec[SGR_MAXGEOM * SGR_REC / 4];
  __shared__ unsigned short slist[SGR_MAXGEOM];
  __shared__ int swc[4];
  const int tid = threadIdx.x;
  const int k = blockIdx.x / a.ntiles, tile = blockIdx.x - k * a.ntiles;
  const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
  const int W = a.cam.width, H = a.cam.height;
  // 1. stage the env's records (a NaN / inf anywhere but in the meta word: the env renders as background)
  const float4* src = (const float4*)(a.recs + (size_t)k * a.ngeom * SGR_REC);
  bool bad = false;
  for (int i = tid; i < a.ngeom * (SGR_REC / 4); i += 256) {
    const float4 v = src[i];
    bad |= !isfinite(v.x) || !isfinite(v.y) || !isfinite(v.z) || ((i & 3) != 3 && !isfinite(v.w));
    srec[i] = v;
  }
  bad = __syncthreads_or(bad);
  const float* recs = (const float*)srec;
  // 2. cull against the tile's ray cone (corner pixels of the tile, clipped to the image)
  int n = 0;
  if (!bad) {
    const int i0 = tx * SGR_TILE, j0 = ty * SGR_TILE, i1 = min(i0 + SGR_TILE - 1, W - 1), j1 = min(j0 + SGR_TILE - 1, H - 1);
    float d0[3], d1[3], d2[3], d3[3], axis[3], cs, sn;
    sgr_ray(a.cam, i0, j0, d0); sgr_ray(a.cam, i1, j0, d1); sgr_ray(a.cam, i0, j1, d2); sgr_ray(a.cam, i1, j1, d3);
    sgr_tile_cone(d0, d1, d2, d3, axis, &cs, &sn);
    const int w = tid >> 6, lane = tid & 63;
    for (int base = 0; base < a.ngeom; base += 256) {
      const int g = base + tid;
      const bool keep = g < a.ngeom && sgr_cone_keep(recs + SGR_REC * g, axis, cs, sn);
      const unsigned long long m = __ballot(keep);
      if (lane == 0) swc[w] = __popcll(m);
      __syncthreads();
      int off = n, tot = 0;
      for (int q = 0; q < 4; q++) { off += q < w ? swc[q] : 0; tot += swc[q]; }
      if (keep) slist[off + __popcll(m & ((1ull << lane) - 1ull))] = (unsigned short)g;   // (ascending geom id: ties go to the smaller id)
      n += tot;
      __syncthreads();
    }
  }
  // 3. a lane per pixel
  const int i = tx * SGR_TILE + (tid & (SGR_TILE - 1)), j = ty * SGR_TILE + (tid >> 4);
  if (i >= W || j >= H) return;
  SgrHit h;
  if (bad) {
    h.depth = INFINITY; h.geom = -1;
    sgr_background(h.rgba);
  } else {
    float d[3];
    sgr_ray(a.cam, i, j, d);
    h = sgr_trace(recs, slist, n, a.cam, d);
  }
  const size_t px = ((size_t)k * H + j) * W + i;
  if (a.rgba) ((uchar4*)a.rgba)[px] = make_uchar4(h.rgba[0], h.rgba[1], h.rgba[2], h.rgba[3]);
  if (a.depth) a.depth[px] = h.depth;
  if (a.segid) a.segid[px] = h.geom;
}

// ---- the skin (sg_render_ex with SG_RENDER_SKIN): triangles bound to bodies, sg_skin.h ----
//   sg_skin_vert_kernel  256 lanes = one listed env, a lane per vertex: world position from the body poses sg_kin_kernel wrote (fp64, the
//                        eye subtracted before the cast), positions into LDS, then the vertex normal over the host-built vertex -> face
//                        adjacency list.  Writes [n_ids][nvert] records of 2 x float4.  Once per env and not per tile: a 640 x 480 image
//                        has 1 200 tiles per env.  A NaN env writes NaN.
//   sg_rskin_kernel      sg_render_kernel's sibling (that kernel keeps its code, LDS and registers): additionally stages the env's vertex
//                        positions (4 KB) and the faces (2 KB) in LDS, leaves the geoms the skin replaces out of the culled list, culls the
//                        triangles' bounding spheres against the tile cone into a second LDS list (1 KB; 432 faces = two passes of 256
//                        lanes), traces geoms then triangles and reads the normals of the hit's three vertices only.
struct SgSkinDev {
  const int* vert_body;      // [nvert]
  const double* vert_pos;    // [nvert][3]
  const uint32_t* faces;     // [nface] sgr_pack_face
  const int* adj_start;      // [nvert + 1]
  const int* adj;            // [3 nface]
  const int* hidden;         // [ngeom] 1: a geom the skin replaces
  int nvert, nface;
  float rgb[3];
};

struct SgSkinVertArgs {
  SgSkinDev s;
  const double *xpos, *xquat;   // [n_ids][nbody][3 | 4]
  int nbody;
  double eye[3];
  float* vrec;                  // [n_ids][nvert][SGR_VREC]
};

__global__ __launch_bounds__(256) void sg_skin_vert_kernel(SgSkinVertArgs a) {
  __shared__ float4 spos[SGR_MAXVERT];
  const int k = blockIdx.x, v = threadIdx.x;
  if (v < a.s.nvert) {
    const size_t kb = (size_t)k * a.nbody + a.s.vert_body[v];
    double R[9], t[3];
    sgk_quat_mat(R, a.xquat + kb * 4);
    sgk_mv(t, R, a.s.vert_pos + 3 * v);
    const double* bp = a.xpos + kb * 3;
    spos[v] = make_float4((float)(bp[0] + t[0] - a.eye[0]), (float)(bp[1] + t[1] - a.eye[1]), (float)(bp[2] + t[2] - a.eye[2]), 0.0f);
  }
  __syncthreads();
  if (v < a.s.nvert) {
    float n[3];
    sgr_vertex_normal(v, (const float*)spos, a.s.faces, a.s.adj_start, a.s.adj, n);
    float4* dst = (float4*)(a.vrec + ((size_t)k * a.s.nvert + v) * SGR_VREC);
    dst[0] = spos[v];
    dst[1] = make_float4(n[0], n[1], n[2], 0.0f);
  }
}

struct SgSkinRenderArgs {
  SgRenderArgs r;
  SgSkinDev s;
  const float* vrec;   // [n_ids][nvert][SGR_VREC]
};

__global__ __launch_bounds__(256) void sg_rskin_kernel(SgSkinRenderArgs A) {
  __shared__ float4 srec[SGR_MAXGEOM * SGR_REC / 4];
  __shared__ float4 svert[SGR_MAXVERT];
  __shared__ uint32_t sface[SGR_MAXFACE];
  __shared__ unsigned short slist[SGR_MAXGEOM];
  __shared__ unsigned short sflist[SGR_MAXFACE];
  __shared__ int swc[4];
  const SgRenderArgs& a = A.r;
  const int tid = threadIdx.x;
  const int k = blockIdx.x / a.ntiles, tile = blockIdx.x - k * a.ntiles;
  const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
  const int W = a.cam.width, H = a.cam.height;
  const int nvert = A.s.nvert, nface = A.s.nface;
  // 1. stage the env's records, its vertex positions and the faces (a NaN / inf: the env renders as background)
  const float4* src = (const float4*)(a.recs + (size_t)k * a.ngeom * SGR_REC);
  bool bad = false;
  for (int i = tid; i < a.ngeom * (SGR_REC / 4); i += 256) {
    const float4 v = src[i];
    bad |= !isfinite(v.x) || !isfinite(v.y) || !isfinite(v.z) || ((i & 3) != 3 && !isfinite(v.w));
    srec[i] = v;
  }
  const float* vrec = A.vrec + (size_t)k * nvert * SGR_VREC;
  if (tid < nvert) {
    const float4 v = ((const float4*)vrec)[2 * tid];
    bad |= !isfinite(v.x) || !isfinite(v.y) || !isfinite(v.z);
    svert[tid] = v;
  }
  for (int i = tid; i < nface; i += 256) sface[i] = A.s.faces[i];
  bad = __syncthreads_or(bad);
  const float* recs = (const float*)srec;
  const float* vpos = (const float*)svert;
  // 2. cull against the tile's ray cone: the geoms the skin does not replace, then the triangles
  int n = 0, nf = 0;
  if (!bad) {
    const int i0 = tx * SGR_TILE, j0 = ty * SGR_TILE, i1 = min(i0 + SGR_TILE - 1, W - 1), j1 = min(j0 + SGR_TILE - 1, H - 1);
    float d0[3], d1[3], d2[3], d3[3], axis[3], cs, sn;
    sgr_ray(a.cam, i0, j0, d0); sgr_ray(a.cam, i1, j0, d1); sgr_ray(a.cam, i0, j1, d2); sgr_ray(a.cam, i1, j1, d3);
    sgr_tile_cone(d0, d1, d2, d3, axis, &cs, &sn);
    const int w = tid >> 6, lane = tid & 63;
    for (int base = 0; base < a.ngeom; base += 256) {
      const int g = base + tid;
      const bool keep = g < a.ngeom && !A.s.hidden[g] && sgr_cone_keep(recs + SGR_REC * g, axis, cs, sn);
      const unsigned long long m = __ballot(keep);
      if (lane == 0) swc[w] = __popcll(m);
      __syncthreads();
      int off = n, tot = 0;
      for (int q = 0; q < 4; q++) { off += q < w ? swc[q] : 0; tot += swc[q]; }
      if (keep) slist[off + __popcll(m & ((1ull << lane) - 1ull))] = (unsigned short)g;
      n += tot;
      __syncthreads();
    }
    for (int base = 0; base < nface; base += 256) {
      const int f = base + tid;
      bool keep = false;
      if (f < nface) {
        const uint32_t fw = sface[f];
        keep = sgr_tri_cone_keep(vpos + 4 * (fw & 0xFF), vpos + 4 * ((fw >> 8) & 0xFF), vpos + 4 * ((fw >> 16) & 0xFF), axis, cs, sn);
      }
      const unsigned long long m = __ballot(keep);
      if (lane == 0) swc[w] = __popcll(m);
      __syncthreads();
      int off = nf, tot = 0;
      for (int q = 0; q < 4; q++) { off += q < w ? swc[q] : 0; tot += swc[q]; }
      if (keep) sflist[off + __popcll(m & ((1ull << lane) - 1ull))] = (unsigned short)f;   // (ascending face index: ties go to the smaller one)
      nf += tot;
      __syncthreads();
    }
  }
  // 3. a lane per pixel
  const int i = tx * SGR_TILE + (tid & (SGR_TILE - 1)), j = ty * SGR_TILE + (tid >> 4);
  if (i >= W || j >= H) return;
  SgrHit h;
  if (bad) {
    h.depth = INFINITY; h.geom = -1;
    sgr_background(h.rgba);
  } else {
    float d[3];
    int face;
    sgr_ray(a.cam, i, j, d);
    h = sgr_trace_skin(recs, slist, n, vpos, sface, sflist, nf, vrec, A.s.rgb, a.ngeom, a.cam, d, &face);
  }
  const size_t px = ((size_t)k * H + j) * W + i;
  if (a.rgba) ((uchar4*)a.rgba)[px] = make_uchar4(h.rgba[0], h.rgba[1], h.rgba[2], h.rgba[3]);
  if (a.depth) a.depth[px] = h.depth;
  if (a.segid) a.segid[px] = h.geom;
}
