// sg_ray_kernels.h -- ray queries on the current state (mj_ray, fp64) for sg_ray.
//
// Kernels of sg_readout.hip's translation unit, so their device assembly is in sg_readout.device.s and under the build's assembly
// check.  The poses come from sg_kin_kernel, unchanged: its fp64 xpos / xquat / geom_xpos / geom_xmat outputs, written
// into buffers the batch owns.  The kernels here only read those and the kinematics table; the per-ray math is sg_ray.h.
//
// Two layouts, because the two uses sit at opposite ends (which one a call gets: sg_ray in sg_readout.hip):
//   sg_ray_rays_kernel    lane per ray.  256 lanes = one listed env x one block of 256 rays.  The env's geoms are staged in LDS as fp64
//                         records (128 B a geom, 40 KB at the 320-geom limit: three workgroups share a CU's 160 KB); a record that is not
//                         finite marks the env bad.  Each lane maps its ray through its body's pose and walks the records in id order.
//   sg_ray_geoms_kernel   lanes over geoms.  One wavefront per (env, ray), no staging: lane l takes geoms l, l + 64, ... from global
//                         memory, then one wave reduction of (t, geom id) by smaller t, then smaller id.
// Both call sgy_visit per (ray, geom) and order hits by sgy_better, and sg_ray.h forms no fused multiply-add of its own, so the two give
// the same bits.  An env whose qpos holds a NaN or inf (sg_kin_kernel writes NaN poses for it) gets dist = NaN, normal = NaN, geomid = -1.
#pragma once
#include "sg_ray.h"
#include "sg_render.h"

static_assert(SGY_MAXGEOM == SGR_MAXGEOM, "sg_ray takes the models sg_render takes");
static_assert(SGY_PLANE == SGR_PLANE && SGY_SPHERE == SGR_SPHERE && SGY_CAPSULE == SGR_CAPSULE && SGY_BOX == SGR_BOX, "geom type codes");

struct SgRayArgs {
  const double* D;       // kinematics table: geom_size
  const int* I;          // kinematics table: geom type | category << 8, geom body
  int gsize, gmeta, gbody, ngeom, nbody;
  const double *xpos, *xquat, *gxpos, *gxmat;   // [n_ids][nbody][3 | 4], [n_ids][ngeom][3 | 9]: what sg_kin_kernel wrote
  const double *origin, *dir;                   // [n_rays][3], or [n_ids][n_rays][3] with per_env
  const int *ray_body, *ray_exclude;            // [n_rays] each, device (NULL: all -1)
  int n_ids, n_rays, per_env, cat_mask;
  double limit;                                 // max_dist, INFINITY for none
  double *dist, *normal;                        // [n_ids][n_rays], [n_ids][n_rays][3]; any may be NULL
  int32_t* geomid;                              // [n_ids][n_rays]
};

// geom g of listed env k as a record; false when a pose value is not finite
__device__ __forceinline__ bool sg_ray_record(const SgRayArgs& a, int k, int g, double* rec) {
  const size_t kg = (size_t)k * a.ngeom + g;
  bool ok = true;
  for (int c = 0; c < 3; c++) { rec[c] = a.gxpos[kg * 3 + c]; ok &= isfinite(rec[c]); }
  for (int c = 0; c < 9; c++) { rec[3 + c] = a.gxmat[kg * 9 + c]; ok &= isfinite(rec[3 + c]); }
  for (int c = 0; c < 3; c++) rec[12 + c] = a.D[a.gsize + 3 * g + c];
  const int m = a.I[a.gmeta + g];
  rec[15] = sgy_meta_word(sgy_meta(m & 0xFF, (m >> 8) & 0xFF, a.I[a.gbody + g]));
  return ok;
}

// ray r of listed env k in the world frame; false: a miss by its direction
__device__ __forceinline__ bool sg_ray_world(const SgRayArgs& a, int k, int r, double* o, double* d, int* exclude) {
  const size_t at = ((a.per_env ? (size_t)k * a.n_rays : 0) + r) * 3;
  const double oi[3] = {a.origin[at], a.origin[at + 1], a.origin[at + 2]}, di[3] = {a.dir[at], a.dir[at + 1], a.dir[at + 2]};
  const int body = a.ray_body ? a.ray_body[r] : -1;
  *exclude = a.ray_exclude ? a.ray_exclude[r] : -1;
  const size_t kb = (size_t)k * a.nbody + (body >= 0 ? body : 0);
  return sgy_map_ray(body >= 0 ? a.xpos + kb * 3 : nullptr, a.xquat + kb * 4, oi, di, o, d);
}

__device__ __forceinline__ void sg_ray_write(const SgRayArgs& a, size_t at, double dist, int geom, const double* n) {
  if (a.dist) a.dist[at] = dist;
  if (a.geomid) a.geomid[at] = geom;
  if (a.normal)
    for (int c = 0; c < 3; c++) a.normal[3 * at + c] = n[c];
}

__global__ __launch_bounds__(256) void sg_ray_rays_kernel(SgRayArgs a, int nblk) {
  extern __shared__ double sy_rec[];   // [ngeom][SGY_REC]
  const int tid = threadIdx.x;
  const int k = blockIdx.x / nblk, r = (blockIdx.x - k * nblk) * 256 + tid;
  bool bad = false;
  for (int g = tid; g < a.ngeom; g += 256) {
    double rec[SGY_REC];
    bad |= !sg_ray_record(a, k, g, rec);
    for (int c = 0; c < SGY_REC; c++) sy_rec[SGY_REC * g + c] = rec[c];
  }
  bad = __syncthreads_or(bad);
  if (r >= a.n_rays) return;
  const size_t at = (size_t)k * a.n_rays + r;
  const double qnan = __longlong_as_double(0x7ff8000000000000ll);
  double n[3] = {qnan, qnan, qnan};
  if (bad) {
    sg_ray_write(a, at, qnan, -1, n);
    return;
  }
  double o[3], d[3], dist;
  int exclude, geom;
  SgyBest best = {INFINITY, -1, 0};
  if (sg_ray_world(a, k, r, o, d, &exclude))
    for (int g = 0; g < a.ngeom; g++) sgy_visit(g, sy_rec + SGY_REC * g, o, d, a.cat_mask, exclude, a.limit, &best);
  sgy_finish(best, sy_rec + SGY_REC * (best.geom >= 0 ? best.geom : 0), o, d, a.limit, &dist, &geom, n);
  sg_ray_write(a, at, dist, geom, n);
}

__global__ __launch_bounds__(64) void sg_ray_geoms_kernel(SgRayArgs a) {
  const int lane = threadIdx.x;
  const int k = blockIdx.x / a.n_rays, r = blockIdx.x - k * a.n_rays;
  double o[3], d[3];
  int exclude;
  const bool live = sg_ray_world(a, k, r, o, d, &exclude);
  SgyBest best = {INFINITY, -1, 0};
  bool bad = false;
  for (int g = lane; g < a.ngeom; g += 64) {
    double rec[SGY_REC];
    bad |= !sg_ray_record(a, k, g, rec);
    if (live) sgy_visit(g, rec, o, d, a.cat_mask, exclude, a.limit, &best);
  }
  bad = __any(bad);
  for (int m = 32; m >= 1; m >>= 1) {
    const double t = __shfl_xor(best.t, m);
    const int g = __shfl_xor(best.geom, m), ax = __shfl_xor(best.ax, m);
    if (sgy_better(t, g, best.t, best.geom)) { best.t = t; best.geom = g; best.ax = ax; }
  }
  if (lane != 0) return;
  const size_t at = (size_t)k * a.n_rays + r;
  const double qnan = __longlong_as_double(0x7ff8000000000000ll);
  double n[3] = {qnan, qnan, qnan}, dist, rec[SGY_REC];
  int geom;
  if (bad) {
    sg_ray_write(a, at, qnan, -1, n);
    return;
  }
  if (best.geom >= 0) sg_ray_record(a, k, best.geom, rec);   // (a miss reads no record: sgy_finish does not look at it)
  sgy_finish(best, rec, o, d, a.limit, &dist, &geom, n);
  sg_ray_write(a, at, dist, geom, n);
}
