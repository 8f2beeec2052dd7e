// sg_ray_skin_kernels.h -- sg_ray with SG_RAY_SKIN: the soft object's skin as candidates of a ray query (fp64).
//
// Siblings of the two kernels of sg_ray_kernels.h, which keep their code, registers and LDS (the plain call launches them as before); the
// per-(ray, triangle) math is sg_ray_skin.h, the per-(ray, geom) math sg_ray.h, the traversal of the lanes-over-candidates kernel sg_ray_walk.h.
//   sg_skinray_vert_kernel   256 lanes = one listed env, a lane per vertex: xpos[body] + R(xquat[body]) vert_pos from the poses sg_kin_kernel
//                            wrote for this call, into a batch-owned fp64 buffer [n_ids][nvert][3] that BOTH layouts read.
//   sg_skinray_rays_kernel   lane per ray.  256 lanes = one listed env x one block of 256 rays.  Staged in LDS: the records of the geoms
//                            the skin does not replace (128 B each, with their ids: the ids stay the model's), the env's vertices (24 B
//                            each), the packed faces and the vertices' bodies.  At the limits (320 geoms none of them hidden, 256
//                            vertices, 512 faces) 40 960 + 6 144 + 2 048 + 1 024 + 640 = 50 816 B: three workgroups share a CU's 160 KB.
//                            Each lane walks the geoms, then the faces; every LDS read is one address per wavefront (a broadcast).
//   sg_skinray_geoms_kernel  lanes over candidates.  One wavefront per (env, ray): lane l takes geoms l, l + 64, ... (the hidden ones
//                            skipped), then faces l, l + 64, ..., from global memory, then the wave reduction of (t, id) by sgy_better:
//                            sgyw_walk, sgyw_reduce and sgyw_finish, the text the host builds compile.  The other three ray kernels keep
//                            loops of their own in the same order (profiles/r11_ray_walk_merged_rays_body.txt, r11_ray_walk_bench.json).
// All call sgy_visit / sgys_visit per candidate and order by sgy_better: the same bits.  An env with a pose of a visible geom or a
// vertex that is not finite gets dist = NaN, normal = NaN, geomid = -1 (a hidden geom rides on a body a vertex is bound to).
#pragma once
#include "sg_ray_kernels.h"
#include "sg_ray_walk.h"

static_assert(SGYS_MAXVERT == SGR_MAXVERT && SGYS_MAXFACE == SGR_MAXFACE && SGYS_CAT_ELEM == SGR_CAT_ELEM, "sg_ray takes the skins sg_render_ex takes");

struct SgSkinRayVertArgs {
  const int* vert_body;         // [nvert]
  const double* vert_pos;       // [nvert][3]
  const double *xpos, *xquat;   // [n_ids][nbody][3 | 4]
  int nvert, nbody;
  double* vtx;                  // [n_ids][nvert][3]
};

struct SgSkinRayArgs {
  SgRayArgs r;
  const double* vtx;       // [n_ids][nvert][3] world positions (sg_skinray_vert_kernel)
  const uint32_t* faces;   // [nface] sgr_pack_face
  const int* vert_body;    // [nvert]
  const int* hidden;       // [ngeom] 1: a geom the skin replaces
  const int* vis;          // [nvis] the other geoms' ids, ascending
  int nvert, nface, nvis;
};

// dynamic LDS of sg_skinray_rays_kernel (the carving below)
static inline size_t sg_skinray_lds(int nvis, int nvert, int nface) {
  return sizeof(double) * (SGY_REC * (size_t)nvis + 3 * (size_t)nvert) + 4 * (size_t)nface + 4 * (size_t)nvert + 2 * (size_t)nvis;
}

__global__ __launch_bounds__(256) void sg_skinray_vert_kernel(SgSkinRayVertArgs a) {
  const int k = blockIdx.x, v = threadIdx.x;
  if (v >= a.nvert) return;
  const size_t kb = (size_t)k * a.nbody + a.vert_body[v];
  const double vp[3] = {a.vert_pos[3 * v], a.vert_pos[3 * v + 1], a.vert_pos[3 * v + 2]};
  double out[3];
  sgys_vertex(a.xpos + kb * 3, a.xquat + kb * 4, vp, out);
  double* dst = a.vtx + ((size_t)k * a.nvert + v) * 3;
  for (int c = 0; c < 3; c++) dst[c] = out[c];
}

__device__ __forceinline__ void sg_skinray_finish(const SgSkinRayArgs& A, const SgyBest& best, const double* vtx, uint32_t face, size_t at) {
  int ia, ib, ic, geom;
  sgys_face(face, &ia, &ib, &ic);
  double dist, n[3];
  sgys_finish(best, vtx + 3 * ia, vtx + 3 * ib, vtx + 3 * ic, A.r.limit, &dist, &geom, n);
  sg_ray_write(A.r, at, dist, geom, n);
}

__global__ __launch_bounds__(256) void sg_skinray_rays_kernel(SgSkinRayArgs A, int nblk) {
  extern __shared__ double sk_dyn[];
  const SgRayArgs& a = A.r;
  double* srec = sk_dyn;                                        // [nvis][SGY_REC]
  double* svtx = srec + SGY_REC * A.nvis;                       // [nvert][3]
  uint32_t* sface = (uint32_t*)(svtx + 3 * A.nvert);            // [nface]
  int* svb = (int*)(sface + A.nface);                           // [nvert]
  unsigned short* sid = (unsigned short*)(svb + A.nvert);       // [nvis]
  const int tid = threadIdx.x;
  const int k = blockIdx.x / nblk, r = (blockIdx.x - k * nblk) * 256 + tid;
  bool bad = false;
  for (int q = tid; q < A.nvis; q += 256) {
    const int g = A.vis[q];
    double rec[SGY_REC];
    bad |= !sg_ray_record(a, k, g, rec);
    for (int c = 0; c < SGY_REC; c++) srec[SGY_REC * q + c] = rec[c];
    sid[q] = (unsigned short)g;
  }
  const double* vtx = A.vtx + (size_t)k * A.nvert * 3;
  for (int i = tid; i < 3 * A.nvert; i += 256) {
    const double x = vtx[i];
    bad |= !isfinite(x);
    svtx[i] = x;
  }
  for (int i = tid; i < A.nface; i += 256) sface[i] = A.faces[i];
  for (int i = tid; i < A.nvert; i += 256) svb[i] = A.vert_body[i];
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
  int exclude, geom, slot = 0;
  SgyBest best = {INFINITY, -1, 0};
  if (sg_ray_world(a, k, r, o, d, &exclude)) {
    for (int q = 0; q < A.nvis; q++) {
      const int was = best.geom;
      sgy_visit((int)sid[q], srec + SGY_REC * q, o, d, a.cat_mask, exclude, a.limit, &best);
      if (best.geom != was) slot = q;
    }
    if ((a.cat_mask >> SGYS_CAT_ELEM) & 1) {
      SgysFrame fr;
      sgys_frame(d, &fr);
      for (int f = 0; f < A.nface; f++) {
        int ia, ib, ic;
        sgys_face(sface[f], &ia, &ib, &ic);
        sgys_visit(a.ngeom + f, svtx + 3 * ia, ia, svtx + 3 * ib, ib, svtx + 3 * ic, ic, svb, fr, o, d, exclude, &best);
      }
    }
  }
  if (best.geom >= a.ngeom) {
    sg_skinray_finish(A, best, svtx, sface[best.geom - a.ngeom], at);
    return;
  }
  sgy_finish(best, srec + SGY_REC * slot, o, d, a.limit, &dist, &geom, n);
  sg_ray_write(a, at, dist, geom, n);
}

// the walk's source of sg_skinray_geoms_kernel: a record built from global memory per visit; bad: one held a pose that is not finite
struct SgSkinRayFetch {
  const SgSkinRayArgs& A;
  int k;
  bool bad;
  __device__ __forceinline__ int count() const { return A.r.ngeom; }
  __device__ __forceinline__ bool hidden(int g) const { return A.hidden[g]; }
  __device__ __forceinline__ const double* record(int g, double* buf) { bad |= !sg_ray_record(A.r, k, g, buf); return buf; }
};

// (the faces of an env that turns out bad are walked too, on vertices that are not finite; its results are NaN)
__global__ __launch_bounds__(64) void sg_skinray_geoms_kernel(SgSkinRayArgs A) {
  const SgRayArgs& a = A.r;
  const int lane = threadIdx.x;
  const int k = blockIdx.x / a.n_rays, r = blockIdx.x - k * a.n_rays;
  double o[3], d[3], dist, n[3];
  int exclude, geom;
  const bool live = sg_ray_world(a, k, r, o, d, &exclude);
  SgSkinRayFetch G = {A, k, false};
  const SgywSkin K = {A.vtx + (size_t)k * A.nvert * 3, A.faces, A.vert_body, A.nface};
  SgyBest best = {INFINITY, -1, 0};
  sgyw_walk(G, K, lane, 64, live, o, d, a.cat_mask, exclude, a.limit, &best);
  for (int i = lane; i < 3 * A.nvert; i += 64) G.bad |= !isfinite(K.vtx[i]);
  const bool bad = __any(G.bad);
  sgyw_reduce(&best);
  if (lane != 0) return;
  sgyw_finish(G, K, bad, best, o, d, a.limit, &dist, &geom, n);
  sg_ray_write(a, (size_t)k * a.n_rays + r, dist, geom, n);
}
