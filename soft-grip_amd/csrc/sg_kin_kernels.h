// sg_kin_kernels.h -- pose read-out (mj_kinematics, fp64) and the headless renderer (fp32 ray casting) for sg_get_poses / sg_render.
//
// Kernels of sg_readout.hip's translation unit: their device assembly is in sg_readout.device.s and under the build's assembly check.
// Both kernels only READ the batch's canonical qpos ([n_envs][nq], what sg_get_state copies out), so every pipeline (rows, tree, the
// legacy ones) is served without touching its kernels.
//
//   sg_kin_kernel     one wavefront per listed env.  Bodies go level by level through a depth schedule built on the host (a lane per body
//                     of the level, 64-body strides), their poses stay in LDS (nbody x 7 doubles); then a lane per geom.  Writes any of
//                     xpos / xquat / geom_xpos / geom_xmat and, for the renderer, the geoms' fp32 records relative to the camera eye.
//   sg_render_kernel  256 lanes = one 16 x 16 pixel tile of one env.  Stages the env's records in LDS, culls their bounding spheres
//                     against the tile's ray cone (ballot + prefix count into an LDS list, planes always kept), then a lane per pixel
//                     traces its ray through the list only (sg_render.h).
// An env whose qpos holds a NaN or inf gets NaN poses and renders as background; nothing is indexed by a state value.
#pragma once
#include "sg_readout.h"
#include "sg_render.h"

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

// ---- what sg_render_kernel and sg_rskin_kernel share, each with the instruction stream it had before.  Staging the records is NOT shared
// and the compaction is a macro: as forced-inline functions they moved both kernels' code (profiles/r09_readout_split_asm_same.txt). ----
// One pass of 256 lanes over a keep-predicate: the kept ids go to list[n ..) in lane order -- ballot, prefix count over the four
// wavefronts in swc -- so a list built by ascending passes is ascending (ties go to the smaller id); n moves on.  w, lane: tid >> 6, tid & 63
#define SGR_COMPACT(keep, id, list, n, swc, w, lane)                                                   \
  do {                                                                                                 \
    const unsigned long long m = __ballot(keep);                                                       \
    if (lane == 0) swc[w] = __popcll(m);                                                               \
    __syncthreads();                                                                                   \
    int off = n, tot = 0;                                                                              \
    for (int q = 0; q < 4; q++) { off += q < w ? swc[q] : 0; tot += swc[q]; }                          \
    if (keep) list[off + __popcll(m & ((1ull << lane) - 1ull))] = (unsigned short)(id);                \
    n += tot;                                                                                          \
    __syncthreads();                                                                                   \
  } while (0)

__device__ __forceinline__ void sgr_write_pixel(const SgRenderArgs& a, size_t px, uchar4 c, float depth, int geom) {
  if (a.rgba) ((uchar4*)a.rgba)[px] = c;
  if (a.depth) a.depth[px] = depth;
  if (a.segid) a.segid[px] = geom;
}

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
      SGR_COMPACT(keep, g, slist, n, swc, w, lane);
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
  sgr_write_pixel(a, ((size_t)k * H + j) * W + i, make_uchar4(h.rgba[0], h.rgba[1], h.rgba[2], h.rgba[3]), h.depth, h.geom);
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
      SGR_COMPACT(keep, g, slist, n, swc, w, lane);
    }
    for (int base = 0; base < nface; base += 256) {
      const int f = base + tid;
      bool keep = false;
      if (f < nface) {
        const uint32_t fw = sface[f];
        keep = sgr_tri_cone_keep(vpos + 4 * (fw & 0xFF), vpos + 4 * ((fw >> 8) & 0xFF), vpos + 4 * ((fw >> 16) & 0xFF), axis, cs, sn);
      }
      SGR_COMPACT(keep, f, sflist, nf, swc, w, lane);
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
  sgr_write_pixel(a, ((size_t)k * H + j) * W + i, make_uchar4(h.rgba[0], h.rgba[1], h.rgba[2], h.rgba[3]), h.depth, h.geom);
}
