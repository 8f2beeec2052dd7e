// sg_shape_kernel.h -- the kernel of the soft object's read-outs (sg_get_skin_vertices / sg_get_shape / sg_get_subtree), fp64.
//
// A kernel of sg_readout.hip's translation unit: its device assembly is in sg_readout.device.s and under the build's assembly check.
// It only READS the batch's canonical qpos and qvel, so every pipeline is served without touching its kernels.
//
//   sg_shape_kernel   one wavefront per listed env, sg_dyn_kernel's shape.  Bodies go level by level through the kinematics table's depth
//                     schedule into LDS (nbody x 13 doubles, sg_dyn.h's records); a lane per skin vertex (64-strides) then puts its
//                     position and velocity into LDS (nvert x 6 doubles) and writes pos / vel / local.  As the outputs ask: lanes over
//                     faces (64-strides) and twelve wavefront sums give the shape; per direction lanes over vertices and a butterfly
//                     min / max with the smaller index on a tie give the extents; a lane per body puts its subtree shares into LDS
//                     (nbody x 9 doubles) and a lane per body then adds its subtree's list in ascending body order.  ONE launch serves
//                     whichever outputs an entry point passes: a NULL output's section is skipped, and no section reads what another
//                     section wrote to memory.
// Sums: every lane adds its 64-strided shares in ascending order, then the xor butterfly of wave_sum2 (sg_work.h).  No atomics: two calls
// give the same bits, and an env's bits depend neither on the envs listed beside it nor on the directions listed beside one.
// An env whose qpos or qvel holds a NaN or inf gets NaN in every double output and -1 in every int output; nothing is indexed by a
// state value.
#pragma once
#include "sg_shape.h"

struct SgShapeArgs {
  const double* D;    // the kinematics table (sg_readout.h)
  const int* I;
  SgKinOff o;
  const double* DD;   // the dynamics table (sg_dyn.h)
  const int* DI;
  SgDynOff d;
  const double* HD;   // the shape table (sg_shape.h)
  const int* HI;
  SgShapeOff h;
  const double *qpos, *qvel;
  const int* env_ids;   // device, n_ids entries (NULL: env k = k)
  int n_ids, frame_body, n_dirs;
  const double* dir;      // device [n_dirs][3]
  const int* dir_body;    // device [n_dirs] (NULL: all -1)
  double *pos, *vel, *local;   // [n_ids][nvert][3]; any may be NULL
  double* shape;               // [n_ids][SGH_SHAPE_N]
  double *lo, *hi;             // [n_ids][n_dirs]
  int *lo_vert, *hi_vert;      // [n_ids][n_dirs]
  double *com, *linvel, *angmom;   // [n_ids][nbody][3]
};

__global__ __launch_bounds__(64) void sg_shape_kernel(SgShapeArgs a) {
  extern __shared__ double sh_lds[];   // [nbody][SGD_REC], [nvert][SGH_VREC], [nbody][SGH_SHARE]
  const SgKinOff& o = a.o;
  const SgDynOff& d = a.d;
  const SgShapeOff& h = a.h;
  double* recs = sh_lds;
  double* vtx = recs + (size_t)SGD_REC * o.nbody;
  double* shares = vtx + (size_t)SGH_VREC * h.nvert;
  const int k = blockIdx.x, lane = threadIdx.x;
  const int env = a.env_ids ? a.env_ids[k] : k;
  const double* q = a.qpos + (size_t)env * o.nq;
  const double* qd = a.qvel + (size_t)env * d.nv;
  bool bad = false;
  for (int i = lane; i < o.nq; i += 64) bad |= !isfinite(q[i]);
  for (int i = lane; i < d.nv; i += 64) bad |= !isfinite(qd[i]);
  bad = __syncthreads_or(bad);
  const double qnan = __longlong_as_double(0x7ff8000000000000ll);
  if (lane < SGD_REC) recs[lane] = lane == 3 ? 1.0 : 0.0;   // the world: at rest at the origin
  __syncthreads();
  if (!bad) {
    for (int L = 1; L < o.nlevel; L++) {
      const int b0 = a.I[o.lstart + L], b1 = a.I[o.lstart + L + 1];
      for (int s = b0 + lane; s < b1; s += 64) {
        const int i = a.I[o.lbody + s], p = a.I[o.bpar + i];
        sgd_body(a.D, a.I, o, a.DI + d.jdof, q, qd, i, recs + SGD_REC * p, recs + SGD_REC * i);
      }
      __syncthreads();
    }
  }
  const bool want_ext = a.n_dirs > 0 && (a.lo || a.hi || a.lo_vert || a.hi_vert);
  // 1. vertices: a lane per vertex
  if (a.pos || a.vel || a.local || a.shape || want_ext) {
    for (int v = lane; v < h.nvert; v += 64) {
      double* pv = vtx + SGH_VREC * v;
      if (!bad) sgh_vertex(recs + SGD_REC * a.HI[h.vbody + v], a.HD + h.vpos + 3 * v, pv);
      const size_t at = ((size_t)k * h.nvert + v) * 3;
      if (a.pos)
        for (int c = 0; c < 3; c++) a.pos[at + c] = bad ? qnan : pv[c];
      if (a.vel)
        for (int c = 0; c < 3; c++) a.vel[at + c] = bad ? qnan : pv[3 + c];
      if (a.local) {
        double l3[3] = {qnan, qnan, qnan};
        if (!bad) {
          if (a.frame_body < 0)
            for (int c = 0; c < 3; c++) l3[c] = pv[c];
          else
            sgh_local(recs + SGD_REC * a.frame_body, pv, l3);
        }
        for (int c = 0; c < 3; c++) a.local[at + c] = l3[c];
      }
    }
    __syncthreads();
  }
  // 2. the shape: lanes over faces, twelve sums
  if (a.shape) {
    double sum[SGH_NSUM];
    for (int c = 0; c < SGH_NSUM; c++) sum[c] = 0.0;
    if (!bad) {
      for (int f = lane; f < h.nface; f += 64) {
        double s1[SGH_NSUM];
        sgh_face(vtx, a.HI[h.face + 3 * f], a.HI[h.face + 3 * f + 1], a.HI[h.face + 3 * f + 2], s1);
        for (int c = 0; c < SGH_NSUM; c++) sum[c] += s1[c];
      }
      for (int c = 0; c < SGH_NSUM; c++) sum[c] = wave_sum2(sum[c]);
    }
    if (lane == 0) {
      double out[SGH_SHAPE_N];
      if (!bad) sgh_finish(sum, vtx, out);
      for (int c = 0; c < SGH_SHAPE_N; c++) a.shape[(size_t)k * SGH_SHAPE_N + c] = bad ? qnan : out[c];
    }
  }
  // 3. the extents: per direction lanes over vertices, a butterfly min / max that keeps the smaller index on a tie
  if (want_ext) {
    for (int j = 0; j < a.n_dirs; j++) {
      double bl = 0.0, bh = 0.0;
      int il = -1, ih = -1;
      if (!bad) {
        double dhat[3], og[3];
        sgh_direction(recs, a.dir + 3 * j, a.dir_body ? a.dir_body[j] : -1, dhat, og);
        for (int v = lane; v < h.nvert; v += 64) {
          const double x = sgh_height(dhat, og, vtx + SGH_VREC * v);
          if (sgh_lower(x, v, bl, il)) { bl = x; il = v; }
          if (sgh_upper(x, v, bh, ih)) { bh = x; ih = v; }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
          const double ol = __shfl_xor(bl, off), oh = __shfl_xor(bh, off);
          const int jl = __shfl_xor(il, off), jh = __shfl_xor(ih, off);
          if (sgh_lower(ol, jl, bl, il)) { bl = ol; il = jl; }
          if (sgh_upper(oh, jh, bh, ih)) { bh = oh; ih = jh; }
        }
      }
      if (lane == 0) {
        const size_t at = (size_t)k * a.n_dirs + j;
        if (a.lo) a.lo[at] = bad ? qnan : bl;
        if (a.hi) a.hi[at] = bad ? qnan : bh;
        if (a.lo_vert) a.lo_vert[at] = bad ? -1 : il;
        if (a.hi_vert) a.hi_vert[at] = bad ? -1 : ih;
      }
    }
  }
  // 4. the subtrees: a lane per body for the shares, then a lane per body over its subtree's list
  if (a.com || a.linvel || a.angmom) {
    if (!bad)
      for (int i = lane; i < o.nbody; i += 64) sgh_body_share(a.DD, d, recs + SGD_REC * i, i, shares + SGH_SHARE * i);
    __syncthreads();
    for (int i = lane; i < o.nbody; i += 64) {
      double c3[3] = {qnan, qnan, qnan}, l3[3] = {qnan, qnan, qnan}, a3[3] = {qnan, qnan, qnan};
      if (!bad) {
        const int s0 = a.HI[h.sstart + i];
        sgh_subtree(a.DD, d, shares, a.HI + h.slist + s0, a.HI[h.sstart + i + 1] - s0, a.HD[h.smass + i], i, c3, l3, a3);
      }
      const size_t at = ((size_t)k * o.nbody + i) * 3;
      for (int c = 0; c < 3; c++) {
        if (a.com) a.com[at + c] = c3[c];
        if (a.linvel) a.linvel[at + c] = l3[c];
        if (a.angmom) a.angmom[at + c] = a3[c];
      }
    }
  }
}
