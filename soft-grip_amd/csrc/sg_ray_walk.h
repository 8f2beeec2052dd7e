// sg_ray_walk.h -- the traversal of sg_ray, written once over sg_ray.h and sg_ray_skin.h: which candidates a walker visits in which order
// (sgyw_walk), how 64 walkers are reduced (sgyw_reduce), how the winner becomes dist / geomid / normal (sgyw_finish).  Compiled by
// sg_skinray_geoms_kernel (sg_ray_skin_kernels.h), the g++ test build (tests/ray_ref.py) and scripts/sanitize/ray_skin_main.cpp.
// The geoms come from a SOURCE, a template parameter: count(), hidden(g) (the skin replaces geom g: it is not fetched) and record(g, buf)
// (geom g's record; buf: SGY_REC doubles it may be built in).  The skin is one view for every caller; "no skin" is nface = 0.
#pragma once
#include "sg_ray_skin.h"

struct SgywSkin {
  const double* vtx;       // [nvert][3] world positions
  const uint32_t* faces;   // [nface] packed (sgys_face)
  const int* vbody;        // [nvert] the bodies the vertices are bound to
  int nface;               // 0: no skin
};

// walker `first` of `stride` (1: one walker; 64: lanes over candidates): the geoms not hidden in ascending id order, then -- with a skin and
// the element bit in cat_mask -- the faces, face f under id count() + f.  A dead ray visits nothing, but the records are fetched all the
// same (a source that builds them finds a pose that is not finite on the way)
template <class Geoms>
SGY_HD void sgyw_walk(Geoms& G, const SgywSkin& K, int first, int stride, bool live, const double* o, const double* d, int cat_mask, int exclude,
                      double limit, SgyBest* best) {
  SGY_NO_CONTRACT
  for (int g = first; g < G.count(); g += stride) {
    if (G.hidden(g)) continue;
    double buf[SGY_REC];
    const double* rec = G.record(g, buf);
    if (live) sgy_visit(g, rec, o, d, cat_mask, exclude, limit, best);
  }
  if (!live || K.nface <= 0 || !((cat_mask >> SGYS_CAT_ELEM) & 1)) return;
  SgysFrame fr;
  sgys_frame(d, &fr);
  for (int f = first; f < K.nface; f += stride) {
    int ia, ib, ic;
    sgys_face(K.faces[f], &ia, &ib, &ic);
    sgys_visit(G.count() + f, K.vtx + 3 * ia, ia, K.vtx + 3 * ib, ib, K.vtx + 3 * ic, ic, K.vbody, fr, o, d, exclude, best);
  }
}

// The 64 walkers of a ray, in sg_tree_lanes.h's manner: a pass of the compiler holds SGYW_NW of them in w[] -- the lane's own on the
// device, where the partner of a lane at distance m comes by __shfl_xor, all 64 on the host, where it is w[l ^ m]
#if defined(__HIPCC__) && defined(__HIP_DEVICE_COMPILE__)
#define SGYW_NW 1
__device__ __forceinline__ SgyBest sgyw_partner(const SgyBest* w, int, int m) { return SgyBest{__shfl_xor(w->t, m), __shfl_xor(w->geom, m), __shfl_xor(w->ax, m)}; }
#else
#define SGYW_NW 64
inline SgyBest sgyw_partner(const SgyBest* w, int l, int m) { return w[l ^ m]; }
#endif

// butterfly m = 32, 16, ..., 1 by sgy_better(partner, mine): the winner ends in every walker
SGY_HD void sgyw_reduce(SgyBest* w) {
  for (int m = 32; m >= 1; m >>= 1) {
    SgyBest nx[SGYW_NW];
    for (int l = 0; l < SGYW_NW; l++) {
      nx[l] = sgyw_partner(w, l, m);
      if (!sgy_better(nx[l].t, nx[l].geom, w[l].t, w[l].geom)) nx[l] = w[l];
    }
    for (int l = 0; l < SGYW_NW; l++) w[l] = nx[l];
  }
}

// the result of a ray from its reduced best.  bad: the env has a pose that is not finite -> NaN, -1, NaN.  A face (best.geom >= count())
// finishes on its vertices, a geom on its record; a miss reads no record (sgy_finish does not look at it)
template <class Geoms>
SGY_HD void sgyw_finish(Geoms& G, const SgywSkin& K, bool bad, const SgyBest& best, const double* o, const double* d, double limit, double* dist,
                        int* geom, double* n) {
  SGY_NO_CONTRACT
  if (bad) {
    const uint64_t u = 0x7ff8000000000000ull;
    memcpy(dist, &u, 8);
    n[0] = n[1] = n[2] = *dist; *geom = -1;
  } else if (K.nface > 0 && best.geom >= G.count()) {
    int ia, ib, ic;
    sgys_face(K.faces[best.geom - G.count()], &ia, &ib, &ic);
    sgys_finish(best, K.vtx + 3 * ia, K.vtx + 3 * ib, K.vtx + 3 * ic, limit, dist, geom, n);
  } else {
    double buf[SGY_REC];
    sgy_finish(best, best.geom >= 0 ? G.record(best.geom, buf) : buf, o, d, limit, dist, geom, n);
  }
}

#if !defined(__HIPCC__)
// the host's source: one record per geom in memory; hidden NULL: no geom is
struct SgywHostGeoms {
  const double* rec;   // [n][SGY_REC]
  const int* hide;     // [n]
  int n;
  int count() const { return n; }
  bool hidden(int g) const { return hide && hide[g]; }
  const double* record(int g, double*) const { return rec + (size_t)SGY_REC * g; }
};

// one ray given in a body's frame (sgy_map_ray), start to finish.  layout 1: 64 walkers striding over the candidates, then the reduction --
// what sg_skinray_geoms_kernel compiles; 0: one walker, which MIRRORS the order of the lane-per-ray kernels' own loops (they do not compile
// this text; tests/test_gpu_ray*.py hold the layouts against each other bit for bit)
inline void sgyw_host_ray(SgywHostGeoms& G, const SgywSkin& K, int layout, const double* xpos, const double* xquat, const double* o_in, const double* d_in,
                          int exclude, int cat_mask, double limit, double* dist, int* geom, double* n) {
  double o[3], d[3];
  const bool live = sgy_map_ray(xpos, xquat, o_in, d_in, o, d);
  const int nw = layout ? SGYW_NW : 1;
  SgyBest w[SGYW_NW];
  for (int l = 0; l < nw; l++) {
    w[l] = SgyBest{INFINITY, -1, 0};
    sgyw_walk(G, K, l, nw, live, o, d, cat_mask, exclude, limit, &w[l]);
  }
  if (layout) sgyw_reduce(w);
  sgyw_finish(G, K, false, w[0], o, d, limit, dist, geom, n);
}
#endif
