// sg_contacts_kernel.h -- the contact list of the current state (mj_collision, fp64) for sg_get_contacts.
//
// The kernel of sg_readout.hip's translation unit that reuses the kinematics table and the per-body / per-geom routines of sg_readout.h; its
// device assembly is in sg_readout.device.s and under the build's assembly check.  The kernel only READS the batch's canonical qpos:
// every pipeline is served, no step kernel is touched.  The per-pair math and the pair table are in sg_contacts.h.
//
//   sg_contacts_kernel   one wavefront per listed env, three stages:
//     1. kinematics: body poses level by level, then geom_xpos / geom_xmat, into LDS (nbody x 7 + ngeom x 12 doubles; a per-env block of
//        global memory instead when the model's poses do not fit -- the second instantiation).  An env whose qpos holds a NaN or inf, or
//        whose poses leave the oracle's +-1e10 range, reports ncon = -1 and stops here: nothing below sees such a value.
//     2. broadphase: lanes stride over the candidate-pair table in the oracle's order, 64 pairs a pass; the survivors of the bounding
//        tests are appended IN ORDER (ballot + prefix count) to a queue in LDS.  The queue is drained 64 survivors at a time, so its 128
//        slots hold any number of survivors.
//     3. narrowphase: a lane per survivor writes its records to a staging block in LDS (8 records a lane).  Box - box pairs, whose polygon
//        clipping needs a 2 x 16-point work space, go eight lanes at a time through eight such work spaces in LDS.  An ordered prefix sum
//        over the lanes' record counts gives every record its slot; each lane then writes geoms, dist, pos and frame of its records.
//   Order guarantee: slot s of an env holds what the oracle's contact[s] holds -- pairs in table order, a pair's records in the order its
//   routine emits them.  ncon = min(records, cap), cap = the model's nconmax when positive, at most 512 (add_contact); records past the cap
//   or past max_contacts are counted (up to the cap) and not written.
#pragma once
#include "sg_contacts.h"
#include "sg_readout.h"

struct SgcRec { double dist, pos[3], n[3]; };
#define SGC_BB_SLOTS 8                                        // box - box pairs in flight
#define SGC_STAGE_DBL (64 * SGC_MAXREC * 7)                   // staging records of one round
#define SGC_POLY_DBL (SGC_BB_SLOTS * 2 * 16 * 3)              // polygon work spaces
#define SGC_QUEUE_DBL 64                                      // 128 ints
#define SGC_FIXED_DBL (SGC_STAGE_DBL + SGC_POLY_DBL + SGC_QUEUE_DBL)
static_assert(sizeof(SgcRec) == 7 * sizeof(double), "staging record layout");

static size_t sgc_pose_doubles(const SgKinOff& o) { return (size_t)o.nbody * 7 + (size_t)o.ngeom * 12; }

struct SgConArgs {
  const double* D;
  const int* I;
  SgKinOff o;
  const double* gaux;   // [ngeom][2]
  const int* pairs;     // [npair][2]
  int npair, cap;
  const double* qpos;
  const int* env_ids;   // device, n_ids entries (NULL: env k = k)
  int n_ids, max_contacts;
  int32_t *ncon, *geom;          // any may be NULL
  double *dist, *pos, *frame;
  double* scratch;               // [n_ids][nbody x 7 + ngeom x 12] when the poses do not fit LDS
};

template <bool POSE_IN_LDS>
__global__ __launch_bounds__(64) void sg_contacts_kernel(SgConArgs a) {
  extern __shared__ double sc_lds[];
  const SgKinOff& o = a.o;
  const int k = blockIdx.x, lane = threadIdx.x;
  SgcRec* stage = (SgcRec*)sc_lds;
  double* polyws = sc_lds + SGC_STAGE_DBL;
  int* queue = (int*)(polyws + SGC_POLY_DBL);
  double* body = POSE_IN_LDS ? sc_lds + SGC_FIXED_DBL : a.scratch + (size_t)k * ((size_t)o.nbody * 7 + (size_t)o.ngeom * 12);
  double* gx = body + 7 * o.nbody;
  double* gm = gx + 3 * o.ngeom;
  const int env = a.env_ids ? a.env_ids[k] : k;
  const double* q = a.qpos + (size_t)env * o.nq;
  // 1. kinematics
  bool bad = false;
  for (int i = lane; i < o.nq; i += 64) bad |= !isfinite(q[i]);
  bad = __syncthreads_or(bad);
  if (lane == 0)
    for (int c = 0; c < 7; c++) body[c] = c == 3 ? 1.0 : 0.0;
  __syncthreads();
  if (!bad) {
    for (int L = 1; L < o.nlevel; L++) {
      const int b0 = a.I[o.lstart + L], b1 = a.I[o.lstart + L + 1];
      for (int s = b0 + lane; s < b1; s += 64) {
        const int i = a.I[o.lbody + s], p = a.I[o.bpar + i];
        sgk_body(a.D, a.I, o, q, i, body + 7 * p, body + 7 * p + 3, body + 7 * i);
      }
      __syncthreads();
    }
    for (int g = lane; g < o.ngeom; g += 64) {
      double x[3], M[9];
      sgk_geom(a.D, a.I, o, body + 7 * a.I[o.gbody + g], g, x, M);
      for (int c = 0; c < 3; c++) { gx[3 * g + c] = x[c]; bad |= !(fabs(x[c]) <= SG_MAXVAL); }
      for (int c = 0; c < 9; c++) { gm[9 * g + c] = M[c]; bad |= !(fabs(M[c]) <= SG_MAXVAL); }
    }
    bad = __syncthreads_or(bad);
  }
  if (bad) {
    if (lane == 0 && a.ncon) a.ncon[k] = -1;
    return;
  }
  // 2. + 3.
  const unsigned long long lt = (1ull << lane) - 1ull;
  const int cap = a.cap, lim = a.max_contacts < cap ? a.max_contacts : cap;   // slots written: below both
  int base = 0, nq = 0, total = 0;
  while (true) {
    while (base < a.npair && nq < 64) {
      const int p = base + lane;
      bool keep = false;
      if (p < a.npair) {
        const int g1 = a.pairs[2 * p], g2 = a.pairs[2 * p + 1];
        keep = sgc_broad(a.I[o.gmeta + g1] & 0xFF, gx + 3 * g1, gm + 9 * g1, gx + 3 * g2, a.gaux[2 * g1 + 1], a.gaux[2 * g2 + 1],
                         fmax(a.gaux[2 * g1], a.gaux[2 * g2]));
      }
      const unsigned long long m = __ballot(keep);
      if (keep) queue[nq + __popcll(m & lt)] = p;
      nq += __popcll(m);
      base += 64;
    }
    __syncthreads();
    if (nq == 0) break;
    const int nr = nq < 64 ? nq : 64;
    const bool active = lane < nr;
    int g1 = 0, g2 = 0, t1 = 0, t2 = 0, cnt = 0;
    double margin = 0;
    if (active) {
      const int p = queue[lane];
      g1 = a.pairs[2 * p]; g2 = a.pairs[2 * p + 1];
      t1 = a.I[o.gmeta + g1] & 0xFF; t2 = a.I[o.gmeta + g2] & 0xFF;
      margin = fmax(a.gaux[2 * g1], a.gaux[2 * g2]);
    }
    const bool isbb = active && t1 == SG_GEOM_BOX;   // (type order: geom2 is a box then too)
    SgcRec* mine = stage + lane * SGC_MAXREC;
    if (active && !isbb)
      cnt = sgc_narrow(t1, t2, gx + 3 * g1, gm + 9 * g1, a.D + o.gsize + 3 * g1, gx + 3 * g2, gm + 9 * g2, a.D + o.gsize + 3 * g2, margin, mine);
    const unsigned long long bbm = __ballot(isbb);
    const int nbb = __popcll(bbm), rank = __popcll(bbm & lt);
    for (int it = 0; it * SGC_BB_SLOTS < nbb; it++) {
      if (isbb && rank / SGC_BB_SLOTS == it) {
        double(*poly)[3] = (double(*)[3])(polyws + (rank % SGC_BB_SLOTS) * 96);
        cnt = sgm::gen_box_box(gx + 3 * g1, gm + 9 * g1, a.D + o.gsize + 3 * g1, gx + 3 * g2, gm + 9 * g2, a.D + o.gsize + 3 * g2, margin, mine, poly,
                               poly + 16);
      }
      __syncthreads();
    }
    // ordered prefix sum over the lanes' counts
    int incl = cnt;
    for (int d = 1; d < 64; d <<= 1) {
      const int v = __shfl_up(incl, d);
      if (lane >= d) incl += v;
    }
    const int slot0 = total + incl - cnt;
    for (int c = 0; c < cnt; c++) {
      const int slot = slot0 + c;
      if (slot >= lim) break;
      const SgcRec& r = mine[c];
      const size_t at = (size_t)k * a.max_contacts + slot;
      if (a.geom) { a.geom[2 * at] = g1; a.geom[2 * at + 1] = g2; }
      if (a.dist) a.dist[at] = r.dist;
      if (a.pos)
        for (int x = 0; x < 3; x++) a.pos[3 * at + x] = r.pos[x];
      if (a.frame) {
        double nn[3] = {r.n[0], r.n[1], r.n[2]}, fr[9];
        sgc_frame(t1, t2, gm + 9 * g2, nn, fr);
        for (int x = 0; x < 9; x++) a.frame[9 * at + x] = fr[x];
      }
    }
    total += __shfl(incl, 63);
    // drop the round's survivors from the queue
    const int rest = nq - nr;
    const int carry = lane < rest ? queue[64 + lane] : 0;
    __syncthreads();
    if (lane < rest) queue[lane] = carry;
    nq = rest;
    if (total >= cap) break;
    __syncthreads();
  }
  if (lane == 0 && a.ncon) a.ncon[k] = total < cap ? total : cap;
}
