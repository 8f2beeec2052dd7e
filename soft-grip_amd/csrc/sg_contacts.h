// sg_contacts.h -- mj_collision at the current state: the per-pair math and the candidate-pair table of sg_get_contacts.
//
// sg_get_contacts returns, for each listed env, the contact list the oracle's collision() (oracle/sg_oracle.c) builds on the geom poses
// of the batch's CURRENT qpos: the same candidate pairs in the same order, the same bounding tests, the same narrowphase, the same cap.
// Geometry only: geom1 / geom2, dist, pos, frame.
//
// Relation to the step's own contacts.  Inside a substep the collision pass runs on the qpos the substep STARTS from, and the Euler
// integration that ends the substep moves qpos on.  After sg_step the batch's qpos is therefore one integration PAST the collision pass
// whose list produced touch_out: the list returned here is the NEXT forward pass's list.  Directly after sg_reset(..., sim_start = 0, ...)
// or sg_set_state nothing lies between the two, and there the touch bits recomputed from this list equal sg_get_touch_words.
//
// This header is plain per-lane / host code (SG_HD, as sg_render.h and sg_general.h): the kernel in sg_contacts_kernel.h calls it on the
// device, and a g++ build runs the same functions pair by pair against the oracle (tests/test_contacts_host.py).
//   sgc_build_pairs  the candidate geom pairs after the static filters, in the oracle's order (body pairs ascending, geoms of the first
//                    body outer; contype / conaffinity, weld-group and parent - child filters; the pair swapped into type order)
//   sgc_broad        the oracle's bounding tests: plane against bounding sphere, bounding sphere against bounding sphere
//   sgc_narrow       every pair type but box - box (at most 4 records), by the routines the step kernels use (sg_math.h, sg_general.h)
//   sgc_frame        mju_makeFrame; the tangent of a plane - capsule contact follows the capsule's axis
// Box - box is sgm::gen_box_box itself (up to 8 records, a 2 x 16-point polygon work space).
#pragma once
#include <string>
#include <vector>

#include "sg_general.h"
#include "sg_pairs.h"   // sgc_pair_allowed, sgc_enum_pairs, sgc_build_pairs: the candidate-pair table (shared with sg_plan.cpp)
#include "../../include/softgrip_model.h"

#define SGC_MAXCON 512        // the oracle's MAXCON: add_contact keeps no more, whatever the model's nconmax says
#define SGC_SIMPLE_MAXREC 4   // records of a pair that is not box - box (plane - box: 4 corners)
#define SGC_MAXREC 8          // records of a box - box pair

// contacts mj_collision keeps at most: the model's nconmax when positive, and the oracle's 512
inline int sgc_cap(int nconmax) { return nconmax > 0 && nconmax < SGC_MAXCON ? nconmax : SGC_MAXCON; }

// bounding tests of collision(): true = the pair goes on to its narrowphase routine.  M1: geom1's orientation (row-major).
SG_HD bool sgc_broad(int t1, const double* p1, const double* M1, const double* p2, double rb1, double rb2, double margin) {
  const double dif[3] = {p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]};
  if (t1 == SG_GEOM_PLANE) {
    const double nrm[3] = {M1[2], M1[5], M1[8]};
    return !(sgm::dot3(dif, nrm) > margin + rb2);
  }
  const double bound = rb1 + rb2 + margin;
  return !(sgm::dot3(dif, dif) > bound * bound);
}

// plane (point pp, unit normal pn) against a sphere (collision(), plane - sphere branch)
template <class Rec>
SG_HD int sgc_plane_sphere(const double* pp, const double* pn, const double* c, double r, double margin, Rec& o) {
  const double e[3] = {c[0] - pp[0], c[1] - pp[1], c[2] - pp[2]}, dist = sgm::dot3(e, pn) - r;
  if (dist > margin) return 0;
  o.dist = dist;
  for (int k = 0; k < 3; k++) { o.pos[k] = c[k] - pn[k] * (r + 0.5 * dist); o.n[k] = pn[k]; }
  return 1;
}

// narrowphase of a pair that is not box - box: records out[0 .. n) in the oracle's order, n <= SGC_SIMPLE_MAXREC.
// (t1, t2): the geoms' types, already in type order.  Rec: dist, pos[3], n[3] (sgm::ConRec or a staging record in LDS).
template <class Rec>
SG_HD int sgc_narrow(int t1, int t2, const double* p1, const double* M1, const double* s1, const double* p2, const double* M2, const double* s2,
                     double margin, Rec* out) {
  if (t1 == SG_GEOM_PLANE) {
    const double nrm[3] = {M1[2], M1[5], M1[8]};
    if (t2 == SG_GEOM_SPHERE) return sgc_plane_sphere(p1, nrm, p2, s2[0], margin, out[0]);
    if (t2 == SG_GEOM_CAPSULE) {
      const double ax[3] = {M2[2], M2[5], M2[8]};
      return sgm::gen_plane_capsule(p1, nrm, p2, ax, s2[0], s2[1], margin, out[0], out[1]);
    }
    return sgm::gen_plane_box(p1, nrm, p2, M2, s2, margin, out);
  }
  sgm::ConRec a, b;
  int mask = 0;
  if (t1 == SG_GEOM_SPHERE) {
    mask = sgm::sphere_box(p1, s1[0], p2, M2, s2, margin, a);
  } else {
    const double ax[3] = {M1[2], M1[5], M1[8]};
    mask = sgm::capsule_box(p1, ax, s1[0], s1[1], p2, M2, s2, margin, a, b);
  }
  int n = 0;
  if (mask & 1) { out[n].dist = a.dist; for (int k = 0; k < 3; k++) { out[n].pos[k] = a.pos[k]; out[n].n[k] = a.n[k]; } n++; }
  if (mask & 2) { out[n].dist = b.dist; for (int k = 0; k < 3; k++) { out[n].pos[k] = b.pos[k]; out[n].n[k] = b.n[k]; } n++; }
  return n;
}

// the contact frame of a record: normal in the first row, completed as the oracle's make_frame; a plane - capsule contact hands the
// capsule's axis (third column of its orientation M2) in as the first tangent
SG_HD void sgc_frame(int t1, int t2, const double* M2, const double* n, double* fr) {
  const double ax[3] = {M2[2], M2[5], M2[8]};
  sgm::make_frame_hint(n, (t1 == SG_GEOM_PLANE && t2 == SG_GEOM_CAPSULE) ? ax : nullptr, fr);
}
