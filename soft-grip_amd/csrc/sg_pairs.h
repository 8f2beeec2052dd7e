// sg_pairs.h -- mj_collision's candidate geom pairs of a model, enumerated ONCE for both users: the plan's pair table of the general
// contact path (sg_plan.cpp) and the contact read-out's pair table (sg_contacts.h).  Host only.
//   sgc_pair_allowed  the oracle's pair_allowed: contype / conaffinity, weld group, parent - child
//   sgc_enum_pairs    the pairs in the oracle's order (body pairs ascending, geoms of the first body outer), each swapped into type order
//   sgc_build_pairs   the read-out's table: sgc_enum_pairs behind a range check of the body / geom tables, refusing the first pair of types
//                     without a narrowphase routine
// The two users share the LIST; what they refuse differs and stays theirs: the plan builder refuses plane - sphere outside tree plans and
// geoms outside its class, pair by pair in list order with its own messages, and does not range-check the tables.
#pragma once
#include <string>
#include <vector>

#include "../../include/softgrip_model.h"

// the oracle's pair_allowed
inline bool sgc_pair_allowed(const int* body_parentid, const int* body_weldid, const int* geom_bodyid, const int* contype, const int* conaffinity,
                             int g1, int g2) {
  const int b1 = geom_bodyid[g1], b2 = geom_bodyid[g2];
  if (!((contype[g1] & conaffinity[g2]) || (contype[g2] & conaffinity[g1]))) return false;
  const int w1 = body_weldid[b1], w2 = body_weldid[b2];
  if (w1 == w2) return false;   // same weld group (both static too)
  const int wp1 = body_weldid[body_parentid[w1]], wp2 = body_weldid[body_parentid[w2]];
  if (w1 != 0 && w2 != 0 && (w1 == wp2 || w2 == wp1)) return false;   // parent - child
  return true;
}

// candidate pairs [npair][2] (geom1, geom2 in mj_collideGeoms' by-type order), whatever their types
inline void sgc_enum_pairs(int nbody, const int* body_parentid, const int* body_weldid, const int* body_geomadr, const int* body_geomnum,
                           const int* geom_bodyid, const int* geom_type, const int* contype, const int* conaffinity, std::vector<int>* pairs) {
  pairs->clear();
  for (int b1 = 0; b1 < nbody; b1++)
    for (int b2 = b1 + 1; b2 < nbody; b2++)
      for (int i = 0; i < body_geomnum[b1]; i++)
        for (int j = 0; j < body_geomnum[b2]; j++) {
          int g1 = body_geomadr[b1] + i, g2 = body_geomadr[b2] + j;
          if (!sgc_pair_allowed(body_parentid, body_weldid, geom_bodyid, contype, conaffinity, g1, g2)) continue;
          if (geom_type[g1] > geom_type[g2]) { const int t = g1; g1 = g2; g2 = t; }
          pairs->push_back(g1);
          pairs->push_back(g2);
        }
}

// the same list after a range check of the tables.  false + err: tables out of range, or a pair of types without a narrowphase routine.
inline bool sgc_build_pairs(int nbody, int ngeom, const int* body_parentid, const int* body_weldid, const int* body_geomadr, const int* body_geomnum,
                            const int* geom_bodyid, const int* geom_type, const int* contype, const int* conaffinity, std::vector<int>* pairs,
                            std::string* err) {
  pairs->clear();
  for (int b = 0; b < nbody; b++) {
    if (body_parentid[b] < 0 || body_parentid[b] >= nbody || body_weldid[b] < 0 || body_weldid[b] >= nbody || body_geomnum[b] < 0 ||
        (body_geomnum[b] > 0 && (body_geomadr[b] < 0 || body_geomadr[b] + body_geomnum[b] > ngeom))) {
      *err = "body tables out of range";
      return false;
    }
  }
  for (int g = 0; g < ngeom; g++)
    if (geom_bodyid[g] < 0 || geom_bodyid[g] >= nbody) { *err = "geom body out of range"; return false; }
  sgc_enum_pairs(nbody, body_parentid, body_weldid, body_geomadr, body_geomnum, geom_bodyid, geom_type, contype, conaffinity, pairs);
  for (size_t p = 0; p < pairs->size(); p += 2) {
    const int t1 = geom_type[(*pairs)[p]], t2 = geom_type[(*pairs)[p + 1]];
    const bool ok = (t1 == SG_GEOM_PLANE && (t2 == SG_GEOM_SPHERE || t2 == SG_GEOM_CAPSULE || t2 == SG_GEOM_BOX)) ||
                    ((t1 == SG_GEOM_SPHERE || t1 == SG_GEOM_CAPSULE || t1 == SG_GEOM_BOX) && t2 == SG_GEOM_BOX);
    if (!ok) { *err = "unsupported collision pair types " + std::to_string(t1) + "-" + std::to_string(t2); pairs->clear(); return false; }
  }
  return true;
}
