// sg_skin.h -- the skin of a composite (host side): triangles bound to bodies, held by sg_model next to the kinematics table and NOT part of
// the model blob.  One vertex per shell element at (0, 0, inflate) in the element body's frame (its z axis points outward and the element
// geom sits inward with its tip at the body origin: at inflate = 0 the vertices are the outermost points of the collision geoms), the
// faces of the shell's six sides wound outward.  mjcf.py Model.composite_skin() builds the same arrays; tests/test_skin_host.py holds
// the two against each other.  Textures are not drawn and the skin is built as at subgrid = 0.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include "sg_render.h"   // the limits and the face packing

struct SgSkinHost {
  int nvert = 0, nface = 0;
  std::vector<int32_t> vert_body, face;   // [nvert], [nface][3]
  std::vector<double> vert_pos;           // [nvert][3], body frame
  float rgba[4] = {0.8f, 0.2f, 0.1f, 1.0f};
  unsigned version = 0;                   // bumped by every sg_model_set_skin: a batch uploads its tables again when it has moved
};

// "<prefix>B<ix>_<iy>_<iz>" -> prefix and indices (the LAST 'B' that three numbers follow)
inline bool sg_skin_parse_name(const std::string& name, std::string* prefix, int* idx) {
  for (size_t at = name.size(); at-- > 0;) {
    if (name[at] != 'B') continue;
    size_t p = at + 1;
    int got = 0;
    bool ok = true;
    for (int k = 0; k < 3 && ok; k++) {
      size_t q = p;
      long v = 0;
      while (q < name.size() && name[q] >= '0' && name[q] <= '9' && q - p < 6) { v = v * 10 + (name[q] - '0'); q++; }
      if (q == p) { ok = false; break; }
      idx[k] = (int)v; got++;
      p = q;
      if (k < 2) {
        if (p < name.size() && name[p] == '_') p++;
        else ok = false;
      }
    }
    if (ok && got == 3 && p == name.size()) { *prefix = name.substr(0, at); return true; }
  }
  return false;
}

// the skin of the composite whose element bodies are named <prefix>B<ix>_<iy>_<iz> (prefix == nullptr: the first such body's prefix).
// false: no such bodies, or the names do not form a full shell within the limits
inline bool sg_composite_skin(const std::vector<std::string>& body_names, const std::string* prefix, double inflate, const float* rgba, SgSkinHost* S) {
  std::string pre;
  bool have = prefix != nullptr;
  if (prefix) pre = *prefix;
  std::map<std::vector<int>, int> body;
  int count[3] = {0, 0, 0};
  for (size_t i = 0; i < body_names.size(); i++) {
    std::string p;
    int idx[3];
    if (!sg_skin_parse_name(body_names[i], &p, idx)) continue;
    if (!have) { pre = p; have = true; }
    if (p != pre) continue;
    body[{idx[0], idx[1], idx[2]}] = (int)i;
    for (int k = 0; k < 3; k++) count[k] = std::max(count[k], idx[k] + 1);
  }
  if (body.empty() || count[0] < 2 || count[1] < 2 || count[2] < 2) return false;
  std::map<std::vector<int>, int> vert;
  S->vert_body.clear(); S->vert_pos.clear(); S->face.clear();
  for (int ix = 0; ix < count[0]; ix++)
    for (int iy = 0; iy < count[1]; iy++)
      for (int iz = 0; iz < count[2]; iz++) {
        if (!(ix == 0 || ix == count[0] - 1 || iy == 0 || iy == count[1] - 1 || iz == 0 || iz == count[2] - 1)) continue;
        auto it = body.find({ix, iy, iz});
        if (it == body.end()) return false;
        vert[{ix, iy, iz}] = (int)S->vert_body.size();
        S->vert_body.push_back(it->second);
        S->vert_pos.push_back(0.0); S->vert_pos.push_back(0.0); S->vert_pos.push_back(inflate);
      }
  if (S->vert_body.size() != body.size() || S->vert_body.size() > SGR_MAXVERT) return false;
  for (int a = 0; a < 3; a++) {
    const int b = (a + 1) % 3, c = (a + 2) % 3;
    for (int side = 0; side < 2; side++)
      for (int i = 0; i + 1 < count[b]; i++)
        for (int j = 0; j + 1 < count[c]; j++) {
          auto at = [&](int di, int dj) {
            std::vector<int> q(3);
            q[a] = side ? count[a] - 1 : 0; q[b] = i + di; q[c] = j + dj;
            return vert[q];
          };
          const int p00 = at(0, 0), p10 = at(1, 0), p11 = at(1, 1), p01 = at(0, 1);
          const int hi[6] = {p00, p10, p11, p00, p11, p01}, lo[6] = {p00, p11, p10, p00, p01, p11};
          S->face.insert(S->face.end(), side ? hi : lo, (side ? hi : lo) + 6);
        }
  }
  S->nvert = (int)S->vert_body.size();
  S->nface = (int)(S->face.size() / 3);
  if (S->nface > SGR_MAXFACE) return false;
  for (int k = 0; k < 4; k++) S->rgba[k] = rgba[k];
  return true;
}

// the tables the kernels read: faces packed (sgr_pack_face), the vertex -> face adjacency list (ascending face index) and the geoms
// the skin replaces (those of the bodies its vertices are bound to)
struct SgSkinTables {
  std::vector<uint32_t> faces;
  std::vector<int> adj_start, adj, hidden;
};

inline void sg_skin_tables(const SgSkinHost& S, const int* geom_body, int ngeom, int nbody, SgSkinTables* T) {
  T->faces.resize(S.nface);
  T->adj_start.assign(S.nvert + 1, 0);
  for (int f = 0; f < S.nface; f++) {
    T->faces[f] = sgr_pack_face(S.face[3 * f], S.face[3 * f + 1], S.face[3 * f + 2]);
    for (int k = 0; k < 3; k++) T->adj_start[S.face[3 * f + k] + 1]++;
  }
  for (int v = 0; v < S.nvert; v++) T->adj_start[v + 1] += T->adj_start[v];
  T->adj.assign(3 * (size_t)S.nface, 0);
  std::vector<int> fill(T->adj_start.begin(), T->adj_start.end() - 1);
  for (int f = 0; f < S.nface; f++)
    for (int k = 0; k < 3; k++) T->adj[fill[S.face[3 * f + k]]++] = f;
  std::vector<char> bound(nbody, 0);
  for (int v = 0; v < S.nvert; v++) bound[S.vert_body[v]] = 1;
  T->hidden.assign(ngeom, 0);
  for (int g = 0; g < ngeom; g++) T->hidden[g] = bound[geom_body[g]];
}
