// The walk of sg_ray with SG_RAY_SKIN (csrc/sg_ray_walk.h over sg_ray_skin.h + sg_ray.h: the text the kernels compile) under AddressSanitizer
// and UBSan: a stand-alone program, nothing of it is loaded into python.  tests/test_ray_skin_host.py builds and runs it:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I soft-grip_amd/csrc scripts/sanitize/ray_skin_main.cpp
// Skins: none at all, one face, and the limits (256 vertices, 512 faces); every array has exactly the size the walk may read, so one
// element past an end is a report.  Both reduction orders (the two kernel layouts) must agree bit for bit.
#include <cstdio>
#include <cstring>
#include <vector>

#include "sg_ray_walk.h"

struct Scene {
  int ng = 0, nvert = 0, nface = 0;
  std::vector<double> recs, verts;   // [ng][SGY_REC], [nvert][3] (world)
  std::vector<int> hidden, vbody;    // [ng], [nvert]
  std::vector<uint32_t> faces;       // [nface]
};

// one ray through the shared walk (csrc/sg_ray_walk.h: the text the kernels compile); layout: which kernel layout's walkers
static void walk(const Scene& S, int layout, const double* o_in, const double* d_in, int excl, int cat_mask, double limit, double* dist, int* geom, double* n) {
  SgywHostGeoms G = {S.recs.data(), S.hidden.data(), S.ng};
  const SgywSkin K = {S.verts.data(), S.faces.data(), S.vbody.data(), S.nface};
  sgyw_host_ray(G, K, layout, nullptr, nullptr, o_in, d_in, excl, cat_mask, limit, dist, geom, n);
}

// a closed-ish surface: a (rows x cols) grid of vertices wrapped on a unit sphere about (0, 0, 1), two triangles per cell, wound outward
static Scene grid_skin(int rows, int cols, int nface_cap, int ngeom) {
  Scene S;
  S.ng = ngeom;
  S.recs.assign((size_t)ngeom * SGY_REC, 0.0);
  S.hidden.assign(ngeom, 0);
  for (int g = 0; g < ngeom; g++) {   // spheres of radius 0.1 well inside and beside the surface; every second one hidden
    double* r = &S.recs[(size_t)SGY_REC * g];
    r[0] = 0.3 * (g % 3 - 1); r[1] = 0.3 * (g % 5 - 2); r[2] = 1.0 + 2.5 * (g % 2);
    r[3] = r[7] = r[11] = 1.0;
    r[12] = 0.1;
    r[15] = sgy_meta_word(sgy_meta(SGY_SPHERE, g % 5, 1 + g));
    S.hidden[g] = g & 1;
  }
  S.nvert = rows * cols;
  const double pi = 3.14159265358979323846;
  for (int i = 0; i < rows; i++)
    for (int j = 0; j < cols; j++) {
      const double th = pi * (i + 0.5) / rows, ph = 2.0 * pi * j / cols;
      S.verts.push_back(sin(th) * cos(ph)); S.verts.push_back(sin(th) * sin(ph)); S.verts.push_back(1.0 + cos(th));
      S.vbody.push_back(100 + (i * cols + j) % 7);
    }
  for (int i = 0; i + 1 < rows; i++)
    for (int j = 0; j < cols; j++) {
      const int a = i * cols + j, b = i * cols + (j + 1) % cols, c = (i + 1) * cols + j, e = (i + 1) * cols + (j + 1) % cols;
      if ((int)S.faces.size() < nface_cap) S.faces.push_back((uint32_t)a | ((uint32_t)c << 8) | ((uint32_t)b << 16));
      if ((int)S.faces.size() < nface_cap) S.faces.push_back((uint32_t)b | ((uint32_t)c << 8) | ((uint32_t)e << 16));
    }
  while ((int)S.faces.size() < nface_cap && !S.faces.empty()) S.faces.push_back(S.faces[S.faces.size() % 7]);   // (coincident faces: up to the cap)
  S.nface = (int)S.faces.size();
  return S;
}

int main() {
  std::vector<Scene> scenes;
  scenes.push_back(grid_skin(0, 0, 0, 3));        // no skin
  {
    Scene one = grid_skin(0, 0, 0, 0);            // one face, no geoms
    one.nvert = 3; one.nface = 1;
    one.verts = {-1, -0.25, -1, 2, -0.25, -1, -1, -0.25, 2};
    one.vbody = {1, 1, 1};
    one.faces = {0u | (1u << 8) | (2u << 16)};
    scenes.push_back(one);
  }
  scenes.push_back(grid_skin(16, 16, 512, 8));    // the limits: 256 vertices, 512 faces
  unsigned long long sum = 0;
  int hits = 0, skin_hits = 0, total = 0;
  unsigned seed = 12345u;
  auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return (double)(seed >> 8) / (double)(1u << 24); };
  for (const Scene& S : scenes) {
    if (S.nvert > SGYS_MAXVERT || S.nface > SGYS_MAXFACE) return 2;
    for (int q = 0; q < 600; q++) {
      double o[3] = {6.0 * rnd() - 3.0, 6.0 * rnd() - 3.0, 5.0 * rnd() - 1.0}, tgt[3] = {rnd() - 0.5, rnd() - 0.5, 0.5 + rnd()};
      if (q % 50 == 0 && S.nvert) for (int c = 0; c < 3; c++) tgt[c] = S.verts[3 * (q % S.nvert) + c];   // exactly at a vertex
      double d[3] = {tgt[0] - o[0], tgt[1] - o[1], tgt[2] - o[2]};
      if (q == 7) d[0] = d[1] = d[2] = 0.0;
      if (q == 8) d[1] = NAN;
      if (q == 9) d[2] = INFINITY;
      const int excl = q % 4 == 0 ? 100 + q % 7 : (q % 4 == 1 ? 1 + q % 8 : -1);
      const int mask = q % 6 == 5 ? 31 & ~(1 << SGYS_CAT_ELEM) : 31;
      const double limit = q % 3 == 0 ? 3.0 : INFINITY;
      double dist[2], n[2][3];
      int geom[2];
      for (int layout = 0; layout < 2; layout++) walk(S, layout, o, d, excl, mask, limit, &dist[layout], &geom[layout], n[layout]);
      if (memcmp(&dist[0], &dist[1], 8) || geom[0] != geom[1] || memcmp(n[0], n[1], 24)) {
        printf("the two reduction orders differ on ray %d: %.17g / %d against %.17g / %d\n", q, dist[0], geom[0], dist[1], geom[1]);
        return 1;
      }
      total++;
      hits += geom[0] >= 0;
      skin_hits += geom[0] >= S.ng;
      unsigned long long bits;
      memcpy(&bits, &dist[0], 8);
      sum = sum * 31 + bits + (unsigned)geom[0];
    }
  }
  printf("ray_skin_main: %d rays, %d hits, %d on a skin, checksum %016llx\n", total, hits, skin_hits, sum);
  return skin_hits > 0 ? 0 : 3;
}
