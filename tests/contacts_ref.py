"""Helpers of the contact read-out tests: the g++ build of csrc/sg_contacts.h run pair by pair as the kernel runs it (broadphase over the
pair table in order, narrowphase per survivor, the cap), the oracle's list for a given qpos, and the comparison both test files use."""
import ctypes as C
import os
import subprocess

import numpy as np

import render_ref as R

TOL = 1e-9          # absolute, on dist / pos / frame: the project's per-step sensor tolerance (both sides are fp64 restatements of one formula)

HOST_DRIVER = r"""
#include <cstring>
#include <string>
#include <vector>
#include "sg_contacts.h"
extern "C" int contacts_host_npairs(int nbody, int ngeom, const int* par, const int* weld, const int* gadr, const int* gnum, const int* gbody,
                                    const int* gtype, const int* ctype, const int* caff) {
  std::vector<int> pairs;
  std::string err;
  if (!sgc_build_pairs(nbody, ngeom, par, weld, gadr, gnum, gbody, gtype, ctype, caff, &pairs, &err)) return -1;
  return (int)(pairs.size() / 2);
}
// the kernel's flow, serially: returns ncon (min(records, cap)); writes the first min(ncon, max_contacts) contacts
extern "C" int contacts_host(int nbody, int ngeom, const int* par, const int* weld, const int* gadr, const int* gnum, const int* gbody, const int* gtype,
                             const int* ctype, const int* caff, const double* gmargin, const double* grb, const double* gsize, int nconmax,
                             const double* gx, const double* gm, int max_contacts, int* geom, double* dist, double* pos, double* frame) {
  std::vector<int> pairs;
  std::string err;
  if (!sgc_build_pairs(nbody, ngeom, par, weld, gadr, gnum, gbody, gtype, ctype, caff, &pairs, &err)) return -2;
  const int cap = sgc_cap(nconmax);
  int total = 0;
  for (size_t p = 0; p < pairs.size() / 2 && total < cap; p++) {
    const int g1 = pairs[2 * p], g2 = pairs[2 * p + 1], t1 = gtype[g1], t2 = gtype[g2];
    const double margin = gmargin[g1] > gmargin[g2] ? gmargin[g1] : gmargin[g2];
    if (!sgc_broad(t1, gx + 3 * g1, gm + 9 * g1, gx + 3 * g2, grb[g1], grb[g2], margin)) continue;
    sgm::ConRec rec[SGC_MAXREC];
    double poly[16][3], tmp[16][3];
    int n;
    if (t1 == SG_GEOM_BOX)
      n = sgm::gen_box_box(gx + 3 * g1, gm + 9 * g1, gsize + 3 * g1, gx + 3 * g2, gm + 9 * g2, gsize + 3 * g2, margin, rec, poly, tmp);
    else
      n = sgc_narrow(t1, t2, gx + 3 * g1, gm + 9 * g1, gsize + 3 * g1, gx + 3 * g2, gm + 9 * g2, gsize + 3 * g2, margin, rec);
    for (int c = 0; c < n; c++, total++) {
      if (total >= cap || total >= max_contacts) continue;
      geom[2 * total] = g1; geom[2 * total + 1] = g2;
      dist[total] = rec[c].dist;
      memcpy(pos + 3 * total, rec[c].pos, 24);
      sgc_frame(t1, t2, gm + 9 * g2, rec[c].n, frame + 9 * total);
    }
  }
  return total < cap ? total : cap;
}
"""


def build_host(tmpdir):
    """compiles sg_contacts.h with g++ into tmpdir -> the ctypes library with contacts_host / contacts_host_npairs"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(tmpdir, "contacts_host.cpp")
    so = os.path.join(tmpdir, "libcontacts_host.so")
    with open(src, "w") as f:
        f.write(HOST_DRIVER)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(root, "soft-grip_amd", "csrc"), "-o", so, src])
    return C.CDLL(so)


def _model_args(m):
    a = lambda x: np.ascontiguousarray(x, dtype=np.int32)  # noqa: E731
    arrs = [a(m.body_parentid), a(m.body_weldid), a(m.body_geomadr), a(m.body_geomnum), a(m.geom_bodyid), a(m.geom_type), a(m.geom_contype),
            a(m.geom_conaffinity)]
    return arrs


def host_npairs(L, m):
    arrs = _model_args(m)
    return L.contacts_host_npairs(C.c_int(m.nbody), C.c_int(m.ngeom), *[x.ctypes.data_as(C.c_void_p) for x in arrs])


def host_contacts(L, m, qpos, max_contacts=512):
    """the host build's list at qpos (geom poses from Model.kinematics): dict ncon, geom [n, 2], dist [n], pos [n, 3], frame [n, 9]"""
    gx, gm = R.geom_poses(m, qpos)
    d = lambda x: np.ascontiguousarray(x, dtype=np.float64)  # noqa: E731
    arrs = _model_args(m) + [d(m.geom_margin), d(m.geom_rbound), d(m.geom_size)]
    gx, gm = d(gx), d(np.reshape(gm, (-1, 9)))
    geom = np.zeros((max_contacts, 2), np.int32)
    dist, pos, frame = np.zeros(max_contacts), np.zeros((max_contacts, 3)), np.zeros((max_contacts, 9))
    p = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    n = L.contacts_host(C.c_int(m.nbody), C.c_int(m.ngeom), *[p(x) for x in arrs], C.c_int(int(m.nconmax)), p(gx), p(gm), C.c_int(max_contacts),
                        p(geom), p(dist), p(pos), p(frame))
    assert n >= 0, n
    k = min(n, max_contacts)
    return dict(ncon=n, geom=geom[:k], dist=dist[:k], pos=pos[:k], frame=frame[:k])


def oracle_contacts(sim, qpos=None):
    """the oracle's forward(); contacts() at qpos (None: its own), in the same dict layout; the sim's qpos is left at qpos"""
    if qpos is not None:
        sim.qpos[:] = qpos
    sim.forward()
    cs = sim.contacts()
    n = len(cs)
    return dict(ncon=n, geom=np.array([(c["geom1"], c["geom2"]) for c in cs], np.int32).reshape(n, 2), dist=np.array([c["dist"] for c in cs]),
                pos=np.array([c["pos"] for c in cs]).reshape(n, 3), frame=np.array([c["frame"] for c in cs]).reshape(n, 9))


def same_list(a, b):
    """the discrete part of two lists: count and geom pairs entry by entry"""
    return a["ncon"] == b["ncon"] and a["geom"].shape == b["geom"].shape and bool((a["geom"] == b["geom"]).all())


def compare(got, ref, what, verbose=False):
    """counts and geom pairs exact, dist / pos / frame within TOL absolute; returns the largest deviation"""
    assert got["ncon"] == ref["ncon"], "%s: ncon %d, the oracle has %d" % (what, got["ncon"], ref["ncon"])
    n = len(got["geom"])
    assert n == min(ref["ncon"], n)
    assert (got["geom"] == ref["geom"][:n]).all(), "%s: geom pairs differ at entries %s" % (what, np.flatnonzero((got["geom"] != ref["geom"][:n]).any(1))[:8])
    err = 0.0
    for key in ("dist", "pos", "frame"):
        if n:
            e = float(np.abs(got[key] - ref[key][:n]).max())
            err = max(err, e)
            assert e <= TOL, "%s: %s off by %.3g (tolerance %.1g)" % (what, key, e, TOL)
    if verbose:
        print("%s: ncon %d, max deviation %.3g" % (what, ref["ncon"], err))
    return err
