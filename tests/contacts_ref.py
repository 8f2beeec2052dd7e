"""Helpers of the contact read-out tests: the g++ build of csrc/sg_contacts.h run pair by pair as the kernel runs it (broadphase over the
pair table in order, narrowphase per survivor, the cap), the oracle's list for a given qpos, and the comparison both test files use."""
import ctypes as C

import numpy as np

import host_build
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
// what the kernel's queue and box - box loop see of a pose: out[0] = broadphase survivors over the whole pair table, out[1] = the most
// box - box pairs in one of the kernel's rounds (round r drains survivors [64 r, 64 r + 64): a window of 64 consecutive survivors)
extern "C" int contacts_host_stats(int nbody, int ngeom, const int* par, const int* weld, const int* gadr, const int* gnum, const int* gbody,
                                   const int* gtype, const int* ctype, const int* caff, const double* gmargin, const double* grb, const double* gx,
                                   const double* gm, int* out) {
  std::vector<int> pairs;
  std::string err;
  if (!sgc_build_pairs(nbody, ngeom, par, weld, gadr, gnum, gbody, gtype, ctype, caff, &pairs, &err)) return -2;
  int nsurv = 0, in_round = 0, most = 0;
  for (size_t p = 0; p < pairs.size() / 2; p++) {
    const int g1 = pairs[2 * p], g2 = pairs[2 * p + 1];
    const double margin = gmargin[g1] > gmargin[g2] ? gmargin[g1] : gmargin[g2];
    if (!sgc_broad(gtype[g1], gx + 3 * g1, gm + 9 * g1, gx + 3 * g2, grb[g1], grb[g2], margin)) continue;
    if (nsurv % 64 == 0) in_round = 0;
    nsurv++;
    if (gtype[g1] == SG_GEOM_BOX && ++in_round > most) most = in_round;
  }
  out[0] = nsurv; out[1] = most;
  return 0;
}
"""


def build_host(tmpdir):
    """compiles sg_contacts.h with g++ into tmpdir -> the ctypes library with contacts_host / contacts_host_npairs"""
    return host_build.build(tmpdir, "contacts_host", HOST_DRIVER)


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


def host_stats(L, m, qpos):
    """(broadphase survivors, most box - box pairs in one of the kernel's rounds of 64 survivors) of the host build at qpos"""
    gx, gm = R.geom_poses(m, qpos)
    d = lambda x: np.ascontiguousarray(x, dtype=np.float64)  # noqa: E731
    arrs = _model_args(m) + [d(m.geom_margin), d(m.geom_rbound), d(gx), d(np.reshape(gm, (-1, 9)))]
    out = np.zeros(2, np.int32)
    rc = L.contacts_host_stats(C.c_int(m.nbody), C.c_int(m.ngeom), *[x.ctypes.data_as(C.c_void_p) for x in arrs], out.ctypes.data_as(C.c_void_p))
    assert rc == 0, rc
    return int(out[0]), int(out[1])


# ---- the pose sweep of the random grippers (tests/test_contacts_host.py on the host build, tests/test_gpu_contacts.py on the device) ----
SWEEP_SEED = 77       # the grippers: successive helpers.random_gripper_xml draws of one RandomState, free = bool(i % 2)
SWEEP_GRIPPERS = 6
SWEEP_POSES = 64      # per gripper, the aligned poses included
SWEEP_ALIGNED = 4
SWEEP_POSE_SEED = 0   # gripper i is swept with seed SWEEP_POSE_SEED + i (with these seeds one gripper's list reaches the model's nconmax)
HINGE_SWING = (0.5, 1.5, 3.0)


def sweep_gripper_xmls():
    """the XML texts of the sweep's grippers"""
    from helpers import random_gripper_xml
    rng = np.random.RandomState(SWEEP_SEED)
    return [random_gripper_xml(rng, free=bool(i % 2)) for i in range(SWEEP_GRIPPERS)]


def pose_sweep(model, n, seed):
    """[n, nq]: qpos0 turned far out of the joint ranges (kinematics does not care; nothing is stepped).  Pose i moves every hinge by up to
    +-HINGE_SWING[i % 3] rad, every slider by up to +-0.02 and a free joint by up to +-0.5 m per axis with a random unit quaternion.
    The last SWEEP_ALIGNED poses are aligned: a pose of the smallest swing with a random half of the hinges at exact multiples of pi / 2,
    so that boxes meet with parallel edges (gen_box_box's parallel-edge skip, its den > 1e-12 guard).  Of the aligned candidates only
    those are kept that aligned_pose_is_posed accepts on the oracle's own list: where the contact normal is an axis of BOTH boxes the
    two face axes tie exactly, the last bit of the kinematics picks the reference box, and with it the order of the pair's records --
    of 240 such poses drawn from qpos0 the g++ build and the oracle disagree on 30, every one of them at such a pair."""
    from helpers import oracle_sim
    rs = np.random.RandomState(seed)
    q0 = np.array(model.qpos0, dtype=np.float64)

    def swept(swing):
        q = q0.copy()
        for j, t in enumerate(model.jnt_type):
            a = int(model.jnt_qposadr[j])
            if t == 3:
                q[a] += rs.uniform(-swing, swing)
            elif t == 2:
                q[a] += rs.uniform(-0.02, 0.02)
            else:
                q[a:a + 3] += rs.uniform(-0.5, 0.5, 3)
                quat = rs.standard_normal(4)
                q[a + 3:a + 7] = quat / np.linalg.norm(quat)
        return q

    qs = [swept(HINGE_SWING[i % 3]) for i in range(n - SWEEP_ALIGNED)]
    hinges = [int(model.jnt_qposadr[j]) for j, t in enumerate(model.jnt_type) if t == 3]
    sim = oracle_sim(model)
    for _ in range(1000):
        if len(qs) == n:
            break
        q = swept(HINGE_SWING[0])
        for a in hinges:
            if rs.rand() < 0.5:
                q[a] = rs.choice([-2, -1, 1, 2]) * (np.pi / 2)
        if aligned_pose_is_posed(model, q, oracle_contacts(sim, q)):
            qs.append(q)
    assert len(qs) == n, "no %d aligned poses among 1000 candidates" % SWEEP_ALIGNED
    return np.array(qs)


def box_pair_flags(model, qpos, ref):
    """of the oracle's list `ref` at qpos: (some contacting box - box pair has two axes parallel to 1e-12, some contacting box - box
    pair's normal is an axis of both boxes to 1e-9: an exact tie between a face of box 1 and a face of box 2)"""
    _, gm = R.geom_poses(model, qpos)
    parallel = tie = False
    for k in range(ref["ncon"]):
        g1, g2 = (int(x) for x in ref["geom"][k])
        if model.geom_type[g1] != 6:
            continue
        nrm = ref["frame"][k, :3]
        on = [bool((np.abs(np.abs(gm[g].T @ nrm) - 1.0) <= 1e-9).any()) for g in (g1, g2)]
        tie |= on[0] and on[1]
        parallel |= bool((np.abs(np.abs(gm[g1].T @ gm[g2]) - 1.0) <= 1e-12).any())
    return parallel, tie


def aligned_pose_is_posed(model, qpos, ref):
    """an aligned candidate is kept when boxes with parallel axes are in contact and no contact normal is an axis of both its boxes"""
    parallel, tie = box_pair_flags(model, qpos, ref)
    return parallel and not tie


PAIR_NAMES = {(0, 2): "plane-sphere", (0, 3): "plane-capsule", (0, 6): "plane-box", (2, 6): "sphere-box", (3, 6): "capsule-box", (6, 6): "box-box"}


def classify(model, qpos, ref):
    """the oracle's list `ref` at qpos by geom pair, from the list and render_ref.geom_poses alone: a list of (pair type name, records,
    class); class is None but for box - box, where it says what the contact normal (first frame row of the pair's first record) is: an
    axis of geom 1 (`face1`), else an axis of geom 2 (`face2`), each to 1e-9, else `edge`"""
    _, gm = R.geom_poses(model, qpos)
    out, i, n = [], 0, ref["ncon"]
    while i < n:
        g1, g2 = (int(x) for x in ref["geom"][i])
        k = i
        while k < n and int(ref["geom"][k, 0]) == g1 and int(ref["geom"][k, 1]) == g2:
            k += 1
        kind, cls = (int(model.geom_type[g1]), int(model.geom_type[g2])), None
        if kind == (6, 6):
            nrm = ref["frame"][i, :3]
            on = lambda g: bool((np.abs(np.abs(gm[g].T @ nrm) - 1.0) <= 1e-9).any())  # noqa: E731  (columns of geom_xmat: the box's axes)
            cls = "face1" if on(g1) else "face2" if on(g2) else "edge"
        out.append((PAIR_NAMES[kind], k - i, cls))
        i = k
    return out


def knife_edge(sim, q, ref, rs):
    """does the oracle's OWN list (count, geom pairs) change under a +-1e-12 perturbation of this qpos?"""
    for _ in range(4):
        if not same_list(oracle_contacts(sim, q + rs.choice([-1e-12, 1e-12], size=q.shape)), ref):
            return True
    return False


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
