// sg_smooth.h -- the per-env arithmetic of the mass-matrix, joint-force and inverse-dynamics read-outs (sg_get_mass_matrix,
// sg_get_joint_forces, sg_inverse_dynamics): the smooth table beside the kinematics and dynamics tables, and what one lane does for one
// body, one dof.  Pure functions of their arguments, compiled for gfx950 (sg_smooth_kernel.h, inside sg_readout.hip) and by g++ for the
// CPU tests (tests/smooth_ref.py), which drive the same text body by body and dof by dof through sgs_host_env (sg_readout_host.h).
//
// Definitions.  Everything is in world axes, and every moment, every angular momentum and every inertia is taken ABOUT THE WORLD ORIGIN,
// so a parent gathers its children by plain addition.  A body's record is 29 doubles:
//    0 .. 12   xpos, xquat, angular velocity, linear velocity of the origin: sgd_body's record, operation by operation
//   13 .. 18   after the forward walk: the angular acceleration and the acceleration of the body frame's origin, with the world
//              accelerating at -gravity (gravity enters as a fictitious force, as in mj_rne);
//              after sgs_body_force: the moment and the force m a_com that the body's own motion takes, then its subtree's
//   19 .. 28   mass, first moment m xipos, inertia about the world origin (xx xy xz yy yz zz): the body's, then its subtree's composite
// A dof's record is 7 doubles: its motion axis as a twist -- the angular part u and the linear velocity at the world origin (anchor x u
// for a hinge; 0, u for a slider; a free joint's linear dofs along the world axes, its angular dofs about the body's own axes through
// xpos) -- and the Newton-Euler force of the dof.  A spatial force (n, f) does the work u . n + lin . f on such a twist.
#pragma once
#include "sg_dyn.h"

#define SGS_REC 29
#define SGS_ACC 13   // a record's acceleration, then force, slots
#define SGS_INR 19   // a record's inertia slots
#define SGS_DOF 7    // (sgs_body writes slots 0 .. 5 of a dof record and never slot 6: sg_point.h keeps its stamp there)
// The kernel's LDS block: nbody records, nv dof records and two doubles per tendon beside its static LDS (SGS_STATIC_LDS bytes: the
// block-wide __syncthreads_or; the kept assembly's figure, held by tests/test_smooth_host.py).  A gfx950 workgroup gets 160 KB when the
// launch asks for it: 1024 dofs and 128 tendons leave room for 449 bodies.
#define SGS_STATIC_LDS 256
#define SGS_LDS_MAX 163840
#define SGS_MAXDOF 1024
#define SGS_MAXTENDON 128
#define SGS_MAXBODY ((SGS_LDS_MAX - SGS_STATIC_LDS - 8 * (SGS_DOF * SGS_MAXDOF + 2 * SGS_MAXTENDON)) / (SGS_REC * 8))

// ---- the smooth table: one double and one int array, sections at the offsets below ----
struct SgSmoothOff {
  int nu, nspatial;   // actuators; tendons of site wraps (0: the tendon forces need no walk over the bodies)
  // doubles
  int ddamp, tdamp, again, abias, agear;
  // ints
  int dbody, dpar, atrn, cstart, child;
};

struct SgSmoothHost {
  bool ok = false;
  std::string err;
  SgSmoothOff o;
  std::vector<double> dbl;
  std::vector<int> ints;
};

// the table from the blob (K, Dn: the model's kinematics and dynamics tables, whose bodies, joints, dofs and tendons it indexes): per dof
// its damping, its body and its parent dof; per tendon its damping; the actuators; every body's children in ascending order.  S->ok says
// whether the three read-outs can run the model
void sgs_build(const void* blob, size_t nbytes, const SgKinHost& K, const SgDynHost& Dn, SgSmoothHost* S);

__host__ __device__ inline double sgs_dot(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// the world's record: at rest at the origin, accelerating at -gravity
__host__ __device__ inline void sgs_world(const double* DD, const SgDynOff& d, double* rec) {
  for (int k = 0; k < SGS_REC; k++) rec[k] = 0.0;
  rec[3] = 1.0;
  for (int k = 0; k < 3; k++) rec[SGS_ACC + 3 + k] = -DD[d.grav + k];
}

// body i from its parent's record par[29] -> out[0 .. 18] and the twists of the body's dofs in S.  Pose and twist are sgd_body's walk;
// the acceleration rides along: it starts as the parent's carried to this body's origin and gains every joint's share as the joint is
// passed -- u qacc, and the rate of change of the joint's axis, which turns with the frame the joint sits in.  qacc NULL: zero
__host__ __device__ inline void sgs_body(const double* D, const int* I, const SgKinOff& o, const double* DD, const SgDynOff& d, const int* jdof, const double* qpos,
                                         const double* qvel, const double* qacc, int i, const double* par, double* out, double* S) {
  const double *pp = par, *pq = par + 3;
  double R[9], t[3], pos[3], quat[4], w[3], v[3], al[3], a[3], c[3], c2[3];
  sgk_quat_mat(R, pq);
  sgk_mv(t, R, D + o.bpos + 3 * i);
  for (int k = 0; k < 3; k++) pos[k] = pp[k] + t[k];
  sgk_quat_mul(quat, pq, D + o.bquat + 4 * i);
  sgd_cross(c, par + 7, t);   // the parent's twist and acceleration at pos: a + al x t + w x (w x t)
  for (int k = 0; k < 3; k++) { w[k] = par[7 + k]; v[k] = par[10 + k] + c[k]; }
  sgd_cross(c2, par + 7, c);
  sgd_cross(c, par + SGS_ACC, t);
  for (int k = 0; k < 3; k++) { al[k] = par[SGS_ACC + k]; a[k] = par[SGS_ACC + 3 + k] + c[k] + c2[k]; }
  const int j0 = I[o.bjadr + i], nj = I[o.bjnum + i];
  for (int j = j0; j < j0 + nj; j++) {
    const int type = I[o.jtype + j], qa = I[o.jqadr + j], da = jdof[j];
    double* Sj = S + SGS_DOF * da;
    if (type == SG_JNT_FREE) {   // as sgd_body: linear in the world frame, angular in the body's; d/dt (R w_b) = R d/dt w_b, as w x w = 0
      for (int k = 0; k < 3; k++) pos[k] = qpos[qa + k];
      for (int k = 0; k < 4; k++) quat[k] = qpos[qa + 3 + k];
      sgk_quat_normalize(quat);
      sgk_quat_mat(R, quat);
      sgk_mv(w, R, qvel + da + 3);
      for (int k = 0; k < 3; k++) v[k] = qvel[da + k];
      const double z[3] = {0.0, 0.0, 0.0};
      sgk_mv(al, R, qacc ? qacc + da + 3 : z);
      for (int k = 0; k < 3; k++) a[k] = -DD[d.grav + k] + (qacc ? qacc[da + k] : 0.0);
      for (int k = 0; k < 3; k++) {
        double* Sl = Sj + SGS_DOF * k;
        double* Sa = Sj + SGS_DOF * (3 + k);
        const double u[3] = {R[k], R[3 + k], R[6 + k]};   // the body's own axis k
        for (int e = 0; e < 3; e++) { Sl[e] = 0.0; Sl[3 + e] = e == k ? 1.0 : 0.0; Sa[e] = u[e]; }
        sgd_cross(Sa + 3, pos, u);
      }
      continue;
    }
    const double* jp = D + o.jpos + 3 * j;
    const double* ja = D + o.jaxis + 3 * j;
    double anchor[3], axis[3], wu[3];
    sgk_quat_mat(R, quat);
    sgk_mv(t, R, jp);
    for (int k = 0; k < 3; k++) anchor[k] = pos[k] + t[k];
    sgk_mv(axis, R, ja);
    const double dq = qpos[qa] - D[o.jq0 + j], qd = qvel[da], qdd = qacc ? qacc[da] : 0.0;
    sgd_cross(wu, w, axis);   // the axis' rate of change
    if (type == SG_JNT_SLIDE) {
      // d2/dt2 (axis dq) = (al x axis + w x (w x axis)) dq + 2 (w x axis) qd + axis qdd
      sgd_cross(c, al, axis);
      sgd_cross(c2, w, wu);
      for (int k = 0; k < 3; k++) {
        pos[k] = pos[k] + axis[k] * dq;
        v[k] += axis[k] * qd + wu[k] * dq;
        a[k] += (c[k] + c2[k]) * dq + 2.0 * wu[k] * qd + axis[k] * qdd;
        Sj[k] = 0.0; Sj[3 + k] = axis[k];
      }
    } else {
      // the anchor as a point of the body before this hinge; behind the hinge the origin turns about it at w + axis qd, al + axis qdd + (w x axis) qd
      sgd_cross(c, w, t);
      sgd_cross(c2, w, c);
      for (int k = 0; k < 3; k++) v[k] += c[k];
      sgd_cross(c, al, t);
      for (int k = 0; k < 3; k++) a[k] += c[k] + c2[k];
      for (int k = 0; k < 3; k++) { al[k] += axis[k] * qdd + wu[k] * qd; w[k] += axis[k] * qd; Sj[k] = axis[k]; }
      sgd_cross(Sj + 3, anchor, axis);
      const double s = sin(dq / 2);
      const double ql[4] = {cos(dq / 2), ja[0] * s, ja[1] * s, ja[2] * s};
      double qn[4];
      sgk_quat_mul(qn, quat, ql);
      for (int k = 0; k < 4; k++) quat[k] = qn[k];
      sgk_quat_mat(R, quat);
      sgk_mv(t, R, jp);
      for (int k = 0; k < 3; k++) pos[k] = anchor[k] - t[k];
      sgd_cross(c, w, t);
      sgd_cross(c2, w, c);
      for (int k = 0; k < 3; k++) v[k] -= c[k];
      sgd_cross(c, al, t);
      for (int k = 0; k < 3; k++) a[k] -= c[k] + c2[k];
    }
  }
  sgk_quat_normalize(quat);
  for (int k = 0; k < 3; k++) out[k] = pos[k];
  for (int k = 0; k < 4; k++) out[3 + k] = quat[k];
  for (int k = 0; k < 3; k++) { out[7 + k] = w[k]; out[10 + k] = v[k]; out[SGS_ACC + k] = al[k]; out[SGS_ACC + 3 + k] = a[k]; }
}

// body i's own Newton-Euler force and inertia from its pose, twist and acceleration: rec[13 .. 18] becomes the moment about the world
// origin and the force, n = R (I al_b + w_b x I w_b) + xipos x f, f = m (a + al x c + w x (w x c)), c = xipos - xpos;
// rec[19 .. 28] its mass, m xipos and R I R' + m (|xipos|^2 E - xipos xipos')
__host__ __device__ inline void sgs_body_force(const double* DD, const SgDynOff& d, double* rec, int i) {
  double R[9], c[3], xi[3], t1[3], t2[3], t3[3], f[3], wl[3], all[3], Iw[3], Ia[3], nl[3], n[3];
  const double m = DD[d.bmass + i];
  const double* Ib = DD + d.bimat + 9 * i;
  const double *w = rec + 7, *al = rec + SGS_ACC, *a = rec + SGS_ACC + 3;
  sgk_quat_mat(R, rec + 3);
  sgk_mv(c, R, DD + d.bipos + 3 * i);
  for (int k = 0; k < 3; k++) xi[k] = rec[k] + c[k];
  sgd_cross(t1, al, c);
  sgd_cross(t2, w, c);
  sgd_cross(t3, w, t2);
  for (int k = 0; k < 3; k++) f[k] = m * (a[k] + t1[k] + t3[k]);
  for (int k = 0; k < 3; k++) {   // R' w, R' al: the body's frame
    wl[k] = R[k] * w[0] + R[3 + k] * w[1] + R[6 + k] * w[2];
    all[k] = R[k] * al[0] + R[3 + k] * al[1] + R[6 + k] * al[2];
  }
  sgk_mv(Iw, Ib, wl);
  sgk_mv(Ia, Ib, all);
  sgd_cross(t1, wl, Iw);
  for (int k = 0; k < 3; k++) nl[k] = Ia[k] + t1[k];
  sgk_mv(n, R, nl);
  sgd_cross(t1, xi, f);
  for (int k = 0; k < 3; k++) { rec[SGS_ACC + k] = n[k] + t1[k]; rec[SGS_ACC + 3 + k] = f[k]; }
  double RI[9], Iw9[9];
  for (int r = 0; r < 3; r++)
    for (int k = 0; k < 3; k++) RI[3 * r + k] = R[3 * r] * Ib[k] + R[3 * r + 1] * Ib[3 + k] + R[3 * r + 2] * Ib[6 + k];
  for (int r = 0; r < 3; r++)
    for (int k = r; k < 3; k++) Iw9[3 * r + k] = RI[3 * r] * R[3 * k] + RI[3 * r + 1] * R[3 * k + 1] + RI[3 * r + 2] * R[3 * k + 2];
  const double x2 = sgs_dot(xi, xi);
  double* J = rec + SGS_INR;
  J[0] = m;
  for (int k = 0; k < 3; k++) J[1 + k] = m * xi[k];
  J[4] = Iw9[0] + m * (x2 - xi[0] * xi[0]); J[5] = Iw9[1] - m * xi[0] * xi[1]; J[6] = Iw9[2] - m * xi[0] * xi[2];
  J[7] = Iw9[4] + m * (x2 - xi[1] * xi[1]); J[8] = Iw9[5] - m * xi[1] * xi[2];
  J[9] = Iw9[8] + m * (x2 - xi[2] * xi[2]);
}

// body i gathers its children: slots [from, from + count) of its record gain the children's, in the child list's (ascending) order.
// Run level by level from the leaves, it leaves every body with its subtree's sums
__host__ __device__ inline void sgs_gather(const int* SI, const SgSmoothOff& s, double* recs, int i, int from, int count) {
  double* me = recs + SGS_REC * i + from;
  for (int k = SI[s.cstart + i]; k < SI[s.cstart + i + 1]; k++) {
    const double* ch = recs + SGS_REC * SI[s.child + k] + from;
    for (int e = 0; e < count; e++) me[e] += ch[e];
  }
}

// the work of the spatial force F = (moment about the world origin, force) on dof twist Sd
__host__ __device__ inline double sgs_project(const double* Sd, const double* F) { return sgs_dot(Sd, F) + sgs_dot(Sd + 3, F + 3); }

// the momentum (angular about the world origin, linear) that the inertia J[10] has when it moves with twist Sd
__host__ __device__ inline void sgs_momentum(const double* J, const double* Sd, double* F) {
  const double *u = Sd, *l = Sd + 3, *h = J + 1;
  double hl[3], uh[3];
  sgd_cross(hl, h, l);
  sgd_cross(uh, u, h);
  F[0] = J[4] * u[0] + J[5] * u[1] + J[6] * u[2] + hl[0];
  F[1] = J[5] * u[0] + J[7] * u[1] + J[8] * u[2] + hl[1];
  F[2] = J[6] * u[0] + J[8] * u[1] + J[9] * u[2] + hl[2];
  for (int k = 0; k < 3; k++) F[3 + k] = J[0] * l[k] + uh[k];
}

// row i and column i of the mass matrix up to the diagonal (composite rigid body): M[i][c] = M[c][i] for every c <= i -- twist c on the
// momentum of dof i's composite inertia where dof c is dof i or one of its ancestors, plus the armature on the diagonal; zero elsewhere.
// Every pair is computed once and stored twice; over all i every entry of M[nv][nv] is written exactly once
__host__ __device__ inline void sgs_mass_row(const int* SI, const SgSmoothOff& s, const double* DD, const SgDynOff& d, const double* recs, const double* S, int i,
                                             double* M) {
  double F[6];
  sgs_momentum(recs + SGS_REC * SI[s.dbody + i] + SGS_INR, S + SGS_DOF * i, F);
  const size_t nv = d.nv;
  int j = i;   // the next ancestor dof on the way down the columns
  for (int c = i; c >= 0; c--) {
    double val = 0.0;
    if (c == j) {
      val = sgs_project(S + SGS_DOF * c, F);
      if (c == i) val += DD[d.arm + i];
      j = SI[s.dpar + j];
    }
    M[i * nv + c] = val;
    M[c * nv + i] = val;
  }
}

// share s of tendon t, sgd_wrap's arithmetic on this header's records: a fixed tendon's coef q and coef qvel, a spatial tendon's segment
__host__ __device__ inline void sgs_wrap(const int* I, const SgKinOff& o, const double* DD, const int* DI, const SgDynOff& d, const double* qpos, const double* qvel,
                                         const double* recs, int w, double* len, double* vel) {
  const int obj = DI[d.wobj + w];
  if (DI[d.wtype + w] == SG_WRAP_JOINT) {
    const double coef = DD[d.wprm + w];
    *len = coef * qpos[I[o.jqadr + obj]];
    *vel = coef * qvel[DI[d.jdof + obj]];
    return;
  }
  const int s1 = DI[d.wobj + w + 1];
  double p0[3], v0[3], p1[3], v1[3];
  sgd_point(recs + SGS_REC * DI[d.sbody + obj], DD + d.spos + 3 * obj, p0, v0);
  sgd_point(recs + SGS_REC * DI[d.sbody + s1], DD + d.spos + 3 * s1, p1, v1);
  const double dx[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};
  const double L = sqrt(dx[0] * dx[0] + dx[1] * dx[1] + dx[2] * dx[2]);
  *len = L;
  *vel = L < 1e-15 ? 0.0 : (dx[0] * (v1[0] - v0[0]) + dx[1] * (v1[1] - v0[1]) + dx[2] * (v1[2] - v0[2])) / L;
}

// the two scalar forces along tendon t from its length and velocity: ft[0] the passive one, -k (L - lengthspring) - damping Ldot, k the
// stiffness this env's next step uses; ft[1] the actuators', sum over the actuators on t of gear (gain act + bias0 + bias1 gear L + bias2 gear Ldot)
__host__ __device__ inline void sgs_tendon_force(const double* SD, const int* SI, const SgSmoothOff& s, const double* DD, const SgDynOff& d, const double* act, int t,
                                                 double L, double Ld, int masked, double kenv, double* ft) {
  const double k = masked ? kenv : DD[d.tstiff + t];
  ft[0] = -k * (L - DD[d.tspring + t]) - SD[s.tdamp + t] * Ld;
  double fa = 0.0;
  for (int u = 0; u < s.nu; u++) {
    if (SI[s.atrn + u] != t) continue;
    const double g = SD[s.agear + u], *b = SD + s.abias + 3 * u;
    fa += g * (SD[s.again + u] * act[u] + b[0] + b[1] * (g * L) + b[2] * (g * Ld));
  }
  ft[1] = fa;
}

// what the spatial tendons' forces do to body i: rec[13 .. 24] becomes (moment about the world origin, force) of the passive forces,
// then of the actuators'.  A segment site a -> site b of unit vector e pulls site b's body by ft e at site b and site a's by -ft e at
// site a (the transpose of sgd_wrap's velocity); a segment shorter than 1e-15 pulls nothing.  Tendons and segments in ascending order
__host__ __device__ inline void sgs_body_tendons(const double* DD, const int* DI, const SgDynOff& d, const double* ften, double* recs, int i) {
  double acc[12];
  for (int k = 0; k < 12; k++) acc[k] = 0.0;
  for (int t = 0; t < d.ntendon; t++) {
    const int w0 = DI[d.tadr + t], n = DI[d.tnum + t];
    if (DI[d.wtype + w0] == SG_WRAP_JOINT) continue;
    for (int w = w0; w < w0 + n - 1; w++) {
      const int sa = DI[d.wobj + w], sb = DI[d.wobj + w + 1], ba = DI[d.sbody + sa], bb = DI[d.sbody + sb];
      if (ba != i && bb != i) continue;
      double p0[3], v0[3], p1[3], v1[3], e[3], m0[3], m1[3];
      sgd_point(recs + SGS_REC * ba, DD + d.spos + 3 * sa, p0, v0);
      sgd_point(recs + SGS_REC * bb, DD + d.spos + 3 * sb, p1, v1);
      const double dx[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};
      const double L = sqrt(dx[0] * dx[0] + dx[1] * dx[1] + dx[2] * dx[2]);
      if (L < 1e-15) continue;
      for (int k = 0; k < 3; k++) e[k] = dx[k] / L;
      sgd_cross(m0, p0, e);
      sgd_cross(m1, p1, e);
      for (int c = 0; c < 2; c++) {
        const double ft = ften[2 * t + c];
        double* A = acc + 6 * c;
        if (bb == i)
          for (int k = 0; k < 3; k++) { A[k] += ft * m1[k]; A[3 + k] += ft * e[k]; }
        if (ba == i)
          for (int k = 0; k < 3; k++) { A[k] -= ft * m0[k]; A[3 + k] -= ft * e[k]; }
      }
    }
  }
  for (int k = 0; k < 12; k++) recs[SGS_REC * i + SGS_ACC + k] = acc[k];
}

// dof i's passive and actuator force: out[0] = the joint's spring -k (q - qpos_spring) (slide and hinge) - dof_damping qvel + the
// tendons' passive forces; out[1] = the actuators' through their tendons.  A fixed tendon gives coef ft at its joints' dofs; the spatial
// ones come as the body's gathered spatial forces rec[13 .. 24] (sgs_body_tendons, sgs_gather), where the model has any
__host__ __device__ inline void sgs_dof_applied(const double* SD, const int* SI, const SgSmoothOff& s, const int* I, const SgKinOff& o, const double* DD, const int* DI,
                                                const SgDynOff& d, const double* qpos, const double* qvel, const double* recs, const double* S, const double* ften,
                                                const int* kmask_jnt, double kenv, int i, double* out) {
  double fp = -SD[s.ddamp + i] * qvel[i], fa = 0.0;
  const int body = SI[s.dbody + i];
  for (int j = I[o.bjadr + body]; j < I[o.bjadr + body] + I[o.bjnum + body]; j++)
    if (DI[d.jdof + j] == i && I[o.jtype + j] != SG_JNT_FREE) {
      const double k = kmask_jnt[j] ? kenv : DD[d.jstiff + j];
      fp += -k * (qpos[I[o.jqadr + j]] - DD[d.jspring + j]);
    }
  for (int t = 0; t < d.ntendon; t++) {
    const int w0 = DI[d.tadr + t], n = DI[d.tnum + t];
    if (DI[d.wtype + w0] != SG_WRAP_JOINT) continue;
    for (int w = w0; w < w0 + n; w++)
      if (DI[d.jdof + DI[d.wobj + w]] == i) {
        fp += DD[d.wprm + w] * ften[2 * t];
        fa += DD[d.wprm + w] * ften[2 * t + 1];
      }
  }
  if (s.nspatial) {
    const double* F = recs + SGS_REC * body + SGS_ACC;
    fp += sgs_project(S + SGS_DOF * i, F);
    fa += sgs_project(S + SGS_DOF * i, F + 6);
  }
  out[0] = fp; out[1] = fa;
}
