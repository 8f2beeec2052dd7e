"""The g++ build of the dyn, smooth, point and solve read-outs' host twins (csrc/sg_readout_host.h: one env serially, in the kernels'
order) on the tables csrc/sg_tables.cpp builds of a model's blob: one thin extern "C" shim for the four families.  dyn_ref, smooth_ref,
point_ref and solve_ref each build it (build(); their BREAKS patch one header of FILES) and call their family's entry through
tables(), the handle of a model's tables, made once per library and model."""
import ctypes as C

import host_build

# what the shim is built from, copied beside it so that a patched header is the one every other file includes
FILES = ("sg_dyn.h", "sg_smooth.h", "sg_point.h", "sg_solve.h", "sg_forces.h", "sg_shape.h", "sg_tables.h", "sg_readout_host.h", "sg_tables.cpp")

HOST_DRIVER = r"""
#include "sg_readout_host.h"
template <class V> static void put(const V& v, void* out) { if (out && !v.empty()) memcpy(out, v.data(), v.size() * sizeof(v[0])); }
template <class H> static int need(const H& t, char* err) { if (!t.ok) strncpy(err, t.err.c_str(), 255); return t.ok ? 0 : -1; }
extern "C" {
void* tables_new(const void* blob, size_t n) {
  SgHostTables* T = new SgHostTables();
  sg_host_tables(blob, n, T);
  return T;
}
void tables_free(void* h) { delete (SgHostTables*)h; }
// every entry: 0, or -1 with the reason in err where the family's table refuses the model
int dyn_host(const void* h, const double* qpos, const double* qvel, double kenv, const int* kmask_jnt, const int* kmask_ten, double* ang, double* lin, double* com_lin,
             double* ten_len, double* ten_vel, double* energy, double* poses, char* err) {
  const SgHostTables& T = *(const SgHostTables*)h;
  if (need(T.dyn, err)) return -1;
  SgdHostOut o;
  sgd_host_env(T, qpos, qvel, kenv, kmask_jnt, kmask_ten, &o);
  put(o.ang, ang); put(o.lin, lin); put(o.com_lin, com_lin); put(o.ten_len, ten_len); put(o.ten_vel, ten_vel); put(o.poses, poses);
  memcpy(energy, o.energy, sizeof o.energy);
  return 0;
}
int smooth_host(const void* h, const double* qpos, const double* qvel, const double* act, const double* qacc, double kenv, const int* kmask_jnt, const int* kmask_ten,
                double* M, double* bias, double* passive, double* actuator, double* inverse, char* err) {
  const SgHostTables& T = *(const SgHostTables*)h;
  if (need(T.smooth, err)) return -1;
  SgsHostOut o;
  sgs_host_env(T, qpos, qvel, act, qacc, kenv, kmask_jnt, kmask_ten, &o);
  put(o.M, M); put(o.bias, bias); put(o.passive, passive); put(o.actuator, actuator); put(o.inverse, inverse);
  return 0;
}
int point_host(const void* h, const double* qpos, const double* qvel, const double* qacc, int n_pts, const int* pt_body, const double* pt_pos, const double* pt_quat,
               double* pos, double* mat, double* vel, double* acc, double* gyro, double* accel, double* jacp, double* jacr, char* err) {
  const SgHostTables& T = *(const SgHostTables*)h;
  if (need(T.point, err)) return -1;
  SgpHostOut o;
  sgp_host_env(T, qpos, qvel, qacc, n_pts, pt_body, pt_pos, pt_quat, &o);
  put(o.pos, pos); put(o.mat, mat); put(o.vel, vel); put(o.acc, acc); put(o.gyro, gyro); put(o.accel, accel); put(o.jacp, jacp); put(o.jacr, jacr);
  return 0;
}
// info: nM, nlevel, right-hand sides per tile, 1 if some D is not finite or not positive; levels[nlevel]: dofs per depth.  Mp, Fp [nM]:
// the packed M and the packed factor
int solve_host(const void* h, const double* qpos, const double* qvel, const double* act, double kenv, const int* kmask_jnt, const int* kmask_ten, int n_rhs,
               const double* y, double* x, const double* applied, double* qacc_s, double* qfrc_s, int n_pts, const int* pt_body, const double* pt_pos, double* W,
               double* Mp, double* Fp, double* pivot, int* info, int* levels, char* err) {
  const SgHostTables& T = *(const SgHostTables*)h;
  if (need(T.solve, err)) return -1;
  SgvHostOut o;
  sgv_host_env(T, qpos, qvel, act, kenv, kmask_jnt, kmask_ten, n_rhs, y, applied, n_pts, pt_body, pt_pos, &o);
  put(o.x, x); put(o.qacc_smooth, qacc_s); put(o.qfrc_smooth, qfrc_s); put(o.W, W); put(o.fac.M, Mp); put(o.fac.F, Fp); put(o.levels, levels);
  *pivot = o.fac.pivot;
  info[0] = T.solve.o.nM; info[1] = T.solve.o.nlevel; info[2] = (int)o.tile; info[3] = o.fac.bad;
  return 0;
}
// the solve table alone, from a dof-parent chain: info as above (nM, nlevel, tile), levels; -1 and the reason where the model is refused
int solve_structure(int nbody, const int* bpar, int nv, const int* dbody, const int* dpar, int ntendon, int* info, int* levels, char* err) {
  SgSolveHost V;
  sgv_build(nbody, bpar, nv, dbody, dpar, ntendon, &V);
  if (need(V, err)) return -1;
  info[0] = V.o.nM; info[1] = V.o.nlevel; info[2] = (int)sgv_tile(nbody, nv, ntendon, V.o.nM);
  for (int L = 0; L < V.o.nlevel; L++) levels[L] = V.ints[V.o.lstart + L + 1] - V.ints[V.o.lstart + L];
  return 0;
}
int smooth_limits(int* out) {
  out[0] = SGS_MAXBODY; out[1] = SGS_MAXDOF; out[2] = SGS_MAXTENDON; out[3] = SGS_STATIC_LDS; out[4] = SGS_LDS_MAX; out[5] = SGS_REC; out[6] = SGS_DOF;
  return 7;
}
int point_limits(int* out) {
  out[0] = SGP_MAXBODY; out[1] = SGP_MAXDOF; out[2] = SGP_STATIC_LDS; out[3] = SGP_LDS_MAX; out[4] = SGP_REC; out[5] = SGP_DOF;
  return 6;
}
int solve_limits(int* out) {
  out[0] = SGV_STATIC_LDS; out[1] = SGV_LDS_MAX; out[2] = SGV_MINRHS; out[3] = SGS_REC; out[4] = SGS_DOF;
  return 5;
}
}
"""


def build(tmpdir, breaks=None, patch=None):
    """the shim as a ctypes library.  patch: a key of `breaks`, name -> (header of FILES, text to replace, its replacement)"""
    tag = "plain" if patch is None else "break%d" % sorted(breaks).index(patch)
    L = host_build.build(tmpdir, "readout_host", HOST_DRIVER, copy=FILES, patch=None if patch is None else breaks[patch], tag=tag)
    L.tables_new.restype = C.c_void_p
    L.tables_new.argtypes = [C.c_char_p, C.c_size_t]
    L._tables = {}
    return L


def tables(L, m):
    """the handle of model m's tables in library L (m is kept with it, so that its id stays its own)"""
    if id(m) not in L._tables:
        blob = m.to_blob()
        L._tables[id(m)] = (m, C.c_void_p(L.tables_new(blob, len(blob))))
    return L._tables[id(m)][1]


def call(entry, *args):
    """an entry of the shim, with the table's refusal as the assertion's text"""
    err = C.create_string_buffer(256)
    assert entry(*args, err) == 0, err.value.decode()
