// sg_blob.h -- the one reader of the model blob (include/softgrip_model.h) and its schema SG_MODEL_ARRAYS, which sg_mjcf.cpp writes from.
// Host only, no HIP: sg_plan.cpp, sg_tables.cpp and the g++ builds under tests/emu and scripts/sanitize all read blobs through it.
//   sg_blob_valid   magic, version, total_bytes == nbytes, and every one of the nrec records with its padded payload inside the buffer
//   sg_blob_find    the array (name, dtype): pointer and count.  Checks every record it walks on its own, so it is safe on bytes nobody
//                   validated: it never reads outside [blob, blob + nbytes)
//   SgModelView     the arrays the plan builder reads and the model's dimensions, resolved once by sg_model_view from the table
//                   SG_MODEL_ARRAYS: a missing array and an array whose count does not fit its dimension are refused by name
// Index VALUES inside the arrays (parent ids, geom addresses, ...) are not validated here.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/softgrip_model.h"

// Walks the records; false = a record header or payload leaves the buffer.  With a name it stops at the first match (*data, *cnt).
inline bool sg_blob_walk(const void* blob, size_t nbytes, const char* name, int dtype, const void** data, long long* cnt) {
  const char* base = (const char*)blob;
  if (!blob || nbytes < sizeof(sg_blob_header)) return false;
  const sg_blob_header* h = (const sg_blob_header*)base;
  size_t off = sizeof(sg_blob_header);
  for (uint32_t r = 0; r < h->nrec; r++) {
    if (nbytes - off < sizeof(sg_blob_record)) return false;
    const sg_blob_record* rec = (const sg_blob_record*)(base + off);
    off += sizeof(sg_blob_record);
    const size_t es = rec->dtype == SG_DT_F64 ? 8 : rec->dtype == SG_DT_I32 ? 4 : 1;
    if (rec->count < 0 || (uint64_t)rec->count > (nbytes - off) / es) return false;   // (no product that could wrap)
    size_t nb = (size_t)rec->count * es;
    nb += (8 - nb % 8) % 8;
    if (nb > nbytes - off) return false;   // the padding too
    if (name && strncmp(rec->name, name, sizeof rec->name) == 0 && (int)rec->dtype == dtype) {
      *data = base + off;
      *cnt = rec->count;
      return true;
    }
    off += nb;
  }
  if (name) *data = nullptr;
  return true;
}

inline bool sg_blob_valid(const void* blob, size_t nbytes) {
  const sg_blob_header* h = (const sg_blob_header*)blob;
  if (!blob || nbytes < sizeof *h || h->magic != SG_BLOB_MAGIC || h->version != SG_BLOB_VERSION || h->total_bytes < 0 || (uint64_t)h->total_bytes != nbytes)
    return false;
  return sg_blob_walk(blob, nbytes, nullptr, 0, nullptr, nullptr);
}

// nullptr: no such array (or a damaged record before it)
inline const void* sg_blob_find(const void* blob, size_t nbytes, const char* name, int dtype, long long* cnt) {
  const void* data = nullptr;
  return sg_blob_walk(blob, nbytes, name, dtype, &data, cnt) ? data : nullptr;
}

// The blob's schema: every array of a model blob in the container's order (the `names` record follows them).  The native MJCF compiler
// (sg_mjcf.cpp) writes from this table, sg_model_view reads from it.  The FIRST array of a dimension defines it (count / items), every
// later one must have items x dimension entries (sg_model_count_fits).
//   X(type, name, items per entry, dimension, part): read by the plan builder.  sg_model_view resolves the table in three parts, because
//   the builder's checks of the free joint and of the position / dof counts sit between them and refusals keep their order.
//   W(type, name, items per entry, dimension, free_only): written only, sg_model_view skips it.  free_only: only blobs with a free joint
//   carry it (only then do joint, position and dof indices differ).
//   Relaxed entries (dimension `none`: at least `items` entries): opt_d, and opt_i, which has grown over time (implicit_tendon_damping
//   is an optional 4th entry; the builder reads it only when n_opt_i says it is there).
#define SG_MODEL_ARRAYS(X, W)                                                                                                                \
  X(double, opt_d, 7, none, 0) X(int, opt_i, 1, none, 0)                                                                                     \
  X(double, body_pos, 3, nbody, 0) X(double, body_quat, 4, nbody, 0) X(double, body_ipos, 3, nbody, 0) X(double, body_imat, 9, nbody, 0)     \
  X(double, body_mass, 1, nbody, 0) X(double, body_invweight0, 2, nbody, 0) X(double, jnt_pos, 3, njnt, 0)                                   \
  X(double, jnt_axis, 3, njnt, 1) X(double, jnt_range, 2, njnt, 1) X(double, jnt_stiffness, 1, njnt, 1) X(double, jnt_margin, 1, njnt, 1)    \
  X(double, jnt_solref, 2, njnt, 1) X(double, jnt_solimp, 5, njnt, 1) X(double, qpos0, 1, nq, 1) X(double, qpos_spring, 1, nq, 1)            \
  X(double, dof_damping, 1, nv, 1) X(double, dof_armature, 1, nv, 1) X(double, dof_invweight0, 1, nv, 1)                                     \
  X(double, geom_size, 3, ngeom, 2) X(double, geom_pos, 3, ngeom, 2) X(double, geom_quat, 4, ngeom, 2) X(double, geom_friction, 3, ngeom, 2) \
  X(double, geom_solref, 2, ngeom, 2) X(double, geom_solimp, 5, ngeom, 2) X(double, geom_solmix, 1, ngeom, 2)                                \
  X(double, geom_margin, 1, ngeom, 2) X(double, geom_gap, 1, ngeom, 2) X(double, geom_rbound, 1, ngeom, 2)                                   \
  X(double, site_pos, 3, nsite, 2) X(double, site_quat, 4, nsite, 2)                                                                         \
  X(double, tendon_stiffness, 1, ntendon, 2) X(double, tendon_damping, 1, ntendon, 2) X(double, tendon_lengthspring, 1, ntendon, 2)          \
  X(double, tendon_length0, 1, ntendon, 2) X(double, tendon_invweight0, 1, ntendon, 2) X(double, wrap_prm, 1, nwrap, 2)                      \
  X(double, eq_solref, 2, neq, 2) X(double, eq_solimp, 5, neq, 2) X(double, eq_data, 5, neq, 2)                                              \
  X(double, actuator_timeconst, 1, nu, 2) X(double, actuator_gain, 1, nu, 2) X(double, actuator_bias, 3, nu, 2)                              \
  X(double, actuator_gear, 1, nu, 2)                                                                                                         \
  X(int, body_parentid, 1, nbody, 2) X(int, body_weldid, 1, nbody, 2) X(int, body_jntadr, 1, nbody, 2) X(int, body_jntnum, 1, nbody, 2)      \
  X(int, body_geomadr, 1, nbody, 2) X(int, body_geomnum, 1, nbody, 2)                                                                        \
  X(int, jnt_type, 1, njnt, 2) W(int, jnt_bodyid, 1, njnt, 0) X(int, jnt_limited, 1, njnt, 2) W(int, dof_parentid, 1, nv, 0)                 \
  X(int, geom_type, 1, ngeom, 2) X(int, geom_bodyid, 1, ngeom, 2) X(int, geom_contype, 1, ngeom, 2) X(int, geom_conaffinity, 1, ngeom, 2)    \
  X(int, geom_condim, 1, ngeom, 2) X(int, geom_priority, 1, ngeom, 2) X(int, site_bodyid, 1, nsite, 2)                                       \
  X(int, tendon_adr, 1, ntendon, 2) X(int, tendon_num, 1, ntendon, 2) X(int, wrap_type, 1, nwrap, 2) X(int, wrap_objid, 1, nwrap, 2)         \
  X(int, eq_type, 1, neq, 2) X(int, eq_obj1id, 1, neq, 2) X(int, eq_obj2id, 1, neq, 2) X(int, actuator_trnid, 1, nu, 2)                      \
  X(int, sensor_type, 1, nsensor, 2) X(int, sensor_objid, 1, nsensor, 2) X(int, sensor_adr, 1, nsensor, 2)                                   \
  W(int, jnt_qposadr, 1, njnt, 1) W(int, jnt_dofadr, 1, njnt, 1) W(int, dof_jntid, 1, nv, 1)
#define SG_SKIP(type, name, per, dim, free_only)

// the table's dimensions (-1 until their first array defines them): njnt joints, nq positions, nv dofs, nwrap tendon wrap objects
struct SgModelDims {
  int nbody = -1, njnt = -1, nq = -1, nv = -1, ngeom = -1, nsite = -1, ntendon = -1, nwrap = -1, neq = -1, nu = -1, nsensor = -1;
  int none = -1;             // (the table's dimension of the relaxed entries)
};
// the table's rule for an array of cnt entries, `per` items per entry of dimension *dim: does the count fit?  Defines *dim when it is the first
inline bool sg_model_count_fits(SgModelDims* D, long long cnt, int per, int* dim) {
  if (dim == &D->none) return cnt >= per;
  if (*dim < 0 && cnt % per == 0 && cnt / per <= INT32_MAX) *dim = (int)(cnt / per);
  return cnt == (long long)per * *dim;
}

struct SgModelView : SgModelDims {
  const void* blob = nullptr;
  size_t nbytes = 0;
  long long n_opt_i = 0;     // entries of opt_i
#define SG_X(type, name, per, dim, part) const type* name = nullptr;
  SG_MODEL_ARRAYS(SG_X, SG_SKIP)
#undef SG_X
};

inline bool sg_model_array(SgModelView* V, const char* name, int dtype, int per, int* dim, const void** out, std::string* err) {
  long long cnt = 0;
  *out = sg_blob_find(V->blob, V->nbytes, name, dtype, &cnt);
  if (!*out) {
    if (err) *err = std::string("model blob lacks ") + name;
    return false;
  }
  if (sg_model_count_fits(V, cnt, per, dim)) return true;
  if (err) *err = std::string("model blob: ") + name + " has " + std::to_string(cnt) + " entries, which does not fit the model's dimensions";
  return false;
}

// resolves part `part` (0, 1, 2 in turn) of SG_MODEL_ARRAYS over a blob that passed sg_blob_valid; false + *err = the first array that fails
inline bool sg_model_view(SgModelView* V, int part, std::string* err) {
  const void* p;
#define SG_X(type, name, per, dim, part_)                                                                                                  \
  if (part_ == part) {                                                                                                                     \
    if (!sg_model_array(V, #name, sizeof(type) == 8 ? SG_DT_F64 : SG_DT_I32, per, &V->dim, &p, err)) return false;                         \
    V->name = (const type*)p;                                                                                                              \
  }
  SG_MODEL_ARRAYS(SG_X, SG_SKIP)
#undef SG_X
  if (part == 0) sg_blob_find(V->blob, V->nbytes, "opt_i", SG_DT_I32, &V->n_opt_i);
  return true;
}
