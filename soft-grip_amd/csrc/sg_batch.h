// sg_batch.h -- what the two halves of the C ABI share: sg_model and sg_batch, and how an entry point fails.  sg_api.hip (life cycle and
// the step path) and sg_readout.hip (the read-outs) include it; nothing in it depends on a build flag, so both see one layout.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "sg_tables.h"   // (sg_readout.h, sg_dyn.h, sg_smooth.h, sg_point.h, sg_solve.h, sg_forces.h)
#include "sg_skin.h"
#include "sg_shape.h"
#include "sg_rows_host.h"   // (sg_work.h, sg_plan.h)
#include "sg_devmem.h"   // SgArena, SgScratch: the owners of every device buffer below (after the HIP runtime's declarations)

// the thread's error text (sg_last_error; one object, in sg_api.hip) and the code handed back
int fail(int code, const std::string& msg);
#define HIPCHK(x)                                                                              \
  do {                                                                                         \
    hipError_t e_ = (x);                                                                       \
    if (e_ != hipSuccess) return fail(SG_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(e_)); \
  } while (0)
// a failed sg_devmem.h call on the buffers of `what`: SG_ERR_NOMEM for the allocation, SG_ERR_HIP for a memset, a copy or the synchronise
int devmem_fail(bool nomem, const std::string& what);

struct sg_model : SgHostTables {   // (the base: kin, con, dyn, smooth, point, solve, forces -- the read-outs' tables, sg_tables.h)
  SgPlan plan;      // the fast kernels' plan (has_fast), else a copy of tplan: header, elements and sizes serve every entry point
  int rounds;       // ceil(nelem / 64)
  bool has_fast;    // the model is in the two-finger class of sg_plan.h
  bool has_tree;    // the tree pipeline (sg_tree.h) runs it
  SgPlan tplan;     // the tree pipeline's plan: same elements / equalities / statics, chains in `tree`, flat box references
  SgTreeDev tree;
  size_t tree_lds = 0;       // the tree kernel's LDS block in bytes and an env's slice of its work space in doubles (sgt::lds_bytes,
  long long tree_cws = 0;    // sgt::cws_doubles: each walks lds_carve, so once per model)
  SgSkinHost skin;  // the composite's skin (sg_skin.h; nvert == 0: none): sg_model_set_skin, drawn by sg_render_ex
};

// device tables and work space of the tree pipeline (sg_tree.h), allocated when the pipeline is first selected
struct SgTreeBufs {
  SgPlanHeader* H = nullptr;
  SgTreeDev* T = nullptr;
  double *elem = nullptr, *cws = nullptr;
  SgGenPair* pairs = nullptr;
  SgEqSlot* sched = nullptr;  // neighbour-row models: the tree plan's block schedule and neighbour tables
  int* nbtab = nullptr;
  int* touch_words = nullptr;   // [n][2]
};

// device tables and work space of the rows pipeline (sg_phase.hip, sg_rows.hip; in legacy builds also of the fused and split pipelines),
// allocated when a pipeline 0 .. 2 is first selected.  What goes into them and how large they are: sg_rows_host.h
struct SgRowsBufs {
  SgPlanHeader* H = nullptr;
  double* elem = nullptr;
  SgGenPair* gpairs = nullptr;  // SgPlan::gpairs (the general contact path's candidate pairs)
  int* nbtab = nullptr;         // neighbour-row models: SgPlan::nbtab and the three tables of SgRowsTables
  SgEqSlot* sched = nullptr;
  unsigned* tab = nullptr;
  int* cpos = nullptr;
  SgWork w = {};                // (w.secprof: the batch's)
  SgRowsShape shape;
  int nsl = 0;                  // sg_rows_nsl(nelem): the solver instantiation's joint-fix rows per lane
  bool ready = false;           // every table and the work space allocated and filled (rows_alloc)
  bool attr_set = false;        // hipFuncSetAttribute(MaxDynamicSharedMemorySize) done on this batch's device
};

struct sg_batch {
  const sg_model* m = nullptr;
  int n = 0, device = 0;
  SgArena mem;       // every buffer that lives as long as the batch: state, the read-outs' tables
  SgArena tree_mem;  // the buffers of `t`: all of them or none (tree_alloc)
  SgArena rows_mem;  // the buffers of `r`: all of them or none (rows_alloc)
  double *qpos = nullptr, *qvel = nullptr, *warm = nullptr, *act = nullptr, *ctrl = nullptr, *kenv = nullptr, *ctrl_row = nullptr;
  unsigned long long* secprof = nullptr;   // [48] cycle sums per kernel section of whichever pipeline runs (written by -DSG_SECTION_PROF builds only)
  int *kmask_jnt = nullptr, *kmask_ten = nullptr, *flags = nullptr, *touch = nullptr, *ncon = nullptr, *nefc = nullptr, *iters = nullptr;
  std::vector<int> kmask_jnt_host, kmask_ten_host;   // what the device masks hold (sg_set_stiffness copies them only when they change)
  int epw_override = 0;  // sg_set_solver_envs_per_wavefront: 0 = automatic
  int pipeline = 3;  // 0 fused (one kernel per call), 1 split (chain / phase / pgs kernel chain), 2 split with the row-parallel PGS kernel, 3 tree
  SgTreeBufs t;
  bool tree_ready = false;    // every table and the work space of the tree pipeline allocated and filled (tree_alloc)
  bool tree_attr_set = false;
  SgRowsBufs r;
  // profiling
  bool prof = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
  double prof_ms = 0;
  long long prof_n = 0;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pgs;  // around every solver-kernel launch (the dominant kernel)
  std::vector<hipEvent_t> ev_pool;  // events handed back by sg_profile_read*: a profiled call creates none once the pool is warm
  double prof_pgs_ms = 0;
  long long prof_pgs_n = 0;
  // ---- the read-outs (sg_readout.hip), everything allocated at first use ----
  // the per-model tables on the batch's device (sg_devmem.h SgDevTable; Readout::need_* in sg_readout.hip brings each up with what it
  // is built on): kin the kinematics table; con the candidate pairs (i) and the margins / bounding radii (d); dyn, smooth, point, solve
  // and forces the tables of sg_dyn.h, sg_smooth.h, sg_point.h, sg_solve.h and sg_forces.h; zero a row of max(nv, 1) zeros, the qvel the
  // point and solve calls that need none walk at
  SgDevTable kin, con, dyn, smooth, point, solve, forces, zero;
  // pose read-out / renderer
  SgScratch<int> kin_ids;    // the listed env ids on the device
  SgScratch<float> rrecs;    // [n_ids][ngeom][SGR_REC] fp32 geom records of the last sg_render
  // the skin (sg_render_ex): tables uploaded at first use and again when the model's skin version has moved
  SgArena skin_mem;
  SgSkinDev skin_dev = {};
  unsigned skin_version = 0;   // the version skin_dev holds (0: none; versions start at 1)
  SgScratch<double> skin_xpos, skin_xquat;   // [n_ids][nbody][3 | 4] body poses of the last skin render
  SgScratch<float> skin_vrec;                // [n_ids][nvert][SGR_VREC] vertex records of the last skin render
  // contact read-out
  SgScratch<double> con_scratch;   // per-env pose blocks of a model whose poses do not fit LDS
  bool con_attr_set = false;
  // ray queries: the poses of the last call's envs and its rays' body / exclude ids
  SgScratch<double> ray_xpos, ray_xquat, ray_gxpos, ray_gxmat;   // [n_ids][nbody][3 | 4], [n_ids][ngeom][3 | 9]
  SgScratch<int> ray_ids;                                         // [2][n_rays]
  SgScratch<double> ray_vtx;                                      // [n_ids][nvert][3] the skin's vertices of the last SG_RAY_SKIN call
  const int* skin_vis = nullptr;                                  // [skin_nvis] the geoms the skin does not replace (in skin_mem, with skin_dev)
  int skin_nvis = 0;
  // mass-matrix, joint-force and inverse-dynamics read-outs
  bool smooth_attr_set = false;
  // point motion and Jacobians: the last call's points (body ids; positions [n_pts][3] then quaternions [n_pts][4])
  bool point_attr_set = false;
  SgScratch<int> pt_ids;
  SgScratch<double> pt_d;
  // mass-matrix solves, smooth forward dynamics and point inertias: the last call's points
  bool solve_attr_set = false;
  SgScratch<int> sv_ids;
  SgScratch<double> sv_pos;
  // constraint forces (sg_get_forces): the chunk's work space (rows' J and W, scalar records, contact list, row directory), allocated at
  // the first call and capped at forces_cap bytes (sg_set_forces_workspace; the env list is processed in chunks that fit)
  SgScratch<double> forces_ws;
  size_t forces_cap = (size_t)256 << 20;
  bool forces_rows_attr_set = false, forces_pgs_attr_set = false;
  // the soft object's read-outs (sg_get_skin_vertices / sg_get_shape / sg_get_subtree): the shape table (sg_shape.h) of the skin version
  // shape_version, in an arena of its own -- the skin is no part of the blob and may change --, and the last call's directions
  SgArena shape_mem;
  SgShapeOff shape_off = {};
  const double* shape_d = nullptr;
  const int* shape_i = nullptr;
  bool shape_up = false;
  unsigned shape_version = 0;
  bool shape_attr_set = false;
  SgScratch<double> shape_dir;
  SgScratch<int> shape_dir_body;
  ~sg_batch() {   // (on the batch's device: sg_batch_destroy.  The arenas and scratch buffers free themselves)
    for (auto& e : ev) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
    for (auto& e : ev_pgs) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
    for (auto& e : ev_pool) (void)hipEventDestroy(e);
  }
};
