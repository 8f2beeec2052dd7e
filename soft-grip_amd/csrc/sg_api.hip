// sg_api.hip -- C ABI (include/softgrip.h) over the gfx950 kernels.  No CPU fallback.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "sg_mjcf.h"
#include "sg_tree.h"
#include "sg_work.h"
#include "sg_kin.hip"   // pose read-out and renderer kernels (compiled in this translation unit)
#include "sg_contacts.hip"   // contact-list read-out kernel (compiled in this translation unit, after sg_kin.hip)
#include "sg_ray.hip"   // ray-query kernels (compiled in this translation unit, after sg_contacts.hip)
#include "sg_devmem.h"   // SgArena, SgScratch: the owners of every device buffer below (after the HIP runtime's declarations)
#ifdef SG_LEGACY_PIPELINES
#include "sg_kernels_args.h"
#endif

#ifdef SG_LEGACY_PIPELINES
#define SG_LEGACY_ON 1
#else
#define SG_LEGACY_ON 0   // (the split pipeline's contact records, 126 MB at 4096 envs, are then not allocated)
#endif

namespace {
thread_local std::string g_err;
int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
#define HIPCHK(x)                                                                              \
  do {                                                                                         \
    hipError_t e_ = (x);                                                                       \
    if (e_ != hipSuccess) return fail(SG_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(e_)); \
  } while (0)
// a failed sg_devmem.h call on the buffers of `what`: SG_ERR_NOMEM for the allocation, SG_ERR_HIP for a memset, a copy or the synchronise
int devmem_fail(bool nomem, const std::string& what) {
  (void)hipGetLastError();   // (the failed call's error must not stay behind as the thread's last one: the next launch check, ours or the caller's, would report it)
  return fail(nomem ? SG_ERR_NOMEM : SG_ERR_HIP, what + (nomem ? ": out of device memory" : ": a HIP memset, copy or synchronise failed"));
}

__global__ void sg_fill_rows_kernel(double* dst, const double* row, int n, int w) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n * w) dst[i] = row[i % w];
}
#define SG_CTRL_BYVAL 8
struct SgCtrlRow { double v[SG_CTRL_BYVAL]; };
__global__ void sg_fill_rows_val_kernel(double* dst, SgCtrlRow row, int n, int w) {  // the row travels in the kernel arguments: no host sync
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n * w) dst[i] = row.v[i % w];
}
__global__ void sg_masked_copy_kernel(const unsigned char* mask, int n, const int* s0, int* d0, const int* s1, int* d1, const int* s2, int* d2,
                                      const int* s3, int* d3, const int* s4, int* d4) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && (!mask || mask[i])) { d0[i] = s0[i]; d1[i] = s1[i]; d2[i] = s2[i]; d3[i] = s3[i]; d4[i] = s4[i]; }
}
}  // namespace

struct sg_model {
  SgPlan plan;      // the fast kernels' plan (has_fast), else a copy of tplan: header, elements and sizes serve every entry point
  int rounds;       // ceil(nelem / 64)
  bool has_fast;    // the model is in the two-finger class of sg_plan.h
  bool has_tree;    // the tree pipeline (sg_tree.h) runs it
  SgPlan tplan;     // the tree pipeline's plan: same elements / equalities / statics, chains in `tree`, flat box references
  SgTreeDev tree;
  size_t tree_lds = 0;       // the tree kernel's LDS block in bytes and an env's slice of its work space in doubles (sgt::lds_bytes,
  long long tree_cws = 0;    // sgt::cws_doubles: each walks lds_carve, so once per model)
  SgKinHost kin;    // kinematics table of sg_get_poses / sg_render (sg_kin.hip)
  SgConHost con;    // candidate pairs, margins and bounding radii of sg_get_contacts (sg_contacts.hip)
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

struct sg_batch {
  const sg_model* m = nullptr;
  int n = 0, device = 0;
  SgArena mem;       // every buffer that lives as long as the batch: state, tables, the rows work space, the read-outs' tables
  SgArena tree_mem;  // the buffers of `t`: all of them or none (tree_alloc)
  SgPlanHeader* dH = nullptr;
  double *delem = nullptr, *qpos = nullptr, *qvel = nullptr, *warm = nullptr, *act = nullptr, *ctrl = nullptr, *kenv = nullptr, *ctrl_row = nullptr;
  SgGenPair* dgpairs = nullptr;  // SgPlan::gpairs on the device (the general contact path's candidate pairs)
  int* dnbtab = nullptr;       // SgPlan::nbtab on the device (neighbour-row models)
  SgEqSlot* dsched = nullptr;  // SgPlan::sched + eight spare rounds of idle slots
  unsigned* dtab = nullptr;    // the same schedule as the solver's LDS table words
  int* dcpos = nullptr;        // per element: where its equality block's step factors sit in a solver wavefront's stream (SgWork::cst)
  int *kmask_jnt = nullptr, *kmask_ten = nullptr, *flags = nullptr, *touch = nullptr, *ncon = nullptr, *nefc = nullptr, *iters = nullptr;
  std::vector<int> kmask_jnt_host, kmask_ten_host;   // what the device masks hold (sg_set_stiffness copies them only when they change)
  int epw_override = 0;  // sg_set_solver_envs_per_wavefront: 0 = automatic
  int pipeline = 3;  // 0 fused (one kernel per call), 1 split (chain / phase / pgs kernel chain), 2 split with the row-parallel PGS kernel, 3 tree
  SgTreeBufs t;
  bool tree_ready = false;    // every table and the work space of the tree pipeline allocated and filled (tree_alloc)
  bool tree_attr_set = false;
  SgWork w = {};
  bool lds_attr_set = false;  // hipFuncSetAttribute(MaxDynamicSharedMemorySize) done on this batch's device
  // profiling
  bool prof = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
  double prof_ms = 0;
  long long prof_n = 0;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pgs;  // around every solver-kernel launch (the dominant kernel)
  std::vector<hipEvent_t> ev_pool;  // events handed back by sg_profile_read*: a profiled call creates none once the pool is warm
  double prof_pgs_ms = 0;
  long long prof_pgs_n = 0;
  // pose read-out / renderer (sg_kin.hip), allocated at first use
  double* kin_d = nullptr;
  int* kin_i = nullptr;
  SgScratch<int> kin_ids;    // the listed env ids on the device
  SgScratch<float> rrecs;    // [n_ids][ngeom][SGR_REC] fp32 geom records of the last sg_render
  // the skin (sg_render_ex): tables uploaded at first use and again when the model's skin version has moved
  SgArena skin_mem;
  SgSkinDev skin_dev = {};
  unsigned skin_version = 0;   // the version skin_dev holds (0: none; versions start at 1)
  SgScratch<double> skin_xpos, skin_xquat;   // [n_ids][nbody][3 | 4] body poses of the last skin render
  SgScratch<float> skin_vrec;                // [n_ids][nvert][SGR_VREC] vertex records of the last skin render
  // contact read-out (sg_contacts.hip), allocated at first use
  int* con_pairs = nullptr;
  double* con_gaux = nullptr;
  SgScratch<double> con_scratch;   // per-env pose blocks of a model whose poses do not fit LDS
  bool con_attr_set = false;
  // ray queries (sg_ray.hip): the poses of the last call's envs and its rays' body / exclude ids
  SgScratch<double> ray_xpos, ray_xquat, ray_gxpos, ray_gxmat;   // [n_ids][nbody][3 | 4], [n_ids][ngeom][3 | 9]
  SgScratch<int> ray_ids;                                         // [2][n_rays]
  ~sg_batch() {   // (on the batch's device: sg_batch_destroy.  The arenas and scratch buffers free themselves)
    for (auto& e : ev) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
    for (auto& e : ev_pgs) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
    for (auto& e : ev_pool) (void)hipEventDestroy(e);
  }
};

static int begin_event_pair(sg_batch* b, std::vector<std::pair<hipEvent_t, hipEvent_t>>& list, hipStream_t s);

// all or nothing: a failed allocation (the work space is ~0.5 MB per env for the four-finger scene) leaves no half-built pipeline behind
// that a second sg_set_pipeline call would take for a complete one
static int tree_alloc(sg_batch* b) {
  if (b->tree_ready) return SG_OK;
  const sg_model* m = b->m;
  if (!m->has_tree) return fail(SG_ERR_MODEL, "the tree pipeline does not run this model");
  const size_t n = b->n;
  SgArena& A = b->tree_mem;
  SgTreeBufs& t = b->t;
  bool ok = A.zeros(&t.H, 1) && A.zeros(&t.T, 1) && A.upload(&t.elem, m->tplan.elem) && A.upload(&t.pairs, m->tplan.gpairs) &&
            A.zeros(&t.cws, n * (size_t)m->tree_cws) && A.zeros(&t.touch_words, 2 * n) && A.upload(&t.sched, m->tplan.sched) &&
            A.upload(&t.nbtab, m->tplan.nbtab) && hipMemcpy(t.H, &m->tplan.h, sizeof(SgPlanHeader), hipMemcpyHostToDevice) == hipSuccess &&
            hipMemcpy(t.T, &m->tree, sizeof(SgTreeDev), hipMemcpyHostToDevice) == hipSuccess;
  bool nomem = A.nomem;
  if (ok && !b->w.secprof) {   // (a model outside the two-finger class has no split-pipeline work space)
    ok = b->mem.zeros(&b->w.secprof, 48);
    nomem = b->mem.nomem;
  }
  if (!ok) {
    A.release();
    t = SgTreeBufs();
    return devmem_fail(nomem, "tree pipeline");
  }
  b->tree_ready = true;
  return SG_OK;
}

// tree pipeline: one launch per call, one env per wavefront (sg_tree.hip)
static int launch_tree(sg_batch* b, int mode, const uint8_t* mask, int nsub, double* sens, long long stride, int32_t* flags, int32_t* touch,
                       hipStream_t s) {
  const sg_model* m = b->m;
  sgt::TreeArgs a;
  a.H = b->t.H; a.T = b->t.T; a.elem = b->t.elem; a.gpairs = b->t.pairs; a.sched = b->t.sched; a.nbtab = b->t.nbtab;
  a.qpos = b->qpos; a.qvel = b->qvel; a.warm = b->warm; a.act = b->act; a.ctrl = b->ctrl;
  a.kenv = b->kenv; a.kmask_jnt = b->kmask_jnt; a.kmask_ten = b->kmask_ten;
  a.mask = mask; a.sens = sens; a.sens_stride = stride > 0 ? stride : m->tplan.h.nsensordata;
  a.flags = flags ? flags : b->flags; a.touch = touch ? touch : b->touch; a.touch_words = b->t.touch_words;
  a.ncon = b->ncon; a.nefc = b->nefc; a.iters = b->iters;
  a.cws = b->t.cws; a.cws_stride = m->tree_cws;
  a.nenv = b->n; a.nsub = nsub; a.mode = mode; a.secprof = b->w.secprof;
  if (!b->tree_attr_set) {
    HIPCHK(sg_tree_prepare());
    b->tree_attr_set = true;
  }
  if (b->prof)
    if (int rc = begin_event_pair(b, b->ev, s)) return rc;
  HIPCHK(sg_launch_tree(a, m->tree.CS, m->tree_lds, s));
  if (b->prof) HIPCHK(hipEventRecord(b->ev.back().second, s));
  return SG_OK;
}

extern "C" {

const char* sg_last_error(void) { return g_err.c_str(); }
const char* sg_version(void) { return "softgrip-mi355x 0.1 (gfx950)"; }

int sg_model_create(const void* blob, size_t nbytes, sg_model** out) {
  if (!blob || !out) return fail(SG_ERR_INVALID, "sg_model_create: null argument");
  sg_model* m = new sg_model();
  std::string err, terr;
  m->has_fast = sg_plan_build(blob, nbytes, &m->plan, &err);
  m->has_tree = sg_tree_plan_build(blob, nbytes, &m->tplan, &m->tree, &terr);
  if (m->has_tree) {
    m->tree_lds = sgt::lds_bytes(m->tree, m->tplan.h.nelem, m->tplan.h.has_free, m->tplan.h.nnb);
    m->tree_cws = sgt::cws_doubles(m->tree, m->tplan.h.nelem, m->tplan.h.has_free, m->tplan.h.nnb);
  }
  if (m->has_tree && m->tree_lds > 160 * 1024) {
    m->has_tree = false;
    terr = "the env's state does not fit the 160 KB of LDS";
  }
  if (!m->has_fast && !m->has_tree) {
    delete m;
    return fail(SG_ERR_MODEL, "sg_model_create: " + err + " (two-finger kernels); " + terr + " (tree pipeline)");
  }
  if (!m->has_fast) m->plan = m->tplan;
  sgk_build(blob, nbytes, m->has_fast ? m->plan : m->tplan, m->has_tree ? &m->tree : nullptr, m->has_fast, &m->kin);
  sgc_from_blob(blob, nbytes, m->kin, &m->con);
  m->rounds = (m->plan.h.nelem + 63) / 64;
  if (m->rounds > 4) {
    delete m;
    return fail(SG_ERR_MODEL, "sg_model_create: more than 256 composite elements");
  }
  if (m->has_fast && m->plan.h.nnb > 0) {  // the rows PGS kernel keeps every equality row of 8 envs in LDS (launch_split)
    if (sizeof(double) * SG_ROWS_LDS_NB(4, m->plan.h.nelem, m->plan.h.eq_rounds, 1) > 160 * 1024 || m->plan.h.nelem > 254) {  // (11-bit slider offsets in the table words)
      delete m;
      return fail(SG_ERR_MODEL, "sg_model_create: too many neighbour equality rows for the PGS kernel's LDS");
    }
  }
  *out = m;
  return SG_OK;
}
void sg_model_destroy(sg_model* m) { delete m; }

int sg_mjcf_compile(const char* xml_path, int flags, void** blob, size_t* nbytes) {
  if (!xml_path || !blob || !nbytes) return fail(SG_ERR_INVALID, "sg_mjcf_compile: null argument");
  std::string out, err;
  if (!sg_mjcf_compile_file(xml_path, !(flags & SG_COMPILE_NO_NEIGHBORS), (flags & SG_COMPILE_IMPLICIT_TENDON_DAMPER) != 0, &out, &err))
    return fail(SG_ERR_MODEL, "sg_mjcf_compile: " + err);
  void* p = malloc(out.size());
  if (!p) return fail(SG_ERR_INVALID, "sg_mjcf_compile: out of memory");
  memcpy(p, out.data(), out.size());
  *blob = p; *nbytes = out.size();
  return SG_OK;
}
void sg_blob_free(void* blob) { free(blob); }

int sg_model_compile(const char* xml_path, int flags, sg_model** out) {
  if (!xml_path || !out) return fail(SG_ERR_INVALID, "sg_model_compile: null argument");
  std::string blob, err;
  SgSkinSpec spec;
  if (!sg_mjcf_compile_file(xml_path, !(flags & SG_COMPILE_NO_NEIGHBORS), (flags & SG_COMPILE_IMPLICIT_TENDON_DAMPER) != 0, &blob, &err, &spec))
    return fail(SG_ERR_MODEL, "sg_mjcf_compile: " + err);
  int rc = sg_model_create(blob.data(), blob.size(), out);
  if (rc != SG_OK || !spec.present) return rc;
  // the composite's <skin>: built from the body names of the blob, as mjcf.py Model.composite_skin() does
  long long c = 0;
  const char* names = (const char*)sg_blob_find(blob.data(), blob.size(), "names", SG_DT_U8, &c);
  std::vector<std::string> body_names(1);
  for (long long i = 0; names && i < c && names[i] != '\n'; i++) {
    if (names[i] == '|') body_names.emplace_back();
    else body_names.back().push_back(names[i]);
  }
  SgSkinHost S;
  // (names that do not form a shell within the limits: the model has no skin, as mjcf.py's Model.skin = None -- the scene still compiles)
  if (sg_composite_skin(body_names, &spec.prefix, spec.inflate, spec.rgba, &S) &&
      sg_model_set_skin(*out, S.nvert, S.vert_body.data(), S.vert_pos.data(), S.nface, S.face.data(), S.rgba) != SG_OK)
    (void)sg_model_set_skin(*out, 0, nullptr, nullptr, 0, nullptr, nullptr);
  return SG_OK;
}
int sg_model_nq(const sg_model* m) { return m->plan.h.nq; }
int sg_model_nv(const sg_model* m) { return m->plan.h.nv; }
int sg_model_njnt(const sg_model* m) { return m->plan.h.njnt; }
int sg_model_nu(const sg_model* m) { return m->plan.h.nu; }
int sg_model_nsensordata(const sg_model* m) { return m->plan.h.nsensordata; }
int sg_model_ntendon(const sg_model* m) { return m->plan.h.ntendon; }
int sg_model_nelem(const sg_model* m) { return m->plan.h.nelem; }

void sg_batch_destroy(sg_batch* b) {
  if (!b) return;
  (void)hipSetDevice(b->device);
  delete b;
}

int sg_batch_create(const sg_model* m, int n_envs, int device, sg_batch** out) {
  if (!m || !out || n_envs <= 0) return fail(SG_ERR_INVALID, "sg_batch_create: bad argument");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(SG_ERR_NO_DEVICE, "sg_batch_create: no HIP device (there is no CPU fallback)");
  if (device < 0 || device >= ndev) return fail(SG_ERR_NO_DEVICE, "sg_batch_create: device index out of range");
  HIPCHK(hipSetDevice(device));
  std::unique_ptr<sg_batch, void (*)(sg_batch*)> guard(new sg_batch(), sg_batch_destroy);   // every early return below destroys the half-built batch
  sg_batch* b = guard.get();
  b->m = m; b->n = n_envs; b->device = device;
  SgArena& A = b->mem;
  const SgPlanHeader& H = m->plan.h;
  const size_t n = n_envs, nv = H.nv, nq = H.nq, njnt = H.njnt, nu = H.nu, nt = H.ntendon;   // nq = nv = njnt unless the model has a free joint
  bool ok = A.zeros(&b->dH, 1) && hipMemcpy(b->dH, &H, sizeof H, hipMemcpyHostToDevice) == hipSuccess && A.upload(&b->delem, m->plan.elem) &&
            A.zeros(&b->qpos, n * nq) && A.zeros(&b->qvel, n * nv) && A.zeros(&b->warm, n * nv) && A.zeros(&b->act, n * nu) &&
            A.zeros(&b->ctrl, n * nu) && A.zeros(&b->kenv, n) && A.zeros(&b->ctrl_row, nu) && A.zeros(&b->kmask_jnt, njnt) &&
            A.zeros(&b->kmask_ten, nt) && A.zeros(&b->flags, n) && A.zeros(&b->touch, n) && A.zeros(&b->ncon, n) && A.zeros(&b->nefc, n) &&
            A.zeros(&b->iters, n) && A.upload(&b->dgpairs, m->plan.gpairs);
  if (!ok) return devmem_fail(A.nomem, "sg_batch_create (state)");
  b->kmask_jnt_host.assign(njnt, 0); b->kmask_ten_host.assign(nt, 0);
  if (m->has_fast) {  // work space of the split pipeline
    const size_t S = 2 * n, N = H.nelem;
    SgWork& w = b->w;
    ok = A.zeros(&w.secprof, 48) && A.zeros(&w.crec, SG_LEGACY_ON ? SG_CAP * ((n + SG_EPW - 1) / SG_EPW + 1) * SG_RF * SG_SPW : 0) && A.zeros(&w.ns, S) &&
         A.zeros(&w.crow, (SG_CAP + 2) * ((n + 7) / 8 + 2) * SG_RK * 64) && A.zeros(&w.cdummy, ((n + 3) / 4) * SG_RK * 64) &&
         A.zeros(&w.envh, 4 * n) && A.zeros(&w.shared, n) && A.zeros(&w.pending, n) && A.zeros(&w.status, n) && A.zeros(&w.iters, n) &&
         A.zeros(&w.ncon, n) && A.zeros(&w.nefc, n) && A.zeros(&w.touch, n) && A.zeros(&w.sMinv, 16 * S) && A.zeros(&w.saF, 4 * S) &&
         A.zeros(&w.lim_active, S) && A.zeros(&w.lim, 4 * SG_MAXLIM * S) && A.zeros(&w.as, n * N) && A.zeros(&w.eqf, n * N) &&
         A.zeros(&w.eqb, n * N) && A.zeros(&w.eqR, n * N) && A.zeros(&w.asme, n * N) && A.zeros(&w.fsm, n * N) &&
         A.zeros(&w.chh, n * 2 * SG_CHW) && A.zeros(&w.nbf, n * (3 * N + 1)) && A.zeros(&w.nbb, n * (3 * N + 1)) && A.zeros(&w.nbR, n * (3 * N + 1)) &&
         A.zeros(&w.cst, (H.nnb > 0 && SG_ROWS_NB_MODE(H.nelem, H.eq_rounds) == 2) ? SG_CST_INDEX((n + 3) / 4, 0, 0, H.eq_rounds + 8) : 0) &&
         A.zeros(&w.gcon, n * SG_GEN_MAXCON * SG_GEN_W) && A.zeros(&w.gen, n) && A.zeros(&w.gen_count, 4) && A.zeros(&w.gen_list, n) &&
         A.zeros(&w.gpairs16, SG_PHASE_SLIM(m->rounds) ? n * SG_PAIRS_CAP(4) : 0) && A.zeros(&w.gcval, SG_PHASE_SLIM(m->rounds) ? n * SG_MAXCH * 64 : 0);
    if (!ok) return devmem_fail(A.nomem, "sg_batch_create (split-pipeline work space)");
    const char* pm = getenv("SG_PIPELINE");
    b->pipeline = (pm && strcmp(pm, "tree") == 0 && m->has_tree) ? 3 : 2;
#ifdef SG_LEGACY_PIPELINES
    if (pm && strcmp(pm, "fused") == 0) b->pipeline = 0;
    if (pm && strcmp(pm, "split") == 0) b->pipeline = 1;
#endif
    if (H.nnb > 0 && b->pipeline != 3) b->pipeline = 2;  // neighbour equality rows: the rows pipeline (or the tree pipeline when asked for)
  }
  if (m->has_fast && H.nnb > 0) {
    std::vector<SgEqSlot> sch = m->plan.sched;
    SgEqSlot idle;
    idle.e = idle.p[0] = idle.p[1] = idle.p[2] = H.nelem;
    for (int g = 0; g < 8 * SG_EQ_SLOTS; g++) sch.push_back(idle);  // the kernel fetches slots a few rounds ahead
    // the solver's table words (sg_pgs_rows_kernel): lane 2 b + h of a 16-lane group holds, for the block e in slot b of the round,
    // x | y << 11 | (2 e + h) << 22: the byte offsets of two slider words, (x, y) = 8 (e, p0) for h = 0 and 8 (p1, p2) for h = 1, and the
    // lane's pair of row states in 16-byte units
    // (models that keep the step factors in LDS -- SG_ROWS_NB_MODE 1, the box scene -- get TWO words per lane and round instead:
    //  x | y << 16 and the byte offset of the lane's pair of 32-byte records)
    const bool two_words = SG_ROWS_NB_MODE(H.nelem, H.eq_rounds) == 1;
    std::vector<unsigned> tab((two_words ? 4 : 2) * sch.size());
    for (size_t i = 0; i < 2 * sch.size(); i++) {
      const SgEqSlot& sl = sch[i >> 1];
      const int h = (int)(i & 1);
      const unsigned x = h ? sl.p[1] : sl.e, y = h ? sl.p[2] : sl.p[0];
      if (two_words) { tab[2 * i] = (8u * x) | ((8u * y) << 16); tab[2 * i + 1] = 64u * (unsigned)sl.e + 32u * (unsigned)h; }
      else tab[i] = (8u * x) | ((8u * y) << 11) | ((2u * (unsigned)sl.e + (unsigned)h) << 22);
    }
    // where the phase kernel puts a block's four step factors: round r, slot g of the schedule = lanes 2 g, 2 g + 1 of the env's
    // 16-lane group, two doubles each (SG_CST_INDEX)
    std::vector<int> cpos(H.nelem, 0);
    for (size_t i = 0; i < m->plan.sched.size(); i++)
      if (m->plan.sched[i].e < H.nelem) cpos[m->plan.sched[i].e] = (int)(i / SG_EQ_SLOTS) * 128 + 4 * (int)(i % SG_EQ_SLOTS);
    if (!(A.upload(&b->dnbtab, m->plan.nbtab) && A.upload(&b->dsched, sch) && A.upload(&b->dtab, tab) && A.upload(&b->dcpos, cpos)))
      return devmem_fail(A.nomem, "sg_batch_create (solver tables)");
  }
  // state as after mj_resetData
  std::vector<double> q0(nq, 0.0);
  for (int c = 0; c < H.nchain; c++)
    for (int d = 0; d < H.chain[c].ndof; d++) q0[H.chain[c].dof0 + d] = H.chain[c].qpos0[d];
  if (!m->has_fast)
    for (int d = 0; d < m->tree.ND; d++) q0[m->tree.d_gid[d]] = m->tree.d_qpos0[d];
  for (int e = 0; e < H.nelem; e++) q0[H.elem_qpos0 + e] = m->plan.elem[(size_t)SGE_QPOS0 * H.nelem + e];
  if (H.has_free)
    for (int c = 0; c < 7; c++) q0[H.free_qadr + c] = H.free_q0[c];
  std::vector<double> qall(n * nq);
  for (size_t i = 0; i < n; i++) memcpy(&qall[i * nq], q0.data(), sizeof(double) * nq);
  HIPCHK(hipMemcpy(b->qpos, qall.data(), sizeof(double) * n * nq, hipMemcpyHostToDevice));
  if (b->pipeline == 3)
    if (int rc = tree_alloc(b)) return rc;
  *out = guard.release();
  return SG_OK;
}
int sg_batch_nenvs(const sg_batch* b) { return b->n; }
int sg_batch_device(const sg_batch* b) { return b->device; }

int sg_set_stiffness(sg_batch* b, const double* k, int k_on_host, const int* jnt_ids, int nj, const int* ten_ids, int nt, void* stream) {
  if (!b || !k || nj < 0 || nt < 0 || (nj && !jnt_ids) || (nt && !ten_ids)) return fail(SG_ERR_INVALID, "sg_set_stiffness: bad argument");
  HIPCHK(hipSetDevice(b->device));
  const SgPlanHeader& H = b->m->plan.h;
  std::vector<int> mj(H.njnt, 0), mt(H.ntendon, 0);
  for (int i = 0; i < nj; i++) {
    if (jnt_ids[i] < 0 || jnt_ids[i] >= H.njnt) return fail(SG_ERR_INVALID, "sg_set_stiffness: joint id out of range");
    mj[jnt_ids[i]] = 1;
  }
  for (int i = 0; i < nt; i++) {
    if (ten_ids[i] < 0 || ten_ids[i] >= H.ntendon) return fail(SG_ERR_INVALID, "sg_set_stiffness: tendon id out of range");
    mt[ten_ids[i]] = 1;
  }
  hipStream_t s = (hipStream_t)stream;
  // Host synchronisation (softgrip.h says so): the id masks are tiny and change once per scene, not once per episode -- they are
  // copied (synchronously: the host vectors' lifetime stays trivial) only when they differ from what the device holds; a HOST k is a
  // synchronous copy by nature (pageable memory).  With unchanged id sets and a DEVICE k the call enqueues one copy and returns.
  const bool masks_changed = mj != b->kmask_jnt_host || mt != b->kmask_ten_host;
  if (masks_changed || k_on_host) HIPCHK(hipStreamSynchronize(s));
  if (masks_changed) {
    HIPCHK(hipMemcpy(b->kmask_jnt, mj.data(), sizeof(int) * H.njnt, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(b->kmask_ten, mt.data(), sizeof(int) * H.ntendon, hipMemcpyHostToDevice));
    b->kmask_jnt_host = mj;
    b->kmask_ten_host = mt;
  }
  if (k_on_host) HIPCHK(hipMemcpy(b->kenv, k, sizeof(double) * b->n, hipMemcpyHostToDevice));
  else HIPCHK(hipMemcpyAsync(b->kenv, k, sizeof(double) * b->n, hipMemcpyDeviceToDevice, s));
  return SG_OK;
}

int sg_set_ctrl(sg_batch* b, const double* ctrl, int broadcast, void* stream) {
  if (!b || !ctrl) return fail(SG_ERR_INVALID, "sg_set_ctrl: bad argument");
  HIPCHK(hipSetDevice(b->device));
  hipStream_t s = (hipStream_t)stream;
  const int nu = b->m->plan.h.nu;
  if (nu == 0) return SG_OK;
  if (broadcast && nu <= SG_CTRL_BYVAL) {
    SgCtrlRow row;
    for (int i = 0; i < SG_CTRL_BYVAL; i++) row.v[i] = i < nu ? ctrl[i] : 0.0;
    int total = b->n * nu;
    hipLaunchKernelGGL(sg_fill_rows_val_kernel, dim3((total + 255) / 256), dim3(256), 0, s, b->ctrl, row, b->n, nu);
    HIPCHK(hipGetLastError());
  } else if (broadcast) {
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipMemcpy(b->ctrl_row, ctrl, sizeof(double) * nu, hipMemcpyHostToDevice));
    int total = b->n * nu;
    hipLaunchKernelGGL(sg_fill_rows_kernel, dim3((total + 255) / 256), dim3(256), 0, s, b->ctrl, b->ctrl_row, b->n, nu);
    HIPCHK(hipGetLastError());
  } else {
    HIPCHK(hipMemcpyAsync(b->ctrl, ctrl, sizeof(double) * b->n * nu, hipMemcpyDeviceToDevice, s));
  }
  return SG_OK;
}

// a pair of events registered in `list` BEFORE anything is recorded (so that a failing HIP call cannot leak them), first one recorded
static int begin_event_pair(sg_batch* b, std::vector<std::pair<hipEvent_t, hipEvent_t>>& list, hipStream_t s) {
  hipEvent_t e[2];
  for (int i = 0; i < 2; i++) {
    if (!b->ev_pool.empty()) { e[i] = b->ev_pool.back(); b->ev_pool.pop_back(); }
    else if (hipEventCreate(&e[i]) != hipSuccess) {
      if (i == 1) b->ev_pool.push_back(e[0]);
      return fail(SG_ERR_HIP, "hipEventCreate failed");
    }
  }
  list.emplace_back(e[0], e[1]);
  HIPCHK(hipEventRecord(e[0], s));
  return SG_OK;
}

// sg_profile_read*: the finished pairs of `list` into the two accumulators, their events back to the pool
static int profile_read(sg_batch* b, std::vector<std::pair<hipEvent_t, hipEvent_t>>& list, double& sum_ms, long long& count, int reset, double* avg_ms,
                        long long* launches) {
  HIPCHK(hipSetDevice(b->device));
  for (auto& e : list) {
    HIPCHK(hipEventSynchronize(e.second));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, e.first, e.second));
    sum_ms += ms; count++;
    b->ev_pool.push_back(e.first); b->ev_pool.push_back(e.second);
  }
  list.clear();
  if (avg_ms) *avg_ms = count ? sum_ms / count : 0.0;
  if (launches) *launches = count;
  if (reset) { sum_ms = 0; count = 0; }
  return SG_OK;
}

// envs per solver wavefront (sg_pgs_rows_kernel<.., EPW>): 8 when that already gives every SIMD of the chip a wavefront
// (SG_EPW8_MIN_WAVES wavefronts of 8 envs), else 4; sg_set_solver_envs_per_wavefront / the env var SG_PGS_EPW override;
// neighbour-row models always run 4 envs of 16 lanes
#define SG_EPW8_MIN_WAVES 1024
static int solver_epw(const sg_batch* b) {
  if (b->m->plan.h.nnb > 0) return 4;
  if (b->epw_override) return b->epw_override;
  if (const char* pe = getenv("SG_PGS_EPW")) return atoi(pe) == 4 ? 4 : 8;
  return (b->n + 7) / 8 >= SG_EPW8_MIN_WAVES ? 8 : 4;
}

// split pipeline: phase(begin) -> pgs -> [phase(finish+begin) -> pgs]* -> phase(finish)
static int launch_split(sg_batch* b, int mode, const uint8_t* mask, int nsub, double* sens, long long stride, int32_t* flags, int32_t* touch,
                        hipStream_t s) {
  const SgPlanHeader& H = b->m->plan.h;
  SgPhaseArgs pa;
  pa.H = b->dH; pa.elem = b->delem;
  pa.qpos = b->qpos; pa.qvel = b->qvel; pa.warm = b->warm; pa.act = b->act; pa.ctrl = b->ctrl;
  pa.kenv = b->kenv; pa.kmask_jnt = b->kmask_jnt; pa.kmask_ten = b->kmask_ten;
  pa.mask = mask; pa.sens = nullptr; pa.sens_stride = stride > 0 ? stride : H.nsensordata;
  pa.w = b->w; pa.nenv = b->n; pa.rowlayout = b->pipeline == 2;
  pa.nbtab = b->dnbtab; pa.cpos = b->dcpos; pa.cst_rounds = (H.nnb > 0 && SG_ROWS_NB_MODE(H.nelem, H.eq_rounds) == 2) ? H.eq_rounds + 8 : 0;
  pa.gpairs = b->dgpairs;
  pa.nelem = H.nelem; pa.nv = H.nv; pa.nu = H.nu; pa.elem_dof0 = H.elem_dof0; pa.nchain = H.nchain; pa.t0_id = H.t0_id; pa.timestep = H.timestep;
  SgPgsArgs ga;
  ga.sched = b->dsched; ga.nbtab = b->dnbtab; ga.tab = b->dtab;
  ga.H = b->dH; ga.elem = b->delem; ga.w = b->w; ga.nenv = b->n;
  const size_t lds = sizeof(double) * ((size_t)(5 * 8 + 2) * H.nelem + 16 * 4 * SG_MAXLIM + 72);   // (split pipeline, test builds)
  (void)lds;
  // rows kernel: joint-fix rows per lane (template parameter, the smallest instantiated value >= ceil(nelem / 8)); its LDS
  // arrays are padded to 8 * NSL rows
  const int nsl = sg_rows_nsl(H.nelem);
  const bool nbm = H.nnb > 0;
  const int epw = solver_epw(b);
  const int nbmode = nbm ? SG_ROWS_NB_MODE(H.nelem, H.eq_rounds) : 0;
  const size_t lds_rows = sizeof(double) * (nbm ? SG_ROWS_LDS_NB(epw, H.nelem, H.eq_rounds, nbmode == 2) : SG_ROWS_LDS_FIX(epw, 8 * (size_t)nsl));
  if (!b->lds_attr_set) {  // per device: a batch on another GPU of the same process needs its own call
    HIPCHK(sg_rows_prepare());
#ifdef SG_LEGACY_PIPELINES
    HIPCHK(sg_legacy_prepare());
#endif
    b->lds_attr_set = true;
  }
  // forward passes to run: (mode 1: one non-integrating forward first) + nsub integrating ones
  const int nfwd = nsub + (mode == 1 ? 1 : 0);
  size_t call_ev = 0;
  if (b->prof) {
    if (int rc = begin_event_pair(b, b->ev, s)) return rc;
    call_ev = b->ev.size() - 1;
  }
  // the main pass over all envs, then (rows pipeline, forward passes only) the general contact pass: a small fixed grid whose
  // its blocks stride over W.gen_list, the envs the main pass has put there -- normally none, and then every block returns at once
  const bool genpass = b->pipeline == 2;
  for (int k = 0; k <= nfwd; k++) {
    SgPhaseArgs p = pa;
    p.first = k == 0;
    p.do_reset = (mode == 1 && k == 0);
    p.do_finish = k > 0;
    p.finish_integrate = (mode == 1) ? (k > 1) : 1;  // forward k-1 was the non-integrating one iff mode 1 and k == 1
    p.do_begin = k < nfwd;
    p.sens = (k == nfwd) ? sens : nullptr;
    if (nfwd == 0) { p.do_begin = 0; p.do_finish = 0; }
    HIPCHK(sg_launch_chain(p, b->n, s));
    p.sens = nullptr;  // the chain kernel writes the sensors (they all sit on finger sites)
    HIPCHK(sg_launch_phase(p, b->m->rounds, nbm, genpass, b->n, s));
    if (k < nfwd) {
      if (b->prof)
        if (int rc = begin_event_pair(b, b->ev_pgs, s)) return rc;
      if (b->pipeline == 2) HIPCHK(sg_launch_rows(ga, nsl, nbmode, epw, b->n, lds_rows, s));
#ifdef SG_LEGACY_PIPELINES
      else HIPCHK(sg_launch_pgs_split(ga, b->n, lds, s));
#endif
      if (b->prof) HIPCHK(hipEventRecord(b->ev_pgs.back().second, s));
    }
  }
  if (b->prof) HIPCHK(hipEventRecord(b->ev[call_ev].second, s));
  // outputs of the call: one small kernel for the five per-env int arrays (five device-to-device copies cost 1 % of a step);
  // with a mask (masked reset) only the selected envs' entries may change
  hipLaunchKernelGGL(sg_masked_copy_kernel, dim3((b->n + 255) / 256), dim3(256), 0, s, mask, b->n, b->w.status, flags ? flags : b->flags,
                     b->w.touch, touch ? touch : b->touch, b->w.ncon, b->ncon, b->w.nefc, b->nefc, b->w.iters, b->iters);
  HIPCHK(hipGetLastError());
  return SG_OK;
}

static int launch(sg_batch* b, int mode, const uint8_t* mask, int nsub, double* sens, long long stride, int32_t* flags, int32_t* touch,
                  hipStream_t s) {
  if (b->pipeline == 3) return launch_tree(b, mode, mask, nsub, sens, stride, flags, touch, s);
  if (b->pipeline >= 1) return launch_split(b, mode, mask, nsub, sens, stride, flags, touch, s);
#ifdef SG_LEGACY_PIPELINES
  const SgPlanHeader& H = b->m->plan.h;
  SgKArgs a;
  a.H = b->dH; a.elem = b->delem;
  a.qpos = b->qpos; a.qvel = b->qvel; a.warm = b->warm; a.act = b->act; a.ctrl = b->ctrl;
  a.kenv = b->kenv; a.kmask_jnt = b->kmask_jnt; a.kmask_ten = b->kmask_ten;
  a.mask = mask;
  a.sens = sens; a.sens_stride = stride > 0 ? stride : H.nsensordata;
  a.flags = flags ? flags : b->flags; a.touch = touch ? touch : b->touch;
  a.ncon = b->ncon; a.nefc = b->nefc; a.iters = b->iters;
  a.nenv = b->n; a.nsub = nsub; a.mode = mode;
  if (b->prof)
    if (int rc = begin_event_pair(b, b->ev, s)) return rc;
  HIPCHK(sg_launch_fused(a, b->m->rounds, b->n, s));
  if (b->prof) HIPCHK(hipEventRecord(b->ev.back().second, s));
  return SG_OK;
#else
  return fail(SG_ERR_MODEL, "the fused pipeline is not part of this build (test builds only: build_native.py --legacy)");
#endif
}

int sg_reset(sg_batch* b, const uint8_t* mask, int sim_start, double* sens_out, int32_t* flags_out, int32_t* touch_out, void* stream) {
  if (!b || sim_start < 0) return fail(SG_ERR_INVALID, "sg_reset: bad argument");
  HIPCHK(hipSetDevice(b->device));
  return launch(b, 1, mask, sim_start, sens_out, 0, flags_out, touch_out, (hipStream_t)stream);
}

int sg_step(sg_batch* b, int n_substeps, double* sens_out, long long sens_stride, int32_t* flags_out, int32_t* touch_out, void* stream) {
  if (!b || n_substeps < 0) return fail(SG_ERR_INVALID, "sg_step: bad argument");
  HIPCHK(hipSetDevice(b->device));
  return launch(b, 0, nullptr, n_substeps, sens_out, sens_stride, flags_out, touch_out, (hipStream_t)stream);
}

int sg_get_state(sg_batch* b, double* qpos, double* qvel, double* act, double* warm, double* ctrl, void* stream) {
  if (!b) return fail(SG_ERR_INVALID, "sg_get_state: bad argument");
  HIPCHK(hipSetDevice(b->device));
  hipStream_t s = (hipStream_t)stream;
  const size_t n = b->n, nv = b->m->plan.h.nv, nu = b->m->plan.h.nu;
  if (qpos) HIPCHK(hipMemcpyAsync(qpos, b->qpos, sizeof(double) * n * b->m->plan.h.nq, hipMemcpyDeviceToDevice, s));
  if (qvel) HIPCHK(hipMemcpyAsync(qvel, b->qvel, sizeof(double) * n * nv, hipMemcpyDeviceToDevice, s));
  if (warm) HIPCHK(hipMemcpyAsync(warm, b->warm, sizeof(double) * n * nv, hipMemcpyDeviceToDevice, s));
  if (act && nu) HIPCHK(hipMemcpyAsync(act, b->act, sizeof(double) * n * nu, hipMemcpyDeviceToDevice, s));
  if (ctrl && nu) HIPCHK(hipMemcpyAsync(ctrl, b->ctrl, sizeof(double) * n * nu, hipMemcpyDeviceToDevice, s));
  return SG_OK;
}

int sg_set_state(sg_batch* b, const double* qpos, const double* qvel, const double* act, const double* warm, const double* ctrl, void* stream) {
  if (!b) return fail(SG_ERR_INVALID, "sg_set_state: bad argument");
  HIPCHK(hipSetDevice(b->device));
  hipStream_t s = (hipStream_t)stream;
  const size_t n = b->n, nv = b->m->plan.h.nv, nu = b->m->plan.h.nu;
  if (qpos) HIPCHK(hipMemcpyAsync(b->qpos, qpos, sizeof(double) * n * b->m->plan.h.nq, hipMemcpyDeviceToDevice, s));
  if (qvel) HIPCHK(hipMemcpyAsync(b->qvel, qvel, sizeof(double) * n * nv, hipMemcpyDeviceToDevice, s));
  if (warm) HIPCHK(hipMemcpyAsync(b->warm, warm, sizeof(double) * n * nv, hipMemcpyDeviceToDevice, s));
  if (act && nu) HIPCHK(hipMemcpyAsync(b->act, act, sizeof(double) * n * nu, hipMemcpyDeviceToDevice, s));
  if (ctrl && nu) HIPCHK(hipMemcpyAsync(b->ctrl, ctrl, sizeof(double) * n * nu, hipMemcpyDeviceToDevice, s));
  return SG_OK;
}

int sg_get_solver_stats(sg_batch* b, int32_t* ncon, int32_t* nefc, int32_t* iters, void* stream) {
  if (!b) return fail(SG_ERR_INVALID, "sg_get_solver_stats: bad argument");
  HIPCHK(hipSetDevice(b->device));
  hipStream_t s = (hipStream_t)stream;
  const size_t n = b->n;
  if (ncon) HIPCHK(hipMemcpyAsync(ncon, b->ncon, sizeof(int) * n, hipMemcpyDeviceToDevice, s));
  if (nefc) HIPCHK(hipMemcpyAsync(nefc, b->nefc, sizeof(int) * n, hipMemcpyDeviceToDevice, s));
  if (iters) HIPCHK(hipMemcpyAsync(iters, b->iters, sizeof(int) * n, hipMemcpyDeviceToDevice, s));
  return SG_OK;
}

int sg_set_pipeline(sg_batch* b, int pipeline) {
  if (!b || pipeline < 0 || pipeline > 3) return fail(SG_ERR_INVALID, "sg_set_pipeline: bad argument");
  if (pipeline == 3) {
    if (!b->m->has_tree) return fail(SG_ERR_MODEL, "sg_set_pipeline: the tree pipeline does not run this model (fix-rows-only models within its capacities)");
    HIPCHK(hipSetDevice(b->device));
    if (int rc = tree_alloc(b)) return rc;
    b->pipeline = 3;
    return SG_OK;
  }
  if (!b->m->has_fast) return fail(SG_ERR_MODEL, "sg_set_pipeline: the model is outside the two-finger class, only the tree pipeline runs it");
#ifndef SG_LEGACY_PIPELINES
  if (pipeline < 2) return fail(SG_ERR_MODEL, "sg_set_pipeline: the fused and split pipelines are not part of this build (test builds only: build_native.py --legacy)");
#endif
  if (b->m->plan.h.nnb > 0 && pipeline != 2)
    return fail(SG_ERR_MODEL, "sg_set_pipeline: the model has neighbour equality rows, which only the rows pipeline supports");
  b->pipeline = pipeline;
  return SG_OK;
}

int sg_get_touch_words(sg_batch* b, int32_t* out, int nwords, void* stream) {
  if (!b || !out || nwords < 1) return fail(SG_ERR_INVALID, "sg_get_touch_words: bad argument");
  HIPCHK(hipSetDevice(b->device));
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(hipMemsetAsync(out, 0, sizeof(int32_t) * (size_t)b->n * nwords, s));
  if (b->pipeline == 3)
    HIPCHK(hipMemcpy2DAsync(out, sizeof(int32_t) * nwords, b->t.touch_words, sizeof(int32_t) * 2, sizeof(int32_t) * (nwords < 2 ? nwords : 2), b->n,
                            hipMemcpyDeviceToDevice, s));
  else
    HIPCHK(hipMemcpy2DAsync(out, sizeof(int32_t) * nwords, b->pipeline == 0 ? b->touch : b->w.touch, sizeof(int32_t), sizeof(int32_t), b->n,
                            hipMemcpyDeviceToDevice, s));
  return SG_OK;
}
int sg_model_nboxes(const sg_model* m) {
  if (!m) return 0;
  if (!m->has_fast) return m->tree.NG;
  int n = 0;
  for (int c = 0; c < m->plan.h.nchain; c++) n += m->plan.h.chain[c].ngeom;
  return n;
}

int sg_set_solver_envs_per_wavefront(sg_batch* b, int epw) {
  if (!b || (epw != 0 && epw != 4 && epw != 8)) return fail(SG_ERR_INVALID, "sg_set_solver_envs_per_wavefront: 0 (automatic), 4 or 8");
  if (b->m->plan.h.nnb > 0 && epw == 8)
    return fail(SG_ERR_MODEL, "sg_set_solver_envs_per_wavefront: a model with neighbour equality rows runs 4 envs of 16 lanes per wavefront");
  b->epw_override = epw;
  return SG_OK;
}
int sg_solver_envs_per_wavefront(const sg_batch* b) { return b ? solver_epw(b) : 0; }
int sg_tree_workgroups_per_cu(const sg_batch* b) {
  if (!b) return fail(SG_ERR_INVALID, "sg_tree_workgroups_per_cu: bad argument");
  if (!b->tree_ready) return 0;
  const sg_model* m = b->m;
  if (hipSetDevice(b->device) != hipSuccess) return fail(SG_ERR_NO_DEVICE, "hipSetDevice");
  if (sg_tree_prepare() != hipSuccess) return fail(SG_ERR_HIP, "sg_tree_prepare");
  return sg_tree_occupancy(m->tree.CS, m->tree_lds);
}

#ifdef SG_SECTION_PROF
// profiling build only (build_native.py --prof, scripts/section_profile.py): read and clear the per-section cycle sums
int sg_debug_sections(sg_batch* b, unsigned long long* out32) {
  if (!b || !out32) return fail(SG_ERR_INVALID, "sg_debug_sections: bad argument");
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(out32, b->w.secprof, sizeof(unsigned long long) * 48, hipMemcpyDeviceToHost));
  HIPCHK(hipMemset(b->w.secprof, 0, sizeof(unsigned long long) * 48));
  return SG_OK;
}
#endif

#ifdef SG_DEBUG_WORK
// debugging build only (build_native.py --ko NAME -DSG_DEBUG_WORK, scripts/dev/work_diff.py): one env's tree-pipeline work space
// (sg_tree.h: staged narrowphase records | contact rows | mass-matrix blocks | the arrays lds_carve backs with global memory), to be
// held word by word against the host emulation's after the same launch.  -> the number of doubles copied (<= cap), or a negative error
long long sg_debug_tree_work(sg_batch* b, int env, double* out, long long cap) {
  if (!b || !out || env < 0 || env >= b->n || !b->t.cws) return fail(SG_ERR_INVALID, "sg_debug_tree_work: bad argument");
  const sg_model* m = b->m;
  long long n = m->tree_cws;
  if (n > cap) n = cap;
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(out, b->t.cws + (size_t)env * m->tree_cws, sizeof(double) * n, hipMemcpyDeviceToHost));
  return n;
}
#endif

int sg_profile_enable(sg_batch* b, int enable) {
  if (!b) return fail(SG_ERR_INVALID, "sg_profile_enable: bad argument");
  b->prof = enable != 0;
  return SG_OK;
}

int sg_profile_read_solver(sg_batch* b, int reset, double* avg_ms, long long* launches) {
  if (!b) return fail(SG_ERR_INVALID, "sg_profile_read_solver: bad argument");
  return profile_read(b, b->ev_pgs, b->prof_pgs_ms, b->prof_pgs_n, reset, avg_ms, launches);
}

int sg_profile_read(sg_batch* b, int reset, double* avg_ms, long long* launches) {
  if (!b) return fail(SG_ERR_INVALID, "sg_profile_read: bad argument");
  return profile_read(b, b->ev, b->prof_ms, b->prof_n, reset, avg_ms, launches);
}

// ---- pose read-out and renderer (sg_kin.hip) ----
int sg_model_nbody(const sg_model* m) { return m ? m->kin.o.nbody : 0; }
int sg_model_ngeom(const sg_model* m) { return m ? m->kin.o.ngeom : 0; }

int sg_model_default_camera(const sg_model* m, double* cam) {
  if (!m || !cam) return fail(SG_ERR_INVALID, "sg_model_default_camera: null argument");
  if (!m->kin.ok) return fail(SG_ERR_MODEL, "sg_model_default_camera: " + m->kin.err);
  sgk_default_camera(m->kin, cam);
  return SG_OK;
}

// the kinematics table on the batch's device and the listed env ids (host array, range-checked here) in a device buffer
static int kin_prepare(sg_batch* b, const char* fn, const int32_t* env_ids, int n_ids, hipStream_t s, const int** dids) {
  const SgKinHost& K = b->m->kin;
  if (!K.ok) return fail(SG_ERR_MODEL, std::string(fn) + ": " + K.err);
  if (n_ids <= 0) return fail(SG_ERR_INVALID, std::string(fn) + ": n_ids must be positive");
  if (!env_ids && n_ids != b->n) return fail(SG_ERR_INVALID, std::string(fn) + ": env_ids == NULL needs n_ids == the batch's env count");
  if (env_ids)
    for (int i = 0; i < n_ids; i++)
      if (env_ids[i] < 0 || env_ids[i] >= b->n)
        return fail(SG_ERR_INVALID, std::string(fn) + ": env id " + std::to_string(env_ids[i]) + " out of range [0, " + std::to_string(b->n) + ")");
  HIPCHK(hipSetDevice(b->device));
  if (!b->kin_d) {   // built on the side: the batch sees the tables only once both are filled
    SgArena A;
    double* d = nullptr;
    int* ip = nullptr;
    if (!(A.upload(&d, K.dbl) && A.upload(&ip, K.ints))) return devmem_fail(A.nomem, std::string(fn) + " (pose tables)");
    A.give_to(b->mem);
    b->kin_d = d; b->kin_i = ip;
  }
  *dids = nullptr;
  if (env_ids) {
    if (!b->kin_ids.reserve(n_ids, s)) return devmem_fail(b->kin_ids.nomem, std::string(fn) + " (env ids)");
    HIPCHK(hipMemcpyAsync(b->kin_ids.p, env_ids, sizeof(int) * n_ids, hipMemcpyHostToDevice, s));
    *dids = b->kin_ids.p;
  }
  return SG_OK;
}

static int launch_kin(sg_batch* b, const int* dids, int n_ids, double* xpos, double* xquat, double* gxpos, double* gxmat, float* recs,
                      const double* eye, hipStream_t s) {
  const SgKinHost& K = b->m->kin;
  SgKinArgs a;
  a.D = b->kin_d; a.I = b->kin_i; a.o = K.o; a.qpos = b->qpos; a.env_ids = dids; a.n_ids = n_ids;
  a.xpos = xpos; a.xquat = xquat; a.gxpos = gxpos; a.gxmat = gxmat; a.recs = recs;
  for (int c = 0; c < 3; c++) a.eye[c] = eye ? eye[c] : 0.0;
  hipLaunchKernelGGL(sg_kin_kernel, dim3(n_ids), dim3(64), sizeof(double) * 7 * K.o.nbody, s, a);
  HIPCHK(hipGetLastError());
  return SG_OK;
}

int sg_get_poses(sg_batch* b, const int32_t* env_ids, int n_ids, double* xpos, double* xquat, double* geom_xpos, double* geom_xmat, void* stream) {
  if (!b) return fail(SG_ERR_INVALID, "sg_get_poses: null batch");
  hipStream_t s = (hipStream_t)stream;
  const int* dids = nullptr;
  if (int rc = kin_prepare(b, "sg_get_poses", env_ids, n_ids, s, &dids)) return rc;
  if (!xpos && !xquat && !geom_xpos && !geom_xmat) return SG_OK;
  return launch_kin(b, dids, n_ids, xpos, xquat, geom_xpos, geom_xmat, nullptr, nullptr, s);
}

// the argument and model checks both render entry points share (before anything touches the device)
static int render_check(const char* fn, const sg_batch* b, const double* cam, int width, int height) {
  const std::string f = std::string(fn) + ": ";
  if (!b || !cam) return fail(SG_ERR_INVALID, f + "null batch or camera");
  if (width <= 0 || height <= 0 || width > 16384 || height > 16384) return fail(SG_ERR_INVALID, f + "image size out of range (1 .. 16384)");
  for (int c = 0; c < 7; c++)
    if (!std::isfinite(cam[c])) return fail(SG_ERR_INVALID, f + "camera values must be finite");
  if (!(cam[3] > 0) || !(cam[6] > 0 && cam[6] < 180)) return fail(SG_ERR_INVALID, f + "camera distance must be > 0 and fovy in (0, 180)");
  const SgKinHost& K = b->m->kin;
  if (K.ok && K.bad_type >= 0)
    return fail(SG_ERR_MODEL, f + "geom type " + std::to_string(K.bad_type) + " has no ray intersection (plane, sphere, capsule and box only)");
  if (K.ok && K.o.ngeom > SGR_MAXGEOM) return fail(SG_ERR_MODEL, f + "more than " + std::to_string(SGR_MAXGEOM) + " geoms");
  return SG_OK;
}

int sg_render(sg_batch* b, const double* cam, const int32_t* env_ids, int n_ids, int width, int height, uint8_t* rgba, float* depth, int32_t* segid,
              void* stream) {
  if (int rc = render_check("sg_render", b, cam, width, height)) return rc;
  const SgKinHost& K = b->m->kin;
  hipStream_t s = (hipStream_t)stream;
  const int* dids = nullptr;
  if (int rc = kin_prepare(b, "sg_render", env_ids, n_ids, s, &dids)) return rc;
  if (!b->rrecs.reserve((size_t)n_ids * K.o.ngeom * SGR_REC, s)) return devmem_fail(b->rrecs.nomem, "sg_render (geom records)");
  SgRenderArgs a;
  double eye[3];
  sgr_camera(cam, width, height, eye, &a.cam);
  if (int rc = launch_kin(b, dids, n_ids, nullptr, nullptr, nullptr, nullptr, b->rrecs.p, eye, s)) return rc;
  a.recs = b->rrecs.p; a.ngeom = K.o.ngeom; a.n_ids = n_ids;
  a.tiles_x = (width + SGR_TILE - 1) / SGR_TILE;
  a.ntiles = a.tiles_x * ((height + SGR_TILE - 1) / SGR_TILE);
  a.rgba = rgba; a.depth = depth; a.segid = segid;
  if (!rgba && !depth && !segid) return SG_OK;
  if ((long long)a.ntiles * n_ids > 0x7fffffffll) return fail(SG_ERR_INVALID, "sg_render: too many tiles x envs for one launch");
  hipLaunchKernelGGL(sg_render_kernel, dim3((unsigned)(a.ntiles * n_ids)), dim3(256), 0, s, a);
  HIPCHK(hipGetLastError());
  return SG_OK;
}

// ---- the skin (sg_skin.h, sg_kin.hip) ----
int sg_model_set_skin(sg_model* m, int nvert, const int32_t* vert_body, const double* vert_pos, int nface, const int32_t* face, const float* rgba) {
  if (!m) return fail(SG_ERR_INVALID, "sg_model_set_skin: null model");
  if (nvert < 0 || nface < 0) return fail(SG_ERR_INVALID, "sg_model_set_skin: negative count");
  if (nvert == 0) {   // removes the skin
    m->skin.nvert = m->skin.nface = 0;
    m->skin.vert_body.clear(); m->skin.vert_pos.clear(); m->skin.face.clear();
    m->skin.version++;
    return SG_OK;
  }
  if (!m->kin.ok) return fail(SG_ERR_MODEL, "sg_model_set_skin: " + m->kin.err);
  if (nvert > SGR_MAXVERT || nface > SGR_MAXFACE)
    return fail(SG_ERR_MODEL, "sg_model_set_skin: more than " + std::to_string(SGR_MAXVERT) + " vertices or " + std::to_string(SGR_MAXFACE) + " faces");
  if (!vert_body || !vert_pos || !rgba || (nface > 0 && !face)) return fail(SG_ERR_INVALID, "sg_model_set_skin: null array with a positive count");
  for (int v = 0; v < nvert; v++) {
    if (vert_body[v] < 0 || vert_body[v] >= m->kin.o.nbody)
      return fail(SG_ERR_INVALID, "sg_model_set_skin: vertex " + std::to_string(v) + " is bound to body " + std::to_string(vert_body[v]) + ", outside [0, nbody)");
    for (int c = 0; c < 3; c++)
      if (!std::isfinite(vert_pos[3 * v + c])) return fail(SG_ERR_INVALID, "sg_model_set_skin: vertex positions must be finite");
  }
  for (int f = 0; f < nface; f++) {
    const int32_t* q = face + 3 * f;
    for (int c = 0; c < 3; c++)
      if (q[c] < 0 || q[c] >= nvert) return fail(SG_ERR_INVALID, "sg_model_set_skin: face " + std::to_string(f) + " has a vertex index outside [0, nvert)");
    if (q[0] == q[1] || q[1] == q[2] || q[0] == q[2]) return fail(SG_ERR_INVALID, "sg_model_set_skin: face " + std::to_string(f) + " repeats a vertex");
  }
  for (int c = 0; c < 4; c++)
    if (!std::isfinite(rgba[c])) return fail(SG_ERR_INVALID, "sg_model_set_skin: rgba must be finite");
  SgSkinHost& S = m->skin;
  S.nvert = nvert; S.nface = nface;
  S.vert_body.assign(vert_body, vert_body + nvert);
  S.vert_pos.assign(vert_pos, vert_pos + 3 * (size_t)nvert);
  S.face.assign(face, face + 3 * (size_t)nface);
  for (int c = 0; c < 4; c++) S.rgba[c] = rgba[c];
  S.version++;
  return SG_OK;
}

int sg_model_skin(const sg_model* m, int* nvert, int* nface, int32_t* vert_body, double* vert_pos, int32_t* face, float* rgba) {
  if (!m) return fail(SG_ERR_INVALID, "sg_model_skin: null model");
  const SgSkinHost& S = m->skin;
  if (nvert) *nvert = S.nvert;
  if (nface) *nface = S.nface;
  if (vert_body) std::copy(S.vert_body.begin(), S.vert_body.end(), vert_body);
  if (vert_pos) std::copy(S.vert_pos.begin(), S.vert_pos.end(), vert_pos);
  if (face) std::copy(S.face.begin(), S.face.end(), face);
  if (rgba)
    for (int c = 0; c < 4; c++) rgba[c] = S.rgba[c];
  return SG_OK;
}

// the skin's tables on the batch's device, uploaded again when the model's skin has changed since (an earlier skin render, on whatever
// stream it went out, may still read the old ones: the device is waited for first -- once per sg_model_set_skin, not per render)
static int skin_prepare(sg_batch* b) {
  const SgSkinHost& S = b->m->skin;
  if (b->skin_version == S.version) return SG_OK;
  const SgKinHost& K = b->m->kin;
  SgSkinTables T;
  sg_skin_tables(S, K.ints.data() + K.o.gbody, K.o.ngeom, K.o.nbody, &T);
  HIPCHK(hipDeviceSynchronize());
  b->skin_version = 0;
  b->skin_mem.release();
  SgArena& A = b->skin_mem;
  int *vb = nullptr, *as = nullptr, *ad = nullptr, *hid = nullptr;
  double* vp = nullptr;
  uint32_t* fc = nullptr;
  if (!(A.upload(&vb, S.vert_body) && A.upload(&vp, S.vert_pos) && A.upload(&fc, T.faces) && A.upload(&as, T.adj_start) && A.upload(&ad, T.adj) &&
        A.upload(&hid, T.hidden))) {
    const bool nomem = A.nomem;
    A.release();
    return devmem_fail(nomem, "sg_render_ex (skin tables)");
  }
  SgSkinDev& d = b->skin_dev;
  d.vert_body = vb; d.vert_pos = vp; d.faces = fc; d.adj_start = as; d.adj = ad; d.hidden = hid;
  d.nvert = S.nvert; d.nface = S.nface;
  for (int c = 0; c < 3; c++) d.rgb[c] = S.rgba[c];
  b->skin_version = S.version;
  return SG_OK;
}

int sg_render_ex(sg_batch* b, const double* cam, const int32_t* env_ids, int n_ids, int width, int height, int flags, uint8_t* rgba, float* depth,
                 int32_t* segid, void* stream) {
  if (flags & ~SG_RENDER_SKIN) return fail(SG_ERR_INVALID, "sg_render_ex: unknown flag bits");
  if (!b || !cam) return fail(SG_ERR_INVALID, "sg_render_ex: null batch or camera");
  if (!(flags & SG_RENDER_SKIN) || b->m->skin.nvert == 0) return sg_render(b, cam, env_ids, n_ids, width, height, rgba, depth, segid, stream);
  if (int rc = render_check("sg_render_ex", b, cam, width, height)) return rc;
  const SgKinHost& K = b->m->kin;
  const SgSkinHost& S = b->m->skin;
  hipStream_t s = (hipStream_t)stream;
  const int* dids = nullptr;
  if (int rc = kin_prepare(b, "sg_render_ex", env_ids, n_ids, s, &dids)) return rc;
  if (int rc = skin_prepare(b)) return rc;
  const size_t nb = K.o.nbody;
  if (!b->rrecs.reserve((size_t)n_ids * K.o.ngeom * SGR_REC, s)) return devmem_fail(b->rrecs.nomem, "sg_render_ex (geom records)");
  if (!b->skin_xpos.reserve((size_t)n_ids * nb * 3, s)) return devmem_fail(b->skin_xpos.nomem, "sg_render_ex (body poses)");
  if (!b->skin_xquat.reserve((size_t)n_ids * nb * 4, s)) return devmem_fail(b->skin_xquat.nomem, "sg_render_ex (body poses)");
  if (!b->skin_vrec.reserve((size_t)n_ids * S.nvert * SGR_VREC, s)) return devmem_fail(b->skin_vrec.nomem, "sg_render_ex (vertex records)");
  SgSkinRenderArgs A;
  SgRenderArgs& a = A.r;
  double eye[3];
  sgr_camera(cam, width, height, eye, &a.cam);
  if (int rc = launch_kin(b, dids, n_ids, b->skin_xpos.p, b->skin_xquat.p, nullptr, nullptr, b->rrecs.p, eye, s)) return rc;
  SgSkinVertArgs V;
  V.s = b->skin_dev; V.xpos = b->skin_xpos.p; V.xquat = b->skin_xquat.p; V.nbody = K.o.nbody; V.vrec = b->skin_vrec.p;
  for (int c = 0; c < 3; c++) V.eye[c] = eye[c];
  hipLaunchKernelGGL(sg_skin_vert_kernel, dim3(n_ids), dim3(256), 0, s, V);
  HIPCHK(hipGetLastError());
  a.recs = b->rrecs.p; a.ngeom = K.o.ngeom; a.n_ids = n_ids;
  a.tiles_x = (width + SGR_TILE - 1) / SGR_TILE;
  a.ntiles = a.tiles_x * ((height + SGR_TILE - 1) / SGR_TILE);
  a.rgba = rgba; a.depth = depth; a.segid = segid;
  A.s = b->skin_dev; A.vrec = b->skin_vrec.p;
  if (!rgba && !depth && !segid) return SG_OK;
  if ((long long)a.ntiles * n_ids > 0x7fffffffll) return fail(SG_ERR_INVALID, "sg_render_ex: too many tiles x envs for one launch");
  hipLaunchKernelGGL(sg_rskin_kernel, dim3((unsigned)(a.ntiles * n_ids)), dim3(256), 0, s, A);
  HIPCHK(hipGetLastError());
  return SG_OK;
}

// ---- contact read-out (sg_contacts.hip) ----
int sg_model_ncollision_pairs(const sg_model* m) {
  if (!m) return 0;
  if (!m->con.ok) return fail(SG_ERR_MODEL, "sg_model_ncollision_pairs: " + m->con.err);
  return (int)(m->con.pairs.size() / 2);
}

int sg_get_contacts(sg_batch* b, const int32_t* env_ids, int n_ids, int max_contacts, int32_t* ncon, int32_t* geom, double* dist, double* pos,
                    double* frame, void* stream) {
  // (argument checks first, in an order that lets each be reached without a device)
  if (n_ids <= 0) return fail(SG_ERR_INVALID, "sg_get_contacts: n_ids must be positive");
  if (max_contacts <= 0 && (geom || dist || pos || frame)) return fail(SG_ERR_INVALID, "sg_get_contacts: max_contacts must be positive when a contact array is given");
  if (!b) return fail(SG_ERR_INVALID, "sg_get_contacts: null batch");
  const SgConHost& Cn = b->m->con;
  const SgKinHost& K = b->m->kin;
  if (K.ok && !Cn.ok) return fail(SG_ERR_MODEL, "sg_get_contacts: " + Cn.err);
  hipStream_t s = (hipStream_t)stream;
  const int* dids = nullptr;
  if (int rc = kin_prepare(b, "sg_get_contacts", env_ids, n_ids, s, &dids)) return rc;
  if (!ncon && !geom && !dist && !pos && !frame) return SG_OK;
  if (!b->con_pairs) {   // (on the side, as the pose tables)
    SgArena A;
    int* dp = nullptr;
    double* dg = nullptr;
    if (!(A.upload(&dp, Cn.pairs) && A.upload(&dg, Cn.gaux))) return devmem_fail(A.nomem, "sg_get_contacts (pair tables)");
    A.give_to(b->mem);
    b->con_pairs = dp; b->con_gaux = dg;
  }
  const size_t npose = sgc_pose_doubles(K.o);
  const size_t lds = sizeof(double) * (SGC_FIXED_DBL + npose);
  const bool in_lds = lds <= 159 * 1024;   // (the kernel has 256 B of static LDS besides; the CU has 160 KB)
  if (!in_lds && !b->con_scratch.reserve((size_t)n_ids * npose, s)) return devmem_fail(b->con_scratch.nomem, "sg_get_contacts (pose blocks)");
  if (in_lds && !b->con_attr_set) {   // per device, as the solver kernels' attribute; what this model's launches ask for (above 64 KB it must be granted)
    HIPCHK(hipFuncSetAttribute((const void*)sg_contacts_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    b->con_attr_set = true;
  }
  SgConArgs a;
  a.D = b->kin_d; a.I = b->kin_i; a.o = K.o; a.gaux = b->con_gaux; a.pairs = b->con_pairs; a.npair = (int)(Cn.pairs.size() / 2); a.cap = Cn.cap;
  a.qpos = b->qpos; a.env_ids = dids; a.n_ids = n_ids; a.max_contacts = max_contacts;
  a.ncon = ncon; a.geom = geom; a.dist = dist; a.pos = pos; a.frame = frame; a.scratch = in_lds ? nullptr : b->con_scratch.p;
  if (in_lds) hipLaunchKernelGGL(sg_contacts_kernel<true>, dim3(n_ids), dim3(64), lds, s, a);
  else hipLaunchKernelGGL(sg_contacts_kernel<false>, dim3(n_ids), dim3(64), sizeof(double) * SGC_FIXED_DBL, s, a);
  HIPCHK(hipGetLastError());
  return SG_OK;
}

// ---- ray queries (sg_ray.hip) ----
// Which layout a call gets: lanes over geoms below SG_RAY_CROSSOVER rays per env, lane per ray from there on.  Measured (DESIGN.md 8.3,
// profiles/r08_ray_bench.json; 4096 envs, softbox): lanes over geoms wins at 16 rays per env (0.18 against 0.33 ms) and loses at 64 (0.55
// against 0.40 ms); the two lines cross near 34.  SG_RAY_LAYOUT=rays|geoms, read per call, forces one (the tests run both at every shape).
#define SG_RAY_CROSSOVER 32
int sg_ray(sg_batch* b, const int32_t* env_ids, int n_ids, int n_rays, const double* origin, const double* dir, const int32_t* ray_body,
           const int32_t* ray_exclude, int cat_mask, double max_dist, int flags, double* dist, int32_t* geomid, double* normal, void* stream) {
  // (argument checks first, in an order that lets most be reached without a device)
  if (n_ids <= 0 || n_rays <= 0) return fail(SG_ERR_INVALID, "sg_ray: n_ids and n_rays must be positive");
  if (cat_mask < 1 || cat_mask > SG_RAY_ALL) return fail(SG_ERR_INVALID, "sg_ray: cat_mask outside [1, 31]");
  if (flags & ~SG_RAY_PER_ENV) return fail(SG_ERR_INVALID, "sg_ray: unknown flag bits");
  if (!std::isfinite(max_dist)) return fail(SG_ERR_INVALID, "sg_ray: max_dist must be finite (<= 0: unlimited)");
  if (!b || !origin || !dir) return fail(SG_ERR_INVALID, "sg_ray: null batch, origin or dir");
  const SgKinHost& K = b->m->kin;
  if (K.ok)
    for (const int32_t* ids : {ray_body, ray_exclude})
      for (int r = 0; ids && r < n_rays; r++)
        if (ids[r] < -1 || ids[r] >= K.o.nbody)
          return fail(SG_ERR_INVALID, "sg_ray: body id " + std::to_string(ids[r]) + " of ray " + std::to_string(r) + " outside [-1, " + std::to_string(K.o.nbody) + ")");
  if (K.ok && K.bad_type >= 0)
    return fail(SG_ERR_MODEL, "sg_ray: geom type " + std::to_string(K.bad_type) + " has no ray intersection (plane, sphere, capsule and box only)");
  if (K.ok && K.o.ngeom > SGY_MAXGEOM) return fail(SG_ERR_MODEL, "sg_ray: more than " + std::to_string(SGY_MAXGEOM) + " geoms");
  if ((long long)n_ids * n_rays > 0x7fffffffll) return fail(SG_ERR_INVALID, "sg_ray: too many envs x rays for one launch");
  hipStream_t s = (hipStream_t)stream;
  const int* dids = nullptr;
  if (int rc = kin_prepare(b, "sg_ray", env_ids, n_ids, s, &dids)) return rc;
  if (!dist && !geomid && !normal) return SG_OK;
  const size_t nb = K.o.nbody, ng = K.o.ngeom;
  if (!b->ray_xpos.reserve((size_t)n_ids * nb * 3, s)) return devmem_fail(b->ray_xpos.nomem, "sg_ray (body poses)");
  if (!b->ray_xquat.reserve((size_t)n_ids * nb * 4, s)) return devmem_fail(b->ray_xquat.nomem, "sg_ray (body poses)");
  if (!b->ray_gxpos.reserve((size_t)n_ids * (ng ? ng : 1) * 3, s)) return devmem_fail(b->ray_gxpos.nomem, "sg_ray (geom poses)");
  if (!b->ray_gxmat.reserve((size_t)n_ids * (ng ? ng : 1) * 9, s)) return devmem_fail(b->ray_gxmat.nomem, "sg_ray (geom poses)");
  if (!b->ray_ids.reserve(2 * (size_t)n_rays, s)) return devmem_fail(b->ray_ids.nomem, "sg_ray (ray body ids)");
  if (ray_body) HIPCHK(hipMemcpyAsync(b->ray_ids.p, ray_body, sizeof(int) * n_rays, hipMemcpyHostToDevice, s));
  if (ray_exclude) HIPCHK(hipMemcpyAsync(b->ray_ids.p + n_rays, ray_exclude, sizeof(int) * n_rays, hipMemcpyHostToDevice, s));
  if (int rc = launch_kin(b, dids, n_ids, b->ray_xpos.p, b->ray_xquat.p, b->ray_gxpos.p, b->ray_gxmat.p, nullptr, nullptr, s)) return rc;
  SgRayArgs a;
  a.D = b->kin_d; a.I = b->kin_i; a.gsize = K.o.gsize; a.gmeta = K.o.gmeta; a.gbody = K.o.gbody; a.ngeom = K.o.ngeom; a.nbody = K.o.nbody;
  a.xpos = b->ray_xpos.p; a.xquat = b->ray_xquat.p; a.gxpos = b->ray_gxpos.p; a.gxmat = b->ray_gxmat.p;
  a.origin = origin; a.dir = dir;
  a.ray_body = ray_body ? b->ray_ids.p : nullptr; a.ray_exclude = ray_exclude ? b->ray_ids.p + n_rays : nullptr;
  a.n_ids = n_ids; a.n_rays = n_rays; a.per_env = (flags & SG_RAY_PER_ENV) ? 1 : 0; a.cat_mask = cat_mask;
  a.limit = max_dist > 0 ? max_dist : INFINITY;
  a.dist = dist; a.geomid = geomid; a.normal = normal;
  bool by_geoms = n_rays < SG_RAY_CROSSOVER;
  if (const char* forced = getenv("SG_RAY_LAYOUT")) {
    if (!strcmp(forced, "rays")) by_geoms = false;
    else if (!strcmp(forced, "geoms")) by_geoms = true;
    else if (*forced) return fail(SG_ERR_INVALID, "sg_ray: SG_RAY_LAYOUT must be rays or geoms");
  }
  if (by_geoms) {
    hipLaunchKernelGGL(sg_ray_geoms_kernel, dim3((unsigned)((long long)n_ids * n_rays)), dim3(64), 0, s, a);
  } else {
    const int nblk = (n_rays + 255) / 256;
    hipLaunchKernelGGL(sg_ray_rays_kernel, dim3((unsigned)((long long)n_ids * nblk)), dim3(256), sizeof(double) * SGY_REC * (ng ? ng : 1), s, a, nblk);
  }
  HIPCHK(hipGetLastError());
  return SG_OK;
}

}  // extern "C"
