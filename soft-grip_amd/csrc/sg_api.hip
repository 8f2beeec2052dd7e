// sg_api.hip -- C ABI (include/softgrip.h) over the gfx950 kernels: models, batches and the step path (the read-outs: sg_readout.hip).
// No CPU fallback.
#include <cstdio>
#include <cstring>
#include <memory>

#include "sg_batch.h"   // sg_model, sg_batch, fail, HIPCHK, devmem_fail: shared with the read-outs (sg_readout.hip)
#include "sg_blob.h"
#include "sg_mjcf.h"
#include "sg_tree.h"
#ifdef SG_LEGACY_PIPELINES
#include "sg_kernels_args.h"
#define SG_LEGACY_ON 1
#else
#define SG_LEGACY_ON 0   // (the split pipeline's contact records, 126 MB at 4096 envs, are then not allocated)
#endif

static thread_local std::string g_err;
int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
int devmem_fail(bool nomem, const std::string& what) {
  (void)hipGetLastError();   // (the failed call's error must not stay behind as the thread's last one: the next launch check, ours or the caller's, would report it)
  return fail(nomem ? SG_ERR_NOMEM : SG_ERR_HIP, what + (nomem ? ": out of device memory" : ": a HIP memset, copy or synchronise failed"));
}

namespace {
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
  if (!ok) {
    A.release();
    t = SgTreeBufs();
    return devmem_fail(A.nomem, "tree pipeline");
  }
  b->tree_ready = true;
  return SG_OK;
}

// the same for pipelines 0 .. 2: the plan's tables, the solver's (sg_rows_host.h) and the work space, every buffer sized by
// sg_rows_work_each -- ~0.1 MB per env, which a batch that only ever runs the tree pipeline does not hold
static int rows_alloc(sg_batch* b) {
  SgRowsBufs& r = b->r;
  if (r.ready) return SG_OK;
  const sg_model* m = b->m;
  const SgPlanHeader& H = m->plan.h;
  SgArena& A = b->rows_mem;
  r.shape = sg_rows_shape(H);
  r.nsl = sg_rows_nsl(H.nelem);
  r.w.secprof = b->secprof;
  bool ok = A.zeros(&r.H, 1) && hipMemcpy(r.H, &H, sizeof H, hipMemcpyHostToDevice) == hipSuccess && A.upload(&r.elem, sg_rows_elem_table(m->plan)) &&
            A.upload(&r.gpairs, m->plan.gpairs) &&
            sg_rows_work_each(r.w, H, m->rounds, (size_t)b->n, SG_LEGACY_ON != 0, [&A](auto** p, size_t count) { return A.zeros(p, count); });
  if (ok && r.shape.nb_mode) {
    SgRowsTables T;
    sg_rows_tables(m->plan, &T);
    ok = A.upload(&r.nbtab, m->plan.nbtab) && A.upload(&r.sched, T.sched) && A.upload(&r.tab, T.tab) && A.upload(&r.cpos, T.cpos);
  }
  if (!ok) {
    A.release();
    r = SgRowsBufs();
    return devmem_fail(A.nomem, "rows pipeline");
  }
  r.ready = true;
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
  a.nenv = b->n; a.nsub = nsub; a.mode = mode; a.secprof = b->secprof;
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
  sg_tables_build(blob, nbytes, m->has_fast ? m->plan : m->tplan, m->has_tree ? &m->tree : nullptr, m->has_fast, m);
  m->rounds = (m->plan.h.nelem + 63) / 64;
  if (m->rounds > 4) {
    delete m;
    return fail(SG_ERR_MODEL, "sg_model_create: more than 256 composite elements");
  }
  if (m->has_fast && !sg_rows_admits(m->plan.h, &err)) {
    delete m;
    return fail(SG_ERR_MODEL, "sg_model_create: " + err);
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

// the pipeline a new batch starts on: the rows pipeline for the two-finger class, unless SG_PIPELINE names another that runs the model
static int first_pipeline(const sg_model* m) {
  if (!m->has_fast) return 3;
  const char* pm = getenv("SG_PIPELINE");
  int p = (pm && strcmp(pm, "tree") == 0 && m->has_tree) ? 3 : 2;
#ifdef SG_LEGACY_PIPELINES
  if (pm && strcmp(pm, "fused") == 0) p = 0;
  if (pm && strcmp(pm, "split") == 0) p = 1;
#endif
  if (m->plan.h.nnb > 0 && p != 3) p = 2;  // neighbour equality rows: the rows pipeline (or the tree pipeline when asked for)
  return p;
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
  bool ok = A.zeros(&b->qpos, n * nq) && A.zeros(&b->qvel, n * nv) && A.zeros(&b->warm, n * nv) && A.zeros(&b->act, n * nu) &&
            A.zeros(&b->ctrl, n * nu) && A.zeros(&b->kenv, n) && A.zeros(&b->ctrl_row, nu) && A.zeros(&b->kmask_jnt, njnt) &&
            A.zeros(&b->kmask_ten, nt) && A.zeros(&b->flags, n) && A.zeros(&b->touch, n) && A.zeros(&b->ncon, n) && A.zeros(&b->nefc, n) &&
            A.zeros(&b->iters, n) && A.zeros(&b->secprof, 48);
  if (!ok) return devmem_fail(A.nomem, "sg_batch_create (state)");
  b->kmask_jnt_host.assign(njnt, 0); b->kmask_ten_host.assign(nt, 0);
  b->pipeline = first_pipeline(m);
  if (int rc = b->pipeline == 3 ? tree_alloc(b) : rows_alloc(b)) return rc;
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
  SgRowsBufs& r = b->r;   // (allocated: the batch is on pipeline 1 or 2, sg_batch_create / sg_set_pipeline)
  SgPhaseArgs pa;
  pa.H = r.H; pa.elem = r.elem;
  pa.qpos = b->qpos; pa.qvel = b->qvel; pa.warm = b->warm; pa.act = b->act; pa.ctrl = b->ctrl;
  pa.kenv = b->kenv; pa.kmask_jnt = b->kmask_jnt; pa.kmask_ten = b->kmask_ten;
  pa.mask = mask; pa.sens = nullptr; pa.sens_stride = stride > 0 ? stride : H.nsensordata;
  pa.w = r.w; pa.nenv = b->n; pa.rowlayout = b->pipeline == 2;
  pa.nbtab = r.nbtab; pa.cpos = r.cpos; pa.cst_rounds = r.shape.cst_rounds;
  pa.gpairs = r.gpairs;
  pa.nelem = H.nelem; pa.nv = H.nv; pa.nu = H.nu; pa.elem_dof0 = H.elem_dof0; pa.nchain = H.nchain; pa.t0_id = H.t0_id; pa.timestep = H.timestep;
  SgPgsArgs ga;
  ga.sched = r.sched; ga.nbtab = r.nbtab; ga.tab = r.tab;
  ga.H = r.H; ga.elem = r.elem; ga.w = r.w; ga.nenv = b->n;
#ifdef SG_LEGACY_PIPELINES
  const size_t lds = sizeof(double) * ((size_t)(5 * 8 + 2) * H.nelem + 16 * 4 * SG_MAXLIM + 72);   // (the split pipeline's solver)
#endif
  // rows kernel: joint-fix rows per lane r.nsl (template parameter, the smallest instantiated value >= ceil(nelem / 8)); its LDS
  // arrays are padded to 8 * NSL rows
  const bool nbm = r.shape.nb_mode != 0;
  const int epw = solver_epw(b);
  const size_t lds_rows = sizeof(double) * r.shape.lds_doubles(epw, r.nsl);
  if (!r.attr_set) {  // per device: a batch on another GPU of the same process needs its own call
    HIPCHK(sg_rows_prepare());
#ifdef SG_LEGACY_PIPELINES
    HIPCHK(sg_legacy_prepare());
#endif
    r.attr_set = true;
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
      if (b->pipeline == 2) HIPCHK(sg_launch_rows(ga, r.nsl, r.shape.nb_mode, epw, b->n, lds_rows, s));
#ifdef SG_LEGACY_PIPELINES
      else HIPCHK(sg_launch_pgs_split(ga, b->n, lds, s));
#endif
      if (b->prof) HIPCHK(hipEventRecord(b->ev_pgs.back().second, s));
    }
  }
  if (b->prof) HIPCHK(hipEventRecord(b->ev[call_ev].second, s));
  // outputs of the call: one small kernel for the five per-env int arrays (five device-to-device copies cost 1 % of a step);
  // with a mask (masked reset) only the selected envs' entries may change
  hipLaunchKernelGGL(sg_masked_copy_kernel, dim3((b->n + 255) / 256), dim3(256), 0, s, mask, b->n, r.w.status, flags ? flags : b->flags,
                     r.w.touch, touch ? touch : b->touch, r.w.ncon, b->ncon, r.w.nefc, b->nefc, r.w.iters, b->iters);
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
  a.H = b->r.H; a.elem = b->r.elem;
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
  HIPCHK(hipSetDevice(b->device));
  if (int rc = rows_alloc(b)) return rc;   // (a batch that started on the tree pipeline)
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
    HIPCHK(hipMemcpy2DAsync(out, sizeof(int32_t) * nwords, b->pipeline == 0 ? b->touch : b->r.w.touch, sizeof(int32_t), sizeof(int32_t), b->n,
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
  HIPCHK(hipMemcpy(out32, b->secprof, sizeof(unsigned long long) * 48, hipMemcpyDeviceToHost));
  HIPCHK(hipMemset(b->secprof, 0, sizeof(unsigned long long) * 48));
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

int sg_model_nbody(const sg_model* m) { return m ? m->kin.o.nbody : 0; }
int sg_model_ngeom(const sg_model* m) { return m ? m->kin.o.ngeom : 0; }

}  // extern "C"
