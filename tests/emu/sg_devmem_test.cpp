// Host test of soft-grip_amd/csrc/sg_devmem.h (SgArena, SgScratch, SgDevTable) over counting fakes of the five HIP calls it uses: one fixed
// sequence, run once clean and once with each allocation and each copy failing in turn; then a table's ensure(), clean and with each
// section's allocation and copy failing.  Whatever fails, no block may outlive its owner.
// Driven by tests/test_devmem_host.py; prints a line per run, exit status 0 = every check held.
#include <cstdio>
#include <cstdlib>
#include <cstring>

typedef int hipError_t;
typedef void* hipStream_t;
enum { hipSuccess = 0, hipErrorInjected = 1 };
enum hipMemcpyKind { hipMemcpyHostToDevice };

static int g_live, g_allocs, g_copies, g_syncs, g_fail_alloc, g_fail_copy, g_empty_requests;

static hipError_t hipMalloc(void** p, size_t bytes) {
  if (bytes == 0) g_empty_requests++;
  if (++g_allocs == g_fail_alloc) return hipErrorInjected;
  *p = malloc(bytes ? bytes : 1);
  memset(*p, 0xAB, bytes);   // (what a fresh device block may hold: the zeroing must be the header's)
  g_live++;
  return hipSuccess;
}
static hipError_t hipFree(void* p) {
  free(p);
  g_live--;
  return hipSuccess;
}
static hipError_t hipMemset(void* p, int v, size_t bytes) {
  memset(p, v, bytes);
  return hipSuccess;
}
static hipError_t hipMemcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind) {
  if (++g_copies == g_fail_copy) return hipErrorInjected;
  memcpy(dst, src, bytes);
  return hipSuccess;
}
static hipError_t hipStreamSynchronize(hipStream_t) {
  g_syncs++;
  return hipSuccess;
}

#include "../../soft-grip_amd/csrc/sg_devmem.h"

static int g_bad;
#define CHECK(c)                                                                                                      \
  do {                                                                                                                \
    if (!(c)) { printf("  FAILED line %d (fail_alloc %d, fail_copy %d): %s\n", __LINE__, g_fail_alloc, g_fail_copy, #c); g_bad++; } \
  } while (0)

// the sequence makes 8 allocations and 3 copies when nothing fails
enum { N_ALLOCS = 8, N_COPIES = 3 };

static void run(int fail_alloc, int fail_copy) {
  g_live = g_allocs = g_copies = g_syncs = g_empty_requests = 0;
  g_fail_alloc = fail_alloc; g_fail_copy = fail_copy;
  const bool clean = !fail_alloc && !fail_copy;
  {
    SgArena A;
    SgScratch<int> S;
    int *a = nullptr, *b = nullptr;
    double* u = nullptr;
    float* z = nullptr;
    const std::vector<double> src = {1.0, 2.0, 3.0};
    const bool ok = A.zeros(&a, 5) && A.zeros(&b, 3) && A.upload(&u, src, 2) && A.zeros(&z, 0);
    CHECK(ok == !((fail_alloc >= 1 && fail_alloc <= 4) || fail_copy == 1));
    if (!ok) CHECK(A.nomem == (fail_alloc != 0));
    if (ok) {
      for (int i = 0; i < 5; i++) CHECK(a[i] == 0);
      for (int i = 0; i < 3; i++) CHECK(b[i] == 0);
      CHECK(u[0] == 1.0 && u[1] == 2.0 && u[2] == 3.0 && u[3] == 0.0 && u[4] == 0.0);
      CHECK(z != nullptr && z != (float*)u && *z == 0.0f);   // a zero-count buffer has a pointer of its own
      CHECK(A.bufs.size() == 4);
      // a group built on the side and handed over only when complete
      const size_t before = A.bufs.size();
      SgArena side;
      int* p = nullptr;
      double* q = nullptr;
      const std::vector<int> ids = {4, 5};
      if (side.upload(&p, ids) && side.upload(&q, src)) {
        side.give_to(A);
        CHECK(side.bufs.empty() && A.bufs.size() == before + 2);
        CHECK(p[0] == 4 && p[1] == 5 && q[2] == 3.0);
      } else {
        CHECK(fail_alloc == 5 || fail_alloc == 6 || fail_copy == 2 || fail_copy == 3);
        CHECK(side.nomem == (fail_alloc != 0));
        CHECK(A.bufs.size() == before);   // the target is as it was
      }
    }
    // grow, grow, reuse
    const int syncs0 = g_syncs;
    if (!S.reserve(1, nullptr)) CHECK(S.nomem && S.p == nullptr && S.cap == 0);
    else CHECK(S.p != nullptr && S.cap == 1);
    if (!S.reserve(3, nullptr)) CHECK(S.nomem && S.p == nullptr && S.cap == 0);
    else CHECK(S.p != nullptr && S.cap == 3);
    CHECK(g_syncs == syncs0 + 2);   // one wait per growth, before the old block goes
    const int allocs0 = g_allocs;
    int* const p3 = S.p;
    const size_t cap3 = S.cap;
    if (cap3 >= 2) {
      CHECK(S.reserve(2, nullptr) && g_allocs == allocs0 && g_syncs == syncs0 + 2 && S.p == p3 && S.cap == cap3);   // no allocation, no wait
    } else {
      CHECK(S.reserve(2, nullptr) && S.cap == 2);   // (the growth before it failed: this one allocates)
    }
    CHECK(g_live > 0);
  }
  CHECK(g_live == 0);
  CHECK(g_empty_requests == 0);
  if (clean) CHECK(g_allocs == N_ALLOCS && g_copies == N_COPIES);
  if (fail_alloc) CHECK(g_allocs >= fail_alloc);   // the failure was reached
  if (fail_copy) CHECK(g_copies >= fail_copy);
  printf("run fail_alloc=%d fail_copy=%d live=%d\n", fail_alloc, fail_copy, g_live);
}

// SgDevTable::ensure over the same fakes.  fail_alloc / fail_copy: the allocation / copy of the FIRST ensure that fails (0: none)
static void run_table(int fail_alloc, int fail_copy) {
  g_live = g_allocs = g_copies = g_syncs = g_empty_requests = 0;
  g_fail_alloc = fail_alloc; g_fail_copy = fail_copy;
  {
    SgArena owner;
    int* keep = nullptr;
    CHECK(owner.zeros(&keep, 2));   // (what the batch holds already: allocation 1)
    const std::vector<double> dbl = {1.5, 2.5, 3.5};
    const std::vector<int> ints = {7, 8};
    SgDevTable T;
    const int allocs0 = g_allocs;
    const bool ok = T.ensure(owner, &dbl, &ints);
    CHECK(ok == (!fail_alloc && !fail_copy));
    if (!ok) {   // the first section is freed, every pointer stays NULL, the owner is as it was
      CHECK(T.d == nullptr && T.i == nullptr);
      CHECK(T.nomem == (fail_alloc != 0));
      CHECK(owner.bufs.size() == 1 && g_live == 1);
      g_fail_alloc = g_fail_copy = 0;
      const int allocs1 = g_allocs;
      CHECK(T.ensure(owner, &dbl, &ints) && !T.nomem);   // a later ensure succeeds
      CHECK(g_allocs == allocs1 + 2);
    } else {
      CHECK(g_allocs == allocs0 + 2);   // one allocation per section
    }
    CHECK(T.d && T.i && T.d[0] == 1.5 && T.d[2] == 3.5 && T.i[0] == 7 && T.i[1] == 8);
    CHECK(owner.bufs.size() == 3 && g_live == 3);   // the owner holds them
    const int allocs2 = g_allocs, copies2 = g_copies;
    double* const d = T.d;
    CHECK(T.ensure(owner, &dbl, &ints) && g_allocs == allocs2 && g_copies == copies2 && T.d == d);   // a second ensure allocates nothing
    // a table of one section: the other pointer stays NULL, and the table counts as up
    SgDevTable one;
    CHECK(one.ensure(owner, nullptr, &ints) && one.d == nullptr && one.i && one.i[1] == 8 && owner.bufs.size() == 4);
    const int allocs3 = g_allocs;
    CHECK(one.ensure(owner, nullptr, &ints) && g_allocs == allocs3);
  }
  CHECK(g_live == 0);
  CHECK(g_empty_requests == 0);
  printf("table fail_alloc=%d fail_copy=%d live=%d\n", fail_alloc, fail_copy, g_live);
}

int main() {
  run(0, 0);
  for (int k = 1; k <= N_ALLOCS; k++) run(k, 0);
  for (int k = 1; k <= N_COPIES; k++) run(0, k);
  run_table(0, 0);
  run_table(2, 0);   // the first section's allocation (allocation 1 is the owner's own block)
  run_table(3, 0);   // the second section's allocation
  run_table(0, 1);   // the first section's copy
  run_table(0, 2);   // the second section's copy
  printf(g_bad ? "FAIL\n" : "PASS\n");
  return g_bad ? 1 : 0;
}
