// sg_devmem.h -- the owners of the C ABI's device memory (sg_batch.h).  No HIP include here: hipMalloc, hipFree, hipMemset, hipMemcpy,
// hipStreamSynchronize, hipStream_t and hipSuccess are whatever the including file declares (the host test includes this over counting fakes).
// Every call returns true on success; after a failure `nomem` says whether it was the allocation (else a memset, a copy or the synchronise).
#pragma once
#include <cstddef>
#include <vector>

// a group of buffers that live and die together: freed by release() or the destructor, never one by one
struct SgArena {
  std::vector<void*> bufs;
  bool nomem = false;
  SgArena() = default;
  SgArena(const SgArena&) = delete;
  SgArena& operator=(const SgArena&) = delete;
  ~SgArena() { release(); }
  void release() {
    for (void* p : bufs) (void)hipFree(p);
    bufs.clear();
  }
  // `count` zero-filled elements; count == 0 gives one element, so that every buffer has a pointer of its own
  template <class T>
  bool zeros(T** out, size_t count) {
    const size_t bytes = sizeof(T) * (count ? count : 1);
    void* p = nullptr;
    bufs.reserve(bufs.size() + 1);
    nomem = hipMalloc(&p, bytes) != hipSuccess;
    if (nomem) return false;
    bufs.push_back(p);
    *out = (T*)p;
    return hipMemset(p, 0, bytes) == hipSuccess;
  }
  // the vector's elements, then `spare` zero elements
  template <class T>
  bool upload(T** out, const std::vector<T>& v, size_t spare = 0) {
    return zeros(out, v.size() + spare) && (v.empty() || hipMemcpy(*out, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice) == hipSuccess);
  }
  // publish a group built on the side: `to` owns the buffers from here on
  void give_to(SgArena& to) {
    to.bufs.insert(to.bufs.end(), bufs.begin(), bufs.end());
    bufs.clear();
  }
};

// a per-model table on a batch's device: the device pointers of its sections -- doubles, ints, or both -- all NULL until every section
// is up.  ensure() is the one way up: the sections are uploaded on a side arena and handed to `owner` only when all of them are there, so
// a failure leaves the table and the owner as they were (and a later call may try again); once up, it costs a comparison
struct SgDevTable {
  double* d = nullptr;
  int* i = nullptr;
  bool nomem = false;
  // dbl / ints: the host sections (NULL: the table has no such section)
  bool ensure(SgArena& owner, const std::vector<double>* dbl, const std::vector<int>* ints) {
    if (d || i) return true;
    SgArena side;
    double* pd = nullptr;
    int* pi = nullptr;
    nomem = false;
    if (!((!dbl || side.upload(&pd, *dbl)) && (!ints || side.upload(&pi, *ints)))) {
      nomem = side.nomem;
      return false;
    }
    side.give_to(owner);
    d = pd; i = pi;
    return true;
  }
};

// a buffer that grows on demand and never shrinks; its contents do not survive a growth
template <class T>
struct SgScratch {
  T* p = nullptr;
  size_t cap = 0;   // elements
  bool nomem = false;
  SgScratch() = default;
  SgScratch(const SgScratch&) = delete;
  SgScratch& operator=(const SgScratch&) = delete;
  ~SgScratch() { if (p) (void)hipFree(p); }
  // room for n elements.  Growing waits for the stream first (an earlier launch on it may still read the old block); a failed
  // allocation leaves the buffer empty
  bool reserve(size_t n, hipStream_t s) {
    if (n <= cap) return true;
    nomem = false;
    if (hipStreamSynchronize(s) != hipSuccess) return false;
    if (p) (void)hipFree(p);
    p = nullptr; cap = 0;
    nomem = hipMalloc((void**)&p, sizeof(T) * n) != hipSuccess;
    if (nomem) { p = nullptr; return false; }
    cap = n;
    return true;
  }
};
