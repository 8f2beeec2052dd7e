// sg_plan_dump.cpp -- digests of the kernel plans both builders make of a model (tests/test_plan_digest.py holds them against
// tests/golden/plan_digests.json, so an edit of csrc/sg_plan.cpp cannot change a plan unnoticed).
//   usage: sg_plan_dump FILE...    FILE = a model blob, or an .xml scene (compiled by sg_mjcf_compile_file in both composite variants)
//          sg_plan_dump --table    the blob's schema (csrc/sg_blob.h SG_MODEL_ARRAYS), one array per line in the container's order:
//                                  name, f64 | i32, items per entry, dimension, required | optional (only blobs with a free joint carry it)
// Per input and builder one line: `refused: <message>`, or an FNV-1a hash (64 bits) over the raw bytes of each part of the plan and the
// parts' element counts.  Every part is zero-initialised before the builder fills it, so the bytes are deterministic.  Per compiled .xml
// and variant one more line, `<label> blob: <hash of the blob's bytes>/<byte count>`: what the MJCF compiler wrote is pinned too.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>

#include "../../soft-grip_amd/csrc/sg_blob.h"
#include "../../soft-grip_amd/csrc/sg_mjcf.h"
#include "../../soft-grip_amd/csrc/sg_plan.h"

static uint64_t fnv1a(const void* p, size_t n) {
  uint64_t h = 0xcbf29ce484222325ull;
  for (size_t i = 0; i < n; i++) h = (h ^ ((const unsigned char*)p)[i]) * 0x100000001b3ull;
  return h;
}
template <class V>
static void part(const char* name, const V& v) {
  printf(" %s=%016llx/%zu", name, (unsigned long long)fnv1a(v.data(), v.size() * sizeof(v[0])), v.size());
}

static void dump(const std::string& label, const std::string& blob) {
  for (int tree = 0; tree < 2; tree++) {
    SgPlan P;
    SgTreeDev T;
    memset(&T, 0, sizeof T);
    std::string err;
    const bool ok = tree ? sg_tree_plan_build(blob.data(), blob.size(), &P, &T, &err) : sg_plan_build(blob.data(), blob.size(), &P, &err);
    printf("%s %s:", label.c_str(), tree ? "tree" : "two");
    if (!ok) {
      printf(" refused: %s\n", err.c_str());
      continue;
    }
    printf(" header=%016llx", (unsigned long long)fnv1a(&P.h, sizeof P.h));
    part("elem", P.elem); part("elem_geom", P.elem_geom); part("elem_dofmap", P.elem_dofmap); part("nbtab", P.nbtab);
    part("sched", P.sched); part("gpairs", P.gpairs);
    if (tree) printf(" treedev=%016llx", (unsigned long long)fnv1a(&T, sizeof T));
    printf("\n");
  }
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "--table")) {
#define SG_X(type, name, per, dim, part) printf("%s %s %d %s required\n", #name, sizeof(type) == 8 ? "f64" : "i32", per, #dim);
#define SG_W(type, name, per, dim, free_only) printf("%s %s %d %s %s\n", #name, sizeof(type) == 8 ? "f64" : "i32", per, #dim, free_only ? "optional" : "required");
    SG_MODEL_ARRAYS(SG_X, SG_W)
    return 0;
  }
  for (int i = 1; i < argc; i++) {
    const std::string path = argv[i], base = path.substr(path.find_last_of('/') + 1);
    if (path.size() > 4 && path.compare(path.size() - 4, 4, ".xml") == 0) {
      for (int nb = 0; nb < 2; nb++) {
        std::string blob, err;
        const std::string label = base + " nb=" + std::to_string(nb);
        if (!sg_mjcf_compile_file(path.c_str(), nb != 0, false, &blob, &err)) { printf("%s compile error: %s\n", label.c_str(), err.c_str()); continue; }
        printf("%s blob: %016llx/%zu\n", label.c_str(), (unsigned long long)fnv1a(blob.data(), blob.size()), blob.size());
        dump(label, blob);
      }
    } else {
      std::ifstream f(path, std::ios::binary);
      if (!f) { printf("%s cannot be read\n", base.c_str()); return 1; }
      dump(base, std::string(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>()));
    }
  }
  return 0;
}
