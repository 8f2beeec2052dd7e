// Host program of scripts/sanitize/run.sh (ASan + UBSan, CPU only).
//   host_main FILE.xml ...            compiles each scene in both composite variants and builds both plans (two-finger and tree)
//   host_main --mutate FILE.sgmodel.. feeds both plan builders, and then the read-out tables' builders (sg_tables_build of csrc/sg_tables.cpp),
//                                     damaged copies of each blob: both plan builders must refuse every one with a message, every
//                                     table builder must answer with ok or a message, and none may make a reader leave its buffer
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <string>
#include <vector>
#include "../../soft-grip_amd/csrc/sg_blob.h"
#include "../../soft-grip_amd/csrc/sg_mjcf.h"
#include "../../soft-grip_amd/csrc/sg_readout_host.h"

static bool build_both(const void* blob, size_t n, std::string msg[2]) {
  SgPlan P, PT;
  auto tree = std::make_unique<SgTreeDev>();
  const bool a = sg_plan_build(blob, n, &P, &msg[0]), b = sg_tree_plan_build(blob, n, &PT, tree.get(), &msg[1]);
  return a || b;
}

// every table, on the plans as sg_model_create builds them (planned) or on a plan that names no geom -> the first table that has neither
// ok nor a message, or NULL
static const char* build_tables(const void* blob, size_t n, bool planned) {
  SgHostTables T{};
  bool fast, tree;
  if (planned) sg_host_tables_planned(blob, n, &T, &fast, &tree);
  else sg_host_tables(blob, n, &T);
  auto silent = [](const auto& t) { return !t.ok && t.err.empty(); };
  return silent(T.kin) ? "kin" : silent(T.con) ? "con" : silent(T.dyn) ? "dyn" : silent(T.smooth) ? "smooth" : silent(T.point) ? "point" : silent(T.solve) ? "solve"
       : silent(T.forces) ? "forces" : nullptr;
}

static int n_mut = 0, n_bad = 0;

// one damaged copy, in a heap block of exactly its size (so that a read past it is a report)
static void mutant(const char* what, long long at, const std::string& bytes) {
  std::unique_ptr<char[]> buf(new char[bytes.size() ? bytes.size() : 1]);
  memcpy(buf.get(), bytes.data(), bytes.size());
  std::string msg[2];
  n_mut++;
  if (build_both(buf.get(), bytes.size(), msg) || msg[0].empty() || msg[1].empty()) {
    printf("ACCEPTED: %s at %lld (%zu bytes): '%s' / '%s'\n", what, at, bytes.size(), msg[0].c_str(), msg[1].c_str());
    n_bad++;
  }
  if (const char* silent = build_tables(buf.get(), bytes.size(), false)) {
    printf("SILENT: %s at %lld (%zu bytes): the %s table has neither ok nor a message\n", what, at, bytes.size(), silent);
    n_bad++;
  }
}

static int mutate(const char* path) {
  std::ifstream f(path, std::ios::binary);
  const std::string blob((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  std::string msg[2];
  if (!build_both(blob.data(), blob.size(), msg)) { printf("%s: no builder takes the intact blob: %s / %s\n", path, msg[0].c_str(), msg[1].c_str()); return 1; }
  if (const char* silent = build_tables(blob.data(), blob.size(), true)) {   // the intact blob's tables, on the plans sg_model_create would use
    printf("%s: the %s table of the intact blob has neither ok nor a message\n", path, silent);
    return 1;
  }
  sg_blob_header hd;
  memcpy(&hd, blob.data(), sizeof hd);
  std::vector<size_t> rec_at;   // the records' offsets, then the end
  size_t off = sizeof hd;
  for (uint32_t r = 0; r < hd.nrec; r++) {
    sg_blob_record rec;
    memcpy(&rec, blob.data() + off, sizeof rec);
    rec_at.push_back(off);
    size_t nb = (size_t)rec.count * (rec.dtype == SG_DT_F64 ? 8 : rec.dtype == SG_DT_I32 ? 4 : 1);
    off += sizeof rec + nb + (8 - nb % 8) % 8;
  }
  rec_at.push_back(off);
  const int before = n_mut;
  auto patched = [&](std::string s, size_t at, const void* v, size_t n) { memcpy(&s[at], v, n); return s; };
  // cut at every record boundary and a byte to either side: as it is, and with total_bytes saying the cut is the whole blob
  for (size_t b : rec_at)
    for (int d = -1; d <= 1; d++) {
      const size_t L = b + d;
      if (L >= blob.size()) continue;
      const int64_t tb = (int64_t)L;
      mutant("cut", (long long)L, blob.substr(0, L));
      if (L >= sizeof hd) mutant("cut, total_bytes to match", (long long)L, patched(blob.substr(0, L), offsetof(sg_blob_header, total_bytes), &tb, 8));
    }
  for (uint32_t nrec : {hd.nrec + 1, hd.nrec + 1000, 0xFFFFFFFFu}) mutant("nrec raised", nrec, patched(blob, offsetof(sg_blob_header, nrec), &nrec, 4));
  for (int64_t d : {-1, 1}) {
    const int64_t tb = hd.total_bytes + d;
    mutant("total_bytes off by one", d, patched(blob, offsetof(sg_blob_header, total_bytes), &tb, 8));
  }
  for (size_t r = 0; r + 1 < rec_at.size(); r++) {
    sg_blob_record rec;
    memcpy(&rec, blob.data() + rec_at[r], sizeof rec);
    const int64_t es = rec.dtype == SG_DT_F64 ? 8 : rec.dtype == SG_DT_I32 ? 4 : 1;
    const int64_t left = (int64_t)(blob.size() - rec_at[r] - sizeof rec);
    for (int64_t c : {left / es + 1, (int64_t)1 << 61, INT64_MAX, (int64_t)-1})   // just past the end; products that wrap; negative
      mutant("count raised", (long long)r, patched(blob, rec_at[r] + offsetof(sg_blob_record, count), &c, 8));
  }
  printf("%s: %d damaged copies\n", path, n_mut - before);
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && std::string(argv[1]) == "--mutate") {
    for (int i = 2; i < argc; i++)
      if (mutate(argv[i])) return 1;
    printf("mutation mode: %d damaged copies, %d accepted\n", n_mut, n_bad);
    return n_bad || !n_mut ? 1 : 0;
  }
  for (int i = 1; i < argc; i++) {
    for (int nb = 0; nb < 2; nb++) {
      std::string blob, err;
      bool ok = sg_mjcf_compile_file(argv[i], nb, false, &blob, &err);
      if (!ok) { printf("%s: compile error: %s\n", argv[i], err.c_str()); continue; }
      std::string msg[2];
      build_both(blob.data(), blob.size(), msg);
      printf("%s nb=%d: blob %zu bytes, plan %s %s, tree plan %s %s\n", argv[i], nb, blob.size(), msg[0].empty() ? "ok" : "refused:", msg[0].c_str(),
             msg[1].empty() ? "ok" : "refused:", msg[1].c_str());
    }
  }
  return 0;
}
