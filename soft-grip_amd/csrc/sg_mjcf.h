// sg_mjcf.h -- native MJCF subset compiler (sg_mjcf.cpp): XML file -> model blob
#pragma once
#include <string>

// Compiles the scene at xml_path (includes resolved relative to its directory) into the tagged-array container of
// include/softgrip_model.h.  Returns false and sets *err for files outside the supported MJCF subset.
// what the compiler read off the first <composite> that has a <skin> child (sg_skin.h builds the skin from it and the body names):
// inflate and rgba are read, material / texcoord / subgrid accepted and ignored
struct SgSkinSpec {
  bool present = false;
  std::string prefix;
  double inflate = 0.0;
  float rgba[4] = {0.8f, 0.2f, 0.1f, 1.0f};   // the renderer's element albedo
};

bool sg_mjcf_compile_file(const char* xml_path, bool composite_neighbors, bool implicit_tendon_damping, std::string* blob, std::string* err,
                          SgSkinSpec* skin = nullptr);
