// Recording stand-in for the launcher true CFG adds (csrc/launch.h: cfg_combine), linked next to launch_recorder.cpp,
// step_cache_recorder.cpp and change_map_recorder.cpp by tests/test_true_cfg_cpu.py: one line per launch with every argument, pointers
// as `name+0xoff` of the regions the driver registered through cfg_region.
#include <cstdio>
#include <string>
#include <vector>

#include "launch.h"

namespace tfx {

void* cm_region(const char* name);   // change_map_recorder.cpp
void cm_reset();

static std::vector<std::string> g_cfg_names;
void* cfg_region(const char* name) {
  g_cfg_names.push_back(name);
  return cm_region(name);
}
void cfg_reset() {
  g_cfg_names.clear();
  cm_reset();
}

namespace {
std::string sym(const void* p) {
  const uint64_t v = (uint64_t)p, k = v >> 32, off = v & 0xffffffffull;
  char b[64];
  if (!p) return "0";
  if (k == 0 || k > g_cfg_names.size()) { snprintf(b, sizeof b, "?%#llx", (unsigned long long)v); return b; }
  if (!off) return g_cfg_names[k - 1];
  snprintf(b, sizeof b, "+%#llx", (unsigned long long)off);
  return g_cfg_names[k - 1] + b;
}
}  // namespace

int cfg_combine(const void* v_neg, const void* v_pos, void* out, int C, int64_t rows, const float* scale, hipStream_t) {
  std::printf("cfg_combine v_neg=%s v_pos=%s out=%s C=%d rows=%lld scale=%s\n", sym(v_neg).c_str(), sym(v_pos).c_str(), sym(out).c_str(), C,
              (long long)rows, sym(scale).c_str());
  return 0;
}

}  // namespace tfx
