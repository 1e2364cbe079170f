// Recording stand-ins for the launchers the blends and the multistep sampler add (csrc/launch.h: known_region_blend, change_map_blend,
// multistep_step), linked next to launch_recorder.cpp and step_cache_recorder.cpp by tests/test_change_map_cpu.py: one line per launch
// with every argument, pointers as `name+0xoff` of the regions the driver registered through cm_region.
#include <cstdio>
#include <string>
#include <vector>

#include "launch.h"

namespace tfx {

void* sc_region(const char* name);   // step_cache_recorder.cpp
void sc_reset();

static std::vector<std::string> g_cm_names;
void* cm_region(const char* name) {
  g_cm_names.push_back(name);
  return sc_region(name);
}
void cm_reset() {
  g_cm_names.clear();
  sc_reset();
}

namespace {
std::string sym(const void* p) {
  const uint64_t v = (uint64_t)p, k = v >> 32, off = v & 0xffffffffull;
  char b[64];
  if (!p) return "0";
  if (k == 0 || k > g_cm_names.size()) { snprintf(b, sizeof b, "?%#llx", (unsigned long long)v); return b; }
  if (!off) return g_cm_names[k - 1];
  snprintf(b, sizeof b, "+%#llx", (unsigned long long)off);
  return g_cm_names[k - 1] + b;
}
}  // namespace

int known_region_blend(void* x, int64_t ldx, const void* x0, const void* noise, const void* mask, int C, int64_t rows,
                       const float* keep_sigma, const int* step_ptr, int step, void* xin, int64_t ldxin, hipStream_t) {
  std::printf("known_region_blend x=%s ldx=%lld x0=%s noise=%s mask=%s C=%d rows=%lld sigma=%s step_ptr=%s step=%d xin=%s ldxin=%lld\n",
              sym(x).c_str(), (long long)ldx, sym(x0).c_str(), sym(noise).c_str(), sym(mask).c_str(), C, (long long)rows,
              sym(keep_sigma).c_str(), sym(step_ptr).c_str(), step, sym(xin).c_str(), (long long)ldxin);
  return 0;
}

int change_map_blend(void* x, int64_t ldx, const void* x0, const void* noise, const void* hold, const int* cut, int C, int64_t rows,
                     const float* keep_sigma, const int* step_ptr, int step, void* xin, int64_t ldxin, hipStream_t) {
  std::printf("change_map_blend x=%s ldx=%lld x0=%s noise=%s hold=%s cut=%s C=%d rows=%lld sigma=%s step_ptr=%s step=%d xin=%s ldxin=%lld\n",
              sym(x).c_str(), (long long)ldx, sym(x0).c_str(), sym(noise).c_str(), sym(hold).c_str(), sym(cut).c_str(), C, (long long)rows,
              sym(keep_sigma).c_str(), sym(step_ptr).c_str(), step, sym(xin).c_str(), (long long)ldxin);
  return 0;
}

int multistep_step(const void* v, void* x, void* xin, int64_t ldxin, int C, int64_t rows, const float* coef, const int* step_ptr, int step,
                   void* v_prev, hipStream_t) {
  std::printf("multistep_step v=%s x=%s xin=%s ldxin=%lld C=%d rows=%lld coef=%s step_ptr=%s step=%d v_prev=%s\n", sym(v).c_str(),
              sym(x).c_str(), sym(xin).c_str(), (long long)ldxin, C, (long long)rows, sym(coef).c_str(), sym(step_ptr).c_str(), step,
              sym(v_prev).c_str());
  return 0;
}

}  // namespace tfx
