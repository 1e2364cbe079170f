// Recording stand-ins for the step cache's launchers (csrc/launch.h: step_cache_save / _metric / _store / _apply), linked next to
// launch_recorder.cpp by tests/test_step_cache_cpu.py: one line per launch with every argument.  Pointers print as `name+0xoff` of the
// regions the driver registered through sc_region (which keeps the names in step with launch_recorder.cpp's own table).
#include <cstdio>
#include <string>
#include <vector>

#include "launch.h"

namespace tfx {

void* trace_region(const char* name);   // launch_recorder.cpp
void trace_reset();

static std::vector<std::string> g_sc_names;
void* sc_region(const char* name) {
  g_sc_names.push_back(name);
  return trace_region(name);
}
void sc_reset() {
  g_sc_names.clear();
  trace_reset();
}

namespace {
std::string sym(const void* p) {
  const uint64_t v = (uint64_t)p, k = v >> 32, off = v & 0xffffffffull;
  char b[64];
  if (!p) return "0";
  if (k == 0 || k > g_sc_names.size()) { snprintf(b, sizeof b, "?%#llx", (unsigned long long)v); return b; }
  if (!off) return g_sc_names[k - 1];
  snprintf(b, sizeof b, "+%#llx", (unsigned long long)off);
  return g_sc_names[k - 1] + b;
}
int record(const char* what, const StepCacheArgs& a) {
  std::printf("%s hid=%s ldh=%lld hbs=%lld x0=%s f_prev=%s h1=%s r=%s ld=%lld bs=%lld partials=%s metric=%s rows=%d batch=%d D=%d\n", what,
              sym(a.hid).c_str(), (long long)a.ldh, (long long)a.hbs, sym(a.x0).c_str(), sym(a.f_prev).c_str(), sym(a.h1).c_str(),
              sym(a.r).c_str(), (long long)a.ld, (long long)a.bs, sym(a.partials).c_str(), sym(a.metric).c_str(), a.rows, a.batch, a.D);
  return 0;
}
}  // namespace

int step_cache_save(const StepCacheArgs& a, hipStream_t) { return record("step_cache_save", a); }
int step_cache_metric(const StepCacheArgs& a, hipStream_t) { return record("step_cache_metric", a); }
int step_cache_store(const StepCacheArgs& a, hipStream_t) { return record("step_cache_store", a); }
int step_cache_apply(const StepCacheArgs& a, hipStream_t) { return record("step_cache_apply", a); }

}  // namespace tfx
