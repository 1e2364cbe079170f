// Driver of the step cache's CPU launch-trace test (tests/test_step_cache_cpu.py): tfx_step_desc values over fake device addresses, run
// through tfx_dit_step_run as a whole step (phase 0) and as the three phases of the step cache; the launch layer behind them is
// launch_recorder.cpp + step_cache_recorder.cpp.  Per scenario: a header line, the recorded launches, the return code and the error
// text.  The model of dit_trace_driver.cpp: 2 double + 2 single blocks, batch 2, D = 128 * H.
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>

#include "textflux_hip.h"

namespace tfx {
extern int g_probe_mask;
void* sc_region(const char* name);
void sc_reset();
}  // namespace tfx

namespace {

constexpr int ROWSPLIT = 1, QKN = 2, FP8_QKN = 4;

template <class T = void>
T* region(const std::string& name) { return (T*)tfx::sc_region(name.c_str()); }

struct Cfg { const char* name; int T; int mask; bool fp8; };

struct Model {
  tfx_step_desc s;
  tfx_step_cache c;
  tfx_double_block dbl[2];
  tfx_single_block sgl[2];
  tfx_dit_desc& d() { return s.dit; }
};

void linear(tfx_linear& l, const std::string& name, bool w8) {
  l.w = region(name + ".w");
  l.b = region(name + ".b");
  if (w8) { l.w8 = region(name + ".w8"); l.w8_scale = region<float>(name + ".w8s"); }
}

void build(Model& m, const Cfg& c, int sampler) {
  tfx::sc_reset();
  std::memset(&m, 0, sizeof m);
  tfx_dit_desc& d = m.d();
  const int H = 2, D = 128 * H, S = 256;
  d.D = D; d.H = H; d.in_channels = 64; d.out_channels = 16; d.n_double = 2; d.n_single = 2;
  d.B = 2; d.S = S; d.T = c.T;
  linear(d.x_embedder, "x_embedder", false);
  linear(d.proj_out, "proj_out", false);
  for (int i = 0; i < 2; ++i) {
    tfx_double_block& w = m.dbl[i];
    const std::string n = "d" + std::to_string(i) + ".";
    linear(w.qkv_img, n + "qkv_img", c.fp8); linear(w.qkv_txt, n + "qkv_txt", c.fp8);
    linear(w.out_img, n + "out_img", c.fp8); linear(w.out_txt, n + "out_txt", c.fp8);
    linear(w.ff1_img, n + "ff1_img", c.fp8); linear(w.ff2_img, n + "ff2_img", c.fp8);
    linear(w.ff1_txt, n + "ff1_txt", c.fp8); linear(w.ff2_txt, n + "ff2_txt", c.fp8);
    w.norm_q = region(n + "norm_q"); w.norm_k = region(n + "norm_k");
    w.norm_added_q = region(n + "norm_added_q"); w.norm_added_k = region(n + "norm_added_k");
    w.attn_score_bound = 3.5f + i;
  }
  for (int j = 0; j < 2; ++j) {
    tfx_single_block& w = m.sgl[j];
    const std::string n = "s" + std::to_string(j) + ".";
    linear(w.qkv_mlp, n + "qkv_mlp", c.fp8); linear(w.proj_out, n + "proj_out", c.fp8);
    w.norm_q = region(n + "norm_q"); w.norm_k = region(n + "norm_k");
    w.attn_score_bound = 5.5f + j;
  }
  d.dbl = m.dbl; d.sgl = m.sgl;
  d.xin = region("xin"); d.ctx0 = region("ctx0");
  const int mod_len = 2 * 12 * D + 2 * 3 * D + 2 * D;
  d.mod = region("mod"); d.mod_bstride = mod_len + d.out_channels;
  d.cos_tab = region<float>("cos"); d.sin_tab = region<float>("sin");
  d.hid = region("hid"); d.xn = region("xn"); d.y = region("y"); d.out = region("out");
  d.first_block = 0; d.last_block = -1; d.flags = c.fp8 ? 4 : 0;
  d.q8 = region("q8"); d.q8_scale = region<float>("q8s");
  d.gemm_workspace = region("ws"); d.gemm_workspace_bytes = 128ll << 20;
  d.rope_cs = region<float>("rope_cs");
  m.s.mod_table = region("mod_table"); m.s.mod_cur = const_cast<void*>(d.mod); m.s.mod_step_elems = d.B * d.mod_bstride;
  m.s.step_ptr = region<int32_t>("step_ptr"); m.s.latents = region("latents");
  m.s.coef = region<float>("coef"); m.s.noise = region<float>("noise"); m.s.sampler = sampler;
  if (sampler == 2) { d.euler_gate = (const char*)d.mod + (d.mod_bstride - d.out_channels) * 2; d.euler_gate_bstride = d.mod_bstride; }
  m.c.x0 = region("x0"); m.c.f_prev = region("f_prev"); m.c.h1 = region("h1"); m.c.r = region("r");
  m.c.ld = D; m.c.bstride = (int64_t)S * D;
  m.c.partials = region<float>("partials"); m.c.partials_bytes = 2048 * d.B; m.c.metric = region<float>("metric");
  m.s.cache = &m.c;
}

using Tweak = std::function<void(Model&)>;

void scenario(const std::string& name, const Cfg& c, int sampler, int phase, const Tweak& tweak = nullptr) {
  static Model m;
  build(m, c, sampler);
  m.s.phase = phase;
  if (tweak) tweak(m);
  tfx::g_probe_mask = c.mask;
  std::printf("== %s\n", name.c_str());
  const int rc = tfx_dit_step_run(&m.s, nullptr);
  std::printf("rc %d\nerror %s\n", rc, rc ? tfx_last_error() : "");
  std::fflush(stdout);
}

}  // namespace

int main() {
  const int ALL = ROWSPLIT | QKN | FP8_QKN;
  const Cfg cfgs[3] = {{"bf16_joint", 256, ALL, false}, {"bf16_separate", 100, QKN | FP8_QKN, false}, {"fp8", 256, ALL, true}};
  for (const Cfg& c : cfgs)
    for (int sampler = 0; sampler < 3; ++sampler) {
      const std::string base = std::string(c.name) + "_sampler" + std::to_string(sampler);
      scenario(base + "_whole", c, sampler, 0, [](Model& m) { m.s.cache = nullptr; });
      for (int phase = 1; phase <= 3; ++phase) scenario(base + "_phase" + std::to_string(phase), c, sampler, phase);
    }
  // a cache next to phase 0 changes nothing
  scenario("whole_with_cache", cfgs[0], 2, 0);

  // ---- refusals
  const Cfg& j = cfgs[0];
  scenario("fail_phase_without_cache", j, 0, 1, [](Model& m) { m.s.cache = nullptr; });
  scenario("fail_phase_4", j, 0, 4);
  scenario("fail_phase_negative", j, 0, -1);
  scenario("fail_seq_len", j, 2, 1, [](Model& m) { m.d().seq_len = region<int32_t>("seq_len"); m.d().rope_bstride = 512; });
  scenario("fail_first_block", j, 0, 2, [](Model& m) { m.d().first_block = 1; });
  scenario("fail_last_block", j, 0, 2, [](Model& m) { m.d().last_block = 3; });
  scenario("fail_flags_1", j, 0, 1, [](Model& m) { m.d().flags = 1; });
  scenario("fail_flags_2_phase_0", j, 0, 0, [](Model& m) { m.d().flags = 2; });
  scenario("fail_one_block", j, 0, 1, [](Model& m) { m.d().n_double = 1; m.d().n_single = 0; });
  scenario("fail_null_x0", j, 0, 1, [](Model& m) { m.c.x0 = nullptr; });
  scenario("fail_null_metric", j, 0, 3, [](Model& m) { m.c.metric = nullptr; });
  scenario("fail_partials_small", j, 0, 1, [](Model& m) { m.c.partials_bytes = 8; });
  scenario("fail_cache_ld", j, 0, 1, [](Model& m) { m.c.ld = 128; });
  return 0;
}
