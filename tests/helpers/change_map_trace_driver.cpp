// Driver of change-map sampling's CPU launch-trace test (tests/test_change_map_cpu.py): the step descriptors of
// step_cache_trace_driver.cpp (2 double + 2 single blocks, batch 2, bf16, joint attention) over fake device addresses, run three ways
// per sampler and phase -- tfx_dit_step_run_ex without a blend, with the known-region blend, and tfx_dit_step_run_ex2 with the
// change-map blend -- against launch_recorder.cpp + step_cache_recorder.cpp + change_map_recorder.cpp; then the same step through
// every entry point that must issue it (the `entry_*` scenarios).  Per scenario: a header line, the recorded launches, the return code
// and the error text.
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>

#include "textflux_hip.h"

namespace tfx {
extern int g_probe_mask;
void* cm_region(const char* name);
void cm_reset();
}  // namespace tfx

namespace {

template <class T = void>
T* region(const std::string& name) { return (T*)tfx::cm_region(name.c_str()); }

struct Model {
  tfx_step_desc s;
  tfx_step_cache c;
  tfx_double_block dbl[2];
  tfx_single_block sgl[2];
  tfx_step_extra ex;
  tfx_step_change ch;
  tfx_dit_desc& d() { return s.dit; }
};

void linear(tfx_linear& l, const std::string& name) {
  l.w = region(name + ".w");
  l.b = region(name + ".b");
}

// sampler 0 Euler, 1 AMO, 2 fused Euler, 3 multistep (sampler 0's descriptor and the history buffer)
void build(Model& m, int sampler) {
  tfx::cm_reset();
  std::memset(&m, 0, sizeof m);
  tfx_dit_desc& d = m.d();
  const int H = 2, D = 128 * H, S = 256;
  d.D = D; d.H = H; d.in_channels = 64; d.out_channels = 16; d.n_double = 2; d.n_single = 2;
  d.B = 2; d.S = S; d.T = 256;
  linear(d.x_embedder, "x_embedder");
  linear(d.proj_out, "proj_out");
  for (int i = 0; i < 2; ++i) {
    tfx_double_block& w = m.dbl[i];
    const std::string n = "d" + std::to_string(i) + ".";
    linear(w.qkv_img, n + "qkv_img"); linear(w.qkv_txt, n + "qkv_txt");
    linear(w.out_img, n + "out_img"); linear(w.out_txt, n + "out_txt");
    linear(w.ff1_img, n + "ff1_img"); linear(w.ff2_img, n + "ff2_img");
    linear(w.ff1_txt, n + "ff1_txt"); linear(w.ff2_txt, n + "ff2_txt");
    w.norm_q = region(n + "norm_q"); w.norm_k = region(n + "norm_k");
    w.norm_added_q = region(n + "norm_added_q"); w.norm_added_k = region(n + "norm_added_k");
    w.attn_score_bound = 3.5f + i;
  }
  for (int j = 0; j < 2; ++j) {
    tfx_single_block& w = m.sgl[j];
    const std::string n = "s" + std::to_string(j) + ".";
    linear(w.qkv_mlp, n + "qkv_mlp"); linear(w.proj_out, n + "proj_out");
    w.norm_q = region(n + "norm_q"); w.norm_k = region(n + "norm_k");
    w.attn_score_bound = 5.5f + j;
  }
  d.dbl = m.dbl; d.sgl = m.sgl;
  d.xin = region("xin"); d.ctx0 = region("ctx0");
  const int mod_len = 2 * 12 * D + 2 * 3 * D + 2 * D;
  d.mod = region("mod"); d.mod_bstride = mod_len + d.out_channels;
  d.cos_tab = region<float>("cos"); d.sin_tab = region<float>("sin");
  d.hid = region("hid"); d.xn = region("xn"); d.y = region("y"); d.out = region("out");
  d.first_block = 0; d.last_block = -1; d.flags = 0;
  d.q8 = region("q8"); d.q8_scale = region<float>("q8s");
  d.gemm_workspace = region("ws"); d.gemm_workspace_bytes = 128ll << 20;
  d.rope_cs = region<float>("rope_cs");
  m.s.mod_table = region("mod_table"); m.s.mod_cur = const_cast<void*>(d.mod); m.s.mod_step_elems = d.B * d.mod_bstride;
  m.s.step_ptr = region<int32_t>("step_ptr"); m.s.latents = region("latents");
  m.s.coef = region<float>("coef"); m.s.noise = region<float>("noise"); m.s.sampler = sampler == 3 ? 0 : sampler;
  if (sampler == 2) { d.euler_gate = (const char*)d.mod + (d.mod_bstride - d.out_channels) * 2; d.euler_gate_bstride = d.mod_bstride; }
  m.c.x0 = region("x0"); m.c.f_prev = region("f_prev"); m.c.h1 = region("h1"); m.c.r = region("r");
  m.c.ld = D; m.c.bstride = (int64_t)S * D;
  m.c.partials = region<float>("partials"); m.c.partials_bytes = 2048 * d.B; m.c.metric = region<float>("metric");
  m.s.cache = &m.c;
  if (sampler == 3) m.ex.v_prev = region("v_prev");
  // the blends' buffers: registered in every scenario, so that the regions keep their addresses
  void* kx0 = region("keep_x0"); void* kn = region("keep_noise"); void* km = region("keep_mask"); float* ks = region<float>("keep_sigma");
  m.ch.hold = region("hold"); m.ch.cut = region<int32_t>("cut");
  m.ex.keep_x0 = kx0; m.ex.keep_noise = kn; m.ex.keep_mask = km; m.ex.keep_sigma = ks;
}

using Tweak = std::function<void(Model&)>;

// mode 0: no blend (_ex, keep_* cleared); 1: the known-region blend (_ex); 2: the change-map blend (_ex2, keep_mask cleared)
void scenario(const std::string& name, int sampler, int phase, int mode, const Tweak& tweak = nullptr) {
  static Model m;
  build(m, sampler);
  m.s.phase = phase;
  if (phase == 0) m.s.cache = nullptr;
  if (mode == 0) m.ex.keep_x0 = m.ex.keep_noise = m.ex.keep_mask = nullptr, m.ex.keep_sigma = nullptr;
  if (mode == 2) m.ex.keep_mask = nullptr;
  if (tweak) tweak(m);
  tfx::g_probe_mask = 7;
  std::printf("== %s\n", name.c_str());
  const int rc = mode == 2 ? tfx_dit_step_run_ex2(&m.s, &m.ex, &m.ch, nullptr) : tfx_dit_step_run_ex(&m.s, &m.ex, nullptr);
  std::printf("rc %d\nerror %s\n", rc, rc ? tfx_last_error() : "");
  std::fflush(stdout);
}

// One blend-free step through entry point `how`: "run" tfx_dit_step_run, "ex" tfx_dit_step_run_ex with an all-NULL tfx_step_extra,
// "ex2" tfx_dit_step_run_ex2 with that and no change; for sampler 3 "multistep" tfx_dit_step_run_multistep and "ex" the history
// in a tfx_step_extra
void entry(const std::string& how, int sampler, int phase) {
  static Model m;
  build(m, sampler);
  m.s.phase = phase;
  if (phase == 0) m.s.cache = nullptr;
  tfx_step_extra ex{};
  ex.v_prev = m.ex.v_prev;
  tfx::g_probe_mask = 7;
  std::printf("== entry_%s_sampler%d_phase%d\n", how.c_str(), sampler, phase);
  const int rc = how == "run"         ? tfx_dit_step_run(&m.s, nullptr)
                 : how == "multistep" ? tfx_dit_step_run_multistep(&m.s, ex.v_prev, nullptr)
                 : how == "ex"        ? tfx_dit_step_run_ex(&m.s, &ex, nullptr)
                                      : tfx_dit_step_run_ex2(&m.s, &ex, nullptr, nullptr);
  std::printf("rc %d\nerror %s\n", rc, rc ? tfx_last_error() : "");
  std::fflush(stdout);
}

}  // namespace

int main() {
  const char* modes[3] = {"plain", "keep", "change"};
  for (int sampler = 0; sampler < 4; ++sampler)
    for (int phase : {0, 1, 2, 3})
      for (int mode = 0; mode < 3; ++mode)
        scenario(std::string(modes[mode]) + "_sampler" + std::to_string(sampler) + "_phase" + std::to_string(phase), sampler, phase, mode);
  for (int sampler = 0; sampler < 4; ++sampler)
    for (int phase : {0, 1, 2, 3})
      for (const char* how : {sampler == 3 ? "multistep" : "run", "ex", "ex2"}) entry(how, sampler, phase);
  // change == NULL through _ex2 is _ex
  {
    static Model m;
    build(m, 0);
    m.s.cache = nullptr;
    std::printf("== ex2_null_change\n");
    const int rc = tfx_dit_step_run_ex2(&m.s, &m.ex, nullptr, nullptr);
    std::printf("rc %d\nerror %s\n", rc, rc ? tfx_last_error() : "");
  }
  // ---- refusals of _ex2
  scenario("fail_keep_mask_set", 0, 0, 2, [](Model& m) { m.ex.keep_mask = m.ex.keep_x0; });
  scenario("fail_no_x0", 0, 0, 2, [](Model& m) { m.ex.keep_x0 = nullptr; });
  scenario("fail_no_noise", 2, 0, 2, [](Model& m) { m.ex.keep_noise = nullptr; });
  scenario("fail_no_sigma", 0, 0, 2, [](Model& m) { m.ex.keep_sigma = nullptr; });
  scenario("fail_no_hold", 0, 0, 2, [](Model& m) { m.ch.hold = nullptr; });
  scenario("fail_no_cut", 0, 0, 2, [](Model& m) { m.ch.cut = nullptr; });
  scenario("fail_seq_len", 2, 0, 2, [](Model& m) { m.d().seq_len = region<int32_t>("seq_len"); m.d().rope_bstride = 512; });
  scenario("fail_hold_in_xin", 2, 0, 2, [](Model& m) { m.ch.hold = (const char*)m.d().xin + 2 * 256 * 64 * 2 - 4; });
  scenario("fail_hold_in_latents", 0, 0, 2, [](Model& m) { m.ch.hold = m.s.latents; });
  scenario("fail_cut_in_out", 0, 0, 2, [](Model& m) { m.ch.cut = (const int32_t*)m.d().out; });
  scenario("fail_x0_in_v_prev", 3, 0, 2, [](Model& m) { m.ex.keep_x0 = m.ex.v_prev; });
  return 0;
}
