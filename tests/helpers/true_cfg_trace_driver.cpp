// Driver of true CFG's CPU launch-trace test (tests/test_true_cfg_cpu.py): the step descriptor of change_map_trace_driver.cpp (2 double
// + 2 single blocks, bf16, joint attention) with a batch of 4 = [2 negative; 2 positive] over fake device addresses, run through
// tfx_dit_step_run_ex3 with a tfx_step_cfg -- per sampler without a blend, with the known-region blend and with the change-map blend --
// against launch_recorder.cpp + step_cache_recorder.cpp + change_map_recorder.cpp + true_cfg_recorder.cpp; then the same descriptors with
// cfg == NULL through _ex3 and through _ex2 (the `null_*` scenarios), and every refusal.  Per scenario: a header line, the recorded
// launches, the return code and the error text.
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>

#include "textflux_hip.h"

namespace tfx {
extern int g_probe_mask;
void* cfg_region(const char* name);
void cfg_reset();
}  // namespace tfx

namespace {

template <class T = void>
T* region(const std::string& name) { return (T*)tfx::cfg_region(name.c_str()); }

struct Model {
  tfx_step_desc s;
  tfx_step_cache c;
  tfx_double_block dbl[2];
  tfx_single_block sgl[2];
  tfx_step_extra ex;
  tfx_step_change ch;
  tfx_step_cfg cfg;
  tfx_dit_desc& d() { return s.dit; }
};

void linear(tfx_linear& l, const std::string& name) {
  l.w = region(name + ".w");
  l.b = region(name + ".b");
}

// sampler 0 Euler, 1 AMO, 2 fused Euler, 3 multistep (sampler 0's descriptor and the history buffer); B: dit.B
void build(Model& m, int sampler, int B = 4) {
  tfx::cfg_reset();
  std::memset(&m, 0, sizeof m);
  tfx_dit_desc& d = m.d();
  const int H = 2, D = 128 * H, S = 256;
  d.D = D; d.H = H; d.in_channels = 64; d.out_channels = 16; d.n_double = 2; d.n_single = 2;
  d.B = B; d.S = S; d.T = 256;
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
  if (sampler == 3) m.ex.v_prev = region("v_prev");
  void* kx0 = region("keep_x0"); void* kn = region("keep_noise"); void* km = region("keep_mask"); float* ks = region<float>("keep_sigma");
  m.ch.hold = region("hold"); m.ch.cut = region<int32_t>("cut");
  m.ex.keep_x0 = kx0; m.ex.keep_noise = kn; m.ex.keep_mask = km; m.ex.keep_sigma = ks;
  m.cfg.scale = region<float>("cfg_scale");
}

using Tweak = std::function<void(Model&)>;

// mode 0: no blend; 1: the known-region blend; 2: the change-map blend.  how: "cfg" _ex3 with the tfx_step_cfg, "null" _ex3 with
// cfg == NULL, "ex2" tfx_dit_step_run_ex2
void scenario(const std::string& name, int sampler, int mode, const std::string& how, const Tweak& tweak = nullptr) {
  static Model m;
  build(m, sampler);
  if (mode == 0) m.ex.keep_x0 = m.ex.keep_noise = m.ex.keep_mask = nullptr, m.ex.keep_sigma = nullptr;
  if (mode == 2) m.ex.keep_mask = nullptr;
  if (tweak) tweak(m);
  tfx::g_probe_mask = 7;
  std::printf("== %s\n", name.c_str());
  const tfx_step_change* ch = mode == 2 ? &m.ch : nullptr;
  const int rc = how == "ex2" ? tfx_dit_step_run_ex2(&m.s, &m.ex, ch, nullptr)
                              : tfx_dit_step_run_ex3(&m.s, &m.ex, ch, how == "cfg" ? &m.cfg : nullptr, nullptr);
  std::printf("rc %d\nerror %s\n", rc, rc ? tfx_last_error() : "");
  std::fflush(stdout);
}

}  // namespace

int main() {
  const char* modes[3] = {"plain", "keep", "change"};
  for (int sampler : {0, 1, 3})
    for (int mode = 0; mode < 3; ++mode)
      scenario("cfg_sampler" + std::to_string(sampler) + "_" + modes[mode], sampler, mode, "cfg");
  for (int sampler = 0; sampler < 4; ++sampler)
    for (int mode = 0; mode < 3; ++mode)
      for (const char* how : {"null", "ex2"})
        scenario(std::string(how == std::string("null") ? "null_ex3" : "null_ex2") + "_sampler" + std::to_string(sampler) + "_" + modes[mode],
                 sampler, mode, how);
  // ---- refusals of _ex3 with cfg
  scenario("fail_sampler_2", 2, 0, "cfg");
  scenario("fail_seq_len", 0, 0, "cfg", [](Model& m) { m.d().seq_len = region<int32_t>("seq_len"); m.d().rope_bstride = 512; });
  for (int phase : {1, 2, 3})
    scenario("fail_phase_" + std::to_string(phase), 0, 0, "cfg", [phase](Model& m) { m.s.cache = &m.c; m.s.phase = phase; });
  scenario("fail_odd_B", 0, 0, "cfg", [](Model& m) { m.d().B = 3; m.s.mod_step_elems = 3 * m.d().mod_bstride; });
  scenario("fail_B_1", 0, 0, "cfg", [](Model& m) { m.d().B = 1; m.s.mod_step_elems = m.d().mod_bstride; });
  scenario("fail_null_scale", 0, 0, "cfg", [](Model& m) { m.cfg.scale = nullptr; });
  scenario("fail_scale_misaligned", 0, 0, "cfg", [](Model& m) { m.cfg.scale = (const float*)((const char*)m.cfg.scale + 2); });
  scenario("fail_scale_in_latents", 0, 0, "cfg", [](Model& m) { m.cfg.scale = (const float*)m.s.latents; });
  scenario("fail_scale_in_out_second_half", 0, 0, "cfg", [](Model& m) { m.cfg.scale = (const float*)((const char*)m.d().out + 4 * 256 * 16 * 2 - 4); });
  scenario("fail_scale_in_xin", 1, 0, "cfg", [](Model& m) { m.cfg.scale = (const float*)((const char*)m.d().xin + 4 * 256 * 64 * 2 - 4); });
  scenario("fail_scale_in_mod_cur", 0, 0, "cfg", [](Model& m) { m.cfg.scale = (const float*)m.s.mod_cur; });
  scenario("fail_scale_in_step_ptr", 0, 0, "cfg", [](Model& m) { m.cfg.scale = (const float*)m.s.step_ptr; });
  scenario("fail_scale_in_v_prev", 3, 0, "cfg", [](Model& m) { m.cfg.scale = (const float*)((const char*)m.ex.v_prev + 2 * 256 * 16 * 2 - 4); });
  scenario("fail_scale_in_hid", 0, 0, "cfg", [](Model& m) { m.cfg.scale = (const float*)m.d().hid; });
  // the blends' buffers have B * S rows: keep_x0 may end where the second half of a 2B-row buffer would begin, but not inside latents
  scenario("fail_keep_x0_in_latents", 0, 1, "cfg", [](Model& m) { m.ex.keep_x0 = (const char*)m.s.latents + 2 * 256 * 16 * 2 - 16; });
  scenario("cfg_latents_half_then_keep_x0", 0, 1, "cfg", [](Model& m) { m.ex.keep_x0 = (const char*)m.s.latents + 2 * 256 * 16 * 2; });
  return 0;
}
