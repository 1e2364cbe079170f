// Driver of the mixed-geometry launch trace (tests/test_mixed_batch_cpu.py), the counterpart of dit_trace_driver.cpp for descriptors that
// carry seq_len / rope_bstride: builds tfx_dit_desc / tfx_step_desc values over fake device
// addresses and calls the public entry points; the launch layer behind them is mixed_launch_recorder.cpp.  Per scenario: a header line,
// the recorded launches, the return code and the error text.  A small model: 2 double + 2 single blocks, batch 2, D = 128 * H.
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>

#include "textflux_hip.h"

namespace tfx {
extern int g_probe_mask;
void* trace_region(const char* name);
void trace_reset();
}  // namespace tfx

namespace {

constexpr int ROWSPLIT = 1, QKN = 2, FP8_QKN = 4;   // bits of the recorder's probe mask

template <class T = void>
T* region(const std::string& name) { return (T*)tfx::trace_region(name.c_str()); }

struct Cfg {
  int H = 2, T = 256, S = 256, mask = ROWSPLIT | QKN | FP8_QKN;
  bool fp8 = false;   // flags bit 2, w8 on every Linear
  int part = 0;       // 1: blocks [1, 3) only (the second double and the first single block), no x_embedder, no tail; 2: block 1 only
};

struct Model {
  tfx_step_desc s;
  tfx_double_block dbl[2];
  tfx_single_block sgl[2];
  tfx_dit_desc& d() { return s.dit; }
};

void linear(tfx_linear& l, const std::string& name, bool w8) {
  l.w = region(name + ".w");
  l.b = region(name + ".b");
  if (w8) { l.w8 = region(name + ".w8"); l.w8_scale = region<float>(name + ".w8s"); }
}
void build(Model& m, const Cfg& c) {
  tfx::trace_reset();
  std::memset(&m, 0, sizeof m);
  tfx_dit_desc& d = m.d();
  const int D = 128 * c.H;
  d.D = D; d.H = c.H; d.in_channels = 64; d.out_channels = 16; d.n_double = 2; d.n_single = 2;
  d.B = 2; d.S = c.S; d.T = c.T;
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
  }
  for (int j = 0; j < 2; ++j) {
    tfx_single_block& w = m.sgl[j];
    const std::string n = "s" + std::to_string(j) + ".";
    linear(w.qkv_mlp, n + "qkv_mlp", c.fp8); linear(w.proj_out, n + "proj_out", c.fp8);
    w.norm_q = region(n + "norm_q"); w.norm_k = region(n + "norm_k");
  }
  // block 0 has no score bound of its own: its attention launch falls back to the forward-wide one
  m.dbl[0].attn_score_bound = 0.f; m.dbl[1].attn_score_bound = 3.5f; m.sgl[0].attn_score_bound = 4.5f; m.sgl[1].attn_score_bound = 0.f;
  d.attn_score_bound = 9.25f;
  d.dbl = m.dbl; d.sgl = m.sgl;
  d.xin = region("xin"); d.ctx0 = c.T > 0 ? region("ctx0") : nullptr;
  const int mod_len = 2 * 12 * D + 2 * 3 * D + 2 * D;
  d.mod = region("mod"); d.mod_bstride = mod_len + d.out_channels;   // the dsigma row of sampler 2 travels behind the modulation rows
  d.cos_tab = region<float>("cos"); d.sin_tab = region<float>("sin");
  d.hid = region("hid"); d.xn = region("xn"); d.y = region("y"); d.out = region("out");
  d.first_block = c.part ? 1 : 0; d.last_block = c.part ? 4 - c.part : -1; d.flags = (c.fp8 ? 4 : 0) | (c.part ? 3 : 0);
  d.q8 = region("q8"); d.q8_scale = region<float>("q8s");
  d.gemm_workspace = region("ws"); d.gemm_workspace_bytes = 128ll << 20;
  d.rope_cs = region<float>("rope_cs");
  d.lora_t_xn = region("lora_t_xn"); d.lora_t_y = region("lora_t_y"); d.lora_scale = region<float>("lora_scale");
  m.s.mod_table = region("mod_table"); m.s.mod_cur = const_cast<void*>(d.mod); m.s.mod_step_elems = d.B * d.mod_bstride;
  m.s.step_ptr = region<int32_t>("step_ptr"); m.s.latents = region("latents");
  m.s.coef = region<float>("coef"); m.s.noise = region<float>("noise"); m.s.sampler = 0;
}
void euler_gate(Model& m) {
  tfx_dit_desc& d = m.d();
  d.euler_gate = (const char*)d.mod + (d.mod_bstride - d.out_channels) * 2; d.euler_gate_bstride = d.mod_bstride;
}

using Tweak = std::function<void(Model&)>;
enum Entry { FORWARD, FORWARD_NULL, STEP, STEP_NULL };

void scenario(const char* name, const Cfg& c, const Tweak& tweak = nullptr, Entry entry = FORWARD) {
  static Model m;
  build(m, c);
  if (tweak) tweak(m);
  tfx::g_probe_mask = c.mask;
  std::printf("== %s\n", name);
  int rc = 0;
  switch (entry) {
    case FORWARD: rc = tfx_dit_forward(&m.d(), nullptr); break;
    case FORWARD_NULL: rc = tfx_dit_forward(nullptr, nullptr); break;
    case STEP: rc = tfx_dit_step_run(&m.s, nullptr); break;
    case STEP_NULL: rc = tfx_dit_step_run(nullptr, nullptr); break;
  }
  std::printf("rc %d\nerror %s\n", rc, rc ? tfx_last_error() : "");
  std::fflush(stdout);
}

Cfg cfg(int H, int T, int mask, bool fp8 = false) {
  Cfg c;
  c.H = H; c.T = T; c.mask = mask; c.fp8 = fp8;
  return c;
}
// the mixed-geometry fields: one length per sample, one rotary table per sample N rows apart
void mixed(Model& m) {
  tfx_dit_desc& d = m.d();
  d.seq_len = region<int32_t>("seq_len");
  d.rope_bstride = d.S + d.T;
}

}  // namespace

int main() {
  const int ALL = ROWSPLIT | QKN | FP8_QKN;
  const Cfg joint = cfg(2, 256, ALL), sep100 = cfg(2, 100, QKN | FP8_QKN), fp8 = cfg(2, 256, ALL, true);
  // one whole mixed forward (joint launches, fused q / k norm + RoPE with the per-sample table stride, seq_len on every attention launch)
  scenario("mixed_bf16_joint", joint, mixed);
  // the separate norm + RoPE pass takes the per-sample tables too (no pair table; the text rows apart: T = 100)
  scenario("mixed_bf16_separate_no_rope_cs", sep100, [](Model& m) { mixed(m); m.d().rope_cs = nullptr; m.d().first_block = 1; m.d().last_block = 3; m.d().flags = 3; });
  scenario("mixed_fp8", fp8, [](Model& m) { mixed(m); m.d().first_block = 1; m.d().last_block = 3; m.d().flags = 4 | 3; });
  // per-sample tables without lengths: allowed (the stride alone changes the rotary addressing)
  scenario("rope_bstride_alone", joint, [](Model& m) { m.d().rope_bstride = m.d().S + m.d().T; m.d().first_block = 1; m.d().last_block = 2; m.d().flags = 3; });
  // the step path: only the fused Euler form carries per-sample coefficients
  scenario("mixed_step_sampler_2", joint, [](Model& m) { mixed(m); m.s.sampler = 2; euler_gate(m); m.d().first_block = 1; m.d().last_block = 2; }, STEP);
  // ---- refusals
  scenario("mixed_fail_rope_bstride_0", joint, [](Model& m) { mixed(m); m.d().rope_bstride = 0; });
  scenario("mixed_fail_rope_bstride_negative", joint, [](Model& m) { m.d().rope_bstride = -8; });
  scenario("mixed_step_fail_sampler_0", joint, mixed, STEP);
  scenario("mixed_step_fail_sampler_1", joint, [](Model& m) { mixed(m); m.s.sampler = 1; }, STEP);
  return 0;
}
