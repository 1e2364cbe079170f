// Driver of the CPU launch-trace test (tests/test_dit_launch_trace.py): builds tfx_dit_desc / tfx_step_desc values over fake device
// addresses and calls the public entry points; the launch layer behind them is launch_recorder.cpp.  Per scenario: a header line,
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
void drop_w8(tfx_linear& l) { l.w8 = nullptr; l.w8_scale = nullptr; }
// a runtime LoRA adapter on `l` (in_features K): the up-projection rows behind the weight rows
void adapt(tfx_linear& l, const std::string& name, int K, int R, int nseg, int mask, int scale_off) {
  l.ldw = K + R;
  l.lora_a = region(name + ".lora_a");
  l.lora_r = R; l.lora_nseg = nseg; l.lora_mask = mask; l.lora_scale_off = scale_off;
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
void with_option(const char* option, int value, const char* name, const Cfg& c) {
  tfx_set_option(option, value);
  scenario(name, c);
  tfx_set_option(option, 1);
}

Cfg cfg(int H, int T, int mask, bool fp8 = false) {
  Cfg c;
  c.H = H; c.T = T; c.mask = mask; c.fp8 = fp8;
  return c;
}
Cfg part(Cfg c) { c.part = 1; return c; }
Cfg dbl1(Cfg c) { c.part = 2; return c; }
// no block at all: x_embedder (unless flags bit 0) and the tail (unless bit 1)
void no_blocks(Model& m) { m.d().first_block = m.d().last_block = 4; }

}  // namespace

int main() {
  const int ALL = ROWSPLIT | QKN | FP8_QKN;
  const Cfg joint = cfg(2, 256, ALL), sep100 = cfg(2, 100, QKN | FP8_QKN), fp8 = cfg(2, 256, ALL, true);
  // The scenarios that vary one thing run blocks [1, 3) (part) or the double block 1 alone (dbl1): offsets into mod / dbl[] / sgl[]
  // beyond block 0 are in every one of them.

  // ---- bf16, joint (T = 256: one row-split launch over [text | image])
  scenario("bf16_joint", joint);
  scenario("bf16_joint_qkn_refused", part(cfg(2, 256, ROWSPLIT | FP8_QKN)));
  scenario("bf16_joint_no_rope_cs", part(joint), [](Model& m) { m.d().rope_cs = nullptr; });
  with_option("ln_joint", 0, "bf16_joint_ln_joint_0", dbl1(joint));
  with_option("gemm_group_streams", 0, "bf16_group_streams_0", dbl1(joint));

  // ---- bf16, separate (image launch, then text launch)
  scenario("bf16_separate_T100", sep100);
  scenario("bf16_separate_T100_qkn_refused", part(cfg(2, 100, FP8_QKN)));
  scenario("bf16_separate_T100_no_rope_cs", part(sep100), [](Model& m) { m.d().rope_cs = nullptr; });
  scenario("bf16_separate_T256_rowsplit_refused", dbl1(cfg(2, 256, QKN | FP8_QKN)));
  scenario("bf16_separate_T0", cfg(2, 0, ALL));

  // ---- fp8 linears (flags bit 2, w8 on every block Linear)
  scenario("fp8_H2", fp8);
  scenario("fp8_H2_qkn_refused", part(cfg(2, 256, ROWSPLIT | QKN, true)));
  with_option("fp8_fuse_qkn", 0, "fp8_H2_fuse_qkn_0", part(fp8));
  scenario("fp8_H1_bf16_fallback", part(cfg(1, 256, ALL, true)));   // K = 128 is not a multiple of 256
  scenario("fp8_linears_without_w8", part(fp8), [](Model& m) { drop_w8(m.dbl[1].qkv_img); drop_w8(m.dbl[1].ff2_txt); drop_w8(m.sgl[0].proj_out); });
  scenario("fp8_T0", part(cfg(2, 0, ALL, true)));

  // ---- runtime LoRA adapters
  scenario("lora_joint_img_D384", dbl1(cfg(3, 256, ALL)), [](Model& m) {   // nseg * R = 384 fits the row pitch
    const int D = m.d().D;
    tfx_double_block& w = m.dbl[1];
    adapt(w.qkv_img, "d1.qkv_img", D, 128, 3, 7, 0); w.qkv_txt.ldw = D + 128;
    adapt(w.out_img, "d1.out_img", D, 128, 1, 1, 384); w.out_txt.ldw = D + 128;
    adapt(w.ff1_img, "d1.ff1_img", D, 128, 1, 1, 512); w.ff1_txt.ldw = D + 128;
    adapt(w.ff2_img, "d1.ff2_img", 4 * D, 256, 1, 1, 640); w.ff2_txt.ldw = 4 * D + 256;
  });
  scenario("lora_joint_both_D384", cfg(3, 256, ALL), [](Model& m) {
    const int D = m.d().D;
    adapt(m.dbl[0].qkv_img, "d0.qkv_img", D, 128, 3, 5, 0); adapt(m.dbl[0].qkv_txt, "d0.qkv_txt", D, 128, 3, 3, 384);
    adapt(m.dbl[1].out_img, "d1.out_img", D, 128, 1, 1, 768); adapt(m.dbl[1].out_txt, "d1.out_txt", D, 128, 1, 1, 896);
    adapt(m.dbl[1].ff1_txt, "d1.ff1_txt", D, 128, 1, 1, 1024); m.dbl[1].ff1_img.ldw = D + 128;   // text adapted, image not
  });
  scenario("lora_separate_D384", dbl1(cfg(3, 100, QKN | FP8_QKN)), [](Model& m) {
    const int D = m.d().D;
    tfx_double_block& w = m.dbl[1];
    adapt(w.qkv_img, "d1.qkv_img", D, 128, 3, 7, 0); adapt(w.qkv_txt, "d1.qkv_txt", D, 128, 3, 6, 384);
    adapt(w.out_txt, "d1.out_txt", D, 128, 1, 1, 768);
    adapt(w.ff1_img, "d1.ff1_img", D, 128, 1, 1, 896);
    adapt(w.ff2_txt, "d1.ff2_txt", 4 * D, 128, 1, 1, 1024);
  });
  scenario("lora_separate_no_rope_cs", dbl1(cfg(3, 100, QKN | FP8_QKN)), [](Model& m) {
    m.d().rope_cs = nullptr;
    adapt(m.dbl[1].qkv_img, "d1.qkv_img", m.d().D, 128, 3, 7, 0);
  });
  scenario("lora_planes_joint_D256", dbl1(joint), [](Model& m) {    // nseg * R = 384 > 256: one T matrix per segment
    const int D = m.d().D;
    adapt(m.dbl[1].qkv_img, "d1.qkv_img", D, 128, 3, 5, 0); adapt(m.dbl[1].qkv_txt, "d1.qkv_txt", D, 128, 3, 7, 384);
  });
  scenario("lora_planes_separate_D256", dbl1(sep100), [](Model& m) { adapt(m.dbl[1].qkv_img, "d1.qkv_img", m.d().D, 128, 3, 6, 0); });
  scenario("lora_single_D512", part(cfg(4, 256, ALL)), [](Model& m) {
    const int D = m.d().D;
    adapt(m.sgl[0].qkv_mlp, "s0.qkv_mlp", D, 128, 4, 15, 0);
    adapt(m.sgl[0].proj_out, "s0.proj_out", 5 * D, 128, 1, 1, 512);   // input in y
  });
  scenario("lora_single_planes_D256", joint, [](Model& m) {
    const int D = m.d().D;
    m.d().flags = 3; m.d().first_block = 2;
    adapt(m.sgl[1].qkv_mlp, "s1.qkv_mlp", D, 128, 4, 11, 0);
    adapt(m.sgl[0].proj_out, "s0.proj_out", 5 * D, 256, 1, 1, 512);
  });
  scenario("lora_desc_proj_out", joint, [](Model& m) { no_blocks(m); adapt(m.d().proj_out, "proj_out", m.d().D, 128, 1, 1, 0); });
  scenario("lora_desc_proj_out_euler_gate", joint, [](Model& m) { no_blocks(m); euler_gate(m); adapt(m.d().proj_out, "proj_out", m.d().D, 128, 1, 1, 0); });

  // ---- LoRA failures
  const Tweak qkv0 = [](Model& m) { adapt(m.dbl[0].qkv_img, "d0.qkv_img", m.d().D, 128, 3, 7, 0); m.dbl[0].qkv_txt.ldw = m.d().D + 128; };
  scenario("lora_fail_null_t_xn", joint, [&](Model& m) { qkv0(m); m.d().lora_t_xn = nullptr; });
  scenario("lora_fail_null_t_y", joint, [&](Model& m) { qkv0(m); m.d().lora_t_y = nullptr; });
  scenario("lora_fail_null_scale", joint, [&](Model& m) { qkv0(m); m.d().lora_scale = nullptr; });
  scenario("lora_fail_fp8_quantised_by_ln", fp8, qkv0);
  scenario("lora_fail_fp8_quantise_pass", fp8, [](Model& m) { adapt(m.dbl[0].out_img, "d0.out_img", m.d().D, 128, 1, 1, 0); });
  scenario("lora_fail_fp8_without_w8", fp8, [&](Model& m) { qkv0(m); drop_w8(m.dbl[0].qkv_img); });
  scenario("lora_fail_partner_ldw", joint, [&](Model& m) { qkv0(m); m.dbl[0].qkv_txt.ldw = 0; });
  scenario("lora_fail_partner_rank", joint, [&](Model& m) { qkv0(m); adapt(m.dbl[0].qkv_txt, "d0.qkv_txt", m.d().D, 128, 2, 3, 384); });
  scenario("lora_fail_nseg_5", joint, [&](Model& m) { qkv0(m); m.dbl[0].qkv_img.lora_nseg = 5; });
  scenario("lora_fail_rank_0", sep100, [&](Model& m) { qkv0(m); m.dbl[0].qkv_img.lora_r = 0; });
  scenario("lora_fail_x_embedder", joint, [](Model& m) { adapt(m.d().x_embedder, "x_embedder", 64, 128, 1, 1, 0); });
  scenario("lora_fail_planes_in_y", part(cfg(1, 256, ALL)), [](Model& m) { adapt(m.sgl[0].proj_out, "s0.proj_out", 5 * m.d().D, 256, 4, 15, 0); });

  // ---- block ranges and flags
  scenario("flags_1_skip_embed", joint, [](Model& m) { no_blocks(m); m.d().flags = 1; });
  scenario("flags_2_skip_tail", joint, [](Model& m) { no_blocks(m); m.d().flags = 2; });
  scenario("flags_3", sep100, [](Model& m) { m.d().flags = 3; m.d().last_block = 3; });
  scenario("blocks_0_1", joint, [](Model& m) { m.d().flags = 3; m.d().last_block = 1; });
  scenario("blocks_1_3", part(joint));
  scenario("blocks_3_4_separate", sep100, [](Model& m) { m.d().flags = 3; m.d().first_block = 3; m.d().last_block = 4; });
  scenario("blocks_first_negative_last_beyond", cfg(2, 0, ALL), [](Model& m) { m.d().flags = 3; m.d().first_block = -2; m.d().last_block = 9; });
  scenario("euler_gate", joint, [](Model& m) { no_blocks(m); euler_gate(m); });

  // ---- the step path
  scenario("step_sampler_0", part(joint), [](Model& m) { m.d().flags = 0; }, STEP);
  scenario("step_sampler_1", part(sep100), [](Model& m) { m.s.sampler = 1; m.d().flags = 0; }, STEP);
  scenario("step_sampler_2", part(joint), [](Model& m) { m.s.sampler = 2; m.d().flags = 0; euler_gate(m); }, STEP);
  scenario("step_fail_null_desc", joint, nullptr, STEP_NULL);
  scenario("step_fail_null_mod_table", joint, [](Model& m) { m.s.mod_table = nullptr; }, STEP);
  scenario("step_fail_null_mod_cur", joint, [](Model& m) { m.s.mod_cur = nullptr; }, STEP);
  scenario("step_fail_null_step_ptr", joint, [](Model& m) { m.s.step_ptr = nullptr; }, STEP);
  scenario("step_fail_mod_not_mod_cur", joint, [](Model& m) { m.s.mod_cur = (char*)m.s.mod_cur + 16; }, STEP);
  scenario("step_fail_sampler_3", joint, [](Model& m) { m.s.sampler = 3; }, STEP);
  scenario("step_fail_sampler_negative", joint, [](Model& m) { m.s.sampler = -1; }, STEP);
  scenario("step_fail_sampler_2_null_gate", joint, [](Model& m) { m.s.sampler = 2; }, STEP);
  scenario("step_fail_sampler_2_gate_outside", joint, [](Model& m) { m.s.sampler = 2; m.d().euler_gate = m.d().xn; }, STEP);
  scenario("step_fail_gate_without_sampler_2", joint, euler_gate, STEP);
  scenario("step_fail_null_latents", joint, [](Model& m) { m.s.latents = nullptr; }, STEP);
  scenario("step_fail_null_coef", joint, [](Model& m) { m.s.coef = nullptr; }, STEP);
  scenario("step_fail_amo_null_noise", joint, [](Model& m) { m.s.sampler = 1; m.s.noise = nullptr; }, STEP);
  scenario("step_fail_null_out", joint, [](Model& m) { m.d().out = nullptr; }, STEP);
  scenario("step_fail_forward_refuses", joint, [](Model& m) { m.d().H = 3; }, STEP);

  // ---- descriptor failures
  scenario("fail_D_not_128H", joint, [](Model& m) { m.d().H = 3; });
  scenario("fail_B_0", joint, [](Model& m) { m.d().B = 0; });
  scenario("fail_S_0", joint, [](Model& m) { m.d().S = 0; });
  scenario("fail_T_negative", joint, [](Model& m) { m.d().T = -1; });
  scenario("fail_fp8_null_q8", fp8, [](Model& m) { m.d().q8 = nullptr; });
  scenario("fail_fp8_null_q8_scale", fp8, [](Model& m) { m.d().q8_scale = nullptr; });
  scenario("fail_null_desc", joint, nullptr, FORWARD_NULL);
  scenario("fail_null_xin", joint, [](Model& m) { m.d().xin = nullptr; });
  scenario("fail_null_mod", joint, [](Model& m) { m.d().mod = nullptr; });
  scenario("fail_null_hid", joint, [](Model& m) { m.d().hid = nullptr; });
  scenario("fail_null_xn", joint, [](Model& m) { m.d().xn = nullptr; });
  scenario("fail_null_y", joint, [](Model& m) { m.d().y = nullptr; });
  scenario("fail_null_out", joint, [](Model& m) { m.d().out = nullptr; });
  scenario("fail_null_cos_tab", joint, [](Model& m) { m.d().cos_tab = nullptr; });
  scenario("fail_null_sin_tab", joint, [](Model& m) { m.d().sin_tab = nullptr; });
  scenario("fail_null_dbl", joint, [](Model& m) { m.d().dbl = nullptr; });
  scenario("fail_null_sgl", joint, [](Model& m) { m.d().sgl = nullptr; });
  scenario("fail_null_ctx0", joint, [](Model& m) { m.d().ctx0 = nullptr; });
  return 0;
}
