// extern "C" surface of libtextflux_hip.so (declared in include/textflux_hip.h): argument checks and conversions in front of the
// launch API (launch.h), tfx_set_option, the workspace layout and the step graph.  The DiT forward itself is dit_forward.cpp.
#include "../../include/textflux_hip.h"

#include <cstring>

#include "launch.h"

using namespace tfx;

namespace {

inline hipStream_t S(tfx_stream s) { return (hipStream_t)s; }

// true when one of the pointers is not 16-byte aligned (the kernels behind the entries that ask read and write 16-byte vectors)
template <typename... P>
inline bool misaligned16(P... p) { return (((uintptr_t)p | ...) % 16) != 0; }

#define TRY(x)            \
  do {                    \
    if (int _e = (x)) return _e; \
  } while (0)

}  // namespace

extern "C" {

const char* tfx_version(void) { return "textflux_hip 0.1 (gfx950)"; }
const char* tfx_last_error(void) { return last_error(); }
int tfx_abi_info(int32_t* out, int n) {
  const int32_t v[7] = {TFX_ABI_VERSION, (int32_t)sizeof(tfx_gemm_args), (int32_t)sizeof(tfx_attn_args), (int32_t)sizeof(tfx_dit_desc),
                        (int32_t)sizeof(tfx_step_desc), (int32_t)sizeof(tfx_double_block), (int32_t)sizeof(tfx_single_block)};
  for (int i = 0; i < 7 && i < n; ++i) out[i] = v[i];
  return 7;
}

int tfx_query_arch(char* buf, int buflen) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return fail("tfx_query_arch: no HIP device");
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return fail("tfx_query_arch: hipGetDeviceProperties failed");
  if (buf && buflen > 0) {
    std::strncpy(buf, prop.gcnArchName, buflen - 1);
    buf[buflen - 1] = 0;
  }
  return 0;
}

#ifdef TFX_BENCH
// bench library only (tools/gemm_phase_timers.py, gemm_shapes_power.py): the next tfx_gemm_bf16 calls carry the DiT's fused q / k
// RMSNorm + RoPE epilogue on the [k | v | q | ...] column layout, as tfx_dit_forward attaches it internally
static struct { const void* wq; const void* wk; const float* cs; int D; } g_bench_qkn = {nullptr, nullptr, nullptr, 0};
extern "C" void tfx_bench_gemm_qkn(const void* wq, const void* wk, const float* cs, int D) { g_bench_qkn = {wq, wk, cs, D}; }
#endif

// The one tfx_gemm_args -> GemmArgs conversion: every field of the public struct.  Entry points whose launcher must not see a field
// reset it afterwards (and say why); everything GemmArgs has beyond the public struct keeps its default.
static GemmArgs gemm_args(const tfx_gemm_args* g) {
  GemmArgs a;
  a.A = g->A; a.lda = g->lda; a.a_bstride = g->a_bstride;
  a.W = g->W; a.ldw = g->ldw; a.bias = g->bias; a.w_bstride = g->w_bstride;
  a.C = g->C; a.ldc = g->ldc; a.c_bstride = g->c_bstride;
  a.M = g->M; a.N = g->N; a.K = g->K; a.batch = g->batch;
  a.epilogue = g->epilogue; a.gelu_from_col = g->gelu_from_col;
  a.gate = g->gate; a.gate_bstride = g->gate_bstride;
  a.res = g->res; a.ldr = g->ldr; a.r_bstride = g->r_bstride;
  a.workspace = g->workspace; a.workspace_bytes = g->workspace_bytes;
  a.cscale = g->cscale;
  return a;
}

// Validates a tfx_qkn_args against the GEMM it rides on and attaches it.  The fused epilogue is an instantiation of the bias + GELU
// kernel (norm tiles and GELU tiles are separate straight-line paths): plain bias = GELU from a column beyond N, as tfx_dit_forward
// passes it; it takes neither gate nor residual.
static int attach_qkn(const char* who, GemmArgs& a, const tfx_qkn_args* q) {
  if (!q->norm_q || !q->norm_k || !q->rope_cs) return fail("%s: norm weights and the rotary table are required", who);
  if ((uintptr_t)q->norm_q % 16 || (uintptr_t)q->norm_k % 16 || (uintptr_t)q->rope_cs % 16)
    return fail("%s: norm weights and the rotary table must be 16-byte aligned", who);
  if (q->q0 < 0 || q->q1 < q->q0 || q->q1 > a.N || q->k0 < 0 || q->k1 < q->k0 || q->k1 > a.N || q->pos0 < 0)
    return fail("%s: column ranges outside [0, N)", who);
  if (q->rope_bstride < 0) return fail("%s: rope_bstride must not be negative", who);
  if (a.epilogue != EPI_BIAS && a.epilogue != EPI_BIAS_GELU)
    return fail("%s: with q/k norm the epilogue must be 0 (bias) or 1 (bias + GELU from a column)", who);
  if (a.epilogue == EPI_BIAS) a.gelu_from_col = (a.N + 255) / 256 * 256;
  a.epilogue = EPI_BIAS_GELU;
  a.gate = nullptr; a.gate_bstride = 0; a.res = nullptr; a.ldr = 0; a.r_bstride = 0;
  a.qkn_wq = q->norm_q; a.qkn_wk = q->norm_k; a.qkn_rope_cs = q->rope_cs; a.qkn_pos0 = q->pos0; a.qkn_rope_bstride = q->rope_bstride;
  a.qkn_q0 = q->q0; a.qkn_q1 = q->q1; a.qkn_k0 = q->k0; a.qkn_k1 = q->k1; a.qkn_eps = q->eps;
  return 0;
}

int tfx_gemm_bf16(const tfx_gemm_args* g, int variant, tfx_stream stream) {
  if (!g) return fail("tfx_gemm_bf16: null args");
  GemmArgs a = gemm_args(g);
  if (!a.A || !a.W || !a.C) return fail("tfx_gemm_bf16: null matrix pointer");
#ifdef TFX_BENCH
  if (g_bench_qkn.cs) {
    const int D = g_bench_qkn.D;
    a.qkn_wq = g_bench_qkn.wq; a.qkn_wk = g_bench_qkn.wk; a.qkn_rope_cs = g_bench_qkn.cs; a.qkn_pos0 = 0;
    a.qkn_k0 = 0; a.qkn_k1 = D; a.qkn_q0 = 2 * D; a.qkn_q1 = 3 * D; a.qkn_eps = 1e-6f;
    if (!gemm_qkn_ok(a)) return fail("tfx_bench_gemm_qkn: shape cannot carry the fused epilogue");
  }
#endif
  return variant < 0 ? gemm_bf16(a, S(stream)) : gemm_bf16_variant(a, variant, S(stream));
}

int tfx_gemm_bf16_qkn(const tfx_gemm_args* g, const tfx_qkn_args* q, tfx_stream stream) {
  if (!g || !q) return fail("tfx_gemm_bf16_qkn: null args");
  if (!g->A || !g->W || !g->C) return fail("tfx_gemm_bf16_qkn: null matrix pointer");
  GemmArgs a = gemm_args(g);
  a.cscale = nullptr;                 // the column-scale epilogue is not one this entry point admits
  if (const int rc = attach_qkn("tfx_gemm_bf16_qkn", a, q)) return rc;
  return gemm_bf16(a, S(stream));     // refuses shapes the fused epilogue cannot take (gemm_qkn_ok)
}

int tfx_gemm_bf16_lora(const tfx_gemm_args* g, const tfx_qkn_args* q, const tfx_lora_args* l, tfx_stream stream) {
  if (!g || !l) return fail("tfx_gemm_bf16_lora: null args");
  if (!g->A || !g->W || !g->C) return fail("tfx_gemm_bf16_lora: null matrix pointer");
  if (!l->T || !l->Bm) return fail("tfx_gemm_bf16_lora: null adapter operand (T / Bm)");
  GemmArgs a = gemm_args(g);
  a.workspace = nullptr; a.workspace_bytes = 0;   // an adapted GEMM is never K-sliced
  a.cscale = nullptr;                             // gemm_bf16_lora refuses the column-scale epilogue
  if (q)
    if (const int rc = attach_qkn("tfx_gemm_bf16_lora", a, q)) return rc;
  if (l->split_row > 0) {
    if (!l->W2) return fail("tfx_gemm_bf16_lora: row-split weights need W2");
    if (q && ((uintptr_t)l->norm_q2 % 16 || (uintptr_t)l->norm_k2 % 16)) return fail("tfx_gemm_bf16_lora: norm_q2 / norm_k2 must be 16-byte aligned");
    a.split_row = l->split_row; a.W2 = l->W2; a.bias2 = l->bias2; a.gate2 = l->gate2; a.qkn_wq2 = l->norm_q2; a.qkn_wk2 = l->norm_k2;
  } else if (l->split_row < 0) {
    return fail("tfx_gemm_bf16_lora: split_row must not be negative");
  }
  if (l->t_seg_stride < 0) return fail("tfx_gemm_bf16_lora: t_seg_stride must not be negative");
  LoraArgs la{l->T, l->Bm, l->R, l->seg_cols, l->nseg, l->seg_mask, l->t_seg_stride};
  return gemm_bf16_lora(a, la, S(stream));
}

int tfx_gemm_bf16_f32(const tfx_gemm_args* g, tfx_stream stream) {
  if (!g) return fail("tfx_gemm_bf16_f32: null args");
  if (!g->A || !g->W || !g->C) return fail("tfx_gemm_bf16_f32: null matrix pointer");
  GemmArgs a = gemm_args(g);
  // raw accumulators: gemm_bf16_f32out admits the plain epilogue only, and its fast_ok() looks at gelu_from_col / gate / res solely
  // under the other epilogues -- reset all the same, with the workspace it never K-slices into and the scale vector of an epilogue it refuses
  a.gelu_from_col = 0;
  a.gate = nullptr; a.gate_bstride = 0; a.res = nullptr; a.ldr = 0; a.r_bstride = 0;
  a.workspace = nullptr; a.workspace_bytes = 0; a.cscale = nullptr;
  return gemm_bf16_f32out(a, S(stream));
}

int tfx_gemm_fp8(const tfx_gemm_args* g, const float* a_scale, int64_t a_scale_bstride, const float* w_scale,
                 tfx_stream stream) {
  if (!g) return fail("tfx_gemm_fp8: null args");
  GemmArgs a = gemm_args(g);
  a.cscale = nullptr;                 // gemm_fp8 has no column-scale epilogue (it reports 4 as unknown)
  a.a_scale = a_scale; a.a_scale_bstride = a_scale_bstride; a.w_scale = w_scale;
  if (!a.A || !a.W || !a.C) return fail("tfx_gemm_fp8: null matrix pointer");
  return gemm_fp8(a, S(stream));
}

int tfx_quantize_rows_fp8(const void* x, int64_t ldx, int64_t x_bstride, void* out, int64_t ldo, int64_t o_bstride,
                          float* scale, int64_t s_bstride, int32_t rows, int32_t batch, int32_t K, tfx_stream stream) {
  if (!x || !out || !scale) return fail("tfx_quantize_rows_fp8: null pointer");
  return quantize_rows_fp8(x, ldx, x_bstride, out, ldo, o_bstride, scale, s_bstride, rows, batch, K, S(stream));
}

int tfx_ln_modulate_fp8(const void* x, int64_t ldx, int64_t x_bstride, void* q8, int64_t ldq, int64_t q_bstride,
                        float* q8_scale, int64_t s_bstride, const void* shift, const void* scale, int64_t mod_bstride,
                        int32_t rows_per_batch, int32_t batch, int32_t D, float eps, tfx_stream stream) {
  if (!x || !q8 || !q8_scale || !shift || !scale) return fail("tfx_ln_modulate_fp8: null pointer");
  return ln_modulate_fp8(x, q8, q8_scale, shift, scale, mod_bstride, rows_per_batch, batch, D, ldx, x_bstride, ldq,
                         q_bstride, s_bstride, eps, S(stream));
}

int tfx_ln_modulate(const void* x, int64_t ldx, int64_t x_bstride, void* out, int64_t ldo, int64_t o_bstride,
                    const void* shift, const void* scale, int64_t mod_bstride, int32_t rows_per_batch, int32_t batch,
                    int32_t D, float eps, tfx_stream stream) {
  if (!x || !out || !shift || !scale) return fail("tfx_ln_modulate: null pointer");
  return ln_modulate(x, out, shift, scale, mod_bstride, rows_per_batch, batch, D, ldx, x_bstride, ldo, o_bstride, eps,
                     S(stream));
}

int tfx_ln_modulate_split(const void* x, int64_t ldx, int64_t x_bstride, void* out, int64_t ldo, int64_t o_bstride,
                          const void* shift, const void* scale, const void* shift2, const void* scale2, int32_t split_row,
                          int64_t mod_bstride, int32_t rows_per_batch, int32_t batch, int32_t D, float eps, tfx_stream stream) {
  if (!x || !out || !shift || !scale) return fail("tfx_ln_modulate_split: null pointer");
  return ln_modulate_split(x, out, shift, scale, shift2, scale2, split_row, mod_bstride, rows_per_batch, batch, D, ldx, x_bstride, ldo,
                           o_bstride, eps, S(stream));
}

int tfx_layernorm(const void* x, int64_t ldx, void* out, int64_t ldo, const void* gamma, const void* beta, int64_t rows,
                  int32_t D, float eps, tfx_stream stream) {
  if (!x || !out || !gamma || !beta) return fail("tfx_layernorm: null pointer");
  if (ldx % 8 || ldo % 8) return fail("tfx_layernorm: row strides must be multiples of 8 elements");
  return layernorm_affine(x, out, gamma, beta, rows, D, ldx, ldo, eps, S(stream));
}

int tfx_rmsnorm_rope(void* buf, int64_t ld, int64_t bstride, int32_t q_off, int32_t k_off, int32_t H, int32_t Ntok,
                     int32_t T, int32_t B, const void* wq_img, const void* wk_img, const void* wq_txt,
                     const void* wk_txt, const float* cos_tab, const float* sin_tab, float eps, tfx_stream stream) {
  if (!buf || !wq_img || !wk_img || !wq_txt || !wk_txt || !cos_tab || !sin_tab) return fail("tfx_rmsnorm_rope: null pointer");
  if (ld % 8 || bstride % 8 || q_off % 8 || k_off % 8) return fail("tfx_rmsnorm_rope: offsets/strides must be multiples of 8");
  if (H < 0 || Ntok < 0 || B < 0 || T < 0) return fail("tfx_rmsnorm_rope: negative H, Ntok, B or T");
  if (misaligned16(buf, wq_img, wk_img, wq_txt, wk_txt, cos_tab, sin_tab)) return fail("tfx_rmsnorm_rope: pointers must be 16-byte aligned");
  return rmsnorm_rope(buf, ld, bstride, q_off, k_off, H, Ntok, T, B, wq_img, wk_img, wq_txt, wk_txt, cos_tab, sin_tab,
                      eps, S(stream));
}

int tfx_rmsnorm_rope_batched(void* buf, int64_t ld, int64_t bstride, int32_t q_off, int32_t k_off, int32_t H, int32_t Ntok,
                             int32_t T, int32_t B, const void* wq_img, const void* wk_img, const void* wq_txt,
                             const void* wk_txt, const float* cos_tab, const float* sin_tab, int64_t tab_bstride, float eps,
                             tfx_stream stream) {
  if (!buf || !wq_img || !wk_img || !wq_txt || !wk_txt || !cos_tab || !sin_tab) return fail("tfx_rmsnorm_rope_batched: null pointer");
  if (ld % 8 || bstride % 8 || q_off % 8 || k_off % 8) return fail("tfx_rmsnorm_rope_batched: offsets/strides must be multiples of 8");
  if (H < 0 || Ntok < 0 || B < 0 || T < 0) return fail("tfx_rmsnorm_rope_batched: negative H, Ntok, B or T");
  if (misaligned16(buf, wq_img, wk_img, wq_txt, wk_txt, cos_tab, sin_tab)) return fail("tfx_rmsnorm_rope_batched: pointers must be 16-byte aligned");
  if (tab_bstride < 0 || tab_bstride % 4) return fail("tfx_rmsnorm_rope_batched: tab_bstride must be a non-negative multiple of 4 floats");
  return rmsnorm_rope_tab(buf, ld, bstride, q_off, k_off, H, Ntok, T, B, wq_img, wk_img, wq_txt, wk_txt, cos_tab, sin_tab,
                          tab_bstride, eps, S(stream));
}

int tfx_rmsnorm_rope_qk(void* buf, int64_t ld, int64_t bstride, int32_t q_off, int32_t k_off, int32_t H, int32_t Ntok,
                        int32_t T, int32_t B, const void* wq_img, const void* wk_img, const void* wq_txt,
                        const void* wk_txt, const float* cos_tab, const float* sin_tab, float eps, tfx_stream stream) {
  return tfx_rmsnorm_rope(buf, ld, bstride, q_off, k_off, H, Ntok, T, B, wq_img, wk_img, wq_txt, wk_txt, cos_tab, sin_tab, eps, stream);
}

int tfx_gate_residual(const void* x, int64_t ldx, int64_t x_bstride, const void* gate, int64_t gate_bstride, const void* res,
                      int64_t ldr, int64_t r_bstride, void* out, int64_t ldo, int64_t o_bstride, int32_t rows_per_batch,
                      int32_t batch, int32_t D, tfx_stream stream) {
  if (!x || !gate || !res || !out) return fail("tfx_gate_residual: null pointer");
  if (D <= 0 || D % 8 || (ldx | x_bstride | ldr | r_bstride | ldo | o_bstride | gate_bstride) % 8)
    return fail("tfx_gate_residual: D and every stride must be multiples of 8 elements");
  if (((uintptr_t)x | (uintptr_t)gate | (uintptr_t)res | (uintptr_t)out) % 16) return fail("tfx_gate_residual: pointers must be 16-byte aligned");
  if (rows_per_batch < 0 || batch < 0) return fail("tfx_gate_residual: negative extent");
  return gate_residual(x, ldx, x_bstride, gate, gate_bstride, res, ldr, r_bstride, out, ldo, o_bstride, rows_per_batch, batch, D, S(stream));
}

int tfx_blend_edge_nhwc(const void* a, int64_t a_bstride, int64_t a_tstride, int64_t a_ustride, void* b, int64_t b_bstride,
                        int64_t b_tstride, int64_t b_ustride, int32_t batch, int32_t extent, int32_t len, int32_t C, tfx_stream stream) {
  if (!a || !b) return fail("tfx_blend_edge_nhwc: null pointer");
  if (C <= 0 || C % 8 || (a_bstride | a_tstride | a_ustride | b_bstride | b_tstride | b_ustride) % 8)
    return fail("tfx_blend_edge_nhwc: C and every stride must be multiples of 8 elements");
  if (((uintptr_t)a | (uintptr_t)b) % 16) return fail("tfx_blend_edge_nhwc: pointers must be 16-byte aligned");
  if (batch < 0 || extent < 0 || len < 0) return fail("tfx_blend_edge_nhwc: negative extent");
  return blend_edge(a, a_bstride, a_tstride, a_ustride, b, b_bstride, b_tstride, b_ustride, batch, extent, len, C, S(stream));
}

int tfx_release_scratch(void) { return attention_w4_release(); }

int tfx_attention_mode_counts(int64_t* counts, int32_t n, int32_t reset) {
  if (!counts && n > 0) return fail("tfx_attention_mode_counts: null pointer");
  return attention_mode_counts(counts, n, reset);
}

int tfx_joint_attention(const tfx_attn_args* g, tfx_stream stream) {
  if (!g || !g->q || !g->k || !g->v || !g->o) return fail("tfx_joint_attention: null pointer");
  AttnArgs a;
  a.q = g->q; a.k = g->k; a.v = g->v; a.o = g->o;
  a.ldq = g->ldq; a.ldk = g->ldk; a.ldv = g->ldv; a.ldo = g->ldo;
  a.q_bstride = g->q_bstride; a.k_bstride = g->k_bstride; a.v_bstride = g->v_bstride; a.o_bstride = g->o_bstride;
  a.B = g->B; a.H = g->H; a.N = g->N; a.scale = g->scale; a.score_bound = g->score_bound;
  a.workspace = g->workspace; a.workspace_bytes = g->workspace ? g->workspace_bytes : 0;
  a.seq_len = g->seq_len;
  return joint_attention(a, S(stream));
}

int tfx_euler_step(const void* v, void* x, void* xin, int64_t ldxin, int32_t C, int64_t rows, const float* coef,
                   const int32_t* step_ptr, int32_t step, tfx_stream stream) {
  if (!v || !x || !coef) return fail("tfx_euler_step: null pointer");
  return sched_step(false, v, x, xin, ldxin, C, rows, coef, step_ptr, step, nullptr, S(stream));
}
int tfx_amo_step(const void* v, void* x, void* xin, int64_t ldxin, int32_t C, int64_t rows, const float* coef,
                 const int32_t* step_ptr, int32_t step, const float* noise, tfx_stream stream) {
  if (!v || !x || !coef) return fail("tfx_amo_step: null pointer");
  return sched_step(true, v, x, xin, ldxin, C, rows, coef, step_ptr, step, noise, S(stream));
}

int tfx_multistep_step(const void* v, void* x, void* xin, int64_t ldxin, int32_t C, int64_t rows, const float* coef,
                       const int32_t* step_ptr, int32_t step, void* v_prev, tfx_stream stream) {
  return multistep_step(v, x, xin, ldxin, C, rows, coef, step_ptr, step, v_prev, S(stream));
}

int tfx_known_region_blend(void* x, int64_t ldx, const void* x0, const void* noise, const void* mask, int32_t C, int64_t rows,
                           const float* keep_sigma, const int32_t* step_ptr, int32_t step, void* xin, int64_t ldxin, tfx_stream stream) {
  return known_region_blend(x, ldx, x0, noise, mask, C, rows, keep_sigma, step_ptr, step, xin, ldxin, S(stream));
}

int tfx_cfg_combine(const void* v_neg, const void* v_pos, void* out, int32_t C, int64_t rows, const float* scale, tfx_stream stream) {
  return cfg_combine(v_neg, v_pos, out, C, rows, scale, S(stream));
}
int tfx_x0_predict(const void* x, int64_t ldx, const void* v, void* out, int32_t C, int64_t rows, const float* sigma, const int32_t* step_ptr,
                   int32_t step, tfx_stream stream) {
  return x0_predict(x, ldx, v, out, C, rows, sigma, step_ptr, step, S(stream));
}

int tfx_change_map_blend(void* x, int64_t ldx, const void* x0, const void* noise, const void* hold, const int32_t* cut, int32_t C,
                         int64_t rows, const float* keep_sigma, const int32_t* step_ptr, int32_t step, void* xin, int64_t ldxin,
                         tfx_stream stream) {
  return change_map_blend(x, ldx, x0, noise, hold, cut, C, rows, keep_sigma, step_ptr, step, xin, ldxin, S(stream));
}

int tfx_timestep_embedding(const float* t, void* out, int32_t n, tfx_stream stream) {
  if (!t || !out) return fail("tfx_timestep_embedding: null pointer");
  return timestep_embedding(t, out, n, S(stream));
}
int tfx_silu(const void* a, void* out, int64_t n, tfx_stream stream) {
  if (!a || !out) return fail("tfx_silu: null pointer");
  return silu_bf16(a, out, n, S(stream));
}
int tfx_add(const void* a, const void* b, void* out, int64_t n, tfx_stream stream) {
  if (!a || !b || !out) return fail("tfx_add: null pointer");
  return add_bf16(a, b, out, n, S(stream));
}
int tfx_scatter_cols(const void* src, void* dst, int64_t rows, int32_t C, int64_t ld, int32_t col0, tfx_stream stream) {
  if (!src || !dst) return fail("tfx_scatter_cols: null pointer");
  if (rows < 0) return fail("tfx_scatter_cols: negative row count");
  if (misaligned16(src, dst)) return fail("tfx_scatter_cols: pointers must be 16-byte aligned");
  return scatter_cols(src, dst, rows, C, ld, col0, S(stream));
}
int tfx_copy_rows(const void* src, int64_t src_ld, int64_t src_bstride, void* dst, int64_t dst_ld, int64_t dst_bstride,
                  int32_t rows, int32_t cols, int32_t batch, tfx_stream stream) {
  if (!src || !dst) return fail("tfx_copy_rows: null pointer");
  if (rows < 0 || batch < 0) return fail("tfx_copy_rows: negative row or batch count");
  if (misaligned16(src, dst)) return fail("tfx_copy_rows: pointers must be 16-byte aligned");
  return copy_rows(src, src_ld, src_bstride, dst, dst_ld, dst_bstride, rows, cols, batch, S(stream));
}
int tfx_select_step(const void* table, void* cur, int64_t per_step_elems, int32_t* step_ptr, tfx_stream stream) {
  if (!table || !cur || !step_ptr) return fail("tfx_select_step: null pointer");
  if (per_step_elems < 0) return fail("tfx_select_step: negative per-step size");
  if (misaligned16(table, cur) || (uintptr_t)step_ptr % 4) return fail("tfx_select_step: table and cur must be 16-byte aligned, step_ptr 4-byte");
  return select_step(table, cur, per_step_elems, step_ptr, S(stream));
}
int tfx_advance_step(int32_t* step_ptr, tfx_stream stream) {
  if (!step_ptr) return fail("tfx_advance_step: null pointer");
  return advance_step(step_ptr, S(stream));
}

// tfx_step_cache + a view of hid -> StepCacheArgs, with the checks the three public passes share (and the step path's own use of them)
static int step_cache_args(const char* who, const void* hid, int64_t ldh, int64_t hbs, const tfx_step_cache* c, int32_t rows, int32_t batch,
                           int32_t D, StepCacheArgs& a) {
  if (!hid || !c) return fail("%s: null pointer", who);
  if (!c->x0 || !c->f_prev || !c->h1 || !c->r || !c->partials || !c->metric) return fail("%s: null pointer in tfx_step_cache", who);
  if (rows <= 0 || batch <= 0 || D <= 0) return fail("%s: rows, batch and D must be positive", who);
  if (D % 8) return fail("%s: D must be a multiple of 8", who);
  if (ldh < D || c->ld < D || (ldh | hbs | c->ld | c->bstride) % 8) return fail("%s: row pitches must be >= D, and every stride a multiple of 8 elements", who);
  if (batch > 1 && (hbs < (int64_t)rows * ldh || c->bstride < (int64_t)rows * c->ld)) return fail("%s: batch stride smaller than a sample", who);
  if (((uintptr_t)hid | (uintptr_t)c->x0 | (uintptr_t)c->f_prev | (uintptr_t)c->h1 | (uintptr_t)c->r) % 16 || (uintptr_t)c->partials % 8)
    return fail("%s: pointers must be 16-byte aligned", who);
  if (c->partials_bytes < (int64_t)batch * step_cache_parts((int64_t)rows * (D / 8)) * 8)
    return fail("%s: partials_bytes %lld is too small (2048 bytes per sample serve every shape)", who, (long long)c->partials_bytes);
  a = StepCacheArgs{const_cast<void*>(hid), ldh, hbs, c->x0, c->f_prev, c->h1, c->r, c->ld, c->bstride, c->partials, c->metric, rows, batch, D};
  return 0;
}
int tfx_step_cache_metric(const void* hid, int64_t ldh, int64_t h_bstride, const tfx_step_cache* cache, int32_t rows, int32_t batch,
                          int32_t D, tfx_stream stream) {
  StepCacheArgs a;
  TRY(step_cache_args("tfx_step_cache_metric", hid, ldh, h_bstride, cache, rows, batch, D, a));
  return step_cache_metric(a, S(stream));
}
int tfx_step_cache_store(const void* hid, int64_t ldh, int64_t h_bstride, const tfx_step_cache* cache, int32_t rows, int32_t batch,
                         int32_t D, tfx_stream stream) {
  StepCacheArgs a;
  TRY(step_cache_args("tfx_step_cache_store", hid, ldh, h_bstride, cache, rows, batch, D, a));
  return step_cache_store(a, S(stream));
}
int tfx_step_cache_apply(void* hid, int64_t ldh, int64_t h_bstride, const tfx_step_cache* cache, int32_t rows, int32_t batch, int32_t D,
                         tfx_stream stream) {
  StepCacheArgs a;
  TRY(step_cache_args("tfx_step_cache_apply", hid, ldh, h_bstride, cache, rows, batch, D, a));
  return step_cache_apply(a, S(stream));
}

int tfx_conv3x3_nhwc(const void* x, int32_t B, int32_t inH, int32_t inW, int32_t Cin, const void* w, const void* bias,
                     void* out, int32_t H, int32_t W, int32_t Cout, int32_t stride, int32_t up, int32_t pad_lo,
                     const void* res, const void* zero_page, int variant, tfx_stream stream) {
  if (!x || !w || !out || !zero_page) return fail("tfx_conv3x3_nhwc: null pointer");
  if (up != 1 && up != 2) return fail("tfx_conv3x3_nhwc: up must be 1 or 2");
  GemmArgs a;
  std::memset(&a, 0, sizeof(a));
  // narrow inputs (Cin = 8 / 16 / 32): K = 9 * Cin padded with zero weights to a multiple of 64
  const int K = Cin < 64 ? (9 * Cin + 63) / 64 * 64 : 9 * Cin;
  a.A = x; a.lda = Cin; a.W = w; a.ldw = K; a.bias = bias;
  a.C = out; a.ldc = Cout; a.M = B * H * W; a.N = Cout; a.K = K; a.batch = 1;
  a.epilogue = res ? EPI_BIAS_RES : EPI_BIAS;
  a.res = res; a.ldr = Cout;
  a.conv_cin = Cin; a.conv_inH = inH; a.conv_inW = inW; a.conv_H = H; a.conv_W = W;
  a.conv_stride = stride; a.conv_up_shift = up == 2 ? 1 : 0; a.conv_pad_lo = pad_lo; a.zero_page = zero_page;
  a.conv_kw = 3; a.conv_stride_x = 0; a.qkn_eps = 1e-6f;
  return variant < 0 ? gemm_bf16(a, S(stream)) : gemm_bf16_variant(a, variant, S(stream));
}

int tfx_conv3x3_pair_nhwc(const void* x, int32_t B, int32_t H, int32_t W, int32_t Cin, const void* w_pair, const void* bias_pair,
                          void* out, int32_t Cout, const void* res, const void* zero_page, tfx_stream stream) {
  if (!x || !w_pair || !out || !zero_page) return fail("tfx_conv3x3_pair_nhwc: null pointer");
  if (W % 2 || Cin % 64 || Cout % 4) return fail("tfx_conv3x3_pair_nhwc: W must be even, Cin a multiple of 64, Cout of 4");
  GemmArgs a;
  std::memset(&a, 0, sizeof(a));
  const int K = 12 * Cin;
  a.A = x; a.lda = Cin; a.W = w_pair; a.ldw = K; a.bias = bias_pair;
  a.C = out; a.ldc = 2 * Cout; a.M = B * H * (W / 2); a.N = 2 * Cout; a.K = K; a.batch = 1;
  a.epilogue = res ? EPI_BIAS_RES : EPI_BIAS;
  a.res = res; a.ldr = 2 * Cout;
  a.conv_cin = Cin; a.conv_inH = H; a.conv_inW = W; a.conv_H = H; a.conv_W = W / 2;
  a.conv_stride = 1; a.conv_up_shift = 0; a.conv_pad_lo = 1; a.zero_page = zero_page;
  a.conv_kw = 4; a.conv_stride_x = 2;
  return gemm_bf16(a, S(stream));
}

int tfx_groupnorm_nhwc(const void* x, void* out, const void* gamma, const void* beta, float* workspace, int32_t B,
                       int64_t HW, int32_t C, int32_t groups, float eps, int32_t silu, tfx_stream stream) {
  if (!x || !out || !gamma || !beta || !workspace) return fail("tfx_groupnorm_nhwc: null pointer");
  return groupnorm_silu_nhwc(x, out, gamma, beta, workspace, B, HW, C, groups, eps, silu != 0, S(stream));
}

int tfx_any_negative(const void* x, int32_t dtype, int64_t n, int32_t* flag, tfx_stream stream) {
  if (!x || !flag) return fail("tfx_any_negative: null pointer");
  return any_negative(x, dtype, n, flag, S(stream));
}
int tfx_prep_image(const void* img, int32_t img_dtype, const void* mask, int32_t mask_dtype, void* out, int32_t B, int32_t C,
                   int32_t H, int32_t W, int32_t mask_batch, int32_t norm_mode, int32_t binarize, const int32_t* neg_flag,
                   tfx_stream stream) {
  if (!img || !out) return fail("tfx_prep_image: null pointer");
  return prep_image(img, img_dtype, mask, mask_dtype, out, B, C, H, W, mask_batch, norm_mode, binarize, neg_flag, S(stream));
}
int tfx_compose_canvas(const void* glyph, const void* scene, const void* scene_mask_rgb, void* canvas, void* cmask, int32_t B,
                       int32_t gh, int32_t gw, int32_t sh, int32_t sw, int32_t direction, int32_t mask_rgb, tfx_stream stream) {
  if (!glyph || !scene || !scene_mask_rgb || !canvas || !cmask) return fail("tfx_compose_canvas: null pointer");
  return compose_canvas(glyph, scene, scene_mask_rgb, canvas, cmask, B, gh, gw, sh, sw, direction, mask_rgb, S(stream));
}
int tfx_rgb_to_grey_u8(const void* rgb, void* out, int64_t pixels, tfx_stream stream) {
  if (!rgb || !out) return fail("tfx_rgb_to_grey_u8: null pointer");
  return rgb_to_grey(rgb, out, pixels, S(stream));
}
int tfx_resample_u8(const void* in, void* out, const int32_t* bounds, const int32_t* coeffs, int32_t ksize, int64_t outer,
                    int32_t in_len, int32_t out_len, int32_t inner, tfx_stream stream) {
  if (!in || !out || !bounds || !coeffs) return fail("tfx_resample_u8: null pointer");
  return resample_u8(in, out, bounds, coeffs, ksize, outer, in_len, out_len, inner, S(stream));
}
int tfx_mask_dilate_u8(const void* in, void* out, void* tmp, int32_t B, int32_t H, int32_t W, int32_t radius, tfx_stream stream) {
  if (!in || !out || !tmp) return fail("tfx_mask_dilate_u8: null pointer");
  return mask_dilate_u8(in, out, tmp, B, H, W, radius, S(stream));
}
int tfx_mask_feather_u8(const void* in, void* out, void* tmp, int32_t B, int32_t H, int32_t W, int32_t radius, tfx_stream stream) {
  if (!in || !out || !tmp) return fail("tfx_mask_feather_u8: null pointer");
  return mask_feather_u8(in, out, tmp, B, H, W, radius, S(stream));
}
int tfx_overlay_u8(const void* orig, const void* edit, const void* alpha, void* out, int32_t B, int32_t H, int32_t W, int32_t C,
                   tfx_stream stream) {
  if (!orig || !edit || !alpha || !out) return fail("tfx_overlay_u8: null pointer");
  return overlay_u8(orig, edit, alpha, out, B, H, W, C, S(stream));
}
static_assert(TFX_MASKED_MOMENTS_SCRATCH_BYTES == MASKED_MOMENTS_SCRATCH_BYTES, "the header's scratch bound is the kernels'");
int tfx_masked_moments_u8(const void* a, const void* b, const void* weight, void* out, void* scratch, int64_t scratch_bytes, int32_t B,
                          int32_t H, int32_t W, int32_t C, tfx_stream stream) {
  if (!a || !b || !weight || !out || !scratch) return fail("tfx_masked_moments_u8: null pointer");
  return masked_moments_u8(a, b, weight, out, scratch, scratch_bytes, B, H, W, C, S(stream));
}
int tfx_overlay_lut_u8(const void* orig, const void* edit, const void* alpha, const void* lut, void* out, int32_t B, int32_t H, int32_t W,
                       int32_t C, tfx_stream stream) {
  if (!orig || !edit || !alpha || !lut || !out) return fail("tfx_overlay_lut_u8: null pointer");
  return overlay_lut_u8(orig, edit, alpha, lut, out, B, H, W, C, S(stream));
}
int64_t tfx_seamless_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t C) { return seamless_workspace_bytes(B, H, W, C); }
int tfx_seamless_overlay_u8(const void* orig, const void* ref, const void* edit, const void* alpha, const void* covered, const void* lut,
                            void* out, void* workspace, int64_t workspace_bytes, int32_t B, int32_t H, int32_t W, int32_t C, int32_t smooth,
                            int32_t max_shift, tfx_stream stream) {
  if (!orig || !ref || !edit || !alpha || !out || !workspace) return fail("tfx_seamless_overlay_u8: null pointer");
  return seamless_overlay_u8(orig, ref, edit, alpha, covered, lut, out, workspace, workspace_bytes, B, H, W, C, smooth, max_shift, S(stream));
}
int tfx_highpass_hist_u8(const void* img, const void* sel, int32_t lo, int32_t hi, void* out, int32_t B, int32_t H, int32_t W, int32_t C,
                         tfx_stream stream) {
  if (!img || !sel || !out) return fail("tfx_highpass_hist_u8: null pointer");
  return highpass_hist_u8(img, sel, lo, hi, out, B, H, W, C, S(stream));
}
int tfx_grain_u8(const void* img, const void* alpha, const int32_t* gain, const int32_t* origin, uint32_t seed, void* out, int32_t B,
                 int32_t H, int32_t W, int32_t C, tfx_stream stream) {
  if (!img || !alpha || !gain || !out) return fail("tfx_grain_u8: null pointer");
  return grain_u8(img, alpha, gain, origin, seed, out, B, H, W, C, S(stream));
}
int tfx_highpass_hist_step_u8(const void* img, const void* sel, int32_t lo, int32_t hi, int32_t step, void* out, int32_t B, int32_t H, int32_t W,
                              int32_t C, tfx_stream stream) {
  if (!img || !sel || !out) return fail("tfx_highpass_hist_step_u8: null pointer");
  return highpass_hist_step_u8(img, sel, lo, hi, step, out, B, H, W, C, S(stream));
}
int tfx_grain_shaped_u8(const void* img, const void* alpha, const int32_t* gain, const int32_t* shape, const int32_t* origin, uint32_t seed,
                        void* out, int32_t B, int32_t H, int32_t W, int32_t C, tfx_stream stream) {
  if (!img || !alpha || !gain || !shape || !out) return fail("tfx_grain_shaped_u8: null pointer");
  return grain_shaped_u8(img, alpha, gain, shape, origin, seed, out, B, H, W, C, S(stream));
}
int tfx_change_metric_u8(const void* a, const void* b, void* out, int32_t B, int32_t H, int32_t W, int32_t C, tfx_stream stream) {
  if (!a || !b || !out) return fail("tfx_change_metric_u8: null pointer");
  return change_metric_u8(a, b, out, B, H, W, C, S(stream));
}
int64_t tfx_hysteresis_workspace_bytes(int32_t B, int32_t H, int32_t W) { return hysteresis_workspace_bytes(B, H, W); }
int tfx_hysteresis_u8(const void* m, void* out, int32_t lo, int32_t hi, void* workspace, int64_t workspace_bytes, int32_t* rounds, int32_t B,
                      int32_t H, int32_t W, tfx_stream stream) {
  if (!m || !out || !workspace) return fail("tfx_hysteresis_u8: null pointer");
  return hysteresis_u8(m, out, lo, hi, workspace, workspace_bytes, rounds, B, H, W, S(stream));
}
int tfx_warp_affine_u8(const void* in, void* out, void* coverage, int32_t B, int32_t H, int32_t W, int32_t C, int32_t out_h, int32_t out_w,
                       const int64_t* m, const int16_t* taps, tfx_stream stream) {
  if (!in || !out || !m || !taps) return fail("tfx_warp_affine_u8: null pointer");
  return warp_affine_u8(in, out, coverage, B, H, W, C, out_h, out_w, m, taps, S(stream));
}
int tfx_warp_perspective_u8(const void* in, void* out, void* coverage, int32_t B, int32_t H, int32_t W, int32_t C, int32_t out_h,
                            int32_t out_w, const int64_t* m, const int16_t* taps, tfx_stream stream) {
  if (!in || !out || !m || !taps) return fail("tfx_warp_perspective_u8: null pointer");
  return warp_perspective_u8(in, out, coverage, B, H, W, C, out_h, out_w, m, taps, S(stream));
}
int tfx_warp_grid_u8(const void* in, void* out, void* coverage, int32_t B, int32_t H, int32_t W, int32_t C, int32_t out_h, int32_t out_w,
                     const int64_t* grid, int32_t shift, const int16_t* taps, tfx_stream stream) {
  if (!in || !out || !grid || !taps) return fail("tfx_warp_grid_u8: null pointer");
  return warp_grid_u8(in, out, coverage, B, H, W, C, out_h, out_w, grid, shift, taps, S(stream));
}
int tfx_warp_affine_gather_u8(const void* images, void* out, int64_t out_bytes, const int64_t* table, int32_t n, int32_t* refused, int32_t B,
                              int32_t H, int32_t W, int32_t C, int32_t blocks_per_crop, const int16_t* taps, tfx_stream stream) {
  if (!images || !out || !table || !refused || !taps) return fail("tfx_warp_affine_gather_u8: null pointer");
  return warp_affine_gather_u8(images, out, out_bytes, table, n, refused, B, H, W, C, blocks_per_crop, taps, S(stream));
}
int tfx_change_map_pack(const void* map_u8, void* hold, int32_t B, int32_t H, int32_t W, int32_t mode, int32_t grow, tfx_stream stream) {
  return change_map_pack(map_u8, hold, B, H, W, mode, grow, S(stream));
}
int tfx_keep_mask_pack(const void* mask_u8, void* out, int32_t B, int32_t H, int32_t W, int32_t C, int32_t mode, int32_t grow,
                       tfx_stream stream) {
  return keep_mask_pack(mask_u8, out, B, H, W, C, mode, grow, S(stream));
}

int tfx_pack_mask(const void* mask, int32_t mask_dtype, void* out, int32_t B, int32_t H, int32_t W, int32_t mask_batch,
                  int32_t binarize, int64_t ld, int32_t col0, tfx_stream stream) {
  if (!mask || !out) return fail("tfx_pack_mask: null pointer");
  return pack_mask(mask, mask_dtype, out, B, H, W, mask_batch, binarize, ld, col0, S(stream));
}
int tfx_vae_sample_pack(const void* moments, const void* eps, int32_t eps_dtype, void* out, int32_t B, int32_t h, int32_t w,
                        int32_t L, float shift, float scale, int64_t ld, int32_t col0, tfx_stream stream) {
  if (!moments || !out) return fail("tfx_vae_sample_pack: null pointer");
  return sample_pack(moments, eps, eps_dtype, out, B, h, w, L, shift, scale, ld, col0, S(stream));
}
int tfx_unpack_latents(const void* latents, int64_t ld, void* out, int32_t B, int32_t h, int32_t w, int32_t L, float shift,
                       float scale, tfx_stream stream) {
  if (!latents || !out) return fail("tfx_unpack_latents: null pointer");
  if (L > 0 && ld < 4 * (int64_t)L) return fail("tfx_unpack_latents: ld must be >= 4 L, the columns a token row holds");
  return unpack_latents(latents, ld, out, B, h, w, L, shift, scale, S(stream));
}
int tfx_postprocess(const void* x, void* out, int32_t B, int32_t H, int32_t W, int32_t Cs, int32_t C, int32_t mode, int32_t denorm,
                    int32_t y0, int32_t x0, int32_t Hc, int32_t Wc, tfx_stream stream) {
  if (!x || !out) return fail("tfx_postprocess: null pointer");
  return postprocess(x, out, B, H, W, Cs, C, mode, denorm, y0, x0, Hc, Wc, S(stream));
}
int tfx_transpose(const void* in, int64_t ldi, int64_t in_bstride, void* out, int64_t ldo, int64_t out_bstride, int32_t N,
                  int32_t C, int32_t batch, tfx_stream stream) {
  if (!in || !out) return fail("tfx_transpose: null pointer");
  if (batch > 65535) return fail("tfx_transpose: batch must be <= 65535 (gridDim.z)");
  if (N > 0 && C > 0 && (ldi < C || ldo < N)) return fail("tfx_transpose: ldi must be >= C and ldo >= N");
  return transpose_bf16(in, ldi, in_bstride, out, ldo, out_bstride, N, C, batch, S(stream));
}
int tfx_row_softmax(const float* s, int64_t lds, void* p, int64_t ldp, int32_t rows, int32_t N, float scale, tfx_stream stream) {
  if (!s || !p) return fail("tfx_row_softmax: null pointer");
  return row_softmax(s, lds, p, ldp, rows, N, scale, S(stream));
}

int tfx_attention64(const tfx_attn_args* g, const float* rel_bias, int32_t causal, tfx_stream stream) {
  if (!g || !g->q || !g->k || !g->v || !g->o) return fail("tfx_attention64: null pointer");
  AttnArgs a;
  a.q = g->q; a.k = g->k; a.v = g->v; a.o = g->o;
  a.ldq = g->ldq; a.ldk = g->ldk; a.ldv = g->ldv; a.ldo = g->ldo;
  a.q_bstride = g->q_bstride; a.k_bstride = g->k_bstride; a.v_bstride = g->v_bstride; a.o_bstride = g->o_bstride;
  a.B = g->B; a.H = g->H; a.N = g->N; a.scale = g->scale;
  return attention64(a, rel_bias, causal, S(stream));
}
int tfx_rmsnorm(const void* x, int32_t x_dtype, int64_t ldx, const void* w, void* out, int64_t ldo, int64_t rows, int32_t D,
                float eps, tfx_stream stream) {
  if (!x || !w || !out) return fail("tfx_rmsnorm: null pointer");
  return rmsnorm(x, x_dtype, ldx, w, out, ldo, rows, D, eps, S(stream));
}
int tfx_gather_rows(const void* table, const int64_t* ids, void* out, int64_t n, int32_t D, int64_t vocab, tfx_stream stream) {
  if (!table || !ids || !out) return fail("tfx_gather_rows: null pointer");
  return gather_rows(table, ids, out, n, D, vocab, S(stream));
}
int tfx_add_into_f32(float* x, const void* y, int64_t n, int32_t mode, tfx_stream stream) {
  if (!x || !y) return fail("tfx_add_into_f32: null pointer");
  return add_into_f32(x, y, n, mode, S(stream));
}
int tfx_mul_act(const void* a, int64_t lda, const void* b, int64_t ldb, void* out, int64_t ldo, int64_t rows, int32_t cols,
                int32_t mode, tfx_stream stream) {
  if (!a || !out) return fail("tfx_mul_act: null pointer");
  return mul_act(a, lda, b, ldb, out, ldo, rows, cols, mode, S(stream));
}

int tfx_set_option(const char* name, int value) {
  if (!name) return fail("tfx_set_option: null name");
  if (!std::strcmp(name, "attention_waves")) {
    if (value == 0) { set_attention_waves(0); return 0; }     // back to the library default and its size heuristic
    if (value != 4 && value != 8 && value != 9 && value != 10 && value != 12 && value != 16 && value != 20 && !(value >= 30 && value <= 34) && value != 40)
      return fail("tfx_set_option: attention_waves must be 4, 8, 9 (128 keys per barrier), 10 / 12 (matrix-pipe softmax, 8 / 4 waves), 16 (ping-pong), 20 (half-tile pipelined), 30 .. 34 (one wave per SIMD, 32x32x16 MFMA: 30 bookkeeping on the matrix pipe -- or no reference at all when the call carries an admissible score bound -- / 31 row sums on the VALU / 32 = 31 + lazy reference offset / 33 = 30 + lazy reference offset / 34 = no reference with a score bound, else 33) or 40 (one wave per SIMD, 16x16x32 MFMA)");
#ifndef TFX_BENCH
    if (value != 30 && value != 34)
      return fail("tfx_set_option: attention_waves %d is a bench-only kernel (libtextflux_hip_bench.so, `make bench`); the product library "
                  "carries 30 (the default) and 34", value);
#endif
    set_attention_waves(value);
    return 0;
  }
  if (!std::strcmp(name, "gemm_group_m")) { set_gemm_group_m(value); return 0; }
  if (!std::strcmp(name, "attention_tail_split")) { set_attention_tail_split(value); return 0; }
  if (!std::strcmp(name, "attention_use_bound")) { set_attention_use_bound(value); return 0; }
  if (!std::strcmp(name, "attention_persistent")) { set_attention_persistent(value); return 0; }
  if (!std::strcmp(name, "attention_streamk")) { set_attention_streamk(value); return 0; }
  if (!std::strcmp(name, "gemm_place")) { set_gemm_place(value); return 0; }
  if (!std::strcmp(name, "gemm_waves")) {
#ifndef TFX_BENCH
    if (value != 8 && value != 0) return fail("tfx_set_option: gemm_waves 4 (gemm4w_kernel) is bench-only (libtextflux_hip_bench.so, `make bench`)");
#endif
    set_gemm_waves(value);
    return 0;
  }
  if (!std::strcmp(name, "gemm_group_streams")) { set_gemm_group_streams(value); return 0; }
  if (!std::strcmp(name, "ln_joint")) { set_ln_joint(value); return 0; }
  if (!std::strcmp(name, "ln_prefetch")) { set_ln_prefetch(value); return 0; }
  if (!std::strcmp(name, "fp8_fuse_qkn")) { set_fp8_fuse_qkn(value); return 0; }
  if (!std::strcmp(name, "gemm_splitk")) { set_gemm_splitk(value); return 0; }
  if (!std::strcmp(name, "attention_ablation")) { set_attention_ablation(value); return 0; }  // bench-only
  return fail("tfx_set_option: unknown option '%s'", name);
}

int tfx_debug_attention_timing(void* buf) { set_attention_debug(buf); return 0; }

int tfx_mfma_peak_probe(const void* operands, int64_t operand_bytes, int32_t fp8, int32_t ktiles, double* flops, tfx_stream stream) {
  return mfma_peak_probe(operands, operand_bytes, fp8, ktiles, flops, S(stream));
}

int tfx_prof_enable(int on) { prof_enable(on); return 0; }
int tfx_prof_collect(int kind, double* total_ms, double* total_flops, int* launches) {
  if (kind < 0 || kind > 2) return fail("tfx_prof_collect: kind must be 0 (gemm), 1 (attention) or 2 (fp8 gemm)");
  return prof_collect(kind, total_ms, total_flops, launches);
}

static inline int64_t align256(int64_t v) { return (v + 255) & ~(int64_t)255; }
int tfx_workspace_layout(int32_t B, int32_t Sn, int32_t T, int32_t D, int32_t flags, int64_t* off, int64_t* gemm_ws_bytes) {
  if (B <= 0 || Sn <= 0 || T < 0 || D <= 0 || !off) return fail("tfx_workspace_layout: bad arguments");
  const int64_t N = (int64_t)Sn + T, hid = align256(B * N * D * 2), y = align256(B * N * 7 * (int64_t)D * 2);
  const bool fp8 = (flags & 4) != 0;
  const int64_t q8 = fp8 ? align256(B * N * 5 * (int64_t)D) : 0, q8s = fp8 ? align256(B * N * 4) : 0, gws = 128ll << 20;
  int64_t o = 0;
  off[0] = o; o += hid;
  off[1] = o; o += hid;
  off[2] = o; o += y;
  off[3] = fp8 ? o : -1; o += q8;
  off[4] = fp8 ? o : -1; o += q8s;
  off[5] = o;
  if (flags & 8) {   // runtime LoRA adapters: the T scratch behind everything else (tfx_dit_desc.lora_t_xn / lora_t_y)
    o += gws;
    off[6] = o; o += (D >= 1024 ? 1 : 4) * hid;
    off[7] = o;
  }
  if (gemm_ws_bytes) *gemm_ws_bytes = gws;
  return 0;
}
int64_t tfx_workspace_bytes(int32_t B, int32_t Sn, int32_t T, int32_t D, int32_t flags) {
  int64_t off[8], gws = 0;
  if (tfx_workspace_layout(B, Sn, T, D, flags, off, &gws)) return -1;
  if (flags & 8) return off[7] + ((off[3] >= 0 ? off[3] : off[5]) - off[2]);   // ... + lora_t_y, the size of y
  return off[5] + gws;
}

namespace {
struct StepGraph { hipGraph_t graph; hipGraphExec_t exec; };

int step_check_sampler(const tfx_step_desc* s) {
  if (!s) return fail("tfx_dit_step: null descriptor");
  if (!s->mod_table || !s->mod_cur || !s->step_ptr) return fail("tfx_dit_step: null pointer in descriptor");
  if (s->dit.mod != s->mod_cur) return fail("tfx_dit_step: dit.mod must point at mod_cur (the rows the step selects)");
  if (s->sampler < 0 || s->sampler > 2) return fail("tfx_dit_step: sampler must be 0 (Euler), 1 (AMO) or 2 (Euler fused into proj_out)");
  if (s->dit.seq_len && s->sampler != 2)
    return fail("tfx_dit_step: dit.seq_len (mixed-geometry batch) needs sampler 2: only the fused Euler form carries per-sample coefficients");
  if (s->sampler == 2) {
    const char* g = (const char*)s->dit.euler_gate;
    if (!g || g < (const char*)s->mod_cur || g >= (const char*)s->mod_cur + s->mod_step_elems * 2)
      return fail("tfx_dit_step: sampler 2 needs dit.euler_gate inside mod_cur (the step's dsigma row is selected with its modulation rows)");
    return 0;
  }
  if (s->dit.euler_gate) return fail("tfx_dit_step: dit.euler_gate is set but sampler is not 2");
  if (!s->latents || !s->coef) return fail("tfx_dit_step: null pointer in descriptor");
  if (s->sampler == 1 && !s->noise) return fail("tfx_dit_step: the AMO sampler needs a noise buffer");
  if (!s->dit.out) return fail("tfx_dit_step: dit.out is null");
  return 0;
}

// the image rows of the joint stream as the step cache's passes see them
int step_cache_view(const tfx_step_desc& s, StepCacheArgs& a) {
  const tfx_dit_desc& d = s.dit;
  if (!d.hid) return fail("tfx_dit_step: null buffer in descriptor");
  const int64_t N = (int64_t)d.S + d.T;
  return step_cache_args("tfx_dit_step (step cache)", (const uint16_t*)d.hid + (int64_t)d.T * d.D, d.D, N * d.D, s.cache, d.S, d.B, d.D, a);
}

int step_check(const tfx_step_desc* s) {
  TRY(step_check_sampler(s));
  if (s->phase < 0 || s->phase > 3) return fail("tfx_dit_step: phase must be 0 (whole step), 1 (head), 2 (computed tail) or 3 (cached tail)");
  if (s->phase && !s->cache) return fail("tfx_dit_step: phase %d needs a step cache (tfx_step_desc.cache is null)", s->phase);
  if (!s->cache) return 0;
  const tfx_dit_desc& d = s->dit;
  if (d.seq_len) return fail("tfx_dit_step: the step cache cannot serve a mixed-geometry batch (dit.seq_len): padded rows may hold NaN and would poison the metric's sums");
  const int nblk = d.n_double + d.n_single;
  if (d.first_block > 0 || (d.last_block >= 0 && d.last_block < nblk) || (d.flags & ~4))
    return fail("tfx_dit_step: the step cache needs the whole forward (first_block 0, last_block -1, flags 0 or 4); the phases choose the block ranges");
  if (nblk < 2) return fail("tfx_dit_step: the step cache needs at least 2 blocks (n_double + n_single = %d)", nblk);
  StepCacheArgs a;
  return step_cache_view(*s, a);
}

// the scheduler update behind the final projection and the cursor advance: the end of a whole step and of both tails.
// ex.v_prev: the multistep history buffer -- the second-order update then stands where sampler 0 launches Euler's.  ex.keep_*: the
// known-region blend, behind the update and in front of the step cache's store pass and the cursor advance (it reads the cursor).
// ch: the change-map blend in the same place, its mask decided on the device from hold and cut (keep_mask is then NULL).
// cfg: true CFG -- the batch is [negative; positive], the two halves of dit.out are combined into the first in front of the update,
// the update and the blend run on the first half's rows, and the new latents are copied into the second half of xin behind them
int step_finish(const tfx_step_desc& s, hipStream_t st, const StepCacheArgs* store, const tfx_step_extra& ex, const tfx_step_change* ch,
                const tfx_step_cfg* cfg) {
  const tfx_dit_desc& d = s.dit;
  const int Bx = cfg ? d.B / 2 : d.B;                           // samples of the loop state
  const int64_t rows = (int64_t)Bx * d.S;
  void* xin = const_cast<void*>(d.xin);
  if (cfg) TRY(cfg_combine(d.out, (const uint16_t*)d.out + rows * d.out_channels, d.out, d.out_channels, rows, cfg->scale, st));
  if (ex.v_prev) {
    TRY(multistep_step(d.out, s.latents, xin, d.in_channels, d.out_channels, rows, s.coef, s.step_ptr, 0, ex.v_prev, st));
  } else if (s.sampler != 2) {                                  // sampler 2: the update happened in proj_out's epilogue
    TRY(sched_step(s.sampler == 1, d.out, s.latents, xin, d.in_channels, d.out_channels, rows, s.coef, s.step_ptr, 0, s.noise, st));
  }
  if (ch || ex.keep_mask) {
    const bool fused = s.sampler == 2;                          // the fused Euler form keeps the latents in xin[:, :out_channels]
    void* x = fused ? xin : s.latents;
    const int64_t ldx = fused ? d.in_channels : d.out_channels;
    void* mirror = fused ? nullptr : xin;
    const int64_t ldmirror = fused ? 0 : d.in_channels;
    if (ch)
      TRY(change_map_blend(x, ldx, ex.keep_x0, ex.keep_noise, ch->hold, ch->cut, d.out_channels, rows, ex.keep_sigma, s.step_ptr, 0, mirror,
                           ldmirror, st));
    else
      TRY(known_region_blend(x, ldx, ex.keep_x0, ex.keep_noise, ex.keep_mask, d.out_channels, rows, ex.keep_sigma, s.step_ptr, 0, mirror,
                             ldmirror, st));
  }
  if (cfg)                                                      // sample B + b of the x_embedder input mirrors sample b
    TRY(copy_rows(xin, d.in_channels, (int64_t)d.S * d.in_channels, (uint16_t*)xin + rows * d.in_channels, d.in_channels,
                  (int64_t)d.S * d.in_channels, d.S, d.out_channels, Bx, st));
  if (store) TRY(step_cache_store(*store, st));
  return advance_step(s.step_ptr, st);
}

// blocks [first, last) of the step's forward; flags: bit 0 no embedders, bit 1 no norm_out / proj_out (the fp8 bit rides along)
int step_forward(const tfx_step_desc& s, int first, int last, int flags, hipStream_t st) {
  tfx_dit_desc d = s.dit;
  d.first_block = first; d.last_block = last; d.flags = (s.dit.flags & 4) | flags;
  return tfx_dit_forward(&d, (tfx_stream)st);
}

int step_enqueue(const tfx_step_desc& s, hipStream_t st, const tfx_step_extra& ex, const tfx_step_change* ch, const tfx_step_cfg* cfg) {
  if (s.phase == 0) {
    TRY(select_step(s.mod_table, s.mod_cur, s.mod_step_elems, s.step_ptr, st));
    TRY(tfx_dit_forward(&s.dit, (tfx_stream)st));
    return step_finish(s, st, nullptr, ex, ch, cfg);
  }
  StepCacheArgs a;
  TRY(step_cache_view(s, a));
  const int nblk = s.dit.n_double + s.dit.n_single;
  switch (s.phase) {
    case 1:   // head: what a whole step issues up to and including block 0, with x0 taken between the embedders and the block
      TRY(select_step(s.mod_table, s.mod_cur, s.mod_step_elems, s.step_ptr, st));
      TRY(step_forward(s, 0, 0, 2, st));
      TRY(step_cache_save(a, st));
      TRY(step_forward(s, 0, 1, 3, st));
      return step_cache_metric(a, st);
    case 2:   // computed tail: the rest of the whole step, then r and f_prev
      TRY(step_forward(s, 1, -1, 1, st));
      return step_finish(s, st, &a, ex, ch, nullptr);
    default:  // 3, cached tail: the last computed step's residual stands in for blocks [1, n)
      TRY(step_cache_apply(a, st));
      TRY(step_forward(s, nblk, nblk, 1, st));
      return step_finish(s, st, nullptr, ex, ch, nullptr);
  }
}

// the multistep entry points take sampler 0's descriptor (latents, coef, dit.out; neither seq_len nor euler_gate) and the history
int step_check_multistep(const tfx_step_desc* s, const void* v_prev) {
  TRY(step_check(s));
  if (s->sampler != 0) return fail("tfx_dit_step (multistep): sampler must be 0: the second-order update stands where the unfused Euler launch does");
  if (!v_prev) return fail("tfx_dit_step (multistep): the history buffer v_prev is null");
  if (v_prev == s->latents || v_prev == s->dit.out) return fail("tfx_dit_step (multistep): v_prev must not alias latents or dit.out");
  return 0;
}

// What every step entry point checks.  ex: the history and the blend's buffers, all NULL for the plain step; need_history: the
// *_multistep entry points, which refuse a NULL v_prev.  ch NULL (`who` "ex"): keep_* all set, the known-region blend, or all NULL.
// ch set (`who` "ex2"), the change-map blend: keep_x0 / keep_noise / keep_sigma, hold and cut set, keep_mask NULL.  Neither blend
// with dit.seq_len, and nothing a blend reads may alias a buffer the step writes.
// cfg set (`who` "ex3"), true CFG: sampler 0 or 1, phase 0, an even dit.B, no dit.seq_len, and a scale outside what the step writes;
// latents, v_prev and the blends' buffers then have dit.B / 2 samples.
int step_check_cfg(const tfx_step_desc* s, const tfx_step_extra* ex, const tfx_step_cfg* cfg) {
  const tfx_dit_desc& d = s->dit;
  if (!cfg->scale) return fail("tfx_dit_step (ex3): cfg->scale is null");
  if ((uintptr_t)cfg->scale & 3) return fail("tfx_dit_step (ex3): cfg->scale must be 4-byte aligned");
  if (s->sampler == 2)
    return fail("tfx_dit_step (ex3): true CFG cannot run with sampler 2: the fused Euler epilogue updates each half of the batch on its own");
  if (d.seq_len) return fail("tfx_dit_step (ex3): true CFG cannot serve a mixed-geometry batch (dit.seq_len)");
  if (s->phase != 0) return fail("tfx_dit_step (ex3): true CFG runs whole steps only (phase 0), not the step cache's phase %d", s->phase);
  if (d.B < 2 || d.B % 2) return fail("tfx_dit_step (ex3): true CFG needs an even dit.B (the batch is [negative; positive]), got %d", d.B);
  if (!d.xin) return fail("tfx_dit_step (ex3): dit.xin is null");
  const int64_t N = (int64_t)d.S + d.T, half = (int64_t)(d.B / 2) * d.S * d.out_channels * 2, tok = (int64_t)d.B * N * d.D * 2;
  struct Span { const void* p; int64_t bytes; };
  const Span written[9] = {{s->latents, half}, {d.out, 2 * half}, {d.xin, (int64_t)d.B * d.S * d.in_channels * 2}, {ex->v_prev, half},
                           {s->mod_cur, s->mod_step_elems * 2}, {s->step_ptr, 4}, {d.hid, tok}, {d.xn, tok}, {d.y, 7 * tok}};
  const char* p = (const char*)cfg->scale;
  for (const Span& w : written) {
    const char* q = (const char*)w.p;
    if (q && p < q + w.bytes && q < p + 4) return fail("tfx_dit_step (ex3): cfg->scale must not lie in a buffer the step writes");
  }
  return 0;
}

int step_check_extra(const tfx_step_desc* s, const tfx_step_extra* ex, const tfx_step_change* ch, const tfx_step_cfg* cfg, const char* who,
                     bool need_history) {
  if (!ex)
    return ch ? fail("tfx_dit_step (ex2): null tfx_step_extra: the change-map blend reads keep_x0, keep_noise and keep_sigma from it")
              : fail("tfx_dit_step (ex): null tfx_step_extra (tfx_dit_step_run / tfx_dit_step_capture take none)");
  if (ex->v_prev || need_history) TRY(step_check_multistep(s, ex->v_prev)); else TRY(step_check(s));
  if (cfg) TRY(step_check_cfg(s, ex, cfg));
  if (ch) {
    if (!ch->hold || !ch->cut) return fail("tfx_dit_step (ex2): change->hold and change->cut must both be set");
    if (!ex->keep_x0 || !ex->keep_noise || !ex->keep_sigma) return fail("tfx_dit_step (ex2): with change, keep_x0, keep_noise and keep_sigma must be set");
    if (ex->keep_mask) return fail("tfx_dit_step (ex2): with change, keep_mask must be NULL: the mask is decided on the device from hold and cut");
  } else {
    const int set = (ex->keep_x0 != nullptr) + (ex->keep_noise != nullptr) + (ex->keep_mask != nullptr) + (ex->keep_sigma != nullptr);
    if (set == 0) return 0;
    if (set != 4) return fail("tfx_dit_step (ex): keep_x0, keep_noise, keep_mask and keep_sigma must be all set or all NULL");
  }
  const tfx_dit_desc& d = s->dit;
  if (d.seq_len)
    return fail("tfx_dit_step (%s): the %s blend cannot serve a mixed-geometry batch (dit.seq_len): its buffers are [B * S, C] without padding rows",
                who, ch ? "change-map" : "known-region");
  if (!d.xin) return fail("tfx_dit_step (%s): dit.xin is null", who);
  const int64_t all = (int64_t)d.B * d.S, rows = cfg ? all / 2 : all, kb = rows * d.out_channels * 2;   // true CFG: the loop state is half the batch
  struct Span { const void* p; int64_t bytes; };
  const Span written[4] = {{s->latents, kb}, {d.out, all * d.out_channels * 2}, {d.xin, all * d.in_channels * 2}, {ex->v_prev, kb}};
  const Span read[6] = {{ex->keep_x0, kb}, {ex->keep_noise, kb}, {ex->keep_mask, kb}, {ex->keep_sigma, 4},
                        {ch ? ch->hold : nullptr, rows * 4}, {ch ? ch->cut : nullptr, 4}};
  for (const Span& r : read) {
    const char* p = (const char*)r.p;
    for (const Span& w : written) {
      const char* q = (const char*)w.p;
      if (p && q && (p == q || (p < q + w.bytes && q < p + r.bytes)))
        return fail("tfx_dit_step (%s): %s must not alias latents, dit.out, dit.xin or v_prev", who,
                    ch ? "keep_x0, keep_noise, keep_sigma, hold and cut" : "keep_x0, keep_noise, keep_mask and keep_sigma");
    }
  }
  return 0;
}

int step_capture(const tfx_step_desc* s, const tfx_step_extra& ex, const tfx_step_change* ch, const tfx_step_cfg* cfg, tfx_stream stream,
                 tfx_graph* out) {
  if (!out) return fail("tfx_dit_step_capture: null output handle");
  if (!stream) return fail("tfx_dit_step_capture: the NULL stream cannot be captured; pass a created stream");
  hipStream_t st = S(stream);
  (void)attention_w4_prepare(st);   // the attention kernel's scratch (of this stream) cannot be allocated inside a capture
  hipError_t e = hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal);
  if (e != hipSuccess) return fail("tfx_dit_step_capture: hipStreamBeginCapture: %s", hipGetErrorString(e));
  const int rc = step_enqueue(*s, st, ex, ch, cfg);
  hipGraph_t g = nullptr;
  e = hipStreamEndCapture(st, &g);
  if (rc) { if (g) (void)hipGraphDestroy(g); return rc; }    // last error already set by the failing launcher
  if (e != hipSuccess || !g) return fail("tfx_dit_step_capture: hipStreamEndCapture: %s", hipGetErrorString(e));
  hipGraphExec_t x = nullptr;
  e = hipGraphInstantiate(&x, g, nullptr, nullptr, 0);
  if (e != hipSuccess) { (void)hipGraphDestroy(g); return fail("tfx_dit_step_capture: hipGraphInstantiate: %s", hipGetErrorString(e)); }
  *out = new StepGraph{g, x};
  return 0;
}

// Every step entry point: the checks, then the step on the stream, or (CAPTURE) captured from it into *graph_out
enum { RUN = 0, CAPTURE = 1, NEED_HISTORY = 2 };
int step_entry(const tfx_step_desc* s, const tfx_step_extra* ex, const tfx_step_change* ch, const tfx_step_cfg* cfg, tfx_stream stream,
               tfx_graph* graph_out, int how) {
  TRY(step_check_extra(s, ex, ch, cfg, cfg ? "ex3" : ch ? "ex2" : "ex", (how & NEED_HISTORY) != 0));
  return how & CAPTURE ? step_capture(s, *ex, ch, cfg, stream, graph_out) : step_enqueue(*s, S(stream), *ex, ch, cfg);
}

const tfx_step_extra kPlain{};   // the plain step's tfx_step_extra: no history, no blend

// the *_multistep entry points' tfx_step_extra: the history alone
tfx_step_extra history(void* v_prev) {
  tfx_step_extra ex{};
  ex.v_prev = v_prev;
  return ex;
}
}  // namespace

int tfx_dit_step_run(const tfx_step_desc* s, tfx_stream stream) { return step_entry(s, &kPlain, nullptr, nullptr, stream, nullptr, RUN); }

int tfx_dit_step_capture(const tfx_step_desc* s, tfx_stream stream, tfx_graph* out) { return step_entry(s, &kPlain, nullptr, nullptr, stream, out, CAPTURE); }

int tfx_dit_step_run_multistep(const tfx_step_desc* s, void* v_prev, tfx_stream stream) {
  const tfx_step_extra ex = history(v_prev);
  return step_entry(s, &ex, nullptr, nullptr, stream, nullptr, RUN | NEED_HISTORY);
}

int tfx_dit_step_capture_multistep(const tfx_step_desc* s, void* v_prev, tfx_stream stream, tfx_graph* out) {
  const tfx_step_extra ex = history(v_prev);
  return step_entry(s, &ex, nullptr, nullptr, stream, out, CAPTURE | NEED_HISTORY);
}

int tfx_dit_step_run_ex(const tfx_step_desc* s, const tfx_step_extra* ex, tfx_stream stream) { return step_entry(s, ex, nullptr, nullptr, stream, nullptr, RUN); }

int tfx_dit_step_capture_ex(const tfx_step_desc* s, const tfx_step_extra* ex, tfx_stream stream, tfx_graph* out) {
  return step_entry(s, ex, nullptr, nullptr, stream, out, CAPTURE);
}

int tfx_dit_step_run_ex2(const tfx_step_desc* s, const tfx_step_extra* ex, const tfx_step_change* ch, tfx_stream stream) {
  return step_entry(s, ex, ch, nullptr, stream, nullptr, RUN);
}

int tfx_dit_step_capture_ex2(const tfx_step_desc* s, const tfx_step_extra* ex, const tfx_step_change* ch, tfx_stream stream, tfx_graph* out) {
  return step_entry(s, ex, ch, nullptr, stream, out, CAPTURE);
}

int tfx_dit_step_run_ex3(const tfx_step_desc* s, const tfx_step_extra* ex, const tfx_step_change* ch, const tfx_step_cfg* cfg, tfx_stream stream) {
  return step_entry(s, ex, ch, cfg, stream, nullptr, RUN);
}

int tfx_dit_step_capture_ex3(const tfx_step_desc* s, const tfx_step_extra* ex, const tfx_step_change* ch, const tfx_step_cfg* cfg,
                             tfx_stream stream, tfx_graph* out) {
  return step_entry(s, ex, ch, cfg, stream, out, CAPTURE);
}

int tfx_dit_step_replay(tfx_graph graph, tfx_stream stream) {
  if (!graph) return fail("tfx_dit_step_replay: null graph");
  const hipError_t e = hipGraphLaunch(((StepGraph*)graph)->exec, S(stream));
  if (e != hipSuccess) return fail("tfx_dit_step_replay: hipGraphLaunch: %s", hipGetErrorString(e));
  return 0;
}

int tfx_graph_destroy(tfx_graph graph) {
  if (!graph) return 0;
  StepGraph* g = (StepGraph*)graph;
  (void)hipGraphExecDestroy(g->exec);
  (void)hipGraphDestroy(g->graph);
  delete g;
  return 0;
}

int tfx_dit_forward(const tfx_dit_desc* d, tfx_stream stream) {
  if (!d) return fail("tfx_dit_forward: null descriptor");
  if (!d->xin || !d->mod || !d->hid || !d->xn || !d->y || !d->out || !d->cos_tab || !d->sin_tab)
    return fail("tfx_dit_forward: null buffer in descriptor");
  if ((d->n_double > 0 && !d->dbl) || (d->n_single > 0 && !d->sgl)) return fail("tfx_dit_forward: null block table");
  if (d->T > 0 && !d->ctx0) return fail("tfx_dit_forward: ctx0 is null");
  return dit_forward(*d, S(stream));
}

}  // extern "C"
