// Recording stand-in for the launch layer (csrc/launch.h), linked in place of launch.cpp and the kernel objects by
// tests/test_mixed_batch_cpu.py.  It is launch_recorder.cpp plus what a mixed-geometry forward adds to the launch layer: the per-sample
// fields of the attention and q / k norm arguments (seq_len, rope_bs) and the norm + RoPE pass with one table per sample
// (rmsnorm_rope_tab) -- a file of its own so that the uniform path's recorder, driver and golden stay exactly as they are.
// Every launcher tfx_dit_forward / tfx_dit_step_run can reach prints one line with all of its
// arguments and returns 0, the three shape probes answer from a bit mask and print a `probe` line.  Pointers print as
// `name+0xoff` of the fake regions the driver registered, so the trace reads as a launch plan.  A launcher that is not defined here stays
// an unresolved symbol of the test binary: calling it ends the run.
#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>

#include "launch.h"

namespace tfx {

// ---- what the driver (mixed_trace_driver.cpp) sets
int g_probe_mask = 7;   // bit 0 gemm_rowsplit_ok, 1 gemm_qkn_ok, 2 gemm_fp8_qkn_ok
static std::vector<std::string> g_regions;   // region k + 1 starts at address (k + 1) << 32
void* trace_region(const char* name) {
  g_regions.push_back(name);
  return (void*)((uint64_t)g_regions.size() << 32);
}
void trace_reset() { g_regions.clear(); }

static thread_local std::string g_err;
int fail(const char* fmt, ...) {
  char b[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(b, sizeof b, fmt, ap);
  va_end(ap);
  g_err = b;
  return 1;
}
const char* last_error() { return g_err.c_str(); }

namespace {

std::string sym(const void* p) {
  const uint64_t v = (uint64_t)p, k = v >> 32, off = v & 0xffffffffull;
  char b[64];
  if (!p) return "0";
  if (k == 0 || k > g_regions.size()) { snprintf(b, sizeof b, "?%#llx", (unsigned long long)v); return b; }
  if (!off) return g_regions[k - 1];
  snprintf(b, sizeof b, "+%#llx", (unsigned long long)off);
  return g_regions[k - 1] + b;
}
std::string num(float v) { char b[32]; snprintf(b, sizeof b, "%.9g", v); return b; }
template <class T> std::string num(T v) { return std::to_string((int64_t)v); }

// one text line: the launcher's name, then its arguments in declaration order
struct Line {
  std::string s;
  explicit Line(const char* what) : s(what) {}
  Line& p(const void* v) { s += ' '; s += sym(v); return *this; }
  Line& i(int64_t v) { s += ' '; s += num(v); return *this; }
  Line& f(float v) { s += ' '; s += num(v); return *this; }
  ~Line() { puts(s.c_str()); }
};

// struct arguments: every field that differs from a value-initialised struct, as label=value (labels: the field names, the long
// ones shortened -- *_bstride -> *_bs, qkn_* without the prefix, workspace -> ws, epilogue -> epi, split_row -> split)
#define FIELD_P(x, label) if (a.x != z.x) { l.s += " " label "="; l.s += sym((const void*)a.x); }
#define FIELD_N(x, label) if (a.x != z.x) { l.s += " " label "="; l.s += num(a.x); }
void fields(Line& l, const GemmArgs& a) {
  const GemmArgs z = GemmArgs();
  FIELD_P(A, "A") FIELD_N(lda, "lda") FIELD_N(a_bstride, "a_bs") FIELD_P(W, "W") FIELD_N(ldw, "ldw") FIELD_N(w_bstride, "w_bs") FIELD_P(bias, "bias")
  FIELD_P(C, "C") FIELD_N(ldc, "ldc") FIELD_N(c_bstride, "c_bs") FIELD_N(M, "M") FIELD_N(N, "N") FIELD_N(K, "K") FIELD_N(batch, "batch")
  FIELD_N(epilogue, "epi") FIELD_N(gelu_from_col, "gelu_from") FIELD_P(gate, "gate") FIELD_N(gate_bstride, "gate_bs") FIELD_P(res, "res") FIELD_N(ldr, "ldr") FIELD_N(r_bstride, "r_bs")
  FIELD_N(conv_cin, "conv_cin") FIELD_N(conv_inH, "conv_inH") FIELD_N(conv_inW, "conv_inW") FIELD_N(conv_H, "conv_H") FIELD_N(conv_W, "conv_W") FIELD_N(conv_stride, "conv_stride") FIELD_N(conv_up_shift, "conv_up_shift")
  FIELD_N(conv_pad_lo, "conv_pad_lo") FIELD_N(conv_kw, "conv_kw") FIELD_N(conv_stride_x, "conv_stride_x") FIELD_P(zero_page, "zero_page")
  FIELD_P(a_scale, "a_scale") FIELD_N(a_scale_bstride, "a_scale_bs") FIELD_P(w_scale, "w_scale")
  FIELD_P(qkn_wq, "wq") FIELD_P(qkn_wk, "wk") FIELD_P(qkn_rope_cs, "rope_cs") FIELD_N(qkn_rope_bstride, "rope_bs") FIELD_N(qkn_pos0, "pos0") FIELD_N(qkn_q0, "q0") FIELD_N(qkn_q1, "q1") FIELD_N(qkn_k0, "k0") FIELD_N(qkn_k1, "k1")
  FIELD_N(qkn_eps, "eps") FIELD_P(workspace, "ws") FIELD_N(workspace_bytes, "ws_bytes") FIELD_P(cscale, "cscale") FIELD_N(split_row, "split")
  FIELD_P(W2, "W2") FIELD_P(bias2, "bias2") FIELD_P(gate2, "gate2") FIELD_P(qkn_wq2, "wq2") FIELD_P(qkn_wk2, "wk2")
}
void fields(Line& l, const AttnArgs& a) {
  const AttnArgs z = AttnArgs();
  FIELD_P(q, "q") FIELD_P(k, "k") FIELD_P(v, "v") FIELD_P(o, "o") FIELD_N(ldq, "ldq") FIELD_N(ldk, "ldk") FIELD_N(ldv, "ldv") FIELD_N(ldo, "ldo")
  FIELD_N(q_bstride, "q_bs") FIELD_N(k_bstride, "k_bs") FIELD_N(v_bstride, "v_bs") FIELD_N(o_bstride, "o_bs") FIELD_N(B, "B") FIELD_N(H, "H") FIELD_N(N, "N")
  FIELD_N(scale, "scale") FIELD_N(score_bound, "bound") FIELD_P(workspace, "ws") FIELD_N(workspace_bytes, "ws_bytes") FIELD_P(seq_len, "seq_len")
}
void fields(Line& l, const LoraArgs& a) {
  const LoraArgs z = LoraArgs();
  FIELD_P(T, "T") FIELD_P(Bm, "Bm") FIELD_N(R, "R") FIELD_N(seg_cols, "seg_cols") FIELD_N(nseg, "nseg") FIELD_N(seg_mask, "seg_mask") FIELD_N(t_seg, "t_seg")
}
#undef FIELD_P
#undef FIELD_N

bool probe(const char* what, const GemmArgs& a, bool answer) {
  Line l("probe");
  l.s += ' ';
  l.s += what;
  fields(l, a);
  return answer;
}
int gemm(const char* what, const GemmArgs& a) {
  Line l(what);
  fields(l, a);
  return 0;
}

}  // namespace

bool gemm_rowsplit_ok(const GemmArgs& a) { return probe("gemm_rowsplit_ok", a, a.split_row > 0 && (g_probe_mask & 1)); }
bool gemm_qkn_ok(const GemmArgs& a) { return probe("gemm_qkn_ok", a, g_probe_mask & 2); }
bool gemm_fp8_qkn_ok(const GemmArgs& a) { return probe("gemm_fp8_qkn_ok", a, g_probe_mask & 4); }

int gemm_bf16(const GemmArgs& a, hipStream_t) { return gemm("gemm_bf16", a); }
int gemm_fp8(const GemmArgs& a, hipStream_t) { return gemm("gemm_fp8", a); }
int gemm_bf16_lora(const GemmArgs& a, const LoraArgs& la, hipStream_t) {
  Line l("gemm_bf16_lora");
  fields(l, a);
  l.s += " | lora";
  fields(l, la);
  return 0;
}
int joint_attention(const AttnArgs& a, hipStream_t) {
  Line l("joint_attention");
  fields(l, a);
  return 0;
}

int quantize_rows_fp8(const void* x, int64_t ldx, int64_t x_bstride, void* out, int64_t ldo, int64_t o_bstride, float* scale,
                      int64_t s_bstride, int rows, int batch, int K, hipStream_t) {
  Line("quantize_rows_fp8").p(x).i(ldx).i(x_bstride).p(out).i(ldo).i(o_bstride).p(scale).i(s_bstride).i(rows).i(batch).i(K);
  return 0;
}
int ln_modulate(const void* x, void* out, const void* shift, const void* scale, int64_t mod_bstride, int rows_per_batch, int batch, int D,
                int64_t ldx, int64_t x_bstride, int64_t ldo, int64_t o_bstride, float eps, hipStream_t) {
  Line("ln_modulate").p(x).p(out).p(shift).p(scale).i(mod_bstride).i(rows_per_batch).i(batch).i(D).i(ldx).i(x_bstride).i(ldo).i(o_bstride).f(eps);
  return 0;
}
int ln_modulate_split(const void* x, void* out, const void* shift, const void* scale, const void* shift2, const void* scale2, int split_row,
                      int64_t mod_bstride, int rows_per_batch, int batch, int D, int64_t ldx, int64_t x_bstride, int64_t ldo,
                      int64_t o_bstride, float eps, hipStream_t) {
  Line("ln_modulate_split").p(x).p(out).p(shift).p(scale).p(shift2).p(scale2).i(split_row).i(mod_bstride).i(rows_per_batch).i(batch).i(D)
      .i(ldx).i(x_bstride).i(ldo).i(o_bstride).f(eps);
  return 0;
}
int ln_modulate_fp8(const void* x, void* q8, float* q8_scale, const void* shift, const void* scale, int64_t mod_bstride, int rows_per_batch,
                    int batch, int D, int64_t ldx, int64_t x_bstride, int64_t ldq, int64_t q_bstride, int64_t s_bstride, float eps,
                    hipStream_t) {
  Line("ln_modulate_fp8").p(x).p(q8).p(q8_scale).p(shift).p(scale).i(mod_bstride).i(rows_per_batch).i(batch).i(D).i(ldx).i(x_bstride)
      .i(ldq).i(q_bstride).i(s_bstride).f(eps);
  return 0;
}
int rmsnorm_rope(void* buf, int64_t ld, int64_t bstride, int q_off, int k_off, int H, int Ntok, int T, int B, const void* wq_img,
                 const void* wk_img, const void* wq_txt, const void* wk_txt, const float* cosT, const float* sinT, float eps, hipStream_t) {
  Line("rmsnorm_rope").p(buf).i(ld).i(bstride).i(q_off).i(k_off).i(H).i(Ntok).i(T).i(B).p(wq_img).p(wk_img).p(wq_txt).p(wk_txt).p(cosT)
      .p(sinT).f(eps);
  return 0;
}
int rmsnorm_rope_tab(void* buf, int64_t ld, int64_t bstride, int q_off, int k_off, int H, int Ntok, int T, int B, const void* wq_img,
                     const void* wk_img, const void* wq_txt, const void* wk_txt, const float* cosT, const float* sinT, int64_t tab_bstride,
                     float eps, hipStream_t) {
  Line("rmsnorm_rope_tab").p(buf).i(ld).i(bstride).i(q_off).i(k_off).i(H).i(Ntok).i(T).i(B).p(wq_img).p(wk_img).p(wq_txt).p(wk_txt).p(cosT)
      .p(sinT).i(tab_bstride).f(eps);
  return 0;
}
int copy_rows(const void* src, int64_t sld, int64_t sbs, void* dst, int64_t dld, int64_t dbs, int rows, int cols, int batch, hipStream_t) {
  Line("copy_rows").p(src).i(sld).i(sbs).p(dst).i(dld).i(dbs).i(rows).i(cols).i(batch);
  return 0;
}
int select_step(const void* table, void* cur, int64_t per_step_elems, int* step_ptr, hipStream_t) {
  Line("select_step").p(table).p(cur).i(per_step_elems).p(step_ptr);
  return 0;
}
int sched_step(bool amo, const void* v, void* x, void* xin, int64_t ldxin, int C, int64_t rows, const float* coef, const int* step_ptr,
               int step, const float* noise, hipStream_t) {
  Line("sched_step").i(amo).p(v).p(x).p(xin).i(ldxin).i(C).i(rows).p(coef).p(step_ptr).i(step).p(noise);
  return 0;
}
int advance_step(int* step_ptr, hipStream_t) {
  Line("advance_step").p(step_ptr);
  return 0;
}

}  // namespace tfx
