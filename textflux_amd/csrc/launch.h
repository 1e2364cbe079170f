// Internal (C++) launch API shared between the kernel translation units and the C-ABI layer.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

struct tfx_dit_desc;   // include/textflux_hip.h

namespace tfx {

// Error plumbing: every launcher returns 0 on success; on failure the message is kept per thread and is
// readable through tfx_last_error().
int fail(const char* fmt, ...);
int check_launch(const char* what);
const char* last_error();

// Optional per-launch timing of the dominant kernels (bench.py's live roofline measurement): when enabled, the
// GEMM / attention launchers bracket each launch with hipEvents on the launch stream and account its algorithmic
// FLOPs.  kind: 0 = gemm8p, 1 = attention.
void prof_enable(int on);
bool prof_on();
bool prof_on(hipStream_t st);  // false while `st` is being captured into a graph
void prof_begin(int kind, double flops, hipStream_t st);
void prof_end(int kind, hipStream_t st);
int prof_collect(int kind, double* total_ms, double* total_flops, int* launches);
// The bracket as a scope: prof_begin now (when profiling is on and `st` is not being captured), prof_end on EVERY way out of the
// scope -- a record without its end event would make the next prof_collect fail.
class ProfScope {
 public:
  ProfScope(int kind, double flops, hipStream_t st, bool wanted = true) : kind_(kind), st_(st), on_(wanted && prof_on(st)) {
    if (on_) prof_begin(kind, flops, st);
  }
  ~ProfScope() { if (on_) prof_end(kind_, st_); }
  ProfScope(const ProfScope&) = delete;
  ProfScope& operator=(const ProfScope&) = delete;
 private:
  int kind_; hipStream_t st_; bool on_;
};

// ---- launch state: all of it is per DEVICE (HIP keeps function attributes on the per-device function object, and two devices of
// one process need not have the same CU count).  Lock-free: the tables below are indexed by the device ordinal and a race between two
// threads at most repeats a query / an attribute call, it never skips one.  Ordinals >= MAX_DEVICES are served uncached.
constexpr int MAX_DEVICES = 64;
// The CURRENT device: its CU count (256 when the runtime cannot say or says < 8) and the grid of the persistent kernels, one workgroup
// per CU in a whole number per XCD.  One hipGetDevice per call, no other HIP call after the first on a device.
struct DeviceFacts { int dev, cus, grid; };
DeviceFacts device_facts();
// What prepare_kernel remembers about one kernel: the dynamic LDS limit it set on each device (0 = not prepared there).
struct KernelPrep { std::atomic<int> lds[MAX_DEVICES]; };
template <auto K> inline KernelPrep kernel_prep{};     // one per __global__ function (instantiation)
// Makes `fn` launchable with `lds_bytes` of dynamic LDS on the current device (`dev`, as device_facts() gave it): loads the (lazily loaded) code object, raises the limit
// and remembers it, so that a later call asking for no more is one atomic load.  `vet`, when given, sees the kernel's attributes before
// the limit is raised; a non-zero result (its own fail(...)) is returned and nothing is remembered.  Errors name `family` and the bytes.
using KernelVet = int (*)(const hipFuncAttributes&);
int prepare_kernel(KernelPrep& kp, const void* fn, int dev, int lds_bytes, const char* family, KernelVet vet = nullptr);
template <auto K>
int prepare_kernel(int dev, int lds_bytes, const char* family, KernelVet vet = nullptr) {
  return prepare_kernel(kernel_prep<K>, (const void*)K, dev, lds_bytes, family, vet);
}

// GEMM epilogues (C = epi(A @ W^T + bias)).
enum Epilogue : int {
  EPI_BIAS = 0,           // C = acc + bias
  EPI_BIAS_GELU = 1,      // C = gelu_tanh(acc + bias) for columns >= gelu_from_col, plain bias below it
  EPI_BIAS_GATE_RES = 2,  // C = res + gate[b, col] * (acc + bias)
  EPI_BIAS_RES = 3,       // C = res + (acc + bias)   (VAE residual blocks)
  EPI_COLSCALE = 4,       // C = cscale[col] * acc, cscale fp32 read at run time, no bias (the down projection of a runtime LoRA adapter)
};

struct GemmArgs {
  const void* A; int64_t lda; int64_t a_bstride;     // activations  [batch][M, K] bf16, row stride lda
  const void* W;                                      // weights      [N, K] bf16 (nn.Linear layout), row stride ldw
  int64_t ldw;
  int64_t w_bstride = 0;                              // round 6: per-batch weights [batch][N, K] (elements; 0 = one W for every batch sample): the VAE mid-block attention's k / v^T
  const void* bias;                                   // [N] bf16 or null
  void* C; int64_t ldc; int64_t c_bstride;           // output       [batch][M, N] bf16
  int M, N, K, batch;
  int epilogue;
  int gelu_from_col;                                  // EPI_BIAS_GELU: first column that gets GELU
  const void* gate; int64_t gate_bstride;             // EPI_BIAS_GATE_RES: gate [batch][N] bf16
  const void* res; int64_t ldr; int64_t r_bstride;    // residual [batch][M, N] bf16 (may alias C)
  // implicit-GEMM 3x3 convolution on NHWC activations (conv_cin > 0): A = input [B, inH, inW, Cin], row m = output pixel
  // (b, y, x) of an H x W grid, K = 9 * Cin ordered (tap, ci); the input is read at ((y*stride - pad_lo + dy) >> up_shift,
  // (x*stride - pad_lo + dx) >> up_shift) -- up_shift = 1 folds a nearest 2x upsample into the gather -- and taps that
  // fall outside the (upsampled) input read `zero_page` (>= 128 B of zeros) instead.
  int conv_cin = 0, conv_inH = 0, conv_inW = 0, conv_H = 0, conv_W = 0, conv_stride = 1, conv_up_shift = 0, conv_pad_lo = 1;
  // pixel-pair form (conv_kw = 4, conv_stride_x = 2): one GEMM row = TWO horizontally adjacent output pixels, N = 2 * Cout (their
  // channels are neighbours in NHWC), K = 3 x 4 taps x Cin over the 4 input columns the pair touches, weights [2 Cout][3][4][Cin]
  // with zeros where a pixel does not use a column.  A third more FLOPs, but a 128-channel layer fills the 256-column tile.
  int conv_kw = 3, conv_stride_x = 0;
  const void* zero_page = nullptr;
  // fp8 (e4m3) operands, gemm_fp8 only: A and W hold one byte per element, C = (A.W^T) * a_scale[b][m] * w_scale[n] + bias
  const float* a_scale = nullptr; int64_t a_scale_bstride = 0;   // per activation row
  const float* w_scale = nullptr;                                 // per output channel
  // fused epilogue of the DiT's q | k | v (| mlp) projections (gemm_qkn_ok() shapes only): per-head (128 columns) RMSNorm
  // with weights qkn_wq / qkn_wk on the column ranges [qkn_q0, qkn_q1) / [qkn_k0, qkn_k1), then interleaved-pair RoPE with
  // (cos, sin) pairs qkn_rope_cs [tokens][64][2] fp32 at token qkn_pos0 + row; == rmsnorm_rope() applied afterwards
  const void* qkn_wq = nullptr; const void* qkn_wk = nullptr; const float* qkn_rope_cs = nullptr;
  int qkn_pos0 = 0, qkn_q0 = 0, qkn_q1 = 0, qkn_k0 = 0, qkn_k1 = 0; float qkn_eps = 1e-6f;
  int64_t qkn_rope_bstride = 0;                       // table rows between two batch samples' rotary tables (0 = one table for every sample)
  // optional scratch for the K-sliced units (fp32 partials, 256 KiB per unit); without it few-tile GEMMs run unsplit
  void* workspace = nullptr; int64_t workspace_bytes = 0;
  // row-split weights (persistent MFMA kernel only; split_row a multiple of 256, 0 = off): tiles whose first row inside the batch
  // sample is below split_row use W2 / bias2 / gate2 / qkn_wq2 / qkn_wk2 instead of W / bias / gate / qkn_wq / qkn_wk -- the text and
  // image projections of a double block in ONE launch over the joint [text | image] rows.  W2 must lie behind W within 4 GiB
  // (one buffer descriptor): the engine allocates the pair as one tensor.
  const float* cscale = nullptr;                      // EPI_COLSCALE: [N] fp32 device vector, 16-byte aligned
  int split_row = 0;
  const void* W2 = nullptr; const void* bias2 = nullptr; const void* gate2 = nullptr; const void* qkn_wq2 = nullptr; const void* qkn_wk2 = nullptr;
};
bool gemm_rowsplit_ok(const GemmArgs& a);                       // can this (split_row > 0) GEMM run as one launch?
void set_gemm_group_m(int gm);
void set_gemm_place(int v);
void set_gemm_waves(int v);      // 8 (default): gemm8pp_kernel; 4: gemm4w_kernel (one wave per SIMD) for unsliced bf16 launches
void set_gemm_splitk(int v);
int gemm_bf16(const GemmArgs& a, hipStream_t st);            // dispatches fast MFMA kernel or generic fallback
bool gemm_qkn_ok(const GemmArgs& a);                          // can this GEMM carry the fused q/k norm + RoPE epilogue?
bool gemm_fp8_qkn_ok(const GemmArgs& a);   // ... for the e4m3 path (gemm_fp8): an unsliced launch, same column conditions
// Runtime (unmerged) LoRA adapters as a K-extension of the Linear: C = epi(A W^T + T B^T + bias) in ONE fp32 accumulation, T = bf16(c * A Acat^T)
// from an earlier launch.  T [batch][M, nseg * R] (or nseg matrices [batch][M, R], t_seg) is addressed with A's lda / a_bstride and lies above A inside one 32-bit byte range (the
// caller owns everything between them); Bm [N, R] = W + K, i.e. columns [K, K + R) of W's rows (ldw >= K + R).  R: padded rank, 128 or 256.
// Output column n belongs to segment min(n / seg_cols, nseg - 1) and reads T's column block of that index; bit s of seg_mask = segment s
// carries an adapter (bit 8 + s: for the text rows of a row-split launch).  Persistent kernel, whole tiles only.
constexpr int LORA_MAX_RANK = 256;
// t_seg: elements between the T blocks of two segments (0 = R: column blocks of one matrix; else one matrix of A's shape per segment).
struct LoraArgs { const void* T; const void* Bm; int R, seg_cols, nseg; uint32_t seg_mask; int64_t t_seg = 0; };
int gemm_bf16_lora(const GemmArgs& a, const LoraArgs& l, hipStream_t st);
int gemm_bf16_variant(const GemmArgs& a, int variant, hipStream_t st);  // 0 = generic, 1 = MFMA 8-phase
int gemm_bf16_f32out(const GemmArgs& a, hipStream_t st);     // C = fp32 raw accumulators [batch][M, N] (ldc, c_bstride in floats)
int mfma_peak_probe(const void* operands, int64_t operand_bytes, int fp8, int ktiles, double* flops, hipStream_t st);   // tfx_mfma_peak_probe
int gemm_fp8(const GemmArgs& a, hipStream_t st);             // persistent MFMA kernel on e4m3 operands (K % 256 == 0)
// per-row absmax quantisation bf16 -> e4m3: out = x / scale, scale = absmax / 448 (1 for an all-zero row)
// LayerNorm + modulation whose output is written as the e4m3 quantisation of the bf16 row (fp8 mode; == ln_modulate followed
// by quantize_rows_fp8, bit for bit)
int ln_modulate_fp8(const void* x, void* q8, float* q8_scale, const void* shift, const void* scale, int64_t mod_bstride,
                    int rows_per_batch, int batch, int D, int64_t ldx, int64_t x_bstride, int64_t ldq, int64_t q_bstride,
                    int64_t s_bstride, float eps, hipStream_t st);
int quantize_rows_fp8(const void* x, int64_t ldx, int64_t x_bstride, void* out, int64_t ldo, int64_t o_bstride, float* scale,
                      int64_t s_bstride, int rows, int batch, int K, hipStream_t st);

struct AttnArgs {
  const void* q; const void* k; const void* v; void* o;   // bf16, element (b, n, h, d) at base + b*bstride + n*ld + h*128 + d
  int64_t ldq, ldk, ldv, ldo;
  int64_t q_bstride, k_bstride, v_bstride, o_bstride;
  int B, H, N;
  float scale;
  float score_bound = 0.f;   // caller's promise |scale * q . k| <= score_bound (0 = unknown): see tfx_attn_args
  void* workspace = nullptr; // optional scratch (tfx_attn_args.workspace): lets the head-dim-128 kernel deal (item, key tile) units (stream-K)
  int64_t workspace_bytes = 0;
  const int32_t* seq_len = nullptr;   // optional DEVICE int32 [B]: sample b's queries and keys are its first seq_len[b] rows (tfx_attn_args.seq_len)
};
int joint_attention(const AttnArgs& a, hipStream_t st);
int joint_attention_hp(const AttnArgs& a, hipStream_t st);   // half-tile software-pipelined kernel (attention_hp.hip)
int joint_attention_w16(const AttnArgs& a, hipStream_t st);  // one wave per SIMD on v_mfma_f32_16x16x32_bf16 (attention_w16.hip)
int attention_w4_release();                                    // frees every tail-split scratch buffer (tfx_release_scratch)
int attention_w4_prepare(hipStream_t st);                      // allocates the tail-split scratch of `st` (call outside stream capture)
void set_attention_tail_split(int v);                          // 0 = never split the last round's q-tiles by keys (bench knob)
int joint_attention_w4(const AttnArgs& a, hipStream_t st, int mode);   // one wave per SIMD, 64 query rows per wave (attention_w4.hip); mode (attn_w4_kernel<MODE>): 0 bookkeeping on the matrix pipe, 1 row sums on the VALU, 2 = 1 + lazy reference offset, 3 = 0 + lazy reference offset, 4 no reference at all (only when AttnArgs::score_bound is admissible, attention.hip)
void set_attention_ablation(int a);
void set_attention_use_bound(int v);      // 0: ignore AttnArgs::score_bound
int attention_mode_counts(int64_t* counts, int n, int reset);   // tfx_attention_mode_counts
void attention_note_streamk();                                   // counts[8]: a w4 launch whose last round ran as the stream-K tail
int blend_edge(const void* a, int64_t a_bs, int64_t a_ts, int64_t a_us, void* b, int64_t b_bs, int64_t b_ts, int64_t b_us, int batch,
               int extent, int len, int C, hipStream_t st);
int gate_residual(const void* x, int64_t ldx, int64_t x_bs, const void* gate, int64_t gate_bs, const void* res, int64_t ldr, int64_t r_bs,
                  void* out, int64_t ldo, int64_t o_bs, int rows, int batch, int D, hipStream_t st);   // out = res + bf16(gate[b, :] * x) (tfx_gate_residual)
void set_attention_streamk(int v);     // 0: whole (b, h, q-tile) items only; 1 (default): stream-K dealing when it pays and a workspace was passed; 2: whenever admissible
void set_attention_persistent(int v);  // 0: one workgroup per (b, h, q-tile) item instead of one per CU
void set_attention_debug(void* p);
void set_attention_waves(int nw);  // which attention kernel joint_attention launches: the values of tfx_set_option "attention_waves" (textflux_hip.h), 0 = the default (30)

int groupnorm_silu_nhwc(const void* x, void* out, const void* gamma, const void* beta, float* stats_ws, int B,
                        int64_t HW, int C, int groups, float eps, bool silu, hipStream_t st);
void set_ln_prefetch(int v);   // tfx_set_option ln_prefetch
int ln_modulate_split(const void* x, void* out, const void* shift, const void* scale, const void* shift2, const void* scale2,
                      int split_row, int64_t mod_bstride, int rows_per_batch, int batch, int D, int64_t ldx, int64_t x_bstride, int64_t ldo,
                      int64_t o_bstride, float eps, hipStream_t st);   // rows < split_row of a sample: (shift2, scale2)
int ln_modulate(const void* x, void* out, const void* shift, const void* scale, int64_t mod_bstride,
                int rows_per_batch, int batch, int D, int64_t ldx, int64_t x_bstride, int64_t ldo,
                int64_t o_bstride, float eps, hipStream_t st);
// nn.LayerNorm with elementwise affine on [rows, D] bf16 rows: ONE bf16 rounding, as F.layer_norm (CLIP text model)
int layernorm_affine(const void* x, void* out, const void* gamma, const void* beta, int64_t rows, int D, int64_t ldx, int64_t ldo,
                     float eps, hipStream_t st);
int rmsnorm_rope(void* buf, int64_t ld, int64_t bstride, int q_off, int k_off, int H, int Ntok, int T, int B,
                 const void* wq_img, const void* wk_img, const void* wq_txt, const void* wk_txt, const float* cosT,
                 const float* sinT, float eps, hipStream_t st);
// ... with one cos / sin table per batch sample, tab_bstride floats apart (mixed-geometry batches; 0 = rmsnorm_rope)
int rmsnorm_rope_tab(void* buf, int64_t ld, int64_t bstride, int q_off, int k_off, int H, int Ntok, int T, int B,
                     const void* wq_img, const void* wk_img, const void* wq_txt, const void* wk_txt, const float* cosT,
                     const float* sinT, int64_t tab_bstride, float eps, hipStream_t st);
int sched_step(bool amo, const void* v, void* x, void* xin, int64_t ldxin, int C, int64_t rows, const float* coef,
               const int* step_ptr, int step, const float* noise, hipStream_t st);
// second-order multistep update (coef fp32 [n_steps][2]); v_prev bf16 [rows, C] is read from step 1 on and then holds v
int multistep_step(const void* v, void* x, void* xin, int64_t ldxin, int C, int64_t rows, const float* coef,
                   const int* step_ptr, int step, void* v_prev, hipStream_t st);
// known-region blend behind a sampler update: x <- (1 - mask) scale_noise(x0, keep_sigma[step], noise) + mask x, bf16 per op;
// x [rows, C] with pitch ldx, mirrored into xin[:, :C] when given; a negative keep_sigma entry stands for "x0 itself"
int known_region_blend(void* x, int64_t ldx, const void* x0, const void* noise, const void* mask, int C, int64_t rows,
                       const float* keep_sigma, const int* step_ptr, int step, void* xin, int64_t ldxin, hipStream_t st);
// change-map blend behind a sampler update: known_region_blend with the mask decided on the device, k = hold[row, col & 3] > cut[step]
// (hold u8 [rows, 4], cut int32 [n_steps]); x <- p k + x (1 - k), bf16 per op; cut[step] >= 255 leaves x unwritten (xin still mirrored)
int change_map_blend(void* x, int64_t ldx, const void* x0, const void* noise, const void* hold, const int* cut, int C, int64_t rows,
                     const float* keep_sigma, const int* step_ptr, int step, void* xin, int64_t ldxin, hipStream_t st);
// true CFG in front of a sampler update: out <- neg + g (pos - neg), bf16 per op, g = *scale read on the device; v_neg, v_pos, out
// bf16 [rows, C] contiguous, out may be v_neg itself
int cfg_combine(const void* v_neg, const void* v_pos, void* out, int C, int64_t rows, const float* scale, hipStream_t st);
// the clean-image estimate behind an Euler update: out <- x - sigma[step] v, bf16 per op; x bf16 [rows, C] with pitch ldx, v and out
// contiguous; the step index from *step_ptr when given, else `step`
int x0_predict(const void* x, int64_t ldx, const void* v, void* out, int C, int64_t rows, const float* sigma, const int* step_ptr, int step,
               hipStream_t st);
int timestep_embedding(const float* t, void* out, int n, hipStream_t st);
int silu_bf16(const void* a, void* out, int64_t n, hipStream_t st);
int add_bf16(const void* a, const void* b, void* out, int64_t n, hipStream_t st);
int scatter_cols(const void* src, void* dst, int64_t rows, int C, int64_t ld, int col0, hipStream_t st);
int copy_rows(const void* src, int64_t sld, int64_t sbs, void* dst, int64_t dld, int64_t dbs, int rows, int cols,
              int batch, hipStream_t st);
// image / latent layout kernels around the VAE and the helpers of its mid-block attention (imageops.hip)
int any_negative(const void* x, int dtype, int64_t n, int* flag, hipStream_t st);
int prep_image(const void* img, int img_dtype, const void* mask, int mask_dtype, void* out, int B, int C, int H, int W,
               int mask_b, int norm_mode, int binarize, const int* neg_flag, hipStream_t st);
int compose_canvas(const void* glyph, const void* scene, const void* smask, void* canvas, void* cmask, int B, int gh, int gw, int sh,
                   int sw, int dir, int mask_rgb, hipStream_t st);
int rgb_to_grey(const void* rgb, void* out, int64_t n, hipStream_t st);
int resample_u8(const void* in, void* out, const int* bounds, const int* coeffs, int ksize, int64_t outer, int in_len, int out_len,
                int inner, hipStream_t st);
// paste-back: mask [B, H, W] u8 window passes (tmp: a third buffer of the mask's size) and the alpha blend of [B, H, W, C] u8 images
int mask_dilate_u8(const void* in, void* out, void* tmp, int B, int H, int W, int radius, hipStream_t st);
int mask_feather_u8(const void* in, void* out, void* tmp, int B, int H, int W, int radius, hipStream_t st);
int overlay_u8(const void* orig, const void* edit, const void* alpha, void* out, int B, int H, int W, int C, hipStream_t st);
// colour-matched paste-back: out u64 [B][C][5] = {n, sum a, sum b, sum a a, sum a b} over the pixels with weight != 0 (scratch: partial
// sums of up to 256 workgroups per sample, 17 u64 each), and the blend with the edit sent through lut u8 [B][C][256]
constexpr int64_t MASKED_MOMENTS_SCRATCH_BYTES = 256 * 17 * 8;   // per sample
int masked_moments_u8(const void* a, const void* b, const void* weight, void* out, void* scratch, int64_t scratch_bytes, int B, int H, int W,
                      int C, hipStream_t st);
int overlay_lut_u8(const void* orig, const void* edit, const void* alpha, const void* lut, void* out, int B, int H, int W, int C, hipStream_t st);
// seamless paste: the blend of overlay_lut_u8 (lut may be NULL) with a pull-push membrane of ref - edit, known where alpha == 0 (and
// covered != 0 when given), added to the edit first; workspace: seamless_workspace_bytes (host arithmetic; -1 on bad geometry)
int64_t seamless_workspace_bytes(int B, int H, int W, int C);
int seamless_overlay_u8(const void* orig, const void* ref, const void* edit, const void* alpha, const void* covered, const void* lut, void* out,
                        void* workspace, int64_t workspace_bytes, int B, int H, int W, int C, int smooth, int max_shift, hipStream_t st);
// grain match: out u32 [B][C][1024] = the histogram of |16 p - [1 2 1] x [1 2 1] p| (last bin: 1023 and above) over the pixels with
// lo <= sel <= hi (the call zeroes out), and hashed white grain of gain i32 [B][C] (Q16 of sigma / 147.8, device) added under alpha at
// the scene position origin i32 [B][2] (device, or NULL) + the pixel's place in the window
int highpass_hist_u8(const void* img, const void* sel, int lo, int hi, void* out, int B, int H, int W, int C, hipStream_t st);
int grain_u8(const void* img, const void* alpha, const int* gain, const int* origin, uint32_t seed, void* out, int B, int H, int W, int C,
             hipStream_t st);
// grain spectrum: the histogram with its eight neighbours at distance step in 1..8 and one more row, that of the residuals summed over
// the channels (out u32 [B][C + 1][1024]), and the grain blurred by [s, 256 - 2 s, s] squared and mixed with a share lam / 256 of one
// field common to the channels (shape i32 [B][2] = (s, lam), device; gain in [0, 2^18])
int highpass_hist_step_u8(const void* img, const void* sel, int lo, int hi, int step, void* out, int B, int H, int W, int C, hipStream_t st);
int grain_shaped_u8(const void* img, const void* alpha, const int* gain, const int* shape, const int* origin, uint32_t seed, void* out, int B,
                    int H, int W, int C, hipStream_t st);
// keyed paste: out u8 [B, H, W] = max over the channels of (|[1 2 1] x [1 2 1] (a - b)| + 8) >> 4, and its hysteresis threshold: 255 where
// m >= lo and an 8-connected path of such pixels leads to one with m >= hi, else 0; the launch is repeated until a round marks nothing
// (one stream synchronisation per round; refused on a capturing stream); workspace: hysteresis_workspace_bytes (-1 on bad geometry)
int change_metric_u8(const void* a, const void* b, void* out, int B, int H, int W, int C, hipStream_t st);
int64_t hysteresis_workspace_bytes(int B, int H, int W);
int hysteresis_u8(const void* m, void* out, int lo, int hi, void* workspace, int64_t workspace_bytes, int* rounds, int B, int H, int W,
                  hipStream_t st);
// rectified per-line edits: out [B, out_h, out_w, C] u8 = in [B, H, W, C] sampled at the Q16 affine image (m i64 [B][6], device) of every
// destination pixel, 4 x 4 taps from the i16 [256][4] table (device), edge replicated; coverage [B, out_h, out_w] u8 or NULL
int warp_affine_u8(const void* in, void* out, void* coverage, int B, int H, int W, int C, int out_h, int out_w, const int64_t* m,
                   const int16_t* taps, hipStream_t st);
// perspective per-line edits: the same under a homography m i64 [B][9] (device): positions Nx / D, Ny / D by floor division to 8
// fractional bits; D <= 0 writes 0 with coverage 0 and reads nothing
int warp_perspective_u8(const void* in, void* out, void* coverage, int B, int H, int W, int C, int out_h, int out_w, const int64_t* m,
                        const int16_t* taps, hipStream_t st);
// curved per-line edits: the same under a control grid i64 [B][gh][gw][2] (device) of Q16 source positions, one node per
// (1 << shift) destination pixels, blended bilinearly in integers; a pixel next to a node whose x is INT64_MIN writes 0 with coverage 0
// and reads nothing
int warp_grid_u8(const void* in, void* out, void* coverage, int B, int H, int W, int C, int out_h, int out_w, const int64_t* grid,
                 int shift, const int16_t* taps, hipStream_t st);
// candidates: the crops of table i64 [n][10] = (b, m0..m5, out_h, out_w, byte offset) (device) from images [B, H, W, C] u8, each
// warp_affine_u8's, packed as [out_h, out_w, C] at its byte offset in out; a row that cannot be served writes nothing and adds 1 to
// *refused (device); blocks_per_crop workgroups stride over a crop's tiles
int warp_affine_gather_u8(const void* images, void* out, int64_t out_bytes, const int64_t* table, int n, int* refused, int B, int H, int W,
                          int C, int blocks_per_crop, const int16_t* taps, hipStream_t st);
int pack_mask(const void* mask, int mask_dtype, void* out, int B, int H, int W, int mask_b, int binarize, int64_t ld, int col0,
              hipStream_t st);
// uint8 pixel mask [B, H, W] -> packed latent mask bf16 [B, (H/16)(W/16), C] of 1.0 / 0.0; mode 0 nearest (grow 0), 1 cover (grow 0..8)
int keep_mask_pack(const void* mask_u8, void* out, int B, int H, int W, int C, int mode, int grow, hipStream_t st);
// uint8 change map [B, H, W] -> hold u8 [B, (H/16)(W/16), 4] = 255 - map per latent pixel; mode 0 nearest (grow 0), 1 cover = maximum (grow 0..8)
int change_map_pack(const void* map_u8, void* hold, int B, int H, int W, int mode, int grow, hipStream_t st);
int sample_pack(const void* moments, const void* eps, int eps_dtype, void* out, int B, int h, int w, int L, float shift,
                float scale, int64_t ld, int col0, hipStream_t st);
int unpack_latents(const void* lat, int64_t ld, void* out, int B, int h, int w, int L, float shift, float scale, hipStream_t st);
int postprocess(const void* x, void* out, int B, int H, int W, int Cs, int C, int mode, int denorm, int y0, int x0, int Hc, int Wc,
                hipStream_t st);
int transpose_bf16(const void* in, int64_t ldi, int64_t ibs, void* out, int64_t ldo, int64_t obs, int N, int C, int batch,
                   hipStream_t st);
int row_softmax(const float* s, int64_t lds, void* p, int64_t ldp, int rows, int N, float scale, hipStream_t st);
// text-encoder kernels (textenc.hip)
int attention64(const AttnArgs& a, const float* rel_bias, int causal, hipStream_t st);
int rmsnorm(const void* x, int x_dtype, int64_t ldx, const void* w, void* out, int64_t ldo, int64_t rows, int D, float eps,
            hipStream_t st);
int gather_rows(const void* table, const int64_t* ids, void* out, int64_t n, int D, int64_t vocab, hipStream_t st);
int add_into_f32(float* x, const void* y, int64_t n, int mode, hipStream_t st);
int mul_act(const void* a, int64_t lda, const void* b, int64_t ldb, void* out, int64_t ldo, int64_t rows, int cols, int mode,
            hipStream_t st);
int select_step(const void* table, void* cur, int64_t per_step_elems, int* step_ptr, hipStream_t st);
int advance_step(int* step_ptr, hipStream_t st);

// The first-block step cache (tfx_step_cache, DESIGN.md section 4 "Step cache"): hid = the image rows of the joint stream as a strided
// view [batch][rows, ldh] (batch stride hbs), the cache's four bf16 buffers [batch][rows, ld] (batch stride bs).
struct StepCacheArgs {
  void* hid; int64_t ldh, hbs;
  void* x0; void* f_prev; void* h1; void* r; int64_t ld, bs;
  float* partials; float* metric;
  int rows, batch, D;
};
// The partition of the metric's sums, a function of (rows, D) alone: workgroups per sample (each 256 threads, <= STEP_CACHE_MAX_PARTS) and
// the 16-byte chunks one thread walks through in sequence.
constexpr int STEP_CACHE_MAX_PARTS = 256;
inline int step_cache_parts(int64_t chunks) { return (int)(chunks >= 256ll * STEP_CACHE_MAX_PARTS ? STEP_CACHE_MAX_PARTS : (chunks + 255) / 256); }
int step_cache_save(const StepCacheArgs& a, hipStream_t st);     // x0 <- hid
int step_cache_metric(const StepCacheArgs& a, hipStream_t st);   // f = bf16(hid - x0) over x0, h1 <- hid, metric[b] = sum|f - f_prev| / sum|f_prev|
int step_cache_store(const StepCacheArgs& a, hipStream_t st);    // r <- bf16(hid - h1), f_prev <- x0
int step_cache_apply(const StepCacheArgs& a, hipStream_t st);    // hid <- bf16(hid + r)

// One DiT forward on the launchers above (dit_forward.cpp; tfx_dit_forward checks the descriptor's pointers in front of it) and its
// process-wide A/B knobs (tfx_set_option fp8_fuse_qkn / ln_joint / gemm_group_streams, all default 1).
int dit_forward(const tfx_dit_desc& d, hipStream_t st);
void set_fp8_fuse_qkn(int v);
void set_ln_joint(int v);
void set_gemm_group_streams(int v);

}  // namespace tfx
