/* libtextflux_hip.so -- C ABI of the MI355X (gfx950) TextFlux / FLUX.1-Fill denoising engine.
 *
 * The reference (yyyyyxie/textflux @ 2025-09-26) has no FFI: its hot path sits behind Python object protocols of the
 * vendored diffusers 0.32.0.dev0.  Each entry point below names the reference call site(s) it
 * replaces; `D/` = diffusers/src/diffusers in the reference tree.  INTEGRATION.md shows the ctypes binding and how
 * the reference-side classes would call it.
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on error; tfx_last_error() then describes it (thread local);
 *   - all tensor arguments are DEVICE pointers to bf16 (uint16 bit pattern) unless typed otherwise; nothing is
 *     allocated or freed by the library, no pointer is retained after a call returns;
 *   - `stream` is a hipStream_t (NULL = default stream); all work is enqueued asynchronously on it and is safe to
 *     capture into a hipGraph (no allocation, no synchronisation, no host read-back inside any entry point);
 *   - row-major matrices with explicit leading dimensions (`ld*`, in elements) and batch strides (`*_bstride`).
 */
#ifndef TEXTFLUX_HIP_H
#define TEXTFLUX_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* tfx_stream;

/* ---- library -------------------------------------------------------------------------------------------- */
const char* tfx_version(void);
const char* tfx_last_error(void);
/* ABI stamp.  TFX_ABI_VERSION is bumped whenever a struct below grows or the meaning of a field / entry point changes;
 * tfx_abi_info writes {TFX_ABI_VERSION the library was built with, sizeof(tfx_gemm_args), sizeof(tfx_attn_args),
 * sizeof(tfx_dit_desc), sizeof(tfx_step_desc), sizeof(tfx_double_block), sizeof(tfx_single_block)} (as many as fit in n; the last
 * two since ABI 6) and returns how many values there are.  A binding
 * compares them with its own view of this header BEFORE the first call that passes a struct: a library built from an older
 * header would otherwise ignore the tail fields of a grown struct silently (no reference counterpart: the reference has no FFI). */
#define TFX_ABI_VERSION 11
int tfx_abi_info(int32_t* out, int n);
/* Writes the gcnArchName of the current device (e.g. "gfx950:sramecc+:xnack-") into buf.  Needs a GPU. */
int tfx_query_arch(char* buf, int buflen);

/* ---- GEMM:  C[b] = epi(A[b] @ W^T + bias)  (every nn.Linear on the path: D/models/attention_processor.py:1990-1992,
 *      2009-2011, 2052, 2056; D/models/attention.py:1217-1232; transformer_flux.py:724, 732, 1086, 1099, 1203;
 *      D/models/normalization.py:168, 200, 364; D/models/embeddings.py:1008-1021, 1926-1931).
 *      A [batch][M,K] (lda, a_bstride), W [N,K] nn.Linear layout (ldw), bias [N] or NULL, C [batch][M,N].
 *      epilogue: 0 bias | 1 bias, then tanh-GELU on columns >= gelu_from_col (activations.py:83; the split form is the
 *      fused [k|v|q|mlp] projection of FluxSingleTransformerBlock) | 3 C = res + (A@W^T + bias) | 2 C = res + gate[b,:] * (A@W^T + bias)
 *      (gated residual, transformer_flux.py:733-735, 817-818, 824-826, 830-831, 837; res may alias C) | 4 (ABI 9) C = bf16(cscale[n] *
 *      (A@W^T)): a per-output-column fp32 factor read from DEVICE memory at run time, bias must be NULL -- the down projection
 *      t = bf16(c * (x @ Acat^T)) of runtime LoRA adapters (tfx_gemm_bf16_lora below; PEFT's lora_A + scaling, D/utils/peft_utils.py:103-120):
 *      a captured graph sees a new adapter scale without re-capture.  tfx_gemm_bf16 only.
 *      variant: -1 auto, 0 generic FMA kernel (any shape), 1 MFMA path (K % 64 == 0, N % 8 == 0, 16-byte aligned;
 *      the persistent kernel when K % 128 == 0, else the one-tile kernel), 2 / 3 force the one-tile / persistent MFMA
 *      kernel (tests: the two agree bit for bit). */
typedef struct tfx_gemm_args {
  const void* A; int64_t lda; int64_t a_bstride;
  const void* W; int64_t ldw;
  const void* bias;
  void* C; int64_t ldc; int64_t c_bstride;
  int32_t M, N, K, batch;
  int32_t epilogue;
  int32_t gelu_from_col;
  const void* gate; int64_t gate_bstride;
  const void* res; int64_t ldr; int64_t r_bstride;
  /* optional caller-owned scratch (>= 16-byte aligned): when a GEMM has fewer 256x256 tiles than the device has CUs, the
   * auto path splits K into 2-4 slices, writes fp32 partials [slices][batch][M][N] here and finishes in a second pass
   * (deterministic: slices are summed in order).  NULL / too small = no split. */
  void* workspace; int64_t workspace_bytes;
  /* ABI 7 (round 6): per-batch weights, W [batch][N, K] with batch stride w_bstride elements (a multiple of 8; 0 = ONE weight matrix
   * for every batch sample, every nn.Linear).  bf16 entry points only; what the VAE mid-block attention's q k^T and P v products are
   * (k and v^T differ per image): one launch per query-row chunk for the whole batch instead of one per image. */
  int64_t w_bstride;
  /* ABI 9: epilogue 4's factors, fp32 [N], 16-byte aligned (ignored by every other epilogue) */
  const float* cscale;
} tfx_gemm_args;
int tfx_gemm_bf16(const tfx_gemm_args* args, int variant, tfx_stream stream);

/* Round 6 (ABI 7).  The fused q | k | v (| mlp) projection of a FLUX block as ONE operation: tfx_gemm_bf16 (epilogue 0 or 1) whose
 * epilogue also applies the per-head RMSNorm (weights norm_q / norm_k, bf16 [128]) and the interleaved-pair RoPE to the q and k column
 * ranges [q0, q1) / [k0, k1) of the output (multiples of 256: whole pairs of 128-wide heads), rounding for rounding as tfx_rmsnorm_rope
 * does it after the fact (D/models/attention_processor.py:1990-1992, 2001-2004, 2023-2037; transformer_flux.py:715-739).  rope_cs: the
 * rotary table as fp32 (cos, sin) pairs [rows, 64, 2]; output row m of a batch sample uses table row pos0 + m.  This is the kernel
 * tfx_dit_forward launches internally for every block projection with at least as many 256 x 256 tiles as the device has CUs; shapes it
 * cannot take (K % 128 != 0, unaligned ranges, fewer tiles than CUs with a workspace: the K-sliced path has no such epilogue) are
 * refused -- run tfx_gemm_bf16 + tfx_rmsnorm_rope instead. */
typedef struct tfx_qkn_args {
  const void* norm_q; const void* norm_k;
  const float* rope_cs;
  int32_t pos0, q0, q1, k0, k1;
  float eps;
  /* ABI 10, mixed-geometry batches: one rotary table per batch sample, rope_bstride table ROWS apart -- output row m of sample b uses
   * table row b * rope_bstride + pos0 + m; 0 = one table for every sample (what the reference computes: one img_ids per call,
   * transformer_flux.py:1117-1126).  The fp8 form of the epilogue inside tfx_dit_forward takes the same stride. */
  int64_t rope_bstride;
} tfx_qkn_args;
int tfx_gemm_bf16_qkn(const tfx_gemm_args* args, const tfx_qkn_args* qkn, tfx_stream stream);

/* ABI 9.  A Linear with RUNTIME (unmerged) LoRA adapters (PEFT's lora.Linear.forward, scaled per call as
 * transformer_flux.py:1073-1079 / D/utils/peft_utils.py:103-120 do): the low-rank update is a K-extension of the GEMM,
 *     C = epi(A @ W^T + T @ Bm^T + bias)          ONE fp32 accumulation, then the epilogue of tfx_gemm_bf16 / tfx_gemm_bf16_qkn,
 * where T = bf16(c * (A @ Acat^T)) [batch][M, nseg * R] is the scaled down-projection the caller computed before (c = scale * adapter
 * weight * alpha / r), so the fused q / k norm + RoPE epilogue (qkn != NULL) sees the adapted projection.  The engine's rounding points:
 * T once to bf16, the sum once in the epilogue; PEFT rounds the down projection, the up projection, the scaled update and the base
 * Linear separately.
 *   R          padded rank: 128 or 256 (zero-pad smaller ranks; several adapters on one Linear concatenate along the rank axis);
 *   segments   a fused weight holds several reference Linears as row ranges of seg_cols rows (a multiple of 256), each with its own
 *              A: output column n belongs to segment min(n / seg_cols, nseg - 1), nseg <= 4, and reads T's columns
 *              [seg * R, seg * R + R) -- or, t_seg_stride != 0 (where nseg * R exceeds A's row pitch), the R columns of a T matrix of its
 *              own, t_seg_stride elements above the previous segment's (a multiple of 8, no overlap).  seg_mask bit s = segment s carries an adapter; tiles of other segments skip the tail (their
 *              T block and Bm rows are never read).  Row-split launches: bit 8 + s for the rows below split_row;
 *   placement  the kernel addresses the tail through the descriptors of A and W, so: T is addressed with args->lda / a_bstride
 *              (nseg * R <= lda) and lies ABOVE A with both inside one caller-owned byte range below 4 GiB - 64 KiB that is readable
 *              throughout (e.g. one allocation [x | T]); Bm == W + K, i.e. row n of Bm is stored behind row n of W (ldw >= K + R).
 *   row split  split_row > 0 (a multiple of 256, < M): rows below it (the TEXT rows of the joint [text | image] stream) use W2 / bias2 /
 *              gate2 / norm_q2 / norm_k2; W2 (with its own Bm behind its rows, same ldw) lies above W within 4 GiB.  0 = off.
 * Always the persistent MFMA kernel on whole tiles (K % 128 == 0, N % 8 == 0, 16-byte aligned rows; args->workspace is ignored: an
 * adapted GEMM is never K-sliced); operands it cannot take are refused, there is no fallback.  bf16 only. */
typedef struct tfx_lora_args {
  const void* T; const void* Bm;
  int32_t R, seg_cols, nseg;
  uint32_t seg_mask;
  int32_t split_row;
  const void* W2; const void* bias2; const void* gate2; const void* norm_q2; const void* norm_k2;
  int64_t t_seg_stride;
} tfx_lora_args;
int tfx_gemm_bf16_lora(const tfx_gemm_args* args, const tfx_qkn_args* qkn /* NULL = no q/k norm */, const tfx_lora_args* lora,
                       tfx_stream stream);

/* Same operands, C = fp32 raw accumulators [batch][M, N] (ldc / c_bstride in floats, C 16-byte aligned); bias must be
 * NULL and epilogue 0.  Used where a product must reach its consumer unrounded: the q k^T scores of the VAE mid-block
 * attention (D/models/attention_processor.py:2858-2862) on their way to tfx_row_softmax. */
int tfx_gemm_bf16_f32(const tfx_gemm_args* args, tfx_stream stream);

/* ---- fp8 (OCP e4m3) variant of the same Linear, BASELINE config 5 "fp8 weights (CDNA4 fp8 MFMA)"; no reference
 *      counterpart (the reference computes in bf16).  A [batch][M, K] and W [N, K] hold one e4m3 byte per element
 *      (lda / ldw / a_bstride count elements = bytes), C = (A . W^T) * a_scale[b][m] * w_scale[n] + bias with the same
 *      epilogues, bf16 output.  K % 256 == 0, rows 16-byte aligned.  tfx_quantize_rows_fp8 produces both operands:
 *      out = round_e4m3(x / scale), scale[b * s_bstride + row] = max|x[row]| / 448 (1.0 for an all-zero row). */
int tfx_gemm_fp8(const tfx_gemm_args* args, const float* a_scale, int64_t a_scale_bstride, const float* w_scale,
                 tfx_stream stream);
int tfx_quantize_rows_fp8(const void* x, int64_t ldx, int64_t x_bstride, void* out, int64_t ldo, int64_t o_bstride,
                          float* scale, int64_t s_bstride, int32_t rows, int32_t batch, int32_t K, tfx_stream stream);
/* tfx_ln_modulate whose result is written as the e4m3 quantisation of the bf16 row (== tfx_ln_modulate followed by
 * tfx_quantize_rows_fp8, bit for bit): q8 [B][rows, D] bytes with row stride ldq / batch stride q_bstride (bytes),
 * q8_scale[b * s_bstride + row]. */
int tfx_ln_modulate_fp8(const void* x, int64_t ldx, int64_t x_bstride, void* q8, int64_t ldq, int64_t q_bstride,
                        float* q8_scale, int64_t s_bstride, const void* shift, const void* scale, int64_t mod_bstride,
                        int32_t rows_per_batch, int32_t batch, int32_t D, float eps, tfx_stream stream);

/* ---- LayerNorm(no affine, eps) * (1 + scale[b]) + shift[b]   (AdaLayerNormZero / ZeroSingle / Continuous,
 *      D/models/normalization.py:170, 202, 365; norm2 + modulation, transformer_flux.py:820-821, 833-834).
 *      x, out: [batch][rows_per_batch, D]; shift, scale: [batch][D] with stride mod_bstride.  D % 8 == 0, D <= 3072. */
int tfx_ln_modulate(const void* x, int64_t ldx, int64_t x_bstride, void* out, int64_t ldo, int64_t o_bstride,
                    const void* shift, const void* scale, int64_t mod_bstride, int32_t rows_per_batch, int32_t batch,
                    int32_t D, float eps, tfx_stream stream);
/* The same pass with two modulations: rows < split_row of every sample take (shift2, scale2), the others (shift, scale), all four
 * [batch][D] with stride mod_bstride -- the text and image streams of a double block, laid out as joint [text | image] rows, in one
 * launch (what tfx_dit_forward runs).  Bit-identical to two tfx_ln_modulate calls on the two row ranges.  0 <= split_row <=
 * rows_per_batch; shift2 / scale2 may be NULL when split_row == 0.  Added without a new TFX_ABI_VERSION: one new entry point, no
 * stamped struct and no existing entry point changes. */
int tfx_ln_modulate_split(const void* x, int64_t ldx, int64_t x_bstride, void* out, int64_t ldo, int64_t o_bstride,
                          const void* shift, const void* scale, const void* shift2, const void* scale2, int32_t split_row,
                          int64_t mod_bstride, int32_t rows_per_batch, int32_t batch, int32_t D, float eps, tfx_stream stream);

/* ---- per-head RMSNorm * weight, then RoPE, in place on the q and k column ranges of a fused projection buffer
 *      [B][Ntok, ld] (heads of 128) (FluxAttnProcessor2_0, D/models/attention_processor.py:2001-2004, 2023-2037;
 *      RMSNorm D/models/normalization.py:534-549; apply_rotary_emb D/models/embeddings.py:899-918).
 *      Rows < T use w*_txt (norm_added_q/k), rows >= T use w*_img (norm_q/k).  cos/sin: fp32 [Ntok,128].
 *      buf, the four weights and both tables 16-byte aligned; H, Ntok, T, B >= 0 (an empty extent returns 0). */
int tfx_rmsnorm_rope(void* buf, int64_t ld, int64_t bstride, int32_t q_off, int32_t k_off, int32_t H, int32_t Ntok,
                     int32_t T, int32_t B, const void* wq_img, const void* wk_img, const void* wq_txt,
                     const void* wk_txt, const float* cos_tab, const float* sin_tab, float eps, tfx_stream stream);

/* ABI 10, mixed-geometry batches: the same pass with one cos / sin table per batch sample -- sample b reads cos_tab / sin_tab +
 * b * tab_bstride (fp32 elements, a multiple of 4; 0 = tfx_rmsnorm_rope).  No reference counterpart: the reference runs one geometry
 * per call. */
int tfx_rmsnorm_rope_batched(void* buf, int64_t ld, int64_t bstride, int32_t q_off, int32_t k_off, int32_t H, int32_t Ntok,
                             int32_t T, int32_t B, const void* wq_img, const void* wk_img, const void* wq_txt,
                             const void* wk_txt, const float* cos_tab, const float* sin_tab, int64_t tab_bstride, float eps,
                             tfx_stream stream);

/* the name SURVEY.md §8(b) lists for the same entry point (q AND k of one fused buffer): identical arguments and behaviour */
int tfx_rmsnorm_rope_qk(void* buf, int64_t ld, int64_t bstride, int32_t q_off, int32_t k_off, int32_t H, int32_t Ntok,
                        int32_t T, int32_t B, const void* wq_img, const void* wk_img, const void* wq_txt,
                        const void* wk_txt, const float* cos_tab, const float* sin_tab, float eps, tfx_stream stream);

/* ---- gated residual out[b][r, :] = res[b][r, :] + bf16(gate[b][:] * x[b][r, :])   (transformer_flux.py:733-735, 817-818, 824-826,
 *      830-831, 837: `hidden_states + gate.unsqueeze(1) * attn_output`; the product is rounded to bf16 before the add, as the
 *      reference's two bf16 ops do).  Standalone form of tfx_gemm_args.epilogue 2 for a caller that keeps its own Linear (the
 *      attention-processor plugin level); inside tfx_dit_forward the same arithmetic runs in the producing GEMM's epilogue.
 *      x, res, out: bf16 [batch][rows_per_batch, D] with row strides ldx / ldr / ldo and batch strides; gate: bf16 [batch][D] with
 *      batch stride gate_bstride.  D % 8 == 0; out may alias res or x. */
int tfx_gate_residual(const void* x, int64_t ldx, int64_t x_bstride, const void* gate, int64_t gate_bstride, const void* res,
                      int64_t ldr, int64_t r_bstride, void* out, int64_t ldo, int64_t o_bstride, int32_t rows_per_batch,
                      int32_t batch, int32_t D, tfx_stream stream);

/* ---- seam blend of the tiled VAE (AutoencoderKL.blend_v / blend_h, D/models/autoencoders/autoencoder_kl.py:334-344), NHWC bf16,
 *      in place on b: for t in [0, extent), u in [0, len):  b[n][t][u][:] = bf16(bf16(a[n][t][u][:] * (1 - t/extent)) +
 *      bf16(b[n][t][u][:] * (t/extent)))  (the reference's python-float weights in fp32, its three bf16 roundings).  t walks rows for
 *      the vertical blend and columns for the horizontal one: *_tstride / *_ustride are the element strides of t and u, `a` points at
 *      the first of the neighbour tile's last `extent` rows (columns).  C % 8 == 0. */
int tfx_blend_edge_nhwc(const void* a, int64_t a_bstride, int64_t a_tstride, int64_t a_ustride, void* b, int64_t b_bstride,
                        int64_t b_tstride, int64_t b_ustride, int32_t batch, int32_t extent, int32_t len, int32_t C, tfx_stream stream);

/* ---- joint attention softmax(q k^T * scale) v, head_dim 128, no mask (F.scaled_dot_product_attention,
 *      D/models/attention_processor.py:2039-2041).  Element (b, n, h, d) of q is q[b*q_bstride + n*ldq + h*128 + d];
 *      same for k, v, o.  o may alias q. */
typedef struct tfx_attn_args {
  const void* q; const void* k; const void* v; void* o;
  int64_t ldq, ldk, ldv, ldo;
  int64_t q_bstride, k_bstride, v_bstride, o_bstride;
  int32_t B, H, N;
  float scale;
  /* optional promise of the caller: |scale * q . k| <= score_bound for every (query, key) pair, 0 = unknown.  Softmax does not
   * depend on the reference that is subtracted before the exponential; when score_bound * log2(e) + log2(N) + 24 <= 126 (P1024's
   * N = 4608: score_bound <= 62.2; every weight 2^+-90 at most, and a row's sum over N keys times |v| up to 2^24 stays inside the
   * exponent range fp32 and bf16 share) the kernel subtracts none: no running row maximum, no rescaling branch.  tfx_dit_forward
   * takes the bound per block from that block's q / k RMSNorm weights (after the norm |q| <= sqrt(128) max|w_q|, RoPE preserves
   * it).  A wrong promise can overflow to inf / NaN; 0 (or a bound beyond the limit) keeps the kernel's own overflow guard. */
  float score_bound;
  /* optional scratch (ABI 8; NULL = none), 16-byte aligned, 2 * 256 * 256 * 132 * 4 = 69.2 MB for any shape: lets the head-dim-128 kernel deal
   * (item, 64-key tile) units to the CUs instead of whole (b, h, 256-query) items ("attention_streamk", tfx_set_option) when that fills
   * the chip better; contents are scratch, the launch's own stream orders its uses.  tfx_dit_forward passes the split-K scratch. */
  void* workspace; int64_t workspace_bytes;
  /* optional (ABI 10; NULL = every sample has N rows), mixed-geometry batches: DEVICE int32 [B], sample b's valid length L = seq_len[b].
   * Queries [0, L) attend to keys [0, L); K / V rows >= L are never read (the sample's buffer descriptors end at row L, so a ragged
   * last key tile masks as a ragged N does), rows >= L of o are not written, and (b, h, 256-query) items that start at or beyond L are
   * skipped.  Sample b computes, bit for bit, what a launch with B = 1, N = L on its rows computes in whole-item form.  The lengths
   * are read by the kernel when it runs: a captured graph sees new lengths without re-capture; each value is clamped to [1, N]
   * before use, so a bad value cannot address outside the operands.  Launch form: whole items only -- neither the stream-K dealing
   * nor the tail split is taken (tfx_attention_mode_counts entry 8 stays 0 for such launches); score_bound is judged with the
   * launch N; "attention_waves" 30 (the default kernel) only, any other value with seq_len is refused.  No reference counterpart:
   * the reference pads nothing, it runs one geometry per call. */
  const int32_t* seq_len;
} tfx_attn_args;
int tfx_joint_attention(const tfx_attn_args* args, tfx_stream stream);

/* ---- scheduler steps on packed latents x [rows, C] with model output v [rows, C]; the result is also written
 *      into columns [0, C) of xin [rows, ldxin] when xin != NULL (next x_embedder input; replaces the torch.cat of
 *      D/pipelines/flux/pipeline_flux_fill.py:2085).  The step index is *step_ptr (device int) when step_ptr != NULL,
 *      else `step`.
 *      Euler: coef[step] = sigma_{i+1} - sigma_i  (FlowMatchEulerDiscreteScheduler.step,
 *             D/schedulers/scheduling_flow_match_euler_discrete.py:319-330)
 *      AMO:   coef[3*step..] = {t_over - t, a, b}, noise fp32 [rows, C]  (StochasticRFOvershotDiscreteScheduler.step,
 *             D/schedulers/scheduling_stochastic_rf_discrete_overshot.py:306-361 with attn_map None). */
int tfx_euler_step(const void* v, void* x, void* xin, int64_t ldxin, int32_t C, int64_t rows, const float* coef,
                   const int32_t* step_ptr, int32_t step, tfx_stream stream);
int tfx_amo_step(const void* v, void* x, void* xin, int64_t ldxin, int32_t C, int64_t rows, const float* coef,
                 const int32_t* step_ptr, int32_t step, const float* noise, tfx_stream stream);
/* ---- second-order multistep sampler (DESIGN.md section 4 "Multistep sampler"; no reference counterpart): the Adams-Bashforth
 *      update on the same layout, with the same xin mirror and step index as the two steps above.  Added without a new
 *      TFX_ABI_VERSION: three new entry points (this one and tfx_dit_step_run_multistep / tfx_dit_step_capture_multistep below), no
 *      stamped struct and no existing entry point changes.  coef fp32 [n_steps][2], (c0, c1) = coef[2 step], coef[2 step + 1];
 *      v_prev bf16 [rows, C], the previous step's model output, caller-owned, not NULL and aliasing neither v nor x:
 *        step 0:  x <- bf16( f32(x) + c0 f32(v) )                          v_prev is not read (a fresh buffer may hold NaN)
 *        step s:  x <- bf16( f32(x) + (c0 f32(v) + c1 f32(v_prev)) )       each product and sum rounded to fp32 on its own
 *      then v_prev <- v.  C a positive multiple of 8, rows >= 0 (rows C == 0 launches nothing), ldxin % 8 == 0 and ldxin >= C. */
int tfx_multistep_step(const void* v, void* x, void* xin, int64_t ldxin, int32_t C, int64_t rows, const float* coef,
                       const int32_t* step_ptr, int32_t step, void* v_prev, tfx_stream stream);
/* ---- known-region blend (DESIGN.md section 4 "Known-region sampling"; the loop of FluxInpaintPipeline, D/pipelines/flux/
 *      pipeline_flux_inpaint.py:974-984, with scale_noise of scheduling_flow_match_euler_discrete.py:174): behind a sampler update,
 *      what lies outside the mask becomes the original's latents noised to the next sigma.  x bf16 [rows, C] with row pitch ldx
 *      (elements); x0, noise, mask bf16 [rows, C] contiguous; keep_sigma fp32 [n_steps], entry i = sigma_{i+1} ALREADY ROUNDED TO
 *      BF16, a NEGATIVE entry = "no noise" (the reference's last step); s = keep_sigma[*step_ptr or step].  Every op in fp32 on bf16
 *      operands, rounded to bf16 on its own:
 *        a = bf16(s noise)  u = bf16(1 - s)  b = bf16(u x0)  p = bf16(a + b)   (s < 0: p = x0)
 *        w = bf16(1 - mask) c = bf16(w p)    d = bf16(mask x)                  x <- bf16(c + d)
 *      written to x and, when xin != NULL, into columns [0, C) of xin (row pitch ldxin).  No shortcut for binary masks.  Refused: C
 *      not a positive multiple of 8; ldx (ldxin) not a multiple of 8 or < C; a null or not 16-byte aligned pointer; x0 / noise / mask
 *      overlapping x.  rows == 0 launches nothing.  No new TFX_ABI_VERSION: new entry points only. */
int tfx_known_region_blend(void* x, int64_t ldx, const void* x0, const void* noise, const void* mask, int32_t C, int64_t rows,
                           const float* keep_sigma, const int32_t* step_ptr, int32_t step, void* xin, int64_t ldxin, tfx_stream stream);
/* ---- change-map blend (DESIGN.md section 4 "Change-map sampling"; the loop of FluxDifferentialImg2ImgPipeline, D/examples/community/
 *      pipeline_flux_differential_img2img.py:974-986): tfx_known_region_blend with the mask decided on the device from the step cursor.
 *      hold u8 [rows, 4] (4-byte aligned; tfx_change_map_pack: 255 - map per latent pixel of the token's 2x2 patch), cut int32 [n_steps]
 *      (schedulers.change_cut_table).  With i = *step_ptr or step, s = keep_sigma[i], k = (hold[r, c & 3] > cut[i]) ? 1 : 0 for column c
 *      and p as above (s < 0: p = x0):
 *        e = bf16(p k)  w = bf16(1 - k)  d = bf16(x w)  x <- bf16(e + d)
 *      the reference's line 985 op by op, no select, so signed zeros come out as the reference's.  cut[i] >= 255: nothing is held and x
 *      is NOT written (the reference's last step leaves the latents alone; e + d would turn -0 into +0); xin != NULL is still mirrored.
 *      Refused: as tfx_known_region_blend, plus a null or misaligned hold / cut, and hold overlapping x or xin.  rows == 0 launches
 *      nothing.  No new TFX_ABI_VERSION: new entry points only. */
int tfx_change_map_blend(void* x, int64_t ldx, const void* x0, const void* noise, const void* hold, const int32_t* cut, int32_t C,
                         int64_t rows, const float* keep_sigma, const int32_t* step_ptr, int32_t step, void* xin, int64_t ldxin,
                         tfx_stream stream);
/* ---- true CFG combine (DESIGN.md section 4 "True CFG"; D/examples/community/pipeline_flux_with_cfg.py:808, noise_pred = neg +
 *      true_cfg * (pos - neg) on bf16 tensors): v_neg, v_pos, out bf16 [rows, C] contiguous, g = *scale a DEVICE fp32 read when the kernel
 *      runs.  Every torch op rounds on its own and the Python float takes part as fp32:
 *        d = bf16(f32(pos) - f32(neg))   m = bf16(g f32(d))   out = bf16(f32(neg) + f32(m))
 *      out may be v_neg itself (in place).  Refused: C not a positive multiple of 8; a null or not 16-byte aligned tensor pointer, a null or
 *      not 4-byte aligned scale; out overlapping v_pos; out partly overlapping v_neg; scale inside out.  rows == 0 launches nothing.  No new
 *      TFX_ABI_VERSION: new entry points only. */
int tfx_cfg_combine(const void* v_neg, const void* v_pos, void* out, int32_t C, int64_t rows, const float* scale, tfx_stream stream);
/* ---- clean-image estimate (DESIGN.md section 4 "Candidates"): what a flow-matching state would decode to if the model's output held
 *      for the rest of the way, `latents - sigma * noise_pred` on bf16 tensors with a Python float.  x bf16 [rows, C] with row pitch ldx (so
 *      that it also reads the latents kept in xin[:, :C]), v and out bf16 [rows, C] contiguous, sigma fp32 [n_steps + 1] on the DEVICE.
 *      With i = *step_ptr when step_ptr is given, else step, and s = sigma[i]; every torch op rounds on its own and the Python float takes
 *      part as fp32, no FMA contraction:
 *        m = bf16(s f32(v))   out = bf16(f32(x) - f32(m))
 *      A NaN stays a NaN (its payload is not pinned).  Refused: C not a positive multiple of 8; ldx not a multiple of 8 or below C; a
 *      negative row count; a null or not 16-byte aligned x, v or out; a null or not 4-byte aligned sigma or step_ptr; out overlapping x
 *      or v.  rows == 0 launches nothing.  No new TFX_ABI_VERSION: new entry points only. */
int tfx_x0_predict(const void* x, int64_t ldx, const void* v, void* out, int32_t C, int64_t rows, const float* sigma, const int32_t* step_ptr,
                   int32_t step, tfx_stream stream);

/* ---- small ops of the conditioning path (CombinedTimestepGuidanceTextProjEmbeddings, D/models/embeddings.py:1327-1339) */
int tfx_timestep_embedding(const float* t, void* out /* [n,256] = cos|sin */, int32_t n, tfx_stream stream);
int tfx_silu(const void* a, void* out, int64_t n, tfx_stream stream);
int tfx_add(const void* a, const void* b, void* out, int64_t n, tfx_stream stream);
/* dst[r, col0 : col0+C] = src[r, :]  (initial fill of the x_embedder input; C, col0, ld multiples of 8; src, dst 16-byte aligned) */
int tfx_scatter_cols(const void* src, void* dst, int64_t rows, int32_t C, int64_t ld, int32_t col0, tfx_stream stream);
/* generic strided 2-D copy dst[b][r, 0:cols] = src[b][r, 0:cols]  (cols % 8 == 0; src, dst 16-byte aligned) */
int tfx_copy_rows(const void* src, int64_t src_ld, int64_t src_bstride, void* dst, int64_t dst_ld, int64_t dst_bstride,
                  int32_t rows, int32_t cols, int32_t batch, tfx_stream stream);
/* device-side step cursor for single-graph replay: cur[:] = table[*step_ptr][:] (tfx_select_step; per_step_elems a non-negative
 * multiple of 8, table and cur 16-byte aligned), *step_ptr += 1 (tfx_advance_step) */
int tfx_select_step(const void* table, void* cur, int64_t per_step_elems, int32_t* step_ptr, tfx_stream stream);
int tfx_advance_step(int32_t* step_ptr, tfx_stream stream);

/* ---- one full FluxTransformer2DModel.forward (D/models/transformers/transformer_flux.py:1028-1212) ------------------
 * Weight layout (all bf16, nn.Linear [out,in]); fusions are pure row concatenations done at load time:
 *   double block: qkv_img = [to_k; to_v; to_q] (3D x D), qkv_txt = [add_k_proj; add_v_proj; add_q_proj],
 *                 out_img = to_out.0, out_txt = to_add_out, ff1/ff2 = ff.net.0.proj / ff.net.2 (and ff_context)
 *   single block: qkv_mlp = [to_k; to_v; to_q; proj_mlp] (7D x D), proj_out (D x 5D: attn | mlp columns)
 * Modulation: mod [B][mod_len] for THIS step = Linear(SiLU(temb)) of every norm*.linear stacked in the order
 *   double i: [img: shift_msa scale_msa gate_msa shift_mlp scale_mlp gate_mlp | txt: same six]   (12D each)
 *   single j: [shift scale gate] (3D each), then norm_out: [scale shift] (2D).
 * Workspace (caller-owned, bf16): hid [B][N,D], xn [B][N,D], y [B][N,7D], with N = T + S (text rows first). */
/* w8 / w8_scale (optional, may be NULL): the same weight as e4m3 bytes [out,in] with one fp32 scale per output channel
 * (tfx_quantize_rows_fp8 of w); used when tfx_dit_desc.flags bit 2 is set and in % 256 == 0, see below. */
/* ABI 9, runtime (unmerged) LoRA adapters on a block Linear (all 0 / NULL = none: the forward then issues exactly the launches it always
 * did).  ldw: row pitch of w in elements (0 = in_features); an adapted Linear keeps its up-projection rows Bcat [out, lora_r] BEHIND its
 * weight rows, columns [in, in + lora_r) of w (ldw >= in + lora_r); the two Linears of a double block's [img; txt] pair share ldw and
 * lora_r when either is adapted.  lora_a: Acat [lora_nseg * lora_r, in] bf16, the segments' zero-padded A stacked (segment = one
 * reference Linear of the fused weight: D output columns each; 1 segment = the whole Linear); lora_r 128 or 256; lora_mask bit s =
 * segment s is adapted; lora_scale_off: index of this Linear's lora_nseg * lora_r factors c in tfx_dit_desc.lora_scale (a multiple of 4).
 * The Linear then runs as  t = bf16(c * (x @ Acat^T))  (tfx_gemm_bf16, epilogue 4)  +  tfx_gemm_bf16_lora.  Block Linears only: the
 * fields are ignored for x_embedder / proj_out of tfx_dit_desc.  Not with flags bit 2 (fp8 linears): refused. */
typedef struct tfx_linear {
  const void* w; const void* b; const void* w8; const float* w8_scale;
  int64_t ldw;
  const void* lora_a;
  int32_t lora_r, lora_nseg, lora_mask, lora_scale_off;
} tfx_linear;
/* attn_score_bound (ABI 6, optional): tfx_attn_args.score_bound of THIS block's attention launch, from this block's own q / k
 * RMSNorm weights -- 128 * max(max|norm_q|, max|norm_added_q|) * max(max|norm_k|, max|norm_added_k|) * 128^-0.5 (+ rounding margin).
 * 0 = unknown: the launch falls back to tfx_dit_desc.attn_score_bound (0 there too = no promise).  Per block, so that one block
 * with large norm scales only changes the form of its own attention launch. */
typedef struct tfx_double_block {
  tfx_linear qkv_img, qkv_txt, out_img, out_txt, ff1_img, ff2_img, ff1_txt, ff2_txt;
  const void *norm_q, *norm_k, *norm_added_q, *norm_added_k;
  float attn_score_bound;
} tfx_double_block;
typedef struct tfx_single_block {
  tfx_linear qkv_mlp, proj_out;
  const void *norm_q, *norm_k;
  float attn_score_bound;
} tfx_single_block;
typedef struct tfx_dit_desc {
  int32_t D, H, in_channels, out_channels, n_double, n_single;
  int32_t B, S, T;
  tfx_linear x_embedder, proj_out;
  const tfx_double_block* dbl;   /* host array [n_double] */
  const tfx_single_block* sgl;   /* host array [n_single] */
  const void* xin;               /* [B][S, in_channels] */
  const void* ctx0;              /* [B][T, D] context_embedder output (step invariant) */
  const void* mod; int64_t mod_bstride;
  const float* cos_tab; const float* sin_tab;  /* fp32 [N,128] */
  void* hid; void* xn; void* y;
  void* out;                     /* [B][S, out_channels] */
  /* Partial runs (block-level parity tests): blocks [first_block, last_block) of the n_double + n_single sequence
   * (last_block < 0 = all); flags bit 0: skip x_embedder / ctx0 copy (hid is preloaded with [text | image] rows),
   * bit 1: skip norm_out + proj_out.  A full forward is first_block = 0, last_block = -1, flags = 0. */
  int32_t first_block, last_block, flags;
  /* flags bit 2 (BASELINE config 5, fp8 linears): every block Linear that carries w8 runs as
   * tfx_quantize_rows_fp8(activations) -> tfx_gemm_fp8; q8 [B][N, 5D] bytes and q8_scale [B][N] fp32 are the
   * caller-owned workspace of the quantised activations.  Embedders, modulation and proj_out stay bf16. */
  void* q8; float* q8_scale;
  void* gemm_workspace; int64_t gemm_workspace_bytes;   /* optional, passed to every block Linear (tfx_gemm_args.workspace) */
  /* optional: the rotary table as (cos, sin) pairs, fp32 [N, 64, 2] (cos_tab / sin_tab hold every value twice: pair i =
   * columns 2i, 2i + 1).  When set, the q | k | v (| mlp) projections with at least as many 256 x 256 tiles as the device
   * has CUs apply the per-head RMSNorm + RoPE in their GEMM epilogue (bf16 mode, and since round 5 the fp8 mode of flags bit 2);
   * the others -- and every projection when this is NULL -- are followed by tfx_rmsnorm_rope as a separate pass.  Same rounding
   * points either way. */
  const float* rope_cs;
  /* optional: the flow-matching Euler update fused into proj_out's epilogue (scheduling_flow_match_euler_discrete.py:319-330:
   * x' = x + (sigma_next - sigma) * v).  euler_gate: bf16 [B][out_channels] rows (row stride euler_gate_bstride elements), every
   * element = the step's bf16-rounded dsigma.  When set, the final projection runs with the gated-residual epilogue --
   * xin[:, :, :out_channels] <- xin[:, :, :out_channels] + bf16(dsigma * bf16(proj_out(...))), the reference's rounding points,
   * bit-identical to tfx_euler_step on the stored model output -- i.e. the latent state lives IN the x_embedder input, `out` is
   * not written, and there is neither a scheduler launch nor a copy of the new latents into the next step's input. */
  const void* euler_gate; int64_t euler_gate_bstride;
  /* optional: tfx_attn_args.score_bound for the attention launches of blocks whose own attn_score_bound is 0 (0 = unknown).  The
   * caller derives it from the q / k RMSNorm weights: 128 * max|w_q| * max|w_k| * 128^-0.5 (text-stream norms included), see
   * tfx_attn_args; since ABI 6 the per-block fields are the ones the engine fills. */
  float attn_score_bound;
  /* ABI 10, mixed-geometry batches (NULL / 0 = every sample has S image rows: the forward then issues exactly the launches it
   * always did).  Placement: in front of the runtime-LoRA fields, not behind them -- those three are addressed as the struct's LAST
   * fields by bindings written against ABI 9 (this repository's own ctypes mirror is checked for it), so the struct grows in front of
   * them; either way offsets or size change, and a library and a binding of different ABI versions refuse each other (tfx_abi_info).
   * Sample b's rows are [T text rows | S_b image rows | padding]: S is the PADDED image row count (T + S a multiple of 256 keeps
   * the GEMMs on whole tiles), seq_len a DEVICE int32 [B] holding T + S_b, read by the attention kernel at run time (tfx_attn_args.seq_len;
   * a captured step graph serves every mix of lengths up to its size).  rope_bstride: table rows between two samples' rotary tables in
   * cos_tab / sin_tab / rope_cs (each [B][>= T + S rows]), passed to every fused q | k | v projection (tfx_qkn_args.rope_bstride) and to
   * the separate norm + RoPE pass (tfx_rmsnorm_rope_batched); required (> 0) with seq_len.  Everything else of the forward is row-wise:
   * padded rows of xin / hid hold unspecified values, influence no valid row, and their rows of out / xin mean nothing.  fp8 linears
   * and runtime LoRA adapters work unchanged.  In a tfx_dit_step_* call seq_len needs sampler 2: only the fused Euler form carries
   * per-sample coefficients (the dsigma rows of euler_gate), and a sample's sigma schedule depends on its own S_b
   * (calculate_shift, D/pipelines/flux/pipeline_flux_fill.py:1980-1990). */
  const int32_t* seq_len; int64_t rope_bstride;
  /* ABI 9: scratch and factors of the runtime LoRA adapters (required when any block Linear carries lora_a).  lora_t_xn / lora_t_y hold
   * the down projections T of Linears whose input lives in xn / in y: T of input A sits at A + (lora_t_xn - xn) resp. A + (lora_t_y - y),
   * so each region mirrors its buffer's shape -- lora_t_xn: 1 (D >= 1024) or 4 (smaller D: one per segment) matrices [B][N, D],
   * lora_t_y: [B][N, 7D] -- and must lie ABOVE it within 4 GiB - 64 KiB, end included (tfx_workspace_layout flags bit 3 places them).
   * lora_scale: fp32 device vector of every adapted Linear's factors c = call scale * adapter weight * alpha / r, read by the
   * kernels when they run: rewriting it changes the strength of the next forward / graph replay, nothing is re-captured. */
  void* lora_t_xn; void* lora_t_y; const float* lora_scale;
} tfx_dit_desc;
int tfx_dit_forward(const tfx_dit_desc* desc, tfx_stream stream);

/* Caller-owned workspace of tfx_dit_forward for one problem size, as ONE allocation: total bytes, and the byte offsets
 * (256-byte aligned) of its parts in off[0..5] = hid, xn, y, q8, q8_scale, gemm_workspace (q8 / q8_scale only when
 * flags bit 2 (fp8 linears) is set, else -1); *gemm_workspace_bytes = size of the split-K / stream-K scratch (128 MiB).  flags bit 3
 * (ABI 9, runtime LoRA adapters): `off` has 8 entries, off[6] / off[7] = lora_t_xn / lora_t_y, appended BEHIND the parts above (whose
 * offsets do not change); without the bit only off[0..5] are written and the total is what it always was.  Host-side
 * arithmetic only, no GPU needed.  ("never allocate persistent memory except through an explicit
 * workspace the Python side owns".) */
int64_t tfx_workspace_bytes(int32_t B, int32_t S, int32_t T, int32_t D, int32_t flags);
int tfx_workspace_layout(int32_t B, int32_t S, int32_t T, int32_t D, int32_t flags, int64_t* off, int64_t* gemm_workspace_bytes);

/* ---- one denoising step = modulation rows of step *step_ptr -> tfx_dit_forward -> scheduler update -> ++*step_ptr, and
 *      its capture into a hipGraph (D/pipelines/flux/pipeline_flux_fill.py:2077-2116: the loop body; the reference issues
 *      ~4.5 k launches per step from Python, here a step is ONE hipGraphLaunch).  The step index lives on the device, so the
 *      same graph serves every step: mod_table [n_steps][B][mod_len] (tfx_dit_desc.mod must point at mod_cur, which the step
 *      refreshes from the table), coef as for tfx_euler_step / tfx_amo_step (sampler 0 / 1), noise fp32 [B*S, out_channels]
 *      (AMO only; rewritten by the caller between replays), latents [B*S, out_channels] updated in place and mirrored into
 *      columns [0, out_channels) of dit.xin.
 *      tfx_dit_step_run: the eager form (call it at least once before capturing: first launches size LDS limits).
 *      tfx_dit_step_capture: records the same launches on `stream` (must not be the NULL stream) in thread-local capture
 *      mode and instantiates them; tfx_dit_step_replay launches the instantiated graph; tfx_graph_destroy frees it.
 *      All pointers of the descriptor are baked into the graph: they must stay valid (and unmoved) while it is replayed. */
/* ABI 11, the first-block step cache (no reference counterpart; DESIGN.md section 4 "Step cache"): buffers of a step loop that may skip the
 * block stack on steps whose first-block residual barely moved.  All four are bf16 [B][S, ld] over the IMAGE rows of the joint stream
 * (row pitch ld >= D, batch stride bstride, both multiples of 8 elements, 16-byte aligned): x0 = hid[img] before block 0, overwritten
 * by the first-block residual f; f_prev = f of the last computed step; h1 = hid[img] behind block 0; r = the residual of blocks
 * 1 ... end of the last computed step.  partials: fp32 scratch of at least 2048 * B bytes (the per-workgroup sums of the metric);
 * metric: DEVICE fp32 [B], the head phase's result.  Caller-owned like every other buffer. */
typedef struct tfx_step_cache {
  void* x0; void* f_prev; void* h1; void* r;
  int64_t ld, bstride;
  float* partials; int64_t partials_bytes;
  float* metric;
} tfx_step_cache;
/* The three passes on their own (tfx_dit_step_run issues them for phases 1 - 3 of tfx_step_desc).  hid: the image rows of the joint
 * stream as a strided view, bf16 [batch][rows, ldh] with batch stride h_bstride (inside tfx_dit_step_*: hid + T * D, D, (T + S) * D).
 * D % 8 == 0, rows / batch / D positive, every pointer 16-byte aligned and every stride a multiple of 8 elements.
 *   metric: f = bf16(f32(hid) - f32(x0)) (ONE rounding) written over x0;  h1 <- hid;  per sample b
 *           metric[b] = sum |f32(f) - f32(f_prev)| / sum |f32(f_prev)|  (+inf when the denominator is 0).  fp32 sums with a partition
 *           and an order that depend on (rows, D) alone -- per-workgroup partial sums, then one finishing workgroup per sample; no
 *           atomics: the same inputs give the same bits on every run and every device.
 *   store:  r <- bf16(f32(hid) - f32(h1));  f_prev <- x0 (which holds f).
 *   apply:  hid <- bf16(f32(hid) + f32(r)). */
int tfx_step_cache_metric(const void* hid, int64_t ldh, int64_t h_bstride, const tfx_step_cache* cache, int32_t rows, int32_t batch,
                          int32_t D, tfx_stream stream);
int tfx_step_cache_store(const void* hid, int64_t ldh, int64_t h_bstride, const tfx_step_cache* cache, int32_t rows, int32_t batch,
                         int32_t D, tfx_stream stream);
int tfx_step_cache_apply(void* hid, int64_t ldh, int64_t h_bstride, const tfx_step_cache* cache, int32_t rows, int32_t batch,
                         int32_t D, tfx_stream stream);

typedef struct tfx_step_desc {
  tfx_dit_desc dit;
  const void* mod_table; void* mod_cur; int64_t mod_step_elems;   /* elements per step = B * mod_len */
  int32_t* step_ptr;
  void* latents;
  const float* coef; const float* noise;
  int32_t sampler;                                                 /* 0 Euler, 1 AMO, 2 Euler fused into proj_out's epilogue:
                                                                      dit.euler_gate must point into mod_cur (the step's dsigma row
                                                                      travels with its modulation rows: mod_step_elems covers it), the
                                                                      latents live in dit.xin[:, :, :out_channels]; `latents` / `coef` are
                                                                      not used -- copy the result out with tfx_copy_rows after the loop */
  /* ABI 11, the step cache (NULL / 0 = one whole step, exactly the launches it always issued).  phase: 0 whole step | 1 head:
   * select_step, x_embedder + ctx0 copy, x0 <- hid[img], block 0, the metric pass (cache->metric is then read by the HOST, which
   * decides between the two tails) | 2 computed tail: blocks [1, n), norm_out / proj_out and the sampler update as in a whole step,
   * then the store pass and the cursor advance | 3 cached tail: the apply pass, norm_out / proj_out and the sampler update with no
   * block in between, the cursor advance; f_prev and r stay.  Phases 1 + 2 issue the launches of a whole step in the same order
   * (the added passes write only the cache's own buffers): a loop that never takes phase 3 is bit-equal to the plain loop.
   * Refused: a phase without cache; cache with dit.seq_len (padded rows of a mixed batch may hold NaN and would poison the sums);
   * cache with dit.first_block / last_block / flags other than the whole forward (flags bit 2 is allowed); fewer than 2 blocks. */
  const tfx_step_cache* cache;
  int32_t phase;
} tfx_step_desc;
typedef void* tfx_graph;
int tfx_dit_step_run(const tfx_step_desc* step, tfx_stream stream);
int tfx_dit_step_capture(const tfx_step_desc* step, tfx_stream stream, tfx_graph* out);
int tfx_dit_step_replay(tfx_graph graph, tfx_stream stream);
int tfx_graph_destroy(tfx_graph graph);
/* The same step with the second-order multistep update (tfx_multistep_step) where sampler 0 launches tfx_euler_step: `step` is a
 * sampler 0 descriptor (latents, coef, dit.out; neither dit.seq_len nor dit.euler_gate) whose coef is the multistep table
 * [n_steps][2]; v_prev bf16 [B*S, out_channels] is the caller's history buffer, aliasing neither latents nor dit.out.  Every
 * other launch, the phases of the step cache and the graph handle (tfx_dit_step_replay / tfx_graph_destroy) are those of
 * tfx_dit_step_run / tfx_dit_step_capture; one graph serves every step, step 0 included (the kernel branches on the device's step
 * index).  The history travels beside the descriptor, so tfx_step_desc and TFX_ABI_VERSION stay as they are. */
int tfx_dit_step_run_multistep(const tfx_step_desc* step, void* v_prev, tfx_stream stream);
int tfx_dit_step_capture_multistep(const tfx_step_desc* step, void* v_prev, tfx_stream stream, tfx_graph* out);
/* The step with what travels beside the descriptor (tfx_step_desc and TFX_ABI_VERSION stay as they are).  v_prev != NULL: the
 * multistep update, exactly tfx_dit_step_run_multistep (sampler 0 descriptor).  keep_x0 / keep_noise / keep_mask (bf16 [B*S,
 * out_channels]) and keep_sigma (fp32 [n_steps]), all set or all NULL: tfx_known_region_blend behind the sampler update and in front
 * of the step cache's store pass and the cursor advance -- on dit.xin with pitch in_channels for sampler 2 (the fused Euler keeps
 * the latents there), else on latents, mirrored into dit.xin.  Every sampler, phases 0 / 2 / 3, one graph for every step.  Refused:
 * a NULL extra, a partial keep set, keep_* with dit.seq_len, keep_* overlapping latents, dit.out, dit.xin or v_prev.  All fields
 * NULL is the plain step. */
typedef struct tfx_step_extra {
  void* v_prev;
  const void* keep_x0;
  const void* keep_noise;
  const void* keep_mask;
  const float* keep_sigma;
} tfx_step_extra;
int tfx_dit_step_run_ex(const tfx_step_desc* step, const tfx_step_extra* extra, tfx_stream stream);
int tfx_dit_step_capture_ex(const tfx_step_desc* step, const tfx_step_extra* extra, tfx_stream stream, tfx_graph* out);
/* The step with the change-map blend (DESIGN.md section 4 "Change-map sampling"): a second struct beside the descriptor, so that
 * tfx_step_extra keeps its layout.  change == NULL is tfx_dit_step_run_ex.  With change set, extra->keep_x0 / keep_noise / keep_sigma
 * must be set and keep_mask NULL; tfx_change_map_blend runs where tfx_known_region_blend runs (behind the sampler update, in front of
 * the step cache's store pass and the cursor advance; on dit.xin with pitch in_channels for sampler 2, else on latents mirrored into
 * dit.xin).  Every sampler, phases 0 / 2 / 3, one graph for every step.  Refused: dit.seq_len, and hold / cut / keep_* overlapping
 * latents, dit.out, dit.xin or v_prev. */
typedef struct tfx_step_change {
  const void* hold;     /* u8 [B*S, 4] */
  const int32_t* cut;   /* int32 [n_steps] */
} tfx_step_change;
int tfx_dit_step_run_ex2(const tfx_step_desc* step, const tfx_step_extra* extra, const tfx_step_change* change, tfx_stream stream);
int tfx_dit_step_capture_ex2(const tfx_step_desc* step, const tfx_step_extra* extra, const tfx_step_change* change, tfx_stream stream,
                             tfx_graph* out);
/* The step with true CFG (DESIGN.md section 4 "True CFG"; the loop of FluxCFGPipeline, D/examples/community/pipeline_flux_with_cfg.py:
 * 778-812): a third struct beside the descriptor, so that every other struct keeps its layout.  cfg == NULL is tfx_dit_step_run_ex2.
 * With cfg set, step->dit describes a batch of 2B: samples [0, B) carry the negative conditioning and [B, 2B) the positive (the order of
 * the reference's torch.cat); latents, noise, extra->v_prev, the keep_* buffers and hold have B * S rows.  A step is: the modulation rows,
 * tfx_dit_forward on 2B, tfx_cfg_combine over the two halves of dit.out into the first, the sampler update on B * S rows (sampler 0,
 * sampler 1 or the multistep update), the known-region or change-map blend when given, tfx_copy_rows of columns [0, out_channels) of
 * dit.xin's first half into its second (sample B + b mirrors sample b), the cursor advance.  scale: DEVICE fp32, read when the step runs
 * -- one captured graph serves every step and every scale.  Refused: sampler 2 (the fused Euler epilogue updates each half on its own),
 * dit.seq_len, a phase other than 0, an odd dit.B, a NULL or misaligned scale, scale inside a buffer the step writes. */
typedef struct tfx_step_cfg {
  const float* scale;
} tfx_step_cfg;
int tfx_dit_step_run_ex3(const tfx_step_desc* step, const tfx_step_extra* extra, const tfx_step_change* change, const tfx_step_cfg* cfg,
                         tfx_stream stream);
int tfx_dit_step_capture_ex3(const tfx_step_desc* step, const tfx_step_extra* extra, const tfx_step_change* change, const tfx_step_cfg* cfg,
                             tfx_stream stream, tfx_graph* out);

/* ---- VAE ends (AutoencoderKL, D/models/autoencoders/autoencoder_kl.py:263-332) on NHWC bf16 activations -------------
 * 3x3 convolution as an implicit GEMM on the MFMA kernel (ResnetBlock2D convs D/models/resnet.py:327-366, Upsample2D
 * nearest-2x + conv D/models/upsampling.py:142-192 with up = 2, Downsample2D pad (0,1,0,1) stride 2
 * D/models/downsampling.py:132-150 with stride = 2, pad_lo = 0).  x [B, inH, inW, Cin] (Cin % 64 == 0),
 * w [Cout, 3, 3, Cin] (KRSC) -- or the narrow form of the two conv_in layers: Cin in {8, 16, 32} with w [Cout, Kp],
 * Kp = 9 Cin rounded up to a multiple of 64, columns (tap, ci) then zeros --, out [B, H, W, Cout] = conv(x) + bias (+ res when res != NULL; may alias out),
 * zero_page: >= 128 bytes of zeros (source of out-of-image taps).  variant: -1 auto, 0 generic, 1 MFMA. */
int tfx_conv3x3_nhwc(const void* x, int32_t B, int32_t inH, int32_t inW, int32_t Cin, const void* w, const void* bias,
                     void* out, int32_t H, int32_t W, int32_t Cout, int32_t stride, int32_t up, int32_t pad_lo,
                     const void* res, const void* zero_page, int variant, tfx_stream stream);
/* The same convolution (stride 1, pad 1, no upsample) in PIXEL-PAIR form, for layers with few output channels: one GEMM row is two
 * horizontally adjacent output pixels (W even), N = 2 * Cout -- their channels are neighbours in NHWC, so `out` / `res` are the
 * ordinary [B, H, W, Cout] tensors -- and K runs over the 3 x 4 input taps the pair touches: w_pair [2 * Cout][3][4][Cin] holds,
 * for pixel o of the pair, the kernel's column dx at position dx + o and zeros elsewhere; bias_pair [2 * Cout] = the bias twice.
 * 4/3 of the FLOPs, but a 128-channel layer then fills the MFMA kernel's 256-column tile instead of half of it (VAE: the
 * full-resolution blocks of D/models/autoencoders/vae.py:60-360; same result up to fp32 summation order). */
int tfx_conv3x3_pair_nhwc(const void* x, int32_t B, int32_t H, int32_t W, int32_t Cin, const void* w_pair, const void* bias_pair,
                          void* out, int32_t Cout, const void* res, const void* zero_page, tfx_stream stream);
/* GroupNorm(groups, eps, affine) followed by SiLU when silu != 0, x/out [B, HW, C] NHWC.  workspace: fp32
 * [B * (ceil(HW/1024) + 1) * groups * 2]: the per-chunk partial sums [B, ceil(HW/1024), groups, 2] (sum, sum of squares), then the
 * statistics [B, groups, 2] = (mean, rstd = rsqrt(var + eps)) the normalisation used, left there for the caller to read.
 * groups in [1, 64], C a multiple of 8 and of groups, C / groups a multiple of 4, C / 8 a divisor of 256. */
int tfx_groupnorm_nhwc(const void* x, void* out, const void* gamma, const void* beta, float* workspace, int32_t B,
                       int64_t HW, int32_t C, int32_t groups, float eps, int32_t silu, tfx_stream stream);

/* ---- the pixel / latent layout steps around the VAE (FluxFillPipeline.__call__, D/pipelines/flux/pipeline_flux_fill.py
 *      "P:", and VaeImageProcessor, D/image_processor.py "IP:"), so that no NCHW tensor and no torch op sits between the
 *      caller's image and the encoder, or between the decoder and the caller's image.  dtype codes: 0 f32, 1 bf16, 2 u8. */
/* *flag |= 1 when any element of x is negative (IP:700-707: tensors already in [-1, 1] are not re-normalised). */
int tfx_any_negative(const void* x, int32_t dtype, int64_t n, int32_t* flag, tfx_stream stream);
/* out [B, H, W, 8] bf16 NHWC (channels >= C zero) = bf16( norm(img) * (1 - mask) ): the encoder input.  img: f32 / bf16
 * planes [B, C, H, W], or u8 interleaved [B, H, W, C] read as value / 255 (PIL branch, IP:133-154 inverse).  mask: NULL or
 * f32 / u8 [mask_batch, H, W] (mask_batch 1 or B), binarised at 0.5 when binarize != 0 (IP:535-536).  norm_mode: 0 none,
 * 1 x -> 2x - 1 (IP:221-225), 2 the same unless *neg_flag != 0.   (IP:587-716 + P:2030-2031) */
int tfx_prep_image(const void* img, int32_t img_dtype, const void* mask, int32_t mask_dtype, void* out, int32_t B, int32_t C,
                   int32_t H, int32_t W, int32_t mask_batch, int32_t norm_mode, int32_t binarize, const int32_t* neg_flag,
                   tfx_stream stream);
/* The callers' composition step on the device (reference: /root/reference/run_inference.py:409-467 and
 * scripts/run_eval.py:143-198 stack the rendered glyph image and the scene -- glyph first -- and a black mask for the glyph part
 * over the scene's mask; IP's do_convert_grayscale then takes PIL's "L" of the RGB mask): canvas [B, H, W, 3] u8 and
 * cmask [B, H, W] u8 from glyph [B, gh, gw, 3], scene [B, sh, sw, 3] and the scene's RGB mask [B, sh, sw, 3] (u8,
 * interleaved).  direction 0: vertical, H = gh + sh, W = gw = sw; 1: horizontal, W = gw + sw, H = gh = sh.  Grey value =
 * Pillow's (19595 R + 38470 G + 7471 B + 0x8000) >> 16.  mask_rgb != 0: cmask is [B, H, W, 3] and keeps the RGB values (a
 * resize follows: the reference resizes the RGB mask, then takes "L").  The outputs feed tfx_prep_image (dtype 2) /
 * tfx_pack_mask, directly or through tfx_resample_u8 + tfx_rgb_to_grey_u8. */
int tfx_compose_canvas(const void* glyph, const void* scene, const void* scene_mask_rgb, void* canvas, void* cmask, int32_t B,
                       int32_t gh, int32_t gw, int32_t sh, int32_t sw, int32_t direction, int32_t mask_rgb, tfx_stream stream);
/* out [pixels] u8 = PIL convert("L") of interleaved RGB u8 [pixels][3]. */
int tfx_rgb_to_grey_u8(const void* rgb, void* out, int64_t pixels, tfx_stream stream);
/* One pass of Pillow's 8-bit convolution resampler (PIL.Image.resize of "RGB" / "L" images; the callers' resize to a multiple
 * of 32, /root/reference/run_inference.py:65-69) along the middle axis of in [outer][in_len][inner] u8 -> out
 * [outer][out_len][inner]: horizontal pass of [B, H, W, C]: outer = B H, len = W, inner = C; vertical pass: outer = B, len = H,
 * inner = W C (Pillow runs the horizontal pass first; both round to u8).  bounds [out_len][2] = (first input index, count),
 * coeffs [out_len][ksize] = the filter weights in fixed point with 22 fractional bits, computed on the host exactly as
 * libImaging/Resample.c precompute_coeffs + normalize_coeffs_8bpc do (textflux_amd/image_processor.py::pil_resample_tables);
 * out = clip8((2^21 + sum in * k) >> 22): integer arithmetic, bit-identical to Pillow. */
int tfx_resample_u8(const void* in, void* out, const int32_t* bounds, const int32_t* coeffs, int32_t ksize, int64_t outer,
                    int32_t in_len, int32_t out_len, int32_t inner, tfx_stream stream);
/* ---- paste-back (DESIGN.md section 4 "Paste-back"): the edited pixels go back into the ORIGINAL image under a feathered mask.
 *      Added without a new TFX_ABI_VERSION: three new entry points, no stamped struct and no existing entry point changes, so a
 *      caller built against the previous header finds everything it knew unchanged.  All tensors contiguous, batch-major, u8;
 *      B, H, W (, C) >= 1; radius in [0, 255]; integer arithmetic throughout, so the results are exact.  `tmp` is the caller's
 *      scratch of the mask's size; in, out and tmp are three different buffers.
 * tfx_mask_dilate_u8: square max filter of a mask [B, H, W]: out[y, x] = max in[y', x'] over |y' - y| <= radius, |x' - x| <= radius,
 *      the window clipped at the image border (x pass into tmp, y pass into out).  radius 0 copies. */
int tfx_mask_dilate_u8(const void* in, void* out, void* tmp, int32_t B, int32_t H, int32_t W, int32_t radius, tfx_stream stream);
/* tfx_mask_feather_u8: three box passes along x, then three along y, each rounding to u8.  One pass along an axis of length L with
 *      n = 2 radius + 1: s = sum over k in [-radius, radius] of v[clamp(i + k, 0, L - 1)] (edge replicated), out = (2 s + n) / (2 n) in
 *      integer division.  radius 0 copies; an all-255 (all-0) mask stays all-255 (all-0); the support grows by at most 3 radius
 *      per axis. */
int tfx_mask_feather_u8(const void* in, void* out, void* tmp, int32_t B, int32_t H, int32_t W, int32_t radius, tfx_stream stream);
/* tfx_overlay_u8: orig, edit, out [B, H, W, C], alpha [B, H, W]: out = (orig (255 - a) + edit a + 127) / 255 in integer division:
 *      a = 0 gives orig, a = 255 gives edit, and min(orig, edit) <= out <= max(orig, edit).  out may be orig (no other aliasing). */
int tfx_overlay_u8(const void* orig, const void* edit, const void* alpha, void* out, int32_t B, int32_t H, int32_t W, int32_t C,
                   tfx_stream stream);
/* ---- colour-matched paste-back (DESIGN.md section 4 "Per-line edits"): a per-channel look-up table, fitted on the host from exact
 *      moments, takes an edit's colours to those of the unchanged surroundings before the blend.  Added without a new
 *      TFX_ABI_VERSION: two new entry points, no stamped struct and no existing entry point changes.  Tensors contiguous, batch-major,
 *      u8 unless said otherwise; B, H, W >= 1, B <= 65535, C in 1..4; integer arithmetic throughout, so the results are exact.
 * tfx_masked_moments_u8: a, b [B, H, W, C], weight [B, H, W] -> out u64 [B][C][5] = {n, sum a, sum b, sum a a, sum a b} over the pixels
 *      of the sample whose weight != 0 (n is repeated per channel).  Every sum is 64-bit; no atomics: workgroups write partial sums
 *      into `scratch`, one finishing workgroup per sample adds them, so the result does not depend on the partition.
 *      TFX_MASKED_MOMENTS_SCRATCH_BYTES bytes of scratch per sample serve every shape; scratch_bytes < B times that is refused.  out and
 *      scratch are 8-byte aligned. */
#define TFX_MASKED_MOMENTS_SCRATCH_BYTES 34816
int tfx_masked_moments_u8(const void* a, const void* b, const void* weight, void* out, void* scratch, int64_t scratch_bytes, int32_t B,
                          int32_t H, int32_t W, int32_t C, tfx_stream stream);
/* tfx_overlay_lut_u8: tfx_overlay_u8 with the edit sent through lut u8 [B][C][256] first:
 *      out = (orig (255 - a) + lut[b][c][edit] a + 127) / 255 in integer division.  With the identity table it is tfx_overlay_u8 bit
 *      for bit.  out may be orig (no other aliasing). */
int tfx_overlay_lut_u8(const void* orig, const void* edit, const void* alpha, const void* lut, void* out, int32_t B, int32_t H, int32_t W,
                       int32_t C, tfx_stream stream);
/* ---- seamless paste (DESIGN.md section 4 "Seamless paste"): before the blend the edit is corrected by a membrane, the difference
 *      ref - edit known just outside the blend and interpolated smoothly across alpha's support by a pull-push pyramid, so that the edit
 *      meets the scene at the seam and keeps its own gradients inside.  Added without a new TFX_ABI_VERSION: two new entry points (one of
 *      them host arithmetic), no stamped struct and no existing entry point changes.  Tensors contiguous, batch-major, u8; B, H, W >= 1,
 *      B <= 65535, C in 1..4; smooth and max_shift in [0, 255]; integer arithmetic throughout, so the results are exact.
 * tfx_seamless_workspace_bytes: the bytes of `workspace` the call below needs for this geometry (host arithmetic, no device is touched);
 *      -1 with tfx_last_error for a geometry outside the contract.
 * tfx_seamless_overlay_u8: orig, ref, edit, out [B, H, W, C], alpha [B, H, W], covered [B, H, W] or NULL, lut [B][C][256] or NULL.  Per
 *      sample and channel, in integers (// is floor division, >> an arithmetic shift):
 *          e = lut[b][c][edit] with a table, else edit
 *          free  = alpha > 0;   known = alpha == 0 and (covered == NULL or covered != 0);   the rest is neither
 *          level 0 (H, W):  v = (ref - e) * 64 on the known pixels (|v| <= 16320: i16), filled = known
 *          pull, level l (h, w) -> l + 1 ((h + 1) / 2, (w + 1) / 2), until the level is 1 x 1: of a coarse pixel's up to four in-bounds
 *                   children the n filled ones with the sum s of their values: filled iff n > 0, value (2 s + n) // (2 n), 0 when n = 0
 *          top:     an unfilled 1 x 1 level holds 0 (nothing known: the membrane is 0 everywhere)
 *          push, top down: every unfilled pixel (y, x) of level l takes the 2x upsample of the completed level l + 1 (hc, wc) = c:
 *                   i = y >> 1, i2 = clamp(i + (y & 1 ? 1 : -1), 0, hc - 1);  j, j2 alike from x
 *                   v = (9 c[i, j] + 3 c[i, j2] + 3 c[i2, j] + c[i2, j2] + 8) >> 4;   filled pixels keep their values
 *          smooth:  `smooth` Jacobi sweeps at level 0 between two buffers (no pixel depends on the update order): a free pixel becomes
 *                   (N + S + E + W + 2) >> 2, a neighbour outside the window counting as the pixel's own value; all others stay
 *          apply:   d = clamp((v + 32) >> 6, -max_shift, max_shift),  e' = clamp(e + d, 0, 255)
 *                   out = (orig (255 - a) + e' a + 127) / 255 where a = alpha > 0,  out = orig where alpha == 0
 *      Hence, exactly: a difference that is one constant k on the known set gives v = 64 k everywhere; every v lies between the least and
 *      the greatest known value; max_shift = 0 is tfx_overlay_lut_u8 (tfx_overlay_u8 without a table) bit for bit, and so is a call with
 *      nothing known; alpha == 0 everywhere gives orig.  ref is the image the difference is taken against: orig itself, or, when the edit
 *      was generated from an earlier state of the scene than the one it is blended over, that earlier state.
 *      out may be orig and ref may be orig (no other aliasing).  workspace: 16-byte aligned, workspace_bytes at least
 *      tfx_seamless_workspace_bytes(B, H, W, C), else the call is refused; nothing in it survives the call.  No atomics; every launch
 *      goes on `stream`.  Every neighbour index is clamped as written above and every offset that can pass 2^31 is formed in 64 bits, so
 *      the call is memory-safe whatever the masks hold. */
int64_t tfx_seamless_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t C);
int tfx_seamless_overlay_u8(const void* orig, const void* ref, const void* edit, const void* alpha, const void* covered, const void* lut,
                            void* out, void* workspace, int64_t workspace_bytes, int32_t B, int32_t H, int32_t W, int32_t C, int32_t smooth,
                            int32_t max_shift, tfx_stream stream);
/* ---- grain match (DESIGN.md section 4 "Grain match"): a pasted edit is cleaner than the photo around it; the noise level of both is
 *      estimated from the histogram of a high-pass residual, and the missing variance is added as hashed white grain under the blend's
 *      alpha.  Added without a new TFX_ABI_VERSION: two new entry points, no stamped struct and no existing entry point changes.  Tensors
 *      contiguous, batch-major, u8 unless said otherwise; B, H, W >= 1, B <= 65535, C in 1..4; integer arithmetic throughout, so the
 *      results are exact.  Every neighbour index is clamped and every offset that can pass 2^31 is formed in 64 bits; every launch goes on
 *      `stream`.
 * tfx_highpass_hist_u8: img [B, H, W, C], sel [B, H, W] -> out u32 [B][C][1024].  A pixel is selected when lo <= sel <= hi.  For every
 *      selected pixel and channel v = |16 p - sum w p'| with w = [1 2 1] x [1 2 1] over the 3 x 3 neighbourhood, its indices clamped to the
 *      image (edge replicated), and out[b][c][min(v, 1023)] += 1.  The call zeroes out itself (4-byte aligned; no aliasing with img or
 *      sel); nothing selected gives all zeros; each channel's bins sum to the number of selected pixels.  Workgroups count in LDS and add
 *      their bins with integer atomics, so the result does not depend on the partition.  H W < 2^32 (the counts are 32-bit). */
int tfx_highpass_hist_u8(const void* img, const void* sel, int32_t lo, int32_t hi, void* out, int32_t B, int32_t H, int32_t W, int32_t C,
                         tfx_stream stream);
/* tfx_grain_u8: img, out [B, H, W, C], alpha [B, H, W], gain i32 [B][C] and origin i32 [B][2] = (x, y) (NULL: (0, 0)) DEVICE pointers.  Per
 *      byte, with x = origin_x + column and y = origin_y + row, the pixel's SCENE coordinates, all in uint32 wrap-around arithmetic:
 *          mix(h): h ^= h >> 16; h *= 0x7feb352d; h ^= h >> 15; h *= 0x846ca68b; h ^= h >> 16
 *          h = mix(mix(x * 0x9E3779B1 + y * 0x85EBCA77 + c * 0xC2B2AE3D) ^ seed)
 *          n = (h & 255) + ((h >> 8) & 255) + ((h >> 16) & 255) + (h >> 24) - 510        in [-510, 510], standard deviation 147.8005
 *          d = floor((n gain[b][c] alpha + 255 * 32768) / (255 * 65536))                  floor division in 64 bits
 *          out = clamp(img + d, 0, 255)
 *      gain is sigma / 147.8005 in Q16, in [0, 65536]: the caller refuses what lies outside (ops.grain does); the kernel clamps it into
 *      that range.  Hence, exactly: alpha == 0 leaves the byte unchanged, gain == 0 copies, and the grain of a scene pixel does not depend
 *      on the window that contains it.  out may be img (no other aliasing). */
int tfx_grain_u8(const void* img, const void* alpha, const int32_t* gain, const int32_t* origin, uint32_t seed, void* out, int32_t B,
                 int32_t H, int32_t W, int32_t C, tfx_stream stream);
/* ---- grain spectrum (DESIGN.md section 4 "Grain spectrum"): camera noise after demosaicing and JPEG is correlated over two or three
 *      pixels and mostly shared by the channels; white grain is neither.  The blur and the shared part are estimated from histograms at two
 *      neighbour distances and of the channel sum, and the grain is shaped to match.  Added without a new TFX_ABI_VERSION: two new entry
 *      points, no stamped struct and no existing entry point changes.  Geometry, alignment and aliasing rules as in the grain match above.
 * tfx_highpass_hist_step_u8: img [B, H, W, C], sel [B, H, W] -> out u32 [B][C + 1][1024]; step in 1..8.  For every pixel with
 *      lo <= sel <= hi and every channel r_c = 16 p - sum w p'(x +- step, y +- step), w = [1 2 1] x [1 2 1] with the eight neighbours taken
 *      at distance step (the a-trous form), their indices clamped to the image, and out[b][c][min(|r_c|, 1023)] += 1; row C counts the
 *      signed residuals summed over the channels: out[b][C][min(|sum_c r_c|, 1023)] += 1.  The call zeroes out itself; nothing selected
 *      gives all zeros; every row sums to the number of selected pixels; counted in LDS and added with integer atomics, so the result does
 *      not depend on the partition.  With step == 1 rows 0..C-1 are tfx_highpass_hist_u8's, bit for bit. */
int tfx_highpass_hist_step_u8(const void* img, const void* sel, int32_t lo, int32_t hi, int32_t step, void* out, int32_t B, int32_t H, int32_t W,
                              int32_t C, tfx_stream stream);
/* tfx_grain_shaped_u8: as tfx_grain_u8, with shape i32 [B][2] = (s, lam) a DEVICE pointer, s in [0, 64], lam in [0, 256], and gain in
 *      [0, 2^18].  With n(x, y, c) the hash of tfx_grain_u8 and nL(x, y) = n(x, y, 255), a channel index that no image channel has, at SCENE
 *      coordinates in uint32 wrap-around arithmetic (neighbours are never clamped to the window):
 *          m(x, y, c) = (256 - lam) n(x, y, c) + lam nL(x, y)                                   Q8, |m| <= 130560
 *          k = [s, 256 - 2 s, s]
 *          f(x, y, c) = sum over dy, dx in {-1, 0, 1} of k[dy + 1] k[dx + 1] m(x + dx, y + dy, c)   Q24, 64 bits
 *          d = floor((f gain[b][c] alpha + 255 * 2^39) / (255 * 2^40))                          floor division in 64 bits
 *          out = clamp(img + d, 0, 255)
 *      |f gain alpha| <= 130560 * 2^16 * 2^18 * 255 < 2^59.  The caller refuses gain, s and lam outside their ranges (ops.grain_shaped
 *      does); the kernel clamps them into them.  Hence, exactly: (s, lam) = (0, 0) with gain <= 65536 is tfx_grain_u8 (the 2^24 cancels
 *      in the floor division), alpha == 0 leaves the byte unchanged, gain == 0 copies, and the grain of a scene pixel does not depend on
 *      the window that contains it, the window's border included.  out may be img (no other aliasing). */
int tfx_grain_shaped_u8(const void* img, const void* alpha, const int32_t* gain, const int32_t* shape, const int32_t* origin, uint32_t seed,
                        void* out, int32_t B, int32_t H, int32_t W, int32_t C, tfx_stream stream);
/* ---- keyed paste (DESIGN.md section 4 "Keyed paste"): inside the blend a pixel keeps the scene's byte unless the edit really differs
 *      there.  The difference of the blended result to the scene is measured, thresholded with hysteresis, grown and feathered into a key,
 *      and the result goes over the scene once more under that key.  Added without a new TFX_ABI_VERSION: three new entry points (one of
 *      them host arithmetic), no stamped struct and no existing entry point changes.  Tensors contiguous, batch-major, u8; B, H, W >= 1,
 *      B <= 65535, C in 1..4; integer arithmetic throughout, so the results are exact.  Every offset that can pass 2^31 is formed in 64
 *      bits.
 * tfx_change_metric_u8: a, b [B, H, W, C] -> out [B, H, W].  Per pixel and channel s_c = sum w[dy] w[dx] (a - b) over the 3 x 3
 *      neighbourhood, w = [1 2 1], the neighbour indices clamped to the image (edge replicated: tfx_highpass_hist_u8's stencil), and
 *      out = max over c of (|s_c| + 8) >> 4.  Hence, exactly: a == b on a pixel's neighbourhood gives 0, a - b == k there gives |k|, and
 *      out lies in 0..255 (|s_c| <= 16 * 255).  out may alias neither a nor b.
 * tfx_hysteresis_workspace_bytes: the bytes of `workspace` the call below needs (host arithmetic, no device is touched); -1 with
 *      tfx_last_error for a geometry outside the contract.
 * tfx_hysteresis_u8: m [B, H, W] -> out [B, H, W] in {0, 255}; 0 <= lo <= hi <= 256.  out = 255 exactly on the pixels with m >= lo that an
 *      8-connected path of pixels with m >= lo, inside the same sample, joins to a pixel with m >= hi (a pixel with m >= hi is such a pixel
 *      itself); every other pixel is 0.  That set is unique: the result depends on no tiling, launch order or number of rounds.  hi == 256
 *      gives all zeros, hi == 0 all 255, lo == hi the plain threshold m >= hi.  A neighbour outside the image does not exist, so no read
 *      leaves the buffers and the call is memory-safe whatever m holds.
 *      One round is one launch: every workgroup spreads the marks inside its tile (and from its one-pixel halo) until nothing changes,
 *      stores 255 on the pixels it newly reached and, if there were any, the round's number into a word of the workspace, with ordinary
 *      stores: all writers of an address store the same value, a pixel only ever goes from 0 to 255, and no workgroup waits for another
 *      (no atomics, no grid-wide barrier).  The entry point repeats the launch until a round leaves the word as it was, so every round but
 *      the last has marked at least one new pixel and the call ends after at most B H W + 1 rounds; *rounds (may be NULL) receives their
 *      number, at least 1.  THE CALL SYNCHRONISES `stream` ONCE PER ROUND, to read the word back (an image of a single tile, 64 x 16,
 *      takes one round and is not synchronised), AND IS REFUSED, with tfx_last_error, ON A CAPTURING STREAM.  m, out and workspace are
 *      three different buffers; workspace: 4-byte aligned, workspace_bytes at least tfx_hysteresis_workspace_bytes(B, H, W), else the call
 *      is refused; nothing in it survives the call.
 *      The keyed paste (textflux_amd/paste_back.py) is, with orig the scene, result today's blend of the edit and alpha its weight:
 *          m     = tfx_change_metric_u8(result, orig)
 *          key   = tfx_mask_feather_u8(tfx_mask_dilate_u8(tfx_hysteresis_u8(m, lo_eff, hi_eff), dilate), feather),   dilate >= 3 feather
 *          final = tfx_overlay_u8(orig, result, key)
 *      Hence, exactly: final == orig wherever key == 0, and everywhere outside the grown mask, where result == orig whatever the key
 *      holds; hi_eff == 0 (lo == hi == 0 on a scene whose noise estimate is 0, or with noise == 0) gives result's bytes; every pixel with
 *      m >= hi_eff has key == 255 and carries result's byte; and min(orig, result) <= final <= max(orig, result). */
int tfx_change_metric_u8(const void* a, const void* b, void* out, int32_t B, int32_t H, int32_t W, int32_t C, tfx_stream stream);
int64_t tfx_hysteresis_workspace_bytes(int32_t B, int32_t H, int32_t W);
int tfx_hysteresis_u8(const void* m, void* out, int32_t lo, int32_t hi, void* workspace, int64_t workspace_bytes, int32_t* rounds, int32_t B,
                      int32_t H, int32_t W, tfx_stream stream);
/* ---- rectified per-line edits (DESIGN.md section 4 "Rectified lines"): a slanted text line is cut as an oriented rectangle, edited
 *      upright and warped back.  Added without a new TFX_ABI_VERSION: one new entry point, no stamped struct and no existing entry point
 *      changes.  Tensors contiguous, batch-major; B, H, W, out_h, out_w >= 1, B <= 65535, C in 1..4; in, out and coverage are three
 *      different buffers; m and taps are 8-byte aligned DEVICE pointers.  Integer arithmetic throughout, so the results are exact.
 * tfx_warp_affine_u8: in u8 [B, H, W, C] -> out u8 [B, out_h, out_w, C]; out[b, j, i, c] is in[b] sampled at the affine image of the
 *      destination pixel (i, j) under m i64 [B][6] (one matrix per sample), in Q16 and 64-bit integers:
 *          X = m0 i + m1 j + m2,  Y = m3 i + m4 j + m5     (the caller folds the pixel-centre offsets into m2, m5 and keeps |X|, |Y| < 2^62)
 *          xi = X >> 16 (arithmetic shift: floor), fx = (X >> 8) & 255; yi, fy from Y alike
 *          acc = sum over r, k in 0..3 of taps[fy][r] taps[fx][k] in[b, clamp(yi - 1 + r, 0, H - 1), clamp(xi - 1 + k, 0, W - 1), c]
 *          out = clamp((acc + 2^27) >> 28, 0, 255)
 *      taps i16 [256][4]: row f holds the weights of the four taps at distances 1 + t, t, 1 - t, 2 - t for t = f / 256, with 14
 *      fractional bits; every row sums to exactly 1 << 14 (the Catmull-Rom table of textflux_amd/rectify.py::catmull_rom_taps), so a
 *      constant image stays that constant.  The indices are clamped (edge replicate): no read leaves `in`, whatever m holds.
 *      coverage (may be NULL) u8 [B, out_h, out_w] = 255 where 0 <= xi < W and 0 <= yi < H, else 0: whether the sample position lies in
 *      the image. */
int tfx_warp_affine_u8(const void* in, void* out, void* coverage, int32_t B, int32_t H, int32_t W, int32_t C, int32_t out_h, int32_t out_w,
                       const int64_t* m, const int16_t* taps, tfx_stream stream);
/* ---- perspective per-line edits (DESIGN.md section 4 "Perspective lines"): a text line seen at an angle is cut as a quadrilateral,
 *      edited upright and warped back under a homography.  Added without a new TFX_ABI_VERSION: one new entry point, no stamped struct
 *      and no existing entry point changes.  The tensor contract is tfx_warp_affine_u8's: contiguous, batch-major; B, H, W, out_h,
 *      out_w >= 1, B <= 65535, C in 1..4; in, out and coverage are three different buffers; m and taps are 8-byte aligned DEVICE
 *      pointers; taps is the same i16 [256][4] table.  Integer arithmetic throughout, so the results are exact.
 * tfx_warp_perspective_u8: in u8 [B, H, W, C] -> out u8 [B, out_h, out_w, C] (coverage: NULL or u8 [B, out_h, out_w]) under
 *      m i64 [B][9] (one matrix per sample).  Per destination pixel (i, j), in 64-bit integers:
 *          Nx = m0 i + m1 j + m2,  Ny = m3 i + m4 j + m5,  D = m6 i + m7 j + m8
 *          D <= 0:  out = 0 on every channel, coverage = 0, and NO read of `in`         (the pixel lies at or behind the horizon)
 *          D >  0:  PX = floor((Nx * 256) / D),  PY = floor((Ny * 256) / D)             (floor, not truncation: a negative numerator
 *                   rounds DOWN; Nx * 256 is formed with wrapping, as an unsigned shift left by 8 does)
 *                   xi = PX >> 8, fx = PX & 255; yi, fy from PY alike
 *                   acc = sum over r, k in 0..3 of taps[fy][r] taps[fx][k] in[b, clamp(yi - 1 + r, 0, H - 1), clamp(xi - 1 + k, 0, W - 1), c]
 *                   out = clamp((acc + 2^27) >> 28, 0, 255);  coverage = 255 where 0 <= xi < W and 0 <= yi < H, else 0
 *                   -- from xi, fx, yi, fy on exactly as in tfx_warp_affine_u8.
 *      The caller keeps |Nx|, |Ny| < 2^54 and 0 < D < 2^54 over the destination wherever it wants a defined pixel (the * 256 then stays
 *      inside 64 bits).  Whatever m holds the call is memory-safe: the products wrap, the division is guarded by D <= 0, and the indices are
 *      clamped in 64 bits before they are narrowed, so no read leaves `in`.
 *      Affine embedding: with m6 = m7 = 0, m8 = 2^16 and m0..m5 a Q16 affine matrix the result is tfx_warp_affine_u8's bit for bit
 *      (floor(X 256 / 2^16) = X >> 8). */
int tfx_warp_perspective_u8(const void* in, void* out, void* coverage, int32_t B, int32_t H, int32_t W, int32_t C, int32_t out_h,
                            int32_t out_w, const int64_t* m, const int16_t* taps, tfx_stream stream);
/* ---- curved per-line edits (DESIGN.md section 4 "Curved lines"): a text line along a bend is cut along its own centre line, edited
 *      upright and warped back; no single matrix expresses a bend, so this warp reads its source positions from a coarse control grid.
 *      With shift = 0 it is a general per-pixel remap.  Added without a new TFX_ABI_VERSION: one new entry point, no stamped struct and
 *      no existing entry point changes.  The tensor contract is tfx_warp_affine_u8's: contiguous, batch-major; B, H, W, out_h, out_w >= 1,
 *      B <= 65535, C in 1..4; in, out and coverage are three different buffers; coverage may be NULL; grid and taps are 8-byte aligned
 *      DEVICE pointers; taps is the same i16 [256][4] table.  Integer arithmetic throughout, so the results are exact.
 * tfx_warp_grid_u8: in u8 [B, H, W, C] -> out u8 [B, out_h, out_w, C] (coverage: NULL or u8 [B, out_h, out_w]) under
 *      grid i64 [B][gh][gw][2], shift in 0..5, c = 1 << shift the cell size in destination pixels,
 *          gh = ((out_h - 1) >> shift) + 2,  gw = ((out_w - 1) >> shift) + 2
 *      node (r, q) = the Q16 source position (x, y) of destination pixel (q c, r c); the pixel-centre convention is the affine warp's (the
 *      caller folds it in).  Per destination pixel (i, j), in 64-bit integers:
 *          gx = i >> shift, gy = j >> shift, ax = i & (c - 1), ay = j & (c - 1)
 *          g00 = node (gy, gx), g01 = node (gy, gx + 1), g10 = node (gy + 1, gx), g11 = node (gy + 1, gx + 1)
 *          the x of any of the four == INT64_MIN:  out = 0 on every channel, coverage = 0, and NO read of `in`   (the pixel has no source:
 *                   the perspective kernel's horizon rule)
 *          otherwise:  X = ((c - ax)(c - ay) g00x + ax (c - ay) g01x + (c - ax) ay g10x + ax ay g11x) >> (2 shift)    (an ARITHMETIC
 *                   shift: it floors; products and sums are formed with wrapping, as unsigned arithmetic does);  Y alike from the y's
 *                   xi = X >> 16, fx = (X >> 8) & 255; yi, fy from Y alike
 *                   acc = sum over r, k in 0..3 of taps[fy][r] taps[fx][k] in[b, clamp(yi - 1 + r, 0, H - 1), clamp(xi - 1 + k, 0, W - 1), c]
 *                   out = clamp((acc + 2^27) >> 28, 0, 255);  coverage = 255 where 0 <= xi < W and 0 <= yi < H, else 0
 *                   -- from X, Y on exactly as in tfx_warp_affine_u8.
 *      The caller keeps |g| < 2^50 on every unmarked component: the four weights sum to c^2 <= 2^10, so the sum stays inside 64 bits.
 *      Whatever the grid holds the call is memory-safe: node indices lie inside [gh][gw] by the construction of gh and gw, the products
 *      wrap, and the sample indices are clamped in 64 bits before they are narrowed, so no read leaves `in` or `grid`.
 *      Affine embedding: nodes that hold a Q16 affine matrix evaluated at their pixels interpolate it exactly (the weighted sum is
 *      c^2 X with no remainder), so the result is tfx_warp_affine_u8's bit for bit at every shift. */
int tfx_warp_grid_u8(const void* in, void* out, void* coverage, int32_t B, int32_t H, int32_t W, int32_t C, int32_t out_h, int32_t out_w,
                     const int64_t* grid, int32_t shift, const int16_t* taps, tfx_stream stream);
/* ---- candidates (DESIGN.md section 4 "Candidates"): all line crops of a batch in one launch, packed for tfx_ocr_resize_norm.  Added
 *      without a new TFX_ABI_VERSION: one new entry point, no stamped struct and no existing entry point changes.
 * tfx_warp_affine_gather_u8: images u8 [B, H, W, C] (contiguous, B, H, W >= 1, C in 1..4), table i64 [n][10] on the DEVICE, 8-byte aligned,
 *      one row per crop: (b, m0, m1, m2, m3, m4, m5, out_h, out_w, offset).  Crop k is images[b] under the Q16 matrix m0..m5 exactly as
 *      tfx_warp_affine_u8 computes it (the same map, the same taps table, edge replicated), written as u8 [out_h, out_w, C] at BYTE
 *      `offset` of the packed buffer out u8 [out_bytes].  Offsets are byte-granular: no alignment of a crop's start is assumed.  The
 *      caller keeps the crops' byte ranges apart from each other.
 *      A row that cannot be served writes NOTHING and adds 1 to *refused (DEVICE int32, 4-byte aligned, zeroed by the caller): b outside
 *      [0, B), out_h or out_w outside 1..2^24, or [offset, offset + out_h out_w C) not inside [0, out_bytes).  Every other row is served.
 *      blocks_per_crop in 1..65535: how many workgroups share one crop's 32 x 8 tiles; the result does not depend on it.
 *      Refused on the host: a null pointer, n < 0 or n > 65535, C outside 1..4, out_bytes < 0, misaligned table, taps or refused, or
 *      images, out, table and refused overlapping.  n == 0 launches nothing. */
int tfx_warp_affine_gather_u8(const void* images, void* out, int64_t out_bytes, const int64_t* table, int32_t n, int32_t* refused, int32_t B,
                              int32_t H, int32_t W, int32_t C, int32_t blocks_per_crop, const int16_t* taps, tfx_stream stream);
/* out[b, t, col0 + (i*8+j)*4 + py*2+px] = mask[(2ty+py)*8 + i, (2tx+px)*8 + j]  (P:1563-1580: 8x8 pixel blocks -> channels,
 * then _pack_latents), t = ty * (W/16) + tx, row stride ld. */
int tfx_pack_mask(const void* mask, int32_t mask_dtype, void* out, int32_t B, int32_t H, int32_t W, int32_t mask_batch,
                  int32_t binarize, int64_t ld, int32_t col0, tfx_stream stream);
/* The packed latent mask of known-region sampling (DESIGN.md section 4 "Known-region sampling"): mask_u8 [B, H, W] uint8 (8-byte
 * aligned, H and W multiples of 16) -> out bf16 [B, (H/16)(W/16), C] of 1.0 / 0.0, out[b, t, c*4 + py*2+px] = m(2ty+py, 2tx+px) for
 * every c: _pack_latents of the latent-resolution mask repeated over the latent channels (FluxInpaintPipeline.prepare_mask_latents).
 *   mode 0 (nearest, the reference's F.interpolate): m(ly, lx) = mask[8 ly, 8 lx] >= 128; grow must be 0
 *   mode 1 (cover): m = 1 if any pixel of the 8x8 blocks of latent pixels [ly-grow, ly+grow] x [lx-grow, lx+grow] (clipped to the
 *           image) is >= 128, 0 <= grow <= 8: a latent pixel counts as known only when nothing masked touches it or its neighbours
 * C a positive multiple of 8 (64 for the Fill model). */
int tfx_keep_mask_pack(const void* mask_u8, void* out, int32_t B, int32_t H, int32_t W, int32_t C, int32_t mode, int32_t grow,
                       tfx_stream stream);
/* The hold bytes of change-map sampling (DESIGN.md section 4 "Change-map sampling"): map_u8 [B, H, W] uint8 (8-byte aligned, H and W
 * multiples of 16; 255 = free to change from the first step, 0 = never changes) -> hold u8 [B, (H/16)(W/16), 4] (4-byte aligned),
 * hold[b, t, py*2+px] = 255 - g(2ty+py, 2tx+px), t = ty * (W/16) + tx.
 *   mode 0 (nearest, the reference's F.interpolate): g(ly, lx) = map[8 ly, 8 lx]; grow must be 0
 *   mode 1 (cover): g = the maximum of map over the 8x8 blocks of latent pixels [ly-grow, ly+grow] x [lx-grow, lx+grow] (clipped to the
 *           image), 0 <= grow <= 8: tfx_keep_mask_pack's cover on grey values -- a token is held no longer than the freest pixel near it */
int tfx_change_map_pack(const void* map_u8, void* hold, int32_t B, int32_t H, int32_t W, int32_t mode, int32_t grow, tfx_stream stream);
/* moments [B, h, w, 2L] NHWC bf16 (mean | logvar: the encoder's conv_out), eps [B, L, h, w] f32 / bf16 or NULL (mode) ->
 * out[b, t, col0 + c*4 + py*2+px] = ((mean + exp(0.5 clamp(logvar, -30, 20)) * eps) - shift) * scale, every intermediate
 * rounded to bf16 as the reference's tensor ops do (D/models/autoencoders/vae.py:781-802, P:1528-1530, 1743-1748). */
int tfx_vae_sample_pack(const void* moments, const void* eps, int32_t eps_dtype, void* out, int32_t B, int32_t h, int32_t w,
                        int32_t L, float shift, float scale, int64_t ld, int32_t col0, tfx_stream stream);
/* latents [B, (h/2)(w/2), >= 4L] (row stride ld) -> z [B, h, w, L] NHWC bf16 = latents / scale + shift, un-patchified
 * (P:1752-1765, 2126-2127): the decoder input.  ld >= 4L. */
int tfx_unpack_latents(const void* latents, int64_t ld, void* out, int32_t B, int32_t h, int32_t w, int32_t L, float shift,
                       float scale, tfx_stream stream);
/* x [B, H, W, Cs] NHWC bf16 (first C channels), window rows [y0, y0 + Hc) x columns [x0, x0 + Wc) -> mode 0 NCHW bf16 |
 * 1 NHWC f32 | 2 NHWC u8 = round(255 v) | 3 NCHW f32; denorm != 0: v = clamp(x / 2 + 0.5, 0, 1) in bf16 steps (IP:227-239,
 * 196-209, 133-154).  The window is the callers' result crop (run_inference.py:460-465), applied on the device. */
int tfx_postprocess(const void* x, void* out, int32_t B, int32_t H, int32_t W, int32_t Cs, int32_t C, int32_t mode, int32_t denorm,
                    int32_t y0, int32_t x0, int32_t Hc, int32_t Wc, tfx_stream stream);
/* helpers of the VAE mid-block attention (one head of dim C over h*w tokens, AttnProcessor2_0,
 * D/models/attention_processor.py:2799-2881): out[b][c, n] = in[b][n, c]; p[r, :N] = bf16(softmax(scale * s[r, :N])) with
 * s fp32 (row stride lds) from tfx_gemm_bf16_f32 and p bf16 (row stride ldp), fp32 statistics -- what a flash kernel
 * keeps in registers, here through HBM because one head of dim 512 does not fit the 128-wide attention kernel.
 * tfx_transpose: ldi >= C, ldo >= N, batch <= 65535. */
int tfx_transpose(const void* in, int64_t ldi, int64_t in_bstride, void* out, int64_t ldo, int64_t out_bstride, int32_t N,
                  int32_t C, int32_t batch, tfx_stream stream);
int tfx_row_softmax(const float* s, int64_t lds, void* p, int64_t ldp, int32_t rows, int32_t N, float scale, tfx_stream stream);

/* ---- text encoders of encode_prompt (P:1411-1503: CLIP-L pooled output of `prompt`, T5-XXL sequence of `prompt_2`).  The
 *      reference calls third-party `transformers` (pinned 4.43.3: models/t5/modeling_t5.py T5Stack / T5Block / T5Attention /
 *      T5LayerNorm / T5DenseGatedActDense; models/clip/modeling_clip.py CLIPTextTransformer / CLIPEncoderLayer / CLIPAttention /
 *      CLIPMLP); the Linear layers run on tfx_gemm_bf16 (residual adds in its epilogue: the bf16 residual stream of a
 *      torch_dtype = bfloat16 load), and: */
/* nn.LayerNorm(D, eps) with elementwise affine over bf16 rows: out[r, :] = bf16((x[r, :] - mean) * rstd * gamma + beta), fp32
 * arithmetic and ONE rounding (what F.layer_norm does on bf16 tensors; CLIPEncoderLayer.layer_norm1 / 2, final_layer_norm).
 * Any gamma (no (1 + scale) re-parameterisation).  D % 8 == 0, D <= 3072, ldx / ldo in elements, multiples of 8. */
int tfx_layernorm(const void* x, int64_t ldx, void* out, int64_t ldo, const void* gamma, const void* beta, int64_t rows,
                  int32_t D, float eps, tfx_stream stream);
/* softmax(scale * q k^T + bias) v for heads of dim 64 and N <= 512 keys (tfx_attn_args with 64-wide heads: element (b, n, h, d)
 * at base + b*bstride + n*ld + h*64 + d).  rel_bias: NULL or fp32 [H, 2N-1], bias(h, query, key) = rel_bias[h][key - query +
 * N - 1] (T5Attention.compute_bias: a function of key - query only); causal != 0 masks key > query (CLIP). */
int tfx_attention64(const tfx_attn_args* args, const float* rel_bias, int32_t causal, tfx_stream stream);
/* T5LayerNorm: out[r, :] = bf16(w * bf16(x[r, :] * rsqrt(mean(x[r, :]^2) + eps))); x f32 (x_dtype 0) or bf16 (1). */
int tfx_rmsnorm(const void* x, int32_t x_dtype, int64_t ldx, const void* w, void* out, int64_t ldo, int64_t rows, int32_t D,
                float eps, tfx_stream stream);
/* out[i, :] = table[ids[i], :] (bf16 rows of D elements, ids int64 clamped to [0, vocab)): nn.Embedding. */
int tfx_gather_rows(const void* table, const int64_t* ids, void* out, int64_t n, int32_t D, int64_t vocab, tfx_stream stream);
/* fp32 accumulation buffer helper (T5 under torch_dtype = float16 keeps `wo` in fp32 and its residual stream promotes to fp32;
 * under bfloat16 -- what the reference loads -- the stream is bf16 and this is not on the path): mode 0 x += y (bf16),
 * 1 x += y (f32), 2 x = y (bf16 -> f32). */
int tfx_add_into_f32(float* x, const void* y, int64_t n, int32_t mode, tfx_stream stream);
/* mode 0: out = a * b (T5DenseGatedActDense: gelu(wi_0 x) * wi_1 x), mode 1: out = a * sigmoid(1.702 a) (CLIP quick_gelu);
 * bf16 [rows, cols] with row strides. */
int tfx_mul_act(const void* a, int64_t lda, const void* b, int64_t ldb, void* out, int64_t ldo, int64_t rows, int32_t cols,
                int32_t mode, tfx_stream stream);

/* ---- read-back: the text recogniser that scores what an edit wrote (eval/recognizer.py + eval/ocr_recog of the reference: a
 *      MobileNetV1Enhance backbone, a two-block SVTR neck, a CTC head) and the CTC decode / loss behind it (ocr.hip; DESIGN.md §4
 *      "Read-back").  Activations are fp32 NHWC with the channels contiguous; weights are fp32 with BatchNorm folded in by the caller.
 *      No floating-point atomics: two runs give the same bits.  act: 0 none, 1 relu, 2 hard-swish (x * relu6(x + 3)) / 6, 3 hard-sigmoid
 *      relu6(x + 3) / 6 (both with an IEEE division), 4 swish x * (1 / (1 + exp(-x))). ---- */
/* TextRecognizer.resize_norm_img for n line crops in ONE launch: crop i is u8 [h, w, 3] at src + table[i][0], table = device int32
 * [n][4] = {byte offset, h, w, turn}; src_bytes is the size of the packed buffer (an entry that leaves it, or has h or w < 1, writes
 * zeros and reads nothing).  turn != 0 reads the crop through the reference's quarter turn (transpose(1, 2).flip(dims=[1]): turned
 * pixel (r, c) = source pixel (c, w - 1 - r)).  out fp32 [n, img_h, img_w, 3]: bilinear with align_corners = True to
 * (img_h, resized_w), resized_w = min(img_w, ceil(img_h * w / h)) of the turned size in fp64, then (v / 255 - 0.5) / 0.5; the
 * columns >= resized_w are 0.0. */
int tfx_ocr_resize_norm(const void* src, int64_t src_bytes, const int32_t* table, float* out, int32_t n, int32_t img_h, int32_t img_w,
                        tfx_stream stream);
/* Dense convolution as an implicit GEMM on v_mfma_f32_16x16x4_f32 (exact f32 products and sums): x [B, H, W, Cin] with pixel pitch
 * ldx floats, w [Cout][ksize][ksize][Cin], bias [Cout] or NULL, ksize 1 or 3, padding ksize / 2, strides >= 1; pixel p of the
 * [B, Ho, Wo] output grid writes out[p * ldo + co_off + n] = act(sum + bias[n]) for n < Cout, so a result can land in a column range of
 * a wider buffer.  A linear [M, K] -> [M, N] is B = M, H = W = 1, ksize = 1.  The sum over k = (ky, kx, ci) is taken in 16-wide chunks:
 * chunk c goes to partial sum c % 4, inside a chunk the products are added in the order k = j, 4 + j, 8 + j, 12 + j for j = 0 .. 3 (one
 * fmaf each), and the four partial sums are added in rising order; taps outside the image add 0. */
int tfx_ocr_conv_f32(const float* x, const float* w, const float* bias, float* out, int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout,
                     int32_t ksize, int32_t stride_h, int32_t stride_w, int32_t act, int64_t ldx, int64_t ldo, int32_t co_off, tfx_stream stream);
/* Depthwise convolution: x [B, H, W, C] contiguous, w [ksize][ksize][C], bias [C] or NULL, ksize 3 or 5, padding ksize / 2, strides 1
 * or 2 each, act 0 or 2; C % 4 == 0 and 16-byte aligned pointers.  One fmaf per tap in (ky, kx) order; taps outside the image are
 * skipped (the padding may be wider than the image). */
int tfx_ocr_conv_dw(const float* x, const float* w, const float* bias, float* out, int32_t B, int32_t H, int32_t W, int32_t C, int32_t ksize,
                    int32_t stride_h, int32_t stride_w, int32_t act, tfx_stream stream);
/* mode 0: out [B, C] = the sum over (h, w) in row-major order, then ONE division by H * W (nn.AdaptiveAvgPool2d(1));
 * mode 1: out [B, H / 2, W / 2, C] with pixel pitch ldo = ((x00 + x01) + (x10 + x11)) * 0.25 (nn.AvgPool2d(2, 2)). */
int tfx_ocr_pool(const float* x, float* out, int32_t B, int32_t H, int32_t W, int32_t C, int32_t mode, int64_t ldo, tfx_stream stream);
/* out[b, p, c] = x[b, p, c] * s[b, c] for p < HW (the squeeze-excite product); C % 4 == 0, 16-byte aligned pointers; out may be x. */
int tfx_ocr_scale_channels(const float* x, const float* s, float* out, int32_t B, int64_t HW, int32_t C, tfx_stream stream);
/* nn.LayerNorm on fp32 rows [rows, D], D <= 512, with row pitches: mean = sum / D, var = sum (x - mean)^2 / D,
 * y = (x - mean) * (1 / sqrt(var + eps)) * gamma + beta; the sums are wave reductions in a fixed order. */
int tfx_ocr_layernorm(const float* x, int64_t ldx, float* out, int64_t ldo, const float* gamma, const float* beta, int64_t rows, int32_t D,
                      float eps, tfx_stream stream);
/* Softmax attention of the SVTR blocks: qkv fp32 [B, N, 3 * H * d] contiguous (column = which * H * d + head * d + e) -> out
 * [B, N, H * d]; d <= 32, N <= 256.  q is multiplied by scale (rounded) BEFORE the product, as the reference does; scores are fmaf
 * chains over e; the softmax is exp(s - max) / sum in fp32; the output sums p[j] v[j] over the first ceil(N / 2) keys and over the
 * rest, each as an fmaf chain in rising j, and adds the two.  One workgroup per (b, head), scores in LDS. */
int tfx_ocr_attention(const float* qkv, float* out, int32_t B, int32_t N, int32_t H, int32_t d, float scale, tfx_stream stream);
/* Per row of C logits (rows with pitch ld): row_max = the maximum, row_arg = its FIRST index (numpy's argmax tie rule), row_lse =
 * max + log(sum exp(x - max)).  Thread t of 256 takes the classes t, t + 256, ... in rising order; a fixed tree folds the 256 partial results. */
int tfx_ctc_rows(const float* logits, int64_t ld, int64_t rows, int32_t C, float* row_max, int32_t* row_arg, float* row_lse, tfx_stream stream);
/* Per sample of logits [n, T, C] (T <= 256), from tfx_ctc_rows' row_arg / row_lse [n, T]: the greedy decode of TextRecognizer.decode
 * -- collapse repeats, then drop the blank 0 -- as ids / time_index int32 [n, T] (the first count[n] entries; the rest 0 / -1) and
 * count [n]; and, when loss != NULL, loss[n] = -log p(target | logits) by the forward recursion in log space over the 2 L + 1 states
 * (torch.nn.CTCLoss(reduction='none'), blank 0): targets = the concatenated int32 ids, offsets int32 [n + 1], L <= max_target <= 127.
 * L = 0 is valid; a target that cannot be emitted in T steps gives +inf. */
int tfx_ctc_score(const float* logits, const int32_t* row_arg, const float* row_lse, const int32_t* targets, const int32_t* offsets,
                  int32_t max_target, int32_t n, int32_t T, int32_t C, int32_t* ids, int32_t* time_index, int32_t* count, float* loss,
                  tfx_stream stream);

/* ---- tuning knobs (no reference counterpart).  "attention_waves" selects the attention kernel: 30 (default) = one
 *      256-thread workgroup per CU -- one wave per SIMD, 64 query rows per wave, the tile loop pipelined per (32-key block,
 *      32-row q-block) unit (attention_w4.hip); it stores whole output rows in 16-byte pieces, so output views whose row or
 *      batch stride is not a multiple of 8 elements are served by 10.  10 = one 512-thread workgroup of 256 query rows per
 *      CU, 32 rows per wave; both keep the softmax bookkeeping on the matrix pipe (pre-scaled Q, lazy reference maximum
 *      subtracted by an extra MFMA k-step, row sums from a ones-block of the PV MFMA).  8 = the 512-thread schedule with the
 *      textbook exact online maximum (the independent implementation the tests compare with); 20 = 10 pipelined per
 *      half-tile (attention_hp.hip).  Bench builds only (-DTFX_BENCH): 12 / 4 = two independent 256-thread workgroups per
 *      CU of 10 / 8; 9 = 8 with 128 keys per barrier; 16 = softmax / MFMA ping-pong between the wave groups.  All compute
 *      the same softmax; 10, 12, 20 and 30 differ from the others in rounding only (one extra bf16 rounding of q * scale,
 *      row sums of the bf16 weights); 40 = 30 on v_mfma_f32_16x16x32_bf16 (attention_w16.hip); 0 restores the default.
 *      "attention_streamk": 1 (default) lets kernel 30 deal the (b, h, 256-query) items of a batch sample's last, partly filled
 *                         round of CUs as (item, 64-key tile) units -- every CU of the sample's group gets the same number of key
 *                         tiles, an item cut by a CU boundary is finished by a merge pass -- when tfx_attn_args.workspace is given
 *                         and the library's estimate says it pays (P1024 batch 8: -1.1 % per launch, 2048 x 1024 batch 1: -12 %,
 *                         1024 x 672 batch 1: -16 %); 2 = whenever admissible; 0 = whole items only: a sample's bits then do not
 *                         depend on how many samples share its batch (identical samples of ONE batch agree either way).  (With the
 *                         step cache of tfx_step_desc.phase in use, a sample's bits depend on its batch-mates in another way too:
 *                         the caller skips a step for the whole batch, by the largest metric among its samples.)
 *      "attention_tail_split": 1 lets kernel 30 cut the q-tiles of a partly filled last round of workgroups into two key ranges
 *      (+ a merge kernel; faster at small batches, but a sample's bits then depend on the batch size: default 0).
 *      "gemm_group_m": row tiles per group of the GEMM tile order (default 0 = by shape: 1 for N <= 3072, else 4).
 *      "gemm_place": slot assignment of the persistent GEMM's operand requests, 1 or 2 (default 2; gemm.hip).
 *      "gemm_splitk": 0 disables the split-K path of few-tile GEMMs (default 1).
 *      "fp8_fuse_qkn": 0 = in fp8 mode the q | k | v (| mlp) projections are followed by the separate q / k norm + RoPE pass (default 1:
 *      fused into the e4m3 GEMM's epilogue like the bf16 mode's).
 *      "ln_joint": 0 = the LayerNorm + modulation of a double block's text and image rows as two launches (default 1: one launch over the
 *      joint rows, the text rows taking the second modulation; bit-identical, round 6).
 *      "ln_prefetch": the LayerNorm + modulation kernel requests the modulation rows up front: 0 never, 1 always, 2 (default) for <= 16384
 *      rows (latency-bound launches: batch 1); bit-identical either way. */
int tfx_set_option(const char* name, int value);
/* The only device memory the library ever allocates itself is behind an opt-in knob: the attention tail-split partials
 * ("attention_tail_split" 1; 138 MB per (device, stream) that launched with it, at most 8).  tfx_release_scratch synchronises the
 * device and frees them all; streams seen afterwards allocate afresh.  Graphs captured while the knob was on hold the old pointers
 * and must be destroyed first (tfx_graph_destroy).  With the defaults this is a no-op.  Returns 0. */
int tfx_release_scratch(void);

/* ---- measurement hooks (no reference counterpart: the reference has no profiling) --------------------
 * When enabled, every MFMA-GEMM (kind 0) / attention (kind 1) launch is bracketed by hipEvents on its own stream and
 * its algorithmic FLOPs (2*M*N*K*batch, 4*B*H*N^2*128) are recorded; tfx_prof_collect waits for those launches and
 * returns the summed kernel time, FLOPs and launch count (kind 2: fp8 GEMM launches), then clears the records.  Not capturable into a graph. */
int tfx_prof_enable(int on);
int tfx_prof_collect(int kind, double* total_ms, double* total_flops, int* launches);
/* Round 6 (ABI 7).  The matrix-pipe rate the BOARD sustains at its power cap, as the denominator of a roofline fraction that does not
 * depend on which box runs the bench: one launch of a kernel that issues nothing but the GEMM kernels' own MFMA sections
 * (v_mfma_f32_16x16x32_bf16; fp8 != 0: v_mfma_scale_f32_16x16x128_f8f6f4 with unit scales) on fragments read ONCE from `operands`
 * (operand_bytes >= 16 KiB of the caller's data -- random N(0, 1) values for the worst-case figure; power, and with it the clock,
 * depends on operand entropy), one 8-wave workgroup per CU, `ktiles` (a multiple of 48) K-tiles of 64 (fp8: 32) MFMAs per wave.
 * Writes the launch's FLOPs to *flops; the caller times it (events on `stream`) over 2-3 s: shorter runs finish inside the power
 * controller's averaging window and report the uncapped clock.  No reference counterpart. */
int tfx_mfma_peak_probe(const void* operands, int64_t operand_bytes, int32_t fp8, int32_t ktiles, double* flops, tfx_stream stream);
/* Which form of the attention kernel the launches took (host-side counters, also counted at graph capture, not at replay):
 * counts[0..7] = launches since the last reset of { 0: kernel 30 with its own overflow guard, 1..3: its option-31..33 variants,
 * 4: kernel 30 reference-free (score_bound accepted), 5: attention_hp (20), 6: the 16 x 16 kernel (40), 7: any other schedule };
 * counts[8] (ABI 8) = how many of those launches dealt the items of their last, partly filled round as (item, 64-key tile) units
 * ("attention_streamk").  Copies min(n, 9) counters, then clears them when reset != 0.  Returns the number copied. */
int tfx_attention_mode_counts(int64_t* counts, int32_t n, int32_t reset);
/* Phase timing of the attention kernels (tools/attn_timing.py): buf = device uint64 [blocks][8 waves][4 phases] that the
 * instrumented kernel variants fill with cycle counts, NULL switches back to the plain kernels. */
int tfx_debug_attention_timing(void* buf);

#ifdef __cplusplus
}
#endif
#endif /* TEXTFLUX_HIP_H */
