// The host-side DiT forward that strings the kernels together (one FluxTransformer2DModel.forward, reference:
// diffusers/src/diffusers/models/transformers/transformer_flux.py:1028-1212).  Everything it launches goes through launch.h, which is
// what lets tests/test_dit_launch_trace.py record the whole launch plan without a device.
#include "../../include/textflux_hip.h"

#include "launch.h"

namespace tfx {
namespace {

#define TRY(x)            \
  do {                    \
    if (int _e = (x)) return _e; \
  } while (0)

int g_fp8_fuse_qkn = 1;    // tfx_set_option fp8_fuse_qkn: 0 = fp8 projections followed by the separate q / k norm + RoPE pass (round 4; A/B knob)
int g_ln_joint = 1;        // tfx_set_option ln_joint: 0 = the LayerNorm + modulation of a double block's text and image rows as two launches (A/B knob)
int g_group_streams = 1;   // tfx_set_option gemm_group_streams: 0 = the text and image GEMMs of a double block as separate launches (A/B knob)

struct Buf { uint16_t* p; int64_t ld, bs; };   // a workspace matrix [B][N, ld] bf16: row pitch, batch stride (elements)
// A launch group: rows [row0, row0 + rows) of every sample's joint [text | image] stream.  split > 0: a joint launch whose rows below
// `split` are the text rows and take the text stream's weights / modulation / norm weights.
struct Rows { int row0, rows, split; };

// What one forward call works on: the descriptor, the stream and everything derived from them.  Built per call, so two forwards on
// two threads share nothing.
struct Ctx {
  const tfx_dit_desc& d;
  hipStream_t st;
  const int D, H, B, Sn, T, N;
  const int64_t D7, hid_bs, y_bs;
  const Buf hid, xn, y;              // y = [k | v | q | ...]; the attention output overwrites q
  const uint16_t* mod; const int64_t mbs;
  void* const q8; float* const q8s;  // fp8 linears (flags bit 2): the workspace of the quantised activations [B][N][D] bytes / [B][N], else null
  void* const ws; const int64_t ws_bytes;   // the split-K scratch of the block Linears; idle between GEMMs, so attention's stream-K partials too
  const float eps = 1e-6f;
  Ctx(const tfx_dit_desc& d_, hipStream_t st_)
      : d(d_), st(st_), D(d.D), H(d.H), B(d.B), Sn(d.S), T(d.T), N(d.S + d.T), D7(7ll * d.D), hid_bs((int64_t)N * D), y_bs((int64_t)N * D7),
        hid{(uint16_t*)d.hid, D, hid_bs}, xn{(uint16_t*)d.xn, D, hid_bs}, y{(uint16_t*)d.y, D7, y_bs},
        mod((const uint16_t*)d.mod), mbs(d.mod_bstride), q8((d.flags & 4) ? d.q8 : nullptr), q8s((d.flags & 4) ? d.q8_scale : nullptr),
        ws(d.gemm_workspace), ws_bytes(d.gemm_workspace_bytes) {}

  // LayerNorm + modulation hid -> xn of rows [row0, row0 + rows) of every sample
  int ln(int row0, int rows, const uint16_t* shift, const uint16_t* scale) const {
    return ln_modulate(hid.p + (int64_t)row0 * D, xn.p + (int64_t)row0 * D, shift, scale, mbs, rows, B, D, D, hid_bs, D, hid_bs, eps, st);
  }
  // RMSNorm + RoPE of q, k on a row group of y as a separate pass (projections that did not carry it in their epilogue)
  int norm_rope(const Rows& r, const void* nq, const void* nk, const void* nq_txt, const void* nk_txt) const {
    if (r.rows <= 0) return 0;
    if (d.rope_bstride > 0)   // mixed-geometry batch: one table per sample
      return rmsnorm_rope_tab(y.p + r.row0 * D7, D7, y_bs, 2 * D, 0, H, r.rows, r.split, B, nq, nk, r.split ? nq_txt : nq, r.split ? nk_txt : nk,
                              d.cos_tab + (int64_t)r.row0 * 128, d.sin_tab + (int64_t)r.row0 * 128, d.rope_bstride * 128, eps, st);
    return rmsnorm_rope(y.p + r.row0 * D7, D7, y_bs, 2 * D, 0, H, r.rows, r.split, B, nq, nk, r.split ? nq_txt : nq, r.split ? nk_txt : nk,
                        d.cos_tab + (int64_t)r.row0 * 128, d.sin_tab + (int64_t)r.row0 * 128, eps, st);
  }
  int attention(float block_bound) const {   // the block's own score bound (ABI 6), else the forward-wide one
    AttnArgs a;
    a.q = y.p + 2 * D; a.k = y.p; a.v = y.p + D; a.o = y.p + 2 * D;
    a.ldq = a.ldk = a.ldv = a.ldo = D7;
    a.q_bstride = a.k_bstride = a.v_bstride = a.o_bstride = y_bs;
    a.B = B; a.H = H; a.N = N; a.scale = 0.08838834764831845f /* 128^-0.5 */; a.score_bound = block_bound > 0.f ? block_bound : d.attn_score_bound;
    a.workspace = ws; a.workspace_bytes = ws_bytes;
    a.seq_len = d.seq_len;
    return joint_attention(a, st);
  }
};

// One Linear of the forward as a GEMM under construction.
struct Gemm {
  GemmArgs a = GemmArgs();
  const tfx_linear* lin;
  const tfx_linear* lin2 = nullptr;     // row-split launches: the Linear of the rows below split_row
  const Buf* in = nullptr;              // block Linears: the workspace matrix the input lives in (xn or y)
  bool fp8 = false;                     // a block Linear of a forward in fp8 mode: runs on its w8 when it has one
  int ln_row0 = -1;                     // >= 0: the producing LayerNorm already quantised the input, rows from ln_row0 of the q8 workspace
  Gemm(const void* A, int64_t lda, int64_t abs_, const tfx_linear& l, void* C, int64_t ldc, int64_t cbs, int M, int N, int K, int batch)
      : lin(&l) {
    a.A = A; a.lda = lda; a.a_bstride = abs_;
    a.W = l.w; a.ldw = l.ldw > 0 ? l.ldw : K; a.bias = l.b;
    a.C = C; a.ldc = ldc; a.c_bstride = cbs;
    a.M = M; a.N = N; a.K = K; a.batch = batch;
    a.epilogue = EPI_BIAS;
  }
  Gemm& gelu(int from_col) { a.epilogue = EPI_BIAS_GELU; a.gelu_from_col = from_col; return *this; }
  // C = C + gate[b, col] * (acc + bias): the gated residual in place on the output
  Gemm& gate_res(const void* gate, int64_t gbs) {
    a.epilogue = EPI_BIAS_GATE_RES; a.gate = gate; a.gate_bstride = gbs; a.res = a.C; a.ldr = a.ldc; a.r_bstride = a.c_bstride;
    return *this;
  }
  Gemm& scratch(void* ws, int64_t bytes) { a.workspace = ws; a.workspace_bytes = bytes; return *this; }
  // row-split weights: rows [0, split_row) of every sample (the text rows of the joint stream) take l2 / gate2 / the norm weights wq2, wk2;
  // split_row = 0: not a joint launch, nothing to do
  Gemm& rowsplit(int split_row, const tfx_linear& l2, const void* gate2 = nullptr, const void* wq2 = nullptr, const void* wk2 = nullptr) {
    if (split_row <= 0) return *this;
    a.split_row = split_row; a.W2 = l2.w; a.bias2 = l2.b; a.gate2 = gate2; a.qkn_wq2 = wq2; a.qkn_wk2 = wk2; lin2 = &l2;
    return *this;
  }
  // the launch with the fused per-head RMSNorm + RoPE on the k / q column ranges [0, D) / [2D, 3D) of a [k | v | q | ...] projection
  GemmArgs with_qknorm(const void* wq, const void* wk, const float* cs, int64_t cs_bstride, int pos0, int D, float eps) const {
    GemmArgs q = a;
    q.qkn_wq = wq; q.qkn_wk = wk; q.qkn_rope_cs = cs; q.qkn_rope_bstride = cs_bstride; q.qkn_pos0 = pos0;
    q.qkn_k0 = 0; q.qkn_k1 = D; q.qkn_q0 = 2 * D; q.qkn_q1 = 3 * D; q.qkn_eps = eps;
    if (q.epilogue == EPI_BIAS) { q.epilogue = EPI_BIAS_GELU; q.gelu_from_col = 1 << 30; }   // bias only: GELU never starts
    return q;
  }
  bool adapted() const { return lin->lora_a || (a.split_row > 0 && lin2 && lin2->lora_a); }
  bool fp8_ready() const { return fp8 && lin->w8 && lin->w8_scale && a.K % 256 == 0; }

  // t = bf16(c * (x @ Acat^T)) into the T scratch that mirrors x's buffer, then the GEMM with the low-rank tail (gemm_bf16_lora)
  int run_lora(const Ctx& f) const {
    const tfx_dit_desc& d = f.d;
    if (!d.lora_t_xn || !d.lora_t_y || !d.lora_scale)
      return fail("dit_forward: a block Linear carries a runtime LoRA adapter but lora_t_xn / lora_t_y / lora_scale are null");
    const tfx_linear* l2 = a.split_row > 0 ? lin2 : nullptr;
    const tfx_linear& ref = lin->lora_a ? *lin : *l2;
    const int R = ref.lora_r, nseg = ref.lora_nseg;
    if (R <= 0 || nseg <= 0 || nseg > 4) return fail("dit_forward: bad lora_r / lora_nseg on an adapted Linear");
    if (l2 && (l2->ldw != lin->ldw || (l2->lora_a && lin->lora_a && (l2->lora_r != R || l2->lora_nseg != nseg))))
      return fail("dit_forward: the [img; txt] Linears of a joint launch must share ldw, lora_r and lora_nseg");
    const bool in_xn = in == &f.xn;
    if (!in_xn && in != &f.y) return fail("dit_forward: adapted Linear whose input is neither xn nor y");
    const int64_t hid_elems = f.B * f.hid_bs;
    const char* A = (const char*)a.A;
    char* T = const_cast<char*>(A) + (in_xn ? (const char*)d.lora_t_xn - (const char*)d.xn : (const char*)d.lora_t_y - (const char*)d.y);
    const bool planes = (int64_t)nseg * R > a.lda;        // the segments' T blocks do not fit one row: a matrix per segment
    if (planes && (!in_xn || d.D >= 1024)) return fail("dit_forward: lora_nseg * lora_r exceeds the input's row pitch");
    auto down = [&](const tfx_linear& l, int row0, int rows) -> int {
      if (!l.lora_a || rows <= 0) return 0;
      GemmArgs g = GemmArgs();
      g.A = A + (int64_t)row0 * a.lda * 2; g.lda = a.lda; g.a_bstride = a.a_bstride;
      g.ldw = a.K; g.bias = nullptr;
      g.ldc = a.lda; g.c_bstride = a.a_bstride;
      g.M = rows; g.K = a.K; g.batch = a.batch;
      g.epilogue = EPI_COLSCALE;
      g.workspace = a.workspace; g.workspace_bytes = a.workspace_bytes;
      for (int s = 0; s < (planes ? nseg : 1); ++s) {
        if (planes && !((l.lora_mask >> s) & 1)) continue;
        g.W = (const char*)l.lora_a + (int64_t)s * R * a.K * 2;
        g.C = T + (int64_t)row0 * a.lda * 2 + (int64_t)s * hid_elems * 2;
        g.N = planes ? R : nseg * R;
        g.cscale = d.lora_scale + l.lora_scale_off + s * R;
        if (int e = gemm_bf16(g, f.st)) return e;
      }
      return 0;
    };
    if (l2) {
      TRY(down(*l2, 0, a.split_row));
      TRY(down(*lin, a.split_row, a.M - a.split_row));
    } else {
      TRY(down(*lin, 0, a.M));
    }
    LoraArgs la{T, (const char*)a.W + (int64_t)a.K * 2, R, nseg > 1 ? d.D : a.N, nseg,
                (uint32_t)lin->lora_mask | (l2 ? (uint32_t)l2->lora_mask << 8 : 0u), planes ? hid_elems : 0};
    return gemm_bf16_lora(a, la, f.st);
  }

  // The launch(es) of the Linear: the runtime-LoRA tail; else, in fp8 mode on a Linear with w8 and K % 256 == 0, the e4m3 GEMM on
  // activation rows the producing LayerNorm quantised (ln_row0) or a quantisation pass writes to the head of the q8 workspace; else bf16.
  int run(const Ctx& f) const {
    if (adapted())
      return fp8 ? fail("dit_forward: runtime LoRA adapters and fp8 linears (flags bit 2) cannot be combined") : run_lora(f);
    if (!fp8_ready()) return gemm_bf16(a, f.st);
    GemmArgs g = a;
    if (ln_row0 >= 0) {
      g.A = (const uint8_t*)f.q8 + (int64_t)ln_row0 * f.D; g.lda = f.D; g.a_bstride = f.hid_bs;
      g.a_scale = f.q8s + ln_row0; g.a_scale_bstride = f.N;
    } else {
      g.A = f.q8; g.lda = a.K; g.a_bstride = (int64_t)a.M * a.K;
      g.a_scale = f.q8s; g.a_scale_bstride = a.M;
      TRY(quantize_rows_fp8(a.A, a.lda, a.a_bstride, f.q8, g.lda, g.a_bstride, f.q8s, a.M, a.M, a.batch, a.K, f.st));
    }
    g.W = lin->w8; g.w_scale = lin->w8_scale;
    return gemm_fp8(g, f.st);
  }
};

struct Forward : Ctx {
  using Ctx::Ctx;

  // A block Linear on a row group: columns [src_col, src_col + K) of `src` -> columns [dst_col, dst_col + n) of `dst`.  Every block
  // Linear gets the split-K scratch and, in fp8 mode, may run on its e4m3 weights; x_embedder and the final proj_out get neither.
  Gemm linear(const Buf& src, int src_col, const tfx_linear& l, int K, const Buf& dst, int dst_col, int n, const Rows& r) const {
    Gemm gm(src.p + r.row0 * src.ld + src_col, src.ld, src.bs, l, dst.p + r.row0 * dst.ld + dst_col, dst.ld, dst.bs, r.rows, n, K, B);
    gm.in = &src; gm.fp8 = q8 != nullptr;
    return gm.scratch(ws, ws_bytes);
  }

  // Does this q | k | v (| mlp) projection carry the per-head q / k RMSNorm + RoPE in its epilogue?  (Attached when so.)  It needs
  // the rotary table as pairs; the launch layer must take the shape -- asked with the scratch the launch will have: a GEMM the auto
  // path K-slices cannot carry it (persistent kernel, enough tiles to fill the chip unsplit; since round 5 in fp8 mode too) -- except
  // that the LoRA tail launch is never K-sliced, so the epilogue rides on every adapted projection.
  bool carries_qknorm(Gemm& gm, int pos0, const void* nq, const void* nk) const {
    if (!d.rope_cs) return false;
    const GemmArgs fused = gm.with_qknorm(nq, nk, d.rope_cs, d.rope_bstride, pos0, D, eps);
    if (!gm.adapted()) {
      if (gm.fp8_ready() && !g_fp8_fuse_qkn) return false;
      if (fused.split_row > 0 && !(fused.qkn_wq2 && fused.qkn_wk2)) return false;
      if (!(gm.fp8_ready() ? gemm_fp8_qkn_ok(fused) : gemm_qkn_ok(fused))) return false;
    }
    gm.a = fused;
    return true;
  }
  // LayerNorm + modulation (m = [shift | scale]) of a row group feeding ONE Linear, then that Linear.  A joint group is one split launch
  // (the text rows taking m_txt), or the image rows then the text rows under ln_joint = 0.  fp8 mode: the norm writes the e4m3 rows +
  // scales straight into the q8 workspace and the GEMM consumes them -- no bf16 round trip, no separate quantisation pass.
  int norm_run(const Rows& r, const uint16_t* m, const uint16_t* m_txt, Gemm gm) const {
    if (r.split > 0 && g_ln_joint) {
      TRY(ln_modulate_split(hid.p, xn.p, m, m + D, m_txt, m_txt + D, r.split, mbs, r.rows, B, D, D, hid_bs, D, hid_bs, eps, st));
    } else if (r.split > 0) {
      TRY(ln(r.split, r.rows - r.split, m, m + D));
      TRY(ln(0, r.split, m_txt, m_txt + D));
    } else if (gm.fp8_ready()) {
      TRY(ln_modulate_fp8(hid.p + (int64_t)r.row0 * D, (uint8_t*)q8 + (int64_t)r.row0 * D, q8s + r.row0, m, m + D, mbs, r.rows, B, D, D, hid_bs,
                          D, hid_bs, N, eps, st));
      gm.ln_row0 = r.row0;
    } else {
      TRY(ln(r.row0, r.rows, m, m + D));
    }
    return gm.run(*this);
  }
  // norm1 + the projection of a row group into y with q / k norm + RoPE: in the GEMM's epilogue, else as the separate pass behind it
  int project_qkv(const Rows& r, const uint16_t* m, const uint16_t* m_txt, Gemm gm, const void* nq, const void* nk, const void* nq_txt,
                  const void* nk_txt) const {
    const bool fused = carries_qknorm(gm, r.row0, nq, nk);
    TRY(norm_run(r, m, m_txt, gm));
    return fused ? 0 : norm_rope(r, nq, nk, nq_txt, nk_txt);
  }

  // ---- FluxTransformerBlock.forward (transformer_flux.py:794-841)
  int double_block(int blk) const {
    const tfx_double_block& w = d.dbl[blk];
    const uint16_t* mi = mod + (int64_t)blk * 12 * D;
    // a stream's Linears, q / k norm weights and modulation rows: shift_msa scale_msa gate_msa shift_mlp scale_mlp gate_mlp
    struct Stream { const tfx_linear &qkv, &out, &ff1, &ff2; const void *nq, *nk; const uint16_t* m; };
    const Stream img{w.qkv_img, w.out_img, w.ff1_img, w.ff2_img, w.norm_q, w.norm_k, mi};
    const Stream txt{w.qkv_txt, w.out_txt, w.ff1_txt, w.ff2_txt, w.norm_added_q, w.norm_added_k, mi + 6 * D};
    // The four Linears on a row group of stream s; a joint group (r.split = T) pairs them with the text stream's for the rows below T.
    struct Group { Rows r; const Stream* s; };
    auto qkv = [&](const Group& g) { return linear(xn, 0, g.s->qkv, D, y, 0, 3 * D, g.r).rowsplit(g.r.split, txt.qkv, nullptr, txt.nq, txt.nk); };
    auto out = [&](const Group& g) {     // hidden += gate_msa * to_out(attn)   (:817-818, 830-831)
      return linear(y, 2 * D, g.s->out, D, hid, 0, D, g.r).gate_res(g.s->m + 2 * D, mbs).rowsplit(g.r.split, txt.out, txt.m + 2 * D);
    };
    auto ff1 = [&](const Group& g) { return linear(xn, 0, g.s->ff1, D, y, 3 * D, 4 * D, g.r).gelu(0).rowsplit(g.r.split, txt.ff1); };
    auto ff2 = [&](const Group& g) {
      return linear(y, 3 * D, g.s->ff2, 4 * D, hid, 0, D, g.r).gate_res(g.s->m + 5 * D, mbs).rowsplit(g.r.split, txt.ff2, txt.m + 5 * D);
    };
    // The text and image Linears of the block as ONE launch each over the joint [text | image] rows (row-split weights) when the text
    // length is a whole number of tiles and the two weight matrices sit in one allocation (the engine's loader puts them there); else
    // the image rows, then the text rows.  bf16 mode only.
    const Group both{{0, N, T}, &img}, apart[2] = {{{T, Sn, 0}, &img}, {{0, T, 0}, &txt}};
    const bool joint = g_group_streams && T > 0 && !q8 && gemm_rowsplit_ok(qkv(both).a) && gemm_rowsplit_ok(out(both).a) &&
                       gemm_rowsplit_ok(ff1(both).a) && gemm_rowsplit_ok(ff2(both).a);
    const Group* const groups = joint ? &both : apart;
    const int ng = joint || T == 0 ? 1 : 2;
    for (int i = 0; i < ng; ++i) {
      const Group& g = groups[i];
      TRY(project_qkv(g.r, g.s->m, txt.m, qkv(g), g.s->nq, g.s->nk, txt.nq, txt.nk));
    }
    TRY(attention(w.attn_score_bound));
    for (int i = 0; i < ng; ++i) TRY(out(groups[i]).run(*this));
    // MLP: norm2 * (1 + scale_mlp) + shift_mlp -> ff -> gated residual (:820-826, 833-837)
    for (int i = 0; i < ng; ++i) TRY(norm_run(groups[i].r, groups[i].s->m + 3 * D, txt.m + 3 * D, ff1(groups[i])));
    for (int i = 0; i < ng; ++i) TRY(ff2(groups[i]).run(*this));
    return 0;
  }

  // ---- FluxSingleTransformerBlock.forward (transformer_flux.py:715-739) on the joint [text | image] sequence
  int single_block(int j) const {
    const tfx_single_block& w = d.sgl[j];
    const uint16_t* ms = mod + (int64_t)d.n_double * 12 * D + (int64_t)j * 3 * D;  // shift scale gate
    const Rows all{0, N, 0};
    TRY(project_qkv(all, ms, nullptr, linear(xn, 0, w.qkv_mlp, D, y, 0, 7 * D, all).gelu(3 * D), w.norm_q, w.norm_k, nullptr, nullptr));
    TRY(attention(w.attn_score_bound));
    return linear(y, 2 * D, w.proj_out, 5 * D, hid, 0, D, all).gate_res(ms + 2 * D, mbs).run(*this);
  }

  int forward() const {
    const int64_t xbs = (int64_t)Sn * d.in_channels;
    if (!(d.flags & 1)) {
      // x_embedder (transformer_flux.py:1086) straight into the image rows of the joint stream; text rows <- ctx0
      TRY(Gemm(d.xin, d.in_channels, xbs, d.x_embedder, hid.p + (int64_t)T * D, D, hid_bs, Sn, D, d.in_channels, B).run(*this));
      if (T > 0) TRY(copy_rows(d.ctx0, D, (int64_t)T * D, hid.p, D, hid_bs, T, D, B, st));
    }
    const int nblk = d.n_double + d.n_single;
    const int first = d.first_block < 0 ? 0 : d.first_block;
    const int last = (d.last_block < 0 || d.last_block > nblk) ? nblk : d.last_block;
    for (int blk = first; blk < last; ++blk) TRY(blk < d.n_double ? double_block(blk) : single_block(blk - d.n_double));
    if (!(d.flags & 2)) {
      // norm_out (AdaLayerNormContinuous: chunk order scale, shift) + proj_out on the image rows (:1200-1203)
      const uint16_t* mo = mod + (int64_t)d.n_double * 12 * D + (int64_t)d.n_single * 3 * D;
      TRY(ln(T, Sn, mo + D, mo));
      Gemm po(xn.p + (int64_t)T * D, D, hid_bs, d.proj_out, d.out, d.out_channels, (int64_t)Sn * d.out_channels, Sn, d.out_channels, D, B);
      po.in = &xn;   // bf16 without the scratch, but an adapter on it finds its T scratch like a block Linear's
      if (d.euler_gate) {
        // flow-matching Euler step in the epilogue: x' = x + bf16(dsigma * bf16(v)), in place on the latent columns of xin
        // (gate = the step's dsigma in every column, residual = output = xin[:, :, :out_channels])
        po.a.C = const_cast<void*>(d.xin); po.a.ldc = d.in_channels; po.a.c_bstride = xbs;
        po.gate_res(d.euler_gate, d.euler_gate_bstride);
      }
      TRY(po.run(*this));
    }
    return 0;
  }
};

}  // namespace

void set_fp8_fuse_qkn(int v) { g_fp8_fuse_qkn = v; }
void set_ln_joint(int v) { g_ln_joint = v; }
void set_gemm_group_streams(int v) { g_group_streams = v; }

int dit_forward(const tfx_dit_desc& d, hipStream_t st) {
  if (d.D != d.H * 128) return fail("dit_forward: inner dim %d != heads %d * 128", d.D, d.H);
  if (d.B <= 0 || d.S <= 0 || d.T < 0) return fail("dit_forward: bad B/S/T");
  if ((d.flags & 4) && (!d.q8 || !d.q8_scale)) return fail("dit_forward: fp8 flag set but the q8 workspace is null");
  if (d.seq_len && d.rope_bstride <= 0)
    return fail("dit_forward: seq_len (mixed-geometry batch) needs rope_bstride > 0: one rotary table per sample");
  if (d.rope_bstride < 0) return fail("dit_forward: rope_bstride must not be negative");
  return Forward(d, st).forward();
}

}  // namespace tfx
