// The two ends of FluxFillPipeline.__call__ around the VAE, as HBM-bound layout kernels (reference sites in
// D/pipelines/flux/pipeline_flux_fill.py and D/image_processor.py; "P:" / "IP:" below):
//   prep_image      IP:587-716 (tensor / PIL branches: /255, 2x-1) + P:2030 `image * (1 - mask)` + the bf16 cast of
//                   P:2031, written straight as the NHWC, 8-channel-padded input of the encoder's conv_in
//   pack_mask       P:1563-1580  mask [B,1,H,W] -> 8x8 pixel blocks -> 2x2 patchify -> [B,S,256] (binarised, IP:535-536)
//   sample_pack     P:1528-1530, 1554-1560  posterior sample (mean + std * eps), (z - shift) * scale, 2x2 patchify
//   unpack_latents  P:1752-1765, 2126-2127  un-patchify + z / scale + shift, written NHWC for the decoder's conv_in
//   postprocess     IP:718-771   denormalise, clamp, -> NCHW bf16 ("pt") / NHWC fp32 ("np") / NHWC uint8 ("pil")
// plus two helpers of the VAE mid-block attention (single head of dim C, D/models/attention_processor.py:2799-2881):
//   transpose       v [N, C] -> v^T [C, N] so that P @ v runs on the MFMA GEMM (C = A @ W^T)
//   row_softmax     bf16 softmax(scale * s) over rows of the fp32 score matrix (tfx_gemm_bf16_f32), fp32 statistics
// Every bf16 rounding point of the reference's op chain is kept (each torch op on bf16 tensors rounds its result).
// Python-scalar operands (shift_factor, scaling_factor) follow the semantics of the reference's DEVICE kernels: the scalar
// stays fp32 (opmath) and `tensor / scalar` is a multiply by the fp32 reciprocal -- torch's CPU kernels round the scalar to
// bf16 first and divide, so a bf16 CPU run of the reference differs from its GPU run in exactly these two places.
#include "common.h"
#include "launch.h"

#include <type_traits>

namespace tfx {

// flag |= 1 if any element is negative (VaeImageProcessor.preprocess skips the 2x-1 normalisation for tensors that are
// already in [-1, 1]: `if do_normalize and image.min() < 0: do_normalize = False`, IP:700-707) -- decided on the device
template <typename T>
__global__ __launch_bounds__(256) void any_negative_kernel(const T* __restrict__ x, int64_t n, int* __restrict__ flag) {
  bool neg = false;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    float v;
    if constexpr (sizeof(T) == 2) v = bf2f(x[i]); else v = x[i];
    neg |= v < 0.f;
  }
  if (__any(neg) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

__device__ __forceinline__ float ld_f(const float* p, int64_t i) { return p[i]; }
__device__ __forceinline__ float ld_f(const bf16_t* p, int64_t i) { return bf2f(p[i]); }
__device__ __forceinline__ float ld_f(const uint8_t* p, int64_t i) { return __fdiv_rn((float)p[i], 255.0f); }

// out[b, y, x, 0..7] = bf16( img * (1 - mask) ), channels C..7 zero.  TI: float / bf16 planes [B, C, H, W], or uint8
// interleaved [B, H, W, C] (values / 255).  mask (optional): float / uint8 [Bm, H, W], Bm in {1, B}.
// norm_mode: 0 none, 1 always 2x-1, 2 2x-1 unless *neg_flag != 0.
template <typename TI, typename TM>
__global__ __launch_bounds__(256) void prep_image_kernel(const TI* __restrict__ img, const TM* __restrict__ mask,
                                                         bf16_t* __restrict__ out, int B, int C, int H, int W, int mask_b,
                                                         int norm_mode, int binarize, const int* __restrict__ neg_flag) {
  const int64_t hw = (int64_t)H * W;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= B * hw) return;
  const int b = (int)(i / hw);
  const int64_t pix = i - b * hw;
  const bool norm = norm_mode == 1 || (norm_mode == 2 && *neg_flag == 0);
  float keep = 1.0f;
  if (mask) {
    float m = ld_f(mask, (mask_b == 1 ? 0 : b) * hw + pix);
    if (binarize) m = m < 0.5f ? 0.f : 1.f;
    keep = 1.0f - m;
  }
  float v[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    v[c] = 0.f;
    if (c < C) {
      float x;
      if constexpr (sizeof(TI) == 1) x = ld_f(img, (b * hw + pix) * C + c);
      else x = ld_f(img, ((int64_t)b * C + c) * hw + pix);
      if (norm) x = __fsub_rn(__fmul_rn(2.0f, x), 1.0f);
      v[c] = __fmul_rn(x, keep);
    }
  }
  *reinterpret_cast<u32x4*>(out + i * 8) = pack8(v);
}

// mask [Bm, H, W] -> out[b, t, col0 + (i*8+j)*4 + py*2+px] = mask[(2ty+py)*8 + i, (2tx+px)*8 + j], h = H/8, w = W/8,
// t = ty * (w/2) + tx.  One thread = one token x 8 consecutive packed columns (i, j0..j0+1, all four (py, px)).
template <typename TM>
__global__ __launch_bounds__(256) void pack_mask_kernel(const TM* __restrict__ mask, bf16_t* __restrict__ out, int B, int H,
                                                        int W, int mask_b, int binarize, int64_t ld, int col0) {
  const int h2 = H / 16, w2 = W / 16;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t S = (int64_t)h2 * w2;
  if (i >= B * S * 32) return;
  const int c8 = (int)(i & 31);
  const int64_t bt = i >> 5;
  const int b = (int)(bt / S);
  const int t = (int)(bt - b * S);
  const int ty = t / w2, tx = t - ty * w2;
  const int ii = c8 >> 2, j0 = (c8 & 3) * 2;
  const TM* mb = mask + (int64_t)(mask_b == 1 ? 0 : b) * H * W;
  float v[8];
#pragma unroll
  for (int jj = 0; jj < 2; ++jj)
#pragma unroll
    for (int pp = 0; pp < 4; ++pp) {
      const int y = (2 * ty + (pp >> 1)) * 8 + ii, x = (2 * tx + (pp & 1)) * 8 + j0 + jj;
      float m = ld_f(mb, (int64_t)y * W + x);
      if (binarize) m = m < 0.5f ? 0.f : 1.f;
      v[jj * 4 + pp] = m;
    }
  *reinterpret_cast<u32x4*>(out + bt * ld + col0 + c8 * 8) = pack8(v);
}

// The per-token packers of known-region and change-map sampling: in [B, H, W] uint8, one thread = one token =
// four latent pixels (ly, lx) = (2ty+py, 2tx+px), each reduced over the bytes of a window of the image:
//   mode 0  nearest, the references' F.interpolate: the one byte in[8 ly, 8 lx]
//   mode 1  cover: the 8x8 blocks of latent pixels [ly-grow, ly+grow] x [lx-grow, lx+grow] (clipped), each block row one 8-byte load
// `Reduce` folds the 8-byte words into its Acc (a single byte stands as the word that holds it alone), turns a pixel's Acc into the
// pixel's value and stores the token's four.

// The packed latent mask of known-region sampling: out [B, S, C] bf16 1.0 / 0.0 with out[b, t, c*4 + py*2+px] = m(ly, lx) for every c
// -- _pack_latents of the latent-resolution mask repeated over the latent channels (FluxInpaintPipeline.prepare_mask_latents,
// D/pipelines/flux/pipeline_flux_inpaint.py:615, :656-662).  m = 1 if any byte of the window is >= 128 (the top bit of a byte);
// C/8 equal 16-byte stores.
struct AnyTopBit {
  using Acc = uint64_t;
  bf16_t* out;
  int C;
  static __device__ __forceinline__ Acc merge(Acc any, uint64_t v) { return any | v; }
  static __device__ __forceinline__ uint32_t value(Acc any) { return (any & 0x8080808080808080ull) != 0; }
  __device__ __forceinline__ void store(int64_t i, const uint32_t (&on)[4]) const {
    float v[8];
#pragma unroll
    for (int pp = 0; pp < 4; ++pp) v[pp] = v[pp + 4] = on[pp] ? 1.0f : 0.0f;
    const u32x4 packed = pack8(v);
    bf16_t* o = out + i * C;
    for (int c8 = 0; c8 < C / 8; ++c8) *reinterpret_cast<u32x4*>(o + c8 * 8) = packed;
  }
};

// The hold bytes of change-map sampling: map (255 = free from the first step, 0 = never changes) -> hold [B, S, 4] uint8,
// hold[b, t, py*2+px] = 255 - g(ly, lx), g the maximum byte of the window, taken on the two 4-byte halves of a word; one 32-bit store.
struct ByteMax {
  using Acc = uint32_t;
  uint32_t* hold;
  static __device__ __forceinline__ Acc merge(Acc g, uint64_t v) {
#pragma unroll
    for (int k = 0; k < 8; ++k) g = max(g, (uint32_t)(v >> (8 * k)) & 0xffu);
    return g;
  }
  static __device__ __forceinline__ uint32_t value(Acc g) { return 255u - g; }
  __device__ __forceinline__ void store(int64_t i, const uint32_t (&byte)[4]) const {
    uint32_t word = 0;
#pragma unroll
    for (int pp = 0; pp < 4; ++pp) word |= byte[pp] << (8 * pp);
    hold[i] = word;
  }
};

template <class Reduce>
__global__ __launch_bounds__(256) void latent_pack_kernel(const uint8_t* __restrict__ in, const Reduce red, int B, int H, int W, int mode,
                                                          int grow) {
  const int h = H / 8, w = W / 8, h2 = H / 16, w2 = W / 16;
  const int64_t S = (int64_t)h2 * w2;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= B * S) return;
  const int b = (int)(i / S);
  const int t = (int)(i - b * S);
  const int ty = t / w2, tx = t - ty * w2;
  const uint8_t* mb = in + (int64_t)b * H * W;
  uint32_t px[4];
#pragma unroll
  for (int pp = 0; pp < 4; ++pp) {
    const int ly = 2 * ty + (pp >> 1), lx = 2 * tx + (pp & 1);
    if (mode == 0) {
      px[pp] = Reduce::value(mb[(int64_t)ly * 8 * W + lx * 8]);
    } else {
      const int r0 = max(ly - grow, 0) * 8, r1 = (min(ly + grow, h - 1) + 1) * 8;
      const int c0 = max(lx - grow, 0), c1 = min(lx + grow, w - 1);
      typename Reduce::Acc acc = 0;
      for (int r = r0; r < r1; ++r) {
        const uint64_t* rowp = reinterpret_cast<const uint64_t*>(mb + (int64_t)r * W);
        for (int c = c0; c <= c1; ++c) acc = Reduce::merge(acc, rowp[c]);
      }
      px[pp] = Reduce::value(acc);      // per branch: a pixel leaves either one as one register, not as a 64-bit Acc
    }
  }
  red.store(i, px);
}

// moments NHWC [B, h, w, 2L] (mean | logvar) bf16, eps [B, L, h, w] bf16 or fp32 (null: the mode) ->
// out[b, t, col0 + c*4 + py*2+px] = bf16chain( (mean + exp(0.5 * clamp(logvar)) * eps - shift) * scale ) at pixel
// (2ty+py, 2tx+px); every intermediate rounded to bf16 as the reference's bf16 tensor ops round them
// (DiagonalGaussianDistribution, D/models/autoencoders/vae.py:781-802; P:1530).
template <typename TE>
__global__ __launch_bounds__(256) void sample_pack_kernel(const bf16_t* __restrict__ mom, const TE* __restrict__ eps,
                                                          bf16_t* __restrict__ out, int B, int h, int w, int L, float shift,
                                                          float scale, int64_t ld, int col0) {
  const int h2 = h / 2, w2 = w / 2;
  const int64_t S = (int64_t)h2 * w2;
  const int cpt = L / 2;                       // 8-column groups per token (2 channels x 4 positions each)
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= B * S * cpt) return;
  const int g = (int)(i % cpt);
  const int64_t bt = i / cpt;
  const int b = (int)(bt / S);
  const int t = (int)(bt - b * S);
  const int ty = t / w2, tx = t - ty * w2;
  float v[8];
#pragma unroll
  for (int cc = 0; cc < 2; ++cc)
#pragma unroll
    for (int pp = 0; pp < 4; ++pp) {
      const int c = g * 2 + cc, y = 2 * ty + (pp >> 1), x = 2 * tx + (pp & 1);
      const bf16_t* m = mom + (((int64_t)b * h + y) * w + x) * (2 * L);
      const float mean = bf2f(m[c]);
      float z = mean;
      if (eps) {
        const float lv = fminf(fmaxf(bf2f(m[L + c]), -30.f), 20.f);
        const float sd = round_bf(expf(round_bf(0.5f * lv)));
        const float e = ld_f(eps, (((int64_t)b * L + c) * h + y) * w + x);
        z = round_bf(mean + round_bf(sd * round_bf(e)));
      }
      v[cc * 4 + pp] = round_bf(z - shift) * scale;
    }
  *reinterpret_cast<u32x4*>(out + bt * ld + col0 + g * 8) = pack8(v);
}

// latents [B, S, 4L] -> z NHWC [B, h, w, L] = bf16(bf16(lat * (1 / scale)) + shift); z[b, y, x, c] <- col c*4 + (y&1)*2 + (x&1)
// of token (y>>1, x>>1).  One thread = one pixel x 8 channels.
__global__ __launch_bounds__(256) void unpack_latents_kernel(const bf16_t* __restrict__ lat, int64_t ld, bf16_t* __restrict__ out,
                                                             int B, int h, int w, int L, float shift, float scale) {
  const int cg = L / 8;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)B * h * w * cg) return;
  const int g = (int)(i % cg);
  const int64_t p = i / cg;
  const int x = (int)(p % w);
  const int y = (int)((p / w) % h);
  const int b = (int)(p / ((int64_t)w * h));
  const bf16_t* row = lat + ((int64_t)b * (h / 2) * (w / 2) + (int64_t)(y >> 1) * (w / 2) + (x >> 1)) * ld + (y & 1) * 2 + (x & 1);
  const float inv_scale = __fdiv_rn(1.0f, scale);
  float v[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = round_bf(__fmul_rn(bf2f(row[(g * 8 + e) * 4]), inv_scale)) + shift;
  *reinterpret_cast<u32x4*>(out + i * 8) = pack8(v);
}

// x NHWC [B, H, W, Cs] bf16 (first C channels used), cropped to the window (y0, x0, Hc, Wc) -> mode 0: NCHW bf16,
// 1: NHWC fp32, 2: NHWC uint8 (round(255 v)), 3: NCHW fp32.  denorm: v = clamp(bf16(bf16(x * 0.5) + 0.5), 0, 1)
// (VaeImageProcessor.denormalize, IP:227-239).  The window is the callers' result crop (run_inference.py:460-465: only the
// scene part of the concatenated image is kept), applied before the image leaves the device.
__global__ __launch_bounds__(256) void postprocess_kernel(const bf16_t* __restrict__ x, void* __restrict__ out, int B, int H, int W,
                                                          int Cs, int C, int mode, int denorm, int y0, int x0, int Hc, int Wc) {
  const int64_t HWc = (int64_t)Hc * Wc;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= B * HWc) return;
  const int b = (int)(i / HWc);
  const int64_t pix = i - b * HWc;
  const int yy = (int)(pix / Wc), xx = (int)(pix - (int64_t)yy * Wc);
  const bf16_t* src = x + (((int64_t)b * H + y0 + yy) * W + x0 + xx) * Cs;
  for (int c = 0; c < C; ++c) {
    float v = bf2f(src[c]);
    if (denorm) v = fminf(fmaxf(round_bf(round_bf(v * 0.5f) + 0.5f), 0.f), 1.f);
    if (mode == 0) ((bf16_t*)out)[((int64_t)b * C + c) * HWc + pix] = f2bf(v);
    else if (mode == 1) ((float*)out)[i * C + c] = v;
    else if (mode == 2) ((uint8_t*)out)[i * C + c] = (uint8_t)rintf(__fmul_rn(v, 255.0f));
    else ((float*)out)[((int64_t)b * C + c) * HWc + pix] = v;
  }
}

// out[b][c, n] = in[b][n, c]  (64 x 64 tiles through LDS)
__global__ __launch_bounds__(256) void transpose_kernel(const bf16_t* __restrict__ in, int64_t ldi, int64_t ibs,
                                                        bf16_t* __restrict__ out, int64_t ldo, int64_t obs, int N, int C) {
  __shared__ bf16_t tile[64][66];
  const int b = blockIdx.z, n0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (int r = ty; r < 64; r += 4)
    if (n0 + r < N && c0 + tx < C) tile[r][tx] = in[b * ibs + (int64_t)(n0 + r) * ldi + c0 + tx];
  __syncthreads();
  for (int r = ty; r < 64; r += 4)
    if (c0 + r < C && n0 + tx < N) out[b * obs + (int64_t)(c0 + r) * ldo + n0 + tx] = tile[tx][r];
}

// p[r, :N] = bf16( softmax(scale * s[r, :N]) ): fp32 scores in (row stride lds), bf16 weights out (row stride ldp), fp32
// statistics, one 256-thread block per row (the row stays in L2 between the three passes).
__global__ __launch_bounds__(256) void row_softmax_kernel(const float* __restrict__ s, int64_t lds, bf16_t* __restrict__ pout,
                                                          int64_t ldp, int N, float scale_log2e) {
  __shared__ float red[4];
  const float* row = s + (int64_t)blockIdx.x * lds;
  bf16_t* prow = pout + (int64_t)blockIdx.x * ldp;
  const int tid = threadIdx.x;
  const bool vec = (N % 8 == 0) && (lds % 4 == 0) && (ldp % 8 == 0) && ((uintptr_t)s % 16 == 0) && ((uintptr_t)pout % 16 == 0);
  auto block_reduce = [&](float v, bool is_max) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float u = __shfl_xor(v, o, 64);
      v = is_max ? fmaxf(v, u) : v + u;
    }
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    return is_max ? fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])) : (red[0] + red[1]) + (red[2] + red[3]);
  };
  auto ld8 = [&](int c, float* f) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(row + c * 8), b = *reinterpret_cast<const f32x4*>(row + c * 8 + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) { f[e] = a[e]; f[4 + e] = b[e]; }
  };
  float mx = -INFINITY;
  if (vec) {
    for (int c = tid; c < N / 8; c += 256) {
      float f[8];
      ld8(c, f);
#pragma unroll
      for (int e = 0; e < 8; ++e) mx = fmaxf(mx, f[e]);
    }
  } else {
    for (int c = tid; c < N; c += 256) mx = fmaxf(mx, row[c]);
  }
  mx = block_reduce(mx, true);
  const float mc = mx * scale_log2e;
  float sum = 0.f;
  if (vec) {
    for (int c = tid; c < N / 8; c += 256) {
      float f[8];
      ld8(c, f);
#pragma unroll
      for (int e = 0; e < 8; ++e) sum += __builtin_amdgcn_exp2f(f[e] * scale_log2e - mc);
    }
  } else {
    for (int c = tid; c < N; c += 256) sum += __builtin_amdgcn_exp2f(row[c] * scale_log2e - mc);
  }
  sum = block_reduce(sum, false);
  const float inv = 1.0f / sum;
  if (vec) {
    for (int c = tid; c < N / 8; c += 256) {
      float f[8];
      ld8(c, f);
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] = __builtin_amdgcn_exp2f(f[e] * scale_log2e - mc) * inv;
      *reinterpret_cast<u32x4*>(prow + c * 8) = pack8(f);
    }
  } else {
    for (int c = tid; c < N; c += 256) prow[c] = f2bf(__builtin_amdgcn_exp2f(row[c] * scale_log2e - mc) * inv);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
static inline unsigned blocks_for(int64_t n) { return (unsigned)((n + 255) / 256); }

int any_negative(const void* x, int dtype, int64_t n, int* flag, hipStream_t st) {
  if (n <= 0) return 0;
  unsigned grid = blocks_for(n);
  if (grid > 4096) grid = 4096;
  if (dtype == 0) any_negative_kernel<float><<<grid, 256, 0, st>>>((const float*)x, n, flag);
  else if (dtype == 1) any_negative_kernel<bf16_t><<<grid, 256, 0, st>>>((const bf16_t*)x, n, flag);
  else return fail("any_negative: dtype must be 0 (f32) or 1 (bf16)");
  return check_launch("any_negative");
}

int prep_image(const void* img, int img_dtype, const void* mask, int mask_dtype, void* out, int B, int C, int H, int W,
               int mask_b, int norm_mode, int binarize, const int* neg_flag, hipStream_t st) {
  if (C < 1 || C > 8) return fail("prep_image: 1..8 channels");
  if (norm_mode == 2 && !neg_flag) return fail("prep_image: norm_mode 2 needs the negative-values flag");
  if (mask && mask_b != 1 && mask_b != B) return fail("prep_image: mask batch must be 1 or B");
  const int64_t n = (int64_t)B * H * W;
  if (n <= 0) return 0;
  const unsigned grid = blocks_for(n);
  bf16_t* o = (bf16_t*)out;
#define TFX_PREP(TI, TM) prep_image_kernel<TI, TM><<<grid, 256, 0, st>>>((const TI*)img, (const TM*)mask, o, B, C, H, W, mask_b, norm_mode, binarize, neg_flag)
  const int md = mask ? mask_dtype : 0;
  if (md != 0 && md != 2) return fail("prep_image: mask dtype must be 0 (f32) or 2 (u8)");
  switch (img_dtype * 4 + md) {
    case 0: TFX_PREP(float, float); break;
    case 2: TFX_PREP(float, uint8_t); break;
    case 4: TFX_PREP(bf16_t, float); break;
    case 6: TFX_PREP(bf16_t, uint8_t); break;
    case 8: TFX_PREP(uint8_t, float); break;
    case 10: TFX_PREP(uint8_t, uint8_t); break;
    default: return fail("prep_image: image dtype must be 0 (f32 planes), 1 (bf16 planes) or 2 (u8 interleaved)");
  }
#undef TFX_PREP
  return check_launch("prep_image");
}

// Composition of the pipeline's input canvas out of its parts (reference: run_inference.py:409-467 -- the rendered glyph
// image and the scene are stacked, glyph first, the glyph part of the mask is black -- and PIL's convert("L") of the RGB mask
// in VaeImageProcessor.preprocess): canvas [B, H, W, 3] u8, cmask [B, H, W] u8 from glyph [B, gh, gw, 3], scene [B, sh, sw, 3]
// and the scene's RGB mask [B, sh, sw, 3], all u8 interleaved.  dir 0: vertical (H = gh + sh, W = gw = sw), 1: horizontal.
// The grey value is Pillow's integer formula (L24 = 19595 R + 38470 G + 7471 B + 0x8000) >> 16, bit for bit.
__global__ __launch_bounds__(256) void compose_canvas_kernel(const uint8_t* __restrict__ glyph, const uint8_t* __restrict__ scene,
                                                             const uint8_t* __restrict__ smask, uint8_t* __restrict__ canvas,
                                                             uint8_t* __restrict__ cmask, int B, int gh, int gw, int sh, int sw,
                                                             int dir, int mask_rgb) {
  const int H = dir ? sh : gh + sh, W = dir ? gw + sw : sw;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)B * H * W) return;
  const int x = (int)(i % W);
  const int64_t by = i / W;
  const int y = (int)(by % H), b = (int)(by / H);
  const bool in_glyph = dir ? x < gw : y < gh;
  uint8_t r, g, bl, m0 = 0, m1 = 0, m2 = 0;
  if (in_glyph) {
    const uint8_t* p = glyph + (((int64_t)b * gh + y) * gw + x) * 3;
    r = p[0]; g = p[1]; bl = p[2];
  } else {
    const int sy = dir ? y : y - gh, sx = dir ? x - gw : x;
    const int64_t o = (((int64_t)b * sh + sy) * sw + sx) * 3;
    r = scene[o]; g = scene[o + 1]; bl = scene[o + 2];
    m0 = smask[o]; m1 = smask[o + 1]; m2 = smask[o + 2];
  }
  uint8_t* c = canvas + i * 3;
  c[0] = r; c[1] = g; c[2] = bl;
  if (mask_rgb) {            // the mask stays RGB when a resize follows (the reference resizes the RGB mask, then takes "L")
    uint8_t* mm = cmask + i * 3;
    mm[0] = m0; mm[1] = m1; mm[2] = m2;
  } else {
    cmask[i] = (uint8_t)((19595u * m0 + 38470u * m1 + 7471u * m2 + 0x8000u) >> 16);
  }
}

// PIL's convert("L") of interleaved RGB u8: (19595 R + 38470 G + 7471 B + 0x8000) >> 16.
__global__ __launch_bounds__(256) void rgb_to_grey_kernel(const uint8_t* __restrict__ rgb, uint8_t* __restrict__ out, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint8_t* p = rgb + i * 3;
  out[i] = (uint8_t)((19595u * p[0] + 38470u * p[1] + 7471u * p[2] + 0x8000u) >> 16);
}

// One pass of Pillow's 8-bit convolution resampler (libImaging/Resample.c: ImagingResampleHorizontal_8bpc / Vertical_8bpc)
// along the middle axis of in [outer][in_len][inner] -> out [outer][out_len][inner]: per output position xx the window
// [bounds[2xx], + bounds[2xx+1]) and its ksize fixed-point coefficients (22 fractional bits, precomputed on the host exactly as
// precompute_coeffs + normalize_coeffs_8bpc do), ss = 2^21 + sum in * k, out = clip8(ss >> 22).  Integer arithmetic: bit-exact.
__global__ __launch_bounds__(256) void resample_u8_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out,
                                                          const int* __restrict__ bounds, const int* __restrict__ coeffs, int ksize,
                                                          int64_t outer, int in_len, int out_len, int inner) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= outer * out_len * inner) return;
  const int e = (int)(i % inner);
  const int64_t ox = i / inner;
  const int xx = (int)(ox % out_len);
  const int64_t o = ox / out_len;
  const int xmin = bounds[2 * xx], xmax = bounds[2 * xx + 1];
  const int* k = coeffs + (int64_t)xx * ksize;
  const uint8_t* src = in + ((o * in_len + xmin) * inner + e);
  int ss = 1 << 21;
  for (int x = 0; x < xmax; ++x) ss += (int)src[(int64_t)x * inner] * k[x];
  ss >>= 22;
  out[i] = (uint8_t)(ss < 0 ? 0 : ss > 255 ? 255 : ss);
}

// ---- paste-back (DESIGN.md section 4 "Paste-back"): two window passes over a u8 mask and the blend, integer arithmetic only.
// One pass along the middle axis of in [outer][len][inner] -> out, the layout resample_u8_kernel walks: the x pass of a
// [B, H, W] mask is outer = B H, len = W, inner = 1, the y pass outer = B, len = H, inner = W.  One thread per output byte; a
// wave's 64 threads read 64 neighbouring bytes per window step (x pass: overlapping, y pass: one row segment).
//   OP 0 (dilate): max over |k| <= r, the window clipped at both ends of the axis.
//   OP 1 (box):    s = sum over |k| <= r of v[clamp(p + k, 0, len - 1)] (edge replicated), out = (2 s + n) / (2 n), n = 2 r + 1
//                  -- s <= 511 * 255, and the quotient is at most 255.
template <int OP>
__global__ __launch_bounds__(256) void window_pass_u8_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int64_t outer,
                                                             int len, int64_t inner, int r) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= outer * len * inner) return;
  const int64_t e = i % inner, op = i / inner;
  const int p = (int)(op % len);
  const uint8_t* src = in + (op / len) * len * inner + e;
  if constexpr (OP == 0) {
    const int lo = p - r < 0 ? 0 : p - r, hi = p + r > len - 1 ? len - 1 : p + r;
    unsigned m = 0;
    for (int k = lo; k <= hi; ++k) m = max(m, (unsigned)src[k * inner]);
    out[i] = (uint8_t)m;
  } else {
    unsigned s = 0;
    for (int k = p - r; k <= p + r; ++k) s += src[(int64_t)(k < 0 ? 0 : k > len - 1 ? len - 1 : k) * inner];
    const unsigned n = 2u * r + 1u;
    out[i] = (uint8_t)((2u * s + n) / (2u * n));
  }
}

// out = (orig (255 - a) + edit a + 127) / 255 per channel, a = alpha of the pixel; out may be orig (each thread reads the byte it
// writes, and no other), so neither carries __restrict__.
__global__ __launch_bounds__(256) void overlay_u8_kernel(const uint8_t* orig, const uint8_t* __restrict__ edit,
                                                         const uint8_t* __restrict__ alpha, uint8_t* out, int64_t n, int C) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const unsigned a = alpha[i / C];
  out[i] = (uint8_t)((orig[i] * (255u - a) + edit[i] * a + 127u) / 255u);
}

// ---- colour-matched paste-back (DESIGN.md section 4 "Per-line edits"): the moments a per-channel linear fit needs, and the blend
// through the fitted look-up table.  Integer arithmetic only, every sum in 64 bits: exact, whatever the partition.
constexpr int kMomentVals = 17;                      // n, then (sum a, sum b, sum a a, sum a b) per channel, C <= 4
constexpr int kMomentParts = 256;                    // workgroups per sample at the most: the finishing workgroup has one thread for each
static_assert((int64_t)kMomentParts * kMomentVals * 8 == MASKED_MOMENTS_SCRATCH_BYTES, "launch.h and the kernel disagree on the scratch bound");

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t lo = __shfl_xor((uint32_t)v, o, 64), hi = __shfl_xor((uint32_t)(v >> 32), o, 64);
    v += ((uint64_t)hi << 32) | lo;
  }
  return v;
}
// The workgroup's sum of each of the NV values its 256 threads hold: dst[k] = sum over the threads of acc[k] (plain stores).
template <int NV>
__device__ __forceinline__ void block_sum_u64(const uint64_t (&acc)[NV], uint64_t* __restrict__ dst) {
  __shared__ uint64_t red[4][NV];
  const int tid = threadIdx.x;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const uint64_t s = wave_sum_u64(acc[k]);
    if ((tid & 63) == 0) red[tid >> 6][k] = s;
  }
  __syncthreads();
  if (tid < NV) dst[tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}
// partials[b][part][0 .. 4 C] over the pixels of sample b with weight != 0 that workgroup `part` walks, four consecutive pixels per
// thread and step.  VEC (H W a multiple of 4 and every base pointer 4-byte aligned): the four weights are one 32-bit load and the
// 4 C bytes of a and of b are C 32-bit loads each; else byte loads, the last group cut at H W.
template <int C, bool VEC>
__global__ __launch_bounds__(256) void masked_moments_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
                                                             const uint8_t* __restrict__ weight, uint64_t* __restrict__ partials, int64_t hw) {
  const int s = blockIdx.y;
  a += (int64_t)s * hw * C; b += (int64_t)s * hw * C; weight += (int64_t)s * hw;
  uint64_t acc[1 + 4 * C];
#pragma unroll
  for (int k = 0; k < 1 + 4 * C; ++k) acc[k] = 0;
  const int64_t groups = (hw + 3) / 4;
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (int64_t)gridDim.x * 256) {
    const int64_t p0 = g * 4;
    uint8_t wv[4], av[4 * C], bv[4 * C];
    if constexpr (VEC) {
      const uint32_t w4 = *reinterpret_cast<const uint32_t*>(weight + p0);
      if (w4 == 0) continue;
#pragma unroll
      for (int j = 0; j < 4; ++j) wv[j] = (uint8_t)(w4 >> (8 * j));
#pragma unroll
      for (int q = 0; q < C; ++q) {
        const uint32_t a4 = *reinterpret_cast<const uint32_t*>(a + p0 * C + 4 * q), b4 = *reinterpret_cast<const uint32_t*>(b + p0 * C + 4 * q);
#pragma unroll
        for (int j = 0; j < 4; ++j) { av[4 * q + j] = (uint8_t)(a4 >> (8 * j)); bv[4 * q + j] = (uint8_t)(b4 >> (8 * j)); }
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool in = p0 + j < hw;
        wv[j] = in ? weight[p0 + j] : (uint8_t)0;
#pragma unroll
        for (int c = 0; c < C; ++c) {
          av[j * C + c] = wv[j] ? a[(p0 + j) * C + c] : (uint8_t)0;
          bv[j * C + c] = wv[j] ? b[(p0 + j) * C + c] : (uint8_t)0;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (!wv[j]) continue;
      acc[0] += 1;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const uint32_t x = av[j * C + c], y = bv[j * C + c];
        acc[1 + 4 * c] += x; acc[2 + 4 * c] += y; acc[3 + 4 * c] += x * x; acc[4 + 4 * c] += x * y;
      }
    }
  }
  block_sum_u64<1 + 4 * C>(acc, partials + ((int64_t)s * gridDim.x + blockIdx.x) * kMomentVals);
}
// One 256-thread workgroup per sample: thread t holds partial t (zeros beyond `parts` <= 256); out[b][c] = {n, sum a, sum b, sum a a, sum a b}.
template <int C>
__global__ __launch_bounds__(256) void masked_moments_finish_kernel(const uint64_t* __restrict__ partials, uint64_t* __restrict__ out, int parts) {
  const int s = blockIdx.x, tid = threadIdx.x;
  uint64_t acc[1 + 4 * C];
#pragma unroll
  for (int k = 0; k < 1 + 4 * C; ++k) acc[k] = tid < parts ? partials[((int64_t)s * parts + tid) * kMomentVals + k] : 0;
  __shared__ uint64_t tot[1 + 4 * C];
  block_sum_u64<1 + 4 * C>(acc, tot);
  __syncthreads();
  if (tid < 5 * C) {
    const int c = tid / 5, k = tid - 5 * c;
    out[((int64_t)s * C + c) * 5 + k] = k == 0 ? tot[0] : tot[4 * c + k];
  }
}

// out = (orig (255 - a) + lut[b][c][edit] a + 127) / 255: overlay_u8_kernel with the edit's byte sent through the table of its sample
// and channel, which the workgroup keeps in LDS (256 C bytes).  n = H W C bytes per sample.  VEC (n a multiple of 4, orig / edit / out
// 4-byte aligned): four consecutive bytes per thread and step, one 32-bit load of orig and of edit and one 32-bit store.  out may be
// orig: a thread reads the bytes it writes, and no others.
template <bool VEC>
__global__ __launch_bounds__(256) void overlay_lut_u8_kernel(const uint8_t* orig, const uint8_t* __restrict__ edit, const uint8_t* __restrict__ alpha,
                                                             const uint8_t* __restrict__ lut, uint8_t* out, int64_t n, int C) {
  __shared__ uint8_t tab[4 * 256];
  const int s = blockIdx.y;
  for (int k = threadIdx.x; k < 256 * C; k += 256) tab[k] = lut[(int64_t)s * 256 * C + k];
  __syncthreads();
  orig += s * n; edit += s * n; out += s * n; alpha += s * (n / C);
  if constexpr (VEC) {
    for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; i < n; i += (int64_t)gridDim.x * 1024) {
      const uint32_t o4 = *reinterpret_cast<const uint32_t*>(orig + i), e4 = *reinterpret_cast<const uint32_t*>(edit + i);
      int64_t pix = i / C;
      int c = (int)(i - pix * C);
      uint32_t r4 = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const unsigned al = alpha[pix], o = (o4 >> (8 * j)) & 255u, e = tab[c * 256 + ((e4 >> (8 * j)) & 255u)];
        r4 |= ((o * (255u - al) + e * al + 127u) / 255u) << (8 * j);
        if (++c == C) { c = 0; ++pix; }
      }
      *reinterpret_cast<uint32_t*>(out + i) = r4;
    }
  } else {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
      const int64_t pix = i / C;
      const unsigned al = alpha[pix], e = tab[(int)(i - pix * C) * 256 + edit[i]];
      out[i] = (uint8_t)((orig[i] * (255u - al) + e * al + 127u) / 255u);
    }
  }
}

// ---- seamless paste (DESIGN.md section 4 "Seamless paste"): a membrane v (i16, 6 fractional bits, C values per pixel) that equals
// ref - edit on the known pixels (alpha == 0 and covered) and is interpolated across alpha's support by a pull-push pyramid, then
// smoothed by Jacobi sweeps and added to the edit before the blend.  include/textflux_hip.h spells the arithmetic out; it is integer
// arithmetic only, so the result is exact.  Level l of a sample is (values i16 [h][w][C], flags u8 [h][w]); flag bit 0 = filled (at
// level 0: known), bit 1 (level 0 only) = free (alpha > 0).  One thread per pixel and all its channels; blockIdx.y = the sample in
// the per-level kernels.  Every neighbour index is clamped into its level, so no access leaves the workspace whatever the masks hold.
constexpr int kSeamFilled = 1, kSeamFree = 2;
constexpr int kSeamTopPixels = 2048;                 // the levels from the first one whose whole pyramid has at most this many pixels up to 1 x 1 are one launch, in LDS
constexpr int kSeamTopLevels = 16;                   // 2048 pixels halve to one in at most 12 levels
constexpr int kSeamMaxLevels = 33;                   // a side below 2^31 halves (rounding up) to 1 in at most 31 steps

__device__ __forceinline__ int seam_floor_div(int n, int d) {                // floor(n / d) for d > 0
  const int q = n / d;
  return (n % d < 0) ? q - 1 : q;
}

// Coarse pixel (y, x) of the level (hc, wc) from its up to four in-bounds, filled children in the fine level (h, w).
template <int C>
__device__ __forceinline__ void seam_pull_px(const int16_t* fv, const uint8_t* ff, int h, int w, int16_t* cv, uint8_t* cf, int wc, int y, int x) {
  int n = 0, s[C];
#pragma unroll
  for (int c = 0; c < C; ++c) s[c] = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int yy = 2 * y + (k >> 1), xx = 2 * x + (k & 1);
    if (yy >= h || xx >= w) continue;
    const int64_t p = (int64_t)yy * w + xx;
    if (!(ff[p] & kSeamFilled)) continue;
    ++n;
#pragma unroll
    for (int c = 0; c < C; ++c) s[c] += fv[p * C + c];
  }
  const int64_t o = (int64_t)y * wc + x;
  cf[o] = n > 0 ? kSeamFilled : 0;
#pragma unroll
  for (int c = 0; c < C; ++c) cv[o * C + c] = (int16_t)(n > 0 ? seam_floor_div(2 * s[c] + n, 2 * n) : 0);
}

// Unfilled fine pixel (y, x) of the level (h, w) from the complete coarse level (hc, wc): the 2x upsample with weights 9 3 3 1.
template <int C>
__device__ __forceinline__ void seam_push_px(int16_t* fv, const uint8_t* ff, int w, const int16_t* cv, int hc, int wc, int y, int x) {
  const int64_t p = (int64_t)y * w + x;
  if (ff[p] & kSeamFilled) return;
  const int i = y >> 1, j = x >> 1;
  int i2 = i + ((y & 1) ? 1 : -1), j2 = j + ((x & 1) ? 1 : -1);
  i2 = i2 < 0 ? 0 : i2 > hc - 1 ? hc - 1 : i2;
  j2 = j2 < 0 ? 0 : j2 > wc - 1 ? wc - 1 : j2;
  const int64_t a = ((int64_t)i * wc + j) * C, b = ((int64_t)i * wc + j2) * C, d = ((int64_t)i2 * wc + j) * C, e = ((int64_t)i2 * wc + j2) * C;
#pragma unroll
  for (int c = 0; c < C; ++c) fv[p * C + c] = (int16_t)((9 * cv[a + c] + 3 * cv[b + c] + 3 * cv[d + c] + cv[e + c] + 8) >> 4);
}

// Level 0: flags, and v = (ref - lut[edit]) * 64 on the known pixels, 0 elsewhere.  hw = H W pixels per sample.
template <int C>
__global__ __launch_bounds__(256) void seam_init_kernel(const uint8_t* __restrict__ ref, const uint8_t* __restrict__ edit,
                                                        const uint8_t* __restrict__ alpha, const uint8_t* __restrict__ covered,
                                                        const uint8_t* __restrict__ lut, int16_t* __restrict__ v, uint8_t* __restrict__ flags,
                                                        int64_t hw) {
  __shared__ uint8_t tab[C * 256];
  const int s = blockIdx.y;
  if (lut) {
    for (int k = threadIdx.x; k < 256 * C; k += 256) tab[k] = lut[(int64_t)s * 256 * C + k];
    __syncthreads();
  }
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= hw) return;
  const int64_t q = s * hw + p;
  const unsigned a = alpha[q];
  const bool known = a == 0 && (!covered || covered[q] != 0);
  flags[q] = (uint8_t)((known ? kSeamFilled : 0) | (a > 0 ? kSeamFree : 0));
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const int e = lut ? tab[c * 256 + edit[q * C + c]] : edit[q * C + c];
    v[q * C + c] = (int16_t)(known ? ((int)ref[q * C + c] - e) * 64 : 0);
  }
}

template <int C>
__global__ __launch_bounds__(256) void seam_pull_kernel(const int16_t* __restrict__ fv, const uint8_t* __restrict__ ff, int h, int w,
                                                        int16_t* __restrict__ cv, uint8_t* __restrict__ cf) {
  const int hc = (h + 1) / 2, wc = (w + 1) / 2;
  const int64_t n = (int64_t)hc * wc, k = (int64_t)blockIdx.x * 256 + threadIdx.x, s = blockIdx.y;
  if (k >= n) return;
  const int64_t fn = (int64_t)h * w;
  seam_pull_px<C>(fv + s * fn * C, ff + s * fn, h, w, cv + s * n * C, cf + s * n, wc, (int)(k / wc), (int)(k % wc));
}

template <int C>
__global__ __launch_bounds__(256) void seam_push_kernel(int16_t* __restrict__ fv, const uint8_t* __restrict__ ff, int h, int w,
                                                        const int16_t* __restrict__ cv) {
  const int hc = (h + 1) / 2, wc = (w + 1) / 2;
  const int64_t n = (int64_t)h * w, k = (int64_t)blockIdx.x * 256 + threadIdx.x, s = blockIdx.y;
  if (k >= n) return;
  seam_push_px<C>(fv + s * n * C, ff + s * n, w, cv + s * (int64_t)hc * wc * C, hc, wc, (int)(k / w), (int)(k % w));
}

// The small levels in one launch: one workgroup per sample loads the level (h, w) (its pyramid up to 1 x 1 has at most kSeamTopPixels
// pixels: the launcher picks it so), pulls up to 1 x 1 and pushes back down in LDS, and stores the completed level.  An unfilled 1 x 1
// top holds 0 (seam_pull_px writes 0 there, seam_init_kernel when the image itself is 1 x 1).
template <int C>
__global__ __launch_bounds__(256) void seam_top_kernel(int16_t* __restrict__ gv, const uint8_t* __restrict__ gf, int h, int w) {
  __shared__ int16_t sv[kSeamTopPixels * C];
  __shared__ uint8_t sf[kSeamTopPixels];
  int lh[kSeamTopLevels], lw[kSeamTopLevels], lo[kSeamTopLevels];
  int L = 0;
  lh[0] = h; lw[0] = w; lo[0] = 0;
  while ((lh[L] > 1 || lw[L] > 1) && L < kSeamTopLevels - 1) {
    lh[L + 1] = (lh[L] + 1) / 2; lw[L + 1] = (lw[L] + 1) / 2; lo[L + 1] = lo[L] + lh[L] * lw[L];
    ++L;
  }
  const int n0 = h * w, tid = threadIdx.x;
  gv += (int64_t)blockIdx.x * n0 * C;
  gf += (int64_t)blockIdx.x * n0;
  for (int k = tid; k < n0; k += 256) sf[k] = gf[k];
  for (int k = tid; k < n0 * C; k += 256) sv[k] = gv[k];
  __syncthreads();
  for (int l = 0; l < L; ++l) {
    const int wc = lw[l + 1], nc = lh[l + 1] * wc;
    for (int k = tid; k < nc; k += 256)
      seam_pull_px<C>(sv + lo[l] * C, sf + lo[l], lh[l], lw[l], sv + lo[l + 1] * C, sf + lo[l + 1], wc, k / wc, k % wc);
    __syncthreads();
  }
  for (int l = L - 1; l >= 0; --l) {
    const int wf = lw[l], nf = lh[l] * wf;
    for (int k = tid; k < nf; k += 256) seam_push_px<C>(sv + lo[l] * C, sf + lo[l], wf, sv + lo[l + 1] * C, lh[l + 1], lw[l + 1], k / wf, k % wf);
    __syncthreads();
  }
  for (int k = tid; k < n0 * C; k += 256) gv[k] = sv[k];
}

// One Jacobi sweep at level 0, src -> dst (two buffers: no pixel depends on the update order): free pixels become
// (N + S + E + W + 2) >> 2 with a neighbour outside the window counted as the centre; all others are copied.
template <int C>
__global__ __launch_bounds__(256) void seam_smooth_kernel(const int16_t* __restrict__ src, int16_t* __restrict__ dst,
                                                          const uint8_t* __restrict__ flags, int H, int W) {
  const int64_t hw = (int64_t)H * W, p = (int64_t)blockIdx.x * 256 + threadIdx.x, s = blockIdx.y;
  if (p >= hw) return;
  src += s * hw * C; dst += s * hw * C;
  if (!(flags[s * hw + p] & kSeamFree)) {
#pragma unroll
    for (int c = 0; c < C; ++c) dst[p * C + c] = src[p * C + c];
    return;
  }
  const int y = (int)(p / W), x = (int)(p % W);
  const int64_t pn = y > 0 ? p - W : p, ps = y < H - 1 ? p + W : p, pw = x > 0 ? p - 1 : p, pe = x < W - 1 ? p + 1 : p;
#pragma unroll
  for (int c = 0; c < C; ++c) dst[p * C + c] = (int16_t)((src[pn * C + c] + src[ps * C + c] + src[pe * C + c] + src[pw * C + c] + 2) >> 2);
}

// out = orig where alpha == 0, else (orig (255 - a) + e' a + 127) / 255 with e' = clamp(lut[edit] + clamp((v + 32) >> 6, -max_shift,
// max_shift), 0, 255).  out may be orig (a thread reads the bytes it writes, and no others), so neither carries __restrict__.
template <int C>
__global__ __launch_bounds__(256) void seam_apply_kernel(const uint8_t* orig, const uint8_t* __restrict__ edit, const uint8_t* __restrict__ alpha,
                                                         const uint8_t* __restrict__ lut, const int16_t* __restrict__ v, uint8_t* out, int64_t hw,
                                                         int max_shift) {
  __shared__ uint8_t tab[C * 256];
  const int s = blockIdx.y;
  if (lut) {
    for (int k = threadIdx.x; k < 256 * C; k += 256) tab[k] = lut[(int64_t)s * 256 * C + k];
    __syncthreads();
  }
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= hw) return;
  const int64_t q = s * hw + p;
  const unsigned a = alpha[q];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const unsigned o = orig[q * C + c];
    unsigned r = o;
    if (a > 0) {
      int e = lut ? tab[c * 256 + edit[q * C + c]] : edit[q * C + c];
      int d = ((int)v[q * C + c] + 32) >> 6;
      d = d < -max_shift ? -max_shift : d > max_shift ? max_shift : d;
      e += d;
      e = e < 0 ? 0 : e > 255 ? 255 : e;
      r = (o * (255u - a) + (unsigned)e * a + 127u) / 255u;
    }
    out[q * C + c] = (uint8_t)r;
  }
}

// ---- line warps (DESIGN.md section 4 "Rectified lines", "Perspective lines", "Curved lines"): out[b, j, i, :] = in[b] sampled at the
// image of the destination pixel (i, j) under a map, 4 x 4 Catmull-Rom taps, edge replicated.  Integer arithmetic only
// (include/textflux_hip.h spells it out), so the result is exact.  One kernel, warp_u8_kernel<C, Map>, does everything but the map: one
// 256-thread workgroup per 32 x 8 destination tile (its rotated source footprint is a compact patch of about 40 x 25 pixels that stays
// in cache), the bounds check, the output offset, warp_sample_u8, and the tail of a pixel without a source (0, coverage 0, `in` is not
// read).  A Map is a small functor passed by value -- it lives in the kernel arguments, hence in SGPRs -- whose one member takes
// (b, i, j, out_h, out_w) and either yields the integer position (xi, yi) with the fractions fx, fy in 0..255 to `sample`, or says
// `none()`: no source.  The two are continuations, not a returned flag: each map then compiles to the control flow it had as a kernel
// of its own (a flag costs the perspective map two VGPRs).  Three maps: WarpAffine, WarpPerspective, WarpGrid.  Every index is clamped
// into the image in 64 bits before it is narrowed: whatever a map holds, no load leaves `in`.
// warp_sample_u8: one destination pixel (its C bytes at `dst`, its coverage byte at `cov` unless NULL) from the sample `src` [H, W, C]
// at the integer position (xi, yi) with the fractions fx, fy in 0..255.
template <int C>
__device__ __forceinline__ void warp_sample_u8(const uint8_t* __restrict__ src, int H, int W, int64_t xi, int64_t yi, int fx, int fy,
                                               const int16_t* __restrict__ taps, uint8_t* __restrict__ dst, uint8_t* __restrict__ cov) {
  const int16_t* tx = taps + fx * 4;
  const int16_t* ty = taps + fy * 4;
  int cx[4];
  int64_t row[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t x = xi - 1 + k, y = yi - 1 + k;
    cx[k] = (int)(x < 0 ? 0 : x > W - 1 ? W - 1 : x) * C;
    row[k] = (y < 0 ? 0 : y > H - 1 ? H - 1 : y) * (int64_t)W * C;
  }
  int64_t acc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const uint8_t* p = src + row[r];
    int s[C];                        // |sum of a row's taps times a byte| < 2^23: 32 bits hold it; the same integer as the 64-bit sum
#pragma unroll
    for (int c = 0; c < C; ++c) s[c] = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int wx = tx[k];
#pragma unroll
      for (int c = 0; c < C; ++c) s[c] += wx * (int)p[cx[k] + c];
    }
    const int64_t wy = ty[r];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] += wy * s[c];
  }
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const int64_t v = (acc[c] + ((int64_t)1 << 27)) >> 28;
    dst[c] = (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
  }
  if (cov) *cov = (xi >= 0 && xi < W && yi >= 0 && yi < H) ? 255 : 0;
}

// Rectified lines: the Q16 affine image under p i64 [B][6].  The sample's matrix sits at an address that is uniform over the workgroup,
// so it is read once per workgroup, not once per thread.
struct WarpAffine {
  const int64_t* __restrict__ p;
  template <typename Sample, typename None>
  __device__ __forceinline__ void operator()(int b, int i, int j, int, int, const Sample& sample, const None&) const {
    const int64_t* mb = p + (int64_t)b * 6;
    const int64_t m0 = mb[0], m1 = mb[1], m2 = mb[2], m3 = mb[3], m4 = mb[4], m5 = mb[5];
    const int64_t X = m0 * i + m1 * j + m2, Y = m3 * i + m4 * j + m5;        // Q16
    sample(X >> 16, Y >> 16, (int)((X >> 8) & 255), (int)((Y >> 8) & 255));
  }
};

// Perspective lines: the homography p i64 [B][9].  Per destination pixel two rational positions Nx / D, Ny / D, brought to 8 fractional
// bits by a FLOOR division in 64-bit integers (the header spells it out).  At or behind the horizon (D <= 0) there is no source.
// Memory-safe whatever p holds: the linear forms and the * 256 wrap in unsigned arithmetic (no undefined signed overflow), D > 0 rules
// out the two faulting divisions (by 0, INT64_MIN / -1), and warp_sample_u8 clamps in 64 bits.  Two plain 64-bit divisions per pixel:
// measured beside the affine map by tools/perspective_cost.py.
__device__ __forceinline__ int64_t floor_div_pos(int64_t n, int64_t d) {     // floor(n / d) for d > 0; C++ truncates towards zero
  const int64_t q = n / d;
  return (n % d < 0) ? q - 1 : q;
}

struct WarpPerspective {
  const int64_t* __restrict__ p;
  template <typename Sample, typename None>
  __device__ __forceinline__ void operator()(int b, int i_, int j_, int, int, const Sample& sample, const None& none) const {
    const uint64_t* mb = (const uint64_t*)p + (int64_t)b * 9;
    const uint64_t i = (unsigned)i_, j = (unsigned)j_;           // zero-extended: the tile index is unsigned
    const uint64_t Nx = mb[0] * i + mb[1] * j + mb[2], Ny = mb[3] * i + mb[4] * j + mb[5];
    const int64_t D = (int64_t)(mb[6] * i + mb[7] * j + mb[8]);
    if (D <= 0) return none();
    const int64_t PX = floor_div_pos((int64_t)(Nx << 8), D), PY = floor_div_pos((int64_t)(Ny << 8), D);
    sample(PX >> 8, PY >> 8, (int)(PX & 255), (int)(PY & 255));
  }
};

// Curved lines: a coarse control grid, which is also the set's general remap (shift = 0: one node per pixel).  p i64 [B][gh][gw][2]
// holds the Q16 source position (x, y) of every destination pixel (q << shift, r << shift); a pixel's position is the bilinear blend of
// the four nodes around it, with integer weights that sum to 4^shift, floored by an arithmetic shift (the header spells it out).  A
// pixel one of whose four nodes carries INT64_MIN in x has no source.  The four nodes of a 32 x 8 tile's pixels are a few cache lines
// that the tile's lanes share.  Memory-safe whatever the grid holds: gh and gw are sized so that node (gy + 1, gx + 1) exists for every
// destination pixel, products and sums wrap in unsigned arithmetic, and warp_sample_u8 clamps in 64 bits.
struct WarpGrid {
  const int64_t* __restrict__ p;
  int shift;
  template <typename Sample, typename None>
  __device__ __forceinline__ void operator()(int b, int i, int j, int out_h, int out_w, const Sample& sample, const None& none) const {
    const int64_t gh = ((out_h - 1) >> shift) + 2, gw = ((out_w - 1) >> shift) + 2;
    const int cell = 1 << shift;
    const int gx = i >> shift, gy = j >> shift;
    const uint64_t ax = i & (cell - 1), ay = j & (cell - 1), bx = cell - ax, by = cell - ay;
    const uint64_t* g0 = (const uint64_t*)p + (((int64_t)b * gh + gy) * gw + gx) * 2;           // g00, g01 = g0 + 2
    const uint64_t* g1 = g0 + gw * 2;                                                            // g10, g11 = g1 + 2
    const uint64_t x00 = g0[0], y00 = g0[1], x01 = g0[2], y01 = g0[3], x10 = g1[0], y10 = g1[1], x11 = g1[2], y11 = g1[3];
    const uint64_t marker = (uint64_t)1 << 63;                                                    // INT64_MIN
    if (x00 == marker || x01 == marker || x10 == marker || x11 == marker) return none();
    const uint64_t w00 = bx * by, w01 = ax * by, w10 = bx * ay, w11 = ax * ay;
    const int64_t X = (int64_t)(w00 * x00 + w01 * x01 + w10 * x10 + w11 * x11) >> (2 * shift);   // Q16, floored
    const int64_t Y = (int64_t)(w00 * y00 + w01 * y01 + w10 * y10 + w11 * y11) >> (2 * shift);
    sample(X >> 16, Y >> 16, (int)((X >> 8) & 255), (int)((Y >> 8) & 255));
  }
};

template <int C, typename Map>
__global__ __launch_bounds__(256) void warp_u8_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out,
                                                      uint8_t* __restrict__ coverage, int H, int W, int out_h, int out_w, const Map map,
                                                      const int16_t* __restrict__ taps) {
  const int b = blockIdx.z;
  const unsigned i = blockIdx.x * 32 + (threadIdx.x & 31), j = blockIdx.y * 8 + (threadIdx.x >> 5);
  if (i >= (unsigned)out_w || j >= (unsigned)out_h) return;
  const int64_t o = ((int64_t)b * out_h + j) * out_w + i;
  const auto sample = [&](int64_t xi, int64_t yi, int fx, int fy) {
    warp_sample_u8<C>(in + (int64_t)b * H * W * C, H, W, xi, yi, fx, fy, taps, out + o * C, coverage ? coverage + o : nullptr);
  };
  const auto none = [&] {
#pragma unroll
    for (int c = 0; c < C; ++c) out[o * C + c] = 0;
    if (coverage) coverage[o] = 0;
  };
  map(b, (int)i, (int)j, out_h, out_w, sample, none);
}

// Candidates (DESIGN.md section 4 "Candidates"): every line crop of a batch in one launch.  table i64 [n][10] holds per crop (b, m0..m5,
// out_h, out_w, byte offset); crop k = blockIdx.y is images[b] under the Q16 matrix m, written as [out_h, out_w, C] at its byte offset
// in the packed buffer `out` -- the layout tfx_ocr_resize_norm reads.  The map is WarpAffine on the row's own six words and the taps are
// warp_sample_u8's: a crop is tfx_warp_affine_u8's bit for bit.  The crops' sizes live on the device, so the grid cannot be sized by
// them: gridDim.x workgroups walk a crop's 32 x 8 tiles in a stride, whatever their number.  The row's address is uniform over the
// workgroup.  A row that cannot be served (b outside [0, B), a side outside 1..kGatherMaxSide, [offset, offset + h w C) outside
// [0, out_bytes)) writes nothing and its first workgroup's first lane adds 1 to *refused (a vector atomic).  Stores are single bytes:
// a crop may start at any byte.  The side bound keeps h w C below 2^50 and the pixel indices inside an int.
static const int64_t kGatherMaxSide = (int64_t)1 << 24;

template <int C>
__global__ __launch_bounds__(256) void warp_gather_u8_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int64_t out_bytes,
                                                             const int64_t* __restrict__ table, int* __restrict__ refused, int B, int H,
                                                             int W, const int16_t* __restrict__ taps) {
  const int64_t* row = table + (int64_t)blockIdx.y * 10;
  const int64_t b = row[0], oh = row[7], ow = row[8], off = row[9];
  const bool served = b >= 0 && b < B && oh >= 1 && oh <= kGatherMaxSide && ow >= 1 && ow <= kGatherMaxSide && off >= 0 &&
                      off <= out_bytes && oh * ow * C <= out_bytes - off;
  if (!served) {
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(refused, 1);
    return;
  }
  const uint8_t* src = in + b * H * W * C;
  uint8_t* dst = out + off;
  const WarpAffine map{row + 1};
  const int64_t tiles_x = (ow + 31) >> 5, tiles = tiles_x * ((oh + 7) >> 3);
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int64_t ty = t / tiles_x;
    const int i = (int)(t - ty * tiles_x) * 32 + (threadIdx.x & 31), j = (int)ty * 8 + (threadIdx.x >> 5);
    if (i >= ow || j >= oh) continue;
    uint8_t* px = dst + ((int64_t)j * ow + i) * C;
    map(0, i, j, (int)oh, (int)ow,
        [&](int64_t xi, int64_t yi, int fx, int fy) { warp_sample_u8<C>(src, H, W, xi, yi, fx, fy, taps, px, nullptr); }, [] {});
  }
}

int compose_canvas(const void* glyph, const void* scene, const void* smask, void* canvas, void* cmask, int B, int gh, int gw, int sh,
                   int sw, int dir, int mask_rgb, hipStream_t st) {
  if (dir != 0 && dir != 1) return fail("compose_canvas: direction 0 (vertical) or 1 (horizontal)");
  if (dir == 0 ? gw != sw : gh != sh) return fail("compose_canvas: glyph and scene must share the side they are stacked along");
  const int64_t n = (int64_t)B * (dir ? sh : gh + sh) * (dir ? gw + sw : sw);
  if (n <= 0) return 0;
  compose_canvas_kernel<<<blocks_for(n), 256, 0, st>>>((const uint8_t*)glyph, (const uint8_t*)scene, (const uint8_t*)smask,
                                                       (uint8_t*)canvas, (uint8_t*)cmask, B, gh, gw, sh, sw, dir, mask_rgb);
  return check_launch("compose_canvas");
}

int rgb_to_grey(const void* rgb, void* out, int64_t n, hipStream_t st) {
  if (n <= 0) return 0;
  rgb_to_grey_kernel<<<blocks_for(n), 256, 0, st>>>((const uint8_t*)rgb, (uint8_t*)out, n);
  return check_launch("rgb_to_grey");
}

int resample_u8(const void* in, void* out, const int* bounds, const int* coeffs, int ksize, int64_t outer, int in_len, int out_len,
                int inner, hipStream_t st) {
  if (ksize < 1 || in_len < 1 || out_len < 1 || inner < 1) return fail("resample_u8: bad geometry");
  const int64_t n = outer * out_len * inner;
  if (n <= 0) return 0;
  resample_u8_kernel<<<blocks_for(n), 256, 0, st>>>((const uint8_t*)in, (uint8_t*)out, bounds, coeffs, ksize, outer, in_len, out_len, inner);
  return check_launch("resample_u8");
}

static const int64_t kMaxBytes = (int64_t)1 << 38;   // one thread per byte, 256 per block: the grid stays below 2^31 blocks

static int window_geometry(const char* what, int B, int H, int W, int radius) {
  if (B < 1 || H < 1 || W < 1) return fail("%s: B, H, W must be at least 1", what);
  if (radius < 0 || radius > 255) return fail("%s: radius must be in [0, 255]", what);
  if ((int64_t)B * H * W > kMaxBytes) return fail("%s: more than 2^38 pixels", what);
  return 0;
}

template <int OP>
static void window_pass(const uint8_t* in, uint8_t* out, int B, int H, int W, int radius, bool along_x, hipStream_t st) {
  const int64_t n = (int64_t)B * H * W;
  if (along_x) window_pass_u8_kernel<OP><<<blocks_for(n), 256, 0, st>>>(in, out, (int64_t)B * H, W, 1, radius);
  else window_pass_u8_kernel<OP><<<blocks_for(n), 256, 0, st>>>(in, out, B, H, W, radius);
}

int mask_dilate_u8(const void* in, void* out, void* tmp, int B, int H, int W, int radius, hipStream_t st) {
  if (window_geometry("mask_dilate_u8", B, H, W, radius)) return 1;
  if (in == out || in == tmp || out == tmp) return fail("mask_dilate_u8: in, out and tmp must be three different buffers");
  window_pass<0>((const uint8_t*)in, (uint8_t*)tmp, B, H, W, radius, true, st);
  window_pass<0>((const uint8_t*)tmp, (uint8_t*)out, B, H, W, radius, false, st);
  return check_launch("mask_dilate_u8");
}

int mask_feather_u8(const void* in, void* out, void* tmp, int B, int H, int W, int radius, hipStream_t st) {
  if (window_geometry("mask_feather_u8", B, H, W, radius)) return 1;
  if (in == out || in == tmp || out == tmp) return fail("mask_feather_u8: in, out and tmp must be three different buffers");
  const uint8_t* src = (const uint8_t*)in;
  uint8_t* a = (uint8_t*)tmp;
  uint8_t* b = (uint8_t*)out;
  for (int pass = 0; pass < 6; ++pass) {       // x x x y y y; in -> tmp -> out -> tmp -> out -> tmp -> out
    window_pass<1>(src, a, B, H, W, radius, pass < 3, st);
    src = a;
    uint8_t* t = a; a = b; b = t;
  }
  return check_launch("mask_feather_u8");
}

int overlay_u8(const void* orig, const void* edit, const void* alpha, void* out, int B, int H, int W, int C, hipStream_t st) {
  if (B < 1 || H < 1 || W < 1 || C < 1) return fail("overlay_u8: B, H, W, C must be at least 1");
  if (edit == out || alpha == out) return fail("overlay_u8: out may alias orig only");
  const int64_t n = (int64_t)B * H * W * C;
  if (n > kMaxBytes) return fail("overlay_u8: more than 2^38 bytes");
  overlay_u8_kernel<<<blocks_for(n), 256, 0, st>>>((const uint8_t*)orig, (const uint8_t*)edit, (const uint8_t*)alpha, (uint8_t*)out, n, C);
  return check_launch("overlay_u8");
}

static inline bool aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }

template <int C>
static void masked_moments_launch(const uint8_t* a, const uint8_t* b, const uint8_t* w, uint64_t* out, uint64_t* scratch, int B, int64_t hw,
                                  hipStream_t st) {
  const int64_t groups = (hw + 3) / 4;
  const int parts = (int)(groups >= 256ll * kMomentParts ? kMomentParts : (groups + 255) / 256);
  if (hw % 4 == 0 && aligned4(a) && aligned4(b) && aligned4(w)) masked_moments_kernel<C, true><<<dim3(parts, B), 256, 0, st>>>(a, b, w, scratch, hw);
  else masked_moments_kernel<C, false><<<dim3(parts, B), 256, 0, st>>>(a, b, w, scratch, hw);
  masked_moments_finish_kernel<C><<<B, 256, 0, st>>>(scratch, out, parts);
}

int masked_moments_u8(const void* a, const void* b, const void* weight, void* out, void* scratch, int64_t scratch_bytes, int B, int H, int W,
                      int C, hipStream_t st) {
  if (B < 1 || H < 1 || W < 1) return fail("masked_moments_u8: B, H, W must be at least 1");
  if (C < 1 || C > 4) return fail("masked_moments_u8: 1..4 channels");
  if (B > 65535) return fail("masked_moments_u8: batch %d exceeds 65535", B);
  if ((int64_t)H * W * C > kMaxBytes) return fail("masked_moments_u8: more than 2^38 bytes per sample");
  if (scratch_bytes < (int64_t)B * MASKED_MOMENTS_SCRATCH_BYTES)
    return fail("masked_moments_u8: scratch of %lld bytes, needs %lld per sample", (long long)scratch_bytes, (long long)MASKED_MOMENTS_SCRATCH_BYTES);
  if (((uintptr_t)out | (uintptr_t)scratch) & 7) return fail("masked_moments_u8: out and scratch must be 8-byte aligned");
  const uint8_t *pa = (const uint8_t*)a, *pb = (const uint8_t*)b, *pw = (const uint8_t*)weight;
  uint64_t *po = (uint64_t*)out, *ps = (uint64_t*)scratch;
  const int64_t hw = (int64_t)H * W;
  switch (C) {
    case 1: masked_moments_launch<1>(pa, pb, pw, po, ps, B, hw, st); break;
    case 2: masked_moments_launch<2>(pa, pb, pw, po, ps, B, hw, st); break;
    case 3: masked_moments_launch<3>(pa, pb, pw, po, ps, B, hw, st); break;
    default: masked_moments_launch<4>(pa, pb, pw, po, ps, B, hw, st); break;
  }
  return check_launch("masked_moments_u8");
}

int overlay_lut_u8(const void* orig, const void* edit, const void* alpha, const void* lut, void* out, int B, int H, int W, int C, hipStream_t st) {
  if (B < 1 || H < 1 || W < 1) return fail("overlay_lut_u8: B, H, W must be at least 1");
  if (C < 1 || C > 4) return fail("overlay_lut_u8: 1..4 channels");
  if (B > 65535) return fail("overlay_lut_u8: batch %d exceeds 65535", B);
  if (edit == out || alpha == out || lut == out) return fail("overlay_lut_u8: out may alias orig only");
  const int64_t n = (int64_t)H * W * C;
  if (n > kMaxBytes) return fail("overlay_lut_u8: more than 2^38 bytes per sample");
  const bool vec = n % 4 == 0 && aligned4(orig) && aligned4(edit) && aligned4(out);
  const int64_t per_block = vec ? 1024 : 256;
  const int64_t want = (n + per_block - 1) / per_block;
  const unsigned grid = (unsigned)(want > 4096 ? 4096 : want);      // grid-stride beyond: the table is loaded once per workgroup
  if (vec) overlay_lut_u8_kernel<true><<<dim3(grid, B), 256, 0, st>>>((const uint8_t*)orig, (const uint8_t*)edit, (const uint8_t*)alpha,
                                                                      (const uint8_t*)lut, (uint8_t*)out, n, C);
  else overlay_lut_u8_kernel<false><<<dim3(grid, B), 256, 0, st>>>((const uint8_t*)orig, (const uint8_t*)edit, (const uint8_t*)alpha,
                                                                   (const uint8_t*)lut, (uint8_t*)out, n, C);
  return check_launch("overlay_lut_u8");
}

// The seamless paste's workspace: per level the values i16 [B][h][w][C] and the flags u8 [B][h][w], level 0 with a second value buffer
// for the Jacobi ping-pong; every part starts at a multiple of 16 bytes.  Host arithmetic only.
struct SeamLayout {
  int levels;                                        // level `levels - 1` is 1 x 1
  int h[kSeamMaxLevels], w[kSeamMaxLevels];
  int64_t v[kSeamMaxLevels], f[kSeamMaxLevels], v0b, bytes;
  int top;                                           // the level seam_top_kernel starts from
};

static int seam_geometry(const char* what, int B, int H, int W, int C) {
  if (B < 1 || H < 1 || W < 1) return fail("%s: B, H, W must be at least 1", what);
  if (C < 1 || C > 4) return fail("%s: 1..4 channels", what);
  if (B > 65535) return fail("%s: batch %d exceeds 65535", what, B);
  if ((int64_t)H * W * C > kMaxBytes) return fail("%s: more than 2^38 bytes per sample", what);
  return 0;
}

static void seam_layout(int B, int H, int W, int C, SeamLayout* L) {
  auto up16 = [](int64_t n) { return (n + 15) & ~(int64_t)15; };
  int n = 0;
  L->h[0] = H; L->w[0] = W;
  while (L->h[n] > 1 || L->w[n] > 1) {
    L->h[n + 1] = (L->h[n] + 1) / 2; L->w[n + 1] = (L->w[n] + 1) / 2;
    ++n;
  }
  L->levels = n + 1;
  int64_t off = 0, tail = 0;
  L->top = n;
  for (int l = n; l >= 0; --l) {                     // the lowest level whose pyramid fits seam_top_kernel's LDS
    tail += (int64_t)L->h[l] * L->w[l];
    if (tail <= kSeamTopPixels && n - l < kSeamTopLevels) L->top = l;
  }
  for (int l = 0; l <= n; ++l) {
    const int64_t px = (int64_t)B * L->h[l] * L->w[l];
    L->v[l] = off; off += up16(px * C * 2);
    if (l == 0) { L->v0b = off; off += up16(px * C * 2); }
    L->f[l] = off; off += up16(px);
  }
  L->bytes = off;
}

int64_t seamless_workspace_bytes(int B, int H, int W, int C) {
  if (seam_geometry("seamless_workspace_bytes", B, H, W, C)) return -1;
  SeamLayout L;
  seam_layout(B, H, W, C, &L);
  return L.bytes;
}

template <int C>
static void seamless_launch(const uint8_t* orig, const uint8_t* ref, const uint8_t* edit, const uint8_t* alpha, const uint8_t* covered,
                            const uint8_t* lut, uint8_t* out, char* ws, const SeamLayout& L, int B, int smooth, int max_shift, hipStream_t st) {
  auto V = [&](int l) { return (int16_t*)(ws + L.v[l]); };
  auto F = [&](int l) { return (uint8_t*)(ws + L.f[l]); };
  auto grid = [&](int l) { return dim3(blocks_for((int64_t)L.h[l] * L.w[l]), B); };
  const int64_t hw = (int64_t)L.h[0] * L.w[0];
  seam_init_kernel<C><<<grid(0), 256, 0, st>>>(ref, edit, alpha, covered, lut, V(0), F(0), hw);
  for (int l = 0; l < L.top; ++l) seam_pull_kernel<C><<<grid(l + 1), 256, 0, st>>>(V(l), F(l), L.h[l], L.w[l], V(l + 1), F(l + 1));
  seam_top_kernel<C><<<B, 256, 0, st>>>(V(L.top), F(L.top), L.h[L.top], L.w[L.top]);
  for (int l = L.top - 1; l >= 0; --l) seam_push_kernel<C><<<grid(l), 256, 0, st>>>(V(l), F(l), L.h[l], L.w[l], V(l + 1));
  int16_t *cur = V(0), *other = (int16_t*)(ws + L.v0b);
  for (int k = 0; k < smooth; ++k) {
    seam_smooth_kernel<C><<<grid(0), 256, 0, st>>>(cur, other, F(0), L.h[0], L.w[0]);
    int16_t* t = cur; cur = other; other = t;
  }
  seam_apply_kernel<C><<<grid(0), 256, 0, st>>>(orig, edit, alpha, lut, cur, out, hw, max_shift);
}

int seamless_overlay_u8(const void* orig, const void* ref, const void* edit, const void* alpha, const void* covered, const void* lut, void* out,
                        void* workspace, int64_t workspace_bytes, int B, int H, int W, int C, int smooth, int max_shift, hipStream_t st) {
  if (seam_geometry("seamless_overlay_u8", B, H, W, C)) return 1;
  if (smooth < 0 || smooth > 255) return fail("seamless_overlay_u8: smooth must be in [0, 255]");
  if (max_shift < 0 || max_shift > 255) return fail("seamless_overlay_u8: max_shift must be in [0, 255]");
  if (edit == out || alpha == out || covered == out || lut == out || workspace == out || (ref == out && ref != orig))
    return fail("seamless_overlay_u8: out may alias orig only");
  SeamLayout L;
  seam_layout(B, H, W, C, &L);
  if (workspace_bytes < L.bytes)
    return fail("seamless_overlay_u8: workspace of %lld bytes, needs %lld (tfx_seamless_workspace_bytes)", (long long)workspace_bytes, (long long)L.bytes);
  if ((uintptr_t)workspace & 15) return fail("seamless_overlay_u8: workspace must be 16-byte aligned");
  const uint8_t *po = (const uint8_t*)orig, *pr = (const uint8_t*)ref, *pe = (const uint8_t*)edit, *pa = (const uint8_t*)alpha,
                *pc = (const uint8_t*)covered, *pl = (const uint8_t*)lut;
  switch (C) {
    case 1: seamless_launch<1>(po, pr, pe, pa, pc, pl, (uint8_t*)out, (char*)workspace, L, B, smooth, max_shift, st); break;
    case 2: seamless_launch<2>(po, pr, pe, pa, pc, pl, (uint8_t*)out, (char*)workspace, L, B, smooth, max_shift, st); break;
    case 3: seamless_launch<3>(po, pr, pe, pa, pc, pl, (uint8_t*)out, (char*)workspace, L, B, smooth, max_shift, st); break;
    default: seamless_launch<4>(po, pr, pe, pa, pc, pl, (uint8_t*)out, (char*)workspace, L, B, smooth, max_shift, st); break;
  }
  return check_launch("seamless_overlay_u8");
}

// ---- grain match (DESIGN.md section 4 "Grain match"): the histogram of a high-pass residual, from whose median the host estimates a
// noise level, and hashed white grain added under alpha.  Integer arithmetic only: counts and bytes are exact, whatever the partition.
constexpr int kHistBins = 1024;
constexpr int kHistParts = 256;                      // workgroups per sample at the most; grid-stride beyond

// out[b][c][min(|r_c|, 1023)] += 1 over the pixels of sample b with lo <= sel <= hi, r_c = 16 p - sum w p', w = [1 2 1] x [1 2 1] over the
// eight neighbours at distance `step` (1: the 3 x 3 neighbourhood; more: the a-trous form) with their indices clamped to the image.
// kSum adds row C, the histogram of min(|sum_c r_c|, 1023) over the same pixels.  One thread per pixel and step of the grid; the
// workgroup counts into its own histogram in LDS (4 KiB per row) and adds the bins it touched to `out` (zeroed by the caller on the same
// stream) with integer atomics: sums of integers, so the order does not matter.
template <int C, bool kSum>
__global__ __launch_bounds__(256) void highpass_hist_kernel(const uint8_t* __restrict__ img, const uint8_t* __restrict__ sel, int lo, int hi,
                                                            int step, uint32_t* __restrict__ out, int H, int W) {
  constexpr int kRows = C + (kSum ? 1 : 0);
  __shared__ uint32_t hist[kRows * kHistBins];
  for (int k = threadIdx.x; k < kRows * kHistBins; k += 256) hist[k] = 0;
  __syncthreads();
  const int s = blockIdx.y;
  const int64_t hw = (int64_t)H * W;
  img += (int64_t)s * hw * C; sel += (int64_t)s * hw;
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < hw; p += (int64_t)gridDim.x * 256) {
    const int m = sel[p];
    if (m < lo || m > hi) continue;
    const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
    const int64_t r0 = (int64_t)(y >= step ? y - step : 0) * W, r1 = (int64_t)y * W, r2 = (int64_t)(y < H - step ? y + step : H - 1) * W;
    const int x0 = x >= step ? x - step : 0, x2 = x < W - step ? x + step : W - 1;
    int sum = 0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      auto at = [&](int64_t row, int col) { return (int)img[(row + col) * C + c]; };
      const int blur = at(r0, x0) + 2 * at(r0, x) + at(r0, x2) + 2 * at(r1, x0) + 4 * at(r1, x) + 2 * at(r1, x2) + at(r2, x0) + 2 * at(r2, x) + at(r2, x2);
      int v = 16 * at(r1, x) - blur;
      sum += v;
      v = v < 0 ? -v : v;
      atomicAdd(&hist[c * kHistBins + (v > kHistBins - 1 ? kHistBins - 1 : v)], 1u);
    }
    if (kSum) {
      sum = sum < 0 ? -sum : sum;
      atomicAdd(&hist[C * kHistBins + (sum > kHistBins - 1 ? kHistBins - 1 : sum)], 1u);
    }
  }
  __syncthreads();
  out += (int64_t)s * kRows * kHistBins;
  for (int k = threadIdx.x; k < kRows * kHistBins; k += 256)
    if (hist[k]) atomicAdd(&out[k], hist[k]);
}

__device__ __forceinline__ uint32_t grain_mix(uint32_t h) {
  h ^= h >> 16; h *= 0x7feb352du; h ^= h >> 15; h *= 0x846ca68bu; h ^= h >> 16;
  return h;
}

// n in [-510, 510] of scene position (x, y), channel c and the seed (include/textflux_hip.h: tfx_grain_u8)
__device__ __forceinline__ int grain_noise(uint32_t x, uint32_t y, uint32_t c, uint32_t seed) {
  const uint32_t h = grain_mix(grain_mix(x * 0x9E3779B1u + y * 0x85EBCA77u + c * 0xC2B2AE3Du) ^ seed);
  return (int)((h & 255u) + ((h >> 8) & 255u) + ((h >> 16) & 255u) + (h >> 24)) - 510;
}

// out = clamp(img + d, 0, 255), d = floor((n gain[b][c] alpha + 255 * 32768) / (255 * 65536)) with n in [-510, 510] the sum of the four
// bytes of a hash of the pixel's SCENE position (origin + its place in the window), its channel and the seed, less 510.  One thread per
// byte; n = H W C bytes per sample.  out may be img: a thread reads the byte it writes, and no other.  A gain outside [0, 65536] is the
// caller's to refuse; it is clamped here so that the numerator stays within the bound the floor division below relies on.
__global__ __launch_bounds__(256) void grain_u8_kernel(const uint8_t* img, const uint8_t* __restrict__ alpha, const int32_t* __restrict__ gain,
                                                       const int32_t* __restrict__ origin, uint32_t seed, uint8_t* out, int64_t n, int W, int C) {
  const int s = blockIdx.y;
  img += s * n; out += s * n; alpha += s * (n / C);
  const uint32_t ox = origin ? (uint32_t)origin[2 * s] : 0u, oy = origin ? (uint32_t)origin[2 * s + 1] : 0u;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t pix = i / C;
    const int c = (int)(i - pix * C);
    const int64_t row = pix / W;
    const uint32_t x = ox + (uint32_t)(pix - row * W), y = oy + (uint32_t)row;
    int g = gain[s * C + c];
    g = g < 0 ? 0 : g > 65536 ? 65536 : g;
    const int nz = grain_noise(x, y, (uint32_t)c, seed);
    // floor division of a numerator that may be negative: |n gain alpha| <= 510 * 65536 * 255 = 510 den, so adding 510 den makes it
    // positive and takes exactly 510 off the quotient
    constexpr uint64_t den = 255ull * 65536ull;
    const int64_t num = (int64_t)nz * g * (int)alpha[pix] + 255 * 32768;
    const int d = (int)((uint64_t)(num + (int64_t)(510 * den)) / den) - 510;
    const int v = (int)img[i] + d;
    out[i] = (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
  }
}

// ---- grain spectrum (DESIGN.md section 4 "Grain spectrum"): the same grain, correlated over neighbouring pixels by a 3 x 3 blur and
// over the channels by a share of one common field.  A workgroup takes a 64 x 16 tile; its 256 threads are 64 columns by 4 rows.
constexpr int kShapeTW = 64, kShapeTH = 16;
constexpr int kShapeHW = kShapeTW + 2, kShapeHH = kShapeTH + 2;      // the tile with its one-pixel halo
constexpr int kShapeParts = 2048;                    // workgroups per sample at the most (256 CUs x 8 resident); each goes on to further tiles

// out = clamp(img + d, 0, 255), d = floor((f gain[b][c] alpha + 255 * 2^39) / (255 * 2^40)), f the [s, 256 - 2 s, s] x [s, 256 - 2 s, s]
// blur of m = (256 - lam) n(x, y, c) + lam n(x, y, 255) over the SCENE positions around the pixel (uint32 wrap-around, never clamped to
// the window: the halo is hashed, not read, so a pixel's grain does not depend on the window).  m of the tile and its halo is hashed
// into LDS once (66 x 18 x C ints, 19 KiB at the most) and filtered from there: lanes of a wave read consecutive dwords of one row.
// The rows pass fits 32 bits (|.| <= 256 * 130560); the columns pass and the product with gain and alpha take 64.  out may be img: a
// thread reads the byte it writes, and no other.  gain, s and lam are clamped into [0, 2^18], [0, 64] and [0, 256], the bounds the
// floor division relies on; the caller refuses what lies outside.
template <int C>
__global__ __launch_bounds__(256) void grain_shaped_kernel(const uint8_t* img, const uint8_t* __restrict__ alpha, const int32_t* __restrict__ gain,
                                                           const int32_t* __restrict__ shape, const int32_t* __restrict__ origin, uint32_t seed,
                                                           uint8_t* out, int H, int W, int tiles_x, int64_t tiles) {
  __shared__ int m[C][kShapeHH * kShapeHW];
  const int b = blockIdx.y;
  const int64_t hw = (int64_t)H * W;
  img += b * hw * C; out += b * hw * C; alpha += b * hw;
  const uint32_t ox = origin ? (uint32_t)origin[2 * b] : 0u, oy = origin ? (uint32_t)origin[2 * b + 1] : 0u;
  int s = shape[2 * b], lam = shape[2 * b + 1], g[C];
  s = s < 0 ? 0 : s > 64 ? 64 : s;
  lam = lam < 0 ? 0 : lam > 256 ? 256 : lam;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    g[c] = gain[b * C + c];
    g[c] = g[c] < 0 ? 0 : g[c] > (1 << 18) ? (1 << 18) : g[c];
  }
  const int k0 = s, k1 = 256 - 2 * s;
  const int tx = threadIdx.x & (kShapeTW - 1), ty = threadIdx.x / kShapeTW;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int tile_y = (int)(t / tiles_x), x0 = (int)(t - (int64_t)tile_y * tiles_x) * kShapeTW, y0 = tile_y * kShapeTH;
    for (int k = threadIdx.x; k < kShapeHH * kShapeHW; k += 256) {
      const int hy = k / kShapeHW, hx = k - hy * kShapeHW;
      const uint32_t x = ox + (uint32_t)(x0 + hx - 1), y = oy + (uint32_t)(y0 + hy - 1);
      const int shared = lam * grain_noise(x, y, 255u, seed);
#pragma unroll
      for (int c = 0; c < C; ++c) m[c][k] = (256 - lam) * grain_noise(x, y, (uint32_t)c, seed) + shared;
    }
    __syncthreads();
    const int x = x0 + tx;
    if (x < W) {
      for (int r = ty; r < kShapeTH && y0 + r < H; r += 256 / kShapeTW) {
        const int64_t pix = (int64_t)(y0 + r) * W + x;
        const int a = alpha[pix];
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const int* p = &m[c][r * kShapeHW + tx];                    // the halo's row r is the scene row above the pixel's
          const int h0 = k0 * (p[0] + p[2]) + k1 * p[1];
          const int h1 = k0 * (p[kShapeHW] + p[kShapeHW + 2]) + k1 * p[kShapeHW + 1];
          const int h2 = k0 * (p[2 * kShapeHW] + p[2 * kShapeHW + 2]) + k1 * p[2 * kShapeHW + 1];
          const int64_t f = (int64_t)k0 * ((int64_t)h0 + h2) + (int64_t)k1 * h1;
          // floor division of a numerator that may be negative: |f gain alpha| <= 130560 * 2^16 * 2^18 * 255 < 2041 den, so adding
          // 2048 den makes it positive (and stays below 2^63) and takes exactly 2048 off the quotient; den = 255 * 2^40, and
          // floor(floor(v / 2^40) / 255) = floor(v / den) for v >= 0, which leaves a 32-bit division
          constexpr int64_t den = 255ll << 40;
          const int64_t num = f * (int64_t)(g[c] * a) + (255ll << 39);
          const int d = (int)((uint32_t)((uint64_t)(num + 2048 * den) >> 40) / 255u) - 2048;
          const int v = (int)img[pix * C + c] + d;
          out[pix * C + c] = (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
        }
      }
    }
    __syncthreads();                                                  // before the next tile's hashes replace m
  }
}

static int grain_geometry(const char* what, int B, int H, int W, int C) {
  if (B < 1 || H < 1 || W < 1) return fail("%s: B, H, W must be at least 1", what);
  if (C < 1 || C > 4) return fail("%s: 1..4 channels", what);
  if (B > 65535) return fail("%s: batch %d exceeds 65535", what, B);
  if ((int64_t)H * W * C > kMaxBytes) return fail("%s: more than 2^38 bytes per sample", what);
  return 0;
}

// both histogram entry points: kSum false is tfx_highpass_hist_u8 (C rows, step 1), true tfx_highpass_hist_step_u8 (C + 1 rows)
template <bool kSum>
static int highpass_hist(const char* what, const void* img, const void* sel, int lo, int hi, int step, void* out, int B, int H, int W, int C,
                         hipStream_t st) {
  if (grain_geometry(what, B, H, W, C)) return 1;
  if (step < 1 || step > 8) return fail("%s: step must be in 1..8, got %d", what, step);
  const int64_t hw = (int64_t)H * W;
  if (hw > 0xffffffffll) return fail("%s: more than 2^32 - 1 pixels per sample (the counts are 32-bit)", what);
  if ((uintptr_t)out & 3) return fail("%s: out must be 4-byte aligned", what);
  if (out == img || out == sel) return fail("%s: out may alias neither img nor sel", what);
  if (hipMemsetAsync(out, 0, (size_t)B * (C + (kSum ? 1 : 0)) * kHistBins * 4, st) != hipSuccess) return fail("%s: clearing out failed", what);
  const int64_t want = (hw + 255) / 256;
  const dim3 grid((unsigned)(want > kHistParts ? kHistParts : want), B);
  const uint8_t *pi = (const uint8_t*)img, *ps = (const uint8_t*)sel;
  switch (C) {
    case 1: highpass_hist_kernel<1, kSum><<<grid, 256, 0, st>>>(pi, ps, lo, hi, step, (uint32_t*)out, H, W); break;
    case 2: highpass_hist_kernel<2, kSum><<<grid, 256, 0, st>>>(pi, ps, lo, hi, step, (uint32_t*)out, H, W); break;
    case 3: highpass_hist_kernel<3, kSum><<<grid, 256, 0, st>>>(pi, ps, lo, hi, step, (uint32_t*)out, H, W); break;
    default: highpass_hist_kernel<4, kSum><<<grid, 256, 0, st>>>(pi, ps, lo, hi, step, (uint32_t*)out, H, W); break;
  }
  return check_launch(what);
}

int highpass_hist_u8(const void* img, const void* sel, int lo, int hi, void* out, int B, int H, int W, int C, hipStream_t st) {
  return highpass_hist<false>("highpass_hist_u8", img, sel, lo, hi, 1, out, B, H, W, C, st);
}

int highpass_hist_step_u8(const void* img, const void* sel, int lo, int hi, int step, void* out, int B, int H, int W, int C, hipStream_t st) {
  return highpass_hist<true>("highpass_hist_step_u8", img, sel, lo, hi, step, out, B, H, W, C, st);
}

int grain_u8(const void* img, const void* alpha, const int* gain, const int* origin, uint32_t seed, void* out, int B, int H, int W, int C,
             hipStream_t st) {
  if (grain_geometry("grain_u8", B, H, W, C)) return 1;
  if (alpha == out || (const void*)gain == out || (origin && (const void*)origin == out)) return fail("grain_u8: out may alias img only");
  if (((uintptr_t)gain | (uintptr_t)origin) & 3) return fail("grain_u8: gain and origin must be 4-byte aligned");
  const int64_t n = (int64_t)H * W * C;
  const int64_t want = (n + 255) / 256;
  const dim3 grid((unsigned)(want > 4096 ? 4096 : want), B);          // grid-stride beyond, as overlay_lut_u8
  grain_u8_kernel<<<grid, 256, 0, st>>>((const uint8_t*)img, (const uint8_t*)alpha, gain, origin, seed, (uint8_t*)out, n, W, C);
  return check_launch("grain_u8");
}

int grain_shaped_u8(const void* img, const void* alpha, const int* gain, const int* shape, const int* origin, uint32_t seed, void* out, int B,
                    int H, int W, int C, hipStream_t st) {
  if (grain_geometry("grain_shaped_u8", B, H, W, C)) return 1;
  if (alpha == out || (const void*)gain == out || (const void*)shape == out || (origin && (const void*)origin == out))
    return fail("grain_shaped_u8: out may alias img only");
  if (((uintptr_t)gain | (uintptr_t)shape | (uintptr_t)origin) & 3) return fail("grain_shaped_u8: gain, shape and origin must be 4-byte aligned");
  const int tiles_x = (W + kShapeTW - 1) / kShapeTW;
  const int64_t tiles = (int64_t)tiles_x * ((H + kShapeTH - 1) / kShapeTH);
  const dim3 grid((unsigned)(tiles > kShapeParts ? kShapeParts : tiles), B);
  const uint8_t *pi = (const uint8_t*)img, *pa = (const uint8_t*)alpha;
  switch (C) {
    case 1: grain_shaped_kernel<1><<<grid, 256, 0, st>>>(pi, pa, gain, shape, origin, seed, (uint8_t*)out, H, W, tiles_x, tiles); break;
    case 2: grain_shaped_kernel<2><<<grid, 256, 0, st>>>(pi, pa, gain, shape, origin, seed, (uint8_t*)out, H, W, tiles_x, tiles); break;
    case 3: grain_shaped_kernel<3><<<grid, 256, 0, st>>>(pi, pa, gain, shape, origin, seed, (uint8_t*)out, H, W, tiles_x, tiles); break;
    default: grain_shaped_kernel<4><<<grid, 256, 0, st>>>(pi, pa, gain, shape, origin, seed, (uint8_t*)out, H, W, tiles_x, tiles); break;
  }
  return check_launch("grain_shaped_u8");
}

// ---- keyed paste (DESIGN.md section 4 "Keyed paste"): how much two images differ around a pixel, and the hysteresis threshold of that
// metric.  Integer arithmetic only, so both are exact whatever the partition.

// out[p] = max over the channels of (|s_c| + 8) >> 4, s_c = sum w (a - b) with w = [1 2 1] x [1 2 1] over the 3 x 3 neighbourhood, its
// indices clamped to the image: highpass_hist_kernel's stencil at step 1, on the difference.  |s_c| <= 16 * 255, so out <= 255.  One
// thread per pixel and step of the grid.
template <int C>
__global__ __launch_bounds__(256) void change_metric_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
                                                            uint8_t* __restrict__ out, int H, int W) {
  const int s = blockIdx.y;
  const int64_t hw = (int64_t)H * W;
  a += (int64_t)s * hw * C; b += (int64_t)s * hw * C; out += (int64_t)s * hw;
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < hw; p += (int64_t)gridDim.x * 256) {
    const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
    const int64_t r0 = (int64_t)(y > 0 ? y - 1 : 0) * W, r1 = (int64_t)y * W, r2 = (int64_t)(y < H - 1 ? y + 1 : H - 1) * W;
    const int x0 = x > 0 ? x - 1 : 0, x2 = x < W - 1 ? x + 1 : W - 1;
    int best = 0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      auto at = [&](int64_t row, int col) { const int64_t i = (row + col) * C + c; return (int)a[i] - (int)b[i]; };
      int v = at(r0, x0) + 2 * at(r0, x) + at(r0, x2) + 2 * at(r1, x0) + 4 * at(r1, x) + 2 * at(r1, x2) + at(r2, x0) + 2 * at(r2, x) + at(r2, x2);
      v = v < 0 ? -v : v;
      best = v > best ? v : best;
    }
    out[p] = (uint8_t)((best + 8) >> 4);
  }
}

int change_metric_u8(const void* a, const void* b, void* out, int B, int H, int W, int C, hipStream_t st) {
  if (grain_geometry("change_metric_u8", B, H, W, C)) return 1;
  if (out == a || out == b) return fail("change_metric_u8: out may alias neither a nor b");
  const int64_t want = ((int64_t)H * W + 255) / 256;
  const dim3 grid((unsigned)(want > 4096 ? 4096 : want), B);            // grid-stride beyond, as grain_u8
  const uint8_t *pa = (const uint8_t*)a, *pb = (const uint8_t*)b;
  switch (C) {
    case 1: change_metric_kernel<1><<<grid, 256, 0, st>>>(pa, pb, (uint8_t*)out, H, W); break;
    case 2: change_metric_kernel<2><<<grid, 256, 0, st>>>(pa, pb, (uint8_t*)out, H, W); break;
    case 3: change_metric_kernel<3><<<grid, 256, 0, st>>>(pa, pb, (uint8_t*)out, H, W); break;
    default: change_metric_kernel<4><<<grid, 256, 0, st>>>(pa, pb, (uint8_t*)out, H, W); break;
  }
  return check_launch("change_metric_u8");
}

// Hysteresis: a tile of 64 x 16 pixels per workgroup of 256 threads, every thread a run of four pixels of one row, so that a row of the
// tile is one 64-byte read.  The tile and its one-pixel halo take 18 rows of 68 bytes of LDS, 1224 bytes: the LDS never bounds the
// occupancy, and a byte per pixel lets neighbouring threads update their pixels without touching each other's.
constexpr int kHystTW = 64, kHystTH = 16, kHystPitch = 68;
enum : uint8_t { kHystOff = 0, kHystWeak = 1, kHystOn = 2 };          // below lo or outside the image; >= lo and not reached; reached

// One round.  kFirst: the state comes from m alone (on: m >= hi, weak: m >= lo) and every pixel of the tile is written, 255 or 0.  Later
// rounds: on where out == 255, weak where m >= lo; a halo pixel is on or off, since nothing spreads THROUGH another tile's pixel here;
// only the newly reached pixels are written.  Inside the tile the on state spreads over the eight neighbours until a sweep changes
// nothing.  Every store into out and into *changed writes a value that every other writer of that address writes in this launch (255;
// `round`), and a pixel only ever goes from 0 to 255, so a halo read that races with its owner's store sees either a state that was or
// one that will be true: the fixed point, where a round marks nothing, is the one set whatever the order.  A neighbour outside the image
// does not exist: no read leaves the buffers, whatever m holds.
template <bool kFirst>
__global__ __launch_bounds__(256) void hysteresis_kernel(const uint8_t* __restrict__ m, uint8_t* out, int lo, int hi, uint32_t* changed,
                                                         uint32_t round, int H, int W, int tiles_x) {
  __shared__ uint8_t st[(kHystTH + 2) * kHystPitch];
  const int64_t base = (int64_t)blockIdx.y * H * W;
  const int ty0 = (int)(blockIdx.x / (unsigned)tiles_x) * kHystTH, tx0 = (int)(blockIdx.x % (unsigned)tiles_x) * kHystTW;
  for (int k = threadIdx.x; k < (kHystTH + 2) * (kHystTW + 2); k += 256) {
    const int r = k / (kHystTW + 2), c = k - r * (kHystTW + 2);
    const int gy = ty0 - 1 + r, gx = tx0 - 1 + c;
    uint8_t v = kHystOff;
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
      const int64_t i = base + (int64_t)gy * W + gx;
      const bool inner = r >= 1 && r <= kHystTH && c >= 1 && c <= kHystTW;
      const int mv = m[i];
      if (kFirst) v = mv >= hi ? kHystOn : (inner && mv >= lo) ? kHystWeak : kHystOff;
      else v = out[i] == 255 ? kHystOn : (inner && mv >= lo) ? kHystWeak : kHystOff;
    }
    st[r * kHystPitch + c] = v;
  }
  __syncthreads();
  const int row = threadIdx.x / (kHystTW / 4), col = (threadIdx.x % (kHystTW / 4)) * 4;      // the thread's four pixels: (row, col .. col + 3)
  uint8_t* mine = &st[(row + 1) * kHystPitch + col + 1];
  uint8_t before[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) before[k] = mine[k];
  auto reached = [&](const uint8_t* p) {
    return p[-kHystPitch - 1] == kHystOn || p[-kHystPitch] == kHystOn || p[-kHystPitch + 1] == kHystOn || p[-1] == kHystOn || p[1] == kHystOn ||
           p[kHystPitch - 1] == kHystOn || p[kHystPitch] == kHystOn || p[kHystPitch + 1] == kHystOn;
  };
  for (;;) {                                         // ends: a sweep that changes something turns a weak pixel on, of which there are 1024
    int moved = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)                      // left to right, then right to left: a run is crossed in one sweep either way
      if (mine[k] == kHystWeak && reached(mine + k)) { mine[k] = kHystOn; moved = 1; }
#pragma unroll
    for (int k = 3; k >= 0; --k)
      if (mine[k] == kHystWeak && reached(mine + k)) { mine[k] = kHystOn; moved = 1; }
    if (!__syncthreads_or(moved)) break;             // the last sweep changed nothing, so every thread read the final state
  }
  const int gy = ty0 + row;
  bool marked = false;
  if (gy < H) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int gx = tx0 + col + k;
      if (gx >= W) break;
      const bool on = mine[k] == kHystOn;
      if (kFirst) out[base + (int64_t)gy * W + gx] = on ? 255 : 0;
      else if (on && before[k] != kHystOn) out[base + (int64_t)gy * W + gx] = 255;
      marked |= on && (kFirst || before[k] != kHystOn);
    }
  }
  if (marked) *changed = round;                      // an ordinary store: every writer of this launch stores the same value
}

int64_t hysteresis_workspace_bytes(int B, int H, int W) {
  if (B < 1 || H < 1 || W < 1 || B > 65535) { fail("hysteresis_workspace_bytes: B in 1..65535, H and W at least 1"); return -1; }
  const int64_t tiles = (int64_t)((W + kHystTW - 1) / kHystTW) * ((H + kHystTH - 1) / kHystTH);
  if (tiles > 0x7fffffffll) { fail("hysteresis_workspace_bytes: more than 2^31 - 1 tiles per sample"); return -1; }
  return 64;                                         // the word that a round raises
}

int hysteresis_u8(const void* m, void* out, int lo, int hi, void* workspace, int64_t workspace_bytes, int* rounds, int B, int H, int W,
                  hipStream_t st) {
  const int64_t need = hysteresis_workspace_bytes(B, H, W);
  if (need < 0) return 1;
  if (lo < 0 || lo > hi || hi > 256) return fail("hysteresis_u8: 0 <= lo <= hi <= 256 required, got %d, %d", lo, hi);
  if (workspace_bytes < need) return fail("hysteresis_u8: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)need);
  if ((uintptr_t)workspace & 3) return fail("hysteresis_u8: workspace must be 4-byte aligned");
  if (out == m || workspace == m || workspace == out) return fail("hysteresis_u8: m, out and workspace must be different buffers");
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cs) != hipSuccess) { (void)hipGetLastError(); cs = hipStreamCaptureStatusNone; }
  if (cs != hipStreamCaptureStatusNone)
    return fail("hysteresis_u8: the stream is capturing; the call reads a word back after every round and cannot be captured");
  const int tiles_x = (W + kHystTW - 1) / kHystTW;
  const dim3 grid((unsigned)((int64_t)tiles_x * ((H + kHystTH - 1) / kHystTH)), B);      // hysteresis_workspace_bytes bounded it
  const uint8_t* pm = (const uint8_t*)m;
  uint32_t* word = (uint32_t*)workspace;
  if (hipMemsetAsync(word, 0, 4, st) != hipSuccess) return fail("hysteresis_u8: clearing the workspace failed");
  hysteresis_kernel<true><<<grid, 256, 0, st>>>(pm, (uint8_t*)out, lo, hi, word, 1u, H, W, tiles_x);
  if (check_launch("hysteresis_u8")) return 1;
  int done = 1;
  if (grid.x > 1) {                                  // one tile per sample has no neighbour to hear from: its first round is its last
    for (;;) {
      uint32_t raised = 0;
      if (hipMemcpyAsync(&raised, word, 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return fail("hysteresis_u8: reading the round's word back failed");
      if (raised != (uint32_t)done) break;           // round `done` marked nothing
      ++done;
      hysteresis_kernel<false><<<grid, 256, 0, st>>>(pm, (uint8_t*)out, lo, hi, word, (uint32_t)done, H, W, tiles_x);
      if (check_launch("hysteresis_u8")) return 1;
    }
  }
  if (rounds) *rounds = done;
  return 0;
}

// The one launcher of the line warps: `name` is the declared function's, `arg` what its messages call the map's pointer.
template <typename Map>
static int warp_u8(const char* name, const char* arg, const void* in, void* out, void* coverage, int B, int H, int W, int C, int out_h,
                   int out_w, const Map map, const int16_t* taps, hipStream_t st) {
  if (B < 1 || H < 1 || W < 1 || out_h < 1 || out_w < 1) return fail("%s: B, H, W, out_h, out_w must be at least 1", name);
  if (C < 1 || C > 4) return fail("%s: 1..4 channels", name);
  if constexpr (std::is_same_v<Map, WarpGrid>)
    if (map.shift < 0 || map.shift > 5) return fail("%s: shift %d outside 0..5", name, map.shift);
  if (B > 65535) return fail("%s: batch %d exceeds 65535", name, B);
  if ((out_h + 7) / 8 > 65535) return fail("%s: out_h %d exceeds 524280", name, out_h);
  if ((int64_t)H * W * C > kMaxBytes || (int64_t)out_h * out_w * C > kMaxBytes) return fail("%s: more than 2^38 bytes per sample", name);
  if (in == out || in == coverage || out == coverage) return fail("%s: in, out and coverage must be different buffers", name);
  if (((uintptr_t)map.p | (uintptr_t)taps) & 7) return fail("%s: %s and taps must be 8-byte aligned", name, arg);
  const dim3 grid((out_w + 31) / 32, (out_h + 7) / 8, B);
  const uint8_t* pi = (const uint8_t*)in;
  uint8_t *po = (uint8_t*)out, *pc = (uint8_t*)coverage;
  switch (C) {
    case 1: warp_u8_kernel<1><<<grid, 256, 0, st>>>(pi, po, pc, H, W, out_h, out_w, map, taps); break;
    case 2: warp_u8_kernel<2><<<grid, 256, 0, st>>>(pi, po, pc, H, W, out_h, out_w, map, taps); break;
    case 3: warp_u8_kernel<3><<<grid, 256, 0, st>>>(pi, po, pc, H, W, out_h, out_w, map, taps); break;
    default: warp_u8_kernel<4><<<grid, 256, 0, st>>>(pi, po, pc, H, W, out_h, out_w, map, taps); break;
  }
  return check_launch(name);
}

int warp_affine_u8(const void* in, void* out, void* coverage, int B, int H, int W, int C, int out_h, int out_w, const int64_t* m,
                   const int16_t* taps, hipStream_t st) {
  return warp_u8("warp_affine_u8", "m", in, out, coverage, B, H, W, C, out_h, out_w, WarpAffine{m}, taps, st);
}

int warp_perspective_u8(const void* in, void* out, void* coverage, int B, int H, int W, int C, int out_h, int out_w, const int64_t* m,
                        const int16_t* taps, hipStream_t st) {
  return warp_u8("warp_perspective_u8", "m", in, out, coverage, B, H, W, C, out_h, out_w, WarpPerspective{m}, taps, st);
}

int warp_grid_u8(const void* in, void* out, void* coverage, int B, int H, int W, int C, int out_h, int out_w, const int64_t* grid,
                 int shift, const int16_t* taps, hipStream_t st) {
  return warp_u8("warp_grid_u8", "grid", in, out, coverage, B, H, W, C, out_h, out_w, WarpGrid{grid, shift}, taps, st);
}

// blocks_per_crop: how many workgroups share a crop's tiles (the kernel strides over them, so any value >= 1 gives the same bytes)
int warp_affine_gather_u8(const void* images, void* out, int64_t out_bytes, const int64_t* table, int n, int* refused, int B, int H, int W,
                          int C, int blocks_per_crop, const int16_t* taps, hipStream_t st) {
  const char* who = "warp_affine_gather_u8";
  if (n < 0) return fail("%s: negative crop count", who);
  if (B < 1 || H < 1 || W < 1) return fail("%s: B, H, W must be at least 1", who);
  if (C < 1 || C > 4) return fail("%s: 1..4 channels", who);
  if (out_bytes < 0) return fail("%s: negative out_bytes", who);
  if (n > 65535) return fail("%s: %d crops exceed 65535", who, n);
  if (blocks_per_crop < 1 || blocks_per_crop > 65535) return fail("%s: blocks_per_crop outside 1..65535", who);
  if ((int64_t)H * W * C > kMaxBytes) return fail("%s: more than 2^38 bytes per sample", who);
  if (((uintptr_t)table | (uintptr_t)taps) & 7) return fail("%s: table and taps must be 8-byte aligned", who);
  if ((uintptr_t)refused & 3) return fail("%s: refused must be 4-byte aligned", who);
  const char *pi = (const char*)images, *po = (const char*)out, *pt = (const char*)table, *pr = (const char*)refused;
  const int64_t in_bytes = (int64_t)B * H * W * C, table_bytes = (int64_t)n * 80;
  const auto overlap = [](const char* a, int64_t na, const char* b, int64_t nb) { return a < b + nb && b < a + na; };
  if (overlap(po, out_bytes, pi, in_bytes) || overlap(po, out_bytes, pt, table_bytes) || overlap(po, out_bytes, pr, 4) ||
      overlap(pr, 4, pi, in_bytes) || overlap(pr, 4, pt, table_bytes))
    return fail("%s: images, out, table and refused must not overlap", who);
  if (n == 0) return 0;
  const dim3 grid((unsigned)blocks_per_crop, (unsigned)n);
  const uint8_t* src = (const uint8_t*)images;
  uint8_t* dst = (uint8_t*)out;
  switch (C) {
    case 1: warp_gather_u8_kernel<1><<<grid, 256, 0, st>>>(src, dst, out_bytes, table, refused, B, H, W, taps); break;
    case 2: warp_gather_u8_kernel<2><<<grid, 256, 0, st>>>(src, dst, out_bytes, table, refused, B, H, W, taps); break;
    case 3: warp_gather_u8_kernel<3><<<grid, 256, 0, st>>>(src, dst, out_bytes, table, refused, B, H, W, taps); break;
    default: warp_gather_u8_kernel<4><<<grid, 256, 0, st>>>(src, dst, out_bytes, table, refused, B, H, W, taps); break;
  }
  return check_launch(who);
}

int pack_mask(const void* mask, int mask_dtype, void* out, int B, int H, int W, int mask_b, int binarize, int64_t ld, int col0,
              hipStream_t st) {
  if (H % 16 || W % 16) return fail("pack_mask: H and W must be multiples of 16");
  if (ld % 8 || col0 % 8) return fail("pack_mask: ld / col0 must be multiples of 8");
  if (mask_b != 1 && mask_b != B) return fail("pack_mask: mask batch must be 1 or B");
  const int64_t n = (int64_t)B * (H / 16) * (W / 16) * 32;
  if (n <= 0) return 0;
  if (mask_dtype == 0) pack_mask_kernel<float><<<blocks_for(n), 256, 0, st>>>((const float*)mask, (bf16_t*)out, B, H, W, mask_b, binarize, ld, col0);
  else if (mask_dtype == 2) pack_mask_kernel<uint8_t><<<blocks_for(n), 256, 0, st>>>((const uint8_t*)mask, (bf16_t*)out, B, H, W, mask_b, binarize, ld, col0);
  else return fail("pack_mask: mask dtype must be 0 (f32) or 2 (u8)");
  return check_launch("pack_mask");
}

// The argument checks the two latent packers share; C: the packed mask's channel count, nullptr where the output has none
static int latent_pack_check(const char* who, int B, int H, int W, const int* C, int mode, int grow) {
  if (B < 0 || H < 0 || W < 0 || H % 16 || W % 16) return fail("%s: B >= 0; H and W non-negative multiples of 16", who);
  if (C && (*C <= 0 || *C % 8)) return fail("%s: C must be a positive multiple of 8", who);
  if (mode != 0 && mode != 1) return fail("%s: mode must be 0 (nearest) or 1 (cover)", who);
  if (mode == 0 && grow != 0) return fail("%s: grow must be 0 in mode 0 (nearest)", who);
  if (grow < 0 || grow > 8) return fail("%s: grow %d outside 0..8", who, grow);
  return 0;
}

int keep_mask_pack(const void* mask_u8, void* out, int B, int H, int W, int C, int mode, int grow, hipStream_t st) {
  if (int e = latent_pack_check("keep_mask_pack", B, H, W, &C, mode, grow)) return e;
  const int64_t n = (int64_t)B * (H / 16) * (W / 16);
  if (n == 0) return 0;
  if (!mask_u8 || !out) return fail("keep_mask_pack: null pointer");
  if (((uintptr_t)mask_u8 & 7) || ((uintptr_t)out & 15)) return fail("keep_mask_pack: mask must be 8-byte and out 16-byte aligned");
  latent_pack_kernel<<<blocks_for(n), 256, 0, st>>>((const uint8_t*)mask_u8, AnyTopBit{(bf16_t*)out, C}, B, H, W, mode, grow);
  return check_launch("keep_mask_pack");
}

int change_map_pack(const void* map_u8, void* hold, int B, int H, int W, int mode, int grow, hipStream_t st) {
  if (int e = latent_pack_check("change_map_pack", B, H, W, nullptr, mode, grow)) return e;
  const int64_t n = (int64_t)B * (H / 16) * (W / 16);
  if (n == 0) return 0;
  if (!map_u8 || !hold) return fail("change_map_pack: null pointer");
  if (((uintptr_t)map_u8 & 7) || ((uintptr_t)hold & 3)) return fail("change_map_pack: map must be 8-byte and hold 4-byte aligned");
  latent_pack_kernel<<<blocks_for(n), 256, 0, st>>>((const uint8_t*)map_u8, ByteMax{(uint32_t*)hold}, B, H, W, mode, grow);
  return check_launch("change_map_pack");
}

int sample_pack(const void* moments, const void* eps, int eps_dtype, void* out, int B, int h, int w, int L, float shift,
                float scale, int64_t ld, int col0, hipStream_t st) {
  if (h % 2 || w % 2 || L % 2 || ld % 8 || col0 % 8) return fail("sample_pack: h, w, L even; ld / col0 multiples of 8");
  const int64_t n = (int64_t)B * (h / 2) * (w / 2) * (L / 2);
  if (n <= 0) return 0;
  if (!eps || eps_dtype == 1)
    sample_pack_kernel<bf16_t><<<blocks_for(n), 256, 0, st>>>((const bf16_t*)moments, (const bf16_t*)eps, (bf16_t*)out, B, h, w, L, shift, scale, ld, col0);
  else if (eps_dtype == 0)
    sample_pack_kernel<float><<<blocks_for(n), 256, 0, st>>>((const bf16_t*)moments, (const float*)eps, (bf16_t*)out, B, h, w, L, shift, scale, ld, col0);
  else return fail("sample_pack: eps dtype must be 0 (f32) or 1 (bf16)");
  return check_launch("sample_pack");
}

int unpack_latents(const void* lat, int64_t ld, void* out, int B, int h, int w, int L, float shift, float scale, hipStream_t st) {
  if (h % 2 || w % 2 || L % 8) return fail("unpack_latents: h, w even; L a multiple of 8");
  const int64_t n = (int64_t)B * h * w * (L / 8);
  if (n <= 0) return 0;
  unpack_latents_kernel<<<blocks_for(n), 256, 0, st>>>((const bf16_t*)lat, ld, (bf16_t*)out, B, h, w, L, shift, scale);
  return check_launch("unpack_latents");
}

int postprocess(const void* x, void* out, int B, int H, int W, int Cs, int C, int mode, int denorm, int y0, int x0, int Hc, int Wc,
                hipStream_t st) {
  if (mode < 0 || mode > 3 || C > Cs) return fail("postprocess: mode 0..3, C <= Cs");
  if (y0 < 0 || x0 < 0 || Hc <= 0 || Wc <= 0 || y0 + Hc > H || x0 + Wc > W) return fail("postprocess: crop window outside the image");
  const int64_t n = (int64_t)B * Hc * Wc;
  if (n <= 0) return 0;
  postprocess_kernel<<<blocks_for(n), 256, 0, st>>>((const bf16_t*)x, out, B, H, W, Cs, C, mode, denorm, y0, x0, Hc, Wc);
  return check_launch("postprocess");
}

int transpose_bf16(const void* in, int64_t ldi, int64_t ibs, void* out, int64_t ldo, int64_t obs, int N, int C, int batch,
                   hipStream_t st) {
  if (N <= 0 || C <= 0 || batch <= 0) return 0;
  transpose_kernel<<<dim3((N + 63) / 64, (C + 63) / 64, batch), 256, 0, st>>>((const bf16_t*)in, ldi, ibs, (bf16_t*)out, ldo, obs, N, C);
  return check_launch("transpose");
}

int row_softmax(const float* s, int64_t lds, void* p, int64_t ldp, int rows, int N, float scale, hipStream_t st) {
  if (rows <= 0 || N <= 0) return 0;
  row_softmax_kernel<<<rows, 256, 0, st>>>(s, lds, (bf16_t*)p, ldp, N, scale * 1.4426950408889634f);
  return check_launch("row_softmax");
}

}  // namespace tfx
