// Read-back: the kernels of the on-device text recogniser (MobileNetV1Enhance backbone, two-block SVTR neck, CTC head) and of the
// CTC decode / loss behind it, with their extern "C" entry points (include/textflux_hip.h, "read-back").  Activations are fp32 NHWC,
// channels contiguous.  No floating-point atomics; every reduction runs in a fixed order, so two runs give the same bits.
#include "../../include/textflux_hip.h"

#include <math.h>

#include "common.h"
#include "launch.h"

namespace tfx {
namespace {

enum OcrAct : int { ACT_NONE = 0, ACT_RELU = 1, ACT_HSWISH = 2, ACT_HSIGMOID = 3, ACT_SWISH = 4 };

// relu6(x + 3): one rounded add, two exact clamps
__device__ __forceinline__ float relu6p3(float x) { return fminf(fmaxf(x + 3.0f, 0.0f), 6.0f); }
// hard-swish is (x * relu6(x + 3)) / 6 and hard-sigmoid relu6(x + 3) / 6, both with a true (IEEE) division; swish is x * (1 / (1 + exp(-x)))
__device__ __forceinline__ float ocr_act(float v, int act) {
  switch (act) {
    case ACT_RELU: return fmaxf(v, 0.0f);
    case ACT_HSWISH: return (v * relu6p3(v)) / 6.0f;
    case ACT_HSIGMOID: return relu6p3(v) / 6.0f;
    case ACT_SWISH: return v * (1.0f / (1.0f + expf(-v)));
    default: return v;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// resize + normalise: crop i is u8 [h, w, 3] at src + table[i][0], table[i] = {byte offset, h, w, turn}
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ocr_resize_norm_kernel(const uint8_t* __restrict__ src, int64_t src_bytes,
                                                              const int32_t* __restrict__ table, float* __restrict__ out, int n, int imgH,
                                                              int imgW) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)n * imgH * imgW) return;
  const int x = (int)(idx % imgW), y = (int)((idx / imgW) % imgH), i = (int)(idx / ((int64_t)imgW * imgH));
  const int off = table[4 * i], h = table[4 * i + 1], w = table[4 * i + 2], turn = table[4 * i + 3];
  float* o = out + idx * 3;
  // an entry that does not lie inside the packed buffer reads nothing
  if (h < 1 || w < 1 || off < 0 || (int64_t)off + (int64_t)h * w * 3 > src_bytes) { o[0] = o[1] = o[2] = 0.0f; return; }
  const int th = turn ? w : h, tw = turn ? h : w;                 // the size after the quarter turn
  const double ratio = (double)tw / (double)th;
  int rw = (int)ceil((double)imgH * ratio);
  if (rw > imgW) rw = imgW;
  if (x >= rw) { o[0] = o[1] = o[2] = 0.0f; return; }            // the padding comes after the normalisation
  const float sy = imgH > 1 ? (float)(th - 1) / (float)(imgH - 1) : 0.0f, sx = rw > 1 ? (float)(tw - 1) / (float)(rw - 1) : 0.0f;
  const float fy = sy * (float)y, fx = sx * (float)x;
  const int y0 = (int)fy, x0 = (int)fx;
  const int y1 = y0 + (y0 < th - 1 ? 1 : 0), x1 = x0 + (x0 < tw - 1 ? 1 : 0);
  const float ly1 = fy - (float)y0, ly0 = 1.0f - ly1, lx1 = fx - (float)x0, lx0 = 1.0f - lx1;
  // turned pixel (r, c) is source pixel (c, w - 1 - r): transpose(1, 2).flip(dims=[1]) of a CHW image
  const uint8_t* base = src + off;
  auto at = [&](int r, int c) -> const uint8_t* { return turn ? base + ((int64_t)c * w + (w - 1 - r)) * 3 : base + ((int64_t)r * w + c) * 3; };
  const uint8_t *p00 = at(y0, x0), *p01 = at(y0, x1), *p10 = at(y1, x0), *p11 = at(y1, x1);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float v = ly0 * (lx0 * (float)p00[c] + lx1 * (float)p01[c]) + ly1 * (lx0 * (float)p10[c] + lx1 * (float)p11[c]);
    o[c] = (v / 255.0f - 0.5f) / 0.5f;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// dense convolution / linear as an implicit GEMM on v_mfma_f32_16x16x4_f32: out[m, co_off + n] = act(sum_k A[m, k] W[n, k] + bias[n]),
// m = (b, oy, ox), k = (ky, kx, ci).  One workgroup = a 16 x 32 output tile; its four waves take the 16-wide k chunks
// w, w + 4, ... and their partial sums are added in wave order.  Within a chunk lane l holds k = 4 (l >> 4) + j for MFMA j.
// ---------------------------------------------------------------------------------------------------------------------------------
struct OcrConv {
  const float* x; const float* w; const float* bias; float* out;
  int B, H, W, Cin, Ho, Wo, N, kh, kw, sh, sw, act, co_off, M, K;
  int64_t ldx, ldo;
};

template <bool VEC>
__global__ __launch_bounds__(256) void ocr_conv_f32_kernel(const OcrConv a) {
  __shared__ float red[3][2][4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, kq = lane >> 4;
  const int m0 = blockIdx.y * 16, n0 = blockIdx.x * 32;
  const int m = m0 + r;
  const bool mv = m < a.M;
  int iy0 = 0, ix0 = 0;
  const float* xb = a.x;
  if (mv) {
    const int ox = m % a.Wo, oy = (m / a.Wo) % a.Ho, b = m / (a.Wo * a.Ho);
    iy0 = oy * a.sh - a.kh / 2;
    ix0 = ox * a.sw - a.kw / 2;
    xb = a.x + (int64_t)b * a.H * a.W * a.ldx;
  }
  const int na = n0 + r, nb = n0 + 16 + r;
  const bool nav = na < a.N, nbv = nb < a.N;
  const float* wa = a.w + (int64_t)(nav ? na : 0) * a.K;
  const float* wb = a.w + (int64_t)(nbv ? nb : 0) * a.K;
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  for (int kc = wave * 16; kc < a.K; kc += 64) {
    const int k = kc + 4 * kq;
    float av[4] = {0.f, 0.f, 0.f, 0.f}, b0[4] = {0.f, 0.f, 0.f, 0.f}, b1[4] = {0.f, 0.f, 0.f, 0.f};
    if (VEC) {                                       // Cin % 4 == 0: four consecutive k share a tap and lie inside K together
      if (k < a.K) {
        if (mv) {
          const int tap = k / a.Cin, ci = k - tap * a.Cin, ky = tap / a.kw, kx = tap - ky * a.kw;
          const int iy = iy0 + ky, ix = ix0 + kx;
          if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) {
            const f32x4 v = *(const f32x4*)(xb + ((int64_t)iy * a.W + ix) * a.ldx + ci);
            av[0] = v[0]; av[1] = v[1]; av[2] = v[2]; av[3] = v[3];
          }
        }
        if (nav) { const f32x4 v = *(const f32x4*)(wa + k); b0[0] = v[0]; b0[1] = v[1]; b0[2] = v[2]; b0[3] = v[3]; }
        if (nbv) { const f32x4 v = *(const f32x4*)(wb + k); b1[0] = v[0]; b1[1] = v[1]; b1[2] = v[2]; b1[3] = v[3]; }
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int kk = k + j;
        if (kk < a.K) {
          if (mv) {
            const int tap = kk / a.Cin, ci = kk - tap * a.Cin, ky = tap / a.kw, kx = tap - ky * a.kw;
            const int iy = iy0 + ky, ix = ix0 + kx;
            if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) av[j] = xb[((int64_t)iy * a.W + ix) * a.ldx + ci];
          }
          if (nav) b0[j] = wa[kk];
          if (nbv) b1[j] = wb[kk];
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], b0[j], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], b1[j], acc1, 0, 0, 0);
    }
  }
  if (wave > 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) { red[wave - 1][0][i][lane] = acc0[i]; red[wave - 1][1][i][lane] = acc1[i]; }
  }
  __syncthreads();
  if (wave > 0) return;
  // C/D map of the 16 x 16 MFMA: column = lane & 15, row = 4 (lane >> 4) + register
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = m0 + 4 * kq + i;
    if (row >= a.M) continue;
    float s0 = acc0[i], s1 = acc1[i];
#pragma unroll
    for (int w = 0; w < 3; ++w) { s0 += red[w][0][i][lane]; s1 += red[w][1][i][lane]; }
    float* o = a.out + (int64_t)row * a.ldo + a.co_off;
    if (nav) o[na] = ocr_act(s0 + (a.bias ? a.bias[na] : 0.0f), a.act);
    if (nbv) o[nb] = ocr_act(s1 + (a.bias ? a.bias[nb] : 0.0f), a.act);
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// depthwise convolution: one thread = one output pixel x four channels; the taps are an fmaf chain in (ky, kx) order
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ocr_conv_dw_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                          float* __restrict__ out, int B, int H, int W, int C, int Ho, int Wo, int ks, int sh,
                                                          int sw, int act) {
  const int C4 = C >> 2;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)B * Ho * Wo * C4) return;
  const int c = (int)(idx % C4) * 4;
  const int64_t pix = idx / C4;
  const int ox = (int)(pix % Wo), oy = (int)((pix / Wo) % Ho), b = (int)(pix / ((int64_t)Wo * Ho));
  const int pad = ks / 2;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int ky = 0; ky < ks; ++ky) {
    const int iy = oy * sh - pad + ky;
    if (iy < 0 || iy >= H) continue;
    for (int kx = 0; kx < ks; ++kx) {
      const int ix = ox * sw - pad + kx;
      if (ix < 0 || ix >= W) continue;
      const f32x4 v = *(const f32x4*)(x + (((int64_t)b * H + iy) * W + ix) * C + c);
      const f32x4 k = *(const f32x4*)(w + (int64_t)(ky * ks + kx) * C + c);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = __builtin_fmaf(v[j], k[j], acc[j]);
    }
  }
  f32x4 o;
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = ocr_act(acc[j] + (bias ? bias[c + j] : 0.0f), act);
  *(f32x4*)(out + pix * C + c) = o;
}

// mode 0: out[b, c] = (sum over (h, w) in row-major order) / (H W), one IEEE division; mode 1: 2 x 2 stride-2 average,
// ((x00 + x01) + (x10 + x11)) * 0.25, out [B, H/2, W/2, C] with pixel pitch ldo
__global__ __launch_bounds__(256) void ocr_pool_kernel(const float* __restrict__ x, float* __restrict__ out, int B, int H, int W, int C, int mode,
                                                       int64_t ldo) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (mode == 0) {
    if (idx >= (int64_t)B * C) return;
    const int c = (int)(idx % C), b = (int)(idx / C);
    const float* p = x + (int64_t)b * H * W * C + c;
    float s = 0.0f;
    for (int i = 0; i < H * W; ++i) s += p[(int64_t)i * C];
    out[idx] = s / (float)(H * W);
  } else {
    const int Ho = H / 2, Wo = W / 2;
    if (idx >= (int64_t)B * Ho * Wo * C) return;
    const int c = (int)(idx % C);
    const int64_t pix = idx / C;
    const int ox = (int)(pix % Wo), oy = (int)((pix / Wo) % Ho), b = (int)(pix / ((int64_t)Wo * Ho));
    const float* p = x + (((int64_t)b * H + 2 * oy) * W + 2 * ox) * C + c;
    out[pix * ldo + c] = ((p[0] + p[C]) + (p[(int64_t)W * C] + p[(int64_t)W * C + C])) * 0.25f;
  }
}

__global__ __launch_bounds__(256) void ocr_scale_channels_kernel(const float* __restrict__ x, const float* __restrict__ s, float* __restrict__ out,
                                                                 int64_t per_sample4, int C4, int64_t total4) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total4) return;
  const int b = (int)(idx / per_sample4), c4 = (int)(idx % C4);
  const f32x4 v = ((const f32x4*)x)[idx], k = ((const f32x4*)s)[(int64_t)b * C4 + c4];
  ((f32x4*)out)[idx] = v * k;
}

// nn.LayerNorm on fp32 rows, one wave per row: mean = sum / D, var = sum (x - mean)^2 / D, y = (x - mean) * (1 / sqrt(var + eps)) * g + b
__global__ __launch_bounds__(256) void ocr_layernorm_kernel(const float* __restrict__ x, int64_t ldx, float* __restrict__ out, int64_t ldo,
                                                            const float* __restrict__ g, const float* __restrict__ bt, int64_t rows, int D,
                                                            float eps) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* p = x + row * ldx;
  float v[8];
  float s = 0.0f;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int c = lane + 64 * i;
    v[i] = c < D ? p[c] : 0.0f;
    s += v[i];
  }
  const float mean = wave_sum(s) / (float)D;
  float q = 0.0f;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int c = lane + 64 * i;
    const float d = v[i] - mean;
    v[i] = d;
    q += c < D ? d * d : 0.0f;
  }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)D + eps);
  float* o = out + row * ldo;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int c = lane + 64 * i;
    if (c < D) o[c] = v[i] * rstd * g[c] + bt[c];
  }
}

// attention of one (b, head) per workgroup: K [N][dp] (dp odd), V [N][d] and one row of weights per wave in LDS.  Wave w takes query
// rows w, w + 4, ...: lane j scores keys j, j + 64, ... as an fmaf chain over d of (q * scale) * k; softmax = exp(s - max) / sum in fp32;
// the output column d sums p[j] v[j][d] over j in two halves (lanes < 32: the first ceil(N / 2) keys), first half + second half.
__global__ __launch_bounds__(256) void ocr_attention_kernel(const float* __restrict__ qkv, float* __restrict__ out, int Hh, int N, int d, float scale) {
  extern __shared__ float lds[];
  const int dp = d | 1;
  float* Ks = lds;
  float* Vs = Ks + (int64_t)N * dp;
  float* Ps = Vs + (int64_t)N * d;          // [4][N]
  float* Qs = Ps + 4 * N;                   // [4][32]
  const int b = blockIdx.x / Hh, h = blockIdx.x % Hh;
  const int64_t ld = 3 * (int64_t)Hh * d;
  const float* base = qkv + (int64_t)b * N * ld + (int64_t)h * d;
  for (int i = threadIdx.x; i < N * d; i += 256) {
    const int j = i / d, e = i - j * d;
    Ks[j * dp + e] = base[(int64_t)j * ld + (int64_t)Hh * d + e];
    Vs[j * d + e] = base[(int64_t)j * ld + 2 * (int64_t)Hh * d + e];
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* P = Ps + wave * N;
  float* Q = Qs + wave * 32;
  const int half = (N + 1) / 2;
  for (int i0 = 0; i0 < N; i0 += 4) {             // the same trip count in every wave: the barriers below are workgroup barriers
    const int i = i0 + wave;
    const bool on = i < N;
    if (on && lane < d) Q[lane] = base[(int64_t)i * ld + lane] * scale;
    __syncthreads();
    float s[4], mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int j = lane + 64 * t;
      s[t] = -INFINITY;
      if (on && j < N) {
        float acc = 0.0f;
        for (int e = 0; e < d; ++e) acc = __builtin_fmaf(Q[e], Ks[j * dp + e], acc);
        s[t] = acc;
      }
      mx = fmaxf(mx, s[t]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    float sum = 0.0f;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int j = lane + 64 * t;
      s[t] = (on && j < N) ? expf(s[t] - mx) : 0.0f;
      sum += s[t];
    }
    sum = wave_sum(sum);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int j = lane + 64 * t;
      if (on && j < N) P[j] = s[t] / sum;
    }
    __syncthreads();
    const int e = lane & 31, j0 = lane < 32 ? 0 : half, j1 = lane < 32 ? half : N;
    float acc = 0.0f;
    if (on && e < d)
      for (int j = j0; j < j1; ++j) acc = __builtin_fmaf(P[j], Vs[j * d + e], acc);
    const float other = __shfl_xor(acc, 32, 64);
    if (on && lane < d) out[((int64_t)b * N + i) * ((int64_t)Hh * d) + (int64_t)h * d + lane] = acc + other;
  }
}

// per row of C logits: the maximum, its first index (numpy's argmax tie rule) and max + log(sum exp(x - max)).  Thread t scans the
// classes t, t + 256, ... in rising order; the 256 partial results are folded by a fixed tree.
__global__ __launch_bounds__(256) void ctc_rows_kernel(const float* __restrict__ x, int64_t ld, int C, float* __restrict__ omax, int32_t* __restrict__ oarg,
                                                       float* __restrict__ olse) {
  __shared__ float sv[256];
  __shared__ int si[256];
  const float* p = x + (int64_t)blockIdx.x * ld;
  const int t = threadIdx.x;
  float best = -INFINITY;
  int bi = 0x7fffffff;
  for (int c = t; c < C; c += 256) {
    const float v = p[c];
    if (v > best || bi == 0x7fffffff) { best = v; bi = c; }
  }
  sv[t] = best; si[t] = bi;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) {
      const float v2 = sv[t + o]; const int i2 = si[t + o];
      if (i2 != 0x7fffffff && (si[t] == 0x7fffffff || v2 > sv[t] || (v2 == sv[t] && i2 < si[t]))) { sv[t] = v2; si[t] = i2; }
    }
    __syncthreads();
  }
  const float mx = sv[0];
  const int arg = si[0];
  __syncthreads();
  float s = 0.0f;
  for (int c = t; c < C; c += 256) s += expf(p[c] - mx);
  sv[t] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) sv[t] += sv[t + o];
    __syncthreads();
  }
  if (t == 0) {
    omax[blockIdx.x] = mx;
    oarg[blockIdx.x] = arg;
    olse[blockIdx.x] = mx + logf(sv[0]);
  }
}

__device__ __forceinline__ float lse3(float a, float b, float c) {
  const float m = fmaxf(a, fmaxf(b, c));
  if (m == -INFINITY) return -INFINITY;
  return m + logf(expf(a - m) + expf(b - m) + expf(c - m));
}

// one workgroup per sample: thread 0 walks the T arg-max ids (collapse repeats, drop blank 0); threads 0 .. 2L run the CTC forward
// recursion in log space over the states blank, l1, blank, l2, ..., blank
__global__ __launch_bounds__(256) void ctc_score_kernel(const float* __restrict__ logits, const int32_t* __restrict__ arg, const float* __restrict__ lse,
                                                        const int32_t* __restrict__ targets, const int32_t* __restrict__ offsets, int T, int C,
                                                        int32_t* __restrict__ ids, int32_t* __restrict__ tix, int32_t* __restrict__ count,
                                                        float* __restrict__ loss) {
  __shared__ float alpha[2][256];
  const int n = blockIdx.x, s = threadIdx.x;
  if (s == 0) {
    int cnt = 0, prev = -1;
    for (int t = 0; t < T; ++t) {
      const int a = arg[(int64_t)n * T + t];
      if (a != 0 && a != prev) { ids[(int64_t)n * T + cnt] = a; tix[(int64_t)n * T + cnt] = t; ++cnt; }
      prev = a;
    }
    count[n] = cnt;
    for (int t = cnt; t < T; ++t) { ids[(int64_t)n * T + t] = 0; tix[(int64_t)n * T + t] = -1; }
  }
  if (!loss) return;
  const int t0 = offsets[n], L = offsets[n + 1] - t0, S = 2 * L + 1;
  if (L < 0 || L > 127) {                            // more states than the workgroup has threads: refused on the host, NaN here
    if (s == 0) loss[n] = NAN;
    return;
  }
  const bool live = s < S;
  int cls = 0;
  bool skip = false;
  if (live && (s & 1)) {
    cls = targets[t0 + (s >> 1)];
    cls = cls < 0 ? 0 : (cls >= C ? C - 1 : cls);
    skip = s >= 3 && targets[t0 + (s >> 1) - 1] != targets[t0 + (s >> 1)];
  }
  const float* lg = logits + (int64_t)n * T * C;
  const float* ls = lse + (int64_t)n * T;
  alpha[0][s] = (live && s < 2) ? lg[cls] - ls[0] : -INFINITY;
  __syncthreads();
  int cur = 0;
  for (int t = 1; t < T; ++t) {
    float v = -INFINITY;
    if (live) {
      const float a0 = alpha[cur][s], a1 = s >= 1 ? alpha[cur][s - 1] : -INFINITY, a2 = skip ? alpha[cur][s - 2] : -INFINITY;
      const float l = lse3(a0, a1, a2);
      v = l == -INFINITY ? -INFINITY : l + (lg[(int64_t)t * C + cls] - ls[t]);
    }
    alpha[cur ^ 1][s] = v;
    __syncthreads();
    cur ^= 1;
  }
  if (s == 0) {
    const float a = alpha[cur][S - 1], b = S >= 2 ? alpha[cur][S - 2] : -INFINITY;
    const float m = fmaxf(a, b);
    loss[n] = m == -INFINITY ? INFINITY : -(m + logf(expf(a - m) + expf(b - m)));
  }
}

inline hipStream_t S(tfx_stream s) { return (hipStream_t)s; }
inline unsigned blocks256(int64_t n) { return (unsigned)((n + 255) / 256); }
constexpr int64_t MAX_ELEMS = (int64_t)1 << 31;     // a 1-D grid of 256-thread workgroups over more would not fit the x dimension

}  // namespace
}  // namespace tfx

using namespace tfx;

extern "C" {

int tfx_ocr_resize_norm(const void* src, int64_t src_bytes, const int32_t* table, float* out, int32_t n, int32_t img_h, int32_t img_w,
                        tfx_stream stream) {
  if (!src || !table || !out) return fail("tfx_ocr_resize_norm: null pointer");
  if (n < 0 || img_h < 1 || img_w < 1 || src_bytes < 0) return fail("tfx_ocr_resize_norm: n >= 0, img_h, img_w >= 1 and src_bytes >= 0 are required");
  if (src_bytes >= MAX_ELEMS) return fail("tfx_ocr_resize_norm: the packed crops must stay below 2 GiB (int32 offsets)");
  const int64_t total = (int64_t)n * img_h * img_w;
  if (total >= MAX_ELEMS) return fail("tfx_ocr_resize_norm: n * img_h * img_w must stay below 2^31");
  if (total == 0) return 0;
  ocr_resize_norm_kernel<<<blocks256(total), 256, 0, S(stream)>>>((const uint8_t*)src, src_bytes, table, out, n, img_h, img_w);
  return check_launch("ocr_resize_norm");
}

int tfx_ocr_conv_f32(const float* x, const float* w, const float* bias, float* out, int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout,
                     int32_t ksize, int32_t stride_h, int32_t stride_w, int32_t act, int64_t ldx, int64_t ldo, int32_t co_off, tfx_stream stream) {
  if (!x || !w || !out) return fail("tfx_ocr_conv_f32: null pointer");
  if (ksize != 1 && ksize != 3) return fail("tfx_ocr_conv_f32: the filter is 1 x 1 or 3 x 3");
  if (B < 0 || H < 1 || W < 1 || Cin < 1 || Cout < 1 || stride_h < 1 || stride_w < 1) return fail("tfx_ocr_conv_f32: bad geometry");
  if (act < ACT_NONE || act > ACT_SWISH) return fail("tfx_ocr_conv_f32: act is 0 none, 1 relu, 2 hard-swish, 3 hard-sigmoid or 4 swish");
  if (ldx < Cin || co_off < 0 || ldo < (int64_t)co_off + Cout) return fail("tfx_ocr_conv_f32: ldx >= Cin and ldo >= co_off + Cout are required");
  OcrConv a;
  a.x = x; a.w = w; a.bias = bias; a.out = out;
  a.B = B; a.H = H; a.W = W; a.Cin = Cin; a.N = Cout; a.kh = a.kw = ksize; a.sh = stride_h; a.sw = stride_w; a.act = act; a.co_off = co_off;
  a.Ho = (H + 2 * (ksize / 2) - ksize) / stride_h + 1;
  a.Wo = (W + 2 * (ksize / 2) - ksize) / stride_w + 1;
  const int64_t M = (int64_t)B * a.Ho * a.Wo, K = (int64_t)ksize * ksize * Cin;
  if (M > 16 * 65535 || K >= (1 << 24) || (int64_t)B * H * W * ldx >= ((int64_t)1 << 40))
    return fail("tfx_ocr_conv_f32: at most 1048560 output pixels (gridDim.y) and K < 2^24");
  if (M == 0) return 0;
  a.M = (int)M; a.K = (int)K; a.ldx = ldx; a.ldo = ldo;
  const dim3 grid((Cout + 31) / 32, (unsigned)((M + 15) / 16));
  const bool vec = Cin % 4 == 0 && ldx % 4 == 0 && ((uintptr_t)x | (uintptr_t)w) % 16 == 0;
  if (vec) ocr_conv_f32_kernel<true><<<grid, 256, 0, S(stream)>>>(a);
  else ocr_conv_f32_kernel<false><<<grid, 256, 0, S(stream)>>>(a);
  return check_launch("ocr_conv_f32");
}

int tfx_ocr_conv_dw(const float* x, const float* w, const float* bias, float* out, int32_t B, int32_t H, int32_t W, int32_t C, int32_t ksize,
                    int32_t stride_h, int32_t stride_w, int32_t act, tfx_stream stream) {
  if (!x || !w || !out) return fail("tfx_ocr_conv_dw: null pointer");
  if (ksize != 3 && ksize != 5) return fail("tfx_ocr_conv_dw: the filter is 3 x 3 or 5 x 5");
  if (B < 0 || H < 1 || W < 1 || C < 4 || C % 4) return fail("tfx_ocr_conv_dw: C must be a positive multiple of 4");
  if ((stride_h != 1 && stride_h != 2) || (stride_w != 1 && stride_w != 2)) return fail("tfx_ocr_conv_dw: strides are 1 or 2");
  if (act != ACT_NONE && act != ACT_HSWISH) return fail("tfx_ocr_conv_dw: act is 0 none or 2 hard-swish");
  if (((uintptr_t)x | (uintptr_t)w | (uintptr_t)out) % 16) return fail("tfx_ocr_conv_dw: x, w and out must be 16-byte aligned");
  const int Ho = (H + 2 * (ksize / 2) - ksize) / stride_h + 1, Wo = (W + 2 * (ksize / 2) - ksize) / stride_w + 1;
  const int64_t total = (int64_t)B * Ho * Wo * (C / 4);
  if (total >= MAX_ELEMS || (int64_t)B * H * W * C >= ((int64_t)1 << 40)) return fail("tfx_ocr_conv_dw: too many elements");
  if (total == 0) return 0;
  ocr_conv_dw_kernel<<<blocks256(total), 256, 0, S(stream)>>>(x, w, bias, out, B, H, W, C, Ho, Wo, ksize, stride_h, stride_w, act);
  return check_launch("ocr_conv_dw");
}

int tfx_ocr_pool(const float* x, float* out, int32_t B, int32_t H, int32_t W, int32_t C, int32_t mode, int64_t ldo, tfx_stream stream) {
  if (!x || !out) return fail("tfx_ocr_pool: null pointer");
  if (B < 0 || H < 1 || W < 1 || C < 1) return fail("tfx_ocr_pool: bad geometry");
  if (mode != 0 && mode != 1) return fail("tfx_ocr_pool: mode is 0 (global mean) or 1 (2 x 2 stride-2 average)");
  if (mode == 1 && (H < 2 || W < 2 || ldo < C)) return fail("tfx_ocr_pool: the 2 x 2 pool needs H, W >= 2 and ldo >= C");
  if ((int64_t)H * W >= (1 << 24)) return fail("tfx_ocr_pool: H * W must stay below 2^24");
  const int64_t total = mode == 0 ? (int64_t)B * C : (int64_t)B * (H / 2) * (W / 2) * C;
  if (total >= MAX_ELEMS) return fail("tfx_ocr_pool: too many elements");
  if (total == 0) return 0;
  ocr_pool_kernel<<<blocks256(total), 256, 0, S(stream)>>>(x, out, B, H, W, C, mode, ldo);
  return check_launch("ocr_pool");
}

int tfx_ocr_scale_channels(const float* x, const float* s, float* out, int32_t B, int64_t HW, int32_t C, tfx_stream stream) {
  if (!x || !s || !out) return fail("tfx_ocr_scale_channels: null pointer");
  if (B < 0 || HW < 0 || C < 4 || C % 4) return fail("tfx_ocr_scale_channels: C must be a positive multiple of 4");
  if (((uintptr_t)x | (uintptr_t)s | (uintptr_t)out) % 16) return fail("tfx_ocr_scale_channels: x, s and out must be 16-byte aligned");
  const int64_t per = HW * (C / 4), total = per * B;
  if (total >= MAX_ELEMS) return fail("tfx_ocr_scale_channels: too many elements");
  if (total == 0) return 0;
  ocr_scale_channels_kernel<<<blocks256(total), 256, 0, S(stream)>>>(x, s, out, per, C / 4, total);
  return check_launch("ocr_scale_channels");
}

int tfx_ocr_layernorm(const float* x, int64_t ldx, float* out, int64_t ldo, const float* gamma, const float* beta, int64_t rows, int32_t D,
                      float eps, tfx_stream stream) {
  if (!x || !out || !gamma || !beta) return fail("tfx_ocr_layernorm: null pointer");
  if (D < 1 || D > 512) return fail("tfx_ocr_layernorm: 1 <= D <= 512");
  if (rows < 0 || ldx < D || ldo < D) return fail("tfx_ocr_layernorm: rows >= 0 and row pitches >= D are required");
  if (rows >= MAX_ELEMS) return fail("tfx_ocr_layernorm: too many rows");
  if (rows == 0) return 0;
  ocr_layernorm_kernel<<<(unsigned)((rows + 3) / 4), 256, 0, S(stream)>>>(x, ldx, out, ldo, gamma, beta, rows, D, eps);
  return check_launch("ocr_layernorm");
}

int tfx_ocr_attention(const float* qkv, float* out, int32_t B, int32_t N, int32_t H, int32_t d, float scale, tfx_stream stream) {
  if (!qkv || !out) return fail("tfx_ocr_attention: null pointer");
  if (d < 1 || d > 32 || N < 1 || N > 256 || H < 1 || B < 0) return fail("tfx_ocr_attention: 1 <= d <= 32, 1 <= N <= 256, H >= 1 are required");
  if ((int64_t)B * H > 0x7fffffff) return fail("tfx_ocr_attention: B * H does not fit a grid");
  if (B == 0) return 0;
  const int lds = (N * (d | 1) + N * d + 4 * N + 4 * 32) * (int)sizeof(float);
  if (const int rc = prepare_kernel<ocr_attention_kernel>(device_facts().dev, 80 * 1024, "ocr_attention")) return rc;
  ocr_attention_kernel<<<(unsigned)(B * H), 256, lds, S(stream)>>>(qkv, out, H, N, d, scale);
  return check_launch("ocr_attention");
}

int tfx_ctc_rows(const float* logits, int64_t ld, int64_t rows, int32_t C, float* row_max, int32_t* row_arg, float* row_lse, tfx_stream stream) {
  if (!logits || !row_max || !row_arg || !row_lse) return fail("tfx_ctc_rows: null pointer");
  if (C < 1 || ld < C || rows < 0 || rows >= MAX_ELEMS) return fail("tfx_ctc_rows: C >= 1, ld >= C and 0 <= rows < 2^31 are required");
  if (rows == 0) return 0;
  ctc_rows_kernel<<<(unsigned)rows, 256, 0, S(stream)>>>(logits, ld, C, row_max, row_arg, row_lse);
  return check_launch("ctc_rows");
}

int tfx_ctc_score(const float* logits, const int32_t* row_arg, const float* row_lse, const int32_t* targets, const int32_t* offsets,
                  int32_t max_target, int32_t n, int32_t T, int32_t C, int32_t* ids, int32_t* time_index, int32_t* count, float* loss,
                  tfx_stream stream) {
  if (!logits || !row_arg || !ids || !time_index || !count) return fail("tfx_ctc_score: null pointer");
  if (loss && (!row_lse || !targets || !offsets)) return fail("tfx_ctc_score: the loss needs row_lse, targets and offsets (null pointer)");
  if (T < 1 || T > 256 || C < 1 || n < 0) return fail("tfx_ctc_score: 1 <= T <= 256 and C >= 1 are required");
  if (max_target < 0 || max_target > 127) return fail("tfx_ctc_score: targets of at most 127 symbols (max_target is the caller's longest)");
  if (n == 0) return 0;
  ctc_score_kernel<<<(unsigned)n, 256, 0, S(stream)>>>(logits, row_arg, row_lse, targets, offsets, T, C, ids, time_index, count, loss);
  return check_launch("ctc_score");
}

}  // extern "C"
