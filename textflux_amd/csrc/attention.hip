// Joint image+text attention of the FLUX blocks: softmax(Q K^T / sqrt(128)) V, no mask, non-causal, head_dim 128
// (reference site: F.scaled_dot_product_attention, D/models/attention_processor.py:2039-2041).
//
// Flash-style, one workgroup = 256 query rows of one (batch, head): 8 waves x 32 rows.  Per 64-key tile:
//   S^T[key][q] = K . Q^T      v_mfma_f32_32x32x16_bf16(A = K rows from LDS, B = Q rows held in registers)
//   online softmax in fp32, lane-local: with the swapped product every lane owns ONE query row (col = lane&31)
//                               and 32 of the tile's 64 keys; the partner lane (lane^32) owns the other 32.
//   O^T[d][q] += V^T . P^T     A = V^T fragments via ds_read_b64_tr_b16 (hardware transpose read), B = P straight
//                               from the S accumulator registers (bf16-packed) -- the MFMA k-slot order is chosen
//                               to match the accumulator's row order, so P never moves between lanes.
// K and V tiles are staged global -> registers -> LDS (issue early / write late), double buffered, one barrier
// per tile.  K rows (256 B) have their 16-byte chunks XOR-swizzled with (key & 15); V rows have their 64-byte
// segments XOR-swizzled with (key & 3); both make the respective LDS reads bank-conflict free.
#include <atomic>
#include <type_traits>

#include "common.h"
#include "launch.h"

namespace tfx {

constexpr int KVBLK = 64, HD = 128;
#ifdef TFX_BENCH
constexpr int K_BYTES = KVBLK * HD * 2;          // 16 KiB
constexpr int ATT_LDS = 2 * 2 * K_BYTES;         // K,V x 2 buffers = 64 KiB
constexpr int ATT_LDS2 = 2 * ATT_LDS;            // two 64-key sub-tiles per buffer = 128 KiB
constexpr int ATT_LDS_PP = 5 * K_BYTES;          // ping-pong kernel: K x 2, V x 3 buffers = 80 KiB
#endif

typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
__device__ unsigned long long* g_dbg_ptr = nullptr;  // bench-only (tools/attn_timing.py)

// raw barrier (no vmcnt drain: the staged global loads stay in flight across it); LDS traffic of the issuing wave
// is drained first so the partner group sees completed ds_writes.
#define TFX_ATT_BARRIER()                                   \
  do {                                                      \
    __builtin_amdgcn_sched_barrier(0);                      \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      \
    __builtin_amdgcn_s_barrier();                           \
    __builtin_amdgcn_sched_barrier(0);                      \
  } while (0)

// Round 6: the 8-wave kernels of this file (attn_kernel: exact online maximum; attn_mx_kernel: matrix-pipe softmax, the round-1 default;
// attn_pp_kernel: ping-pong) are superseded by attn_w4_kernel (attention_w4.hip) and compiled into the BENCH library only
// (`make bench`, -DTFX_BENCH: tools/variant_tests/ runs their sweeps there); the product library carries the dispatcher below and the
// two attn_w4_kernel instantiations the DiT launches.
#ifdef TFX_BENCH
// Q and O may alias (the single-stream blocks write O over Q; a block only touches its own QBLK rows of one head).
// SUB = 64-key sub-tiles staged per barrier (SUB = 2: 128 keys per barrier, 128 KiB LDS, half the barriers).
// NW waves per workgroup (QBLK = 32 * NW query rows).  NW = 8: one workgroup per CU; NW = 4: two independent
// workgroups per CU (64 KiB LDS each) whose waves share the SIMDs without a common barrier, so one's softmax (VALU)
// overlaps the other's MFMA phases.
// ABL: bench-only ablations (wrong results): bit0 no softmax math, bit1 K fragments read once, bit2 V fragments read
// once, bit3 no K/V staging after the first tile.
template <int NW, int ABL = 0, int SUB = 1>
__global__ __launch_bounds__(NW * 64, 2) void attn_kernel(const bf16_t* Q, const bf16_t* __restrict__ Kp,
                                                   const bf16_t* __restrict__ Vp, bf16_t* O,
                                                   int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, int64_t q_bs,
                                                   int64_t k_bs, int64_t v_bs, int64_t o_bs, int H, int N, int nqb,
                                                   float scale_log2e) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hi = lane >> 5, l31 = lane & 31;

  // block -> (b, h, q-block).  Blocks are dealt round-robin to the 8 XCDs; remap so that each XCD gets a
  // contiguous range of (b, h, q-block), i.e. all q-blocks of a head share one XCD's L2 for that head's K/V.
  int bid = blockIdx.x;
  {
    const int nwg = gridDim.x, q = nwg >> 3, r = nwg & 7, xcd = bid & 7, k = bid >> 3;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + k;
  }
  const int qb = bid % nqb;
  bid /= nqb;
  const int h = bid % H;
  const int b = bid / H;

  const bf16_t* Qb = Q + b * q_bs + h * HD;
  const bf16_t* Kb = Kp + b * k_bs + h * HD;
  const bf16_t* Vb = Vp + b * v_bs + h * HD;
  bf16_t* Ob = O + b * o_bs + h * HD;

  // ---- Q fragments: lane (q = l31, hi) holds d = s*16 + hi*8 + [0,8) for s = 0..7
  constexpr int QBLK = NW * 32, NT = NW * 64, CPT = 1024 / NT;  // chunks of a 16 KiB tile per thread
  const int qrow = qb * QBLK + wave * 32 + l31;
  const int qrow_c = qrow < N ? qrow : N - 1;
  bf16x8 qf[8];
#pragma unroll
  for (int s = 0; s < 8; ++s)
    qf[s] = *reinterpret_cast<const bf16x8*>(Qb + (int64_t)qrow_c * ldq + s * 16 + hi * 8);

  // ---- staging: thread t copies chunks c = t and t + 512 of the 1024 16-byte chunks of a K (and V) tile
  const int nkv = (N + KVBLK - 1) / KVBLK;
  u32x4 kreg[SUB][CPT], vreg[SUB][CPT];
  auto load_tile = [&](int jg) {   // group jg = sub-tiles jg*SUB .. jg*SUB+SUB-1
#pragma unroll
    for (int sb = 0; sb < SUB; ++sb)
#pragma unroll
      for (int i = 0; i < CPT; ++i) {
        const int c = tid + i * NT;
        int key = (jg * SUB + sb) * KVBLK + (c >> 4);
        if (key > N - 1) key = N - 1;
        kreg[sb][i] = *reinterpret_cast<const u32x4*>(Kb + (int64_t)key * ldk + (c & 15) * 8);
        vreg[sb][i] = *reinterpret_cast<const u32x4*>(Vb + (int64_t)key * ldv + (c & 15) * 8);
      }
  };
  auto write_tile = [&](int buf) {
#pragma unroll
    for (int sb = 0; sb < SUB; ++sb) {
      char* kd = smem + (buf * SUB + sb) * 2 * K_BYTES;
      char* vd = kd + K_BYTES;
#pragma unroll
      for (int i = 0; i < CPT; ++i) {
        const int c = tid + i * NT;
        const int key = c >> 4, ch = c & 15;
        *reinterpret_cast<u32x4*>(kd + key * 256 + ((ch ^ (key & 15)) << 4)) = kreg[sb][i];
        *reinterpret_cast<u32x4*>(vd + key * 256 + ((((ch >> 2) ^ (key & 3)) << 6) | ((ch & 3) << 4))) = vreg[sb][i];
      }
    }
  };

  // ---- per-lane LDS read offsets
  // K: row key = kb*32 + l31, chunk (2s+hi) ^ (key & 15); key & 15 == lane & 15.
  uint32_t koff[8];
#pragma unroll
  for (int s = 0; s < 8; ++s) koff[s] = l31 * 256 + (((2 * s + hi) ^ (lane & 15)) << 4);
  // V (transpose read): lane i = lane & 15 of a 16-lane group supplies the address of row (i >> 2),
  // 8-byte piece (i & 3) of the group's 4-key x 16-d block; the group's d offset is 16 * ((lane >> 4) & 1).
  const int vi = lane & 15;
  const uint32_t vrow = (4 * hi + (vi >> 2)) * 256 + 32 * ((lane >> 4) & 1) + (vi & 3) * 8;
  uint32_t voff[4];
#pragma unroll
  for (int db = 0; db < 4; ++db) voff[db] = vrow + ((db ^ ((vi >> 2) & 3)) << 6);

  f32x16 o[4];
#pragma unroll
  for (int db = 0; db < 4; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[db][r] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;

  const int ngrp = (nkv + SUB - 1) / SUB;
  load_tile(0);
  write_tile(0);
  if (ngrp > 1) load_tile(1);
  __syncthreads();

  bf16x8 kab[8], vab;
  unsigned long long tq = 0, tsm = 0, tpv = 0, tst = 0, tmk = 0;
#define LTM() do { if (ABL & 16) { __builtin_amdgcn_sched_barrier(0); tmk = __builtin_readcyclecounter(); } } while (0)
#define LTA(x) do { if (ABL & 16) { __builtin_amdgcn_sched_barrier(0); unsigned long long n_ = __builtin_readcyclecounter(); x += n_ - tmk; tmk = n_; } } while (0)
  for (int jg = 0; jg < ngrp; ++jg) {
    const int buf = jg & 1;
    // staging: group jg+1 (requested one whole group ago) goes into the other buffer -- idle since the barrier that
    // ended group jg-1 -- right away, and the registers are re-used for the request of group jg+2: the loads get a full
    // group of latency hiding and the barrier at the end of the group no longer waits for memory.
    if (jg + 1 < ngrp && !(ABL & 8)) {
      write_tile(buf ^ 1);
      if (jg + 2 < ngrp) load_tile(jg + 2);
    }
#pragma unroll
   for (int sb = 0; sb < SUB; ++sb) {
    const int j = jg * SUB + sb;
    if (j >= nkv) break;
    LTM();
    const char* kt = smem + (buf * SUB + sb) * 2 * K_BYTES;
    const char* vt = kt + K_BYTES;

    // ---- S^T = K Q^T : two 32-key blocks
    f32x16 s0, s1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { s0[r] = 0.f; s1[r] = 0.f; }
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      bf16x8 k0, k1;
      if ((ABL & 2) && j > 0) { k0 = kab[s]; k1 = kab[s]; }
      else {
        k0 = *reinterpret_cast<const bf16x8*>(kt + koff[s]);
        k1 = *reinterpret_cast<const bf16x8*>(kt + koff[s] + 32 * 256);
        if (ABL & 2) kab[s] = k0;
      }
      s0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(k0, qf[s], s0, 0, 0, 0);
      s1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(k1, qf[s], s1, 0, 0, 0);
    }
    LTA(tq);
    if (j == nkv - 1 && (N & (KVBLK - 1))) {  // ragged last tile: keys >= N get -inf
      const int kbase = j * KVBLK + 4 * hi;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = kbase + (r & 3) + 8 * (r >> 2);
        if (key >= N) s0[r] = -INFINITY;
        if (key + 32 >= N) s1[r] = -INFINITY;
      }
    }
    // ---- online softmax (this lane: one query row, 32 keys; partner lane^32: the other 32)
    if (!(ABL & 1)) {
    float mx = s0[0];
#pragma unroll
    for (int r = 1; r < 16; ++r) mx = fmaxf(mx, s0[r]);
#pragma unroll
    for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s1[r]);
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m_new = fmaxf(m_run, mx);
    const float mc = m_new * scale_log2e;
    const float alpha = __builtin_amdgcn_exp2f(m_run * scale_log2e - mc);
    m_run = m_new;
    float psum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      s0[r] = __builtin_amdgcn_exp2f(s0[r] * scale_log2e - mc);
      s1[r] = __builtin_amdgcn_exp2f(s1[r] * scale_log2e - mc);
      psum += s0[r] + s1[r];
    }
    l_run = l_run * alpha + psum;
    if (!__all(alpha == 1.0f)) {  // exact: alpha is exactly 1 whenever the running max did not move
#pragma unroll
      for (int db = 0; db < 4; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[db][r] *= alpha;
    }
    }
    // P as MFMA B operands: step ks covers keys 16*ks + {0..3, 8..11} + 4*hi = accumulator regs 8*(ks&1)..+7
    bf16x8 pf[4];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      pf[0][e] = (__bf16)s0[e];
      pf[1][e] = (__bf16)s0[8 + e];
      pf[2][e] = (__bf16)s1[e];
      pf[3][e] = (__bf16)s1[8 + e];
    }
    LTA(tsm);
    // ---- O^T += V^T P^T
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
#pragma unroll
      for (int db = 0; db < 4; ++db) {
        const char* va = vt + voff[db] + ks * 16 * 256;
        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(va));
        const s16x4 hi4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(va + 8 * 256));
        typedef __attribute__((ext_vector_type(8))) short s16x8;
        const s16x8 both = __builtin_shufflevector(lo, hi4, 0, 1, 2, 3, 4, 5, 6, 7);
        bf16x8 vf = __builtin_bit_cast(bf16x8, both);
        if (ABL & 4) { if (j == 0 && ks == 0 && db == 0) vab = vf; else vf = vab; }
        o[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf[ks], o[db], 0, 0, 0);
      }
    }
    LTA(tpv);
   }
    LTM();
    __syncthreads();
    LTA(tst);
  }
  if ((ABL & 16) && lane == 0 && g_dbg_ptr) {
    unsigned long long* d = g_dbg_ptr + ((size_t)blockIdx.x * 8 + wave) * 4;
    d[0] = tq; d[1] = tsm; d[2] = tpv; d[3] = tst;
  }
#undef LTM
#undef LTA

  // ---- finish: combine the two half-row sums, normalise, store 4 consecutive d per (db, quad)
  const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
  const float inv = 1.0f / l_tot;
  if (qrow < N) {
    bf16_t* orow = Ob + (int64_t)qrow * ldo + 4 * hi;
#pragma unroll
    for (int db = 0; db < 4; ++db)
#pragma unroll
      for (int qd = 0; qd < 4; ++qd) {
        u32x2 w;
        w[0] = pack_bf2(o[db][qd * 4 + 0] * inv, o[db][qd * 4 + 1] * inv);
        w[1] = pack_bf2(o[db][qd * 4 + 2] * inv, o[db][qd * 4 + 3] * inv);
        *reinterpret_cast<u32x2*>(orow + db * 32 + qd * 8) = w;
      }
  }
}


// -------------------------------------------------------------------------------------------------------------
// Matrix-pipe softmax variant (attention_waves = 10).  The lock-step loop above is bound by VALU ISSUE, not by the matrix
// pipe: per 64-key tile a wave issues 32 MFMAs and ~190 VALU instructions, and only ~5 single-issue instructions fit
// beside one 32-cycle MFMA (a v_exp_f32 counts for several) -- the ping-pong experiment below shows the two streams
// mostly serialise.  This kernel moves the softmax's bookkeeping arithmetic onto the idle matrix pipe:
//   * Q is pre-multiplied by scale*log2(e) once per block (one extra bf16 rounding of q), so the scores leave the MFMA in
//     the exp2 domain: no per-score multiply;
//   * the running reference maximum is subtracted BY the MFMA: one extra k-step whose K-side operand is 1 and whose
//     Q-side operand is -m_ref[q] (kept bf16-exact), so S' = K.Q^T - m_ref arrives ready for exp2: no per-score subtract;
//   * the reference maximum is lazy: it only moves when a row's tile maximum exceeds it by more than ATT_THR (in log2
//     units), so P <= 2^ATT_THR and the O rescale, its exp2 and the per-score subtract sit in a rarely taken branch
//     (always taken on the first tile, which pins m_ref to the true row maximum: no underflow of the row sum);
//   * the row sums come out of the PV MFMA: a fifth "d block" whose V-side operand is all ones (4 MFMAs per tile)
//     accumulates l[q] = sum_k bf16(P[k][q]) -- the sum of exactly the weights PV used -- and no lane-local adds.
// Per tile: 38 MFMAs (+19 %), ~90 VALU instructions (-53 %).  Mathematically the same softmax; rounding differs from the
// exact-online-max kernel in q*c and in l (documented, tested against the fp32 oracle with the same tolerance).
constexpr float ATT_THR = 4.0f;

template <int NW>
__global__ __launch_bounds__(NW * 64, 2) void attn_mx_kernel(const bf16_t* Q, const bf16_t* __restrict__ Kp,
                                                         const bf16_t* __restrict__ Vp, bf16_t* O, int64_t ldq,
                                                         int64_t ldk, int64_t ldv, int64_t ldo, int64_t q_bs, int64_t k_bs,
                                                         int64_t v_bs, int64_t o_bs, int H, int N, int nqb, float scale_log2e) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hi = lane >> 5, l31 = lane & 31;
  int bid = blockIdx.x;
  {
    const int nwg = gridDim.x, q = nwg >> 3, r = nwg & 7, xcd = bid & 7, k = bid >> 3;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + k;
  }
  const int qb = bid % nqb;
  bid /= nqb;
  const int h = bid % H;
  const int b = bid / H;
  const bf16_t* Qb = Q + b * q_bs + h * HD;
  const bf16_t* Kb = Kp + b * k_bs + h * HD;
  const bf16_t* Vb = Vp + b * v_bs + h * HD;
  bf16_t* Ob = O + b * o_bs + h * HD;

  // ---- Q fragments, pre-scaled into the exp2 domain
  constexpr int NT = NW * 64, CPT = 1024 / NT;   // threads, 16-byte chunks of a 16 KiB tile per thread
  const int qrow = qb * (NW * 32) + wave * 32 + l31;
  const int qrow_c = qrow < N ? qrow : N - 1;
  bf16x8 qf[8];
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    qf[s] = *reinterpret_cast<const bf16x8*>(Qb + (int64_t)qrow_c * ldq + s * 16 + hi * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) qf[s][e] = (__bf16)((float)qf[s][e] * scale_log2e);
  }

  const int nkv = (N + KVBLK - 1) / KVBLK;
  u32x4 kreg[CPT], vreg[CPT];
  // staging requests: full tiles advance a per-thread row pointer (one 64-bit add per request); only the last, possibly
  // ragged tile recomputes clamped addresses
  const bf16_t* kp[CPT];
  const bf16_t* vp[CPT];
#pragma unroll
  for (int i = 0; i < CPT; ++i) {
    const int c = tid + i * NT;
    kp[i] = Kb + (int64_t)(c >> 4) * ldk + (c & 15) * 8;
    vp[i] = Vb + (int64_t)(c >> 4) * ldv + (c & 15) * 8;
  }
  auto load_tile = [&](int j) {
    if (j == nkv - 1) {
#pragma unroll
      for (int i = 0; i < CPT; ++i) {
        const int c = tid + i * NT;
        int key = j * KVBLK + (c >> 4);
        if (key > N - 1) key = N - 1;
        kreg[i] = *reinterpret_cast<const u32x4*>(Kb + (int64_t)key * ldk + (c & 15) * 8);
        vreg[i] = *reinterpret_cast<const u32x4*>(Vb + (int64_t)key * ldv + (c & 15) * 8);
      }
    } else {
      const int64_t ko = (int64_t)j * KVBLK * ldk, vo = (int64_t)j * KVBLK * ldv;
#pragma unroll
      for (int i = 0; i < CPT; ++i) {
        kreg[i] = *reinterpret_cast<const u32x4*>(kp[i] + ko);
        vreg[i] = *reinterpret_cast<const u32x4*>(vp[i] + vo);
      }
    }
  };
  auto write_tile = [&](int buf) {
    char* kd = smem + buf * 2 * K_BYTES;
    char* vd = kd + K_BYTES;
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
      const int c = tid + i * NT;
      const int key = c >> 4, ch = c & 15;
      *reinterpret_cast<u32x4*>(kd + key * 256 + ((ch ^ (key & 15)) << 4)) = kreg[i];
      *reinterpret_cast<u32x4*>(vd + key * 256 + ((((ch >> 2) ^ (key & 3)) << 6) | ((ch & 3) << 4))) = vreg[i];
    }
  };
  uint32_t koff[8];
#pragma unroll
  for (int s = 0; s < 8; ++s) koff[s] = l31 * 256 + (((2 * s + hi) ^ (lane & 15)) << 4);
  const int vi = lane & 15;
  const uint32_t vrow = (4 * hi + (vi >> 2)) * 256 + 32 * ((lane >> 4) & 1) + (vi & 3) * 8;
  uint32_t voff[4];
#pragma unroll
  for (int db = 0; db < 4; ++db) voff[db] = vrow + ((db ^ ((vi >> 2) & 3)) << 6);

  f32x16 o[4], ol;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    ol[r] = 0.f;
#pragma unroll
    for (int db = 0; db < 4; ++db) o[db][r] = 0.f;
  }
  // constant operands of the two bookkeeping MFMAs.  k-slot 0 belongs to the lanes with hi == 0 (element 0).
  bf16x8 kone, vone, qm;
#pragma unroll
  for (int e = 0; e < 8; ++e) { kone[e] = (__bf16)0.f; vone[e] = (__bf16)1.0f; qm[e] = (__bf16)0.f; }
  if (hi == 0) kone[0] = (__bf16)1.0f;
  float m_ref = 0.f;   // bf16-exact reference maximum of this lane's query row (exp2 domain); -m_ref sits in qm[0]

  load_tile(0);
  write_tile(0);
  if (nkv > 1) load_tile(1);
  __syncthreads();

  // one 64-key tile out of LDS buffer BUF (a compile-time constant: the tile loop is unrolled by two so that the K / V
  // fragment addresses are a per-lane base plus an immediate instead of 14 VALU adds per tile)
  auto tile = [&](int j, auto BUF) {
    constexpr int buf = decltype(BUF)::value;
    if (j + 1 < nkv) {
      write_tile(buf ^ 1);
      if (j + 2 < nkv) load_tile(j + 2);
    }
    const char* kt = smem + buf * 2 * K_BYTES;
    const char* vt = kt + K_BYTES;

    // ---- S'^T = K Q^T - m_ref : the offset k-step first (C = 0), then the 8 real ones
    f32x16 s0, s1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { s0[r] = 0.f; s1[r] = 0.f; }
    s0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kone, qm, s0, 0, 0, 0);
    s1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kone, qm, s1, 0, 0, 0);
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const bf16x8 k0 = *reinterpret_cast<const bf16x8*>(kt + koff[s]);
      const bf16x8 k1 = *reinterpret_cast<const bf16x8*>(kt + koff[s] + 32 * 256);
      s0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(k0, qf[s], s0, 0, 0, 0);
      s1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(k1, qf[s], s1, 0, 0, 0);
    }
    if (j == nkv - 1 && (N & (KVBLK - 1))) {  // ragged last tile: keys >= N get -inf
      const int kbase = j * KVBLK + 4 * hi;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = kbase + (r & 3) + 8 * (r >> 2);
        if (key >= N) s0[r] = -INFINITY;
        if (key + 32 >= N) s1[r] = -INFINITY;
      }
    }
    // ---- row maximum of the tile relative to m_ref (this lane: 32 keys; partner lane^32: the other 32)
    float mx = s0[0];
#pragma unroll
    for (int r = 1; r < 16; ++r) mx = fmaxf(mx, s0[r]);
#pragma unroll
    for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s1[r]);
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    if (j == 0 || !__all(mx <= ATT_THR)) {
      // move the reference: everything accumulated against the old one is rescaled exactly once, the scores of this
      // tile are shifted before they are exponentiated (first tile: pin m_ref to the true maximum, whatever its sign)
      const float m_new = round_bf(m_ref + (j == 0 ? mx : fmaxf(mx, 0.f)));
      const float d = m_new - m_ref;
      const float f = __builtin_amdgcn_exp2f(-d);
      m_ref = m_new;
      qm[0] = (__bf16)(hi == 0 ? -m_new : 0.f);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        s0[r] -= d;
        s1[r] -= d;
        ol[r] *= f;
#pragma unroll
        for (int db = 0; db < 4; ++db) o[db][r] *= f;
      }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      s0[r] = __builtin_amdgcn_exp2f(s0[r]);
      s1[r] = __builtin_amdgcn_exp2f(s1[r]);
    }
    bf16x8 pf[4];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      pf[0][e] = (__bf16)s0[e];
      pf[1][e] = (__bf16)s0[8 + e];
      pf[2][e] = (__bf16)s1[e];
      pf[3][e] = (__bf16)s1[8 + e];
    }
    // ---- O^T += V^T P^T, l += 1^T P^T
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
#pragma unroll
      for (int db = 0; db < 4; ++db) {
        const char* va = vt + voff[db] + ks * 16 * 256;
        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(va));
        const s16x4 hi4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(va + 8 * 256));
        typedef __attribute__((ext_vector_type(8))) short s16x8;
        const s16x8 both = __builtin_shufflevector(lo, hi4, 0, 1, 2, 3, 4, 5, 6, 7);
        o[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, both), pf[ks], o[db], 0, 0, 0);
      }
      ol = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vone, pf[ks], ol, 0, 0, 0);
    }
    __syncthreads();
  };
  for (int j = 0; j < nkv; j += 2) {
    tile(j, std::integral_constant<int, 0>{});
    if (j + 1 < nkv) tile(j + 1, std::integral_constant<int, 1>{});
  }

  // ---- finish: every row of the ones-block holds the full row sum (all 64 keys of every tile)
  const float inv = 1.0f / ol[0];
  if (qrow < N) {
    bf16_t* orow = Ob + (int64_t)qrow * ldo + 4 * hi;
#pragma unroll
    for (int db = 0; db < 4; ++db)
#pragma unroll
      for (int qd = 0; qd < 4; ++qd) {
        u32x2 w;
        w[0] = pack_bf2(o[db][qd * 4 + 0] * inv, o[db][qd * 4 + 1] * inv);
        w[1] = pack_bf2(o[db][qd * 4 + 2] * inv, o[db][qd * 4 + 3] * inv);
        *reinterpret_cast<u32x2*>(orow + db * 32 + qd * 8) = w;
      }
  }
}


// -------------------------------------------------------------------------------------------------------------
// Ping-pong variant.  Same math and data layouts as attn_kernel<8>, different schedule: the tile loop is split into
// a VALU phase   PA(u) = request the 16 V(u) fragments into registers; online softmax of tile u (scores already in
//                        registers); O *= alpha (skipped, exactly, when no row maximum of the wave moved)
// and an MFMA phase PB(u) = O^T += V(u)^T P(u)^T out of registers, the K(u+1) fragments read into the registers the V
//                        fragments vacate, S(u+1) = K(u+1) Q^T out of registers, then the staging writes / requests,
// and the two wave groups (waves 0-3 / 4-7, one wave of each per SIMD) run half an iteration apart, offset by one
// s_barrier: while one group's waves are in their softmax the partner waves on the same SIMDs issue 32 MFMAs whose
// operands are already in registers, so the matrix pipe and the VALU overlap instead of both waves of a SIMD queueing
// for the same pipe.  Slots: G0 PA(u) = 2u, PB(u) = 2u+1; G1 one slot later.
// LDS: K(t) (2 buffers) is read in PB(t-1) and written in PB(t-2); V(t) (3 buffers) is read in PA(t) and written in
// PB(t-2): every write lands >= 1 barrier after the last read of the bytes it replaces and >= 1 barrier before its first
// reader.  Each thread stages its chunks global -> registers one iteration ahead of the write (V(u+3), K(u+3) are
// requested in PB(u) and written in PB(u+1)).
template <bool TIMING>
__global__ __launch_bounds__(512, 2) void attn_pp_kernel(const bf16_t* Q, const bf16_t* __restrict__ Kp,
                                                         const bf16_t* __restrict__ Vp, bf16_t* O, int64_t ldq,
                                                         int64_t ldk, int64_t ldv, int64_t ldo, int64_t q_bs, int64_t k_bs,
                                                         int64_t v_bs, int64_t o_bs, int H, int N, int nqb,
                                                         float scale_log2e, unsigned long long* dbg) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = wave >> 2;
  unsigned long long t_pa = 0, t_b1 = 0, t_pb = 0, t_b2 = 0, tmark = 0;
#define ATM() do { if (TIMING) tmark = __builtin_readcyclecounter(); } while (0)
#define ATA(x) do { if (TIMING) { unsigned long long n_ = __builtin_readcyclecounter(); x += n_ - tmark; tmark = n_; } } while (0)
  const int hi = lane >> 5, l31 = lane & 31;
  int bid = blockIdx.x;
  {
    const int nwg = gridDim.x, q = nwg >> 3, r = nwg & 7, xcd = bid & 7, k = bid >> 3;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + k;
  }
  const int qb = bid % nqb;
  bid /= nqb;
  const int h = bid % H;
  const int b = bid / H;
  const bf16_t* Qb = Q + b * q_bs + h * HD;
  const bf16_t* Kb = Kp + b * k_bs + h * HD;
  const bf16_t* Vb = Vp + b * v_bs + h * HD;
  bf16_t* Ob = O + b * o_bs + h * HD;

  const int qrow = qb * 256 + wave * 32 + l31;
  const int qrow_c = qrow < N ? qrow : N - 1;
  bf16x8 qf[8];
#pragma unroll
  for (int s = 0; s < 8; ++s) qf[s] = *reinterpret_cast<const bf16x8*>(Qb + (int64_t)qrow_c * ldq + s * 16 + hi * 8);

  const int nkv = (N + KVBLK - 1) / KVBLK;
  char* kbuf = smem;                 // K(t) at kbuf + (t&1)*16K
  char* vbuf = smem + 2 * K_BYTES;   // V(t) at vbuf + (t%3)*16K
  u32x4 kreg[2], vreg[2];
  // staging addresses are rebuilt from an opaque copy of the thread id in every iteration: derived from `tid` they are
  // loop invariants that hipcc parks in ~12 VGPRs, which this kernel does not have
  auto opaque_tid = [&]() { int t_ = tid; asm volatile("" : "+v"(t_)); return t_; };
  auto load_rows = [&](const bf16_t* base, int64_t ld, int t, u32x4* reg) {
    const int te = opaque_tid();
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = te + i * 512;
      int key = t * KVBLK + (c >> 4);
      if (key > N - 1) key = N - 1;
      reg[i] = *reinterpret_cast<const u32x4*>(base + (int64_t)key * ld + (c & 15) * 8);
    }
  };
  auto write_k = [&](int t) {
    char* kd = kbuf + (t & 1) * K_BYTES;
    const int te = opaque_tid();
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = te + i * 512, key = c >> 4, ch = c & 15;
      *reinterpret_cast<u32x4*>(kd + key * 256 + ((ch ^ (key & 15)) << 4)) = kreg[i];
    }
  };
  auto write_v = [&](int t) {
    char* vd = vbuf + (t % 3) * K_BYTES;
    const int te = opaque_tid();
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = te + i * 512, key = c >> 4, ch = c & 15;
      *reinterpret_cast<u32x4*>(vd + key * 256 + ((((ch >> 2) ^ (key & 3)) << 6) | ((ch & 3) << 4))) = vreg[i];
    }
  };

  uint32_t koff[8];
#pragma unroll
  for (int s = 0; s < 8; ++s) koff[s] = l31 * 256 + (((2 * s + hi) ^ (lane & 15)) << 4);
  const int vi = lane & 15;
  const uint32_t vrow = (4 * hi + (vi >> 2)) * 256 + 32 * ((lane >> 4) & 1) + (vi & 3) * 8;
  uint32_t voff[4];
#pragma unroll
  for (int db = 0; db < 4; ++db) voff[db] = vrow + ((db ^ ((vi >> 2) & 3)) << 6);

  f32x16 o[4], s0, s1;
#pragma unroll
  for (int db = 0; db < 4; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[db][r] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;
  bf16x8 pf[4];
  typedef __attribute__((ext_vector_type(8))) short s16x8;

  // V fragment i = ks * 4 + db of the tile in buffer vt (two transpose reads each)
  auto ldvf = [&](const char* vt, int i) -> bf16x8 {
    const char* va = vt + voff[i & 3] + (i >> 2) * 16 * 256;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(va));
    const s16x4 hi4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(va + 8 * 256));
    return __builtin_bit_cast(bf16x8, (s16x8)__builtin_shufflevector(lo, hi4, 0, 1, 2, 3, 4, 5, 6, 7));
  };

  // ---- prologue: K(0), K(1), V(0), V(1) into LDS; K(2), V(2) requested; S(0) = K(0) Q^T
  load_rows(Kb, ldk, 0, kreg);
  load_rows(Vb, ldv, 0, vreg);
  write_k(0);
  write_v(0);
  if (nkv > 1) {
    load_rows(Kb, ldk, 1, kreg);
    load_rows(Vb, ldv, 1, vreg);
    write_k(1);
    write_v(1);
    if (nkv > 2) {
      load_rows(Kb, ldk, 2, kreg);
      load_rows(Vb, ldv, 2, vreg);
    }
  }
  __syncthreads();
  {
#pragma unroll
    for (int r = 0; r < 16; ++r) { s0[r] = 0.f; s1[r] = 0.f; }
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const bf16x8 k0 = *reinterpret_cast<const bf16x8*>(kbuf + koff[s]);
      const bf16x8 k1 = *reinterpret_cast<const bf16x8*>(kbuf + koff[s] + 32 * 256);
      s0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(k0, qf[s], s0, 0, 0, 0);
      s1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(k1, qf[s], s1, 0, 0, 0);
    }
  }
  TFX_ATT_BARRIER();
  if (g == 1) TFX_ATT_BARRIER();  // stagger: group 1 runs one slot behind

  int vslot = 0;  // u % 3
  for (int u = 0; u < nkv; ++u) {
    ATM();
    // ================= PA(u): V(u) fragments -> registers; online softmax of tile u; rescale of O (VALU) =============
    bf16x8 vf[16];
    {
      const char* vt = vbuf + vslot * K_BYTES;
#pragma unroll
      for (int i = 0; i < 16; ++i) vf[i] = ldvf(vt, i);
    }
    if (u == nkv - 1 && (N & (KVBLK - 1))) {
      const int kbase = u * KVBLK + 4 * hi;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = kbase + (r & 3) + 8 * (r >> 2);
        if (key >= N) s0[r] = -INFINITY;
        if (key + 32 >= N) s1[r] = -INFINITY;
      }
    }
    {
      float mx = s0[0];
#pragma unroll
      for (int r = 1; r < 16; ++r) mx = fmaxf(mx, s0[r]);
#pragma unroll
      for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s1[r]);
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float m_new = fmaxf(m_run, mx);
      const float mc = m_new * scale_log2e;
      const float alpha = __builtin_amdgcn_exp2f(m_run * scale_log2e - mc);
      m_run = m_new;
      float psum = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        s0[r] = __builtin_amdgcn_exp2f(s0[r] * scale_log2e - mc);
        s1[r] = __builtin_amdgcn_exp2f(s1[r] * scale_log2e - mc);
        psum += s0[r] + s1[r];
      }
      l_run = l_run * alpha + psum;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        pf[0][e] = (__bf16)s0[e];
        pf[1][e] = (__bf16)s0[8 + e];
        pf[2][e] = (__bf16)s1[e];
        pf[3][e] = (__bf16)s1[8 + e];
      }
      if (!__all(alpha == 1.0f)) {  // exact: alpha is exactly 1 whenever the running max did not move
#pragma unroll
        for (int db = 0; db < 4; ++db)
#pragma unroll
          for (int r = 0; r < 16; ++r) o[db][r] *= alpha;
      }
    }
    ATA(t_pa);
    TFX_ATT_BARRIER();
    ATA(t_b1);
    // ================= PB(u): PV(u) and QK(u+1) out of registers (MFMA), staging ====================================
    const char* kt = kbuf + ((u + 1) & 1) * K_BYTES;
    bf16x8 kf[8][2];
    uint32_t kofs[8];   // rebuilt here (opaque lane id): as loop invariants they would sit in 8 VGPRs across PA, the peak
    {
      int le = lane;
      asm volatile("" : "+v"(le));
#pragma unroll
      for (int s = 0; s < 8; ++s) kofs[s] = (le & 31) * 256 + (((2 * s + (le >> 5)) ^ (le & 15)) << 4);
    }
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
#pragma unroll
      for (int db = 0; db < 4; ++db) o[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf[ks * 4 + db], pf[ks], o[db], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      // K(u+1) fragments of k-steps 2ks, 2ks+1 into the registers the V fragments above just vacated (the last tile
      // reads a stale buffer: harmless, its scores are never used)
#pragma unroll
      for (int s = 2 * ks; s < 2 * ks + 2; ++s) {
        kf[s][0] = *reinterpret_cast<const bf16x8*>(kt + kofs[s]);
        kf[s][1] = *reinterpret_cast<const bf16x8*>(kt + kofs[s] + 32 * 256);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int db = 0; db < 4; ++db) asm volatile("" : "+v"(o[db]));   // PV stays in front of what follows
#pragma unroll
    for (int r = 0; r < 16; ++r) { s0[r] = 0.f; s1[r] = 0.f; }
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      s0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[s][0], qf[s], s0, 0, 0, 0);
      s1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[s][1], qf[s], s1, 0, 0, 0);
    }
    asm volatile("" : "+v"(s0), "+v"(s1));
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(0);
    if (u + 2 < nkv) {
      write_k(u + 2);
      write_v(u + 2);
      if (u + 3 < nkv) {
        load_rows(Kb, ldk, u + 3, kreg);
        load_rows(Vb, ldv, u + 3, vreg);
      }
    }
    vslot = vslot == 2 ? 0 : vslot + 1;
    ATA(t_pb);
    TFX_ATT_BARRIER();
    ATA(t_b2);
  }
  if (g == 0) TFX_ATT_BARRIER();
  if (TIMING && lane == 0 && dbg) {
    unsigned long long* d = dbg + ((size_t)blockIdx.x * 8 + wave) * 4;
    d[0] = t_pa; d[1] = t_b1; d[2] = t_pb; d[3] = t_b2;
  }
#undef ATM
#undef ATA

  const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
  const float inv = 1.0f / l_tot;
  if (qrow < N) {
    bf16_t* orow = Ob + (int64_t)qrow * ldo + 4 * hi;
#pragma unroll
    for (int db = 0; db < 4; ++db)
#pragma unroll
      for (int qd = 0; qd < 4; ++qd) {
        u32x2 w;
        w[0] = pack_bf2(o[db][qd * 4 + 0] * inv, o[db][qd * 4 + 1] * inv);
        w[1] = pack_bf2(o[db][qd * 4 + 2] * inv, o[db][qd * 4 + 3] * inv);
        *reinterpret_cast<u32x2*>(orow + db * 32 + qd * 8) = w;
      }
  }
}

#endif  // TFX_BENCH

static int g_attn_bound = 1;   // 0: ignore AttnArgs::score_bound (A/B knob, tfx_set_option attention_use_bound)
void set_attention_use_bound(int v) { g_attn_bound = v; }
// which kernel form the launches took (tfx_attention_mode_counts): host counters, bumped at launch (and at graph capture)
static std::atomic<int64_t> g_attn_mode_count[9];   // [8]: launches (already counted under their mode) whose last round was dealt as (item, tile) units -- stream-K tail
// (zero-initialised: static storage; launches may come from several host threads)
void attention_note_streamk() { ++g_attn_mode_count[8]; }
int attention_mode_counts(int64_t* counts, int n, int reset) {
  n = n < 0 ? 0 : n > 9 ? 9 : n;
  for (int i = 0; i < n; ++i) counts[i] = g_attn_mode_count[i].load(std::memory_order_relaxed);
  if (reset) for (int i = 0; i < 9; ++i) g_attn_mode_count[i].store(0, std::memory_order_relaxed);
  return n;
}
// The reference-free stream (attn_w4_kernel<4>) is admissible when nothing can leave the exponent range fp32 and bf16 share without any
// reference subtracted: scores s in +-b (exp2 domain, b = score_bound * log2 e), weights 2^s in [2^-b, 2^b] (no underflow while b <= 126:
// a row's sum is never 0), row sums <= N 2^b, un-normalised outputs <= N 2^b max|v|.  With |v| <= 2^24 granted (bf16 activations of a
// network; the guarded kernels make the same kind of assumption about N max|v| alone) the condition is b + log2 N + 24 <= 126.
// P1024 (N = 4608): score_bound <= 62.2, i.e. max|w_q| max|w_k| <= 5.3 of a block's q / k RMSNorm weights; round 4 used a flat
// 41 (3.55) out of caution -- the bound is the kernel's property, not the bench weights'.
static bool attn_bound_admissible(float score_bound, int N) {
  return score_bound > 0.f && score_bound * 1.4426950408889634f + log2f((float)N) + 24.0f <= 126.0f;
}
static int g_attn_waves = 30;  // 30 (default) one wave per SIMD, 64 rows per wave, 32x32x16 MFMA (attention_w4.hip); 10 matrix-pipe softmax, 8 waves x 32 rows; 8 exact-online-max lock-step kernel; 4 / 12 = 4-wave workgroups of 8 / 10; 9 = 128 keys per barrier; 16 = ping-pong
static unsigned long long* g_attn_dbg = nullptr;  // bench-only phase timing buffer
void set_attention_debug(void* p) {
  g_attn_dbg = (unsigned long long*)p;
  (void)hipMemcpyToSymbol(HIP_SYMBOL(g_dbg_ptr), &p, sizeof(p));
}
static int g_attn_abl = 0;  // bench-only (tools/bench_kernels.py)
void set_attention_ablation(int a) { g_attn_abl = a; }
void set_attention_waves(int nw) {
  if (nw == 0) { g_attn_waves = 30; return; }
  g_attn_waves = (nw == 4 || nw == 8 || nw == 9 || nw == 10 || nw == 12 || nw == 20 || (nw >= 30 && nw <= 34) || nw == 40) ? nw : 16;
}

// The product library carries the default kernel only (attention_w4.hip: attn_w4_kernel<4>, the reference-free stream the DiT's
// per-block score bound selects, and attn_w4_kernel<0>, the guarded form every other call gets).  It needs 16-byte aligned output
// rows (whole-row stores) and fails loudly otherwise -- the DiT's layouts always are.  Everything else that was tried on the way
// (8: exact online maximum, 10: matrix-pipe softmax with 8 waves x 32 rows, 20: half-tile pipelined, 31 .. 33: other bookkeeping
// modes of the one-wave-per-SIMD kernel, 40: the 16 x 16 x 32 kernel, 4 / 9 / 12 / 16: further schedules) and the timing ablations are
// compiled only with -DTFX_BENCH (`make bench` -> libtextflux_hip_bench.so, used by tools/ and tools/variant_tests/).
int joint_attention(const AttnArgs& a, hipStream_t st) {
  if (a.B <= 0 || a.H <= 0 || a.N <= 0) return 0;
  if ((a.ldq | a.ldk | a.ldv | a.q_bstride | a.k_bstride | a.v_bstride) % 8 || (a.ldo | a.o_bstride) % 4)
    return fail("attention: strides must be multiples of 8 elements (q,k,v) / 4 (o)");
  if (((uintptr_t)a.q | (uintptr_t)a.k | (uintptr_t)a.v) % 16 || (uintptr_t)a.o % 8)
    return fail("attention: q/k/v must be 16-byte aligned, o 8-byte aligned");
  // per-sample lengths (mixed-geometry batches) are a form of kernel 30 alone
  if (a.seq_len && g_attn_waves != 30)
    return fail("attention: seq_len (per-sample lengths) is served by kernel 30 only, attention_waves is %d", g_attn_waves);
  if (a.seq_len && (uintptr_t)a.seq_len % 4) return fail("attention: seq_len must be 4-byte aligned");
#ifdef TFX_BENCH
  if (g_attn_waves == 20 && !g_attn_abl) {   // half-tile software-pipelined kernel
    ProfScope prof(1, 4.0 * a.B * a.H * (double)a.N * a.N * HD, st);
    const int rc = joint_attention_hp(a, st);
    ++g_attn_mode_count[5];
    return rc ? rc : check_launch("joint_attention");
  }
#endif
  // option 30: whole-row 16-byte output stores; its K / V buffer descriptors cover one head's rows with a 32-bit byte count,
  // and its pipeline requests up to three 64-key tiles past the last one: those offsets are computed in 32 bits too and must
  // stay beyond the descriptor's range (zero fill) instead of wrapping back into it
  const uint64_t w4_rows = (uint64_t)((a.N + 63) / 64 + 3) * 64;
  const bool w4_ok = (a.ldo | a.o_bstride) % 8 == 0 && w4_rows * (uint64_t)a.ldk * 2 + 256 < (1ull << 32) &&
                     w4_rows * (uint64_t)a.ldv * 2 + 256 < (1ull << 32);
  // 40 = the 16 x 16 x 32 kernel (attention_w16.hip): fewer matrix cycles and, alone on the chip, 4 % faster than 30 (it sustains
  // 2.23 GHz where 30 sustains 1.95) -- but ~9 % more wave cycles per tile (474 instructions against 358), and inside the DiT step
  // the clock is set by the power-capped GEMMs around it (~1.7 GHz): there cycles decide and 40 measures 2 % SLOWER per forward
  // (tools/dit_ab.py attention_waves=30,40: 481.5 vs 471.1 ms).  Kept selectable, not the default.
  if (a.seq_len && !w4_ok)
    return fail("attention: seq_len needs kernel 30's layout: 16-byte aligned output rows and one head's K / V rows addressable in 32 bits");
#ifdef TFX_BENCH
  if (g_attn_waves == 40 && w4_ok) {     // same output-store and descriptor constraints as 30
    ProfScope prof(1, 4.0 * a.B * a.H * (double)a.N * a.N * HD, st);
    const int rc = joint_attention_w16(a, st);
    ++g_attn_mode_count[6];
    return rc ? rc : check_launch("joint_attention");
  }
#endif
#ifdef TFX_BENCH
  if (((g_attn_waves >= 30 && g_attn_waves <= 34) || g_attn_waves == 40) && w4_ok) {
#else
  if ((g_attn_waves == 30 || g_attn_waves == 34) && w4_ok) {
#endif
    ProfScope prof(1, 4.0 * a.B * a.H * (double)a.N * a.N * HD, st);
    // 30 (the default) takes the reference-free stream (34) when the caller's score bound allows it (attn_bound_admissible above);
    // an explicit 31 .. 33 runs as named
    const bool bounded = attn_bound_admissible(a.score_bound, a.N);
#ifdef TFX_BENCH
    const int mode = g_attn_waves == 34 ? (bounded ? 4 : 3) : g_attn_waves == 30 ? (bounded && g_attn_bound ? 4 : 0)
                   : g_attn_waves >= 31 && g_attn_waves <= 33 ? g_attn_waves - 30 : 0;
#else
    const int mode = bounded && (g_attn_bound || g_attn_waves == 34) ? 4 : 0;    // 30 / 34; the other bookkeeping modes are bench-only
#endif
    const int rc = joint_attention_w4(a, st, mode);
    ++g_attn_mode_count[mode];
    return rc ? rc : check_launch("joint_attention");
  }
#ifndef TFX_BENCH
  if (g_attn_waves != 30 && g_attn_waves != 34)
    return fail("attention: kernel variant %d is a bench-only schedule (libtextflux_hip_bench.so, `make bench`)", g_attn_waves);
  return fail("attention: output rows must be 16-byte aligned (ldo and o_bstride multiples of 8 elements) and one head's K / V rows "
              "addressable in 32 bits; got ldo %lld, o_bstride %lld, N %d, ldk %lld, ldv %lld", (long long)a.ldo, (long long)a.o_bstride,
              a.N, (long long)a.ldk, (long long)a.ldv);
#else
  const int NW = (g_attn_waves == 16 || g_attn_waves == 9 || g_attn_waves == 10 || g_attn_waves >= 30) ? 8 : g_attn_waves == 12 ? 4 : g_attn_waves;
  const int qblk = NW * 32;
  const int dev = device_facts().dev;
  if (prepare_kernel<attn_kernel<8>>(dev, ATT_LDS, "attention") || prepare_kernel<attn_mx_kernel<8>>(dev, ATT_LDS, "attention") ||
      prepare_kernel<attn_kernel<4>>(dev, ATT_LDS, "attention") || prepare_kernel<attn_mx_kernel<4>>(dev, ATT_LDS, "attention") ||
      prepare_kernel<attn_kernel<8, 0, 2>>(dev, ATT_LDS2, "attention") || prepare_kernel<attn_pp_kernel<false>>(dev, ATT_LDS_PP, "attention"))
    return 1;     // the message is prepare_kernel's
  const int nqb = (a.N + qblk - 1) / qblk;
  const unsigned grid = (unsigned)(a.B * a.H * nqb);
  ProfScope prof(1, 4.0 * a.B * a.H * (double)a.N * a.N * HD, st);
  const float sl2 = a.scale * 1.4426950408889634f;
#define ATT_ARGS (const bf16_t*)a.q, (const bf16_t*)a.k, (const bf16_t*)a.v, (bf16_t*)a.o, a.ldq, a.ldk, a.ldv, a.ldo, a.q_bstride, \
                 a.k_bstride, a.v_bstride, a.o_bstride, a.H, a.N, nqb, sl2
#ifdef TFX_BENCH
  if (g_attn_abl) {
    (void)hipFuncSetAttribute((const void*)attn_kernel<8, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, ATT_LDS);
    (void)hipFuncSetAttribute((const void*)attn_kernel<8, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, ATT_LDS);
    (void)hipFuncSetAttribute((const void*)attn_kernel<8, 4>, hipFuncAttributeMaxDynamicSharedMemorySize, ATT_LDS);
    (void)hipFuncSetAttribute((const void*)attn_kernel<8, 8>, hipFuncAttributeMaxDynamicSharedMemorySize, ATT_LDS);
    (void)hipFuncSetAttribute((const void*)attn_kernel<8, 15>, hipFuncAttributeMaxDynamicSharedMemorySize, ATT_LDS);
    (void)hipFuncSetAttribute((const void*)attn_kernel<8, 16>, hipFuncAttributeMaxDynamicSharedMemorySize, ATT_LDS);
    switch (g_attn_abl) {
      case 1: attn_kernel<8, 1><<<grid, 512, ATT_LDS, st>>>(ATT_ARGS); break;
      case 2: attn_kernel<8, 2><<<grid, 512, ATT_LDS, st>>>(ATT_ARGS); break;
      case 4: attn_kernel<8, 4><<<grid, 512, ATT_LDS, st>>>(ATT_ARGS); break;
      case 8: attn_kernel<8, 8><<<grid, 512, ATT_LDS, st>>>(ATT_ARGS); break;
      case 16: attn_kernel<8, 16><<<grid, 512, ATT_LDS, st>>>(ATT_ARGS); break;
      default: attn_kernel<8, 15><<<grid, 512, ATT_LDS, st>>>(ATT_ARGS); break;
    }
  } else if (g_attn_waves == 16) {
    if (g_attn_dbg) {
      (void)hipFuncSetAttribute((const void*)attn_pp_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, ATT_LDS_PP);
      attn_pp_kernel<true><<<grid, 512, ATT_LDS_PP, st>>>(ATT_ARGS, g_attn_dbg);
    } else {
      attn_pp_kernel<false><<<grid, 512, ATT_LDS_PP, st>>>(ATT_ARGS, nullptr);
    }
  } else if (g_attn_waves == 12) {   // matrix-pipe softmax, two independent 4-wave workgroups per CU
    attn_mx_kernel<4><<<grid, 256, ATT_LDS, st>>>(ATT_ARGS);
  } else if (g_attn_waves == 9) {    // 8 waves, two 64-key sub-tiles per barrier
    attn_kernel<8, 0, 2><<<grid, 512, ATT_LDS2, st>>>(ATT_ARGS);
  } else if (g_attn_waves == 4) {
    attn_kernel<4><<<grid, 256, ATT_LDS, st>>>(ATT_ARGS);
  } else
#endif
  if (g_attn_waves == 10 || (g_attn_waves >= 30 && g_attn_waves <= 34))   // matrix-pipe softmax, one 8-wave workgroup per CU (30 lands here when its alignment needs are not met)
    attn_mx_kernel<8><<<grid, 512, ATT_LDS, st>>>(ATT_ARGS);
  else                               // exact online maximum
    attn_kernel<8><<<grid, 512, ATT_LDS, st>>>(ATT_ARGS);
#undef ATT_ARGS
  ++g_attn_mode_count[7];
  return check_launch("joint_attention");
#endif  // TFX_BENCH
}

}  // namespace tfx
