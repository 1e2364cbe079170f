// One-wave-per-SIMD joint attention (attention_waves = 30, the default): same math and matrix-pipe softmax bookkeeping as
// attn_mx_kernel (attention.hip), rebuilt around the SIMD's ISSUE budget.
//
// attn_mx_kernel gives every wave 32 query rows; per 64-key tile a wave issues 38 MFMAs (304 issue cycles), 32 v_exp_f32
// (8 cycles each), ~60 other VALU instructions and 48 LDS fragment reads -- about as many issue cycles as the 1216
// matrix-pipe cycles its MFMAs occupy, and with two waves per SIMD (served oldest-first, not interleaved) the two streams
// add up instead of overlapping: the pipe is 53-57 % busy whatever the schedule.  What does overlap is work issued by the
// SAME wave behind its own MFMA (tools/ubench/mfma_fill: one wave hides ~24 issue cycles behind each 32-cycle MFMA: four
// simple VALU instructions, or two v_exp_f32 and one more, or two LDS reads and two VALU).  The K / V fragment reads and
// the staging traffic are per WAVE, not per row, so here
//   * a workgroup is 4 waves (one per SIMD, the whole 512-register file each), a wave owns 64 query rows = two 32-row
//     q-blocks: every K / V fragment read from LDS feeds two MFMAs, staging per row halves;
//   * the tile loop is software-pipelined at the granularity of a UNIT = (32-key block, q-block): in step u the MFMA stream
//     is S(u+1) = K Q^T - m_ref (1 + 8 MFMAs, a dependent chain) interleaved with O^T += V^T P(u-1)^T, l += 1^T P(u-1)^T
//     (2 x (4 + 1) MFMAs, independent accumulators), and the VALU stream in their shadow is the softmax of unit u
//     (row maximum -> [rarely] move the lazy reference -> 16 v_exp_f32 + 8 v_cvt_pk_bf16_f32).  Consecutive units
//     alternate between the two q-blocks, so the unit whose reference may move (u) never has MFMAs in flight on its own
//     accumulators: moving the reference rescales O / l of q-block u & 1 only;
//   * units run (kb0,q0) (kb0,q1) (kb1,q0) (kb1,q1): the K fragments of a key block serve two consecutive S chains and
//     the V fragments two consecutive P.V groups; each fragment register is reloaded shortly after its last use, one whole
//     step (~600 cycles) before its next, so no LDS latency is ever waited for and no fragment is double-buffered;
//   * ONE MFMA per scheduling region (sched_barrier), each followed by <= ~24 issue cycles of other work: an MFMA that finds
//     the pipe busy blocks its wave's issue until the pipe takes it, so work placed behind two adjacent MFMAs is not hidden
//     by the first.  Common path = fall-through (the reference move and the ragged mask are out of line): with one wave
//     per SIMD nothing hides the instruction-fetch bubble of a taken branch.
// Register files: the MFMAs are hipcc builtins and this file is compiled with -mllvm -amdgpu-mfma-vgpr-form (Makefile): the
// scores must come out in ArchVGPRs (the VALU reads them; the AGPR form costs a v_accvgpr_read per score), hipcc then keeps
// C / D of every MFMA in ArchVGPRs (O + l = 160, scores 32, weights 16) and most K / V fragments, the staging registers and
// -- pinned by an empty asm -- the 64 Q registers in the AccVGPRs, which srcA / srcB read directly (256 + ~165 registers).
// A hazard hipcc cannot see: the row maxima and the bf16 packs are inline asm (so that they stay where the schedule puts
// them); an MFMA result needs ~11 issued instructions before a VALU read and the hazard pass does not know those asm
// statements are VALU.  The score chain therefore runs one MFMA AHEAD of the P.V group: its last MFMA is followed by three
// MFMAs of its own step and the first of the next before the scores are read (reading earlier returned stale rows,
// sporadically: tests/test_kernels_gpu.py::test_attention_default_kernel_is_deterministic_and_nan_free); the only read
// right behind a chain (prologue) and the output sit behind an explicit drain.  (An MFMA's A / B operands, on the other
// hand, are safe as soon as it has issued: tools/ubench/mfma_war.)
// LDS: ring of 3 tiles (K rows padded to 272 B -> conflict-free b128 reads from ONE per-lane base register + immediates;
// V rows 256 B with their 64-byte segments XOR-swizzled for the transpose reads; PMC: 2.6 M conflict cycles in 199 M LDS-array
// cycles = 1.3 %, profiles/r03_attention_pmc.json), one barrier per
// 64-key tile.  Staging global -> registers -> LDS runs as a stream in the MFMA gaps of step 1 of every tile: piece g of tile
// j + 2 goes to LDS and its register is refilled with the same piece of tile j + 3 right behind, four steps (> 1 us) before
// it is needed -- with one wave per SIMD nothing else runs while a wave waits for memory.  The buffer descriptors are sized
// to the N valid rows, so the rows of a ragged last tile and whole tiles requested past the end read as zeros without any
// clamping code (their scores are masked / their weights are zero).
// Measured (MI355X, B = 8, H = 24, N = 4608, random data): 1.12-1.14 PFLOP/s vs 1.04-1.07 for attn_mx_kernel on the same
// box, 480 vs 495 ms per 57-block DiT forward; on zero data (no power cap) 1.44 PFLOP/s.  Both are power-limited on random
// data: 1.9 GHz at 1300 W.
#include <mutex>
#include <type_traits>

#include "common.h"
#include "launch.h"

namespace tfx {

namespace {
constexpr int W4_KV = 64, W4_HD = 128;
constexpr int W4_VT = W4_KV * 256;             // V tile bytes
constexpr int W4_KROW = 272;                   // K row pitch
constexpr int W4_KT = W4_KV * W4_KROW;         // K tile bytes
constexpr int W4_NBUF = 3;
constexpr int W4_KBASE = W4_NBUF * W4_VT;      // V tiles first, then K tiles
constexpr int W4_PROW = 132;                   // floats per row of a partial (size only: 128 d + row sum + reference maximum + pad; 256 rows per slot)
// Layout of one partial slot (256 x 132 floats; round 6 -- until then row-major, which made every store instruction of the producing kernel
// touch 64 different lines): the un-normalised O in the PRODUCER's register order -- 16-byte element ((wq, db, qd), lane), wq = wave * 2 +
// q-block, lane = hi * 32 + row-in-block, holds columns db * 32 + qd * 8 + hi * 4 .. + 4 of row wq * 32 + (lane & 31): one store instruction
// = 1 KiB contiguous -- followed by (row sum, reference maximum) pairs per row.
__device__ __forceinline__ int w4_part_off(int r, int col) {   // float offset of columns col .. col + 3 (col % 4 == 0) of row r (0 .. 255)
  return ((((r >> 5) * 4 + (col >> 5)) * 4 + ((col >> 3) & 3)) * 64 + ((col >> 2) & 1) * 32 + (r & 31)) * 4;
}
constexpr int W4_PART_LM = 256 * 128;          // float offset of the (l, m) pairs
constexpr float W4_THR = 4.0f;                 // lazy-reference threshold (log2 units), as attn_mx_kernel (MODE 0 / 1)
constexpr float W4_BIG = 64.0f;                // MODE 2: a row's reference stays 0 while its scores stay inside +-W4_BIG
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((ext_vector_type(2))) __bf16 bf2_t;
template <int V>
using IC = std::integral_constant<int, V>;
}  // namespace

constexpr int ATT_LDS_W4 = W4_NBUF * (W4_VT + W4_KT);   // 99 KiB

#define W4_GAP() __builtin_amdgcn_sched_barrier(0)
#ifndef W4_ABL
#define W4_ABL 0   // timing ablations (wrong results): 1 no exp / pack, 2 no fragment reloads, 4 no staging, 8 no row maximum / branch, 16 no barrier, 64 no staging writes (requests kept), 128 no staging requests (writes kept), 256 requests as LDS-DMA into a scratch region (use with 64), 512 V fragments by one ds_read_b128 (a transposed V tile), 1024 the Q-side RMSNorm + RoPE in the Q prologue (what moving it out of the projection GEMM would cost here)
#endif
// wait until every issued MFMA has written its result (there is no counter for the matrix pipe): 24 x 16 idle issue slots,
// used twice per workgroup (before the first softmax, before the output)
#define W4_DRAIN_MFMA()                                                                                                 \
  asm volatile("s_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\t"      \
               "s_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\t"      \
               "s_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15" ::: "memory")

// The scores are read by inline-asm VALU instructions (below), which hipcc's hazard recogniser does not see as VALU: it would
// not insert the wait states an MFMA result needs before a VALU read (8-pass MFMA: 11).  W4_TOUCH(acc) is a COMPILER-VISIBLE
// VALU read of the accumulator tuple (v_readfirstlane_b32 of one element; the hazard is tracked per destination tuple) placed
// in program order before the first asm read: the recogniser pads in front of IT, whatever a future compiler or a schedule
// change does to the distance, and every later read is at least as far from the MFMA.  tools/check_mfma_hazard.py verifies
// the emitted ISA (tests/test_isa_hazards.py; -DW4_NO_TOUCH removes the touch and shortens the distance: the self-test).
#ifndef W4_NO_TOUCH
#define W4_TOUCH(acc)                                                                  \
  do {                                                                                 \
    const int t_ = __builtin_amdgcn_readfirstlane(__float_as_int((acc)[0]));           \
    asm volatile("" ::"s"(t_));                                                        \
  } while (0)
#else
#define W4_TOUCH(acc) do { } while (0)
#endif

__device__ __forceinline__ void w4_mfma_s0(f32x16& d, const bf16x8& k, const bf16x8& q) {
  f32x16 z;
#pragma unroll
  for (int r = 0; r < 16; ++r) z[r] = 0.f;
  d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(k, q, z, 0, 0, 0);
}
__device__ __forceinline__ void w4_mfma_s(f32x16& d, const bf16x8& k, const bf16x8& q) {
  d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(k, q, d, 0, 0, 0);
}
__device__ __forceinline__ void w4_mfma_o(f32x16& d, const bf16x8& v, const u32x4& p) {
  d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(v, __builtin_bit_cast(bf16x8, p), d, 0, 0, 0);
}
__device__ __forceinline__ void w4_mfma_l(f32x16& d, const bf16x8& ones, const u32x4& p) {
  d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ones, __builtin_bit_cast(bf16x8, p), d, 0, 0, 0);
}
// single-instruction VALU helpers: hipcc would canonicalise MFMA outputs (v_max x, x) in front of fmaxf and sink the
// exponentials / conversions to their first use in the NEXT step -- these stay where the schedule puts them
__device__ __forceinline__ float w4_max7(float a, float b, float c, float d, float e, float f, float g) {
  float r;
  asm("v_max3_f32 %0, %1, %2, %3\n\tv_max3_f32 %0, %0, %4, %5\n\tv_max3_f32 %0, %0, %6, %7"
      : "=&v"(r) : "v"(a), "v"(b), "v"(c), "v"(d), "v"(e), "v"(f), "v"(g));
  return r;
}
__device__ __forceinline__ float w4_max4(float a, float b, float c, float d) {
  float r;
  asm("v_max3_f32 %0, %1, %2, %3\n\tv_max_f32 %0, %0, %4" : "=&v"(r) : "v"(a), "v"(b), "v"(c), "v"(d));
  return r;
}
__device__ __forceinline__ float w4_max(float a, float b) {
  float r;
  asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
// l += p.lo + p.hi (the two bf16 weights of a packed register, times 1.0 each), fp32 accumulate
__device__ __forceinline__ void w4_dot2c(float& l, uint32_t p) {
  asm volatile("v_dot2c_f32_bf16 %0, 0x3f803f80, %1" : "+v"(l) : "v"(p));
}
__device__ __forceinline__ uint32_t w4_cvt_pk(float lo, float hi) {
  uint32_t r;
  asm volatile("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
  return r;
}
// MODE 0: the round-2 bookkeeping (row sums and the reference offset on the matrix pipe: 76 MFMAs per 64-key tile, 64 of them
// Q.K^T / P.V).  MODE 1: the row sums leave the matrix pipe -- with the swapped Q.K^T a query row is lane-local, so l += sum p is
// eight v_dot2c_f32_bf16 (p0 * 1 + p1 * 1 + l: exactly the bf16 weights P.V multiplies) per unit, issued one step later in the
// MFMA shadow of the step's first regions; per-lane partial sums (each lane holds 16 of a unit's 32 keys), the two halves of a
// row meet once, at the end: 68 MFMAs per tile.  MODE 2: as 1, and the reference offset (one MFMA per unit whose only job is
// to subtract m_ref) is issued only while some row of the wave HAS a non-zero reference: the reference stays 0 as long as a row's
// scores stay inside +-W4_BIG (exp2 domain; softmax does not depend on the reference, and fp32 / bf16 share an exponent range
// that holds 2^+-64 weights and their sums over 2^13 keys with room to spare), is pinned to the row maximum by the first tile
// only when that lies outside, and moves later only when a row's maximum exceeds it by more than W4_BIG: 64 MFMAs per tile on
// ordinary data, the MODE-1 stream otherwise (a wave-uniform, not-taken branch in front of the chain).  MODE 3: MODE 0's stream
// (row sums on the matrix pipe) with MODE 2's lazy reference offset: 72 MFMAs per tile, no VALU instruction more than MODE 0.
// MODE 4: no reference at all (no row maximum, no branch, no offset MFMA) -- only launched when the caller's score bound is ADMISSIBLE
// (attention.hip::attn_bound_admissible, round 5): with |scale q.k| <= score_bound the exp2-domain scores lie in +-b, b = bound log2 e,
// every weight in [2^-b, 2^b], a row sum <= N 2^b and an un-normalised output <= N 2^b max|v|; nothing leaves the exponent range fp32 and
// bf16 share while b + log2 N + 24 <= 126, which GRANTS |v| <= 2^24 (a property of the caller's V that the library cannot verify from the
// norm weights; the guarded modes assume the same kind of thing about N max|v|).  N = 4608: b <= 89.8, score_bound <= 62.2 -- more than
// W4_BIG, which only governs the lazy reference of modes 2 / 3.  The DiT derives the bound from the q / k RMSNorm weights: after the
// norm |q| <= sqrt(128) max|w_q|, RoPE preserves the norm, so |q . k| scale <= 128 max|w_q| max|w_k| 128^-1/2.
#ifdef TFX_BENCH
// bench library only (tools/attn_item_timers.py): s_memtime sums of wave 0 per workgroup {prologue, tile loop, output, items}
__device__ unsigned long long* g_w4_timers = nullptr;
#define W4_STAMP(i) do { if (wave == 0) w4_stamp[i] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define W4_STAMP(i) ((void)0)
#endif
// Stream-K tail of the persistent form (round 6, tfx_set_option attention_streamk).  Every batch sample has its own group of C / B CUs.  The
// sample's items run as whole items, round by round (CU c takes items c, c + group, ...: the CUs of a group work on neighbouring items at any
// time, so a head's K / V stay L2-resident among them), as long as a round is full; the R < group items of the last, partly filled round are
// dealt as (item, 64-key tile) units instead: their R nkv units, item-major, are cut into `group` contiguous ranges of `share` units, one per
// CU, so that every CU ends with the same number of key tiles (13 items + half an item each at P1024 batch 8 instead of 14 items on half of
// the CUs and 13 on the others).  Boundary c of the tail = c * share, snapped to the item boundary when it would leave a piece shorter than
// W4_SK_MIN tiles.  A tail item cut by a boundary leaves un-normalised partials (the tail split's format) that attn_w4_merge_sk_kernel adds up.
// Every sample is dealt by the same rule: identical samples of a batch produce identical bits; a sample's bits do depend on the batch
// size (as with the K-sliced GEMMs).  (First version of the round: ALL units of a sample dealt contiguously -- 15 % SLOWER at P1024 batch 8:
// the CUs of an XCD then sit 13 items apart and nothing they load is shared in L2.)
constexpr int W4_SK_MIN = 4;
__host__ __device__ __forceinline__ int w4_sk_bound(int c, int group, int share, int nkv, int total) {
  if (c >= group) return total;
  int p = c * share;
  if (p >= total) return total;
  const int r = p % nkv;
  if (r < W4_SK_MIN) p -= r;
  else if (r > nkv - W4_SK_MIN) p += nkv - r;
  return p < total ? p : total;
}

// Per-sample lengths (VL, tfx_attn_args.seq_len; mixed-geometry batches): sample b's length, clamped to [1, N] so that a bad value cannot
// address outside the operands.  b is workgroup-uniform: a scalar load.
__device__ __forceinline__ int w4_len(const int32_t* __restrict__ seq_len, int b, int N) {
  const int L = seq_len[b];
  return L < 1 ? 1 : L > N ? N : L;
}

// the kernel, in its two forms (attention_w4_body.h)
#define W4_KERNEL_NAME attn_w4_kernel
#define W4_VL 0
#define W4_SEQ_LEN_PARAM
#define W4_SEQ_LEN_NULL constexpr const int32_t* seq_len = nullptr;     // (named by the discarded VL branches only)
#include "attention_w4_body.h"
#undef W4_KERNEL_NAME
#undef W4_VL
#undef W4_SEQ_LEN_PARAM
#undef W4_SEQ_LEN_NULL
// per-sample lengths (tfx_attn_args.seq_len): whole items, persistent or one workgroup per item; sk_share = 0, nsplit = 1
#define W4_KERNEL_NAME attn_w4v_kernel
#define W4_VL 1
#define W4_SEQ_LEN_PARAM , const int32_t* __restrict__ seq_len
#define W4_SEQ_LEN_NULL
#include "attention_w4_body.h"
#undef W4_KERNEL_NAME
#undef W4_VL
#undef W4_SEQ_LEN_PARAM
#undef W4_SEQ_LEN_NULL

// Finishes the q-tiles of a tail split: O = sum_r o_r 2^(m_r - m) / sum_r l_r 2^(m_r - m), m = max_r m_r (exp2 domain, the
// kernel's own bookkeeping).  One thread per (row, 4 head-dim columns).
__global__ __launch_bounds__(256) void attn_w4_merge_kernel(const float* part, bf16_t* O, int64_t ldo, int64_t o_bs, int H, int N,
                                                            int nqb, int xsplit, int nsplit) {
  const int rg = blockIdx.x * 8 + (threadIdx.x >> 5), c = (threadIdx.x & 31) * 4;
  const int ptile = rg >> 8, r = rg & 255;
  const int pair = H * nqb - xsplit + ptile % xsplit, b = ptile / xsplit, h = pair / nqb, qblk = pair % nqb;
  const int row = qblk * 256 + r;
  if (row >= N) return;
  const float* pr = part + (int64_t)ptile * nsplit * (256 * W4_PROW);
  const int po = w4_part_off(r, c), lo = W4_PART_LM + r * 2;
  float m = -INFINITY;
  for (int k = 0; k < nsplit; ++k) m = fmaxf(m, pr[(int64_t)k * 256 * W4_PROW + lo + 1]);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  float l = 0.f;
  for (int k = 0; k < nsplit; ++k) {
    const float* pk = pr + (int64_t)k * 256 * W4_PROW;
    const float w = __builtin_amdgcn_exp2f(pk[lo + 1] - m);
    const f32x4 v = *reinterpret_cast<const f32x4*>(pk + po);
    acc += v * w;
    l += pk[lo] * w;
  }
  const float inv = 1.0f / l;
  u32x2 o2;
  o2[0] = pack_bf2(acc[0] * inv, acc[1] * inv);
  o2[1] = pack_bf2(acc[2] * inv, acc[3] * inv);
  *reinterpret_cast<u32x2*>(O + b * o_bs + (int64_t)row * ldo + h * W4_HD + c) = o2;
}

// Stream-K: adds up the partials of every tail item that a CU boundary cuts.  8 blocks per (sample, boundary), one per 32-row block of the item;
// the blocks of a boundary that cuts nothing, or that is not the FIRST boundary inside its item, leave at once.  Parts of tail item i, in key
// order: slot B (2 L + 1) of the CU whose range contains the item's first tile, then slot A (2 L) of every CU whose non-empty range starts
// inside the item.  Threads read in the producer's register order (w4_part_off: wave w = column block db, 1 KiB contiguous per load
// instruction; the first version read row-major positions out of that layout and ran at 1.6 TB/s -- 36 us per launch, more than the
// dealing saves), the bf16 rows leave through an LDS tile as whole 256-byte rows.  Same arithmetic as attn_w4_merge_kernel (the reference
// maxima are all 0 on the reference-free stream: the weights are 1, the merge a plain sum).
__global__ __launch_bounds__(256) void attn_w4_merge_sk_kernel(const float* part, bf16_t* O, int64_t ldo, int64_t o_bs, int H, int N, int nqb,
                                                               int group, int share, int Tp) {
  __shared__ __attribute__((aligned(16))) unsigned short sm[32][128 + 8];
  const int bi = blockIdx.x >> 3, wq = blockIdx.x & 7;
  const int sample = bi / group, c = bi - sample * group;
  if (c == 0) return;
  const int nkv = (N + W4_KV - 1) / W4_KV, full = (Tp / group) * group, total = (Tp - full) * nkv;
  const int p = w4_sk_bound(c, group, share, nkv, total);
  if (p >= total || p % nkv == 0) return;
  const int il = p / nkv, istart = il * nkv, iend = istart + nkv;
  if (w4_sk_bound(c - 1, group, share, nkv, total) > istart) return;
  const int gi = full + il, h = gi / nqb, qblk = gi - h * nqb;
  if (qblk * 256 + wq * 32 >= N) return;
  int slots[8], np = 0;
  slots[np++] = 2 * (sample * group + c - 1) + 1;
  for (int j = c; j < group && np < 8; ++j) {
    const int lo = w4_sk_bound(j, group, share, nkv, total), hi = w4_sk_bound(j + 1, group, share, nkv, total);
    if (lo >= iend || lo >= total) break;
    if (hi > lo) slots[np++] = 2 * (sample * group + j);
  }
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l31 = lane & 31, hi = lane >> 5;
  const int lmo = W4_PART_LM + (wq * 32 + l31) * 2, vo = ((wq * 4 + w) * 4 * 64 + lane) * 4;
  float2 lm[8];
  float m = -INFINITY;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    lm[k] = float2{0.f, -INFINITY};
    if (k < np) lm[k] = *reinterpret_cast<const float2*>(part + (int64_t)slots[k] * (256 * W4_PROW) + lmo);
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) m = fmaxf(m, lm[k].y);
  f32x4 acc[4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  float l = 0.f;
#pragma unroll
  for (int k = 0; k < 8; ++k)
    if (k < np) {            // block-uniform
      const float* pk = part + (int64_t)slots[k] * (256 * W4_PROW) + vo;
      f32x4 v[4];
#pragma unroll
      for (int qd = 0; qd < 4; ++qd) v[qd] = *reinterpret_cast<const f32x4*>(pk + qd * 256);
      const float wgt = __builtin_amdgcn_exp2f(lm[k].y - m);
#pragma unroll
      for (int qd = 0; qd < 4; ++qd) acc[qd] += v[qd] * wgt;
      l += lm[k].x * wgt;
    }
  const float inv = 1.0f / l;
#pragma unroll
  for (int qd = 0; qd < 4; ++qd) {
    u32x2 o2;
    o2[0] = pack_bf2(acc[qd][0] * inv, acc[qd][1] * inv);
    o2[1] = pack_bf2(acc[qd][2] * inv, acc[qd][3] * inv);
    *reinterpret_cast<u32x2*>(&sm[l31][w * 32 + qd * 8 + hi * 4]) = o2;
  }
  __syncthreads();
  const int orow = tid >> 3, och = tid & 7, row = qblk * 256 + wq * 32 + orow;
  if (row < N) {
    bf16_t* dst = O + sample * o_bs + (int64_t)row * ldo + h * W4_HD + och * 16;
    *reinterpret_cast<u32x4*>(dst) = *reinterpret_cast<const u32x4*>(&sm[orow][och * 16]);
    *reinterpret_cast<u32x4*>(dst + 8) = *reinterpret_cast<const u32x4*>(&sm[orow][och * 16 + 8]);
  }
}

// scratch of the tail split: one per (device, stream) that ever ran a split launch -- two launches in flight on different streams
// (a graph replay on a side stream next to an eager call) must not share partials.  Allocated on first use outside a stream
// capture, freed only by tfx_release_scratch (captured graphs keep the pointer); a launch on a stream without scratch (first seen
// during capture, or the table is full) simply runs unsplit.
static constexpr int W4_PART_TILES = 1024;   // (q-tile, key range) slots: 2 rounds of a 512-CU chip, 138 MB
static constexpr int W4_PART_SLOTS = 8;
struct W4Scratch { int dev; hipStream_t st; float* part; int cus; };
static W4Scratch g_w4_scr[W4_PART_SLOTS];
static int g_w4_nscr = 0;
static std::mutex g_w4_mu;
// tfx_set_option attention_tail_split: OFF by default -- a sample's attention output must not depend on how many samples share its
// batch (tests/test_fullsize_gpu.py asserts it bit for bit), and which tiles fall into the last round does; 1 = split when it pays
static int g_w4_split = 0;
void set_attention_tail_split(int v) { g_w4_split = v; }

// the scratch of (current device, st); allocates it when `may_alloc` (never inside a stream capture)
static const W4Scratch* w4_scratch(hipStream_t st, bool may_alloc) {
  const DeviceFacts dv = device_facts();
  std::lock_guard<std::mutex> lk(g_w4_mu);
  for (int i = 0; i < g_w4_nscr; ++i)
    if (g_w4_scr[i].dev == dv.dev && g_w4_scr[i].st == st) return &g_w4_scr[i];
  if (!may_alloc || g_w4_nscr == W4_PART_SLOTS) return nullptr;
  W4Scratch s{dv.dev, st, nullptr, dv.cus};
  if (hipMalloc((void**)&s.part, (size_t)W4_PART_TILES * 256 * W4_PROW * sizeof(float)) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  g_w4_scr[g_w4_nscr] = s;
  return &g_w4_scr[g_w4_nscr++];
}

int attention_w4_release() {
  std::lock_guard<std::mutex> lk(g_w4_mu);
  if (g_w4_nscr == 0) return 0;
  (void)hipDeviceSynchronize();
  int cur = 0;
  (void)hipGetDevice(&cur);
  for (int i = 0; i < g_w4_nscr; ++i) {
    (void)hipSetDevice(g_w4_scr[i].dev);
    (void)hipDeviceSynchronize();
    (void)hipFree(g_w4_scr[i].part);
  }
  (void)hipSetDevice(cur);
  (void)hipGetLastError();
  g_w4_nscr = 0;
  return 0;
}

int attention_w4_prepare(hipStream_t st) {
  if (!g_w4_split) return 0;      // nothing to allocate while the tail split is off (the default)
  return w4_scratch(st, true) ? 0 : fail("attention: cannot allocate the tail-split scratch");
}

// tfx_set_option attention_streamk: 1 (default) = deal (item, key tile) units instead of whole items when the estimate below says it pays and
// the caller passed a workspace (AttnArgs::workspace); 0 = whole items only (a sample's bits then do not depend on the batch size); 2 = always
// when admissible (tests).
static int g_w4_streamk = 1;
void set_attention_streamk(int v) { g_w4_streamk = v; }
static int g_w4_persist = 1;     // tfx_set_option attention_persistent: 0 = one workgroup per (b, h, q-tile) item (round 3)
void set_attention_persistent(int v) { g_w4_persist = v; }

#ifdef TFX_BENCH
extern "C" void tfx_bench_attn_timers(unsigned long long* dev) {
  (void)hipMemcpyToSymbol(HIP_SYMBOL(g_w4_timers), &dev, sizeof(dev));
}
#endif

template <int MODE>
static int w4_launch(const AttnArgs& a, hipStream_t st, unsigned grid, const DeviceFacts& dv, int nqb, int nfull, int nparts, int nsplit, int xsplit,
                     float* part, int sk_group, int sk_share) {
  constexpr int lds = ATT_LDS_W4 + ((W4_ABL & 256) ? 4096 : 0);
  // built without -mllvm -amdgpu-mfma-vgpr-form (see Makefile) the accumulators land in the AccVGPRs and ~500 registers spill
  const KernelVet no_spills = [](const hipFuncAttributes& fa) {
    return fa.localSizeBytes == 0 ? 0 : fail("attention: attn_w4_kernel<%d> spills %zu bytes per lane -- attention_w4.hip must be compiled with "
                                             "-mllvm -amdgpu-mfma-vgpr-form", MODE, (size_t)fa.localSizeBytes);
  };
  if (a.seq_len) {               // per-sample lengths: whole items (the caller passes nsplit = 1, sk_share = 0), persistent when there are more items than CUs
    if (const int rc = prepare_kernel<attn_w4v_kernel<MODE>>(dv.dev, lds, "attention (attn_w4v_kernel)", no_spills)) return rc;
    int T_items = 0;
    if (g_w4_persist && (int)grid > dv.grid) { T_items = (int)grid; grid = (unsigned)dv.grid; }
    attn_w4v_kernel<MODE><<<grid, 256, lds, st>>>((const bf16_t*)a.q, (const bf16_t*)a.k, (const bf16_t*)a.v, (bf16_t*)a.o, a.ldq, a.ldk, a.ldv,
                                                   a.ldo, a.q_bstride, a.k_bstride, a.v_bstride, a.o_bstride, a.H, a.N, nqb,
                                                   a.scale * 1.4426950408889634f, nfull, 0, 1, 0, nullptr, T_items, 0, 0, a.seq_len);
    return 0;
  }
  if (const int rc = prepare_kernel<attn_w4_kernel<MODE>>(dv.dev, lds, "attention (attn_w4_kernel)", no_spills)) return rc;
  const int pgrid = dv.grid;     // workgroups of the persistent form: one per CU, a whole number per XCD
  // persistent form: one workgroup per CU over all (b, h, q-tile) items, when there are more items than CUs and no tail split
  int T_items = 0;
  if (sk_share > 0) {            // stream-K: one workgroup per CU, T_items = items of one sample, nfull = samples
    T_items = a.H * nqb;
    nfull = a.B;
    grid = (unsigned)pgrid;
  } else if (g_w4_persist && nsplit == 1 && (int)grid > pgrid) {
    T_items = (int)grid;
    grid = (unsigned)pgrid;
  }
  attn_w4_kernel<MODE><<<grid, 256, lds, st>>>((const bf16_t*)a.q, (const bf16_t*)a.k, (const bf16_t*)a.v, (bf16_t*)a.o, a.ldq,
                                                       a.ldk, a.ldv, a.ldo, a.q_bstride, a.k_bstride, a.v_bstride, a.o_bstride, a.H,
                                                       a.N, nqb, a.scale * 1.4426950408889634f, nfull, nparts, nsplit, xsplit, part, T_items, sk_group, sk_share);
  return 0;
}

// mode: 0 .. 4 = attn_w4_kernel<MODE> (tfx_set_option attention_waves 30 .. 34; 34 only when AttnArgs::score_bound allows it)
int joint_attention_w4(const AttnArgs& a, hipStream_t st, int mode) {
  const int nqb = (a.N + 255) / 256;
  const int T = a.B * a.H * nqb;
  // Tail split: T workgroups of equal length on C CUs take ceil(T / C) rounds, and when the last one is partly filled the chip
  // idles for the rest of it.  Cut the tiles of that last round -- the last m (head, q-tile) pairs of every sample, B m = the
  // tail rounded up to a multiple of B -- into two key ranges: the ordinary workgroups then fill whole rounds and the halves one
  // short one.  P1024 batch 8: 3456 workgroups = 13.5 rounds -> 3328 ordinary (13 rounds) + 256 halves: 1.861 -> 1.851 ms (a half
  // costs ~0.6 of a whole, and the rounds of a long kernel are not in step any more: the ideal 3.6 % shrinks to 0.5 %); batch 2:
  // 864 = 3.375 rounds -> 768 + 192 halves, 0.508 -> 0.481 ms.  Not
  // taken when a half would be shorter than 24 key tiles (its prologue, Q load and partial store cost more than the round
  // gains), without a full round in front, or when the last round is more than half full (the halves would need two rounds).
  int nfull = T, nsplit = 1, nparts = 0, xsplit = 0;
  float* part = nullptr;
  if (g_w4_split && !a.seq_len) {   // (per-sample lengths: whole items only)
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    const bool capturing = !(hipStreamIsCapturing(st, &cs) == hipSuccess && cs == hipStreamCaptureStatusNone);
    (void)hipGetLastError();
    if (const W4Scratch* sc = w4_scratch(st, !capturing)) {
      const int C = sc->cus, tail = T % C, nkv = (a.N + W4_KV - 1) / W4_KV;
      const int m = (tail + a.B - 1) / a.B;
      if (tail && T >= C && m * a.B * 2 <= C + 8 && nkv >= 48 && m < a.H * nqb && m * a.B * 2 <= W4_PART_TILES) {
        xsplit = m; nsplit = 2; nfull = T - m * a.B; nparts = m * a.B * 2; part = sc->part;
      }
    }
  }
  // Stream-K tail (see w4_sk_bound): per sample, the R items of the partly filled last round are dealt as (item, tile) units to the sample's
  // group of C / B CUs.  Estimate in 64-key tile times on the slowest CU: whole items cost ceil(Tp / group) (nkv + F); the dealt form
  // floor(Tp / group) (nkv + F) + share + (share / nkv + 1) F + M -- F = an item's prologue + output (tools/attn_item_timers.py: 6 - 9 tile
  // times), M = the partial stores, the merge pass (10 - 12 us) and the gap in front of it.  A piece count per item <= 8 (attn_w4_merge_sk_kernel) needs share >= nkv / 6.
  int sk_group = 0, sk_share = 0;
  const DeviceFacts dv = device_facts();
  const int pgrid = dv.grid;
  if (g_w4_streamk && g_w4_persist && nsplit == 1 && a.workspace && a.B <= pgrid && !a.seq_len) {
    const int C = pgrid, nkv = (a.N + W4_KV - 1) / W4_KV, Tp = a.H * nqb, group = C / a.B;
    const int full = (Tp / group) * group, R = Tp - full;
    const int share = R ? (R * nkv + group - 1) / group : 0;
    const int64_t need = (int64_t)2 * a.B * group * 256 * W4_PROW * (int64_t)sizeof(float);
    const float F = 7.f, M = 20.f;      // fitted to nine shapes (tools/attn_streamk_time.py, profiles/r06_attn_streamk.log): 0.65 F + M = 25 +- 10
    const float t_whole = (float)(full / group) * ((float)nkv + F);
    const float t_now = t_whole + (float)nkv + F, t_sk = t_whole + (float)share + ((float)share / (float)nkv + 1.f) * F + M;
    if (R > 0 && nkv >= 16 && share * 6 >= nkv && share >= 8 && need <= a.workspace_bytes && ((uintptr_t)a.workspace & 15) == 0 &&
        (g_w4_streamk >= 2 || t_sk < 0.99f * t_now)) {
      sk_group = group; sk_share = share; part = (float*)a.workspace;
    }
  }
  const unsigned grid = nsplit > 1 ? (unsigned)(((nfull + 7) & ~7) + nparts) : (unsigned)T;
#ifdef TFX_BENCH
  const int rc = mode == 4 ? w4_launch<4>(a, st, grid, dv, nqb, nfull, nparts, nsplit, xsplit, part, sk_group, sk_share)
               : mode == 3 ? w4_launch<3>(a, st, grid, dv, nqb, nfull, nparts, nsplit, xsplit, part, sk_group, sk_share)
               : mode == 2 ? w4_launch<2>(a, st, grid, dv, nqb, nfull, nparts, nsplit, xsplit, part, sk_group, sk_share)
               : mode == 1 ? w4_launch<1>(a, st, grid, dv, nqb, nfull, nparts, nsplit, xsplit, part, sk_group, sk_share)
                           : w4_launch<0>(a, st, grid, dv, nqb, nfull, nparts, nsplit, xsplit, part, sk_group, sk_share);
#else   // product library: the reference-free stream and the guarded form; modes 1 .. 3 are A/B builds (round 4), bench library only
  if (mode != 4 && mode != 0) return fail("attention: attn_w4_kernel<%d> is bench-only (libtextflux_hip_bench.so)", mode);
  const int rc = mode == 4 ? w4_launch<4>(a, st, grid, dv, nqb, nfull, nparts, nsplit, xsplit, part, sk_group, sk_share)
                           : w4_launch<0>(a, st, grid, dv, nqb, nfull, nparts, nsplit, xsplit, part, sk_group, sk_share);
#endif
  if (rc) return rc;
  if (sk_share > 0) attention_note_streamk();
  if (sk_share > 0)
    attn_w4_merge_sk_kernel<<<(unsigned)(a.B * sk_group * 8), 256, 0, st>>>(part, (bf16_t*)a.o, a.ldo, a.o_bstride, a.H, a.N, nqb, sk_group,
                                                                             sk_share, a.H * nqb);
  if (nsplit > 1)
    attn_w4_merge_kernel<<<(unsigned)(xsplit * a.B * 32), 256, 0, st>>>(part, (bf16_t*)a.o, a.ldo, a.o_bstride, a.H, a.N, nqb,
                                                                              xsplit, nsplit);
  return 0;
}

}  // namespace tfx
