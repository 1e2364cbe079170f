// The definition of the one-wave-per-SIMD attention kernel, included by attention_w4.hip once per form (not a header of its own: it
// relies on everything attention_w4.hip declares in front of the include):
//   W4_KERNEL_NAME attn_w4_kernel,  W4_VL 0: every batch sample has N rows -- the kernel as it always was;
//   W4_KERNEL_NAME attn_w4v_kernel, W4_VL 1: sample b has seq_len[b] <= N rows (tfx_attn_args.seq_len), one more kernel argument.
// Two textual instances instead of one template over VL behind two __global__ wrappers: inlining the body into a wrapper turns the
// kernel arguments' __restrict__ into scoped metadata and perturbs the register allocation and the schedule of this hand-placed
// instruction stream; as its own __global__ the uniform kernel compiles to the code it had before the second form existed.
// With VL an item works on its sample's first Nb = seq_len[b] rows exactly as an item of a launch with N = Nb would -- same key tiles in the same
// order, the ragged last tile masked through the descriptors sized to Nb rows, the same Q row clamp: the same bits --, rows >= Nb of O are
// not written, and items whose q-tile starts at or beyond Nb are skipped: the persistent walk steps over them both for its first item and
// for the NEXT item, so the prefetch chain (next Q rows, next first K / V tile) always targets the item that really runs next.  Whole
// items only: the host takes neither the stream-K dealing nor the tail split with VL.  Without VL every VL expression folds away.
template <int MODE>
__global__ __launch_bounds__(256, 1) void W4_KERNEL_NAME(const bf16_t* Q, const bf16_t* __restrict__ Kp,
                                                         const bf16_t* __restrict__ Vp, bf16_t* O, int64_t ldq, int64_t ldk,
                                                         int64_t ldv, int64_t ldo, int64_t q_bs, int64_t k_bs, int64_t v_bs,
                                                         int64_t o_bs, int H, int N, int nqb, float scale_log2e, int nfull,
                                                         int nparts, int nsplit, int xsplit, float* part, int T_items, int sk_group,
                                                         int sk_share W4_SEQ_LEN_PARAM) {
  constexpr bool VL = W4_VL != 0;
  W4_SEQ_LEN_NULL
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr bool LV = MODE == 1 || MODE == 2, LZ = MODE >= 2, NOREF = MODE == 4, FT = LV || NOREF;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hi = lane >> 5, l31 = lane & 31;
  int bid = blockIdx.x;
  // Tail split (nsplit > 1, joint_attention_w4): the LAST xsplit (head, q-tile) pairs of every batch sample are each cut into
  // nsplit KEY ranges and dispatched after the nfull ordinary workgroups -- nfull a whole number of rounds of the chip, so the last
  // round is made of short workgroups instead of being partly empty; such a workgroup leaves its un-normalised O, row sums and
  // reference maxima in `part`, attn_w4_merge_kernel finishes.  Which tiles are split depends on (head, q-tile) only, never on
  // the batch index: identical samples of a batch still produce identical bits; and the parts of one (batch, head) are neighbours
  // in the dispatch order, so its K / V stay L2-resident among them.  (Measured alternatives: the last q-tile of EVERY head --
  // re-streams all K / V from HBM at the end, no gain; whole heads -- nfull is no longer a multiple of the CU count, some CUs run
  // three halves in a row, 1.4 % slower than no split.)
  // PERSISTENT form (T_items > 0; round 4): one workgroup per CU walks its XCD's contiguous range of the T_items (b, h, q-tile)
  // items.  A fresh workgroup spends 12 k cycles (plus its dispatch) in front of its first tile -- two dependent memory round trips
  // for Q and the first K / V tiles; here the next item's Q rows and its first K / V tile are requested behind the current item's
  // tile loop and fly while its output is normalised, staged and stored: 6 k cycles (tools/attn_item_timers.py).
  int kpart = -1, ptile = 0, qblk, h, b;
  int item = 0, item_step = 0, item_end = 0;
  // stream-K: this CU's range [sk_lo, sk_hi) of its sample's TAIL units, the sample's first item, the CU's two partial slots, its unit list
  int sk_lo = 0, sk_hi = 0, sk_base = 0, sk_slot0 = 0, sk_u = 0, sk_nunits = 0, sk_nwhole = 0, sk_full = 0, sk_cu = 0, sk_tfirst = 0;
  const int nkv_all = (N + W4_KV - 1) / W4_KV;
  // unit u of this CU: (item, first tile, end tile) -- whole items first (stride = the group), then the pieces of its tail range
  auto sk_unit = [&](int u, int& it, int& ts, int& te) __attribute__((always_inline)) {
    if (u < sk_nwhole) {
      it = sk_base + sk_cu + u * sk_group; ts = 0; te = nkv_all;
    } else {
      const int ti = sk_tfirst + (u - sk_nwhole);
      it = sk_base + sk_full + ti; ts = max(sk_lo - ti * nkv_all, 0); te = min(sk_hi - ti * nkv_all, nkv_all);
    }
  };
  int ts = 0, te = nkv_all;      // this pass's key tiles [ts, te) of its item (stream-K; everything otherwise)
  if (sk_share > 0) {            // T_items = items of ONE sample, nfull = number of samples
    const int L = (bid & 7) * (gridDim.x >> 3) + (bid >> 3);            // CUs of one XCD are neighbours in a sample's group
    const int sample = L / sk_group;
    sk_cu = L - sample * sk_group;
    if (sample >= nfull) return;
    sk_full = (T_items / sk_group) * sk_group;
    sk_nwhole = sk_full / sk_group;
    const int total = (T_items - sk_full) * nkv_all;
    sk_lo = w4_sk_bound(sk_cu, sk_group, sk_share, nkv_all, total);
    sk_hi = w4_sk_bound(sk_cu + 1, sk_group, sk_share, nkv_all, total);
    sk_tfirst = sk_lo / nkv_all;
    sk_nunits = sk_nwhole + (sk_hi > sk_lo ? (sk_hi - 1) / nkv_all - sk_tfirst + 1 : 0);
    if (sk_nunits == 0) return;
    sk_base = sample * T_items;
    sk_slot0 = 2 * L;
    sk_unit(0, item, ts, te);
    qblk = item % nqb;
    h = (item / nqb) % H;
    b = item / (nqb * H);
  } else if (T_items > 0) {
    const int nwg = gridDim.x, q = T_items >> 3, r = T_items & 7, xcd = bid & 7, slot = bid >> 3;
    const int xs = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q, xc = q + (xcd < r ? 1 : 0);
    if (slot >= xc) return;
    item = xs + slot;
    item_step = nwg >> 3;
    item_end = xs + xc;
    if constexpr (VL) {          // this CU's first item that has rows
      for (; item < item_end; item += item_step)
        if ((item % nqb) * 256 < w4_len(seq_len, item / (nqb * H), N)) break;
      if (item >= item_end) return;
    }
    qblk = item % nqb;
    h = (item / nqb) % H;
    b = item / (nqb * H);
  } else if (nsplit > 1) {
    const int fpad = (nfull + 7) & ~7, pf = H * nqb - xsplit;      // pf: unsplit pairs per sample
    int pair;
    if (bid < fpad) {
      const int q = nfull >> 3, r = nfull & 7, xcd = bid & 7, k = bid >> 3;
      if (k >= q + (xcd < r ? 1 : 0)) return;
      const int fid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + k;
      b = fid / pf;
      pair = fid % pf;
    } else {
      const int pi = bid - fpad;
      if (pi >= nparts) return;
      kpart = pi % nsplit;
      ptile = pi / nsplit;
      b = ptile / xsplit;
      pair = pf + ptile % xsplit;
    }
    h = pair / nqb;
    qblk = pair % nqb;
  } else {
    const int nwg = gridDim.x, q = nwg >> 3, r = nwg & 7, xcd = bid & 7, k = bid >> 3;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + k;
    qblk = bid % nqb;
    bid /= nqb;
    h = bid % H;
    b = bid / H;
    if constexpr (VL) {
      if (qblk * 256 >= w4_len(seq_len, b, N)) return;
    }
  }
  bf16x8 qn[2][8];               // persistent form: the NEXT item's Q rows (raw), requested behind this item's tile loop
  bool have_pref = false;        // ... and whether qn / kreg / vreg hold this item's Q rows / first K, V tile already
  u32x4 kreg[4], vreg[4];        // staging registers: thread t moves the 16-byte chunks (row t / 16 + 16 i, chunk t % 16), i = 0..3, of a tile's K and V
#ifdef TFX_BENCH
  unsigned long long w4_stamp[4] = {0, 0, 0, 0}, w4_sum[4] = {0, 0, 0, 0};
#endif
  for (;;) {                     // one pass per item (exactly one in the non-persistent form)
  W4_STAMP(0);
  bool has_next = item + item_step < item_end;            // (false in the non-persistent form: all three are 0)
  int item2 = item + item_step, ts2 = 0;
  int Nb = N, Nb2 = N;           // rows of this item's / the next item's batch sample (VL: its own length)
  if constexpr (VL) {
    Nb = w4_len(seq_len, b, N);
    for (; item2 < item_end; item2 += item_step) {          // the next item that has rows
      Nb2 = w4_len(seq_len, item2 / (nqb * H), N);
      if ((item2 % nqb) * 256 < Nb2) break;
    }
    has_next = item2 < item_end;
  }
  if (sk_share > 0) {
    int te2;
    has_next = sk_u + 1 < sk_nunits;
    if (has_next) sk_unit(sk_u + 1, item2, ts2, te2);
  }
  const int qblk2 = item2 % nqb, h2 = (item2 / nqb) % H, b2 = item2 / (nqb * H);
  const bf16_t* Qb = Q + b * q_bs + h * W4_HD;
  const bf16_t* Kb = Kp + b * k_bs + h * W4_HD;   // (advanced to the first key of a split range below)
  const bf16_t* Vb = Vp + b * v_bs + h * W4_HD;
  bf16_t* Ob = O + b * o_bs + h * W4_HD;
  // keys of this workgroup: all N, or (tail split) the 64-key tiles [kpart, kpart + 1) * nkv / nsplit
  int Nk = Nb;
  if (kpart >= 0) {
    const int nkv_all = (N + W4_KV - 1) / W4_KV;
    const int t0 = kpart * nkv_all / nsplit, t1 = (kpart + 1) * nkv_all / nsplit;
    Nk = min(N, t1 * W4_KV) - t0 * W4_KV;
    Kb += (int64_t)t0 * W4_KV * ldk;
    Vb += (int64_t)t0 * W4_KV * ldv;
  }
  int pslot = -1;                // stream-K: >= 0 when this pass covers only a part of its item's keys (its partial slot)
  if (sk_share > 0) {
    if (ts > 0) pslot = sk_slot0;
    else if (te < nkv_all) pslot = sk_slot0 + 1;
    Nk = min(N, te * W4_KV) - ts * W4_KV;
    Kb += (int64_t)ts * W4_KV * ldk;
    Vb += (int64_t)ts * W4_KV * ldv;
  }

  // ---- Q fragments of the wave's two q-blocks, pre-scaled into the exp2 domain (one extra bf16 rounding of q).  All sixteen
  // requests go out before the first conversion: with one wave per SIMD a request-wait-convert loop would pay sixteen memory
  // round trips per workgroup
  int qrow[2];
  bf16x8 qf[2][8];
#pragma unroll
  for (int qb = 0; qb < 2; ++qb) {
    qrow[qb] = qblk * 256 + wave * 64 + qb * 32 + l31;
    const int rc = qrow[qb] < Nb ? qrow[qb] : Nb - 1;
    if (have_pref) {
#pragma unroll
      for (int s = 0; s < 8; ++s) qf[qb][s] = qn[qb][s];
    } else {
#pragma unroll
      for (int s = 0; s < 8; ++s) qf[qb][s] = *reinterpret_cast<const bf16x8*>(Qb + (int64_t)rc * ldq + s * 16 + hi * 8);
    }
  }
  // the next item's Q rows -> qn (requested behind the tile loop)
  auto load_qn = [&]() __attribute__((always_inline)) {
    const bf16_t* Qb2 = Q + b2 * q_bs + h2 * W4_HD;
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
      const int r2 = qblk2 * 256 + wave * 64 + qb * 32 + l31;
      const int rc = r2 < Nb2 ? r2 : Nb2 - 1;
#pragma unroll
      for (int s = 0; s < 8; ++s) qn[qb][s] = *reinterpret_cast<const bf16x8*>(Qb2 + (int64_t)rc * ldq + s * 16 + hi * 8);
    }
  };
  __builtin_amdgcn_sched_barrier(0);
  auto convert_q = [&]() __attribute__((always_inline)) {
    if constexpr (W4_ABL & 1024) {
      // timing ablation (round 6): what the Q-side per-head RMSNorm + RoPE would cost HERE, in the Q prologue,
      // if the projection GEMM's epilogue left q un-normalised -- the real instruction mix on the real registers (sum of squares by
      // v_dot2c on the packed pairs, the two halves of a row meeting by v_permlane32_swap, x / rms -> bf16 -> * weight by v_dot2 -> bf16 ->
      // rotation -> bf16, then the existing pre-scale), with opaque stand-ins for the weight / table VALUES: the 32 float4 table loads per
      // lane and item are NOT issued, so the price measured is a lower bound
      float cc = scale_log2e, sn = scale_log2e * 0.5f;
      uint32_t wlo = 0x3f80u, whi = 0x3f800000u;
      asm volatile("" : "+v"(cc), "+v"(sn), "+v"(wlo), "+v"(whi));
#pragma unroll
      for (int qb = 0; qb < 2; ++qb) {
        float ss = 0.f;
#pragma unroll
        for (int s = 0; s < 8; ++s) {
          const u32x4 pk = __builtin_bit_cast(u32x4, qf[qb][s]);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const uint32_t pi = pk[i];
            ss = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf2_t, pi), __builtin_bit_cast(bf2_t, pi), ss, false);
          }
        }
        const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(ss), __float_as_uint(ss), false, false);
        const float rinv = rsqrtf((__uint_as_float(sw[0]) + __uint_as_float(sw[1])) * (1.0f / 128.0f) + 1e-6f);
#pragma unroll
        for (int s = 0; s < 8; ++s) {
          u32x4 pk = __builtin_bit_cast(u32x4, qf[qb][s]);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const uint32_t a = pack_bf2(__uint_as_float(pk[i] << 16) * rinv, __uint_as_float(pk[i] & 0xffff0000u) * rinv);
            float y0, y1;
            y0 = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf2_t, a), __builtin_bit_cast(bf2_t, wlo), 0.0f, false);
            y1 = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf2_t, a), __builtin_bit_cast(bf2_t, whi), 0.0f, false);
            const uint32_t yp = pack_bf2(y0, y1);
            y0 = __uint_as_float(yp << 16);
            y1 = __uint_as_float(yp & 0xffff0000u);
            pk[i] = pack_bf2(y0 * cc + (-y1) * sn, y1 * cc + y0 * sn);
          }
          qf[qb][s] = __builtin_bit_cast(bf16x8, pk);
        }
      }
    }
#pragma unroll
    for (int qb = 0; qb < 2; ++qb)
#pragma unroll
      for (int s = 0; s < 8; ++s) {
#pragma unroll
        for (int e = 0; e < 8; ++e) qf[qb][s][e] = (__bf16)((float)qf[qb][s][e] * scale_log2e);
        asm volatile("" : "+a"(qf[qb][s]));   // home of the Q fragments: the AccVGPRs (srcB of the score MFMAs reads them there)
      }
  };

  const int nkv = (Nk + W4_KV - 1) / W4_KV;
  // ---- staging (kreg / vreg, declared in front of the item loop)
  // buffer descriptors sized to this head's N valid rows: a request past them (the rows of a ragged last tile, whole tiles
  // requested past the end of the sequence) returns zeros and moves nothing -- the scores of such keys are masked anyway,
  // and their zero V rows meet zero weights.  (The range check covers VGPR + SGPR offset: tools/ubench/buffer_range.hip.)
  const int ldk2 = (int)ldk * 2, ldv2 = (int)ldv * 2;
  const auto rsK = __builtin_amdgcn_make_buffer_rsrc((void*)Kb, 0, (int)((uint32_t)(Nk - 1) * (uint32_t)ldk2 + 256u), 0x00020000);
  const auto rsV = __builtin_amdgcn_make_buffer_rsrc((void*)Vb, 0, (int)((uint32_t)(Nk - 1) * (uint32_t)ldv2 + 256u), 0x00020000);
  // the next item's K / V (persistent form; its first tile is requested after this item's output stores -- load_tile(0) below -- and flies under the next prologue)
  // (stream-K: the next pass may start at tile ts2 of its item -- the first piece of this CU's tail range)
  const auto rsK2 = __builtin_amdgcn_make_buffer_rsrc((void*)(Kp + b2 * k_bs + h2 * W4_HD + (int64_t)ts2 * W4_KV * ldk), 0,
                                                      (int)((uint32_t)(Nb2 - 1 - ts2 * W4_KV) * (uint32_t)ldk2 + 256u), 0x00020000);
  const auto rsV2 = __builtin_amdgcn_make_buffer_rsrc((void*)(Vp + b2 * v_bs + h2 * W4_HD + (int64_t)ts2 * W4_KV * ldv), 0,
                                                      (int)((uint32_t)(Nb2 - 1 - ts2 * W4_KV) * (uint32_t)ldv2 + 256u), 0x00020000);
  // piece i (rows t / 16 + 16 i) of tile j: global -> registers.  Rows are clamped to the last valid key (a no-op on full
  // tiles), tiles to the last tile (the pipeline requests up to two tiles past the end; nobody reads those buffers)
  // tile j: global -> registers, piece i = rows t / 16 + 16 i.  Full tiles: one per-lane offset (rebuilt per burst: as a loop
  // invariant it would pin two registers) and the piece in the scalar offset; the last tile of a ragged N clamps its rows
  // piece i (rows t / 16 + 16 i) of tile j, K or V side: global -> registers.  ko / vo: per-lane byte offset of (row t / 16,
  // chunk t % 16); the tile and the piece go into the scalar offset
  // requests go through rsKs / rsVs: this item's descriptors, except in the last tile of the persistent form, whose staging step
  // requests the NEXT item's first tile (set once per tile: a select per request costs 32 scalar instructions per tile, 3.5 %)
  auto rsKs = rsK, rsVs = rsV;
  auto load_piece = [&](int j, int ko, int vo, auto Ic, bool k_side) __attribute__((always_inline)) {
    constexpr int i = decltype(Ic)::value;
    if (W4_ABL & 32) j = 0;          // timing ablation: every request hits the same (cache-resident) tile
    if constexpr (W4_ABL & 256) {    // timing ablation: the request as LDS-DMA into a scratch region behind the ring (what would a DMA-staged kernel pay?)
      typedef __attribute__((address_space(3))) void lds_void_;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(k_side ? rsKs : rsVs, (lds_void_*)(smem + ATT_LDS_W4 + (tid >> 6) * 1024), 16, k_side ? ko : vo,
                                               (j * W4_KV + 16 * i) * (k_side ? ldk2 : ldv2), 0, 0);
      return;
    }
    if (k_side)
      kreg[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rsKs, ko, (j * W4_KV + 16 * i) * ldk2, 0));
    else
      vreg[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rsVs, vo, (j * W4_KV + 16 * i) * ldv2, 0));
  };
  auto stage_offsets = [&](int& ko, int& vo) __attribute__((always_inline)) {
    int te = tid;
    asm volatile("" : "+v"(te));     // rebuilt where needed: as loop invariants the offsets would pin two registers
    ko = (int)__umul24(te >> 4, ldk2) + (te & 15) * 16;
    vo = (int)__umul24(te >> 4, ldv2) + (te & 15) * 16;
  };
  auto load_tile = [&](int j) __attribute__((always_inline)) {
    int ko, vo;
    stage_offsets(ko, vo);
    load_piece(j, ko, vo, IC<0>{}, true); load_piece(j, ko, vo, IC<0>{}, false); load_piece(j, ko, vo, IC<1>{}, true); load_piece(j, ko, vo, IC<1>{}, false);
    load_piece(j, ko, vo, IC<2>{}, true); load_piece(j, ko, vo, IC<2>{}, false); load_piece(j, ko, vo, IC<3>{}, true); load_piece(j, ko, vo, IC<3>{}, false);
  };
  auto write_piece = [&](int buf, auto Ic, bool k_side) __attribute__((always_inline)) {
    constexpr int i = decltype(Ic)::value;
    const int kr = tid >> 4, ch = tid & 15;
    if (k_side)
      *reinterpret_cast<u32x4*>(smem + W4_KBASE + buf * W4_KT + kr * W4_KROW + ch * 16 + i * 16 * W4_KROW) = kreg[i];
    else
      *reinterpret_cast<u32x4*>(smem + buf * W4_VT + kr * 256 + ((((ch >> 2) ^ (kr & 3)) << 6) | ((ch & 3) << 4)) + i * 16 * 256) = vreg[i];
  };
  auto write_tile = [&](int buf) __attribute__((always_inline)) {
    write_piece(buf, IC<0>{}, true); write_piece(buf, IC<0>{}, false); write_piece(buf, IC<1>{}, true); write_piece(buf, IC<1>{}, false);
    write_piece(buf, IC<2>{}, true); write_piece(buf, IC<2>{}, false); write_piece(buf, IC<3>{}, true); write_piece(buf, IC<3>{}, false);
  };
  // ---- fragment read addresses: one per-lane base for K, four (d blocks) for the V transpose reads, + immediates
  const char* rK = smem + W4_KBASE + l31 * W4_KROW + hi * 16;
  const int vi = lane & 15;
  const char* rV[4];
#pragma unroll
  for (int db = 0; db < 4; ++db)
    rV[db] = smem + (4 * hi + (vi >> 2)) * 256 + 32 * ((lane >> 4) & 1) + (vi & 3) * 8 + ((db ^ ((vi >> 2) & 3)) << 6);
  // koff: byte offset of (buffer, key block) inside the K region; voff: of (buffer, first 16-key step) inside the V region
  auto kread = [&](int koff, int s) __attribute__((always_inline)) -> bf16x8 {
    return *reinterpret_cast<const bf16x8*>(rK + koff + s * 32);
  };
  auto vread = [&](int voff, int ks, int db) __attribute__((always_inline)) -> bf16x8 {
    const char* va = rV[db] + voff + ks * 16 * 256;
    if constexpr (W4_ABL & 512) return *reinterpret_cast<const bf16x8*>(rK + voff + ks * 16 * 256 + db * 64);   // timing ablation: what a V^T tile would cost to read (one b128, K's conflict-free pattern)
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(va));
    const s16x4 hi4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(va + 8 * 256));
    return __builtin_bit_cast(bf16x8, (s16x8)__builtin_shufflevector(lo, hi4, 0, 1, 2, 3, 4, 5, 6, 7));
  };

  f32x16 o[2][4], ol[2], sc[2];
#pragma unroll
  for (int qb = 0; qb < 2; ++qb)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      ol[qb][r] = 0.f;
#pragma unroll
      for (int db = 0; db < 4; ++db) o[qb][db][r] = 0.f;
    }
  bf16x8 kone, vone, qm[2], kf[8], vf[2][4];
  u32x4 pf[2][2];                // bf16 weights of the pending / the current unit, per q-block and 16-key step
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    kone[e] = (__bf16)0.f;
    vone[e] = (__bf16)1.0f;
    qm[0][e] = qm[1][e] = (__bf16)0.f;
  }
  if (hi == 0) kone[0] = (__bf16)1.0f;
  asm volatile("" : "+a"(kone), "+a"(vone));   // constants of the bookkeeping MFMAs: AccVGPR residents, not re-materialised
  float m_ref[2] = {0.f, 0.f};   // bf16-exact lazy reference maximum per q-block row (exp2 domain); -m_ref sits in qm[.][0]
  float lsum[2] = {0.f, 0.f};    // LV: this lane's share (16 of every 32 keys) of the row sums; the halves meet at the end
  bool any_ref = false;          // LZ: some row of this wave has a non-zero reference (wave-uniform): the offset MFMA is needed

#ifdef W4_DEBUG_CLEAR_LDS
  for (int i = tid * 16; i < ATT_LDS_W4; i += 256 * 16) *reinterpret_cast<u32x4*>(smem + i) = u32x4{0, 0, 0, 0};
  __syncthreads();
#endif
  // ---- prologue: tiles 0 and 1 in LDS, tile 2 requested; K fragments of (tile 0, key block 0); S(0)
  // Tiles 0 AND 1 are requested together (tile 1 into the sixteen registers of the K / V fragments, idle until the first
  // fragment read) and the Q conversion runs under their flight: one memory round trip in front of the first MFMA, not three
  if (!have_pref) load_tile(0);                   // (persistent form, later items: requested inside the previous item's last tile)
  u32x4 k1[4], v1[4];
  {
    int ko, vo;
    stage_offsets(ko, vo);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      k1[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rsK, ko, (W4_KV + 16 * i) * ldk2, 0));
      v1[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rsV, vo, (W4_KV + 16 * i) * ldv2, 0));
    }
  }
  __builtin_amdgcn_sched_barrier(0);
  convert_q();
  __builtin_amdgcn_sched_barrier(0);
  write_tile(0);
  load_tile(2);
  {
    const int kr = tid >> 4, ch = tid & 15;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      *reinterpret_cast<u32x4*>(smem + W4_KBASE + W4_KT + kr * W4_KROW + ch * 16 + i * 16 * W4_KROW) = k1[i];
      *reinterpret_cast<u32x4*>(smem + W4_VT + kr * 256 + ((((ch >> 2) ^ (kr & 3)) << 6) | ((ch & 3) << 4)) + i * 16 * 256) = v1[i];
    }
  }
  __syncthreads();
#pragma unroll
  for (int s = 0; s < 8; ++s) kf[s] = kread(0, s);
  W4_GAP();
  if constexpr (LZ) {
    w4_mfma_s0(sc[0], kf[0], qf[0][0]);           // every reference is 0 at the start: the chain starts from a zero C operand
#pragma unroll
    for (int s = 1; s < 8; ++s) w4_mfma_s(sc[0], kf[s], qf[0][s]);
  } else {
    w4_mfma_s0(sc[0], kone, qm[0]);               // reference 0: a zero product, starts the accumulate chain
#pragma unroll
    for (int s = 0; s < 8; ++s) w4_mfma_s(sc[0], kf[s], qf[0][s]);
  }
  // The first read of these scores is the first step's W4_TOUCH (compiler-visible), in front of which hipcc pads for the chain's last
  // MFMA; dependent MFMAs are interlocked among themselves.  Rounds 2-3 put 24 x `s_nop 15` here and before the output (from the time
  // when every read was inline asm with no visible one in front): dead time twice per item, removed in round 4 (-DW4_KEEP_DRAINS restores
  // them; tools/check_mfma_hazard.py and the determinism tests are the net).
#ifdef W4_KEEP_DRAINS
  W4_DRAIN_MFMA();
#endif
  W4_GAP();

  // One pipeline step = unit u of q-block QB (u & 1).
  //   VALU : softmax of S(u) (sc[QB]) -> P(u) (pf[QB]);  rarely: move q-block QB's reference
  //   MFMA : S(u+1) of the OTHER q-block (sc[OQ]) from the K fragments in kf;  pending P(u-1).V of the other q-block (pf[OQ], vf)
  //   EVEN : (QB == 0) last user of kf / vf -> each register is reloaded right after its use: kf <- K rows at KN, vf <- V rows at VN
  //   FIRST: the q-block's first unit pins the reference to the true row maximum
  //   rag  : this unit's key block reaches past N (last tile only): keys >= N are masked; kb_abs = its first key
  //   STG  : staging spread over this step's MFMA gaps: 1 = tile jst -> LDS buffer (STG >> 2) from the registers, 2 = request tile jst
  auto step = [&](auto QBc, auto PVc, auto FIRSTc, auto KNc, auto VNc, auto STGc, int jst, bool rag, int kb_abs) __attribute__((always_inline)) {
    constexpr int QB = decltype(QBc)::value, OQ = 1 - QB;
    constexpr bool EVEN = QB == 0, PV = decltype(PVc)::value != 0, FIRST = decltype(FIRSTc)::value != 0;
    constexpr int KN = decltype(KNc)::value, VN = decltype(VNc)::value, STG = decltype(STGc)::value;
    f32x16& cur = sc[QB];
    f32x16& nxt = sc[OQ];
    if (__builtin_expect_with_probability(rag, 0, 1.0)) {
      int kbase = kb_abs + 4 * hi;
      asm volatile("" : "+v"(kbase));     // keep the index arithmetic inside the (last-tile-only) branch
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (kbase + (r & 3) + 8 * (r >> 2) >= Nk) cur[r] = -INFINITY;
    }
    // MFMA i of the S chain (0: the reference offset, 1..8: the head-dim steps) and of the pending P.V (ks = i / 5, block i % 5)
    auto S = [&](auto Ic) __attribute__((always_inline)) {
      constexpr int i = decltype(Ic)::value;
      if constexpr (i == 0) {
        w4_mfma_s0(nxt, kone, qm[OQ]);
      } else if constexpr (i == 1 && LZ) {
        // the chain starts here; the reference offset joins it (one more MFMA, out of line) only while some row of this wave has one
        w4_mfma_s0(nxt, kf[0], qf[OQ][0]);
        if constexpr (!NOREF) {
          if (__builtin_expect_with_probability(any_ref, 0, 1.0)) w4_mfma_s(nxt, kone, qm[OQ]);
        }
      } else {
        w4_mfma_s(nxt, kf[i - 1], qf[OQ][i - 1]);
        // reloaded two MFMAs after its last reader: spreads the LDS reads over the regions
        if constexpr (EVEN && i >= 2 && !(W4_ABL & 2)) kf[i - 2] = kread(KN, i - 2);
      }
    };
    // LV: eight P.V MFMAs (ks = i / 4, d block i % 4), no row-sum MFMA; each V fragment is reloaded one MFMA after its use, the last
    // one and kf[7] by RL() behind the step's last MFMA
    auto PL = [&](auto Ic) __attribute__((always_inline)) {
      constexpr int i = decltype(Ic)::value, ks = i / 4, db = i % 4;
      if constexpr (PV) w4_mfma_o(o[OQ][db], vf[ks][db], pf[OQ][ks]);
      if constexpr (EVEN && i >= 1 && !(W4_ABL & 2)) vf[(i - 1) / 4][(i - 1) % 4] = vread(VN, (i - 1) / 4, (i - 1) % 4);
    };
    auto RL = [&]() __attribute__((always_inline)) {
      if constexpr (EVEN && !(W4_ABL & 2)) {
        vf[1][3] = vread(VN, 1, 3);
        kf[7] = kread(KN, 7);
      }
    };
    // LV: row sums of the PENDING unit (other q-block, weights pf[OQ] finished last step) -- one v_dot2c_f32_bf16 per packed pair
    auto DL = [&](auto Ic) __attribute__((always_inline)) {
      constexpr int c = decltype(Ic)::value;
      if constexpr (PV && !(W4_ABL & 1)) w4_dot2c(lsum[OQ], pf[OQ][c >> 2][c & 3]);
    };
    auto P = [&](auto Ic) __attribute__((always_inline)) {
      constexpr int i = decltype(Ic)::value, ks = i / 5, db = i % 5;
      if constexpr (PV) {
        if constexpr (db == 4) {
          w4_mfma_l(ol[OQ], vone, pf[OQ][ks]);
        } else {
          w4_mfma_o(o[OQ][db], vf[ks][db], pf[OQ][ks]);
        }
      }
      if constexpr (EVEN && i >= 1 && (i - 1) % 5 < 4 && !(W4_ABL & 2)) vf[(i - 1) / 5][(i - 1) % 5] = vread(VN, (i - 1) / 5, (i - 1) % 5);
      if constexpr (EVEN && i == 9 && !(W4_ABL & 2)) kf[7] = kread(KN, 7);
    };
    // VALU stream of the exponentials, one instruction per call, in an order in which every bf16 pack follows its two
    // v_exp_f32 by at least two instructions (a transcendental result needs one instruction before a VALU reads it, and the asm
    // pack is invisible to hipcc's hazard pass):  e0 e1 e2 c0 e3 e4 c1 e5 e6 c2 ... e13 e14 c6 e15 c7
    auto F = [&](auto Ic) __attribute__((always_inline)) {
      constexpr int k = decltype(Ic)::value;
      if constexpr (W4_ABL & 1) return;
      // LV modes and MODE 4 end  e13 e14 e15 c6 c7  (no MFMA region separates the last pack from its exponentials there)
      constexpr bool is_c = FT ? (k >= 22 || (k >= 3 && k <= 18 && k % 3 == 0)) : ((k == 23) || (k >= 3 && k < 22 && k % 3 == 0));
      if constexpr (is_c) {
        constexpr int c = FT ? (k >= 22 ? k - 16 : k / 3 - 1) : (k == 23 ? 7 : k / 3 - 1);
        pf[QB][c >> 2][c & 3] = w4_cvt_pk(cur[2 * c], cur[2 * c + 1]);
      } else {
        constexpr int e = FT ? (k < 3 ? k : k >= 19 ? k - 6 : k - (k / 3))
                             : (k < 3 ? k : k == 22 ? 15 : k - (k / 3));      // exponentials seen so far = index minus packs before it
        cur[e] = __builtin_amdgcn_exp2f(cur[e]);
      }
    };
    // staging stream of the step that moves tile jst - 1 from the registers into LDS buffer STG >> 2 and refills every register
    // with its piece of tile jst right behind:  W0 W1 L0 W2 L1 W3 L2 ... W7 L6 L7  (piece g = K / V chunk g / 2, K first)
    int stg_ko = 0, stg_vo = 0;
    if constexpr ((STG & 3) == 1 && !(W4_ABL & 4)) stage_offsets(stg_ko, stg_vo);
    auto G = [&](auto Ic) __attribute__((always_inline)) {
      constexpr int n = decltype(Ic)::value;            // 0..15
      if constexpr ((STG & 3) == 1 && !(W4_ABL & 4)) {
        constexpr bool is_w = n == 0 || n == 1 || (n < 15 && (n & 1));   // W0 W1 | L0 W2 L1 W3 ... L5 W7 | L6 L7
        constexpr int g = n < 2 ? n : is_w ? (n + 1) / 2 : n == 15 ? 7 : n / 2 - 1;
        if constexpr (is_w) { if constexpr (!(W4_ABL & 64)) write_piece(STG >> 2, IC<g / 2>{}, (g & 1) == 0); }
        else { if constexpr (!(W4_ABL & 128)) load_piece(jst, stg_ko, stg_vo, IC<g / 2>{}, (g & 1) == 0); }
      }
    };
    // One MFMA per scheduling region, each with <= ~24 issue cycles of other work behind it (an MFMA that finds the pipe busy
    // blocks the wave's issue until the pipe takes it, so work behind TWO adjacent MFMAs is not hidden by the first).
    // The score chain runs one MFMA ahead of the P.V group: its last MFMA S(8) is followed by three more MFMAs of this step
    // and the first of the next before anything reads the scores -- an MFMA result needs ~11 issued instructions before a
    // VALU read, and hipcc cannot insert that wait in front of the inline-asm maxima (it does not know they are VALU).
    float mx = 0.f;
    // the four pieces of the row maximum (VALU, inline asm) and the rare reference move, shared by the three region lists below
    auto MX = [&](auto Ic) __attribute__((always_inline)) {
      constexpr int i = decltype(Ic)::value;
      if constexpr (W4_ABL & 8) return;
      if constexpr (i == 0) mx = w4_max7(cur[0], cur[1], cur[2], cur[3], cur[4], cur[5], cur[6]);
      if constexpr (i == 1) mx = w4_max7(mx, cur[7], cur[8], cur[9], cur[10], cur[11], cur[12]);
      if constexpr (i == 2) mx = w4_max4(mx, cur[13], cur[14], cur[15]);
      if constexpr (i == 3) {
        const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(mx), __float_as_uint(mx), false, false);
        mx = w4_max(__uint_as_float(sw[0]), __uint_as_float(sw[1]));   // both 32-key halves of the row
      }
    };
    auto MOVE = [&]() __attribute__((always_inline)) {
      // out of line: with one wave per SIMD nothing hides the instruction-fetch bubble of a TAKEN branch, so the common
      // path must be the fall-through
      bool take;
      if constexpr (LZ) take = !(W4_ABL & 8) && !__all(FIRST ? fabsf(mx) <= W4_BIG : mx <= W4_BIG);
      else take = FIRST || (!(W4_ABL & 8) && !__all(mx <= W4_THR));
      if (__builtin_expect_with_probability(take, FIRST && !LZ, 1.0)) {
        // move the reference: everything q-block QB accumulated against the old one is rescaled exactly once (no MFMA on
        // o[QB] / ol[QB] is in this step's stream), the scores of this unit are shifted before they are exponentiated
        float m_new;
        if constexpr (LZ) {   // only the rows that need it: a first tile's maximum outside +-W4_BIG pins, a later excess beyond W4_BIG moves
          const bool mv = FIRST ? fabsf(mx) > W4_BIG : mx > W4_BIG;
          m_new = mv ? round_bf(m_ref[QB] + mx) : m_ref[QB];
        } else {
          m_new = round_bf(m_ref[QB] + (FIRST ? mx : fmaxf(mx, 0.f)));
        }
        const float d = m_new - m_ref[QB];
        m_ref[QB] = m_new;
        qm[QB][0] = (__bf16)(hi == 0 ? -m_new : 0.f);
        if constexpr (LZ) any_ref = __any(m_ref[0] != 0.f || m_ref[1] != 0.f);
#pragma unroll
        for (int r = 0; r < 16; ++r) cur[r] -= d;
        if constexpr (!FIRST) {
          const float f = __builtin_amdgcn_exp2f(-d);
          if constexpr (LV) lsum[QB] *= f;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            if constexpr (!LV) ol[QB][r] *= f;
#pragma unroll
            for (int db = 0; db < 4; ++db) o[QB][db][r] *= f;
          }
        }
      }
    };
    if constexpr (MODE == 0) {
    S(IC<0>{});
    W4_TOUCH(cur);
    MX(IC<0>{});
    W4_GAP();
    S(IC<1>{});
    MX(IC<1>{});
    W4_GAP();
    P(IC<0>{});
    MX(IC<2>{});
    W4_GAP();
    S(IC<2>{});
    MX(IC<3>{});
    W4_GAP();
    P(IC<1>{});
    W4_GAP();
    MOVE();
    W4_GAP();
    S(IC<3>{}); F(IC<0>{}); F(IC<1>{}); G(IC<0>{});
    W4_GAP();
    P(IC<2>{}); F(IC<2>{}); F(IC<3>{}); G(IC<1>{});
    W4_GAP();
    S(IC<4>{}); F(IC<4>{}); F(IC<5>{}); G(IC<2>{});
    W4_GAP();
    P(IC<3>{}); F(IC<6>{}); F(IC<7>{}); G(IC<3>{});
    W4_GAP();
    S(IC<5>{}); F(IC<8>{}); F(IC<9>{}); G(IC<4>{});
    W4_GAP();
    P(IC<4>{}); F(IC<10>{}); F(IC<11>{}); G(IC<5>{});
    W4_GAP();
    S(IC<6>{}); F(IC<12>{}); F(IC<13>{}); G(IC<6>{});
    W4_GAP();
    P(IC<5>{}); F(IC<14>{}); F(IC<15>{}); G(IC<7>{});
    W4_GAP();
    S(IC<7>{}); F(IC<16>{}); F(IC<17>{}); G(IC<8>{});
    W4_GAP();
    P(IC<6>{}); F(IC<18>{}); F(IC<19>{}); G(IC<9>{});
    W4_GAP();
    S(IC<8>{}); F(IC<20>{}); F(IC<21>{}); G(IC<10>{});
#ifdef W4_HAZARD_SELFTEST   // a score read from inline asm two instructions behind its chain's last MFMA: what check_mfma_hazard.py must catch
    { const float t_ = w4_max(nxt[0], nxt[1]); asm volatile("" ::"v"(t_)); }
#endif
    W4_GAP();
    P(IC<7>{}); F(IC<22>{}); G(IC<11>{});
    W4_GAP();
    P(IC<8>{}); G(IC<12>{}); G(IC<13>{});
    W4_GAP();
    P(IC<9>{}); G(IC<14>{}); G(IC<15>{});
    W4_GAP();
    F(IC<23>{});
    W4_GAP();
    } else if constexpr (MODE == 1) {
    // 17 MFMAs: S0..S8 interleaved with the eight P.V; the pending unit's row sums (DL) ride behind the first five, the staging
    // stream (G, one step in four) one piece per region
    S(IC<0>{}); W4_TOUCH(cur); MX(IC<0>{}); G(IC<0>{});
    W4_GAP();
    S(IC<1>{}); MX(IC<1>{}); DL(IC<0>{}); G(IC<1>{});
    W4_GAP();
    PL(IC<0>{}); MX(IC<2>{}); DL(IC<1>{}); DL(IC<2>{}); G(IC<2>{});
    W4_GAP();
    S(IC<2>{}); MX(IC<3>{}); DL(IC<3>{}); DL(IC<4>{}); G(IC<3>{});
    W4_GAP();
    PL(IC<1>{}); DL(IC<5>{}); DL(IC<6>{}); DL(IC<7>{}); G(IC<4>{});
    W4_GAP();
    MOVE();
    W4_GAP();
    S(IC<3>{}); F(IC<0>{}); F(IC<1>{}); G(IC<5>{});
    W4_GAP();
    PL(IC<2>{}); F(IC<2>{}); F(IC<3>{}); G(IC<6>{});
    W4_GAP();
    S(IC<4>{}); F(IC<4>{}); F(IC<5>{}); G(IC<7>{});
    W4_GAP();
    PL(IC<3>{}); F(IC<6>{}); F(IC<7>{}); G(IC<8>{});
    W4_GAP();
    S(IC<5>{}); F(IC<8>{}); F(IC<9>{}); G(IC<9>{});
    W4_GAP();
    PL(IC<4>{}); F(IC<10>{}); F(IC<11>{}); G(IC<10>{});
    W4_GAP();
    S(IC<6>{}); F(IC<12>{}); F(IC<13>{}); G(IC<11>{});
    W4_GAP();
    PL(IC<5>{}); F(IC<14>{}); F(IC<15>{}); G(IC<12>{});
    W4_GAP();
    S(IC<7>{}); F(IC<16>{}); F(IC<17>{}); G(IC<13>{});
    W4_GAP();
    PL(IC<6>{}); F(IC<18>{}); F(IC<19>{}); G(IC<14>{});
    W4_GAP();
    S(IC<8>{}); F(IC<20>{}); F(IC<21>{}); G(IC<15>{});
#ifdef W4_HAZARD_SELFTEST
    { const float t_ = w4_max(nxt[0], nxt[1]); asm volatile("" ::"v"(t_)); }
#endif
    W4_GAP();
    PL(IC<7>{}); F(IC<22>{}); RL(); F(IC<23>{});
    W4_GAP();
    } else if constexpr (MODE == 3) {
    // MODE 0's stream without the reference-offset MFMA (it joins S(1), out of line, only while a row of the wave has a reference):
    // 18 MFMAs, the VALU stream unchanged
    S(IC<1>{}); W4_TOUCH(cur); MX(IC<0>{});
    W4_GAP();
    P(IC<0>{}); MX(IC<1>{});
    W4_GAP();
    S(IC<2>{}); MX(IC<2>{});
    W4_GAP();
    P(IC<1>{}); MX(IC<3>{});
    W4_GAP();
    MOVE();
    W4_GAP();
    S(IC<3>{}); F(IC<0>{}); F(IC<1>{}); G(IC<0>{});
    W4_GAP();
    P(IC<2>{}); F(IC<2>{}); F(IC<3>{}); G(IC<1>{});
    W4_GAP();
    S(IC<4>{}); F(IC<4>{}); F(IC<5>{}); G(IC<2>{});
    W4_GAP();
    P(IC<3>{}); F(IC<6>{}); F(IC<7>{}); G(IC<3>{});
    W4_GAP();
    S(IC<5>{}); F(IC<8>{}); F(IC<9>{}); G(IC<4>{});
    W4_GAP();
    P(IC<4>{}); F(IC<10>{}); F(IC<11>{}); G(IC<5>{});
    W4_GAP();
    S(IC<6>{}); F(IC<12>{}); F(IC<13>{}); G(IC<6>{});
    W4_GAP();
    P(IC<5>{}); F(IC<14>{}); F(IC<15>{}); G(IC<7>{});
    W4_GAP();
    S(IC<7>{}); F(IC<16>{}); F(IC<17>{}); G(IC<8>{});
    W4_GAP();
    P(IC<6>{}); F(IC<18>{}); F(IC<19>{}); G(IC<9>{});
    W4_GAP();
    S(IC<8>{}); F(IC<20>{}); F(IC<21>{}); G(IC<10>{});
#ifdef W4_HAZARD_SELFTEST
    { const float t_ = w4_max(nxt[0], nxt[1]); asm volatile("" ::"v"(t_)); }
#endif
    W4_GAP();
    P(IC<7>{}); F(IC<22>{}); G(IC<11>{});
    W4_GAP();
    P(IC<8>{}); G(IC<12>{}); G(IC<13>{});
    W4_GAP();
    P(IC<9>{}); G(IC<14>{}); G(IC<15>{});
    W4_GAP();
    F(IC<23>{});
    W4_GAP();
    } else if constexpr (MODE == 4) {
    // the caller's score bound is admissible (attn_bound_admissible: bound log2 e + log2 N + 24 <= 126, |v| <= 2^24 granted): no reference at all -- no row maximum, no branch, no offset
    // MFMA; the exponentials start with the step and spread over all 18 regions (one staging piece each in 16 of them).  Every pack
    // reads exponentials that are at least TWO regions old (e0 e1 | e2 | e3 | c0 e4 | e5 | c1 e6 | ...), so whatever order hipcc gives
    // the instructions inside a region -- it is free to sink the compiler-visible v_exp_f32 behind the region's asm pack, or to hoist
    // the next region's pack over its MFMA -- an MFMA lies between a transcendental result and its (invisible) reader; the first
    // version kept one region of distance and needed an s_nop in front of every pack (tools/check_mfma_hazard.py found the P.V-less
    // first step's violations)
    auto E = [&](auto Ic) __attribute__((always_inline)) {
      constexpr int e = decltype(Ic)::value;
      if constexpr (!(W4_ABL & 1)) cur[e] = __builtin_amdgcn_exp2f(cur[e]);
    };
    auto C2 = [&](auto Ic) __attribute__((always_inline)) {
      constexpr int c = decltype(Ic)::value;
      if constexpr (!(W4_ABL & 1)) pf[QB][c >> 2][c & 3] = w4_cvt_pk(cur[2 * c], cur[2 * c + 1]);
    };
    S(IC<1>{}); W4_TOUCH(cur); E(IC<0>{}); E(IC<1>{}); G(IC<0>{});
    W4_GAP();
    P(IC<0>{}); E(IC<2>{}); G(IC<1>{});
    W4_GAP();
    S(IC<2>{}); E(IC<3>{}); G(IC<2>{});
    W4_GAP();
    P(IC<1>{}); C2(IC<0>{}); E(IC<4>{}); G(IC<3>{});
    W4_GAP();
    S(IC<3>{}); E(IC<5>{}); G(IC<4>{});
    W4_GAP();
    P(IC<2>{}); C2(IC<1>{}); E(IC<6>{}); G(IC<5>{});
    W4_GAP();
    S(IC<4>{}); E(IC<7>{}); G(IC<6>{});
    W4_GAP();
    P(IC<3>{}); C2(IC<2>{}); E(IC<8>{}); G(IC<7>{});
    W4_GAP();
    S(IC<5>{}); E(IC<9>{}); G(IC<8>{});
    W4_GAP();
    P(IC<4>{}); C2(IC<3>{}); E(IC<10>{}); G(IC<9>{});
    W4_GAP();
    S(IC<6>{}); E(IC<11>{}); G(IC<10>{});
    W4_GAP();
    P(IC<5>{}); C2(IC<4>{}); E(IC<12>{}); G(IC<11>{});
    W4_GAP();
    S(IC<7>{}); E(IC<13>{}); G(IC<12>{});
    W4_GAP();
    P(IC<6>{}); C2(IC<5>{}); E(IC<14>{}); G(IC<13>{});
    W4_GAP();
    S(IC<8>{}); E(IC<15>{}); G(IC<14>{});
#ifdef W4_HAZARD_SELFTEST
    { const float t_ = w4_max(nxt[0], nxt[1]); asm volatile("" ::"v"(t_)); }
#endif
    W4_GAP();
    P(IC<7>{}); C2(IC<6>{}); G(IC<15>{});
    W4_GAP();
    P(IC<8>{});
    W4_GAP();
    P(IC<9>{}); C2(IC<7>{});
    W4_GAP();
    } else {
    // 16 MFMAs on ordinary data (S(1) starts the chain; the reference offset joins it, out of line, only while a row has one)
    S(IC<1>{}); W4_TOUCH(cur); MX(IC<0>{}); G(IC<0>{});
    W4_GAP();
    PL(IC<0>{}); MX(IC<1>{}); DL(IC<0>{}); G(IC<1>{});
    W4_GAP();
    S(IC<2>{}); MX(IC<2>{}); DL(IC<1>{}); DL(IC<2>{}); G(IC<2>{});
    W4_GAP();
    PL(IC<1>{}); MX(IC<3>{}); DL(IC<3>{}); DL(IC<4>{}); G(IC<3>{});
    W4_GAP();
    S(IC<3>{}); DL(IC<5>{}); DL(IC<6>{}); DL(IC<7>{}); G(IC<4>{});
    W4_GAP();
    MOVE();
    W4_GAP();
    PL(IC<2>{}); F(IC<0>{}); F(IC<1>{}); G(IC<5>{});
    W4_GAP();
    S(IC<4>{}); F(IC<2>{}); F(IC<3>{}); G(IC<6>{});
    W4_GAP();
    PL(IC<3>{}); F(IC<4>{}); F(IC<5>{}); G(IC<7>{});
    W4_GAP();
    S(IC<5>{}); F(IC<6>{}); F(IC<7>{}); G(IC<8>{});
    W4_GAP();
    PL(IC<4>{}); F(IC<8>{}); F(IC<9>{}); G(IC<9>{});
    W4_GAP();
    S(IC<6>{}); F(IC<10>{}); F(IC<11>{}); G(IC<10>{});
    W4_GAP();
    PL(IC<5>{}); F(IC<12>{}); F(IC<13>{}); G(IC<11>{});
    W4_GAP();
    S(IC<7>{}); F(IC<14>{}); F(IC<15>{}); G(IC<12>{});
    W4_GAP();
    PL(IC<6>{}); F(IC<16>{}); F(IC<17>{}); G(IC<13>{});
    W4_GAP();
    S(IC<8>{}); F(IC<18>{}); F(IC<19>{}); G(IC<14>{});
#ifdef W4_HAZARD_SELFTEST
    { const float t_ = w4_max(nxt[0], nxt[1]); asm volatile("" ::"v"(t_)); }
#endif
    W4_GAP();
    PL(IC<7>{}); F(IC<20>{}); F(IC<21>{}); G(IC<15>{}); RL();
    W4_GAP();
    F(IC<22>{}); F(IC<23>{});
    W4_GAP();
    }
  };

  const int j_rag = (Nk & (W4_KV - 1)) ? nkv - 1 : -1;          // the tile whose key blocks reach past N
  // one 64-key tile j out of ring buffer B (compile-time: every fragment address is a per-lane base plus an immediate)
  auto tile = [&](int j, auto Bc, auto FIRSTc) __attribute__((always_inline)) {
    constexpr int B = decltype(Bc)::value, NB = (B + 1) % 3, WB = (B + 2) % 3;
    constexpr int FIRST = decltype(FIRSTc)::value;
    // (one scalar compare each against tile indices fixed in front of the loop: with one wave per SIMD every scalar instruction of
    // the tile loop is issue time)
    const bool rag = j == j_rag;
    // (kb0, q0): S(kb0, q1);  pending (tile j-1: kb1, q1);  reload kf <- K(j) kb1, vf <- V(j) kb0
    step(IC<0>{}, IC<!FIRST>{}, IC<FIRST>{}, IC<B * W4_KT + 32 * W4_KROW>{}, IC<B * W4_VT>{}, IC<0>{}, 0, rag, j * W4_KV);
    // (kb0, q1): S(kb1, q0);  pending (kb0, q0);  + staging: tile j + 2 (requested one tile ago) goes into the buffer tile j - 1
    // left before the last barrier, and each register is refilled with its piece of tile j + 3 right behind its write -- four
    // steps (> 1 us) before it is needed: with one wave per SIMD nothing else runs while a wave waits for memory
    step(IC<1>{}, IC<1>{}, IC<FIRST>{}, IC<0>{}, IC<0>{}, IC<1 + 4 * WB>{}, j + 3, rag, j * W4_KV);
    // (kb1, q0): S(kb1, q1);  pending (kb0, q1);  reload kf <- K(j+1) kb0, vf <- V(j) kb1
    step(IC<0>{}, IC<1>{}, IC<0>{}, IC<NB * W4_KT>{}, IC<B * W4_VT + 2 * 16 * 256>{}, IC<0>{}, 0, rag, j * W4_KV + 32);
    // (kb1, q1): S(tile j+1: kb0, q0);  pending (kb1, q0)
    step(IC<1>{}, IC<1>{}, IC<0>{}, IC<0>{}, IC<0>{}, IC<0>{}, 0, rag, j * W4_KV + 32);
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (!(W4_ABL & 16)) __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
  };
  W4_STAMP(1);
  tile(0, IC<0>{}, IC<1>{});
  for (int j = 1; j < nkv; j += 3) {
    tile(j, IC<1>{}, IC<0>{});
    if (j + 1 < nkv) tile(j + 1, IC<2>{}, IC<0>{});
    if (j + 2 < nkv) tile(j + 2, IC<0>{}, IC<0>{});
  }
  W4_STAMP(2);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // requests past the end of the sequence (zeros) still write their registers
  // persistent form: the NEXT item's Q rows are requested here, behind the tile loop, and fly while this item's output is normalised,
  // staged and stored; its first K / V tile is requested behind the output's stores and flies under the next prologue's Q conversion.
  // (Measured on the way, tools/attn_item_timers.py: requests from inside the last tiles cost EVERY tile ~60 cycles -- even a single
  // compare + branch per tile: the next-Q registers live across the loop --, 4.2 k per item; all 24 requests in one burst here make the
  // output's stores queue behind them, +4.6 k.)
  if (has_next) load_qn();
  // ---- drain: the pending P.V of the very last unit (last tile: kb1, q1), V fragments already in registers
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
    for (int db = 0; db < 4; ++db) w4_mfma_o(o[1][db], vf[ks][db], pf[1][ks]);
    if constexpr (!LV) w4_mfma_l(ol[1], vone, pf[1][ks]);
  }
  float ltot[2];                                 // full row sums (LV: the two 16-key halves of every unit live in lanes l and l ^ 32)
  if constexpr (LV) {
#pragma unroll
    for (int c = 0; c < 8; ++c) w4_dot2c(lsum[1], pf[1][c >> 2][c & 3]);
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) ltot[qb] = lsum[qb] + __shfl_xor(lsum[qb], 32, 64);
  }
#ifdef W4_KEEP_DRAINS
  W4_DRAIN_MFMA();                               // the last MFMA results before the VALU reads them
#endif
  if constexpr (!LV) {
    ltot[0] = ol[0][0];                          // every row of the ones-block holds the full row sum
    ltot[1] = ol[1][0];
  }

  // ---- tail split: un-normalised O (fp32), row sum and reference maximum of this key range -> part [tile][range][row][132]
  if (kpart >= 0 || pslot >= 0) {
    float* pp = part + (kpart >= 0 ? (int64_t)ptile * nsplit + kpart : (int64_t)pslot) * (256 * W4_PROW);
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
      float* pr = pp + (wave * 2 + qb) * (16 * 256) + lane * 4;        // w4_part_off: 1 KiB contiguous per store instruction
#pragma unroll
      for (int db = 0; db < 4; ++db)
#pragma unroll
        for (int qd = 0; qd < 4; ++qd)
          *reinterpret_cast<f32x4*>(pr + (db * 4 + qd) * 256) =
              f32x4{o[qb][db][qd * 4 + 0], o[qb][db][qd * 4 + 1], o[qb][db][qd * 4 + 2], o[qb][db][qd * 4 + 3]};
      if (hi == 0) *reinterpret_cast<float2*>(pp + W4_PART_LM + (wave * 64 + qb * 32 + l31) * 2) = float2{ltot[qb], m_ref[qb]};
    }
    if (kpart >= 0) return;
  } else {
  // ---- finish.  The normalised bf16 rows go through a wave-private LDS
  // tile (the K / V ring is free: every wave's last fragment read lies before the last barrier) and leave as whole 256-byte
  // rows, 16 lanes x 16 bytes each (row-per-lane 8-byte stores touch 32 lines per instruction and queue up at the end of
  // the block, when every wave of the workgroup stores at once)
  constexpr int OROW = 272;
  char* ot = smem + wave * (64 * OROW);
#pragma unroll
  for (int qb = 0; qb < 2; ++qb) {
    const float inv = 1.0f / ltot[qb];
    char* orow = ot + (qb * 32 + l31) * OROW + 8 * hi;
#pragma unroll
    for (int db = 0; db < 4; ++db)
#pragma unroll
      for (int qd = 0; qd < 4; ++qd) {
        u32x2 w;
        w[0] = pack_bf2(o[qb][db][qd * 4 + 0] * inv, o[qb][db][qd * 4 + 1] * inv);
        w[1] = pack_bf2(o[qb][db][qd * 4 + 2] * inv, o[qb][db][qd * 4 + 3] * inv);
        *reinterpret_cast<u32x2*>(orow + db * 64 + qd * 16) = w;
      }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  const int row0 = qblk * 256 + wave * 64;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int c = lane + 64 * i, row = c >> 4, ch = c & 15;
    const u32x4 v = *reinterpret_cast<const u32x4*>(ot + row * OROW + ch * 16);
    if (row0 + row < Nb) *reinterpret_cast<u32x4*>(Ob + (int64_t)(row0 + row) * ldo + ch * 8) = v;
  }
  }    // (whole item)
#ifdef TFX_BENCH
  W4_STAMP(3);
  w4_sum[0] += w4_stamp[1] - w4_stamp[0]; w4_sum[1] += w4_stamp[2] - w4_stamp[1]; w4_sum[2] += w4_stamp[3] - w4_stamp[2]; w4_sum[3] += 1;
  if (!has_next && g_w4_timers && tid == 0)
    for (int i = 0; i < 4; ++i) atomicAdd(g_w4_timers + i, w4_sum[i]);
#endif
  if (!has_next) break;
  rsKs = rsK2;
  rsVs = rsV2;
  load_tile(0);                                   // the next item's first K / V tile (its descriptors; kreg / vreg are idle until the next prologue writes them)
  item = item2; b = b2; h = h2; qblk = qblk2;
  if (sk_share > 0) { ++sk_u; int it_; sk_unit(sk_u, it_, ts, te); }
  have_pref = true;
  // every wave has read its output tile out of LDS: the ring buffers are free for the next item.  A bare barrier behind an LDS-only
  // wait -- __syncthreads() would also wait for the next item's requests that were just issued (4.6 k cycles per item, measured)
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
  }
}
