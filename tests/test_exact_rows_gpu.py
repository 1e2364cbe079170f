"""Exact-statistics tests of the HBM-bound row kernels at their shape edges: LayerNorm + modulation (plain, split, fp8), affine LayerNorm,
GroupNorm, the scheduler steps, the text encoders' row kernels and row_softmax.  The inputs of tests/helpers/exact_inputs.py leave a
kernel ONE freedom -- the fp32 row factor rsqrt(var + eps), good to a step or two -- so every output element is compared with the CPU
restatement of the kernel's rounding points at `ulps=1` and a cap of four times the share of elements that freedom can move
(tests/test_exact_inputs_cpu.py measures it on these very cases; a share of 0 makes the comparison bit for bit).  The shapes are the
smallest at which each guard, chunk round and tail of the kernels is live.  Every output is a view inside a canary-filled buffer, every
input a view inside a NaN-filled one: a read or a write outside the operands shows."""
import functools

import pytest
import torch

from tests.helpers import exact_inputs as X
from tests.helpers.framing import CANARY, check_frame, flat_framed, framed, strided

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    from textflux_amd import ops as o
    return o


# ------------------------------------------------------------------------------------------------ LayerNorm + modulation
@pytest.mark.parametrize("offset", X.LN_OFFSETS)
@pytest.mark.parametrize("D", X.LN_DS)
def test_ln_modulate_every_chunk_round_with_and_without_prefetch(ops, D, offset):
    """D / 8 chunks over six rounds of 64 lanes: 1 | 63 | 64 | 65 | 193 | 383 | 384 chunks; 1 .. 37 rows against the four of a workgroup;
    x row- and batch-strided, ldo != ldx, shift / scale slices of one [B, 6 D] table.  Both instantiations (modulation rows requested up
    front or not) give the same bits, and those are the chain's (LN_SHARE is 0)."""
    B = 2
    try:
        for R in X.LN_ROWS:
            cs = X.ln_case(B, R, D, offset)
            mod = cs["mod"].cuda()
            sh, sc, _, _ = X.mod_slices(mod, D)
            want = X.ln_modulate_chain(cs["x"], *X.mod_slices(cs["mod"], D)[:2], cs["mean"], cs["r"])
            x = strided(cs["x"].to(BF))
            assert x.stride(1) > D and x.stride(0) != R * x.stride(1) and sh.stride(0) == 6 * D
            outs = []
            for pref in (0, 1):
                ops.set_option("ln_prefetch", pref)
                buf, out = framed(B, R, D)
                assert out.stride(1) != x.stride(1)
                ops.ln_modulate(x, sh, sc, out=out)
                check_frame(buf, out, f"ln_modulate D {D} R {R} prefetch {pref}")
                X.assert_elementwise(out, want, f"ln_modulate D {D} R {R} offset {offset} prefetch {pref}", ulps=1, cap=4 * X.LN_SHARE)
                outs.append(out.clone())
            assert torch.equal(outs[0], outs[1]), f"D {D} R {R}: the two instantiations differ"
    finally:
        ops.set_option("ln_prefetch", 2)


@pytest.mark.parametrize("split", X.LN_SPLIT_ROWS)
@pytest.mark.parametrize("D", X.LN_SPLIT_DS)
def test_ln_modulate_split_is_two_launches_on_the_two_row_ranges(ops, D, split):
    B, R = 2, X.LN_SPLIT_R
    cs = X.ln_case(B, R, D, 3)
    mod = cs["mod"].cuda()
    sh, sc, sh2, sc2 = X.mod_slices(mod, D)
    x = strided(cs["x"].to(BF))
    want = X.ln_modulate_chain(cs["x"], *X.mod_slices(cs["mod"], D)[:2], cs["mean"], cs["r"], split, *X.mod_slices(cs["mod"], D)[2:])
    try:
        for pref in (0, 1):
            ops.set_option("ln_prefetch", pref)
            buf, out = framed(B, R, D)
            ops.ln_modulate(x, sh, sc, out=out, split_row=split, shift2=sh2, scale2=sc2)
            check_frame(buf, out, f"ln_modulate_split D {D} split {split}")
            two = torch.full((B, R, D), CANARY[BF], dtype=BF, device="cuda")
            if split > 0:
                ops.ln_modulate(x[:, :split], sh2, sc2, out=two[:, :split])
            if split < R:
                ops.ln_modulate(x[:, split:], sh, sc, out=two[:, split:])
            assert torch.equal(out, two), f"D {D} split {split} prefetch {pref}: not the two launches"
            X.assert_elementwise(out, want, f"ln_modulate_split D {D} split {split} prefetch {pref}", ulps=1, cap=4 * X.LN_SHARE)
    finally:
        ops.set_option("ln_prefetch", 2)
    if split == 0:      # no second modulation needed
        assert torch.equal(ops.ln_modulate(x, sh, sc, split_row=0), out)


@pytest.mark.parametrize("D", X.LN_DS)
def test_ln_modulate_fp8_into_strided_views_is_the_quantised_bf16_row(ops, D):
    """ldq > D, q_bstride != R * ldq, s_bstride > R; sample 1 has shift 0 and a constant row 0: an all-zero output row, scale 1 and zero codes."""
    B = 2
    for R in (1, 5, 37):
        cs = X.ln_case(B, R, D, 3)
        cs["mod"][1, :D] = 0
        cs["x"][1, 0] = 3.0
        mod = cs["mod"].cuda()
        sh, sc, _, _ = X.mod_slices(mod, D)
        x = strided(cs["x"].to(BF))
        qbuf, q = framed(B, R, D, torch.uint8)
        sbuf, s = framed(1, B, R, torch.float32, pad_rows=2, pad_cols=8)
        s = s[0]
        assert q.stride(1) > D and q.stride(0) != R * q.stride(1) and s.stride(0) > R
        ops.ln_modulate_fp8(x, sh, sc, out=q, scale_out=s)
        check_frame(qbuf, q, f"ln_modulate_fp8 codes D {D} R {R}")
        check_frame(sbuf, s, f"ln_modulate_fp8 scales D {D} R {R}")
        y = ops.ln_modulate(x, sh, sc)
        q2, s2 = ops.quantize_rows_fp8(y)
        assert torch.equal(s, s2), f"D {D} R {R}: scales"
        bad = (q != q2).nonzero()
        assert bad.numel() == 0, f"D {D} R {R}: {bad.shape[0]} codes differ, first (b, row, col) {bad[0].tolist()}"
        assert bool((y[1, 0] == 0).all()) and s[1, 0].item() == 1.0 and int(q[1, 0].max()) == 0
        assert bool((s[0] > 0).all()) and int(q[0].max()) > 0


# ------------------------------------------------------------------------------------------------ affine LayerNorm
@functools.lru_cache(maxsize=None)
def lna_run(rows, D):
    from textflux_amd import ops
    cs = X.lna_case(rows, D)
    x = strided(cs["x"].to(BF)[None])[0]
    buf, out = framed(1, rows, D)
    ops.layernorm(x, cs["gamma"].cuda(), cs["beta"].cuda(), eps=1e-5, out=out[0])
    check_frame(buf, out[0], f"layernorm D {D} rows {rows}")
    want = X.layernorm_affine_chain(cs["x"], cs["gamma"], cs["beta"], cs["mean"], cs["r"])
    return X.assert_elementwise(out[0], want, f"layernorm D {D} rows {rows}", ulps=1), want.numel()


@pytest.mark.parametrize("rows", X.LNA_ROWS)
@pytest.mark.parametrize("D", X.LNA_DS)
def test_layernorm_affine_within_a_step_of_the_chain(D, rows):
    lna_run(rows, D)


def test_layernorm_affine_differences_stay_under_the_cap():
    """The cap belongs to the cases as a whole: the elements one step of the row factor (or a contracted multiply-add) can move are few and
    sit in a few of the cases, so the share is taken over all of them, as the CPU measurement takes it."""
    runs = [lna_run(rows, D) for D in X.LNA_DS for rows in X.LNA_ROWS]
    diff, n = sum(r[0] for r in runs), sum(r[1] for r in runs)
    print(f"layernorm (affine): {diff} of {n} elements differ from the chain; cap {4 * X.LN_AFFINE_SHARE * n:.1f}")
    assert diff <= 4 * X.LN_AFFINE_SHARE * n


# ------------------------------------------------------------------------------------------------ GroupNorm
def float_steps(a, b):
    """fp32 steps between positive floats."""
    return (a.contiguous().view(torch.int32).long() - b.contiguous().view(torch.int32).long()).abs()


@functools.lru_cache(maxsize=None)
def gn_run(C, groups, HW):
    """tfx_groupnorm_nhwc with the test's own workspace: the statistics it leaves there, the output without SiLU against the chain, the
    output with SiLU against the fp64 SiLU of the kernel's own y.  (sample 1, last group) is constant 0.5: its variance is 0 or the rounding
    residue of E[x^2] - mean^2, and its outputs must be bf16(beta) exactly.  Returns (elements differing from the chain, elements)."""
    from textflux_amd import _lib as L
    B, cpg, nchunk = 2, C // groups, (HW + 1023) // 1024
    cs = X.gn_case(C, groups, HW)
    xc = cs["x"].clone()
    xc[1, :, C - cpg:] = 0.5
    x, gamma, beta = xc.to(BF).cuda(), cs["gamma"].cuda(), cs["beta"].cuda()
    normal = torch.ones(B, groups, dtype=torch.bool)
    normal[1, groups - 1] = False
    chan = normal.repeat_interleave(cpg, 1)[:, None, :].expand(B, HW, C)
    want = X.groupnorm_chain(cs["x"], cs["gamma"], cs["beta"], cs["mean"], cs["rstd"], groups, False)
    want = torch.where(chan, want, cs["beta"].expand(B, HW, C))
    what = f"groupnorm C {C} groups {groups} HW {HW}"
    stream = torch.cuda.current_stream().cuda_stream
    ys = {}
    for silu in (0, 1):
        wbuf, ws = flat_framed((B * (nchunk + 1) * groups * 2,), torch.float32)
        obuf, out = flat_framed((B, HW, C))
        L.check(L.lib().tfx_groupnorm_nhwc(x.data_ptr(), out.data_ptr(), gamma.data_ptr(), beta.data_ptr(), ws.data_ptr(), B, HW, C, groups,
                                           1e-6, silu, stream), what)
        check_frame(obuf, out, what)
        check_frame(wbuf, ws, what + " workspace")
        stat = ws[B * nchunk * groups * 2:].view(B, groups, 2).cpu()
        mean, rstd = stat[..., 0], stat[..., 1]
        assert torch.equal(mean[normal], cs["mean"].float()[normal]), f"{what}: means {mean[normal][:8].tolist()}"
        steps = float_steps(rstd, cs["rstd"].float())[normal]
        assert steps.max().item() <= 2, f"{what}: rstd {steps.max().item()} fp32 steps from the fp64 value (group {steps.argmax().item()})"
        assert torch.isfinite(rstd).all() and abs(mean[1, groups - 1].item() - 0.5) <= 2.0 ** -24
        ys[silu] = out.cpu()
    assert bool(torch.isfinite(ys[0].float()).all()) and bool(torch.isfinite(ys[1].float()).all())
    assert torch.equal(ys[0][~chan], want[~chan]), f"{what}: the constant group is not bf16(beta)"
    n_diff = X.assert_elementwise(ys[0], want, what, ulps=1)
    # SiLU: y / (1 + __expf(-y)) in fp32.  |y| <= 8 here, so the exponent y * log2(e), rounded to fp32, is off by at most 12 * 2^-24 and
    # the power by 2^-21 of itself; the hardware exp2, the sum and the quotient add a few 2^-24: 2^-20 in all, a sixth of the 2^-18
    # margin `settled` keeps from a rounding boundary.
    assert ys[0].float().abs().max().item() <= 8.0
    s64 = X.silu64(ys[0])
    X.assert_elementwise(ys[1], s64.float().to(BF), what + " SiLU", ulps=1)
    sure = X.settled(s64, 2.0 ** -18)
    X.assert_elementwise(torch.where(sure, ys[1], torch.zeros_like(ys[1])), torch.where(sure, s64.float().to(BF), torch.zeros_like(ys[1])),
                         what + " SiLU away from a rounding boundary")
    return n_diff, want.numel()


@pytest.mark.parametrize("C,groups,HW", X.GN_CASES)
def test_groupnorm_statistics_and_output(C, groups, HW):
    """1 pixel | one chunk short of / at / past its edge | 64 groups (the second slot of gn_finalize) over 9 chunks (its chunk loop wraps) |
    64 chunks per pixel | 16 channels per group: one 16-byte chunk never spans two groups, two chunks share one."""
    gn_run(C, groups, HW)


def test_groupnorm_differences_stay_under_the_cap():
    runs = [gn_run(*c) for c in X.GN_CASES]
    diff, n = sum(r[0] for r in runs), sum(r[1] for r in runs)
    print(f"groupnorm: {diff} of {n} elements differ from the chain; cap {4 * X.GN_SHARE * n:.1f}")
    assert diff <= 4 * X.GN_SHARE * n


# ------------------------------------------------------------------------------------------------ scheduler steps
@pytest.mark.parametrize("rows,C,ldxin", [(37, 64, 384), (37, 64, 96), (300, 16, 96), (1, 8, 96)])
def test_scheduler_steps_at_the_tail_and_other_channel_counts(ops, rows, C, ldxin):
    """296 chunks (one workgroup and a tail of 40), 600 chunks of a 16-wide latent (two chunks per xin row), one chunk.  Dyadic coefficients;
    the step index once as an argument and once from device memory."""
    seed = X.shape_seed(rows, C, ldxin)
    v, x0, noise = X.arbitrary_bf16((rows, C), seed), X.arbitrary_bf16((rows, C), seed + 1), torch.randn(rows, C, generator=X.gen(seed + 2))
    ecoef = torch.tensor([0.5, -0.03125, -0.0625])
    acoef = torch.tensor([[0.25, 1.0, 1.0], [-0.0625, 0.75, 0.5], [-0.125, 1.25, -0.25]])
    for step, ptr in ((1, None), (0, torch.tensor([2], dtype=torch.int32, device="cuda"))):
        s = step if ptr is None else 2
        for amo in (False, True):
            xbuf, x = flat_framed((rows, C))
            x.copy_(x0)
            xin = torch.full((rows, ldxin), CANARY[BF], dtype=BF, device="cuda")
            if amo:
                ops.amo_step_(v.cuda(), x, acoef.cuda(), noise.cuda(), step=step, step_ptr=ptr, xin=xin)
                want = X.amo_chain(v, x0, noise, *acoef[s].tolist())
            else:
                ops.euler_step_(v.cuda(), x, ecoef.cuda(), step=step, step_ptr=ptr, xin=xin)
                want = X.euler_chain(v, x0, ecoef[s].item())
            what = f"{'amo' if amo else 'euler'} rows {rows} C {C} step {s}"
            check_frame(xbuf, x, what)
            X.assert_elementwise(x, want, what)
            assert torch.equal(xin[:, :C], x) and bool((xin[:, C:] == CANARY[BF]).all()), f"{what}: xin"


# ------------------------------------------------------------------------------------------------ text-encoder row kernels
@pytest.mark.parametrize("f32", (True, False))
@pytest.mark.parametrize("D", X.T5_DS)
def test_t5_rmsnorm(ops, D, f32):
    for rows in X.T5_ROWS:
        cs = X.t5_case(rows, D, f32)
        x = strided(cs["x"][None], pad_cols=12, col0=4)[0]
        buf, out = framed(1, rows, D, pad_cols=5)
        ops.rmsnorm(x, cs["w"].cuda(), 1e-6, out=out[0])
        check_frame(buf, out[0], f"rmsnorm D {D} rows {rows}")
        X.assert_elementwise(out[0], X.t5_rmsnorm_chain(cs["x"], cs["w"], cs["r"]), f"rmsnorm D {D} rows {rows} f32 {f32}", ulps=1, cap=4 * X.T5_SHARE)


def test_mul_and_quick_gelu_on_strided_operands(ops):
    a, b = X.arbitrary_bf16((5, 100), 1, 2.0), X.arbitrary_bf16((5, 100), 2)
    da, db = strided(a[None], pad_cols=12, col0=4)[0], strided(b[None], pad_cols=7, col0=3)[0]
    buf, out = framed(1, 5, 100, pad_cols=5)
    ops.mul(da, db, out=out[0])
    check_frame(buf, out[0], "mul")
    X.assert_elementwise(out[0], a * b, "mul")
    buf, out = framed(1, 5, 100, pad_cols=5)
    ops.quick_gelu(da, out=out[0])
    check_frame(buf, out[0], "quick_gelu")
    X.assert_elementwise(out[0], X.quick_gelu_chain(a), "quick_gelu", ulps=1)


@pytest.mark.parametrize("n", (1, 257))
def test_add_into_f32_three_modes(ops, n):
    g = X.gen(n)
    x0, y32, ybf = torch.randn(n, generator=g), torch.randn(n, generator=g), X.arbitrary_bf16((n,), n + 1)
    for y, assign, want in ((ybf, False, x0 + ybf.float()), (y32, False, x0 + y32), (ybf, True, ybf.float())):
        buf, x = flat_framed((n,), torch.float32)
        x.copy_(x0)
        ops.add_into_f32_(x, y.cuda(), assign=assign)
        check_frame(buf, x, f"add_into_f32 n {n}")
        X.assert_elementwise(x, want, f"add_into_f32 n {n} {y.dtype} assign {assign}")


def test_gather_rows_clamps_ids_to_the_table(ops):
    vocab, D = 11, 24
    table = X.arbitrary_bf16((vocab, D), 3)
    ids = torch.tensor([0, vocab - 1, -1, -(1 << 40), vocab, 1 << 40, 5, 0])
    buf, out = flat_framed((ids.numel(), D))
    ops.gather_rows(table.cuda(), ids.cuda(), out=out)
    check_frame(buf, out, "gather_rows")
    X.assert_elementwise(out, table[ids.clamp(0, vocab - 1)], "gather_rows")


# ------------------------------------------------------------------------------------------------ row_softmax
@pytest.mark.parametrize("aligned", (True, False))
@pytest.mark.parametrize("N", (1, 7, 255, 256, 257, 1001, 2056))
def test_row_softmax_vector_and_scalar_path(ops, N, aligned):
    """One bf16 step per element against the fp64 softmax: exp2f and the 256-way fp32 sum each stay far inside half a bf16 step.  aligned:
    16-byte rows on both sides (the vector path where N % 8 == 0); otherwise lds % 4 != 0 (the scalar path at every N)."""
    rows, scale = 5, 0.125
    s = torch.randn(rows, N, generator=X.gen(N)) * 24.0
    lds = (N + 11) // 4 * 4 + (0 if aligned else 1)
    sbuf = torch.full((rows + 2, lds), float("nan"), device="cuda")
    sv = sbuf[1:rows + 1, :N]
    sv.copy_(s)
    assert sv.stride(0) % 4 == (0 if aligned else 1) and (not aligned or sv.data_ptr() % 16 == 0)
    buf, out = framed(1, rows, N, pad_cols=16 - N % 8 if aligned else 13)
    assert not aligned or (out.stride(1) % 8 == 0 and out[0].data_ptr() % 16 == 0)
    ops.row_softmax(sv, scale, out[0])
    check_frame(buf, out[0], f"row_softmax N {N}")
    X.assert_elementwise(out[0], X.softmax_rows64(s, scale), f"row_softmax N {N} aligned {aligned}", ulps=1)
