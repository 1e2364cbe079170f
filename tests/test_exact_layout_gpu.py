"""Exact tests of the kernels that run on every call of the pipeline around the matrix-pipe and row kernels: the rest of elementwise.hip
(rmsnorm_rope, gate_residual, copy_rows, scatter_cols, timestep_embedding, silu / add, select_step / advance_step) and the layout kernels at
the top of imageops.hip (any_negative, prep_image, pack_mask, sample_pack, unpack_latents, postprocess, transpose).  Built like
tests/test_exact_rows_gpu.py: every output element is compared with a CPU restatement of the kernel's rounding points (torch's bf16 / fp32
operators, which round correctly, or fp64), bit for bit wherever the arithmetic leaves no freedom; the shapes are the smallest at which each
guard, tail, instantiation and branch is live (each docstring says which); outputs sit in canary frames, inputs in NaN (uint8: zero) frames.
Where an ops.py wrapper allocates its own output the C entry is called directly, so that the output can sit in a frame."""
import functools

import numpy as np
import pytest
import torch

from oracle import pipeline_oracle as po
from tests.helpers import exact_inputs as X
from tests.helpers.framing import CANARY, check_frame, flat_framed, flat_in, framed, strided

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
CANARY_BITS = -256                                  # 0xFF00, the bf16 canary -2^127, as int16
SHIFT, SCALE = 0.1159, 0.3611                       # the VAE's shift_factor / scaling_factor


@pytest.fixture(scope="module")
def ops():
    from textflux_amd import ops as o
    return o


def entry(name, *args):
    """A C entry of the library on the current stream; a non-zero return raises with tfx_last_error."""
    from textflux_amd import _lib as L
    L.check(getattr(L.lib(), name)(*args, torch.cuda.current_stream().cuda_stream), name)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def random_bits(shape, seed):
    """bf16 tensors of arbitrary bit patterns -- NaN payloads, infinities, subnormals, both zeros -- without the canary's."""
    b = torch.randint(-32768, 32768, shape, generator=X.gen(seed), dtype=torch.int16)
    b[b == CANARY_BITS] = 0
    return b.view(BF)


def assert_bits(got, want, what, nan_payload=False):
    """The same bit pattern in every element (so -0.0 is not +0.0); a NaN only has to be a NaN where `want` has one, unless nan_payload
    (pure data movement).  Arithmetic on a NaN gives the x86 host and the device different payloads; that is not the kernel's business."""
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.shape == want.shape and got.dtype == want.dtype == BF, (got.shape, want.shape, got.dtype, want.dtype)
    g, w = bits(got).clone(), bits(want).clone()
    if not nan_payload:
        ng, nw = torch.isnan(got), torch.isnan(want)
        assert torch.equal(ng, nw), f"{what}: NaNs at {(ng != nw).nonzero()[:8].tolist()} on one side only"
        g[ng], w[nw] = 0, 0
    bad = (g != w).nonzero().tolist()
    assert not bad, (f"{what}: {len(bad)} of {g.numel()} bit patterns differ, first at {bad[0]}: got {got[tuple(bad[0])].item()!r}, "
                     f"want {want[tuple(bad[0])].item()!r}")


def outside_bits(view):
    """The bit patterns of the buffer a `strided` / column-slice view lies in, with the view's own elements zeroed: what a kernel writing
    into the view must leave as it was."""
    base = view._base
    b = base.view(torch.int16 if base.dtype == BF else torch.int32).clone()
    b.as_strided(view.shape, view.stride(), view.storage_offset() - base.storage_offset()).zero_()
    return b.cpu()


def flat_outside_intact(buf, view, what):
    """check_frame's first half for a flat frame whose view may itself hold the canary's bit pattern."""
    pad = (buf.numel() - view.numel()) // 2
    assert bool((buf[:pad] == CANARY[buf.dtype]).all()) and bool((buf[pad + view.numel():] == CANARY[buf.dtype]).all()), f"{what}: wrote outside its output"


# ------------------------------------------------------------------------------------------------ rmsnorm_rope
@functools.lru_cache(maxsize=None)
def rope_run(H):
    """Every (B, Ntok, T, table form) of X.rope_cases() at H heads, in both column orders, through ops.rmsnorm_rope_ on a [B, Ntok, ld] view
    with ld > 3 H 128 and pad rows between the samples.  Returns (elements differing from the chain, elements)."""
    from textflux_amd import ops
    D, pad = H * 128, 2
    ld = 3 * D + 24
    diff = n = 0
    for _, B, N, T, per_sample in [c for c in X.rope_cases() if c[0] == H]:
        cs = X.rope_case(H, B, N, T, per_sample)
        want = X.rms_rope_chain(cs["x"], cs["w"], cs["cos"], cs["sin"], cs["r"]).reshape(B, N, 2 * D)
        ws = [w.cuda() for w in cs["ws"]]
        cos, sin = cs["cos"].cuda(), cs["sin"].cuda()
        assert cos.dim() == (3 if per_sample else 2)
        xq, xk = (t.reshape(B, N, D).to(BF).cuda() for t in (cs["x"][:, :, :H], cs["x"][:, :, H:]))
        for q_off, k_off in ((2 * D, 0), (0, 2 * D)):                      # [k | v | q] and [q | v | k]
            what = f"rmsnorm_rope H {H} B {B} Ntok {N} T {T} per-sample tables {per_sample} q_off {q_off}"
            big = torch.full((B, N + 2 * pad, ld), CANARY[BF], dtype=BF, device="cuda")
            buf = big[:, pad:pad + N]
            buf[..., q_off:q_off + D], buf[..., k_off:k_off + D] = xq, xk
            assert buf.stride(1) > 3 * D and buf.stride(0) > N * ld
            ops.rmsnorm_rope_(buf, q_off, k_off, H, T, *ws, cos, sin)
            got = big.cpu()
            keep = torch.ones(got.shape, dtype=torch.bool)
            keep[:, pad:pad + N, q_off:q_off + D] = False
            keep[:, pad:pad + N, k_off:k_off + D] = False
            assert bool((got[keep] == CANARY[BF]).all()), f"{what}: wrote outside q and k (the v columns, the row tail or a pad row)"
            inner = got[:, pad:pad + N]
            qk = torch.cat([inner[..., q_off:q_off + D], inner[..., k_off:k_off + D]], -1)
            diff += X.assert_elementwise(qk, want, what, ulps=1)
            n += qk.numel()
    return diff, n


@pytest.mark.parametrize("H", X.ROPE_HS)
def test_rmsnorm_rope_within_a_step_of_the_chain(H):
    """rmsnorm_rope_kernel deals 2H head rows to four lane groups, per = ceil(2H / 4) each, six at a time, duplicate loads clamped to the
    group's last row.  H 1: two groups with no rows | 3: two rows a group, q and k in different groups | 5: a group whose rows straddle the
    q / k boundary and a last group of one | 13: a second round of six with one row (seven a group), a last group of five | 24: two full
    rounds.  (B, Ntok) (1, 1): one token, 12 of the workgroup's 16 lane groups past the end | (2, 5): the workgroup of tokens 4 .. 7 spans both
    samples | (1, 37): ten workgroups, one token in the last.  T 0 | 2 (the text / image weight switch inside a workgroup's four tokens) |
    Ntok.  Four different non-dyadic weights, the reference's own fp32 rotary tables, shared and per sample.  Both column orders."""
    rope_run(H)


def test_rmsnorm_rope_differences_stay_under_the_cap():
    """The cap belongs to the cases as a whole, as the CPU measurement of X.ROPE_SHARE takes it."""
    runs = [rope_run(H) for H in X.ROPE_HS]
    diff, n = sum(r[0] for r in runs), sum(r[1] for r in runs)
    print(f"rmsnorm_rope: {diff} of {n} elements differ from the chain; cap {4 * X.ROPE_SHARE * n:.1f}")
    assert diff <= 4 * X.ROPE_SHARE * n


# ------------------------------------------------------------------------------------------------ gate_residual
@pytest.mark.parametrize("B,R,D", ((2, 1, 8), (2, 37, 72), (3, 5, 3072)))
def test_gate_residual_is_the_two_bf16_ops_also_in_place_and_on_non_finite_values(ops, B, R, D):
    """gate_residual_kernel: one 16-byte chunk per thread, i -> (b, r, c) by two divisions.  (2, 1, 8): two chunks, one thread per sample |
    (2, 37, 72): nine chunks a row, 666 in all: three workgroups, the last with 154 threads | (3, 5, 3072): the model's width, 384 chunks a
    row.  x, res and out have three different pitches; the gate is a column slice of a [B, 6 D] table.  In place over res and over x (the
    kernel's pointers are not restrict).  The last row of the last sample holds inf, -inf, NaN and -0.0 in x and res, and so do the first
    eight gate columns of that sample: inf * 0, inf - inf, -0.0 + -0.0."""
    seed = X.shape_seed(B, R, D)
    x, res, mod = X.arbitrary_bf16((B, R, D), seed), X.arbitrary_bf16((B, R, D), seed + 1, 2.0), X.arbitrary_bf16((B, 6 * D), seed + 2)
    inf, nan = float("inf"), float("nan")
    for c0 in range(0, D, 8):
        x[-1, -1, c0:c0 + 8] = torch.tensor([inf, -inf, nan, -0.0, 1.0, 0.0, -0.0, 2.0], dtype=BF)
        res[-1, -1, c0:c0 + 8] = torch.tensor([inf, -inf, 0.0, -0.0, 1.0, nan, -0.0, -0.0], dtype=BF)
    mod[-1, 2 * D:2 * D + 8] = torch.tensor([0.0, 1.0, 1.0, 3.0, inf, -inf, nan, -0.0], dtype=BF)
    want = res + mod[:, 2 * D:3 * D].unsqueeze(1) * x
    assert bits(want[-1, -1, 3]).item() == -32768 and want[-1, -1, 1].item() == -inf and bool(torch.isnan(want[-1, -1, 0]))
    gate = mod.cuda()[:, 2 * D:3 * D]
    what = f"gate_residual B {B} R {R} D {D}"
    dx, dres = strided(x), strided(res, pad_cols=40, col0=16)
    buf, out = framed(B, R, D)
    assert len({dx.stride(1), dres.stride(1), out.stride(1)}) == 3 and gate.stride(0) == 6 * D
    ox, ores = outside_bits(dx), outside_bits(dres)
    ops.gate_residual(dx, gate, dres, out=out)
    check_frame(buf, out, what)
    assert_bits(out, want, what)
    assert torch.equal(bits(dx), bits(x)) and torch.equal(bits(dres), bits(res)), f"{what}: an input changed"
    ops.gate_residual(dx, gate, dres, out=dres)
    assert_bits(dres, want, what + " in place over res")
    assert torch.equal(outside_bits(dres), ores), f"{what}: wrote around res"
    dres.copy_(res)
    ops.gate_residual(dx, gate, dres, out=dx)
    assert_bits(dx, want, what + " in place over x")
    assert torch.equal(outside_bits(dx), ox) and torch.equal(bits(dres), bits(res)), f"{what}: wrote around x"


# ------------------------------------------------------------------------------------------------ copy_rows / scatter_cols
@pytest.mark.parametrize("C", (8, 72))
@pytest.mark.parametrize("R", (1, 37))
def test_copy_rows_and_scatter_cols_move_every_bit_pattern(ops, R, C):
    """copy_rows_kernel / scatter_cols_kernel: one 16-byte chunk per thread.  C 8: one chunk a row | 72: nine; B 2, R 1: 2 / 18 chunks |
    37: 74 / 666 chunks (three workgroups, a partial last one).  Arbitrary bit patterns, NaN payloads included, compared as int16.
    scatter_cols at col0 = 0 and at col0 + C == ld; the other columns of dst keep the canary."""
    B = 2
    src = random_bits((B, R, C), X.shape_seed(R, C))
    dsrc = strided(src)
    buf, dst = framed(B, R, C)
    assert dsrc.stride(1) != dst.stride(1)
    ops.copy_rows_(dsrc, dst)
    check_frame(buf, dst, f"copy_rows R {R} C {C}")
    assert_bits(dst, src, f"copy_rows R {R} C {C}", nan_payload=True)
    ld = 3 * C
    flat = flat_in(src.view(B * R, C))
    for col0 in (0, ld - C):
        what = f"scatter_cols R {R} C {C} col0 {col0}"
        buf, dst = flat_framed((B * R, ld))
        ops.scatter_cols_(flat, dst, col0)
        flat_outside_intact(buf, dst, what)
        got = dst.cpu()
        assert_bits(got[:, col0:col0 + C], src.view(B * R, C), what, nan_payload=True)
        rest = torch.cat([got[:, :col0], got[:, col0 + C:]], 1)
        assert bool((rest == CANARY[BF]).all()), f"{what}: wrote outside its columns"
    assert torch.equal(bits(flat), bits(src.view(B * R, C)))


# ------------------------------------------------------------------------------------------------ timestep_embedding
def run_timestep(t):
    dt = flat_in(t)
    buf, out = flat_framed((t.numel(), 256))
    entry("tfx_timestep_embedding", dt.data_ptr(), out.data_ptr(), t.numel())
    check_frame(buf, out, f"timestep_embedding n {t.numel()}")
    return out.cpu()


def test_timestep_embedding_lies_in_the_window_of_its_fp32_angle():
    """timestep_embedding_kernel: one workgroup of 128 threads per timestep, thread j writes cos at j and sin at 128 + j.  n 7 and each t
    alone (n 1).  t 0: exactly 1 .. 1 | 0 .. 0; t 1e-3: sines of 1e-3 down to 1e-7, which an absolute tolerance cannot see; t 999 / 1000:
    angles that need the full range reduction of sinf / cosf.  Window: X.timestep_window."""
    t = torch.tensor(X.TIMESTEPS)
    lo, hi = X.timestep_window(t)
    got = run_timestep(t)
    X.assert_in_window(got, lo, hi, "timestep_embedding n 7")
    assert bool((got[0, :128] == 1).all()) and bool((bits(got[0, 128:]) == 0).all()), "t = 0 must give 1 .. 1 | +0 .. +0"
    for i in range(t.numel()):
        one = run_timestep(t[i:i + 1])
        X.assert_in_window(one, lo[i:i + 1], hi[i:i + 1], f"timestep_embedding n 1, t {t[i].item()}")
        assert torch.equal(bits(one[0]), bits(got[i])), f"t {t[i].item()}: the row depends on n"


# ------------------------------------------------------------------------------------------------ silu / add
def with_specials(t):
    """t (1-d, bf16) with +-0, +-88, +-inf and NaN at its start and, from 16 elements, at its end (the last workgroup's tail lanes)."""
    sp = torch.tensor([0.0, -0.0, 88.0, -88.0, float("inf"), -float("inf"), float("nan")], dtype=BF)
    if t.numel() >= 16:
        t[:7], t[-7:] = sp, sp.flip(0)
    return t


@pytest.mark.parametrize("n", (1, 255, 256, 257, 1001))
def test_silu_and_add_at_the_workgroup_edges(n):
    """unary_binary_kernel, one element per thread: 1 | one short of, exactly and one past a workgroup | three workgroups and a tail of 233.
    add is torch's bf16 add bit for bit (inf + -inf, -0.0 + -0.0 included).  silu is x / (1 + expf(-x)) in fp32: expf is good to a step or
    two of fp32, the sum and the quotient add one each -- gn_run's derivation (tests/test_exact_rows_gpu.py) for the faster __expf bounds
    the whole at 2^-20 of the value, a quarter of the 2^-18 margin `settled` keeps from a rounding boundary -- so the result is the rounded
    fp64 SiLU wherever that is settled and within one bf16 step elsewhere; silu(-inf) is NaN (inf / inf), as in the reference's x * sigmoid(x)."""
    a = with_specials(X.arbitrary_bf16((n,), X.shape_seed(n), 4.0))
    b = with_specials(X.arbitrary_bf16((n,), X.shape_seed(n, 1), 4.0)).flip(0)
    da, db = flat_in(a), flat_in(b)
    buf, out = flat_framed((n,))
    entry("tfx_add", da.data_ptr(), db.data_ptr(), out.data_ptr(), n)
    check_frame(buf, out, f"add n {n}")
    assert_bits(out, a + b, f"add n {n}")
    buf, out = flat_framed((n,))
    entry("tfx_silu", da.data_ptr(), out.data_ptr(), n)
    check_frame(buf, out, f"silu n {n}")
    got, s64 = out.cpu(), X.silu64(a)
    nan = torch.isnan(s64)
    assert torch.equal(torch.isnan(got), nan), f"silu n {n}: NaN positions"
    zero = torch.zeros_like(got)
    got, want = torch.where(nan, zero, got), torch.where(nan, zero, s64.float().to(BF))
    X.assert_elementwise(got[None], want[None], f"silu n {n}", ulps=1)
    sure = X.settled(s64, 2.0 ** -18) & ~nan
    assert n < 16 or sure.float().mean().item() > 0.9
    assert_bits(torch.where(sure, got, zero), torch.where(sure, want, zero), f"silu n {n} away from a rounding boundary")
    assert torch.equal(bits(da), bits(a))


# ------------------------------------------------------------------------------------------------ select_step / advance_step
@pytest.mark.parametrize("per", (8, 8 * 257, 8 * (2048 * 256 + 1)))
def test_select_step_follows_the_device_cursor(ops, per):
    """select_step_kernel copies 16-byte chunks in a grid-stride loop under a grid capped at 2048 workgroups: 1 chunk | 257 (two workgroups,
    one thread in the second) | 2048 * 256 + 1, the first size at which a thread takes a second trip (8 MB a step; the modulation table
    reaches it at batch 4).  The cursor is read from device memory, 0 and then 1 after advance_step_kernel; arbitrary bit patterns."""
    table = random_bits((2, per), X.shape_seed(per)).cuda()
    keep = table.clone()
    ptr = torch.zeros(1, dtype=torch.int32, device="cuda")
    buf, cur = flat_framed((per,))
    for step in (0, 1):
        ops.select_step_(table, cur, ptr)
        assert ptr.item() == step, "select_step must not move the cursor"
        flat_outside_intact(buf, cur, f"select_step per {per} step {step}")
        assert torch.equal(cur.view(torch.int16), keep[step].view(torch.int16)), f"select_step per {per}: cur is not table[{step}]"
        ops.advance_step_(ptr)
        assert ptr.item() == step + 1, "advance_step must add one"
    assert torch.equal(table.view(torch.int16), keep.view(torch.int16)), "the table changed"


# ------------------------------------------------------------------------------------------------ any_negative
@pytest.mark.parametrize("dtype", (torch.float32, BF))
def test_any_negative_sees_the_last_element_and_nothing_else(ops, dtype):
    """any_negative_kernel<float | bf16>: a grid-stride loop under a grid capped at 4096 workgroups.  n 1 | 257 (a second workgroup with one
    thread) | 4096 * 256 + 1: the one element only a second trip reaches, and it holds the only negative.  -0.0 and NaN are not negative; a
    flag that is set stays set.  The input lies between negative numbers: a read outside it would set the flag."""
    for n in (1, 257, 4096 * 256 + 1):
        x = (torch.rand(n, generator=X.gen(n)) + 0.5).to(dtype)
        if n > 1:
            x[3], x[n // 2], x[0] = -0.0, float("nan"), 0.0
        variants = [x] if n > 1 else [x, torch.tensor([-0.0], dtype=dtype), torch.tensor([float("nan")], dtype=dtype)]
        for v in variants:
            dx = flat_in(v, fill=-1.0)
            flag = torch.zeros(1, dtype=torch.int32, device="cuda")
            assert ops.any_negative(dx, flag) is flag and flag.item() == 0, f"n {n} {dtype}: flag set without a negative ({v[:4].tolist()})"
        dx[-1] = -2.0 ** -100
        ops.any_negative(dx, flag)
        assert flag.item() == 1, f"n {n} {dtype}: the negative last element was not seen"
        dx[-1] = 1.0
        ops.any_negative(dx, flag)
        assert flag.item() == 1, f"n {n} {dtype}: a set flag was cleared"
        fresh = torch.zeros(1, dtype=torch.int32, device="cuda")
        ops.any_negative(dx, fresh)
        assert fresh.item() == 0


# ------------------------------------------------------------------------------------------------ prep_image
DT = {torch.float32: 0, BF: 1, torch.uint8: 2}
KIND = {"f32": torch.float32, "bf16": BF, "u8": torch.uint8}


def unit(t):
    """uint8 / 255 as the correctly rounded fp32 quotient; float tensors as fp32."""
    return (t.double() / 255.0).float() if t.dtype == torch.uint8 else t.float()


def mask_values(shape, dtype, binarize, seed):
    """Binarise on: the values either side of and at the threshold (float 0, nextafter(0.5, 0), 0.5, 1; uint8 0, 127, 128, 255); off:
    fractional values."""
    g = X.gen(seed)
    if dtype == torch.uint8:
        return torch.tensor([0, 127, 128, 255], dtype=torch.uint8)[torch.randint(0, 4, shape, generator=g)] if binarize else \
            torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)
    below = float(np.nextafter(np.float32(0.5), np.float32(0.0)))
    return torch.tensor([0.0, below, 0.5, 1.0])[torch.randint(0, 4, shape, generator=g)] if binarize else torch.rand(shape, generator=g)


def mask_weight(mask, binarize):
    m = unit(mask)
    return torch.where(m < 0.5, 0.0, 1.0) if binarize else m


@pytest.mark.parametrize("mask_kind", ("f32", "u8", "none"))
@pytest.mark.parametrize("img_kind", ("f32", "bf16", "u8"))
def test_prep_image_every_instantiation_channel_count_and_mode(img_kind, mask_kind):
    """prep_image_kernel<image, mask>, one pixel (eight output channels, one 16-byte store) per thread: all six instantiations and the
    null-mask branch.  C 1, 3, 4, 8: the `c < C` zero fill, +0 exactly.  (B, H, W) (2, 5, 7): 70 pixels, one partial workgroup | (3, 9, 31):
    837, three full and a tail of 69.  Mask batch 1 and B; norm_mode 0, 1, and 2 with the device flag clear and set; binarise at the
    threshold's neighbours, and off with fractional masks.  Bit-equal to bf16(norm(img) * (1 - m)) in torch fp32."""
    idt, mdt = KIND[img_kind], KIND.get(mask_kind)
    flags = {v: torch.full((1,), v, dtype=torch.int32, device="cuda") for v in (0, 1)}
    for B, H, W in ((2, 5, 7), (3, 9, 31)):
        for C in (1, 3, 4, 8):
            seed = X.shape_seed(B, H, W, C)
            if idt == torch.uint8:
                img = torch.randint(0, 256, (B, H, W, C), generator=X.gen(seed), dtype=torch.uint8)
                planes = unit(img).permute(0, 3, 1, 2)
            else:
                img = (torch.rand(B, C, H, W, generator=X.gen(seed)) * 2 - 1).to(idt)
                planes = unit(img)
            dimg = flat_in(img)
            for mb, binarize in [(mb, bz) for mb in (1, B) for bz in (1, 0)] if mdt is not None else [(1, 1)]:
                keep, dmask = torch.ones(1, 1, H, W), None
                if mdt is not None:
                    mask = mask_values((mb, H, W), mdt, binarize, seed + 10 * mb + binarize)
                    keep, dmask = 1.0 - mask_weight(mask, binarize)[:, None], flat_in(mask)
                for mode, flag in ((0, None), (1, None), (2, 0), (2, 1)):
                    what = f"prep_image {img_kind} / {mask_kind} B {B} H {H} W {W} C {C} mask batch {mb} binarise {binarize} norm {mode} flag {flag}"
                    x = 2.0 * planes - 1.0 if mode == 1 or (mode == 2 and flag == 0) else planes
                    want = (x * keep).to(BF).permute(0, 2, 3, 1)
                    buf, out = flat_framed((B, H, W, 8))
                    entry("tfx_prep_image", dimg.data_ptr(), DT[idt], dmask.data_ptr() if dmask is not None else None, DT[mdt] if mdt else 0,
                          out.data_ptr(), B, C, H, W, mb, mode, binarize, flags[flag].data_ptr() if flag is not None else None)
                    check_frame(buf, out, what)
                    assert_bits(out[..., :C], want, what)
                    assert bool((bits(out[..., C:]) == 0).all()), f"{what}: channels {C} .. 7 are not +0"
    assert flags[0].item() == 0 and flags[1].item() == 1


# ------------------------------------------------------------------------------------------------ pack_mask
@pytest.mark.parametrize("mask_kind", ("f32", "u8"))
def test_pack_mask_is_the_reference_rearrangement_inside_its_columns(ops, mask_kind):
    """pack_mask_kernel<float | uint8>, one token x 8 packed columns per thread (32 threads a token).  (16, 16): one token a sample, 64 threads
    of one workgroup | (48, 32): six tokens a sample, 384 threads: a second, half-filled workgroup, and w2 = 2 != h2 = 3.  Mask batch 1 and
    B = 2; col0 0 and 64 of ld 320 (the other columns keep the canary); binarise at the threshold's neighbours, and off."""
    B, ld, mdt = 2, 320, KIND[mask_kind]
    for H, W in ((16, 16), (48, 32)):
        S = (H // 16) * (W // 16)
        for mb in (1, B):
            for binarize in (1, 0):
                mask = mask_values((mb, H, W), mdt, binarize, X.shape_seed(H, W, mb, binarize))
                want = po.pack_mask(mask_weight(mask, binarize).expand(B, H, W)[:, None].contiguous()).to(BF)
                assert want.shape == (B, S, 256)
                dmask = flat_in(mask)
                for col0 in (0, 64):
                    what = f"pack_mask {mask_kind} H {H} W {W} mask batch {mb} binarise {binarize} col0 {col0}"
                    buf, out = flat_framed((B, S, ld))
                    ops.pack_mask(dmask, out, col0, B, H, W, bool(binarize))
                    flat_outside_intact(buf, out, what)
                    got = out.cpu()
                    assert_bits(got[..., col0:col0 + 256], want, what)
                    assert bool((torch.cat([got[..., :col0], got[..., col0 + 256:]], -1) == CANARY[BF]).all()), f"{what}: wrote outside its columns"


# ------------------------------------------------------------------------------------------------ sample_pack
@pytest.mark.parametrize("B,h,w,L", X.SAMPLE_PACK_CASES)
def test_sample_pack_mode_and_the_three_forms_of_eps(ops, B, h, w, L):
    """sample_pack_kernel<bf16 | float>, one token x 8 packed columns (two channels x four positions) per thread.  (1, 2, 2, 2): one token, one
    thread | (2, 6, 10, 16): 30 tokens x 8 threads = 240, w2 = 5 != h2 = 3.  Log-variances beyond both ends of the clamp [-30, 20].  eps
    none: the mode, bit-equal to the chain | bf16 | fp32 holding bf16 values: the same bits as the bf16 run | fp32 that bf16 does not hold:
    rounded to bf16 first.  With eps the one freedom is expf: bit-equal to the chain where exp64 is settled at 2^-18, elsewhere the chain
    with std or one of its two bf16 neighbours (tests/test_exact_inputs_cpu.py: settled on more than 99 % of these inputs)."""
    cs = X.sample_pack_case(B, h, w, L)
    S, ld = (h // 2) * (w // 2), 320
    mom = flat_in(torch.cat([cs["mean"], cs["logvar"]], 1).permute(0, 2, 3, 1).contiguous())
    std64 = X.sample_pack_std64(cs["logvar"])
    std = std64.float().to(BF)
    sure = po.pack_latents(X.settled(std64, 2.0 ** -18))
    for col0 in (0, 64):
        def run(eps):
            what = f"sample_pack B {B} h {h} w {w} L {L} col0 {col0} eps {None if eps is None else eps.dtype}"
            buf, out = flat_framed((B, S, ld))
            ops.vae_sample_pack(mom, flat_in(eps) if eps is not None else None, out, col0, SHIFT, SCALE)
            flat_outside_intact(buf, out, what)
            got = out.cpu()
            assert bool((torch.cat([got[..., :col0], got[..., col0 + 4 * L:]], -1) == CANARY[BF]).all()), f"{what}: wrote outside its columns"
            return got[..., col0:col0 + 4 * L].contiguous(), what

        got, what = run(None)
        assert_bits(got, X.sample_pack_chain(cs["mean"], None, None, SHIFT, SCALE), what)
        runs = {}
        for name, eps, eps_bf in (("bf16", cs["eps"], cs["eps"]), ("f32 of bf16 values", cs["eps"].float(), cs["eps"]),
                                  ("f32", cs["eps32"], cs["eps32"].to(BF))):
            got, what = run(eps)
            runs[name] = got
            chains = [X.sample_pack_chain(cs["mean"], s, eps_bf, SHIFT, SCALE) for s in (std, X.bf16_neighbour(std, -1), X.bf16_neighbour(std, 1))]
            zero = torch.zeros_like(got)
            assert_bits(torch.where(sure, got, zero), torch.where(sure, chains[0], zero), what + " where exp is settled")
            ok = (bits(got) == bits(chains[0])) | (bits(got) == bits(chains[1])) | (bits(got) == bits(chains[2]))
            assert bool(ok.all()), f"{what}: {int((~ok).sum())} elements are not the chain with std or a neighbour of it, first {(~ok).nonzero()[0].tolist()}"
        assert torch.equal(bits(runs["bf16"]), bits(runs["f32 of bf16 values"])), "fp32 eps holding bf16 values must give the bf16-eps bits"
        assert not torch.equal(bits(runs["bf16"]), bits(runs["f32"]))


# ------------------------------------------------------------------------------------------------ unpack_latents
@pytest.mark.parametrize("L", (8, 16, 32))
def test_unpack_latents_with_a_wider_token_row(L):
    """unpack_latents_kernel, one pixel x 8 channels per thread, gathering every fourth column of a token row.  L 8: one thread a pixel | 16,
    32: two, four.  (h, w) (2, 2): one token a sample | (10, 14): 35 tokens, 140 pixels a sample, w2 = 7.  lat contiguous (ld = 4 L) and
    the first 4 L columns of a NaN-filled [B, S, 384] buffer (ld = 384: the x_embedder input the pipeline could hand over).  (shift, scale)
    the VAE's and (0, 1): the bare layout."""
    from tests.test_imageops_gpu import dev_scalar
    B = 2
    for h, w in ((2, 2), (10, 14)):
        S = (h // 2) * (w // 2)
        lat = X.arbitrary_bf16((B, S, 4 * L), X.shape_seed(L, h, w), 2.0)
        wide = torch.full((B, S, 384), float("nan"), dtype=BF, device="cuda")
        wide[..., :4 * L] = lat
        for shift, scale in ((SHIFT, SCALE), (0.0, 1.0)):
            want = dev_scalar(dev_scalar(po.unpack_latents(lat, 8 * h, 8 * w), "div", scale), "add", shift).permute(0, 2, 3, 1)
            for dlat, ld in ((flat_in(lat), 4 * L), (wide[..., :4 * L], 384)):
                what = f"unpack_latents L {L} h {h} w {w} ld {ld} shift {shift} scale {scale}"
                buf, out = flat_framed((B, h, w, L))
                entry("tfx_unpack_latents", dlat.data_ptr(), ld, out.data_ptr(), B, h, w, L, shift, scale)
                check_frame(buf, out, what)
                assert_bits(out, want, what)


# ------------------------------------------------------------------------------------------------ postprocess
POST_SPECIALS = (0.0, 1.0, -1.0, 1.0078125, -1.0078125, 3.0, -3.0)      # 0 -> 0.5 -> 127.5 -> 128 (half to even); 1.0078125 / 2 + 0.5 rounds in bf16


@pytest.mark.parametrize("denorm", (1, 0))
@pytest.mark.parametrize("mode", (0, 1, 2, 3))
def test_postprocess_every_mode_and_crop_window(mode, denorm):
    """postprocess_kernel, one output pixel (C channels, scalar stores) per thread; modes NCHW bf16 | NHWC fp32 | NHWC uint8 | NCHW fp32, with
    and without denormalisation (uint8 without it on values already in [0, 1]).  (B, H, W, Cs, C) (2, 5, 7, 8, 3) | (1, 9, 31, 8, 8): 279
    pixels, a second workgroup of 23 | (2, 4, 4, 16, 1): one channel of sixteen.  Crops: the whole image | the pixel (0, 0) | the pixel
    (W - 1, H - 1) | a window touching the right and bottom edges.  The corner pixels hold 0 (the 127.5 -> 128 tie), +-1, +-1.0078125, +-3."""
    odt = {0: BF, 1: torch.float32, 2: torch.uint8, 3: torch.float32}[mode]
    sp = torch.tensor(POST_SPECIALS, dtype=BF)
    for B, H, W, Cs, C in ((2, 5, 7, 8, 3), (1, 9, 31, 8, 8), (2, 4, 4, 16, 1)):
        x = X.arbitrary_bf16((B, H, W, Cs), X.shape_seed(B, H, W, Cs, C))
        x.view(-1)[torch.randperm(x.numel(), generator=X.gen(5))[:70]] = sp.repeat(10)
        x[0, 0, 0, :7], x[-1, -1, -1, :7] = sp, sp
        if mode == 2 and not denorm:
            x = x.float().abs().clamp(max=1.0).to(BF)
        dx = flat_in(x)
        for x0, y0, x1, y1 in ((0, 0, W, H), (0, 0, 1, 1), (W - 1, H - 1, W, H), (W // 2, H // 2, W, H)):
            what = f"postprocess mode {mode} denorm {denorm} B {B} H {H} W {W} Cs {Cs} C {C} crop {(x0, y0, x1, y1)}"
            v = x[:, y0:y1, x0:x1, :C]
            if denorm:
                v = (v / 2 + 0.5).clamp(0, 1)
            nchw = mode in (0, 3)
            v = (v.permute(0, 3, 1, 2) if nchw else v).contiguous()
            buf, out = flat_framed(tuple(v.shape), odt)
            entry("tfx_postprocess", dx.data_ptr(), out.data_ptr(), B, H, W, Cs, C, mode, denorm, y0, x0, y1 - y0, x1 - x0)
            check_frame(buf, out, what)
            if mode == 0:
                assert_bits(out, v, what)
            elif mode == 2:
                want = torch.from_numpy(np.round(v.float().numpy() * np.float32(255.0)).astype(np.uint8))
                assert torch.equal(out.cpu(), want), f"{what}: {(out.cpu() != want).nonzero()[:4].tolist()}"
                assert not denorm or (x0, y0) != (0, 0) or out[0, 0, 0, 0].item() == 128, f"{what}: 0 -> 127.5 must round to the even 128"
            else:
                assert torch.equal(out.cpu().view(torch.int32), v.float().view(torch.int32)), f"{what}: {(out.cpu() != v.float()).nonzero()[:4].tolist()}"


# ------------------------------------------------------------------------------------------------ transpose
@pytest.mark.parametrize("N,C", ((1, 1), (63, 65), (64, 64), (65, 63), (100, 72), (130, 8)))
def test_transpose_at_the_tile_edges(ops, N, C):
    """transpose_kernel, 64 x 64 tiles through LDS with both bounds guarded on load and store: one element | one short of a tile one way and
    one past it the other, both ways | exactly one tile | the VAE's (100, 72) | three row tiles of a narrow matrix.  Input pitch > C, output
    pitch > N, gaps between the two samples on both sides; arbitrary bit patterns compared as int16."""
    B = 2
    x = random_bits((B, N, C), X.shape_seed(N, C))
    dx = strided(x)
    buf, out = framed(B, C, N)
    assert dx.stride(1) > C and out.stride(1) > N and dx.stride(0) > N * dx.stride(1) and out.stride(0) > C * out.stride(1)
    ops.transpose(dx, out)
    check_frame(buf, out, f"transpose N {N} C {C}")
    assert_bits(out, x.transpose(1, 2), f"transpose N {N} C {C}", nan_payload=True)
