"""Exact-input tests of the matrix-pipe kernels: every output element of every GEMM, convolution and attention form against the ONE bf16
value the inputs of tests/helpers/exact_inputs.py allow (tests/test_exact_inputs_cpu.py proves the constructions and their
sensitivity without a GPU).  fp32 sums these operands exactly in any order, so nothing is budgeted for the summation order: comparisons
are per element against a CPU restatement -- `ulps=0` unless a docstring derives one bf16 step from the kernel's code -- and a failure
names the batch, row, column and 256 x 256 tile of the first differing elements.  Tests that claim a launch form assert it from the
library's counters, or from the plan the device's CU count implies (skipped, never passed, where the device gives another form)."""
import pytest
import torch

from tests.helpers import exact_inputs as X
from tests.helpers import framing

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
SENTINEL = -1024.0            # no expected value comes near it


@pytest.fixture(scope="module")
def ops():
    from textflux_amd import ops as o
    return o


def grid_of_device():
    """Workgroups of the persistent kernels (launch.cpp::device_facts): one per CU, a whole number of eights."""
    return torch.cuda.get_device_properties(0).multi_processor_count & ~7


def epilogue_operands(B, M, N, seed):
    return X.gates(B, N, seed + 11), X.arbitrary_bf16((B, M, N), seed + 12)


def check_epilogue(got, epi, lin, res, gate, gelu_from, what):
    """got against the chain of `epi` on the exact Linear output lin.  GELU columns: one bf16 step against the fp64 tanh-GELU of the exact
    pre-activation -- common.h::gelu_tanh evaluates x * (rcp(exp2(z - 32) + 2^-32) * 2^-32), z = x * fma(x * x, c1, c0): no cancelling
    subtraction, and v_exp_f32 / v_rcp_f32 are accurate to ~1e-6 relative, far inside half a bf16 step (2e-3), so the device value can only
    land on the other side of a rounding boundary the fp64 value sits next to -- and bit-equal where that value is 0 or x itself.  The
    scale of 2^-32 keeps both transcendental results normal (they flush subnormals) down to values that round to zero: the fp8 cases' scaled
    pre-activations reach x in [-10.4, -10.0], where GELU is 1e-37 .. 1e-40 and the unscaled form returned -0, four and more bf16 steps away."""
    want = X.chain(epi, lin, res=res, gate=gate, gelu_from_col=gelu_from)
    got = got.cpu()
    if epi != 1:
        return X.assert_elementwise(got, want, what)
    exact = X.gelu_exact_mask(lin, gelu_from)
    X.assert_elementwise(torch.where(exact, got, want), want, what + " (plain columns, GELU = 0 or x)")
    return X.assert_elementwise(got, want, what + " (GELU columns)", ulps=1)


# ----------------------------------------------------------------------------------------------------------------- GEMM, bf16
def with_variants(shapes):
    """(B, M, N, K, variant) for the kernel forms that take the shape: 0 generic, 1 auto MFMA, 2 one-tile, 3 persistent (K % 128 == 0 only,
    tests/test_kernels_gpu.py::test_gemm_persistent_rejects_odd_k_tiles)."""
    return [(*s, v) for s in shapes for v in (0, 1, 2, 3) if v != 3 or s[3] % 128 == 0]


@pytest.mark.parametrize("B,M,N,K,variant", with_variants(X.GEMM_EPI_SHAPES + [X.GEMM_ROUNDING_SHAPE]))
def test_gemm_epilogue_chains_per_element(ops, B, M, N, K, variant):
    """Epilogues 0, 1, 2, 3 of every kernel form (0 generic FMA, 1 auto MFMA, 2 one-tile, 3 persistent where K % 128 == 0) against the
    header's rounding chain on the exact integer product; A and C are column slices of wider buffers whose other bytes must stay, res
    aliases C.  The K = 12288 shape is the one at which epilogue 2's intermediate rounding bf16(gate * lin) is observable."""
    seed = X.shape_seed(B, M, N, K)
    cs = X.gemm_operands(B, M, N, K, seed)
    gate, res = epilogue_operands(B, M, N, seed)
    lin = X.linear_bf16(cs["acc"], cs["bias"].float())
    gf = 256 if N > 256 else 0
    abuf = torch.full((B, M, K + 64), 3.0, dtype=BF, device="cuda")
    abuf[:, :, 64:] = cs["a"].cuda()
    a, w, bias = abuf[:, :, 64:], cs["w"].cuda(), cs["bias"].cuda()
    for epi in (0, 1, 2, 3):
        cbuf = torch.full((B, M, N + 136), SENTINEL, dtype=BF, device="cuda")
        out = cbuf[:, :, 128:128 + N]
        kw = {}
        if epi in (2, 3):
            out.copy_(res.cuda())
            kw = dict(res=out, gate=gate.cuda()) if epi == 2 else dict(res=out)
        ops.gemm(a, w, bias, out=out, epilogue=epi, gelu_from_col=gf, variant=variant, **kw)
        check_epilogue(out, epi, lin, res, gate, gf, f"gemm variant {variant} epilogue {epi} ({B}, {M}, {N}, {K})")
        assert (cbuf[:, :, :128] == SENTINEL).all() and (cbuf[:, :, 128 + N:] == SENTINEL).all(), "bytes outside the C slice were written"
    assert (abuf[:, :, :64] == 3.0).all() and torch.equal(abuf[:, :, 64:].cpu(), cs["a"])


@pytest.mark.parametrize("K", X.GEMM_KSLICE_KS)
def test_gemm_whole_k_slicing_is_exact(ops, K):
    """(1, 300, 520, K): 6 tiles, fewer than CUs, so with a workspace the auto path cuts every tile into 2 / 3 / 4 / 6 / 8 K slices (fp32
    partials, summed by tail_reduce_kernel, then the epilogue).  Every epilogue must give the chain's bits, which are also the unsliced
    persistent kernel's -- where Gaussian inputs allow 2 % of one-step flips."""
    B, M, N = X.GEMM_KSLICE_BMN
    want_slices = X.GEMM_KSLICE[K]
    ws = torch.empty(X.GEMM_WS_BYTES, dtype=torch.uint8, device="cuda")
    plan = X.plan_slices_bf16(B, M, N, K, ws.numel(), grid_of_device())
    if plan[0] != want_slices:
        pytest.skip(f"this device plans {plan[0]} slices at K = {K}, not {want_slices}")
    seed = X.shape_seed(B, M, N, K)
    cs = X.gemm_operands(B, M, N, K, seed)
    gate, res = epilogue_operands(B, M, N, seed)
    lin = X.linear_bf16(cs["acc"], cs["bias"].float())
    a, w, bias = cs["a"].cuda(), cs["w"].cuda(), cs["bias"].cuda()
    for epi in (0, 1, 2, 3):
        kw = dict(res=res.cuda(), gate=gate.cuda()) if epi == 2 else dict(res=res.cuda()) if epi == 3 else {}
        sliced = ops.gemm(a, w, bias, epilogue=epi, gelu_from_col=256, variant=1, workspace=ws, **kw)
        check_epilogue(sliced, epi, lin, res, gate, 256, f"K-sliced gemm ({want_slices} slices) epilogue {epi}")
        X.assert_elementwise(sliced, ops.gemm(a, w, bias, epilogue=epi, gelu_from_col=256, variant=3, **kw), f"sliced vs persistent, epilogue {epi}")


def test_gemm_k_slicing_keeps_identical_samples_identical(ops):
    B, M, N, K = 2, 300, 520, 1024
    ws = torch.empty(X.GEMM_WS_BYTES, dtype=torch.uint8, device="cuda")
    if X.plan_slices_bf16(B, M, N, K, ws.numel(), grid_of_device())[0] != 2:
        pytest.skip("this device does not slice 12 tiles in two")
    seed = X.shape_seed(1, M, N, K)
    cs = X.gemm_operands(1, M, N, K, seed)
    gate, res = epilogue_operands(1, M, N, seed)
    lin = X.linear_bf16(cs["acc"], cs["bias"].float()).expand(B, M, N)
    gate2, res2 = gate.expand(B, N).contiguous(), res.expand(B, M, N).contiguous()
    a, w, bias = cs["a"].expand(B, M, K).contiguous().cuda(), cs["w"].cuda(), cs["bias"].cuda()
    for epi in (0, 2):
        kw = dict(res=res2.cuda(), gate=gate2.cuda()) if epi == 2 else {}
        got = ops.gemm(a, w, bias, epilogue=epi, variant=1, workspace=ws, **kw)
        check_epilogue(got, epi, lin, res2, gate2, 0, f"B = 2 K-sliced gemm epilogue {epi}")
        assert torch.equal(got[0], got[1])


def test_gemm_sliced_last_round_is_exact(ops):
    """(1, 4096, 9216, 1024): 576 tiles = two rounds of 256 CUs + 64 tiles, which the auto path cuts into two K slices each.  Reference: a
    torch fp32 matmul ON THE DEVICE -- exact for these operands in any order and any internal blocking, every partial sum being an integer of
    magnitude <= 1024 < 2^24 -- whose rows 61 + 256 i, 125 + 256 i, 189 + 256 i, 253 + 256 i of every row tile (64 rows: each of the 576
    tiles, the sliced ones included) are recomputed in fp64 on the CPU."""
    B, M, N, K = X.GEMM_TAIL_SHAPE
    ws = torch.empty(X.GEMM_WS_BYTES, dtype=torch.uint8, device="cuda")
    grid = grid_of_device()
    plan = X.plan_slices_bf16(B, M, N, K, ws.numel(), grid)
    if plan != (2, 512, 64):
        pytest.skip(f"this device ({grid} persistent workgroups) plans {plan}, not 2 slices of the last 64 tiles")
    seed = X.shape_seed(B, M, N, K)
    cs = X.gemm_operands(B, M, N, K, seed, product=False)
    a, w, bias = cs["a"].cuda(), cs["w"].cuda(), cs["bias"].cuda()
    acc = a[0].float() @ w.float().T
    assert (acc == acc.round()).all() and (acc + bias.float()).abs().max().item() <= X.ACC_LIMIT and acc.abs().max().item() <= X.ACC_LIMIT
    rows = torch.tensor([r + 256 * i for i in range(16) for r in (61, 125, 189, 253)])
    assert torch.equal(acc[rows.cuda()].cpu().double(), cs["a"][0, rows].double() @ cs["w"].double().T)
    lin = (acc + bias.float()).to(BF)[None]
    gate, res = X.gates(B, N, seed + 11).cuda(), X.arbitrary_bf16((B, M, N), seed + 12).cuda()
    for epi in (0, 2):
        kw = dict(res=res, gate=gate) if epi == 2 else {}
        want = lin if epi == 0 else res + gate[:, None, :] * lin                       # torch's bf16 operators on the device: each rounds once
        got = ops.gemm(a, w, bias, epilogue=epi, variant=1, workspace=ws, **kw)
        X.assert_elementwise(got, want, f"sliced last round, epilogue {epi}")


@pytest.mark.parametrize("B,M,N,K", X.GEMM_F32_SHAPES)
def test_gemm_f32_returns_the_exact_integer_product(ops, B, M, N, K):
    seed = X.shape_seed(B, M, N, K)
    cs = X.gemm_operands(B, M, N, K, seed)
    X.assert_elementwise(ops.gemm_f32(cs["a"].cuda(), cs["w"].cuda()), cs["acc"].float(), "gemm_f32")
    if B > 1:
        cb = X.gemm_operands(B, M, N, K, seed, w_batched=True)
        want = cb["acc"].float()
        X.assert_elementwise(ops.gemm_f32(cb["a"].cuda(), cb["w"].cuda()), want, "gemm_f32, per-batch weights")
        wv = torch.full((B, N, K + 64), 5.0, dtype=BF, device="cuda")[:, :, :K]          # row and batch pitch of their own
        wv.copy_(cb["w"].cuda())
        X.assert_elementwise(ops.gemm_f32(cb["a"].cuda(), wv), want, "gemm_f32, strided per-batch weights")
        obuf = torch.full((B, M, N + 9), SENTINEL, dtype=torch.float32, device="cuda")
        ops.gemm_f32(cb["a"].cuda(), wv, out=obuf[:, :, :N])
        X.assert_elementwise(obuf[:, :, :N], want, "gemm_f32, strided output")
        assert (obuf[:, :, N:] == SENTINEL).all()


@pytest.mark.parametrize("B,M,N,K,variant", with_variants(X.GEMM_COLSCALE_SHAPES))
def test_gemm_column_scale_epilogue_is_exact(ops, B, M, N, K, variant):
    """Epilogue 4, bf16(cscale[n] * acc): a power-of-two factor times an integer is exact, the stored value is rounded once."""
    seed = X.shape_seed(B, M, N, K)
    cs = X.gemm_operands(B, M, N, K, seed)
    cscale = X.pow2((N,), -3, 3, seed + 5)
    got = ops.gemm(cs["a"].cuda(), cs["w"].cuda(), None, epilogue=ops.EPI_COLSCALE, cscale=cscale.cuda(), variant=variant)
    X.assert_elementwise(got, X.linear_bf16(cs["acc"], col_scale=cscale), f"column-scale epilogue, variant {variant}")


# ----------------------------------------------------------------------------------------------------------------- runtime LoRA tail
def lora_device(ops, cs, R, K, which=(0,), stacked=False):
    """The operands on the device as tfx_gemm_bf16_lora wants them placed.  stacked: one T matrix per segment (t_seg_stride)."""
    x, T, nseg = cs["x"], cs["T"], cs["nseg"]
    B, M, _ = x.shape
    if stacked:
        buf = torch.zeros(1 + nseg, B, M, max(K, R), dtype=BF, device="cuda")
        buf[0][..., :K] = x.cuda()
        for s in range(nseg):
            buf[1 + s][..., :R] = T[s].cuda()
        xv, tv = buf[0][..., :K], buf[1][..., :R]
    else:
        buf, xv, tv = ops.lora_operands(x.to(BF).cuda(), nseg * R)
        for s in range(nseg):
            tv[..., s * R:(s + 1) * R] = T[s].cuda()
    wb = torch.zeros(len(which), cs["W"].shape[1], K + R, dtype=BF, device="cuda")
    for i, j in enumerate(which):
        wb[i, :, :K], wb[i, :, K:] = cs["W"][j].cuda(), cs["Bm"][j].cuda()
    return buf, xv, tv, wb


@pytest.mark.parametrize("R", X.LORA_RS)
@pytest.mark.parametrize("M", X.LORA_MS)
def test_gemm_lora_tail_is_one_exact_accumulation(ops, M, R):
    """epi(x W^T + T_seg Bm^T + bias) with ternary T and Bm: ONE exact accumulation over K + R.  Every segment's T block and Bm rows come
    from their own seed, so a tile that reads its neighbour's operands stores wrong integers.  Covered: all four epilogues, one segment
    masked (its garbage tail must not arrive), one T matrix per segment (t_seg_stride), and the fused q / k norm + RoPE epilogue."""
    N, K = X.LORA_NK
    B, nseg = 2, 3
    seed = X.shape_seed(M, N, K, R)
    cs = X.lora_case(M, N, K, R, B, nseg, seed)
    gate, res = epilogue_operands(B, M, N, seed)
    bias = cs["bias"][0]
    kw = dict(K=K, R=R, seg_cols=N // nseg, nseg=nseg, bias=bias.to(BF).cuda())
    _, xv, tv, wb = lora_device(ops, cs, R, K)
    for mask in (0b111, 0b101):
        lin = X.linear_bf16(X.lora_acc(cs, mask), bias)
        for epi in (0, 1, 2, 3):
            ekw = dict(res=res.cuda(), gate=gate.cuda()) if epi == 2 else dict(res=res.cuda()) if epi == 3 else {}
            got = ops.gemm_lora(xv, tv, wb[0], seg_mask=mask, epilogue=epi, gelu_from_col=512, **ekw, **kw)
            check_epilogue(got, epi, lin, res, gate, 512, f"gemm_lora M {M} R {R} mask {mask:03b} epilogue {epi}")
    lin = X.linear_bf16(X.lora_acc(cs, 0b111), bias)
    stack, xs, ts, _ = lora_device(ops, cs, R, K, stacked=True)
    got = ops.gemm_lora(xs, ts, wb[0], seg_mask=0b111, t_seg_stride=stack.stride(0), **kw)
    X.assert_elementwise(got, lin, f"gemm_lora M {M} R {R}, one T matrix per segment")
    wq, wk, tab = X.norm_weights(seed + 1), X.norm_weights(seed + 2), X.rope_table(M, seed + 3)
    q = dict(norm_q=wq.cuda(), norm_k=wk.cuda(), rope_cs=tab.cuda(), q_range=(512, 768), k_range=(0, 256))
    want = X.qk_norm_rope(lin, ((512, 768), (0, 256)), (wq, wk), tab)
    fused = ops.gemm_lora(xv, tv, wb[0], seg_mask=0b111, qkn=q, **kw)
    X.assert_elementwise(fused, want, f"gemm_lora M {M} R {R}, fused q / k norm", ulps=1, cap=4 * X.QKN_SHARE_ONE_ULP)


@pytest.mark.parametrize("fused_norm", [False, True])
@pytest.mark.parametrize("R", X.LORA_RS)
def test_gemm_lora_row_split_takes_the_second_weight_set(ops, R, fused_norm):
    """Rows below split_row take W2 / bias2 / Bm2 (/ norm weights 2) and their own segment mask: exact integers from another seed."""
    (N, K), M, B, nseg, split = X.LORA_NK, 1664, 2, 3, 256
    seed = X.shape_seed(M, N, K, R, 2)
    cs = X.lora_case(M, N, K, R, B, nseg, seed, sets=2)
    _, xv, tv, wb = lora_device(ops, cs, R, K, which=(0, 1))
    img = X.linear_bf16(X.lora_acc(cs, 0b101, 0), cs["bias"][0])
    txt = X.linear_bf16(X.lora_acc(cs, 0b010, 1), cs["bias"][1])
    w = [X.norm_weights(seed + i) for i in range(4)]
    tab = X.rope_table(M, seed + 5)
    q, second = None, dict(wb=wb[1], bias=cs["bias"][1].to(BF).cuda())
    if fused_norm:
        rg = ((512, 768), (0, 256))
        img, txt = X.qk_norm_rope(img, rg, (w[0], w[1]), tab), X.qk_norm_rope(txt, rg, (w[2], w[3]), tab)
        q = dict(norm_q=w[0].cuda(), norm_k=w[1].cuda(), rope_cs=tab.cuda(), q_range=rg[0], k_range=rg[1])
        second.update(norm_q=w[2].cuda(), norm_k=w[3].cuda())
    want = torch.cat([txt[:, :split], img[:, split:]], 1)
    got = ops.gemm_lora(xv, tv, wb[0], K=K, R=R, seg_cols=N // nseg, nseg=nseg, seg_mask=0b101 | (0b010 << 8), bias=cs["bias"][0].to(BF).cuda(),
                        qkn=q, split_row=split, second=second)
    X.assert_elementwise(got, want, f"row-split gemm_lora R {R}", ulps=1 if fused_norm else 0, cap=4 * X.QKN_SHARE_ONE_ULP if fused_norm else None)


# ----------------------------------------------------------------------------------------------------------------- GEMM, fp8
@pytest.mark.parametrize("B,M,N,K", X.GEMM_FP8_SHAPES)
def test_gemm_fp8_is_exact_on_ternary_codes(ops, B, M, N, K):
    """The same ternary values as e4m3 bytes, power-of-two row and channel scales: acc * s_a * s_w + bias is an fp32 number (asserted),
    rounded once; epilogues 0, 1, 2, 3, with and without a workspace.  These shapes have two and four 128-byte K-tiles and a slice keeps
    eight, so they are NEVER K-sliced (asserted from the restated plan): both arms run gemm8pp_kernel<EPI, 2, true>, the workspace arm
    only shows that an unused workspace changes nothing.  The sliced fp8 kernels are test_gemm_fp8_whole_k_slicing_is_exact's."""
    seed = X.shape_seed(B, M, N, K)
    cs = X.gemm_operands(B, M, N, K, seed)
    gate, res = epilogue_operands(B, M, N, seed)
    sa, sw = X.pow2((B, M), -3, 3, seed + 5), X.pow2((N,), -3, 3, seed + 6)
    lin = X.linear_bf16(cs["acc"], cs["bias"].float(), row_scale=sa, col_scale=sw)
    aq, wq = X.fp8_bytes(cs["a"]).cuda(), X.fp8_bytes(cs["w"]).cuda()
    ws = torch.empty(X.GEMM_WS_BYTES, dtype=torch.uint8, device="cuda")
    assert X.plan_slices_fp8(B, M, N, K, ws.numel(), grid_of_device()) == (1, 0, 0)
    gf = 256 if N > 256 else 0
    for epi in (0, 1, 2, 3):
        kw = dict(res=res.cuda(), gate=gate.cuda()) if epi == 2 else dict(res=res.cuda()) if epi == 3 else {}
        for wsp in (None, ws):
            got = ops.gemm_fp8(aq, sa.cuda(), wq, sw.cuda(), cs["bias"].cuda(), epilogue=epi, gelu_from_col=gf, workspace=wsp, **kw)
            check_epilogue(got, epi, lin, res, gate, gf, f"gemm_fp8 epilogue {epi} workspace {wsp is not None}")


WS_NAN = 0x7FC0BEEF           # the workspace's fill: a quiet NaN with a payload no arithmetic produces


class Fp8Framed:
    """An X.fp8_sliced_case on the device in the arrangement of test_gemm_epilogue_chains_per_element: A a column slice of a wider uint8
    buffer (row pitch K + 64 bytes, the other bytes hold e4m3 1.0 and must stay), C a column slice inside a sentinel frame, res aliasing C."""

    def __init__(self, ops, cs):
        self.ops, self.cs = ops, cs
        self.B, self.M, self.K = cs["aq"].shape
        self.N = cs["wq"].shape[0]
        self.abuf = torch.full((self.B, self.M, self.K + 64), 0x38, dtype=torch.uint8, device="cuda")
        self.abuf[:, :, 64:] = cs["aq"].cuda()
        self.dev = {k: cs[k].cuda() for k in ("sa", "wq", "sw", "bias", "gate", "res")}

    def run(self, epi, workspace, gelu_from=256):
        d, N = self.dev, self.N
        cbuf = torch.full((self.B, self.M, N + 136), SENTINEL, dtype=BF, device="cuda")
        out = cbuf[:, :, 128:128 + N]
        kw = {}
        if epi in (2, 3):
            out.copy_(d["res"])
            kw = dict(res=out, gate=d["gate"]) if epi == 2 else dict(res=out)
        self.ops.gemm_fp8(self.abuf[:, :, 64:], d["sa"], d["wq"], d["sw"], d["bias"], out=out, epilogue=epi, gelu_from_col=gelu_from,
                          workspace=workspace, **kw)
        assert (cbuf[:, :, :128] == SENTINEL).all() and (cbuf[:, :, 128 + N:] == SENTINEL).all(), "bytes outside the C slice were written"
        return out

    def check_operand_untouched(self):
        assert (self.abuf[:, :, :64] == 0x38).all() and torch.equal(self.abuf[:, :, 64:].cpu(), self.cs["aq"])


def check_sliced_workspace(ws32, B, M, N, slices, acc, what):
    """The device-side proof that `slices` K slices ran: of a workspace filled with WS_NAN, the first T * slices units of 256 KiB -- [slice]
    [tile][256][256] fp32, tiles in the kernels' order, which with at most 12 column tiles is sample, row tile, column tile
    (gemm.hip::make_params: gm = 1) -- have every in-range element overwritten, nothing beyond them has changed, and the slices'
    partials sum to the integer product (they are the raw accumulators: fp8 scales and the bias come after the reduction)."""
    T, _ = X.gemm_tiles(B, M, N)
    tm, tn = (M + 255) // 256, (N + 255) // 256
    assert tn <= 12
    units = T * slices
    changed = (ws32 != WS_NAN).view(-1, 65536)
    touched = changed.any(1).nonzero()
    extent = (int(touched.max()) + 1 if touched.numel() else 0) * 262144
    print(f"{what}: workspace written up to {extent} bytes; T * sk * 256 KiB = {T} * {slices} * 262144 = {units * 262144}")
    assert not bool(changed[units:].any()), f"{what}: the workspace changed beyond {units} units of 256 KiB"

    def in_range(t):
        return t.view(slices, B, tm, tn, 256, 256).permute(0, 1, 2, 4, 3, 5).reshape(slices, B, tm * 256, tn * 256)[:, :, :M, :N]
    assert bool(in_range(changed[:units]).all()), f"{what}: a (slice, tile) unit was not written, or not all of its rows and columns"
    assert extent == units * 262144
    parts = in_range(ws32[:units * 65536].view(torch.float32))
    assert torch.equal(parts.double().sum(0).cpu(), acc), f"{what}: the slices' partials do not sum to the integer product"


def fp8_sliced_checks(ops, B, M, N, K, slices, epilogues):
    """Sliced (workspace) and unsliced (no workspace) launches of one X.fp8_sliced_case under `epilogues`: each against the chain, the two
    against each other bit for bit, the slicing proven from the workspace."""
    cs = X.fp8_sliced_case(B, M, N, K)
    f = Fp8Framed(ops, cs)
    ws32 = torch.empty(X.GEMM_WS_BYTES // 4, dtype=torch.int32, device="cuda")
    for epi in epilogues:
        what = f"gemm_fp8 ({B}, {M}, {N}, {K}) epilogue {epi}"
        ws32.fill_(WS_NAN)
        sliced = f.run(epi, ws32)
        check_sliced_workspace(ws32, B, M, N, slices, cs["acc"], what)
        unsliced = f.run(epi, None)
        check_epilogue(sliced, epi, cs["lin"], cs["res"], cs["gate"], 256, f"{what}, {slices} K slices")
        check_epilogue(unsliced, epi, cs["lin"], cs["res"], cs["gate"], 256, f"{what}, unsliced at {K // 128} K-tiles")
        X.assert_elementwise(sliced, unsliced, f"{what}, sliced vs unsliced")
    f.check_operand_untouched()
    return f


@pytest.mark.parametrize("K", list(X.GEMM_FP8_KSLICE))
def test_gemm_fp8_whole_k_slicing_is_exact(ops, K):
    """The fp8 twin of test_gemm_whole_k_slicing_is_exact.  (1, 300, 520, K): 6 tiles, so with a workspace launch_fp8 cuts every tile into
    2 / 3 / 4 / 6 / 8 K slices -- gemm8pp_kernel<EPI_BIAS, 2, true, true> writes fp32 partials, tail_reduce_kernel<EPI, true> sums them,
    applies the row scale, the channel scale, the bias and the epilogue -- at every slice count the reduction has a case for and at the
    production depths K = 3072, 12288, 15360.  Ternary e4m3 operands, power-of-two scales: ONE bf16 value per element, so every epilogue of
    the sliced launch must give the chain's bits (GELU columns as check_epilogue treats them) and the bits of the launch without a
    workspace, which is itself compared with the chain: the exact test of the unsliced fp8 kernel at 16 .. 120 K-tiles.  A and C are
    column slices of wider buffers, res aliases C.  That slicing happened is read from the workspace (check_sliced_workspace), not inferred
    from the restated plan; the plan only decides the skip on a device whose workgroup count gives another slice count.
    The accumulator bound of X.gemm_operands holds at every K at the default density of a quarter, K = 15360 included."""
    B, M, N = X.GEMM_KSLICE_BMN
    slices = X.GEMM_FP8_KSLICE[K]
    plan = X.plan_slices_fp8(B, M, N, K, X.GEMM_WS_BYTES, grid_of_device())
    if plan[0] != slices:
        pytest.skip(f"this device plans {plan[0]} slices at K = {K}, not {slices}")
    fp8_sliced_checks(ops, B, M, N, K, slices, (0, 1, 2, 3))


def test_gemm_fp8_k_slicing_takes_each_samples_own_row_scales(ops):
    """(2, 300, 520, 3072): 12 tiles in 3 slices.  Two different samples with different row scales, epilogues 0 and 2 -- tail_reduce_kernel
    reads a_scale[b * M + m], the gate and the residual per sample -- and then the first sample twice: identical samples, identical bits."""
    B, M, N, K = X.GEMM_FP8_BATCH2
    slices = X.GEMM_FP8_BATCH2_SLICES
    plan = X.plan_slices_fp8(B, M, N, K, X.GEMM_WS_BYTES, grid_of_device())
    if plan[0] != slices:
        pytest.skip(f"this device plans {plan[0]} slices for 12 tiles at K = {K}, not {slices}")
    cs = X.fp8_sliced_case(B, M, N, K)
    assert not torch.equal(cs["aq"][0], cs["aq"][1]) and int((cs["sa"][0] != cs["sa"][1]).sum()) > M // 2
    f = fp8_sliced_checks(ops, B, M, N, K, slices, (0, 2))
    d = f.dev
    aq = f.abuf[:1, :, 64:].expand(B, M, K).contiguous()
    twice = {k: d[k][:1].expand(B, *d[k].shape[1:]).contiguous() for k in ("sa", "gate", "res")}
    lin, res, gate = (cs[k][:1].expand(B, *cs[k].shape[1:]) for k in ("lin", "res", "gate"))
    ws = torch.empty(X.GEMM_WS_BYTES, dtype=torch.uint8, device="cuda")
    for epi in (0, 2):
        kw = dict(res=twice["res"], gate=twice["gate"]) if epi == 2 else {}
        got = ops.gemm_fp8(aq, twice["sa"], d["wq"], d["sw"], d["bias"], epilogue=epi, workspace=ws, **kw)
        check_epilogue(got, epi, lin, res, gate, 0, f"gemm_fp8 K-sliced, the same sample twice, epilogue {epi}")
        assert torch.equal(got[0], got[1])


def quantize_framed(ops, x):
    """quantize_rows_fp8 of x (CPU) through row- and batch-strided views inside canary frames: x in a bf16 frame of -2^127 (a value read from
    it would become the row maximum), the codes in a uint8 frame, the scales in a flat one.  Returns (codes, scales) on the CPU."""
    B, R, K = x.shape
    xbuf, xv = framing.framed(B, R, K)
    xv.copy_(x)
    qbuf, qv = framing.framed(B, R, K, dtype=torch.uint8)
    sbuf, sv = framing.flat_framed((B, R), dtype=torch.float32)
    assert not xv.is_contiguous() and not qv.is_contiguous() and xv.stride(0) != R * xv.stride(1)
    ops.quantize_rows_fp8(xv, out=qv, scale=sv)
    framing.check_frame(qbuf, qv, "quantize_rows_fp8 codes")
    framing.check_frame(sbuf, sv, "quantize_rows_fp8 scales")
    assert torch.equal(xv.cpu(), x), "quantize_rows_fp8 wrote its input"
    framing.check_frame(xbuf, xv, "quantize_rows_fp8 input")
    return qv.cpu(), sv.cpu()


@pytest.mark.parametrize("shape", X.QUANT_SHAPES)
def test_quantize_rows_fp8_reproduces_known_codes_and_scales(ops, shape):
    """Rows whose scale (a power of two) and codes (integers) are known, at the K edges of all three instantiations: <2> (256, 512), <6>
    (4104: its first K, one lane in the third round; 12288: full), <8> (12296: its first K; 16384: the limit).  The first row's +-448 sits in
    the last column, the second row's in the first.  Contiguous tensors, and row- and batch-strided views of x and of the codes in canary
    frames; K = 16392 is refused."""
    x, codes, scale = X.quantizable_rows(shape, X.shape_seed(*shape), edge_peaks=True)
    q, s = ops.quantize_rows_fp8(x.cuda())
    assert torch.equal(s.cpu(), scale) and torch.equal(q.cpu(), codes)
    q, s = quantize_framed(ops, x)
    assert torch.equal(s, scale) and torch.equal(q, codes)


def test_quantize_rows_fp8_refuses_k_beyond_its_limit(ops):
    K = X.QUANT_K_LIMIT + 8
    with pytest.raises(RuntimeError, match=f"quantize_rows_fp8: K = {K} exceeds {X.QUANT_K_LIMIT}"):
        ops.quantize_rows_fp8(torch.zeros(1, 2, K, dtype=BF, device="cuda"))


# ----------------------------------------------------------------------------------------------------------------- fused q / k norm + RoPE
@pytest.mark.parametrize("B,gelu", [(1, False), (1, True), (2, False)])
def test_gemm_qkn_is_bit_equal_to_the_separate_pass_and_to_the_cpu_chain(ops, B, gelu):
    """tfx_gemm_bf16_qkn against tfx_gemm_bf16 + tfx_rmsnorm_rope on |lin| <= 256 with dyadic norm weights and rotary pairs: the 128
    squares sum exactly in either kernel's order, so both evaluate rsqrtf(ss * (1 / 128) + eps) (gemm.hip:392, elementwise.hip:205) on
    identical bits and every later product is exact -- ALL elements must be bit-equal (Gaussian inputs: a 2 % sliver within 2^-6).
    Against the CPU restatement: one bf16 step per q / k element, and at most 4 x the measured share of elements whose bits change when
    the row factor moves by one fp32 step (the device rsqrt is within one step of the correctly rounded factor the restatement uses; four
    covers both directions and the weight product).  Measured share: 0 of 14.4 M elements (tests/test_exact_inputs_cpu.py), so the cap is
    0 and the q / k ranges are bit-equal as well; v columns `ulps=0`, GELU'd mlp columns as in check_epilogue.  B = 2: one rotary table
    per sample (rope_bstride)."""
    D, M, K, pos0 = X.QKN_D, X.QKN_M, X.QKN_K, X.QKN_POS0
    N = 4 * D if gelu else 3 * D
    seed = X.shape_seed(B, M, N, K)
    cs = X.gemm_operands(B, M, N, K, seed)
    lin = X.linear_bf16(cs["acc"], cs["bias"].float())
    wq, wk = X.norm_weights(seed + 1), X.norm_weights(seed + 2)
    tab = X.rope_table(M + pos0, seed + 3, B=B if B > 1 else 0)
    cos, sin = X.expand_pairs(tab[..., pos0:, :, :])
    a, w, b = cs["a"].cuda(), cs["w"].cuda(), cs["bias"].cuda()
    kw = dict(epilogue=ops.EPI_BIAS_GELU, gelu_from_col=3 * D) if gelu else dict(epilogue=ops.EPI_BIAS)
    sep = ops.gemm(a, w, b, **kw)
    ops.rmsnorm_rope_(sep, 2 * D, 0, 24, 0, wq.cuda(), wk.cuda(), wq.cuda(), wk.cuda(), cos.cuda(), sin.cuda())
    fused = ops.gemm_qkn(a, w, b, wq.cuda(), wk.cuda(), tab.cuda(), (2 * D, 3 * D), (0, D), pos0=pos0, **kw)
    fused_cpu = fused.cpu()
    X.assert_elementwise(fused_cpu, sep.cpu(), "gemm_qkn vs gemm + rmsnorm_rope")
    want = X.qk_norm_rope(X.chain(1, lin, gelu_from_col=3 * D) if gelu else lin, ((2 * D, 3 * D), (0, D)), (wq, wk), tab[..., pos0:, :, :])
    X.assert_elementwise(fused_cpu[..., D:2 * D], want[..., D:2 * D], "v columns")
    for name, lo in (("k", 0), ("q", 2 * D)):
        X.assert_elementwise(fused_cpu[..., lo:lo + D], want[..., lo:lo + D], f"{name} columns vs the CPU chain", ulps=1, cap=4 * X.QKN_SHARE_ONE_ULP)
    if gelu:
        exact = X.gelu_exact_mask(lin, 3 * D)[..., 3 * D:]
        X.assert_elementwise(torch.where(exact, fused_cpu[..., 3 * D:], want[..., 3 * D:]), want[..., 3 * D:], "mlp columns, GELU = 0 or x")
        X.assert_elementwise(fused_cpu[..., 3 * D:], want[..., 3 * D:], "mlp columns", ulps=1)


# ----------------------------------------------------------------------------------------------------------------- attention, head dim 128
def fused_attention(ops, q, k, v, **kw):
    """The blocks' layout: [k | v | q] column ranges of one buffer, the output in place over q; k and v must come back untouched."""
    HD = q.shape[-1]
    y = torch.cat([k, v, q], -1).cuda()
    kv_before = y[:, :, :2 * HD].clone()
    ops.attention(y[:, :, 2 * HD:], y[:, :, :HD], y[:, :, HD:2 * HD], out=y[:, :, 2 * HD:], **kw)
    assert torch.equal(y[:, :, :2 * HD], kv_before), "k / v columns were written"
    return y[:, :, 2 * HD:]


def attention_forms(B, H, N, lengths=None):
    seed = X.shape_seed(B, H, N)
    u = X.uniform_attention(B, H, N, seed, lengths)
    s = X.selector_attention(B, H, N, seed, lengths)
    assert s[4] <= 35.0
    return (("uniform", u), ("selector", s[:4]))


def check_attention(ops, B, H, N, what, streamk_tail=0, **kw):
    """Both forms, both streams (score_bound 0: the guarded kernel, 35: the reference-free one), the form asserted from the counters."""
    for name, (q, k, v, want) in attention_forms(B, H, N):
        for bound, mode in ((0.0, "w4_guarded"), (35.0, "w4_reference_free")):
            ops.attention_mode_counts(reset=True)
            got = fused_attention(ops, q, k, v, score_bound=bound, **kw)
            counts = ops.attention_mode_counts()
            assert counts[mode] == 1 and sum(counts[m] for m in ops.ATTENTION_MODES[:8]) == 1 and counts["streamk_tail"] == streamk_tail, counts
            X.assert_elementwise(got, want, f"attention {what} ({B}, {H}, {N}) {name} form, score_bound {bound}")


@pytest.mark.parametrize("B,H,N", X.ATTN_SHAPES)
def test_attention_exact_forms(ops, B, H, N):
    """q = 0: every weight is exactly 1 and v's +-128 cancel over the valid keys, so each row is the integer c -- a key dropped, doubled
    or read from the padding moves it by >= 128 / N.  q = 3 k[pi(i)]: the softmax selects key pi(i) to within 2^-12, the row is v[pi(i)].
    Every head has its own c and its own permutation.  The default kernel sums the bf16-rounded weights it multiplies with, so both
    forms are exact (`ulps=0`)."""
    check_attention(ops, B, H, N, "default launch")


@pytest.mark.parametrize("B,H,N", X.ATTN_PERSISTENT_SHAPES)
def test_attention_persistent_item_walk_is_exact(ops, B, H, N):
    items = B * H * ((N + 255) // 256)
    if items <= grid_of_device():
        pytest.skip(f"{items} items do not exceed this device's {grid_of_device()} workgroups: no item walk")
    try:
        for pers in (1, 0):
            ops.set_option("attention_persistent", pers)
            check_attention(ops, B, H, N, f"attention_persistent {pers}")
    finally:
        ops.set_option("attention_persistent", 1)


def test_attention_streamk_dealing_is_exact(ops):
    """(2, 5, 2304) with a workspace and attention_streamk 2: 45 items per sample dealt as (item, 64-key tile) units to the sample's half of
    the CUs, pieces merged from un-normalised partials -- integer sums in the uniform form, so still exact.  `streamk_tail` must count
    every launch; the admission rule is restated from attention_w4.hip::joint_attention_w4."""
    B, H, N = X.ATTN_STREAMK_SHAPE
    group, nkv, Tp = grid_of_device() // B, (N + 63) // 64, H * ((N + 255) // 256)
    R = Tp - (Tp // group) * group
    share = (R * nkv + group - 1) // group if R else 0
    if not (R > 0 and nkv >= 16 and share * 6 >= nkv and share >= 8):
        pytest.skip(f"{Tp} items per sample on groups of {group} CUs: nothing to deal")
    ws = torch.empty(72 << 20, dtype=torch.uint8, device="cuda")
    try:
        ops.set_option("attention_streamk", 2)
        check_attention(ops, B, H, N, "stream-K", streamk_tail=1, workspace=ws)
    finally:
        ops.set_option("attention_streamk", 1)


def test_attention_tail_split_is_exact(ops):
    """(1, 24, 3100) with attention_tail_split 1: 312 items on 256 CUs, the last 56 cut into two key ranges (>= 24 key tiles each, the
    second ends in the ragged tile) and merged.  The plan is restated from attention_w4.hip::joint_attention_w4."""
    B, H, N = X.ATTN_TAIL_SHAPE
    C = torch.cuda.get_device_properties(0).multi_processor_count
    T, nkv = B * H * ((N + 255) // 256), (N + 63) // 64
    tail = T % C
    m = (tail + B - 1) // B
    if not (tail and T >= C and m * B * 2 <= C + 8 and nkv >= 48 and m < H * ((N + 255) // 256)):
        pytest.skip(f"{T} items on {C} CUs: the tail split is not taken")
    try:
        ops.set_option("attention_tail_split", 1)
        check_attention(ops, B, H, N, "tail split")
    finally:
        ops.set_option("attention_tail_split", 0)
        ops.release_scratch()


@pytest.mark.parametrize("shape,lengths", X.ATTN_SEQ_LEN_CASES)
def test_attention_seq_len_is_exact_and_leaves_the_padding_alone(ops, shape, lengths):
    """Per-sample lengths: NaN in every padding row of q, k and v, the zero-sum structure and the permutations built over each sample's
    own L rows.  Valid rows equal c / v[pi] exactly; rows >= L keep the sentinel the output was filled with."""
    B, H, N = shape
    sl = torch.tensor(lengths, dtype=torch.int32, device="cuda")
    seed = X.shape_seed(B, H, N)
    forms = (("uniform", X.uniform_attention(B, H, N, seed, lengths)), ("selector", X.selector_attention(B, H, N, seed, lengths)[:4]))
    for name, (q, k, v, want) in forms:
        for bound, mode in ((0.0, "w4_guarded"), (35.0, "w4_reference_free")):
            out = torch.full((B, N, H * 128), SENTINEL, dtype=BF, device="cuda")
            ops.attention_mode_counts(reset=True)
            ops.attention(q.cuda(), k.cuda(), v.cuda(), out=out, score_bound=bound, seq_len=sl)
            counts = ops.attention_mode_counts()
            assert counts[mode] == 1 and counts["streamk_tail"] == 0, counts
            expect = torch.where(torch.isnan(want), torch.full_like(want, SENTINEL), want)     # want is NaN exactly in the rows >= L
            for b, L in enumerate(lengths):
                assert not torch.isnan(want[b, :L].float()).any() and torch.isnan(want[b, L:].float()).all()
            X.assert_elementwise(out, expect, f"attention seq_len {lengths} {name} form, score_bound {bound}")


# ----------------------------------------------------------------------------------------------------------------- attention, dyadic form
# Every softmax weight a power of two, every row sum a power of two, v integer (X.dyadic_attention): the scores, exp2f of an integer, the
# bf16 weights, P.V and the row sums, the exp2f(-d) rescale of a reference move, the merge weights and 1 / l are all exact in fp32, and the
# one rounding is the final bf16 pack -- `ulps=0` in any summation order, with any reference policy and any split into pieces.  Unlike the
# uniform and the selector form this one sees the softmax arithmetic: a reference move whose rescale is lost or lands on the other q-block,
# unshifted scores, a merge weight, a masked key admitted with a small weight (tests/test_exact_inputs_cpu.py injects each of them into the
# host restatement and shows that the expected bits change, and that the cases do move the reference and do merge unequal pieces).
def check_dyadic(ops, B, H, N, what, streamk_tail=0, **kw):
    """Both streams on the bounded family (|score| <= 50, 50 ln 2 <= 35), the guarded one also on the far family (columns near -200 and
    near +250); the form asserted from the counters."""
    seed = X.shape_seed(B, H, N)
    for family, streams in (("bounded", ((0.0, "w4_guarded"), (35.0, "w4_reference_free"))), ("far", ((0.0, "w4_guarded"),))):
        q, k, v, want = X.dyadic_attention(B, H, N, seed, None, family)
        for bound, mode in streams:
            ops.attention_mode_counts(reset=True)
            got = fused_attention(ops, q, k, v, scale=X.DYADIC_SCALE, score_bound=bound, **kw)
            counts = ops.attention_mode_counts()
            assert counts[mode] == 1 and sum(counts[m] for m in ops.ATTENTION_MODES[:8]) == 1 and counts["streamk_tail"] == streamk_tail, counts
            X.assert_elementwise(got, want, f"attention {what} ({B}, {H}, {N}) dyadic form, {family} family, score_bound {bound}")


@pytest.mark.parametrize("B,H,N", X.ATTN_SHAPES)
def test_attention_dyadic_form(ops, B, H, N):
    """The default launch.  The columns' key orders make the guarded kernel's reference move repeatedly (ascending weights), never
    (descending), inside the ragged last tile by more than W4_THR (the late spike), and the far family makes the first unit pin it at
    -200 and +250; the reference-free stream has to place graded scores of +-50 without a reference."""
    check_dyadic(ops, B, H, N, "default launch")


@pytest.mark.parametrize("B,H,N", X.ATTN_PERSISTENT_SHAPES)
def test_attention_dyadic_persistent_item_walk(ops, B, H, N):
    items = B * H * ((N + 255) // 256)
    if items <= grid_of_device():
        pytest.skip(f"{items} items do not exceed this device's {grid_of_device()} workgroups: no item walk")
    try:
        for pers in (1, 0):
            ops.set_option("attention_persistent", pers)
            check_dyadic(ops, B, H, N, f"attention_persistent {pers}")
    finally:
        ops.set_option("attention_persistent", 1)


def test_attention_dyadic_streamk_dealing(ops):
    """The dealt pieces of an item end with different references in most rows (the block columns put their largest weights at a place of
    their own), so attn_w4_merge_sk_kernel's exp2f(m_part - m) weights are powers of two other than 1 on the guarded stream.  Admission
    rule as in test_attention_streamk_dealing_is_exact."""
    B, H, N = X.ATTN_STREAMK_SHAPE
    group, nkv, Tp = grid_of_device() // B, (N + 63) // 64, H * ((N + 255) // 256)
    R = Tp - (Tp // group) * group
    share = (R * nkv + group - 1) // group if R else 0
    if not (R > 0 and nkv >= 16 and share * 6 >= nkv and share >= 8):
        pytest.skip(f"{Tp} items per sample on groups of {group} CUs: nothing to deal")
    ws = torch.empty(72 << 20, dtype=torch.uint8, device="cuda")
    try:
        ops.set_option("attention_streamk", 2)
        check_dyadic(ops, B, H, N, "stream-K", streamk_tail=1, workspace=ws)
    finally:
        ops.set_option("attention_streamk", 1)


def test_attention_dyadic_tail_split(ops):
    """attn_w4_merge_kernel on halves whose references differ either way.  Plan as in test_attention_tail_split_is_exact."""
    B, H, N = X.ATTN_TAIL_SHAPE
    C = torch.cuda.get_device_properties(0).multi_processor_count
    T, nkv = B * H * ((N + 255) // 256), (N + 63) // 64
    tail = T % C
    m = (tail + B - 1) // B
    if not (tail and T >= C and m * B * 2 <= C + 8 and nkv >= 48 and m < H * ((N + 255) // 256)):
        pytest.skip(f"{T} items on {C} CUs: the tail split is not taken")
    try:
        ops.set_option("attention_tail_split", 1)
        check_dyadic(ops, B, H, N, "tail split")
    finally:
        ops.set_option("attention_tail_split", 0)
        ops.release_scratch()


@pytest.mark.parametrize("shape,lengths", X.ATTN_SEQ_LEN_CASES)
def test_attention_dyadic_seq_len(ops, shape, lengths):
    """Per-sample lengths: every sample's multisets are built over its own L keys, NaN in every padding row of q, k and v; rows >= L keep
    the sentinel the output was filled with."""
    B, H, N = shape
    sl = torch.tensor(lengths, dtype=torch.int32, device="cuda")
    seed = X.shape_seed(B, H, N)
    for family, streams in (("bounded", ((0.0, "w4_guarded"), (35.0, "w4_reference_free"))), ("far", ((0.0, "w4_guarded"),))):
        q, k, v, want = X.dyadic_attention(B, H, N, seed, lengths, family)
        for b, L in enumerate(lengths):
            assert not torch.isnan(want[b, :L].float()).any() and torch.isnan(want[b, L:].float()).all()
        expect = torch.where(torch.isnan(want), torch.full_like(want, SENTINEL), want)
        HD = H * 128
        for bound, mode in streams:
            # the blocks' [k | v | q] layout, the output in place over q, whose padding rows hold the sentinel (k / v keep their NaN rows,
            # so they are compared as bits)
            y = torch.cat([k, v, torch.where(torch.isnan(q), torch.full_like(q, SENTINEL), q)], -1).cuda()
            kv_before = y[:, :, :2 * HD].clone()
            ops.attention_mode_counts(reset=True)
            ops.attention(y[:, :, 2 * HD:], y[:, :, :HD], y[:, :, HD:2 * HD], out=y[:, :, 2 * HD:], scale=X.DYADIC_SCALE, score_bound=bound, seq_len=sl)
            counts = ops.attention_mode_counts()
            assert counts[mode] == 1 and counts["streamk_tail"] == 0, counts
            assert torch.equal(y[:, :, :2 * HD].contiguous().view(torch.int16), kv_before.view(torch.int16)), "k / v columns were written"
            X.assert_elementwise(y[:, :, 2 * HD:], expect, f"attention seq_len {lengths} dyadic form, {family} family, score_bound {bound}")


# ----------------------------------------------------------------------------------------------------------------- attention64
def pitched(t, extra=24):
    """t on the device as a view with a row pitch of its own."""
    buf = torch.full((*t.shape[:-1], t.shape[-1] + extra), 9.0, dtype=t.dtype, device="cuda")
    buf[..., :t.shape[-1]] = t.cuda()
    return buf[..., :t.shape[-1]]


def run_attention64(ops, q, k, v, **kw):
    obuf = torch.full((*q.shape[:-1], q.shape[-1] + 12), SENTINEL, dtype=BF, device="cuda")
    out = ops.attention64(pitched(q), pitched(k), pitched(v), 0.125, out=obuf[..., :q.shape[-1]], **kw)
    assert (obuf[..., q.shape[-1]:] == SENTINEL).all()
    return out


@pytest.mark.parametrize("H", X.ATTN64_HS)
@pytest.mark.parametrize("N", X.ATTN64_NS)
def test_attention64_exact_forms(ops, N, H):
    """tfx_attention64 (head dim 64, keys in LDS): uniform form, selector by codes plain and causal (pi(i) <= i), and selector by the
    relative bias -- 24.0 at one offset delta of every head's row, so query i must pick key i + delta: the `key - query + N - 1` index
    itself -- with rows whose target lies outside [0, N) uniform.  attn64_kernel sums its weights unrounded and multiplies their bf16
    roundings (textenc.hip:100-108): exact for weights of 1; the others are <= e^-13 here and move no selected value (none of which is 0)."""
    B, seed = 2, X.shape_seed(2, H, N, 64)
    q, k, v, want = X.uniform_attention(B, H, N, seed, None, 64)
    X.assert_elementwise(run_attention64(ops, q, k, v), want, f"attention64 uniform N {N} H {H}")
    for causal in (False, True):
        q, k, v, want, _ = X.selector_attention(B, H, N, seed, None, 64, X.ATTN64_MULT, 0.125, causal)
        X.assert_elementwise(run_attention64(ops, q, k, v, causal=causal), want, f"attention64 selector causal={causal} N {N} H {H}")
    for delta in sorted({-(N - 1), -1, 0, 1, N - 1}):
        if abs(delta) > N - 1:
            continue
        q, k, v, bias, want = X.bias_selector_attention(B, H, N, delta, seed)
        X.assert_elementwise(run_attention64(ops, q, k, v, rel_bias=bias.cuda()), want, f"attention64 bias selector delta {delta} N {N} H {H}")


def test_attention64_graded_form(ops):
    """Graded weights through attn64_kernel's online rescale: natural scores that are small integers rising along the keys (one-hot q times
    8, scale 0.125), plain, causal and with an integer rel_bias, so that the running maximum moves and alpha != 1 in most 32-key blocks.
    The kernel multiplies by log2 e after the bias, so its exp2-domain scores are no integers and nothing is exact; the expected value is
    X.attention64_graded_chain, the kernel's rounding points (the maximum in force at each block, the bf16 weights under an unrounded
    sum, alpha) with fp64 in between.  Every element within one bf16 step, and over all cases at most 4 * X.ATTN64_GRADED_SHARE of the
    elements different at all -- the share the CPU measures for one fp32 step of every exponential and of the row sum."""
    n = diff = 0
    for N, H, mode in X.attention64_graded_cases():
        q, k, v, bias = X.graded_attention64(2, H, N, X.shape_seed(2, H, N, 64, 1), mode)
        want = X.attention64_graded_chain(q, k, v, 0.125, rel_bias=bias, causal=mode == "causal")
        kw = dict(causal=True) if mode == "causal" else dict(rel_bias=bias.cuda()) if mode == "bias" else {}
        d = X.assert_elementwise(run_attention64(ops, q, k, v, **kw), want, f"attention64 graded {mode} N {N} H {H}", ulps=1)
        n, diff = n + want.numel(), diff + d
    print(f"attention64 graded: {diff} of {n} elements differ from the chain; cap {4 * X.ATTN64_GRADED_SHARE * n:.1f}")
    assert diff <= 4 * X.ATTN64_GRADED_SHARE * n


# ----------------------------------------------------------------------------------------------------------------- convolutions
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("B,H,W,Cin,Cout,stride,up,pad_lo,with_res", X.CONV_CASES)
def test_conv3x3_is_exact(ops, variant, B, H, W, Cin, Cout, stride, up, pad_lo, with_res):
    """Integer convolution against F.conv2d in fp64: plain, ragged with a residual, the folded 2x upsample, the stride-2 downsample with
    pad (0, 1, 0, 1).  Borders and corners are part of every image."""
    cs = X.conv_operands(B, H, W, Cin, Cout, X.shape_seed(B, H, W, Cin, Cout), stride=stride, up=up, with_res=with_res)
    got = ops.conv3x3_nhwc(cs["x"].cuda(), cs["w"].cuda(), cs["bias"].cuda(), stride=stride, up=up, pad_lo=pad_lo,
                           res=cs["res"].cuda() if with_res else None, variant=variant)
    assert got.shape == cs["want"].shape
    X.assert_elementwise(got.flatten(1, 2), cs["want"].flatten(1, 2), f"conv3x3 variant {variant} (rows are pixels y * W + x)")


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("B,H,W,Cin,Cout", X.CONV_NARROW_CASES)
def test_conv3x3_narrow_input_is_exact(ops, variant, B, H, W, Cin, Cout):
    """conv_in's narrow form: Cin 3 / 16 padded to 8 / 16 channels, K = 9 Cin_p padded with zero weights to a multiple of 64."""
    cs = X.conv_operands(B, H, W, Cin, Cout, X.shape_seed(B, H, W, Cin, Cout))
    cp = 8 if Cin <= 8 else 16 if Cin <= 16 else 32
    xp = torch.zeros(B, H, W, cp, dtype=BF)
    xp[..., :Cin] = cs["x"]
    wp = torch.zeros(Cout, 3, 3, cp, dtype=BF)
    wp[..., :Cin] = cs["w"]
    wk = torch.zeros(Cout, (9 * cp + 63) // 64 * 64, dtype=BF)
    wk[:, :9 * cp] = wp.reshape(Cout, 9 * cp)
    got = ops.conv3x3_nhwc(xp.cuda(), wk.cuda(), cs["bias"].cuda(), variant=variant)
    X.assert_elementwise(got.flatten(1, 2), cs["want"].flatten(1, 2), f"narrow conv3x3 variant {variant} Cin {Cin}")


@pytest.mark.parametrize("B,H,W,Cin,Cout,with_res", X.CONV_PAIR_CASES)
def test_conv3x3_pixel_pair_form_is_exact(ops, B, H, W, Cin, Cout, with_res):
    cs = X.conv_operands(B, H, W, Cin, Cout, X.shape_seed(B, H, W, Cin, Cout), with_res=with_res)
    wp, bp = ops.pair_conv_weights(cs["w"].cuda(), cs["bias"].cuda())
    got = ops.conv3x3_pair_nhwc(cs["x"].cuda(), wp, bp, res=cs["res"].cuda() if with_res else None)
    X.assert_elementwise(got.flatten(1, 2), cs["want"].flatten(1, 2), "pixel-pair conv3x3")
