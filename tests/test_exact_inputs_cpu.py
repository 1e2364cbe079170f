"""The exact-input constructions of tests/helpers/exact_inputs.py, proven without a GPU.

Three things, for every shape tests/test_exact_gpu.py uses: each generator meets the exactness condition it asserts; each CPU
restatement in fp64 rounds to the bits the construction claims (uniform attention -> c, selector -> v[pi], the integer GEMM and
convolution chains); and assert_elementwise rejects every emulated kernel fault -- a dropped product, a dropped K-tile, a shifted
bias chunk, another sample's gate, a missing rounding, a left-out K slice, another sample's row scales, a bias added before the fp8
scales, a dropped / padded / swapped key, swapped heads, a shifted rotary pair.  It also holds the one restatement of the K-slice plan
(X.plan_slices) to the slice counts the GPU tests' case tables claim.
The faults are injected into the CPU computation; no kernel code is restated here, with one exception: the dyadic attention form
(power-of-two softmax weights) is there to see the guarded kernel's reference moves and the merges of key ranges, so its faults -- a lost
or misplaced rescale, unshifted scores, a merge weight, an admitted masked key, doubled weights -- are injected into X.guarded_walk, the
host restatement of that kernel's reference policy, which is itself checked against the form's policy-free expected value."""
import pytest
import torch

from tests.helpers import exact_inputs as X

BF = torch.bfloat16


def step(x):
    """The next bf16 value away from zero."""
    return (x.view(torch.int16) + 1).view(BF)


def rejects(got, want, what, **kw):
    with pytest.raises(AssertionError, match=what) as e:
        X.assert_elementwise(got, want, what, **kw)
    return str(e.value)


# ------------------------------------------------------------------------------------------------ assert_elementwise itself
def test_assert_elementwise_counts_steps_and_names_the_tile():
    want = torch.tensor([[1.0, -2.0, 0.0, 300.0]], dtype=BF).repeat(600, 130)            # [600, 520]
    assert X.assert_elementwise(want.clone(), want, "same") == 0
    got = want.clone()
    got[513, 261] = step(got[513, 261])
    msg = rejects(got, want, "one step")
    assert "1 of 312000" in msg and "(batch 0, row 513, col 261)" in msg and "tile (2, 1) at (1, 5)" in msg
    assert X.assert_elementwise(got, want, "one step allowed", ulps=1) == 1
    rejects(got, want, "capped", ulps=1, cap=1e-7)                                       # within a step, but more of them than the cap
    got[513, 261] = step(got[513, 261])
    rejects(got, want, "two steps", ulps=1)
    z = torch.zeros(4, 8, dtype=BF)
    assert X.assert_elementwise(-z, z, "signed zero") == 0                              # -0 == +0, as torch.equal has it
    tiny = z.clone()
    tiny[1, 1] = step(tiny[1, 1])                           # the smallest subnormal: one step from either zero
    assert X.assert_elementwise(-tiny, tiny, "across zero", ulps=2) == 1
    rejects(-tiny, tiny, "across zero", ulps=1)
    nan = want.clone()
    nan[0, 0] = float("nan")
    rejects(nan, want, "NaN got", ulps=1)
    rejects(nan, nan, "NaN both")
    f = torch.arange(12.0).view(3, 4)
    assert X.assert_elementwise(f.clone(), f, "fp32") == 0
    rejects(f + 2 ** -20, f, "fp32")
    msg = rejects(torch.ones(2, 3, 8, dtype=BF), torch.full((2, 3, 8), 2.0, dtype=BF), "batched")
    assert "48 of 48" in msg and "(batch 1," not in msg.split("first 16")[0] and msg.count("\n") == 16


# ------------------------------------------------------------------------------------------------ GEMM: conditions, chains, faults
def all_gemm_shapes():
    return (X.GEMM_EPI_SHAPES + [X.GEMM_ROUNDING_SHAPE] + [(1, 300, 520, K) for K in X.GEMM_KSLICE_KS] + [(2, 300, 520, 1024)] + X.GEMM_F32_SHAPES +
            X.GEMM_COLSCALE_SHAPES + X.GEMM_FP8_SHAPES + [(1, X.QKN_M, 4 * X.QKN_D, X.QKN_K), (2, X.QKN_M, 3 * X.QKN_D, X.QKN_K)])


@pytest.mark.parametrize("B,M,N,K", all_gemm_shapes())
def test_gemm_generator_condition_holds(B, M, N, K):
    cs = X.gemm_operands(B, M, N, K, X.shape_seed(B, M, N, K))
    for t in (cs["a"], cs["w"]):
        assert set(t.float().unique().tolist()) <= {-1.0, 0.0, 1.0} and 0.2 < (t != 0).float().mean().item() < 0.3
    assert cs["bias"].float().abs().max().item() <= 8
    assert torch.equal(cs["a"].float() @ cs["w"].float().T, cs["acc"].float())          # fp32 sums these integers exactly as well
    X.fp8_bytes(cs["a"]), X.fp8_bytes(cs["w"])                                          # ... and every operand is an e4m3 number
    if (B, M, N, K) in X.GEMM_F32_SHAPES[1:]:
        X.gemm_operands(B, M, N, K, X.shape_seed(B, M, N, K), w_batched=True)


def test_gemm_generator_condition_holds_at_the_sliced_last_round_shape():
    B, M, N, K = X.GEMM_TAIL_SHAPE
    cs = X.gemm_operands(B, M, N, K, X.shape_seed(B, M, N, K), product=False)
    acc = cs["a"][0].float() @ cs["w"].float().T                                        # exact in fp32: integer partial sums <= K < 2^24
    X.check_accumulators(acc, cs["bias"])
    rows = torch.arange(0, M, 173)
    assert torch.equal(acc[rows].double(), cs["a"][0, rows].double() @ cs["w"].double().T)


def test_generator_refuses_a_shape_outside_the_exact_regime():
    with pytest.raises(AssertionError, match="exact regime"):
        X.check_accumulators(torch.full((2, 2), 250.0, dtype=torch.float64), torch.full((2,), 8.0))
    with pytest.raises(AssertionError, match="exact regime"):
        X.gemm_operands(1, 64, 64, 65536, 5, p_nonzero=1.0)                              # a shape / density added later cannot leave it silently
    with pytest.raises(AssertionError, match="integers"):
        X.check_accumulators(torch.full((2, 2), 0.5, dtype=torch.float64))


@pytest.fixture(scope="module")
def g():
    """One GEMM case with every epilogue operand: (2, 300, 264, 128), the ragged shape of the GPU file."""
    B, M, N, K = X.GEMM_EPI_SHAPES[0]
    cs = X.gemm_operands(B, M, N, K, X.shape_seed(B, M, N, K))
    cs.update(gate=X.gates(B, N, 11), res=X.arbitrary_bf16((B, M, N), 12), lin=X.linear_bf16(cs["acc"], cs["bias"].float()))
    return cs


def test_chains_are_the_documented_rounding_points(g):
    lin, res, gate = g["lin"], g["res"], g["gate"]
    assert torch.equal(lin.double(), g["acc"] + g["bias"].double())                      # bf16 holds every pre-activation exactly
    assert torch.equal(X.chain(3, lin, res=res), (res.double() + lin.double()).float().to(BF))
    prod = (gate.double()[:, None] * lin.double()).float().to(BF)
    assert torch.equal(X.chain(2, lin, res=res, gate=gate), (res.double() + prod.double()).float().to(BF))
    out = X.chain(1, lin, gelu_from_col=256)
    assert torch.equal(out[..., :256], lin[..., :256])
    ref = torch.nn.functional.gelu(lin[..., 256:].double(), approximate="tanh")
    assert (X.gelu_tanh64(lin[..., 256:]) - ref).abs().max().item() < 1e-12              # the same function (where 1 + tanh does not cancel)
    m = X.gelu_exact_mask(lin, 256)
    assert m[..., :256].all() and 0 < m[..., 256:].float().mean().item() < 1
    mg, lg = m[..., 256:], lin[..., 256:]
    assert torch.equal(out[..., 256:][mg], torch.where(lg > 0, lg, torch.zeros_like(lg))[mg])       # exact cases: 0, or x itself
    cscale = X.pow2((lin.shape[-1],), -3, 3, 13)
    assert torch.equal(X.linear_bf16(g["acc"], col_scale=cscale).double(), g["acc"] * cscale.double())    # epilogue 4: exact


def test_fault_one_product_dropped_from_one_element(g):
    a, w = g["a"].double(), g["w"].double()
    b, m, n = 1, 299, 263
    k = (a[b, m] * w[n]).nonzero()[0].item()
    acc = g["acc"].clone()
    acc[b, m, n] -= a[b, m, k] * w[n, k]
    msg = rejects(X.linear_bf16(acc, g["bias"].float()), g["lin"], "dropped product")
    assert "1 of" in msg and "(batch 1, row 299, col 263)" in msg and "tile (1, 1) at (43, 7)" in msg
    for epi in (2, 3):
        rejects(X.chain(epi, X.linear_bf16(acc, g["bias"].float()), res=g["res"], gate=g["gate"]),
                X.chain(epi, g["lin"], res=g["res"], gate=g["gate"]), "dropped product")


def test_fault_one_k_tile_dropped_for_one_tile():
    B, M, N, K = X.GEMM_EPI_SHAPES[3]
    cs = X.gemm_operands(B, M, N, K, X.shape_seed(B, M, N, K))
    a, w = cs["a"].double(), cs["w"].double()
    acc = cs["acc"].clone()
    acc[1, 256:512, 512:] -= a[1, 256:512, 320:384] @ w[512:, 320:384].T                 # K-tile 5 of tile (1, 2) of sample 1 (ragged in N)
    msg = rejects(X.linear_bf16(acc, cs["bias"].float()), X.linear_bf16(cs["acc"], cs["bias"].float()), "dropped K-tile")
    assert "tile (1, 2)" in msg and "tile (0," not in msg and "batch 0" not in msg


def test_fault_bias_shifted_by_one_chunk(g):
    bias = g["bias"].float().clone()
    bias[256:264] = g["bias"].float()[248:256]                                           # the ragged edge's 8 columns read their neighbour's bias
    assert not torch.equal(bias, g["bias"].float())
    msg = rejects(X.linear_bf16(g["acc"], bias), g["lin"], "shifted bias")
    assert "tile (0, 1)" in msg and "tile (0, 0)" not in msg


def test_fault_gate_of_sample_0_used_for_sample_1(g):
    gate = g["gate"].clone()
    gate[1] = gate[0]
    msg = rejects(X.chain(2, g["lin"], res=g["res"], gate=gate), X.chain(2, g["lin"], res=g["res"], gate=g["gate"]), "wrong gate")
    assert "batch 0" not in msg


def test_fault_intermediate_rounding_of_epilogue_2_omitted(g):
    """gate * lin is a bf16 number while |lin| stays small (always at K <= 3072: `n` is 0 on the fixture's K = 128), so the rounding
    point shows only at the K = 12288 shape the GPU file adds for it."""
    once = (g["res"].double() + g["gate"].double()[:, None] * g["lin"].double()).float().to(BF)
    assert X.mismatches(once, X.chain(2, g["lin"], res=g["res"], gate=g["gate"])).sum().item() == 0
    B, M, N, K = X.GEMM_ROUNDING_SHAPE
    cs = X.gemm_operands(B, M, N, K, X.shape_seed(B, M, N, K))
    lin, gate, res = X.linear_bf16(cs["acc"], cs["bias"].float()), X.gates(B, N, 11), X.arbitrary_bf16((B, M, N), 12)
    want = X.chain(2, lin, res=res, gate=gate)
    once = (res.double() + gate.double()[:, None] * lin.double()).float().to(BF)
    assert X.mismatches(once, want).sum().item() >= 10                                   # 22 of 79200 elements
    rejects(once, want, "one rounding")
    unrounded_gelu = X.gelu_tanh64(g["acc"] + g["bias"].double())                       # (bf16 holds the Linear exactly here: GELU's rounding point
    assert torch.equal(unrounded_gelu.float().to(BF)[..., 256:], X.chain(1, g["lin"], gelu_from_col=256)[..., 256:])   # is not observable, by construction)


def test_fp8_operands_and_quantisable_rows():
    for shape in X.QUANT_SHAPES:
        x, codes, scale = X.quantizable_rows(shape, X.shape_seed(*shape), edge_peaks=True)
        assert torch.equal(x.float().abs().amax(-1) / 448.0, scale)                      # the header's scale, exactly a power of two
        assert torch.equal((x.float() / scale[..., None]).to(X.F8).view(torch.uint8), codes)
        assert bool((x[:, 0, -1].float().abs() == 448 * scale[:, 0]).all()) and bool((x[:, 1, 0].float().abs() == 448 * scale[:, 1]).all())
        last = x.clone()                                                                 # a row maximum that misses the last 8 columns
        last[..., -8:] = 0
        assert not torch.equal(last.float().abs().amax(-1) / 448.0, scale)
    B, M, N, K = X.GEMM_FP8_SHAPES[0]
    cs = X.gemm_operands(B, M, N, K, X.shape_seed(B, M, N, K))
    sa, sw = X.pow2((B, M), -3, 3, 1), X.pow2((N,), -3, 3, 2)
    lin = X.linear_bf16(cs["acc"], cs["bias"].float(), row_scale=sa, col_scale=sw)
    assert torch.equal(lin, (cs["acc"] * sa.double()[..., None] * sw.double() + cs["bias"].double()).float().to(BF))
    sw2 = sw.clone()
    sw2[8:16] = sw[0:8] * 2
    rejects(X.linear_bf16(cs["acc"], cs["bias"].float(), row_scale=sa, col_scale=sw2), lin, "shifted channel scale")


# ------------------------------------------------------------------------------------------------ K-sliced launches: plans, faults
@pytest.mark.parametrize("grid", [256, 304])
def test_restated_slice_plan_gives_the_tabled_slice_counts(grid):
    """X.plan_slices with the 64 MiB workspace of the GPU tests, at the workgroup counts of a 256-CU and a 304-CU device: every table
    entry gets its slice count, and the two GEMM_FP8_SHAPES are never sliced (two and four 128-byte K-tiles, a slice keeps eight)."""
    B, M, N = X.GEMM_KSLICE_BMN
    ws = X.GEMM_WS_BYTES
    for K, want in X.GEMM_KSLICE.items():
        plan = X.plan_slices_bf16(B, M, N, K, ws, grid)
        print(f"grid {grid} bf16 ({B}, {M}, {N}, {K}): {plan}")
        assert plan == (want, 0, 6)
    assert X.plan_slices_bf16(2, M, N, 1024, ws, grid) == (2, 0, 6)
    for K, want in X.GEMM_FP8_KSLICE.items():
        plan = X.plan_slices_fp8(B, M, N, K, ws, grid)
        print(f"grid {grid} fp8  ({B}, {M}, {N}, {K}): {plan}")
        assert plan == (want, 0, 6)
    plan = X.plan_slices_fp8(*X.GEMM_FP8_BATCH2, ws, grid)
    print(f"grid {grid} fp8  {X.GEMM_FP8_BATCH2}: {plan}")
    assert plan == (X.GEMM_FP8_BATCH2_SLICES, 0, 6)
    assert sorted(set(X.GEMM_FP8_KSLICE.values())) == [2, 3, 4, 6, 8] and sorted(set(X.GEMM_KSLICE.values())) == [2, 3, 4, 6, 8]
    for shape in X.GEMM_FP8_SHAPES:
        for bytes_ in (ws, 1 << 40):
            assert X.plan_slices_fp8(*shape, bytes_, grid) == (1, 0, 0), shape
    assert X.plan_slices_fp8(1, 300, 264, 12288, ws, grid) == (8, 0, 4)                   # tests/test_kernels_gpu.py's sliced shape ...
    assert X.plan_slices_fp8(1, 300, 264, 12288, 16 * 300 * 264, grid) == (1, 0, 0)      # ... which a workspace of 16 B M N bytes leaves whole
    assert X.plan_slices_fp8(2, 4736, 3072, 3072, ws, grid) == (1, 0, 0)                 # 456 tiles: fp8 slices whole GEMMs only


def fp8_sliced_cases():
    return [(*X.GEMM_KSLICE_BMN, K, sk) for K, sk in X.GEMM_FP8_KSLICE.items()] + [(*X.GEMM_FP8_BATCH2, X.GEMM_FP8_BATCH2_SLICES)]


@pytest.mark.parametrize("B,M,N,K,slices", fp8_sliced_cases())
def test_fp8_sliced_cases_meet_their_conditions_and_reject_the_slicing_faults(B, M, N, K, slices):
    """The cases of test_gemm_fp8_whole_k_slicing_is_exact and its batch-2 twin: the construction's conditions (asserted by the
    generator), and the comparison of the GPU test -- `ulps=0`, GELU columns one step -- refuses the chain with any one K slice left out,
    with the other sample's row scales, and with the bias added before the scales, under every epilogue."""
    cs = X.fp8_sliced_case(B, M, N, K)
    acc, bias, sa, sw, res, gate = cs["acc"], cs["bias"].float(), cs["sa"], cs["sw"], cs["res"], cs["gate"]
    assert set(cs["aq"].unique().tolist()) <= {0x00, 0x38, 0xB8} and 0.2 < (cs["aq"] != 0).float().mean().item() < 0.3    # 0, 1, -1 as e4m3
    assert torch.equal(cs["lin"], (acc * sa.double()[..., None] * sw.double() + bias.double()).float().to(BF))
    want = {epi: X.chain(epi, cs["lin"], res=res, gate=gate, gelu_from_col=256) for epi in (0, 1, 2, 3)}

    def refused(lin_bad, what):
        moved = []
        for epi in (0, 1, 2, 3):
            got = X.chain(epi, lin_bad, res=res, gate=gate, gelu_from_col=256)
            rejects(got, want[epi], what, ulps=int(epi == 1))
            moved.append(int(X.mismatches(got, want[epi], int(epi == 1)).sum()))
        print(f"({B}, {M}, {N}, {K}) {what}: moves {moved} of {acc.numel()} elements (epilogues 0, 1, 2, 3)")
        assert min(moved) > 0

    parts = X.k_slice_products(cs, slices)
    for s in range(slices):
        refused(X.linear_bf16(acc - parts[s], bias, row_scale=sa, col_scale=sw), f"K slice {s} of {slices} left out")
    scaled_bias = ((acc + bias.double()) * sa.double()[..., None] * sw.double()).float().to(BF)
    refused(scaled_bias, "bias added before the scales")
    if B == 2:
        assert not torch.equal(cs["a"][0], cs["a"][1]) and int((sa[0] != sa[1]).sum()) > M // 2
        refused(X.linear_bf16(acc, bias, row_scale=sa.flip(0), col_scale=sw), "row scales of the other sample")


@pytest.mark.parametrize("M", X.LORA_MS)
@pytest.mark.parametrize("R", X.LORA_RS)
def test_lora_generator_condition_and_neighbour_sensitivity(M, R):
    N, K = X.LORA_NK
    cs = X.lora_case(M, N, K, R, 2, 3, X.shape_seed(M, N, K, R), sets=2)
    full = X.lora_acc(cs, 0b111)
    assert not torch.equal(full, X.lora_acc(cs, 0b101)) and torch.equal(full[..., :256], X.lora_acc(cs, 0b101)[..., :256])
    X.lora_acc(cs, 0b111, which=1)
    wrong = cs["x"].double() @ cs["W"][0].double().T                                    # every segment reads segment 0's T block
    for s in range(3):
        wrong[..., s * 256:(s + 1) * 256] += cs["T"][0].double() @ cs["Bm"][0][s * 256:(s + 1) * 256].double().T
    msg = rejects(X.linear_bf16(wrong, cs["bias"][0]), X.linear_bf16(full, cs["bias"][0]), "neighbour's T")
    assert ", 0) at" not in msg                                                          # segment 0 (column tile 0) is right


# ------------------------------------------------------------------------------------------------ q / k norm + RoPE
@pytest.fixture(scope="module")
def qkn():
    B, M, D, K = 2, 300, 256, X.QKN_K                                                    # two heads per range: same construction, small
    cs = X.gemm_operands(B, M, 3 * D, K, 77)
    cs.update(lin=X.linear_bf16(cs["acc"], cs["bias"].float()), wq=X.norm_weights(1), wk=X.norm_weights(2), tab=X.rope_table(M, 3, B=B),
              ranges=((2 * D, 3 * D), (0, D)))
    cs["want"] = X.qk_norm_rope(cs["lin"], cs["ranges"], (cs["wq"], cs["wk"]), cs["tab"])
    return cs


def test_rope_table_and_norm_inputs_are_dyadic_and_differ_everywhere(qkn):
    tab = qkn["tab"]
    assert tab.shape == (2, 300, 64, 2) and {tuple(p) for p in tab.view(-1, 2).tolist()} == set(X.ROPE_PAIRS)
    assert (tab[:, :, 1:] != tab[:, :, :-1]).any(-1).float().mean().item() > 0.8       # neighbouring pairs differ: a shift is visible
    assert set(qkn["wq"].float().tolist()) <= set(X.NORM_WEIGHTS)
    cos, sin = X.expand_pairs(tab)
    assert cos.shape == (2, 300, 128) and torch.equal(cos[..., 0::2], cos[..., 1::2]) and torch.equal(sin[..., 1::2], tab[..., 1])
    assert torch.equal(qkn["want"][..., 256:512], qkn["lin"][..., 256:512])             # v columns untouched
    assert not torch.equal(qkn["want"][..., :256], qkn["lin"][..., :256])


def test_fault_one_rotary_pair_shifted_by_one(qkn):
    tab = qkn["tab"].clone()
    tab[1, 17] = torch.roll(tab[1, 17], 1, 0)
    got = X.qk_norm_rope(qkn["lin"], qkn["ranges"], (qkn["wq"], qkn["wk"]), tab)
    msg = rejects(got, qkn["want"], "shifted pair")
    assert "(batch 1, row 17," in msg and "batch 0" not in msg
    shared = X.qk_norm_rope(qkn["lin"], qkn["ranges"], (qkn["wq"], qkn["wk"]), qkn["tab"][0])          # sample 1 reads sample 0's table
    assert "batch 0" not in rejects(shared, qkn["want"], "shared table")
    rejects(X.qk_norm_rope(qkn["lin"], qkn["ranges"], (qkn["wk"], qkn["wq"]), qkn["tab"]), qkn["want"], "swapped norm weights")


def qkn_sensitivity(lin, ranges, weights, tab):
    """Share of the q / k elements whose bits change when every row factor moves by one fp32 step, either way."""
    mid = X.qk_norm_rope(lin, ranges, weights, tab)
    moved = torch.zeros(mid.shape, dtype=torch.bool)
    for d in (-1, 1):
        moved |= X.mismatches(X.qk_norm_rope(lin, ranges, weights, tab, r_ulps=d), mid)
    n = sum(hi - lo for lo, hi in ranges) * lin.shape[0] * lin.shape[1]
    return moved.sum().item() / n


def test_qkn_cap_is_the_measured_one_ulp_sensitivity():
    """The cap of the GPU comparison against the CPU restatement: at (M 2344, N 9216, K 256) the share of q / k elements whose stored
    bits change when the row factor r moves by one fp32 step either way -- measured: 0 of 14.4 M (two steps: 47, 3.3e-6; eight: 2008).
    The integer x of these inputs times a 24-bit r lands on a bf16 tie too rarely for one step to cross one.  X.QKN_SHARE_ONE_ULP is
    what the GPU file multiplies by four; it must be this measurement."""
    M, D, K = X.QKN_M, X.QKN_D, X.QKN_K
    for B, N in ((1, 3 * D), (1, 4 * D)):
        cs = X.gemm_operands(B, M, N, K, X.shape_seed(B, M, N, K))
        lin = X.linear_bf16(cs["acc"], cs["bias"].float())
        share = qkn_sensitivity(lin, ((2 * D, 3 * D), (0, D)), (X.norm_weights(1), X.norm_weights(2)),
                                X.rope_table(M + X.QKN_POS0, 3)[X.QKN_POS0:])
        print(f"q/k norm, N {N}: {share:.3e} of the elements change under one fp32 step of the row factor")
        assert share == X.QKN_SHARE_ONE_ULP


# ------------------------------------------------------------------------------------------------ attention
def seq_cases():
    return [(B, H, N, None) for B, H, N in X.ATTN_SHAPES + X.ATTN_PERSISTENT_SHAPES + [X.ATTN_STREAMK_SHAPE, X.ATTN_TAIL_SHAPE]] + \
           [(B, H, N, L) for (B, H, N), L in X.ATTN_SEQ_LEN_CASES]


@pytest.mark.parametrize("B,H,N,L", seq_cases())
def test_attention_generator_conditions_hold(B, H, N, L):
    seed = X.shape_seed(B, H, N)
    q, k, v, want = X.uniform_attention(B, H, N, seed, L)
    assert q.shape == (B, N, H * 128) and (q[:, :(min(L) if L else N)] == 0).all()
    q, k, v, want, bound = X.selector_attention(B, H, N, seed, L)
    assert bound < 35.0 and abs(bound - 33.94) < 0.01                                    # admissible for the reference-free stream
    if L:
        for b, n in enumerate(L):
            assert torch.isnan(v[b, n:].float()).all() and torch.isnan(q[b, n:].float()).all() and torch.isfinite(want[b, :n].float()).all()


def valid(t, L):
    """The rows below each sample's length (beyond them both sides hold NaN, which never compares equal)."""
    return t if L is None else torch.cat([t[b, :n] for b, n in enumerate(L)])


@pytest.mark.parametrize("B,H,N,L", [(B, H, N, None) for B, H, N in X.ATTN_SHAPES] + [(2, 2, 512, (512, 130))])
def test_attention_restatements_round_to_the_claimed_bits(B, H, N, L):
    seed = X.shape_seed(B, H, N)
    q, k, v, want = X.uniform_attention(B, H, N, seed, L)
    got = X.attention_reference(q, k, v, L)
    X.assert_elementwise(valid(got, L), valid(want, L), "uniform -> c")
    if L:
        assert torch.isnan(got[1, L[1]:].float()).all() and torch.isnan(want[1, L[1]:].float()).all()
    q, k, v, want, _ = X.selector_attention(B, H, N, seed, L)
    X.assert_elementwise(valid(X.attention_reference(q, k, v, L), L), valid(want, L), "selector -> v[pi]")


@pytest.fixture(scope="module")
def att():
    """(1, 3, 300): ragged in the last 64-key tile (keys 256 .. 299), three heads."""
    B, H, N = 1, 3, 300
    seed = X.shape_seed(B, H, N)
    return dict(u=X.uniform_attention(B, H, N, seed), s=X.selector_attention(B, H, N, seed), B=B, H=H, N=N)


def test_fault_one_key_dropped_for_one_query_row(att):
    for name in ("u", "s"):
        q, k, v, want = att[name][:4]
        got = want.clone()
        i, h = 123, 1
        sl = slice(h * 128, (h + 1) * 128)
        s = (q[0, i, sl].double() @ k[0, :, sl].double().T) * 128 ** -0.5
        drop = int(s.argmax()) if name == "s" else 40                                    # the selected key / any key of the uniform form
        s[drop] = -float("inf")
        got[0, i, sl] = (torch.softmax(s, -1) @ v[0, :, sl].double()).float().to(BF)
        msg = rejects(got, want, "dropped key")
        assert "128 of" in msg and "(batch 0, row 123, col 128)" in msg


def test_fault_last_valid_key_of_the_ragged_tile_replaced_by_a_padding_row(att):
    for pad in (0.0, 7.0):
        for name in ("u", "s"):
            q, k, v, want = att[name][:4]
            k2, v2 = k.clone(), v.clone()
            k2[0, 299], v2[0, 299] = pad, pad                                            # key 299 = row 43 of key tile 4 reads beyond the operand
            rejects(X.attention_reference(q, k2, v2), want, "padding row")


def test_fault_two_keys_swapped(att):
    q, k, v, want = att["s"][:4]
    k2 = k.clone()
    k2[0, 10], k2[0, 270] = k[0, 270], k[0, 10]
    msg = rejects(X.attention_reference(q, k2, v), want, "swapped keys")
    assert "768 of" in msg                                                               # two query rows per head, every column


def test_fault_two_heads_swapped(att):
    for name in ("u", "s"):
        want = att[name][3]
        got = want.clone()
        got[..., :128], got[..., 128:256] = want[..., 128:256], want[..., :128]
        rejects(got, want, "swapped heads")


def test_fault_value_column_misplaced(att):
    want = att["u"][3]
    got = want.clone()
    got[..., 5], got[..., 6] = want[..., 6], want[..., 5]
    q, k, v, w2 = att["s"][:4]
    v2 = v.clone()
    v2[..., 5], v2[..., 6] = v[..., 6], v[..., 5]
    rejects(X.attention_reference(q, k, v2), w2, "swapped value columns")
    assert (att["u"][3][0, 0, 5] != att["u"][3][0, 0, 6]) == bool(X.mismatches(got, want).any())


# ------------------------------------------------------------------------------------------------ attention, dyadic form
def test_dyadic_scale_times_log2e_is_an_eighth_in_fp32():
    scale = torch.tensor(X.DYADIC_SCALE, dtype=torch.float32)
    assert scale.item() == X.DYADIC_SCALE and X.DYADIC_SCALE == 0.08664339780807495
    assert (scale * torch.tensor(1.4426950408889634, dtype=torch.float32)).item() == 0.125
    ks = torch.arange(-256, 257).float().to(BF)
    assert bool(((ks.float() * 8.0 * 0.125).to(BF) == ks).all())                         # bf16(q * scale_log2e) = 1.0 keeps every k


def head(t, b, h, L):
    return t[b, :L, h * 128:(h + 1) * 128]


@pytest.mark.parametrize("family", X.DYADIC_FAMILIES)
@pytest.mark.parametrize("B,H,N,L", seq_cases())
def test_dyadic_generator_conditions_hold(B, H, N, L, family):
    q, k, v, want = X.dyadic_attention(B, H, N, X.shape_seed(B, H, N), L, family)
    assert q.shape == k.shape == v.shape == want.shape == (B, N, H * 128)
    lens = L or (N,) * B
    far = False
    for b, n in enumerate(lens):
        for t in (q, k, v, want):
            assert torch.isnan(t[b, n:].float()).all() and torch.isfinite(t[b, :n].float()).all()
        for h in range(H):
            qh, kh, vh = (head(t, b, h, n).double() for t in (q, k, v))
            dm = X.dyadic_column(h, torch.arange(n))
            assert bool((qh.sum(1) == 8.0).all()) and bool((qh[torch.arange(n), dm] == 8.0).all())          # one-hot times 8
            assert bool((dm[1:] != dm[:-1]).all()) and len(set(dm.tolist())) == min(n, 128)
            assert bool((kh == kh.round()).all()) and kh.abs().max().item() <= (50 if family == "bounded" else 256)
            far = far or (kh.max().item() > 200 and kh.min().item() < -180)
            c = X.dyadic_offsets(b, h, family).double()
            e = c[None, :] - kh                                                                              # [n, 128]
            assert e.min().item() >= 0 and e.max().item() <= X.DYADIC_DEPTH
            assert bool((torch.exp2(-e).sum(0) == 1.0).all())                                                # every column sums to exactly 1
            assert bool((vh == vh.round()).all()) and vh.abs().min().item() >= 1 and vh.abs().max().item() <= 64
            assert (torch.exp2(16.0 - e).T @ vh.abs()).max().item() < 2 ** 24
        if H > 1 and n > 1:
            assert not torch.equal(head(v, b, 0, n), head(v, b, 1, n))
    assert far == (family == "far")


def exp2_softmax(q, k, v, b, h, L):
    """softmax in the exp2 domain, fp64: exact on dyadic inputs (weights 2^(s - max), integer v, a power-of-two row sum)."""
    s = (head(q, b, h, L).double() @ head(k, b, h, L).double().T) * 0.125
    p = torch.exp2(s - s.max(-1, keepdim=True).values)
    return ((p @ head(v, b, h, L).double()) / p.sum(-1, keepdim=True)).float().to(BF)


@pytest.mark.parametrize("family", X.DYADIC_FAMILIES)
@pytest.mark.parametrize("B,H,N,L", [(B, H, N, None) for B, H, N in X.ATTN_SHAPES] + [(2, 2, 512, (512, 130))])
def test_dyadic_want_is_the_exact_softmax(B, H, N, L, family):
    """`want` (column sums of 2^-e v) against a plain softmax over q, k, v: bit for bit in the exp2 domain, where fp64 is exact, and within
    one bf16 step of the natural-exponential fp64 softmax (many expected values are ties of the bf16 rounding: dyadic fractions)."""
    q, k, v, want = X.dyadic_attention(B, H, N, X.shape_seed(B, H, N), L, family)
    for b, n in enumerate(L or (N,) * B):
        for h in range(H):
            X.assert_elementwise(exp2_softmax(q, k, v, b, h, n), head(want, b, h, n), f"exp2-domain softmax, sample {b} head {h}")
    ref, w = valid(X.attention_reference(q, k, v, L, scale=X.DYADIC_SCALE), L), valid(want, L)
    zero = w == 0                                                                        # an exact cancellation: fp64's exp leaves ~1e-8 there
    assert not bool((X.mismatches(ref, w, 1) & ~zero).any()) and (ref.float().abs() * zero).max().item() < 2.0 ** -20


def walk_rows(k, v, b, h, L, rows, keys=None, **kw):
    s = X.dyadic_scores(k, b, h, L, rows)
    vh = head(v, b, h, L).double()
    if keys is not None:
        s, vh = s[:, keys[0]:keys[1]], vh[keys[0]:keys[1]]
    return X.guarded_walk(s, vh, **kw)


@pytest.mark.parametrize("B,H,N", [s for s in X.ATTN_SHAPES + X.ATTN_PERSISTENT_SHAPES + [X.ATTN_STREAMK_SHAPE, X.ATTN_TAIL_SHAPE] if s[2] >= 33])
def test_dyadic_cases_move_the_guarded_reference(B, H, N):
    """The restated policy on the last head of the last sample (its first 256 rows): finishing its accumulators gives `want`; some rows
    never move (the descending columns); from five tiles on some rows move at least twice; and some move inside the last tile -- the
    ragged one wherever N is no multiple of 64 (the spike columns; at N = 33 the single tile's second unit holds the spike)."""
    for family in X.DYADIC_FAMILIES:
        q, k, v, want = X.dyadic_attention(B, H, N, X.shape_seed(B, H, N), None, family)
        rows = torch.arange(min(N, 256))
        w = walk_rows(k, v, B - 1, H - 1, N, rows)
        X.assert_elementwise(X.finish_rows(w["o"], w["l"]), head(want, B - 1, H - 1, N)[rows], f"restated guarded kernel {family}")
        assert int((w["moves"] == 0).sum()) > 0 and int((w["late"] > 0).sum()) > 0
        kinds = X.dyadic_kind(H - 1, X.dyadic_column(H - 1, rows))
        assert int(w["moves"][kinds == 1].sum()) == 0                                    # descending columns never move
        if N >= 300:
            assert int(w["moves"].max()) >= 2
            assert int(w["moves"][kinds == 0].min()) >= 2                                # ascending columns: repeatedly
            spike = head(k, B - 1, H - 1, N).double()[:, X.dyadic_column(H - 1, rows[kinds == 3])]          # [N, spike rows]
            last = 64 * ((N - 1) // 64)
            assert bool((spike[last:].max(0).values - spike[:last].max(0).values >= 5).all())               # more than W4_THR above every earlier tile


def test_dyadic_lengths_move_the_reference_per_sample():
    (B, H, N), L = X.ATTN_SEQ_LEN_CASES[0]
    q, k, v, want = X.dyadic_attention(B, H, N, X.shape_seed(B, H, N), L, "far")
    for b, n in enumerate(L):
        rows = torch.arange(min(n, 64))
        w = walk_rows(k, v, b, 5, n, rows)
        X.assert_elementwise(X.finish_rows(w["o"], w["l"]), head(want, b, 5, n)[rows], f"sample {b}")
        assert int(w["moves"].max()) >= (2 if n > 64 else 1)


def pieces_of(k, v, b, h, N, rows, tiles):
    return [walk_rows(k, v, b, h, N, rows, keys=(t0 * 64, min(N, t1 * 64))) for t0, t1 in tiles]


def test_dyadic_tail_split_pieces_end_with_different_references():
    """(1, 24, 3100) on 256 CUs: the last 56 (head, q-tile) pairs are cut at key tile 24 of 49 (joint_attention_w4).  Head 23, q-tile 0."""
    B, H, N = X.ATTN_TAIL_SHAPE
    nkv = (N + 63) // 64
    for family in X.DYADIC_FAMILIES:
        q, k, v, want = X.dyadic_attention(B, H, N, X.shape_seed(B, H, N), None, family)
        rows = torch.arange(256)
        ps = pieces_of(k, v, 0, H - 1, N, rows, [(0, nkv // 2), (nkv // 2, nkv)])
        X.assert_elementwise(X.merge_pieces(ps), head(want, 0, H - 1, N)[rows], "merged halves")
        differ = ps[0]["m"] != ps[1]["m"]
        assert int(differ.sum()) >= 128 and int((ps[0]["m"] > ps[1]["m"]).sum()) > 0 and int((ps[0]["m"] < ps[1]["m"]).sum()) > 0
        rejects(X.merge_pieces(ps, wrong=(0, 1)), head(want, 0, H - 1, N)[rows], "merged halves")


def test_dyadic_streamk_pieces_end_with_different_references():
    """(2, 5, 2304) on 256 CUs: all 45 items of a sample are dealt in ranges of 13 key tiles (share), boundaries snapped by w4_sk_bound."""
    B, H, N = X.ATTN_STREAMK_SHAPE
    nqb = (N + 255) // 256
    q, k, v, want = X.dyadic_attention(B, H, N, X.shape_seed(B, H, N), None, "bounded")
    cut = 0
    for item in (0, 7, 22, 44):
        tiles = X.streamk_pieces(H, N, B, 256, item)
        assert tiles is not None and tiles[0][0] == 0 and tiles[-1][1] == (N + 63) // 64 and len(tiles) <= 8
        h, rows = item // nqb, (item % nqb) * 256 + torch.arange(256)
        ps = pieces_of(k, v, 1, h, N, rows, tiles)
        X.assert_elementwise(X.merge_pieces(ps), head(want, 1, h, N)[rows], f"merged pieces of item {item}")
        if len(tiles) > 1:
            cut += 1
            ms = torch.stack([p["m"] for p in ps])
            assert int((ms.max(0).values != ms.min(0).values).sum()) >= 128
            rejects(X.merge_pieces(ps, wrong=(len(ps) - 1, 0)), head(want, 1, h, N)[rows], "merged pieces")
    assert cut >= 3


@pytest.fixture(scope="module")
def dy():
    """(1, 3, 300), bounded family, head 1, all rows padded to whole q-blocks by the kernel's row clamp: ragged in the last tile (keys 256 .. 299)."""
    B, H, N, h = 1, 3, 300, 1
    q, k, v, want = X.dyadic_attention(B, H, N, X.shape_seed(B, H, N), None, "bounded")
    rows = torch.arange(320).clamp(max=N - 1)
    s, vh = X.dyadic_scores(k, 0, h, N, rows), head(v, 0, h, N).double()
    base = X.guarded_walk(s, vh)
    wh = head(want, 0, h, N)[rows]
    X.assert_elementwise(X.finish_rows(base["o"], base["l"]), wh, "the restatement itself")
    return dict(s=s, v=vh, want=wh, base=base, rows=rows, h=h, N=N)


def faulted(dy, what, s=None, v=None, **fault):
    w = X.guarded_walk(dy["s"] if s is None else s, dy["v"] if v is None else v, fault or None)
    return rejects(X.finish_rows(w["o"], w["l"]), dy["want"], what)


def a_move(dy, nth=0):
    """(unit, q-block) of a reference move of a whole-row q-block that is not the very first after the pin."""
    ev = [(u, g) for u, g in dy["base"]["events"] if u >= 2 and g < 8]
    assert len(ev) > 4
    return ev[len(ev) // 2 + nth]


def test_fault_reference_move_without_the_rescale(dy):
    u, g = a_move(dy)
    faulted(dy, "skipped rescale", kind="skip_rescale", unit=u, block=g)


def test_fault_rescale_applied_to_the_other_q_block(dy):
    u, g = a_move(dy)
    faulted(dy, "rescale of the other q-block", kind="rescale_other", unit=u, block=g)


def test_fault_scores_not_shifted_after_a_move(dy):
    u, g = a_move(dy)
    faulted(dy, "unshifted scores", kind="no_shift", unit=u, block=g)


def test_fault_merge_piece_weighted_with_another_reference(dy):
    ps = [X.guarded_walk(dy["s"][:, a:b], dy["v"][a:b]) for a, b in ((0, 128), (128, 300))]
    X.assert_elementwise(X.merge_pieces(ps), dy["want"], "merge")
    rejects(X.merge_pieces(ps, wrong=(1, 0)), dy["want"], "merge")


def test_fault_first_masked_key_admitted_with_a_graded_weight(dy):
    """Key 300, the first masked key of the ragged tile, as a key its column could hold: weight 2^-9 of the row's sum, beside the graded
    weights of keys 288 .. 299."""
    c = X.dyadic_offsets(0, dy["h"], "bounded").double()[X.dyadic_column(dy["h"], dy["rows"])]
    s = torch.cat([dy["s"], (c - 9.0)[:, None]], 1)
    v = torch.cat([dy["v"], torch.full((1, 128), 64.0, dtype=torch.float64)], 0)
    faulted(dy, "admitted masked key", s=s, v=v)


def test_fault_two_keys_with_different_exponents_swapped(dy):
    s = dy["s"].clone()
    i = 77
    j1, j2 = 290, int((s[i] != s[i, 290]).nonzero()[0])
    s[i, j1], s[i, j2] = dy["s"][i, j2], dy["s"][i, j1]
    msg = faulted(dy, "swapped keys", s=s)
    assert "(batch 0, row 77," in msg


def test_fault_weights_of_one_row_doubled_in_one_tile(dy):
    for tile in (0, 2, 4):
        msg = faulted(dy, "doubled weights", kind="double", tile=tile, row=133)
        assert "(batch 0, row 133," in msg and "1 rows" in msg


def test_a_constant_added_to_a_rows_scores_is_invisible_to_the_dyadic_form(dy):
    """What the form cannot see (a wrong constant in every score of a row cancels in the normalisation); the selector form's margin does."""
    s = dy["s"].clone()
    s[40] += 3.0
    s[200] -= 7.0
    w = X.guarded_walk(s, dy["v"])
    X.assert_elementwise(X.finish_rows(w["o"], w["l"]), dy["want"], "shifted row")


# ------------------------------------------------------------------------------------------------ attention64
@pytest.mark.parametrize("N", X.ATTN64_NS)
@pytest.mark.parametrize("H", X.ATTN64_HS)
def test_attention64_constructions(N, H):
    B, seed = 2, X.shape_seed(2, H, N, 64)
    q, k, v, want = X.uniform_attention(B, H, N, seed, None, 64)
    X.assert_elementwise(X.attention64_reference(q, k, v, 0.125), want, "uniform")
    for causal in (False, True):
        q, k, v, want, _ = X.selector_attention(B, H, N, seed, None, 64, X.ATTN64_MULT, 0.125, causal)
        X.assert_elementwise(X.attention64_reference(q, k, v, 0.125, causal=causal), want, f"selector causal={causal}")
    for delta in sorted({-(N - 1), -1, 0, 1, N - 1}):
        if abs(delta) > N - 1:
            continue
        q, k, v, bias, want = X.bias_selector_attention(B, H, N, delta, seed)
        X.assert_elementwise(X.attention64_reference(q, k, v, 0.125, rel_bias=bias), want, f"bias selector delta={delta}")
        if N > 2 and abs(delta) < N - 1:
            off = torch.roll(bias, 1, 1)                                                 # the index formula off by one
            rejects(X.attention64_reference(q, k, v, 0.125, rel_bias=off), want, "bias index")


def graded64(N, H, mode):
    q, k, v, bias = X.graded_attention64(2, H, N, X.shape_seed(2, H, N, 64, 1), mode)
    return q, k, v, dict(rel_bias=bias, causal=mode == "causal")


@pytest.mark.parametrize("N,H,mode", X.attention64_graded_cases())
def test_attention64_graded_form_grades_and_its_chain_is_the_softmax(N, H, mode):
    """Natural scores are small integers; the maximum of most 32-key blocks exceeds every block before it (alpha != 1); the restatement
    with the kernel's rounding points is the fp64 softmax up to the bf16 rounding of its weights (2^-9 of each, |v| <= 64: 0.125) and the
    final rounding (2^-9 |out| <= 0.125); another mask or a shifted bias index is another answer."""
    q, k, v, kw = graded64(N, H, mode)
    s = (q.double().view(2, N, H, 64).transpose(1, 2) @ k.double().view(2, N, H, 64).transpose(1, 2).transpose(-1, -2)) * 0.125
    assert bool((s == s.round()).all()) and s.abs().max().item() <= 72
    nb = (N + 31) // 32
    if nb > 1 and mode == "plain":
        bm = torch.stack([s[..., kb * 32:(kb + 1) * 32].max(-1).values for kb in range(nb)], -1).cummax(-1).values
        assert (bm[..., 1:] > bm[..., :-1]).double().mean().item() > 0.5
    chain = X.attention64_graded_chain(q, k, v, 0.125, **kw)
    ref = X.attention64_reference(q, k, v, 0.125, **kw)
    assert (chain.float() - ref.float()).abs().max().item() <= 0.25
    if N > 2:
        bias = torch.roll(kw["rel_bias"], 1, 1) if mode == "bias" else None
        other = X.attention64_graded_chain(q, k, v, 0.125, rel_bias=bias, causal=mode != "causal")
        assert int(X.mismatches(other, chain, 1).sum()) > 0


def test_attention64_graded_share_is_the_measured_sensitivity():
    """Every exponential of the chain (weights and alpha) and the final row sum moved by one fp32 step, in each of the eight sign
    combinations: the share of all the cases' output elements whose bf16 value changes under any of them."""
    n = m = 0
    for N, H, mode in X.attention64_graded_cases():
        q, k, v, kw = graded64(N, H, mode)
        mid = X.attention64_graded_chain(q, k, v, 0.125, **kw)
        moved = torch.zeros(mid.shape, dtype=torch.bool)
        for e, s in ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (1, -1), (-1, 1), (-1, -1)):
            moved |= X.mismatches(X.attention64_graded_chain(q, k, v, 0.125, exp_ulps=e, sum_ulps=s, **kw), mid)
        n, m = n + mid.numel(), m + int(moved.sum())
    print(f"attention64 graded: {m} of {n} elements ({m / n:.3e}) change under one fp32 step of the exponentials and the row sum")
    assert m / n == X.ATTN64_GRADED_SHARE


# ------------------------------------------------------------------------------------------------ convolution
@pytest.mark.parametrize("B,H,W,Cin,Cout,stride,up,pad_lo,with_res", X.CONV_CASES)
def test_conv_generator_condition_and_border_fault(B, H, W, Cin, Cout, stride, up, pad_lo, with_res):
    cs = X.conv_operands(B, H, W, Cin, Cout, X.shape_seed(B, H, W, Cin, Cout), stride=stride, up=up, with_res=with_res)
    assert cs["want"].shape[0] == B and cs["want"].shape[3] == Cout and cs["x"].shape == (B, H, W, Cin)
    acc = cs["acc"].clone()                                                              # a border pixel takes a tap from outside the image
    acc[0, 0, 0] += cs["w"][:, 0, 0, :].double() @ cs["x"][0, 0, 0].double()
    lin = X.linear_bf16(acc, cs["bias"].float())
    rejects((cs["res"] + lin) if with_res else lin, cs["want"], "border tap")


@pytest.mark.parametrize("B,H,W,Cin,Cout", [c[:5] for c in X.CONV_NARROW_CASES + X.CONV_PAIR_CASES])
def test_conv_generator_condition_holds_for_the_narrow_and_pair_cases(B, H, W, Cin, Cout):
    X.conv_operands(B, H, W, Cin, Cout, X.shape_seed(B, H, W, Cin, Cout), with_res=True)


# ------------------------------------------------------------------------------------------------ rows with exact statistics
def test_zero_sum_rows_meet_their_conditions_in_every_summation_order():
    for D, offset in ((8, 0), (520, 3), (3072, 3), (100, 0)):
        x = X.zero_sum_rows((2, 5), D, X.shape_seed(D, offset), X.LN_AMP, offset)
        assert x.shape == (2, 5, D) and bool((x == x.round()).all()) and x.abs().max().item() <= X.LN_AMP + offset
        assert x.unique().numel() > 8 and not torch.equal(x[0, 0], x[0, 1])
        for order in (torch.arange(D), torch.arange(D - 1, -1, -1), torch.randperm(D, generator=X.gen(1))):     # fp32, three orders
            assert bool((x[..., order].cumsum(-1)[..., -1] == offset * D).all())
            assert torch.equal(((x - offset) ** 2)[..., order].cumsum(-1)[..., -1].double(), ((x.double() - offset) ** 2).sum(-1))
        mean, r = X.layernorm_factor(x, 1e-6)
        assert bool((mean == offset).all()) and r.shape == (2, 5, 1)
    with pytest.raises(AssertionError):
        X.zero_sum_rows((1,), 1 << 20, 1, 16)                                             # partial sums would leave 2^24
    with pytest.raises(AssertionError, match="bf16 number"):
        X.zero_sum_rows((1,), 8, 1, 300, 1)


@pytest.mark.parametrize("C,groups,HW", X.GN_CASES)
def test_zero_sum_groups_meet_their_conditions(C, groups, HW):
    cs = X.gn_case(C, groups, HW)
    off = 3.0 if (C, groups, HW) == X.GN_OFFSET_CASE else 0.0
    assert bool((cs["mean"] == off).all()) and cs["x"].shape == (2, HW, C)
    assert bool((cs["x"].to(BF).float() == cs["x"]).all())
    if HW > 1:
        assert cs["rstd"].unique().numel() > groups                                      # the statistics tell the (sample, group) pairs apart
    if off:
        n = HW * C // groups
        assert n & (n - 1) == 0 and float(torch.tensor(1.0 / n, dtype=torch.float32)) * n == 1.0


def test_chains_are_the_kernels_rounding_points_and_reject_the_faults_they_are_there_for():
    B, R, D = 2, 5, 520
    cs = X.ln_case(B, R, D, 3)
    x, mean, r = cs["x"], cs["mean"], cs["r"]
    sh, sc, sh2, sc2 = X.mod_slices(cs["mod"], D)
    want = X.ln_modulate_chain(x, sh, sc, mean, r)
    xn = ((x.double() - mean.double()) * r.double()).float().to(BF)                       # fp64 restatement, rounded where the chain rounds
    t = (1.0 + sc.double()).float().to(BF)
    prod = (xn.double() * t.double()[:, None]).float().to(BF)
    assert torch.equal(want, (prod.double() + sh.double()[:, None]).float().to(BF))
    split = X.ln_modulate_chain(x, sh, sc, mean, r, 2, sh2, sc2)
    assert torch.equal(split[:, 2:], want[:, 2:]) and torch.equal(split[:, :2], X.ln_modulate_chain(x, sh2, sc2, mean, r)[:, :2])
    rejects(split, want, "second modulation")
    # (1 + scale) not rounded to bf16 before the product
    loose = (xn.float() * (1.0 + sc.float())[:, None]).to(BF) + sh[:, None]
    rejects(loose, want, "unrounded scale term")
    # 1 / D taken from a chunk count padded to the next 64 chunks: the mean of the offset rows moves
    Dp = (D // 8 + 63) // 64 * 64 * 8
    rejects(X.ln_modulate_chain(x, sh, sc, mean * (D / Dp), r), want, "padded D")
    rejects(X.ln_modulate_chain(x, sh, sc, mean, r * (D / Dp) ** 0.5), want, "padded D in the variance")
    # the last chunk of a row taken from its clamped neighbour
    x2 = x.clone()
    x2[..., D - 8:] = x[..., D - 16:D - 8]
    rejects(X.ln_modulate_chain(x2, sh, sc, mean, r), want, "clamped chunk")
    la = X.lna_case(5, 520)
    w = X.layernorm_affine_chain(la["x"], la["gamma"], la["beta"], la["mean"], la["r"])
    e = ((la["x"].double() - la["mean"].double()) * la["r"].double()).float().double() * la["gamma"].double()
    assert torch.equal(w, (e.float().double() + la["beta"].double()).float().to(BF))
    rejects(((la["x"] - la["mean"]) * la["r"]).to(BF) * la["gamma"] + la["beta"], w, "three roundings")
    tc = X.t5_case(5, 100, True)
    w = X.t5_rmsnorm_chain(tc["x"], tc["w"], tc["r"])
    assert torch.equal(w, (tc["w"].double() * (tc["x"].double() * tc["r"].double()).float().to(BF).double()).float().to(BF))
    rejects((tc["w"].float() * (tc["x"] * tc["r"])).to(BF), w, "one rounding")


def test_groupnorm_chain_and_the_second_group_slot():
    C, groups, HW = 256, 64, 300
    cs = X.gn_case(C, groups, HW)
    mean, rstd = cs["mean"].float(), cs["rstd"].float()
    want = X.groupnorm_chain(cs["x"], cs["gamma"], cs["beta"], mean, rstd, groups, False)
    ref = torch.nn.functional.group_norm(cs["x"].double().permute(0, 2, 1), groups, cs["gamma"].double(), cs["beta"].double(), 1e-6).permute(0, 2, 1)
    X.assert_elementwise(want, ref.float().to(BF), "chain vs F.group_norm in fp64", ulps=1, cap=1e-3)
    bad = rstd.clone()
    bad[:, 32:] = 1.0                                                                    # groups 32 .. 63 never finalised
    msg = rejects(X.groupnorm_chain(cs["x"], cs["gamma"], cs["beta"], mean, bad, groups, False), want, "second slot")
    assert "col 128)" in msg or "col 129)" in msg or "col 13" in msg
    y = X.groupnorm_chain(cs["x"], cs["gamma"], cs["beta"], mean, rstd, groups, True)
    assert torch.equal(y, torch.nn.functional.silu(want.double()).float().to(BF))
    sure = X.settled(X.silu64(want), 2.0 ** -18)
    assert 0.99 < sure.float().mean().item() <= 1.0


def _moved(chain, r, steps):
    """bool mask: elements whose bits change when r moves by up to `steps` fp32 steps either way."""
    mid = chain(r)
    moved = torch.zeros(mid.shape, dtype=torch.bool)
    for d in range(1, steps + 1):
        for sgn in (-1, 1):
            moved |= X.mismatches(chain(X.nudge(r, sgn * d)), mid)
    return mid, moved


def test_ln_share_is_the_measured_one_step_sensitivity():
    """Every (D, rows, offset) of the GPU file, B = 2, amp 8, split and plain (the same arithmetic per row)."""
    n = m = 0
    for D in X.LN_DS:
        for R in X.LN_ROWS:
            for off in X.LN_OFFSETS:
                cs = X.ln_case(2, R, D, off)
                sh, sc, _, _ = X.mod_slices(cs["mod"], D)
                mid, moved = _moved(lambda r: X.ln_modulate_chain(cs["x"], sh, sc, cs["mean"], r), cs["r"], 1)
                n, m = n + mid.numel(), m + int(moved.sum())
    print(f"ln_modulate: {m} of {n} elements ({m / n:.3e}) change under one fp32 step of the row factor")
    assert m / n == X.LN_SHARE


def test_ln_affine_share_is_the_measured_sensitivity():
    n = m = 0
    for D in X.LNA_DS:
        for rows in X.LNA_ROWS:
            cs = X.lna_case(rows, D)
            f = lambda r, fused=False: X.layernorm_affine_chain(cs["x"], cs["gamma"], cs["beta"], cs["mean"], r, fused)
            mid, moved = _moved(f, cs["r"], 1)
            moved |= X.mismatches(f(cs["r"], True), mid)
            n, m = n + mid.numel(), m + int(moved.sum())
    print(f"layernorm (affine): {m} of {n} elements ({m / n:.3e}) change under one fp32 step of the row factor or the contracted multiply-add")
    assert m / n == X.LN_AFFINE_SHARE


def test_gn_share_is_the_measured_sensitivity():
    n = m = 0
    for C, groups, HW in X.GN_CASES:
        cs = X.gn_case(C, groups, HW)
        f = lambda r, fused=False: X.groupnorm_chain(cs["x"], cs["gamma"], cs["beta"], cs["mean"], r, groups, False, fused)
        mid, moved = _moved(f, cs["rstd"].float(), 2)
        moved |= X.mismatches(f(cs["rstd"].float(), True), mid)
        n, m = n + mid.numel(), m + int(moved.sum())
    print(f"groupnorm: {m} of {n} elements ({m / n:.3e}) change under two fp32 steps of rstd or the contracted multiply-add")
    assert m / n == X.GN_SHARE


def test_t5_share_is_the_measured_one_step_sensitivity():
    n = m = 0
    for D in X.T5_DS:
        for rows in X.T5_ROWS:
            for f32 in (True, False):
                cs = X.t5_case(rows, D, f32)
                mid, moved = _moved(lambda r: X.t5_rmsnorm_chain(cs["x"], cs["w"], r), cs["r"], 1)
                n, m = n + mid.numel(), m + int(moved.sum())
    print(f"T5 rmsnorm: {m} of {n} elements ({m / n:.3e}) change under one fp32 step of the row factor")
    assert m / n == X.T5_SHARE


def test_scheduler_chains_are_the_reference_steps():
    from oracle import sched_oracle as so
    g = X.gen(5)
    v, x, eps = X.arbitrary_bf16((37, 64), 1), X.arbitrary_bf16((37, 64), 2), torch.randn(37, 64, generator=g)
    ds = torch.tensor(-0.03125)
    assert torch.equal(X.euler_chain(v, x, -0.03125), so.euler_step(v, x, torch.tensor(1.0), torch.tensor(1.0) + ds))


# ------------------------------------------------------------------------------------------------ tests/test_exact_layout_gpu.py
def test_rope_share_is_the_measured_sensitivity():
    """Every case of the GPU file: the q / k elements whose bits change when the row factor moves one fp32 step either way, or when either
    product of the rotation is contracted into the add."""
    n = m = 0
    for case in X.rope_cases():
        cs = X.rope_case(*case)
        f = lambda r, order=0: X.rms_rope_chain(cs["x"], cs["w"], cs["cos"], cs["sin"], r, order)
        mid, moved = _moved(f, cs["r"], 1)
        for order in (1, 2):
            moved |= X.mismatches(f(cs["r"], order), mid)
        n, m = n + mid.numel(), m + int(moved.sum())
    print(f"rmsnorm_rope: {m} of {n} elements ({m / n:.3e}) change under one fp32 step of the row factor or a contracted rotation")
    assert m / n == X.ROPE_SHARE


def test_rope_chain_is_the_reference_and_the_tables_are_not_dyadic():
    """On one case: the chain is the reference's rms_norm + apply_rope to a bf16 step (the reference rounds the same points; its fp32 rsqrt and
    rotation may differ in the last place), and most of the table is neither 0, +-1 nor +-0.5."""
    from oracle import flux_oracle as fo
    H, B, N, T = 5, 2, 5, 0
    cs = X.rope_case(H, B, N, T, True)
    want = X.rms_rope_chain(cs["x"], cs["w"], cs["cos"], cs["sin"], cs["r"])
    assert ((cs["cos"].abs() != 1) & (cs["cos"].abs() != 0.5) & (cs["cos"] != 0)).float().mean().item() > 0.6
    for b in range(B):
        for k, wt in ((0, cs["ws"][0]), (1, cs["ws"][1])):
            x = cs["x"][b, :, k * H:(k + 1) * H].to(BF).permute(1, 0, 2)[None]                        # [1, H, N, 128]
            ref = fo.apply_rope(fo.rms_norm(x, wt), cs["cos"][b], cs["sin"][b])
            X.assert_elementwise(want[b, :, k * H:(k + 1) * H].permute(1, 0, 2), ref[0], "chain against the oracle", ulps=1)


def test_fault_rope_weight_of_the_other_stream_or_the_other_projection():
    H, B, N, T = 5, 2, 5, 2
    cs = X.rope_case(H, B, N, T, False)
    f = lambda w: X.rms_rope_chain(cs["x"], w, cs["cos"], cs["sin"], cs["r"])
    want = f(cs["w"])
    flat = lambda t: t.reshape(B, N, -1)
    msg = rejects(flat(f(X.rope_pick_weights(cs["ws"], B, N, H, T + 1))), flat(want), "text weights for an image row", ulps=1)
    assert "row 2," in msg and "row 1," not in msg and "row 3," not in msg
    wrong = cs["w"].clone()
    wrong[1, 4, H - 1] = cs["w"][1, 4, H]                                                            # the last q head of one token takes the k weight
    msg = rejects(flat(f(wrong)), flat(want), "k weight for a q row", ulps=1)
    assert "(batch 1, row 4," in msg and "batch 0" not in msg


def test_timestep_window_admits_the_oracle_and_rejects_a_zeroed_sine_half():
    from oracle import flux_oracle as fo
    t = torch.tensor(X.TIMESTEPS)
    lo, hi = X.timestep_window(t)
    emb = fo.timestep_embedding(t).to(BF)
    X.assert_in_window(emb, lo, hi, "oracle")
    assert bool((emb[0, :128] == 1).all()) and bool((emb[0, 128:] == 0).all())           # t = 0: 1 .. 1 | 0 .. 0, which the GPU file asserts on its own
    zeroed = emb.clone()
    zeroed[:, 128:] = 0
    with pytest.raises(AssertionError, match=r"zeroed sines.*first \(row 1, col 128\)"):                   # t = 1e-3: sines of 1e-3 .. 1e-7
        X.assert_in_window(zeroed, lo, hi, "zeroed sines")
    with pytest.raises(AssertionError, match="zeroed sines"):
        X.assert_in_window(zeroed[1:2], lo[1:2], hi[1:2], "zeroed sines")
    shifted = emb.clone()
    shifted[:, 128:] = torch.roll(emb[:, 128:], 1, 1)                                                  # the wrong j
    with pytest.raises(AssertionError, match="wrong j"):
        X.assert_in_window(shifted[1:2], lo[1:2], hi[1:2], "wrong j")


def test_sample_pack_inputs_are_settled_almost_everywhere():
    """The GPU check is bit-equality where exp64 is settled at 2^-18 and admits the neighbours of std elsewhere: the exception must be rare."""
    n = m = 0
    for case in X.SAMPLE_PACK_CASES:
        cs = X.sample_pack_case(*case)
        for v in X.SAMPLE_PACK_LOGVARS:
            assert bool((cs["logvar"] == v).any())
        sure = X.settled(X.sample_pack_std64(cs["logvar"]), 2.0 ** -18)
        n, m = n + sure.numel(), m + int(sure.sum())
    print(f"sample_pack: exp settled on {m} of {n} elements")
    assert m / n > 0.99
