"""GPU tests of the runtime (unmerged) LoRA tail of the persistent GEMM: tfx_gemm_bf16_lora computes
    y = epi(x @ W^T + t @ B^T + bias),   t = bf16(c * (x @ A^T))
in ONE fp32 accumulation (the low-rank update is a K-extension of the tile), so that the fused q / k RMSNorm + RoPE epilogue sees the
adapted projection.  Reference: an fp32 torch restatement of the same formula with the same rounding of t.

Tolerances are the ones tests/test_kernels_gpu.py applies to the same epilogues without the tail: close() with max_rel = 1e-2 and
mae_rel = 2e-3 for the plain epilogues; for the fused q / k norm the per-pair bound of
test_gemm_qkn_entry_point_matches_gemm_plus_separate_norm_rope_pass (2^-6 of the rotation pair's length, fewer than 2 % of the elements
different) against tfx_gemm_bf16_lora without the norm followed by tfx_rmsnorm_rope."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
EPIS = ("bias", "gelu", "gate_res", "qkn")
SHAPES = [(768, 256), (9216, 3072), (21504, 3072), (3072, 12288)]


@pytest.fixture(scope="module")
def ops():
    from textflux_amd import ops as o
    return o


def rnd(shape, seed, scale=1.0):
    return (torch.randn(shape, device="cuda", generator=torch.Generator("cuda").manual_seed(seed)) * scale).to(BF)


def close(got, ref, max_rel=1e-2, mae_rel=2e-3):      # tests/test_kernels_gpu.py:30, on the device (the references here are large)
    got, ref = got.float(), ref.float()
    assert got.shape == ref.shape
    assert torch.isfinite(got).all()
    err = (got - ref).abs()
    assert err.max().item() <= max_rel * ref.abs().max().item() + 1e-6, (err.max().item(), ref.abs().max().item())
    assert err.mean().item() <= mae_rel * ref.abs().mean().item() + 1e-7, (err.mean().item(), ref.abs().mean().item())


def layout(N, K):
    """(segment columns, segments, mask, q range, k range, first GELU column) of the fused weight with N rows."""
    if N == 21504:                                   # [k; v; q; mlp] of a single block: the mlp segment carries no adapter
        return 3072, 4, 0b0111, (6144, 9216), (0, 3072), 9216
    if K == 12288:                                   # one target (ff.net.2 / the single blocks' proj_out)
        return N, 1, 0b1, (2048, 3072), (0, 1024), 2048
    D = N // 3                                       # [k; v; q]
    return D, 3, 0b111, (2 * D, 3 * D), (0, D), 2 * D


def make_case(ops, M, N, K, R, batch, seed=0):
    seg_cols, nseg, mask, qr, kr, gelu_from = layout(N, K)
    x = rnd((batch, M, K), seed + 1)
    wb = torch.zeros(N, K + R, dtype=BF, device="cuda")
    wb[:, :K] = rnd((N, K), seed + 2, 0.05)
    r_true = R - 24                                  # a rank that is not a multiple of 128: the padded columns stay zero
    for s in range(nseg):
        if mask >> s & 1:
            wb[s * seg_cols:(s + 1) * seg_cols if s + 1 < nseg else N, K:K + r_true] = rnd(
                ((seg_cols if s + 1 < nseg else N - s * seg_cols), r_true), seed + 10 + s, 0.2)
    A = torch.zeros(nseg, R, K, dtype=BF, device="cuda")
    A[:, :r_true] = rnd((nseg, r_true, K), seed + 3, 0.05)
    c = 0.25 + 0.5 * torch.rand(nseg, generator=torch.Generator().manual_seed(seed + 4)).cuda()
    buf, xv, tv = ops.lora_operands(x, nseg * R)
    t = (c.view(1, 1, nseg, 1) * (x.float() @ A.float().view(nseg * R, K).T).view(batch, M, nseg, R)).to(BF)   # t = bf16(c * x A^T)
    tv.copy_(t.view(batch, M, nseg * R))
    bias = rnd((N,), seed + 5)
    return dict(x=xv, t=tv, buf=buf, wb=wb, bias=bias, seg_cols=seg_cols, nseg=nseg, mask=mask, qr=qr, kr=kr, gelu_from=gelu_from)


def reference(cs, K, R, N):
    """fp32: x W^T + t_seg B^T + bias (before the epilogue's own arithmetic)."""
    x, t, wb = cs["x"].float(), cs["t"].float(), cs["wb"].float()
    lin = x @ wb[:, :K].T + cs["bias"].float()
    for s in range(cs["nseg"]):
        if cs["mask"] >> s & 1:
            lo, hi = s * cs["seg_cols"], ((s + 1) * cs["seg_cols"] if s + 1 < cs["nseg"] else N)
            lin[..., lo:hi] += t[..., s * R:(s + 1) * R] @ wb[lo:hi, K:].T
    return lin


def rope_tables(M, seed):
    ang = torch.randn((M, 64), generator=torch.Generator().manual_seed(seed)) * 3.0
    cs = torch.stack([torch.cos(ang), torch.sin(ang)], -1).contiguous().cuda()
    return cs, torch.cos(ang).repeat_interleave(2, 1).contiguous().cuda(), torch.sin(ang).repeat_interleave(2, 1).contiguous().cuda()


def qkn_check(sep, fused, ranges):
    """the bound of tests/test_kernels_gpu.py:192-198: columns outside q / k identical, q / k within 2^-6 of the rotation pair."""
    N = sep.shape[-1]
    inside = torch.zeros(N, dtype=torch.bool, device=sep.device)
    for lo, hi in ranges:
        inside[lo:hi] = True
    assert torch.isfinite(fused.float()).all()
    assert torch.equal(fused[..., ~inside], sep[..., ~inside])
    for lo, hi in ranges:
        x, y = sep[..., lo:hi].float(), fused[..., lo:hi].float()
        diff = (x - y).abs()
        pair = (x.reshape(*x.shape[:-1], -1, 2) ** 2).sum(-1).sqrt().repeat_interleave(2, dim=-1)
        assert (diff <= 2 ** -6 * pair + 1e-6).all(), (lo, (diff / (2 ** -6 * pair + 1e-6)).max().item())
        assert (diff > 0).float().mean().item() < 2e-2


@pytest.mark.parametrize("batch", [1, 2])
@pytest.mark.parametrize("R", [128, 256])
@pytest.mark.parametrize("N,K", SHAPES)
@pytest.mark.parametrize("M", [80, 1664, 4608])
def test_lora_tail_matches_fp32_restatement(ops, M, N, K, R, batch):
    cs = make_case(ops, M, N, K, R, batch)
    kw = dict(K=K, R=R, seg_cols=cs["seg_cols"], nseg=cs["nseg"], seg_mask=cs["mask"], bias=cs["bias"])
    lin = reference(cs, K, R, N)
    for epi in EPIS:
        if epi == "bias":
            close(ops.gemm_lora(cs["x"], cs["t"], cs["wb"], **kw), lin.to(BF))
        elif epi == "gelu":
            g0 = cs["gelu_from"]
            got = ops.gemm_lora(cs["x"], cs["t"], cs["wb"], epilogue=ops.EPI_BIAS_GELU, gelu_from_col=g0, **kw)
            ref = torch.cat([lin[..., :g0], torch.nn.functional.gelu(lin[..., g0:].to(BF).float(), approximate="tanh")], -1)
            close(got, ref.to(BF))
        elif epi == "gate_res":
            gate, res = rnd((batch, N), 21), rnd((batch, M, N), 22)
            got = ops.gemm_lora(cs["x"], cs["t"], cs["wb"], epilogue=ops.EPI_BIAS_GATE_RES, gate=gate, res=res, **kw)
            ref = res.float() + (gate.float()[:, None, :] * lin.to(BF).float()).to(BF).float()
            close(got, ref.to(BF))
            del gate, res, ref
        else:
            wq, wk = (1 + 0.1 * rnd((128,), 31).float()).to(BF), (1 + 0.1 * rnd((128,), 32).float()).to(BF)
            tab, cos, sin = rope_tables(M, 33)
            sep = ops.gemm_lora(cs["x"], cs["t"], cs["wb"], **kw)
            close(sep, lin.to(BF))
            H = (cs["qr"][1] - cs["qr"][0]) // 128
            ops.rmsnorm_rope_(sep, cs["qr"][0], cs["kr"][0], H, 0, wq, wk, wq, wk, cos, sin)
            q = dict(norm_q=wq, norm_k=wk, rope_cs=tab, q_range=cs["qr"], k_range=cs["kr"])
            fused = ops.gemm_lora(cs["x"], cs["t"], cs["wb"], qkn=q, **kw)
            qkn_check(sep, fused, (cs["qr"], cs["kr"]))
            assert torch.equal(ops.gemm_lora(cs["x"], cs["t"], cs["wb"], qkn=q, **kw), fused)      # deterministic
        got = None
    # nothing was written into the operands
    assert torch.equal(cs["buf"][0][..., :K], cs["x"]) and torch.isfinite(cs["buf"].float()).all()


@pytest.mark.parametrize("M,N,K,batch", [(4608, 9216, 3072, 2), (1664, 21504, 3072, 1), (4608, 3072, 12288, 1), (2304 + 40, 768, 256, 2)])
def test_all_zero_up_projection_reproduces_the_plain_gemm_bit_for_bit(ops, M, N, K, batch):
    """Exact zeros added to the accumulators change nothing: with Bcat = 0 the tail kernel's output equals the persistent whole-tile
    kernel's (tfx_gemm_bf16 variant 3: no K-sliced units) bit for bit, for every epilogue; so does a launch whose mask skips every tail."""
    R = 128
    cs = make_case(ops, M, N, K, R, batch, seed=100)
    cs["wb"][:, K:] = 0
    w = cs["wb"][:, :K]
    gate, res = rnd((batch, N), 121), rnd((batch, M, N), 122)
    for epi, extra in ((ops.EPI_BIAS, {}), (ops.EPI_BIAS_GELU, dict(gelu_from_col=cs["gelu_from"])),
                       (ops.EPI_BIAS_GATE_RES, dict(gate=gate, res=res)), (ops.EPI_BIAS_RES, dict(res=res))):
        base = ops.gemm(cs["x"], w, cs["bias"], epilogue=epi, variant=3, **extra)
        for mask in (cs["mask"], 0):
            got = ops.gemm_lora(cs["x"], cs["t"], cs["wb"], K=K, R=R, seg_cols=cs["seg_cols"], nseg=cs["nseg"], seg_mask=mask,
                                bias=cs["bias"], epilogue=epi, **extra)
            assert torch.equal(got, base), (epi, mask)


def test_masked_segment_ignores_its_tail_operands(ops):
    """The mlp segment of a [k; v; q; mlp] weight carries no adapter: garbage in its Bm rows and in its T block must not reach the output."""
    M, N, K, R = 1664, 21504, 3072, 128
    cs = make_case(ops, M, N, K, R, 1, seed=200)
    kw = dict(K=K, R=R, seg_cols=cs["seg_cols"], nseg=cs["nseg"], seg_mask=cs["mask"], bias=cs["bias"])
    clean = ops.gemm_lora(cs["x"], cs["t"], cs["wb"], **kw)
    cs["wb"][9216:, K:] = 7.0
    cs["t"][..., 3 * R:] = 5.0
    assert torch.equal(ops.gemm_lora(cs["x"], cs["t"], cs["wb"], **kw), clean)


@pytest.mark.parametrize("fused_norm", [False, True])
def test_row_split_text_rows_take_the_text_linear_and_its_up_projection(ops, fused_norm):
    """The joint [text | image] launch of a double block: rows below split_row use the second weight set -- its W, its bias, its Bm (stored
    behind its rows) and its norm weights --, and the text rows of T come from the text Linear's A.  Equal to two separate launches, bit
    for bit (same tiles, same kernel, same accumulation order)."""
    T, S, D, K, R, B = 512, 1152, 1024, 1024, 128, 2
    M, N = T + S, 3 * D
    x = rnd((B, M, K), 301)
    pair = torch.zeros(2, N, K + R, dtype=BF, device="cuda")           # [img; txt] as one tensor: W2 above W inside one descriptor
    pair[:, :, :K] = rnd((2, N, K), 302, 0.05)
    pair[:, :, K:K + 16] = rnd((2, N, 16), 303, 0.2)
    bias = rnd((2, N), 304)
    _, xv, tv = ops.lora_operands(x, 3 * R)
    tv.copy_(rnd((B, M, 3 * R), 305, 0.3))
    kw = dict(K=K, R=R, seg_cols=D, nseg=3)
    wq, wk = (1 + 0.1 * rnd((2, 128), 306).float()).to(BF), (1 + 0.1 * rnd((2, 128), 307).float()).to(BF)
    tab, _, _ = rope_tables(M, 308)
    q = [dict(norm_q=wq[i], norm_k=wk[i], rope_cs=tab, q_range=(2 * D, 3 * D), k_range=(0, D)) if fused_norm else None for i in (0, 1)]
    # image rows adapt k and q only, text rows v only: the per-row-range masks are independent
    joint = ops.gemm_lora(xv, tv, pair[0], seg_mask=0b101 | (0b010 << 8), bias=bias[0], qkn=q[0], split_row=T,
                          second=dict(wb=pair[1], bias=bias[1], norm_q=wq[1], norm_k=wk[1]), **kw)
    q_img = dict(q[0], pos0=T) if fused_norm else None
    img = ops.gemm_lora(xv[:, T:], tv[:, T:], pair[0], seg_mask=0b101, bias=bias[0], qkn=q_img, **kw)
    txt = ops.gemm_lora(xv[:, :T], tv[:, :T], pair[1], seg_mask=0b010, bias=bias[1], qkn=q[1], **kw)
    assert torch.equal(joint[:, T:], img) and torch.equal(joint[:, :T], txt)
    plain = ops.gemm(xv[:, :T], pair[1][:, :K], bias[1], variant=3)
    if not fused_norm:
        assert torch.equal(txt[..., :D], plain[..., :D]) and torch.equal(txt[..., 2 * D:], plain[..., 2 * D:])   # un-adapted segments
        assert not torch.equal(txt[..., D:2 * D], plain[..., D:2 * D])


def test_operands_the_tail_kernel_cannot_take_are_refused(ops):
    M, N, K, R = 512, 768, 256, 128
    cs = make_case(ops, M, N, K, R, 1, seed=400)
    kw = dict(K=K, seg_cols=256, nseg=3, seg_mask=0b111, bias=cs["bias"])
    ops.gemm_lora(cs["x"], cs["t"], cs["wb"], R=R, **kw)
    with pytest.raises(RuntimeError, match="padded rank"):
        ops.gemm_lora(cs["x"], cs["t"], cs["wb"][:, :K + 64], R=64, **kw)
    with pytest.raises(RuntimeError, match="seg_cols"):
        ops.gemm_lora(cs["x"], cs["t"], cs["wb"], R=R, **dict(kw, seg_cols=128))
    with pytest.raises(RuntimeError, match="seg_mask"):
        ops.gemm_lora(cs["x"], cs["t"], cs["wb"], R=R, **dict(kw, seg_mask=0b1111))
    below = torch.zeros(2, 1, M, 3 * R, dtype=BF, device="cuda")      # T BELOW x
    below[1, ..., :K].copy_(cs["x"])
    with pytest.raises(RuntimeError, match="above A"):
        ops.gemm_lora(below[1][..., :K], below[0], cs["wb"], R=R, **kw)
    x192 = torch.zeros(2, 1, M, 3 * R, dtype=BF, device="cuda")
    with pytest.raises(RuntimeError, match="persistent|K %"):
        ops.gemm_lora(x192[0][..., :192], x192[1], torch.zeros(N, 192 + R, dtype=BF, device="cuda"), R=R, **dict(kw, K=192))


@pytest.mark.parametrize("M,N,K,batch", [(1664, 384, 3072, 1), (4608, 128, 12288, 2), (80, 384, 256, 2), (300, 264, 192, 1)])
def test_column_scale_epilogue_is_the_down_projection(ops, M, N, K, batch):
    """tfx_gemm_bf16 epilogue 4: t = bf16(c[n] * (x @ Acat^T)) with c an fp32 DEVICE vector read when the kernel runs -- every kernel form
    (generic, auto incl. K-sliced units, one-tile, persistent), and a rewritten c is seen by the next launch of the same arguments."""
    x, A = rnd((batch, M, K), 501), rnd((N, K), 502, 0.05)
    c = (0.25 + torch.rand(N, generator=torch.Generator().manual_seed(503))).cuda()
    ref = (c * (x.float() @ A.float().T)).to(BF)
    ws = torch.empty(64 << 20, dtype=torch.uint8, device="cuda")
    variants = [0, 1] + ([2] if K % 64 == 0 else []) + ([3] if K % 128 == 0 else [])
    for v in variants if K % 64 == 0 else [0]:
        close(ops.gemm(x, A, None, epilogue=ops.EPI_COLSCALE, cscale=c, variant=v, workspace=ws if v == 1 else None), ref)
    out = torch.empty(batch, M, N, dtype=BF, device="cuda")
    ops.gemm(x, A, None, out=out, epilogue=ops.EPI_COLSCALE, cscale=c)
    first = out.clone()
    c.mul_(0.5)                                                        # a power of two: every output halves exactly
    ops.gemm(x, A, None, out=out, epilogue=ops.EPI_COLSCALE, cscale=c)
    assert torch.equal(out.float(), first.float() * 0.5)
    with pytest.raises(RuntimeError, match="column-scale"):
        ops.gemm(x, A, rnd((N,), 504), epilogue=ops.EPI_COLSCALE, cscale=c)            # no bias with it


@pytest.mark.parametrize("D,M,batch,rank,fused_norm", [(3072, 4608, 2, 128, True), (3072, 1664, 1, 16, True), (256, 320, 2, 16, False),
                                                       (1024, 1664, 1, 192, True)])
def test_adapted_linear_on_the_library_matches_the_merged_weights(ops, D, M, batch, rank, fused_norm):
    """Both launches on the library -- the down projection (epilogue 4) straight into T, then the tail GEMM -- against the Linear with the
    update MERGED in fp32, y = x (W + c B A)^T + b, for a fused [k; v; q] weight whose three targets have their own A, B, alpha and the
    call scale s: the reference of the merged path.  Same bounds as the un-adapted GEMM (close()); with the fused q / k norm the
    reference is the un-normed adapted output + tfx_rmsnorm_rope (per-pair bound)."""
    N, K, s = 3 * D, D, 0.8
    R = (rank + 127) // 128 * 128
    x, W, bias = rnd((batch, M, K), 601), rnd((N, K), 602, 0.05), rnd((N,), 603)
    As, Bs = [rnd((rank, K), 610 + i, 0.05) for i in range(3)], [rnd((D, rank), 620 + i, 0.2) for i in range(3)]
    alphas = [rank, 2 * rank, rank // 2]
    wb = torch.zeros(N, K + R, dtype=BF, device="cuda")
    wb[:, :K] = W
    Acat = torch.zeros(3 * R, K, dtype=BF, device="cuda")
    c = torch.zeros(3 * R, dtype=torch.float32, device="cuda")
    merged = W.float().clone()
    for i in range(3):
        wb[i * D:(i + 1) * D, K:K + rank] = Bs[i]
        Acat[i * R:i * R + rank] = As[i]
        c[i * R:(i + 1) * R] = s * alphas[i] / rank
        merged[i * D:(i + 1) * D] += (s * alphas[i] / rank) * (Bs[i].float() @ As[i].float())
    ref = x.float() @ merged.T + bias.float()
    _, xv, tv = ops.lora_operands(x, 3 * R)
    ops.gemm(xv, Acat, None, out=tv, epilogue=ops.EPI_COLSCALE, cscale=c)
    got = ops.gemm_lora(xv, tv, wb, K=K, R=R, seg_cols=D, nseg=3, seg_mask=0b111, bias=bias)
    close(got, ref.to(BF))
    base = ops.gemm(xv, W, bias)
    far = (base.float() - ref).abs().mean().item()
    assert far > 20 * (got.float() - ref).abs().mean().item()          # the update is far outside the rounding noise it is judged in
    if fused_norm:
        wq, wk = (1 + 0.1 * rnd((128,), 631).float()).to(BF), (1 + 0.1 * rnd((128,), 632).float()).to(BF)
        tab, cos, sin = rope_tables(M, 633)
        fused = ops.gemm_lora(xv, tv, wb, K=K, R=R, seg_cols=D, nseg=3, seg_mask=0b111, bias=bias,
                              qkn=dict(norm_q=wq, norm_k=wk, rope_cs=tab, q_range=(2 * D, 3 * D), k_range=(0, D)))
        ops.rmsnorm_rope_(got, 2 * D, 0, D // 128, 0, wq, wk, wq, wk, cos, sin)
        qkn_check(got, fused, ((2 * D, 3 * D), (0, D)))


# ---------------------------------------------------------------------------------------------------- model / pipeline level
# Reference: oracle.flux_oracle.transformer_forward fed the state dict with W + s (alpha / r) bf16(B) bf16(A) merged in fp32 -- the
# reference of the merged path (tests/test_pipeline_gpu.py::test_lora_merge_matches_oracle_with_premerged_weights), whose conditions
# are taken over unchanged: e_m = MAE(engine(s), oracle(s)) < 2e-2 mean|ref|, MAE(oracle(s), oracle(s')) > 5 e_m and
# MAE(engine(s), oracle(s')) > 3 e_m for the neighbouring scales s'.
MERGE_TARGETS = ["transformer_blocks.0.attn.to_q", "transformer_blocks.0.attn.add_k_proj", "transformer_blocks.1.attn.to_out.0",
                 "transformer_blocks.1.ff.net.0.proj", "transformer_blocks.0.ff_context.net.2",
                 "single_transformer_blocks.0.attn.to_v", "single_transformer_blocks.1.attn.to_k"]
RUNTIME_TARGETS = MERGE_TARGETS + ["single_transformer_blocks.0.proj_mlp", "single_transformer_blocks.1.proj_out",
                                   "transformer_blocks.1.attn.to_k"]


def synthetic_lora(sd, targets, seed, r=16):
    """(file-format state dict, {target: fp32 update at scale 1}): rank r, A, B ~ 0.2 N(0, 1), alternating alpha."""
    gl = torch.Generator().manual_seed(seed)
    lora, delta = {}, {}
    for i, t in enumerate(targets):
        out_f, in_f = sd[t + ".weight"].shape
        A, Bm = torch.randn(r, in_f, generator=gl) * 0.2, torch.randn(out_f, r, generator=gl) * 0.2
        alpha = float(r) if i % 2 == 0 else 8.0
        lora[f"transformer.{t}.lora_A.weight"], lora[f"transformer.{t}.lora_B.weight"] = A, Bm
        if i % 2:
            lora[f"transformer.{t}.alpha"] = torch.tensor(alpha)
        delta[t] = (alpha / r) * (Bm.to(BF).float() @ A.to(BF).float())
    return lora, delta


def merged_sd(sd, *scaled_deltas):
    out = dict(sd)
    for s, delta in scaled_deltas:
        for t, d in delta.items():
            out[t + ".weight"] = out[t + ".weight"] + s * d
    return out


def g3_inputs():
    from oracle import pipeline_oracle as po
    g = torch.Generator().manual_seed(11)
    return dict(hidden_states=torch.randn(1, 64, 384, generator=g), encoder_hidden_states=torch.randn(1, 16, 64, generator=g),
                pooled_projections=torch.randn(1, 32, generator=g), timestep=torch.tensor([0.6]),
                guidance=torch.tensor([30.0]), img_ids=po.latent_image_ids(8, 8), txt_ids=torch.zeros(16, 3))


def tobf(d):
    return {k: (v.to(BF) if v.dtype == torch.float32 and k != "guidance" else v) for k, v in d.items()}


def oracle(sd_f32, inp):
    from oracle import flux_oracle as fo
    from tests.test_pipeline_gpu import G3_CFG
    return fo.transformer_forward(tobf(sd_f32), G3_CFG, **tobf(inp))


def engine(tr, inp, **kw):
    bf = lambda t: t.to(BF).cuda()
    return tr(hidden_states=bf(inp["hidden_states"]), encoder_hidden_states=bf(inp["encoder_hidden_states"]),
              pooled_projections=bf(inp["pooled_projections"]), timestep=bf(inp["timestep"]), guidance=inp["guidance"].cuda(),
              img_ids=inp["img_ids"], txt_ids=inp["txt_ids"], return_dict=False, **kw)[0]


def split_file_format(lora):
    from textflux_amd.pipeline import FluxFillPipeline
    return FluxFillPipeline.lora_state_dict(dict(lora), return_alphas=True)


def test_runtime_adapter_follows_the_call_scale_and_lands_on_the_merged_oracle():
    from oracle import flux_oracle as fo
    from textflux_amd.pipeline import FluxFillPipeline
    from tests.test_pipeline_gpu import G3_CFG, mae, make_pipe
    pipe = make_pipe("euler")
    sd = fo.seeded_state_dict(G3_CFG, 7)
    lora, delta = synthetic_lora(sd, RUNTIME_TARGETS, 3)
    lsd, alphas = split_file_format(lora)
    n = FluxFillPipeline.load_lora_into_transformer(lsd, alphas, pipe.transformer, adapter_name="a", runtime=True)
    assert n == len(RUNTIME_TARGETS) and pipe.get_active_adapters() == ["a"]
    base_w = {k: v.clone() for k, v in pipe.transformer.w.items()}
    inp = g3_inputs()
    refs = {s: oracle(merged_sd(sd, (s, delta)), inp) for s in (0.0, 0.5, 1.0)}
    for s, neighbours in ((0.5, (0.0, 1.0)), (1.0, (0.5,))):
        got = engine(pipe.transformer, inp, joint_attention_kwargs={"scale": s})
        e_m = mae(got, refs[s])
        print(f"runtime LoRA scale {s}: |got - merged oracle| {e_m:.2e}, mean|ref| {refs[s].float().abs().mean().item():.3f}")
        assert e_m < 2e-2 * refs[s].float().abs().mean().item()
        for s2 in neighbours:
            d_ref, d_got = mae(refs[s], refs[s2]), mae(got, refs[s2])
            print(f"   neighbour {s2}: |oracle - oracle'| {d_ref:.2e}  |got - oracle'| {d_got:.2e}")
            assert d_ref > 5 * e_m and d_got > 3 * e_m
    # the call scale does not stick (unscale_lora_layers), and the base weights were never touched
    assert pipe.transformer._lora_call_scale == 1.0
    assert torch.equal(engine(pipe.transformer, inp), engine(pipe.transformer, inp, joint_attention_kwargs={"scale": 1.0}))
    assert all(torch.equal(v, pipe.transformer.w[k]) for k, v in base_w.items())


def test_adapter_lifecycle_unload_fuse_and_two_adapters():
    from oracle import flux_oracle as fo
    from textflux_amd.pipeline import FluxFillPipeline
    from tests.test_pipeline_gpu import G3_CFG, mae, make_pipe
    sd = fo.seeded_state_dict(G3_CFG, 7)
    inp = g3_inputs()
    lora_a, delta_a = synthetic_lora(sd, RUNTIME_TARGETS, 3)
    lora_b, delta_b = synthetic_lora(sd, MERGE_TARGETS[:4] + ["single_transformer_blocks.1.proj_out"], 5, r=8)
    fresh = engine(make_pipe("euler").transformer, inp)
    # attach -> unload == never adapted
    pipe = make_pipe("euler")
    pipe.load_lora_weights(dict(lora_a), adapter_name="a", runtime=True)
    assert not torch.equal(engine(pipe.transformer, inp), fresh)
    pipe.unload_lora_weights()
    assert pipe.get_active_adapters() == [] and torch.equal(engine(pipe.transformer, inp), fresh)
    # fuse_lora == the merged path on the same file
    pipe.load_lora_weights(dict(lora_a), adapter_name="a", runtime=True)
    pipe.fuse_lora()
    assert pipe.get_active_adapters() == []
    merged_pipe = make_pipe("euler")
    merged_pipe.load_lora_weights(dict(lora_a))
    assert torch.equal(engine(pipe.transformer, inp), engine(merged_pipe.transformer, inp))
    # two adapters with weights of their own
    pipe = make_pipe("euler")
    pipe.load_lora_weights(dict(lora_a), adapter_name="a", runtime=True)
    pipe.load_lora_weights(dict(lora_b), adapter_name="b", runtime=True)
    pipe.set_adapters(["a", "b"], [0.7, 0.3])
    assert pipe.get_active_adapters() == ["a", "b"]
    got = engine(pipe.transformer, inp)
    ref = oracle(merged_sd(sd, (0.7, delta_a), (0.3, delta_b)), inp)
    e_m = mae(got, ref)
    print(f"two adapters: |got - merged oracle| {e_m:.2e}")
    assert e_m < 2e-2 * ref.float().abs().mean().item()
    for other in (oracle(merged_sd(sd, (0.3, delta_a), (0.7, delta_b)), inp), oracle(merged_sd(sd, (0.7, delta_a)), inp), oracle(sd, inp)):
        assert mae(ref, other) > 5 * e_m and mae(got, other) > 3 * e_m
    pipe.set_adapters("a")                                   # b inactive: as if it were not there
    solo = make_pipe("euler")
    solo.load_lora_weights(dict(lora_a), adapter_name="a", runtime=True)
    assert mae(engine(pipe.transformer, inp), engine(solo.transformer, inp)) < 0.25 * e_m
    pipe.delete_adapters("b")
    assert torch.equal(engine(pipe.transformer, inp), engine(solo.transformer, inp))
    with pytest.raises(ValueError, match="not attached"):
        pipe.set_adapters(["nope"])
    # no runtime adapter (merged LoRA): a call scale keeps raising
    kw = dict(prompt_embeds=torch.zeros(1, 16, 64, dtype=BF, device="cuda"), pooled_prompt_embeds=torch.zeros(1, 32, dtype=BF, device="cuda"),
              latents=torch.zeros(1, 64, 64, dtype=BF, device="cuda"), masked_image_latents=torch.zeros(1, 64, 320, dtype=BF, device="cuda"),
              height=128, width=128, num_inference_steps=2, output_type="latent")
    with pytest.raises(NotImplementedError, match="merged at load"):
        merged_pipe(joint_attention_kwargs={"scale": 0.5}, **kw)
    # fp8 linears and runtime adapters exclude each other, both ways
    with pytest.raises(RuntimeError, match="fp8"):
        pipe.transformer.enable_fp8(True)
    f8 = make_pipe("euler")
    f8.transformer.enable_fp8(True)
    with pytest.raises(RuntimeError, match="fp8"):
        f8.load_lora_weights(dict(lora_a), adapter_name="a", runtime=True)


def test_step_graph_sees_a_new_scale_without_recapture(golden):
    g = golden("g5_pipeline")
    from oracle import flux_oracle as fo
    from tests.test_pipeline_gpu import G3_CFG, make_pipe
    kw = dict(prompt_embeds=g["prompt_embeds"].to(BF).cuda(), pooled_prompt_embeds=g["pooled"].to(BF).cuda(),
              latents=g["latents"].to(BF).cuda(), masked_image_latents=g["masked_image_latents"].to(BF).cuda(),
              height=128, width=128, num_inference_steps=4, guidance_scale=30.0, output_type="latent")
    pipe = make_pipe("euler")
    lora, _ = synthetic_lora(fo.seeded_state_dict(G3_CFG, 7), RUNTIME_TARGETS, 3)
    pipe.load_lora_weights(dict(lora), adapter_name="a", runtime=True)
    eager = {s: pipe(joint_attention_kwargs={"scale": s}, **kw).images for s in (1.0, 0.5)}
    assert not torch.equal(eager[1.0], eager[0.5])
    pipe.enable_hip_graph(True)
    first = pipe(joint_attention_kwargs={"scale": 1.0}, **kw).images
    ses = pipe.transformer._session
    (key, handle), = ses.graphs.items()
    assert handle is not False and handle
    second = pipe(joint_attention_kwargs={"scale": 0.5}, **kw).images
    assert pipe.transformer._session is ses and ses.graphs[key] is handle and len(ses.graphs) == 1      # no re-capture
    assert torch.equal(first, eager[1.0]) and torch.equal(second, eager[0.5])


def test_run_inference_lora_runtime_flag_from_checkpoint_directory(tmp_path_factory):
    """run_inference_lora.load_flux_pipeline(lora_runtime=True) (what --lora_runtime selects) on the synthetic checkpoint directory:
    the image against the merged oracle, the bound of tests/test_e2e_gpu.py::test_lora_pipeline_from_checkpoint_directory."""
    import os
    import numpy as np
    import run_inference as ri
    import run_inference_lora as rl
    from tests.helpers import tiny_checkpoint as tc
    from tests.test_e2e_gpu import _oracle_image, _scene
    from textflux_amd import glyph
    root, lora_dir = str(tmp_path_factory.mktemp("flux_fill_dev")), str(tmp_path_factory.mktemp("textflux_lora"))
    sd, vsd = tc.write_pipeline_dir(root)
    merged = tc.write_lora(lora_dir, sd)
    rb = lambda d: {k: v.to(BF).float() for k, v in d.items()}
    env = dict(vsd=rb(vsd))
    saved = ri.BASE, ri.TRANSFORMER, ri.PIPE, rl.LORA
    try:
        ri.BASE, ri.TRANSFORMER, ri.PIPE, rl.LORA = root, os.path.join(root, "transformer"), None, lora_dir
        a = rl.build_parser().parse_args(["--image", "i", "--mask", "m", "--words", "w", "--lora_runtime"])
        pipe = rl.load_flux_pipeline(a.lora_runtime, a.lora_scale)
        assert pipe.get_active_adapters() == [rl.LORA_ADAPTER]
        D = pipe.transformer.inner_dim
        assert torch.equal(pipe.transformer.w["d0.qkv_img.w"][2 * D:3 * D].float().cpu(), rb(sd)["transformer_blocks.0.attn.to_q.weight"])
        scene, mask = _scene(1)
        combined, cmask, _ = glyph.compose(scene, mask, ["LoRA"])
        out = ri.run_inference(combined, cmask, "LoRA", num_steps=3, guidance_scale=30, seed=7, pipe=pipe)
        ref = _oracle_image(env, pipe, combined, cmask, ["LoRA"], 3, 7, rb(merged))
        ref0 = _oracle_image(env, pipe, combined, cmask, ["LoRA"], 3, 7, rb(sd))
        img = np.asarray(out).astype(np.float32) / 255.0
        e_m, e_0 = np.abs(img - ref).mean(), np.abs(img - ref0).mean()
        print(f"runtime LoRA pipeline image MAE vs merged oracle {e_m:.3e}, vs unmerged oracle {e_0:.3e}")
        assert e_m < 2e-2 and e_m < e_0
    finally:
        ri.BASE, ri.TRANSFORMER, ri.PIPE, rl.LORA = saved


TEXTFLUX_TARGETS = ["attn.to_k", "attn.to_q", "attn.to_v", "attn.to_out.0", "attn.add_k_proj", "attn.add_q_proj", "attn.add_v_proj",
                    "attn.to_add_out", "ff.net.0.proj", "ff.net.2", "ff_context.net.0.proj", "ff_context.net.2"]    # scripts/train_lora.py:511-524


@pytest.mark.parametrize("S,T,B,h2,w2", [(4096, 512, 2, 64, 64), (1152, 512, 1, 36, 32)], ids=["N4608_batch2", "C2_N1664_batch1"])
def test_full_width_block_pair_with_the_textflux_targets(S, T, B, h2, w2):
    """One double + one single block at the real width (D = 3072, 24 heads) with the twelve TextFlux target patterns adapted (rank 128,
    alpha = r, scale 0.8), driven through tfx_dit_forward's block range as tests/test_model_gpu.py::
    test_full_width_blocks_match_reference_goldens does, against fo.double_block / fo.single_block on the MERGED weights: rel MAE
    < 1e-2 per output (that test's bound), and the base weights are more than 3x further from the merged oracle than the adapted
    engine is.  T = 512 is a whole number of tiles: the double block runs its joint [text | image] launches (row-split weights with a
    tail per stream); batch 1 at N = 1664 is the geometry whose un-adapted launches are K-sliced."""
    from oracle import flux_oracle as fo
    from oracle import pipeline_oracle as po
    from tests.test_model_gpu import build, rel_mae
    heads, seed, r, s = 24, 5, 128, 0.8
    D = heads * 128
    cfg = fo.FluxConfig(num_layers=1, num_single_layers=1, num_attention_heads=heads, joint_attention_dim=64, pooled_projection_dim=32)
    sd = fo.seeded_state_dict(cfg, seed)
    gl = torch.Generator().manual_seed(seed + 10)
    lora, merged = {}, {k: v.to(BF).float() for k, v in sd.items()}
    for key in [k[:-len(".weight")] for k in sd if k.endswith(".weight")]:
        if not any(key.endswith("." + t) for t in TEXTFLUX_TARGETS) or not key.startswith(("transformer_blocks.", "single_transformer_blocks.")):
            continue
        out_f, in_f = sd[key + ".weight"].shape
        A, Bm = (torch.randn(r, in_f, generator=gl) * 0.05).to(BF), (torch.randn(out_f, r, generator=gl) * 0.05).to(BF)
        lora[f"transformer.{key}.lora_A.weight"], lora[f"transformer.{key}.lora_B.weight"] = A, Bm
        merged[key + ".weight"] = merged[key + ".weight"] + s * (Bm.float() @ A.float())
    assert len(lora) == 2 * (12 + 3)

    def rnd(shape, sd_):
        return torch.randn(shape, generator=torch.Generator().manual_seed(sd_))

    hidden, enc, temb = rnd((B, S, D), seed + 1).to(BF), rnd((B, T, D), seed + 2).to(BF), rnd((B, D), seed + 3).to(BF)
    ids_img, ids_txt = po.latent_image_ids(h2, w2), torch.zeros(T, 3)
    cos, sin = fo.flux_pos_embed(torch.cat((ids_txt, ids_img), 0))
    ref_enc, ref_hid, ref_sgl = [], [], []
    for b in range(B):                       # one sample at a time: the fp32 score matrices of 24 heads x 4608^2 are 2 GB each
        e, h = fo.double_block(merged, "transformer_blocks.0", heads, hidden[b:b + 1].float(), enc[b:b + 1].float(), temb[b:b + 1].float(), cos, sin)
        ref_enc.append(e)
        ref_hid.append(h)
        ref_sgl.append(fo.single_block(merged, "single_transformer_blocks.0", heads,
                                       torch.cat((enc[b:b + 1], hidden[b:b + 1]), 1).float(), temb[b:b + 1].float(), cos, sin))
    ref_enc, ref_hid, ref_sgl = torch.cat(ref_enc), torch.cat(ref_hid), torch.cat(ref_sgl)

    def run(m):
        ses = m.session(B, S, T)
        ses.set_conditioning(torch.zeros(B, T, 64, dtype=BF, device="cuda"), ids_txt, ids_img)
        mod = m.modulation(temb.cuda())
        ses.hid[:, :T].copy_(enc)
        ses.hid[:, T:].copy_(hidden)
        ses.run(mod, first_block=0, last_block=1, flags=3)
        dbl = ses.hid.clone()
        ses.hid[:, :T].copy_(enc)
        ses.hid[:, T:].copy_(hidden)
        ses.run(mod, first_block=1, last_block=2, flags=3)
        return dbl[:, :T], dbl[:, T:], ses.hid.clone()

    m = build(cfg, seed)
    base = [rel_mae(o, ref) for o, ref in zip(run(m), (ref_enc, ref_hid, ref_sgl))]
    m.attach_lora("textflux", lora)
    m.set_adapters(["textflux"], [s])
    got = [rel_mae(o, ref) for o, ref in zip(run(m), (ref_enc, ref_hid, ref_sgl))]
    print(f"full width, runtime adapters: rel MAE double enc {got[0]:.2e} hidden {got[1]:.2e} single {got[2]:.2e}; "
          f"base weights: {base[0]:.2e} {base[1]:.2e} {base[2]:.2e}")
    assert max(got) < 1e-2
    assert all(b > 3 * g for b, g in zip(base, got))
