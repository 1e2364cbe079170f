"""Mixed-geometry batches on the GPU: per-sample lengths in the attention kernel (tfx_attn_args.seq_len), per-sample rotary tables
(tfx_qkn_args.rope_bstride, tfx_rmsnorm_rope_batched), the padded forward (tfx_dit_desc.seq_len / rope_bstride) and
FluxFillPipeline.call_mixed.

The yardstick throughout is the sample ALONE: a sample of a mixed batch must compute what its own batch-1 launch at its own
length computes -- bit for bit where every kernel on the way is row-wise or per item (attention in whole-item form, GEMMs without
K slicing), and within the bounds the uniform engine is held to against the fp32 / bf16 oracle.  Padding rows are filled with NaN
(inputs) and a sentinel (outputs): nothing of theirs may reach a valid row, and nothing may be written to them by attention."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import flux_oracle as fo
from oracle import pipeline_oracle as po
from tests.helpers import tiny_checkpoint as tc

BF = torch.bfloat16
SENTINEL = 1234.0


@pytest.fixture(scope="module")
def ops():
    from textflux_amd import ops as o
    return o


def rnd(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def close(got, ref, max_rel=1e-2, mae_rel=2e-3):     # tests/test_kernels_gpu.py's criterion
    got, ref = got.float().cpu(), ref.float().cpu()
    assert got.shape == ref.shape
    assert torch.isfinite(got).all()
    err = (got - ref).abs()
    assert err.max().item() <= max_rel * ref.abs().max().item() + 1e-6, (err.max().item(), ref.abs().max().item())
    assert err.mean().item() <= mae_rel * ref.abs().mean().item() + 1e-7, (err.mean().item(), ref.abs().mean().item())


# ----------------------------------------------------------------------------- attention
ATTN_CASES = {"384_items_on_256_cus": (4, 24, 1024, [1024, 777, 257, 64]), "one_workgroup_per_item": (2, 2, 512, [512, 130])}
_attn_cache = {}


def attn_case(name):
    """q, k, v with NaN padding rows and the fp32 SDPA reference of every sample over its own rows: computed once, never modified."""
    if name not in _attn_cache:
        B, H, N, lens = ATTN_CASES[name]
        q, k, v = (rnd((B, N, H * 128), s).to(BF) for s in (20, 21, 22))
        refs = []
        for b, L in enumerate(lens):
            qh, kh, vh = (t[b:b + 1, :L].float().view(1, L, H, 128).transpose(1, 2).cuda() for t in (q, k, v))
            refs.append(torch.nn.functional.scaled_dot_product_attention(qh, kh, vh).transpose(1, 2).reshape(L, H * 128).cpu())
            for t in (q, k, v):
                t[b, L:] = float("nan")
        sl = torch.tensor(lens, dtype=torch.int32).cuda()
        _attn_cache[name] = (q.cuda(), k.cuda(), v.cuda(), sl, refs)
    return ATTN_CASES[name] + _attn_cache[name]


@pytest.mark.parametrize("bound", [0.0, 30.0])
@pytest.mark.parametrize("name", list(ATTN_CASES))
def test_attention_seq_len_equals_each_sample_alone(ops, name, bound):
    """Sample b of a launch with seq_len computes, bit for bit, what the uniform launch of the same kernel computes on its first
    L_b rows (same tiles in the same order, whole items); rows >= L_b of the output keep the sentinel; K / V / Q padding is NaN, so a
    single read of it would show.  With the guarded stream (bound 0) and the reference-free one (an admissible bound)."""
    B, H, N, lens, q, k, v, sl, refs = attn_case(name)
    ops.set_option("attention_streamk", 0)
    try:
        out = torch.full((B, N, H * 128), SENTINEL, dtype=BF, device="cuda")
        ops.attention_mode_counts(reset=True)
        ops.attention(q, k, v, out=out, score_bound=bound, seq_len=sl)
        c = ops.attention_mode_counts(reset=True)
        assert c["w4_reference_free" if bound else "w4_guarded"] == 1 and c["streamk_tail"] == 0, c
        for b, L in enumerate(lens):
            alone = ops.attention(q[b:b + 1, :L], k[b:b + 1, :L], v[b:b + 1, :L], score_bound=bound)
            assert torch.isfinite(alone.float()).all()
            assert torch.equal(out[b, :L], alone[0]), (b, L)
            close(out[b, :L], refs[b].to(BF), max_rel=2e-2, mae_rel=4e-3)
            assert (out[b, L:] == SENTINEL).all(), (b, L)
        again = torch.full_like(out, SENTINEL)
        ops.attention(q, k, v, out=again, score_bound=bound, seq_len=sl)
        assert torch.equal(again, out)
    finally:
        ops.set_option("attention_streamk", 1)


def test_attention_seq_len_takes_whole_items_and_clamps_bad_lengths(ops):
    """With the default attention_streamk and a workspace the launch still runs whole items (entry 8 of the mode counters stays 0)
    and gives the same bits; lengths outside [1, N] are clamped by the kernel (0 -> 1 row, N + 1000 -> N rows): nothing outside the
    operands is addressed and the result is that of the clamped length."""
    B, H, N, lens, q, k, v, sl, refs = attn_case("384_items_on_256_cus")
    ws = torch.empty(2 * 256 * 256 * 132, dtype=torch.float32, device="cuda")
    ops.set_option("attention_streamk", 0)
    want = torch.full((B, N, H * 128), SENTINEL, dtype=BF, device="cuda")
    ops.attention(q, k, v, out=want, score_bound=30.0, seq_len=sl)
    ops.set_option("attention_streamk", 1)
    ops.attention_mode_counts(reset=True)
    got = torch.full_like(want, SENTINEL)
    ops.attention(q, k, v, out=got, score_bound=30.0, workspace=ws, seq_len=sl)
    assert ops.attention_mode_counts(reset=True)["streamk_tail"] == 0
    assert torch.equal(got, want)
    # clamping: finite data everywhere (a clamped-up length reads the rows that were padding)
    q2, k2, v2 = (rnd((2, 300, 256), s).to(BF).cuda() for s in (31, 32, 33))
    bad = torch.tensor([0, 300 + 1000], dtype=torch.int32).cuda()
    out = torch.full((2, 300, 256), SENTINEL, dtype=BF, device="cuda")
    ops.attention(q2, k2, v2, out=out, seq_len=bad)
    assert torch.equal(out[0, :1], ops.attention(q2[:1, :1], k2[:1, :1], v2[:1, :1])[0]) and (out[0, 1:] == SENTINEL).all()
    assert torch.equal(out[1], ops.attention(q2[1:], k2[1:], v2[1:])[0])


def test_attention_seq_len_is_kernel_30_only(ops):
    B, H, N, lens, q, k, v, sl, refs = attn_case("one_workgroup_per_item")
    try:
        # 8 is a bench-only schedule: the product library refuses to SELECT it (tfx_set_option), so no launch can combine it with
        # seq_len; a library that does carry it (the bench build) must refuse the launch itself
        try:
            ops.set_option("attention_waves", 8)
            selected = True
        except RuntimeError as e:
            assert "bench-only" in str(e), e
            selected = False
        if selected:
            with pytest.raises(RuntimeError, match="kernel 30 only"):
                ops.attention(q, k, v, seq_len=sl)
        ops.set_option("attention_waves", 34)
        with pytest.raises(RuntimeError, match="kernel 30 only"):
            ops.attention(q, k, v, seq_len=sl)
    finally:
        ops.set_option("attention_waves", ops.DEFAULT_ATTENTION)


# ----------------------------------------------------------------------------- rotary tables per sample
def test_rope_tables_per_sample_equal_two_batch_1_calls(ops):
    """tfx_gemm_bf16_qkn with rope_bstride and tfx_rmsnorm_rope_batched at B = 2 with two different tables: bit-equal to two B = 1
    calls with the matching table.  Shape: the QKN-eligible one of tests/test_kernels_gpu.py's fused-epilogue test per sample."""
    D, M, K, pos0 = 3072, 2304 + 40, 512, 7
    N = 3 * D
    a, w, b = rnd((2, M, K), 81).to(BF).cuda(), rnd((N, K), 82, 0.05).to(BF).cuda(), rnd((N,), 83).to(BF).cuda()
    wq, wk = (1 + 0.1 * rnd((128,), 84)).to(BF).cuda(), (1 + 0.1 * rnd((128,), 85)).to(BF).cuda()
    ang = rnd((2, M + pos0, 64), 86) * 3.0
    cs = torch.stack([torch.cos(ang), torch.sin(ang)], -1).contiguous().cuda()                       # [2, rows, 64, 2] fp32
    fused = ops.gemm_qkn(a, w, b, wq, wk, cs, (2 * D, 3 * D), (0, D), pos0=pos0)
    for s in range(2):
        one = ops.gemm_qkn(a[s], w, b, wq, wk, cs[s].contiguous(), (2 * D, 3 * D), (0, D), pos0=pos0)
        assert torch.equal(fused[s], one), s
    assert not torch.equal(fused[0, :, :D], ops.gemm_qkn(a[0], w, b, wq, wk, cs[1].contiguous(), (2 * D, 3 * D), (0, D), pos0=pos0)[:, :D])
    # the separate pass, on a smaller buffer: text rows (T = 100) take the second weight pair
    H, Nt, T = 3, 333, 100
    buf = rnd((2, Nt, 7 * H * 128), 90).to(BF).cuda()
    ang2 = rnd((2, Nt, 64), 91) * 3.0
    cos, sin = (f(ang2).repeat_interleave(2, -1).contiguous().cuda() for f in (torch.cos, torch.sin))
    wq2, wk2 = (1 + 0.1 * rnd((128,), 92)).to(BF).cuda(), (1 + 0.1 * rnd((128,), 93)).to(BF).cuda()
    both = ops.rmsnorm_rope_(buf.clone(), 2 * H * 128, 0, H, T, wq, wk, wq2, wk2, cos, sin)
    for s in range(2):
        one = ops.rmsnorm_rope_(buf[s:s + 1].clone(), 2 * H * 128, 0, H, T, wq, wk, wq2, wk2, cos[s].contiguous(), sin[s].contiguous())
        assert torch.equal(both[s], one[0]), s
    assert not torch.equal(both[1], ops.rmsnorm_rope_(buf[1:].clone(), 2 * H * 128, 0, H, T, wq, wk, wq2, wk2, cos[0].contiguous(),
                                                      sin[0].contiguous())[0])


# ----------------------------------------------------------------------------- forward
T_TXT = 64
GRIDS = [(16, 16), (16, 24), (32, 16)]        # latent grids (h2, w2) of 256 x 256, 384 x 256 and 256 x 512 pixels: 256 / 384 / 512 tokens
SIZES = [(w2 * 16, h2 * 16) for h2, w2 in GRIDS]


def build_model():
    from textflux_amd.transformer import FluxTransformer2DModel
    c = tc.TR_CFG
    m = FluxTransformer2DModel(in_channels=c.in_channels, out_channels=c.out_channels, num_layers=c.num_layers,
                               num_single_layers=c.num_single_layers, num_attention_heads=c.num_attention_heads,
                               joint_attention_dim=c.joint_attention_dim, pooled_projection_dim=c.pooled_projection_dim, guidance_embeds=True)
    return m.load_state_dict(fo.seeded_state_dict(c, 7), device="cuda")


def forward_inputs():
    c = tc.TR_CFG
    xs = [rnd((1, h2 * w2, c.in_channels), 100 + i).to(BF).cuda() for i, (h2, w2) in enumerate(GRIDS)]
    pe = rnd((3, T_TXT, c.joint_attention_dim), 110).to(BF).cuda()
    pooled = rnd((3, c.pooled_projection_dim), 111).to(BF).cuda()
    t = torch.tensor([900.0, 500.0, 120.0]).cuda()
    g = torch.full((3,), 30000.0).cuda()
    ids = [po.latent_image_ids(h2, w2) for h2, w2 in GRIDS]
    return xs, pe, pooled, t, g, ids


def run_alone_and_mixed(m):
    """(outputs of every sample's own B = 1 session, outputs of the mixed session) for the same inputs; the mixed session's inputs and
    workspace are NaN wherever they are padding."""
    xs, pe, pooled, t, g, ids = forward_inputs()
    mod = m.modulation(m.temb(t, g, pooled))
    txt = torch.zeros(T_TXT, 3)
    alone = []
    for b, (h2, w2) in enumerate(GRIDS):
        ses = m.session(1, h2 * w2, T_TXT)
        ses.set_conditioning(pe[b:b + 1], txt, ids[b])
        ses.xin.copy_(xs[b])
        alone.append(ses.run(mod[b:b + 1]).clone()[0])
    S_b = [h2 * w2 for h2, w2 in GRIDS]
    N = (T_TXT + max(S_b) + 255) // 256 * 256
    ses = m.session(3, N - T_TXT, T_TXT, mixed=True)
    ses.set_conditioning(pe, txt, ids)
    assert ses.seq_len.tolist() == [T_TXT + s for s in S_b]
    for buf in (ses.xin, ses.hid, ses.xn, ses.y, ses.out):
        buf.fill_(float("nan"))
    for b in range(3):
        ses.xin[b, :S_b[b]].copy_(xs[b][0])
    out = ses.run(mod).clone()
    return alone, [out[b, :S_b[b]] for b in range(3)]


def test_mixed_forward_equals_each_sample_alone(ops):
    """Three geometries in one session (N = 768: three q-tiles per head, the short samples' last ones skipped) against every sample's
    own B = 1 session.  With gemm_splitk 0 and attention_streamk 0 every kernel is row-wise or per item: bit-equal."""
    m = build_model()
    ops.set_option("gemm_splitk", 0)
    ops.set_option("attention_streamk", 0)
    try:
        alone, mixed = run_alone_and_mixed(m)
        for b in range(3):
            assert torch.isfinite(mixed[b].float()).all(), b
            print(f"sample {b}: max |mixed - alone| = {(mixed[b].float() - alone[b].float()).abs().max().item():.3e}")
            assert torch.equal(mixed[b], alone[b]), b
        # the same session serves another mix of lengths: permuted geometries, nothing re-created
        ses = m._session
        xs, pe, pooled, t, g, ids = forward_inputs()
        perm = [2, 0, 1]
        ses.set_conditioning(pe[perm], torch.zeros(T_TXT, 3), [ids[p] for p in perm])
        assert m.session(3, ses.S, T_TXT, mixed=True) is ses
        ses.xin.fill_(float("nan"))
        for b, p in enumerate(perm):
            ses.xin[b, :xs[p].shape[1]].copy_(xs[p][0])
        mod = m.modulation(m.temb(t[perm], g, pooled[perm]))
        out = ses.run(mod)
        for b, p in enumerate(perm):
            assert torch.equal(out[b, :xs[p].shape[1]], alone[p]), (b, p)
    finally:
        ops.set_option("gemm_splitk", 2)      # the library's default (gemm.hip: g_gemm_splitk)
        ops.set_option("attention_streamk", 1)


def test_mixed_session_refreshes_tables_when_equal_length_samples_swap_places(ops):
    """Two samples of EQUAL token count but transposed grids (16 x 24 and 24 x 16 latent cells: 384 tokens each) in one reused mixed
    session, then the same two swapped: the lengths, and any checksum over the whole batch's ids, are the same both times, the
    per-sample rotary tables are not.  Each sample must be bit-equal to its own B = 1 session in both orders."""
    m = build_model()
    c = tc.TR_CFG
    grids = [(16, 24), (24, 16)]
    S1 = 384
    xs = [rnd((1, S1, c.in_channels), 200 + i).to(BF).cuda() for i in range(2)]
    pe = rnd((2, T_TXT, c.joint_attention_dim), 210).to(BF).cuda()
    pooled = rnd((2, c.pooled_projection_dim), 211).to(BF).cuda()
    t, g = torch.tensor([700.0, 300.0]).cuda(), torch.full((2,), 30000.0).cuda()
    ids = [po.latent_image_ids(h2, w2) for h2, w2 in grids]
    txt = torch.zeros(T_TXT, 3)
    ops.set_option("gemm_splitk", 0)
    ops.set_option("attention_streamk", 0)
    try:
        mod = m.modulation(m.temb(t, g, pooled))
        alone = []
        for b in range(2):
            ses1 = m.session(1, S1, T_TXT)
            ses1.set_conditioning(pe[b:b + 1], txt, ids[b])
            ses1.xin.copy_(xs[b])
            alone.append(ses1.run(mod[b:b + 1]).clone()[0])
        assert not torch.equal(alone[0], alone[1])
        N = (T_TXT + S1 + 255) // 256 * 256
        ses = m.session(2, N - T_TXT, T_TXT, mixed=True)
        for order in ([0, 1], [1, 0], [1, 0], [0, 1]):
            assert m.session(2, N - T_TXT, T_TXT, mixed=True) is ses
            ses.set_conditioning(pe[order], txt, [ids[i] for i in order])
            ses.xin.fill_(float("nan"))
            for k, i in enumerate(order):
                ses.xin[k, :S1].copy_(xs[i][0])
            out = ses.run(mod[order])
            for k, i in enumerate(order):
                assert torch.equal(out[k, :S1], alone[i]), (order, k)
    finally:
        ops.set_option("gemm_splitk", 2)      # the library's default (gemm.hip: g_gemm_splitk)
        ops.set_option("attention_streamk", 1)


def test_mixed_forward_with_fp8_linears(ops):
    """fp8 linears are row-wise too (per-token activation scales, per-channel weight scales): with whole-item attention and unsliced
    GEMMs every sample of the mixed forward is bit-equal to its own B = 1 fp8 run -- which is inside any tolerance an fp8 forward is
    held to (tests/test_model_gpu.py: 3e-2 relative MAE against the fp8 oracle)."""
    m = build_model().enable_fp8()
    ops.set_option("gemm_splitk", 0)
    ops.set_option("attention_streamk", 0)
    try:
        alone, mixed = run_alone_and_mixed(m)
        for b in range(3):
            assert torch.isfinite(mixed[b].float()).all(), b
            e = ((mixed[b].float() - alone[b].float()).abs().mean() / alone[b].float().abs().mean()).item()
            print(f"fp8 sample {b}: rel MAE mixed vs alone {e:.3e}, bit-equal {torch.equal(mixed[b], alone[b])}")
            assert e <= 3e-2, (b, e)
            assert torch.equal(mixed[b], alone[b]), b
    finally:
        ops.set_option("gemm_splitk", 2)      # the library's default (gemm.hip: g_gemm_splitk)
        ops.set_option("attention_streamk", 1)


# ----------------------------------------------------------------------------- pipeline
SCHED = dict(use_dynamic_shifting=True, base_shift=0.5, max_shift=1.15, base_image_seq_len=256, max_image_seq_len=4096, shift=3.0)


def make_pipe(sd):
    from textflux_amd.pipeline import FluxFillPipeline
    from textflux_amd.schedulers import FlowMatchEulerDiscreteScheduler
    from textflux_amd.transformer import FluxTransformer2DModel

    class _VaeCfg:   # output_type "latent" with injected masked_image_latents: only the VAE's config is consulted
        class config:
            block_out_channels = (128, 256, 512, 512)
            latent_channels = 16
            scaling_factor, shift_factor = 0.3611, 0.1159

    c = tc.TR_CFG
    tr = FluxTransformer2DModel(in_channels=c.in_channels, out_channels=c.out_channels, num_layers=c.num_layers,
                                num_single_layers=c.num_single_layers, num_attention_heads=c.num_attention_heads,
                                joint_attention_dim=c.joint_attention_dim, pooled_projection_dim=c.pooled_projection_dim,
                                guidance_embeds=True).load_state_dict(sd, device="cuda")
    pipe = FluxFillPipeline(scheduler=FlowMatchEulerDiscreteScheduler(**SCHED), vae=_VaeCfg(), text_encoder=None, tokenizer=None,
                            text_encoder_2=None, tokenizer_2=None, transformer=tr)
    pipe.set_progress_bar_config(disable=True)
    return pipe


class _Trajectory:
    """Stands in for the progress bar of an eager run: update() is called once per finished step and snapshots the latents, which
    live in columns [0, 64) of the session's x_embedder input under the fused Euler step."""
    def __init__(self, pipe):
        self.pipe, self.steps = pipe, []

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False

    def update(self, n=1):
        self.steps.append(self.pipe.transformer._session.xin[:, :, :64].clone())


def test_call_mixed_matches_each_samples_own_oracle_run_and_reuses_session_and_graph():
    """Four Euler steps over three geometries: eager == graph replay bit for bit; every step's latents of every sample against the
    bf16-faithful oracle run of that sample ALONE at its own geometry and its own sigma schedule, latent MAE <= 1e-3 per step (the
    bound tests/test_configs_gpu.py applies to the uniform engine); a second call with permuted geometries reuses the session and its
    captured graph."""
    c, n = tc.TR_CFG, 4
    sd = {k: v.to(BF) for k, v in fo.seeded_state_dict(c, 7).items()}
    pipe = make_pipe(sd)
    g = torch.Generator().manual_seed(5)
    S_b = [h2 * w2 for h2, w2 in GRIDS]
    lat = [torch.randn(1, s, 64, generator=g).to(BF) for s in S_b]
    mil = [torch.cat([torch.randn(1, s, 64, generator=g), (torch.randn(1, s, 256, generator=g) > 0).float()], -1).to(BF) for s in S_b]
    pe = (torch.randn(3, T_TXT, c.joint_attention_dim, generator=g) * 0.1).to(BF)
    pooled = torch.randn(3, c.pooled_projection_dim, generator=g).to(BF)

    def call(order):
        return pipe.call_mixed(sizes=[SIZES[i] for i in order], latents=[lat[i].cuda() for i in order],
                               masked_image_latents=[mil[i].cuda() for i in order], prompt_embeds=pe[order].cuda(),
                               pooled_prompt_embeds=pooled[order].cuda(), num_inference_steps=n, guidance_scale=30.0,
                               output_type="latent").images

    order = [0, 1, 2]
    traj = _Trajectory(pipe)
    pipe.progress_bar = lambda iterable=None, total=None: traj
    eager = call(order)
    del pipe.progress_bar
    assert len(traj.steps) == n and all(torch.equal(traj.steps[-1][b, :S_b[b]], eager[b]) for b in range(3))
    pipe.enable_hip_graph(True)
    graphed = call(order)
    ses = pipe.transformer._session
    assert ses.mixed and len(ses.graphs) == 1 and all(ses.graphs.values())
    handles = dict(ses.graphs)
    for b in range(3):
        assert eager[b].shape == (S_b[b], 64) and torch.isfinite(eager[b].float()).all()
        assert torch.equal(eager[b], graphed[b]), b
    for b, (h2, w2) in enumerate(GRIDS):
        _, ref = po.denoise(sd, c, lat[b], mil[b], pe[b:b + 1], pooled[b:b + 1], h2, w2, n, 30.0, max_steps=n)
        errs = [(traj.steps[i][b, :S_b[b]].float().cpu() - ref[i][0].float()).abs().mean().item() for i in range(n)]
        print(f"sample {b} ({SIZES[b][0]}x{SIZES[b][1]}): per-step latent MAE vs its own oracle run {['%.2e' % e for e in errs]}")
        assert max(errs) <= 1e-3, (b, errs)
    # permuted geometries, same (B, N): same session, same graph, nothing new captured -- and every sample's result unchanged
    perm = [2, 0, 1]
    again = call(perm)
    assert pipe.transformer._session is ses and dict(ses.graphs) == handles
    for k, i in enumerate(perm):
        assert torch.equal(again[k], eager[i]), (k, i)


def test_call_mixed_equals_the_python_issued_loop():
    """Two samples on the two smallest grids, two steps: call_mixed -- eagerly and as a replayed step graph, both through
    tfx_dit_step_run -- against the same launches issued from Python on a mixed session (helpers/plain_loop.py), bit for bit."""
    from tests.helpers.plain_loop import mixed_fused_loop
    c, n, grids = tc.TR_CFG, 2, GRIDS[:2]
    pipe = make_pipe({k: v.to(BF) for k, v in fo.seeded_state_dict(c, 7).items()})
    g = torch.Generator().manual_seed(6)
    S_b = [h2 * w2 for h2, w2 in grids]
    lat = [torch.randn(1, s, 64, generator=g).to(BF).cuda() for s in S_b]
    mil = [torch.cat([torch.randn(1, s, 64, generator=g), (torch.randn(1, s, 256, generator=g) > 0).float()], -1).to(BF).cuda() for s in S_b]
    pe = (torch.randn(2, T_TXT, c.joint_attention_dim, generator=g) * 0.1).to(BF).cuda()
    pooled = torch.randn(2, c.pooled_projection_dim, generator=g).to(BF).cuda()
    kw = dict(sizes=SIZES[:2], latents=lat, masked_image_latents=mil, prompt_embeds=pe, pooled_prompt_embeds=pooled,
              num_inference_steps=n, guidance_scale=30.0, output_type="latent")
    eager = pipe.call_mixed(**kw).images
    ref = mixed_fused_loop(pipe, lat, mil, pe, pooled, grids, n)
    graphed = pipe.enable_hip_graph(True).call_mixed(**kw).images
    assert all(pipe.transformer._session.graphs.values()) and len(pipe.transformer._session.graphs) == 1
    for b in range(2):
        assert ref[b].shape == (S_b[b], 64) and torch.isfinite(ref[b].float()).all()
        assert torch.equal(eager[b], ref[b]) and torch.equal(graphed[b], ref[b]), b


def test_call_mixed_refuses_amo_and_callbacks():
    from textflux_amd.schedulers import StochasticRFOvershotDiscreteScheduler
    sd = {k: v.to(BF) for k, v in fo.seeded_state_dict(tc.TR_CFG, 7).items()}
    pipe = make_pipe(sd)
    kw = dict(sizes=SIZES[:2], latents=[torch.zeros(1, 256, 64), torch.zeros(1, 384, 64)],
              masked_image_latents=[torch.zeros(1, 256, 320), torch.zeros(1, 384, 320)], prompt_embeds=torch.zeros(2, T_TXT, 64),
              pooled_prompt_embeds=torch.zeros(2, 128), output_type="latent")
    with pytest.raises(NotImplementedError, match="callback"):
        pipe.call_mixed(callback_on_step_end=lambda *a: {}, **kw)
    pipe.scheduler = StochasticRFOvershotDiscreteScheduler(**SCHED)
    with pytest.raises(NotImplementedError, match="AMO"):
        pipe.call_mixed(**kw)
