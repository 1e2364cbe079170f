"""tfx_dit_forward against the same forward issued from Python one launch at a time (tests/helpers/plain_forward.py), in EVERY BIT
of EVERY ELEMENT: the row offsets, column offsets, modulation chunk indices, per-stream weight selection, rotary-table offsets and
pointer arithmetic of textflux_amd/csrc/dit_forward.cpp, the model's loader and the session's descriptor.

Why equality holds: under gemm_splitk 0 and attention_streamk 0 every kernel of the forward is row-wise or per item (what
tests/test_mixed_batch_gpu.py relies on), so an element's bits do not depend on how many rows, tiles or samples share its launch;
the chain's launches are kernels the exact suites cover one by one.  The fused q / k norm + RoPE epilogue differs from the separate
pass by one bf16 step on a sliver of elements by design (its own tests: test_kernels_gpu.py, test_model_gpu.py), so the bf16 and
LoRA sessions here are built with fuse_qk_norm_rope = False; the fp8 shapes have fewer tiles than the chip has CUs, where the engine
takes the separate pass by itself.  Text ids are NON-ZERO throughout: with zero ids the rotary rotation of the text rows is the
identity and two offsets of the forward are dead code (shown in test_zero_text_ids_hide_a_shifted_text_table)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import flux_oracle as fo
from oracle import pipeline_oracle as po
from tests.helpers import plain_forward as pf
from tests.helpers import tiny_checkpoint as tc

BF = torch.bfloat16
CFG = tc.TR_CFG
NBLK = CFG.num_layers + CFG.num_single_layers
SENTINEL = 1234.0
# B, S, T: the smallest shapes at which each branch and tail of dit_forward.cpp is live
CASES = [(1, 64, 16),       # the golden shape; text and image as two groups
         (2, 1, 1),         # one-row LayerNorm / GEMM / attention ranges, N = 2
         (3, 333, 100),     # nothing a multiple of 64; T no tile multiple: the apart form; per-sample modulation stride
         (2, 200, 57),      # N = 257: one query row in a second 256-row attention item
         (2, 64, 0),        # T = 0: one group, no context copy, no text launches
         (2, 256, 256),     # T % 256 == 0: the joint row-split launches and ln_modulate_split
         (1, 300, 512)]     # joint, two text tiles, ragged image rows
JOINT = {(2, 256, 256), (1, 300, 512)}
FP8_CASES = [(2, 256, 256), (3, 333, 100), (2, 64, 0)]
LORA_CASES = [(2, 256, 256), (2, 200, 57)]
FAULT_CASES = [(3, 333, 100), (2, 256, 256)]
cid = lambda c: "B%d_S%d_T%d" % c


@pytest.fixture(scope="module")
def ops():
    from textflux_amd import ops as o
    return o


@pytest.fixture(autouse=True)
def rowwise(ops):
    """Every test of this module: no K-sliced GEMM units, whole-item attention; the library's defaults afterwards."""
    ops.set_option("gemm_splitk", 0)
    ops.set_option("attention_streamk", 0)
    try:
        yield
    finally:
        ops.set_option("gemm_splitk", 2)
        ops.set_option("attention_streamk", 1)


def rnd(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


# ----------------------------------------------------------------------------- models, inputs, the chain's results: built once
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def tiny_sd():
    return cached("sd", lambda: fo.seeded_state_dict(CFG, 7))


def tiny_lora():
    """The adapter of tiny_checkpoint.LORA_TARGETS in the file format: rank 8, alternating alpha."""
    def make():
        g, sd, lora = torch.Generator().manual_seed(3), tiny_sd(), {}
        for i, t in enumerate(tc.LORA_TARGETS):
            o, k = sd[t + ".weight"].shape
            lora[f"transformer.{t}.lora_A.weight"] = (torch.randn(8, k, generator=g) * 0.2).to(BF)
            lora[f"transformer.{t}.lora_B.weight"] = (torch.randn(o, 8, generator=g) * 0.2).to(BF)
            if i % 2:
                lora[f"transformer.{t}.alpha"] = torch.tensor(4.0)
        return lora
    return cached("lora", make)


def build(cfg, sd, fuse=True):
    from textflux_amd.transformer import FluxTransformer2DModel
    m = FluxTransformer2DModel(in_channels=cfg.in_channels, out_channels=cfg.out_channels, num_layers=cfg.num_layers,
                               num_single_layers=cfg.num_single_layers, num_attention_heads=cfg.num_attention_heads,
                               joint_attention_dim=cfg.joint_attention_dim, pooled_projection_dim=cfg.pooled_projection_dim, guidance_embeds=True)
    m.fuse_qk_norm_rope = fuse
    return m.load_state_dict(sd, device="cuda")


def model(kind):
    def make():
        if kind == "fp8":
            return build(CFG, tiny_sd()).enable_fp8()
        if kind == "fused":
            return build(CFG, tiny_sd())
        m = build(CFG, tiny_sd(), fuse=False)
        if kind == "lora":
            from textflux_amd.pipeline import FluxFillPipeline
            lsd, alphas = FluxFillPipeline.lora_state_dict(dict(tiny_lora()), return_alphas=True)
            m.attach_lora("a", lsd, alphas)
        return m
    return cached(("model", kind), make)


def image_ids(S):
    h = max(d for d in range(1, int(S ** 0.5) + 1) if S % d == 0)
    if h > 1 or S == 1:
        return po.latent_image_ids(h, S // h)
    ids = torch.zeros(S, 3)         # no rectangle: an arange grid 7 wide
    ids[:, 1], ids[:, 2] = torch.arange(S) // 7, torch.arange(S) % 7
    return ids


def text_ids(T, zero=False):
    ids = torch.zeros(T, 3)
    if not zero:
        ids[:, 1], ids[:, 2] = torch.arange(T), 3 * torch.arange(T) + 1
    return ids


def inputs(cfg, B, S, T):
    """Every sample with its own timestep and pooled vector: the modulation rows differ per sample."""
    def make():
        return dict(x=rnd((B, S, cfg.in_channels), 100 + S).to(BF).cuda(), pe=rnd((B, T, cfg.joint_attention_dim), 200 + T).to(BF).cuda(),
                    pooled=rnd((B, cfg.pooled_projection_dim), 300 + B).to(BF).cuda(), t=torch.tensor([900.0, 500.0, 120.0])[:B].cuda(),
                    g=torch.full((B,), 30000.0).cuda(), img_ids=image_ids(S))
    return cached(("in", cfg.inner_dim, B, S, T), make)


def setup(kind, case, zero_txt=False):
    """(model, its session conditioned for the case, inputs, modulation rows [B, mod_len])"""
    m, inp = model(kind), inputs(CFG, *case)
    ses = m.session(*case)
    ses.set_conditioning(inp["pe"], text_ids(case[2], zero_txt), inp["img_ids"])
    mod = cached(("mod", kind, case), lambda: m.modulation(m.temb(inp["t"], inp["g"], inp["pooled"])))
    assert mod.shape == (case[0], pf.mod_len(CFG))
    return m, ses, inp, mod


def chain(kind, case, mod, fault=None, zero_txt=False, scale=1.0, **kw):
    """plain_forward on the HIP backend for the case, in buffers of its own"""
    m, inp = model(kind), inputs(CFG, *case)
    W = cached("W", lambda: pf.pack_weights(tiny_sd(), CFG))
    lora = pf.pack_lora(W, tiny_lora(), call_scale=scale) if kind == "lora" else None
    be = pf.HipBackend(W, CFG, *case, fp8=kind == "fp8", lora=lora)
    cos, sin = pf.rope_rows(text_ids(case[2], zero_txt), inp["img_ids"], CFG, fault)
    if "hid0" not in kw:
        kw.update(xin=inp["x"], prompt_embeds=inp["pe"])
    return dict(pf.plain_forward(be, mod, cos, sin, m.attn_score_bounds(), fault=fault, **kw), be=be)


def reference(kind, case, mod, scale=1.0):
    return cached(("ref", kind, case, scale), lambda: chain(kind, case, mod, scale=scale))


def poison(ses, hid=True):
    """run_alone_and_mixed's device: a read of anything the forward did not write first shows in the output"""
    for buf in (ses.xn, ses.y, ses.out) + ((ses.hid,) if hid else ()):
        buf.fill_(float("nan"))


def engine(ses, mod, x, **kw):
    poison(ses)
    ses.xin.copy_(x)
    return ses.run(mod, **kw).clone()


def engine_block(ses, mod, hid0, k):
    poison(ses, hid=False)
    ses.hid.copy_(hid0)
    ses.run(mod, first_block=k, last_block=k + 1, flags=3)
    return ses.hid.clone()


def same(got, ref, what):
    assert got.shape == ref.shape and torch.isfinite(ref.float()).all(), what
    if not torch.equal(got, ref):
        bad = (got != ref) | torch.isnan(got)
        rows = bad.flatten(2).any(-1).nonzero()
        d = (got.float() - ref.float()).abs()
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.numel()} elements differ, max |diff| {d[~torch.isnan(d)].max().item() if (~torch.isnan(d)).any() else float('nan'):.3e}, "
                             f"first (sample, row)s {rows[:6].tolist()}, columns {bad.nonzero()[:6, 2].tolist()}")


def gemm_launches(ops, fn):
    """(result of fn(), bf16 GEMM launches, fp8 GEMM launches) counted by the library's launch profiler"""
    ops.prof_enable(True)
    try:
        ops.prof_collect(0), ops.prof_collect(2)
        r = fn()
        return r, ops.prof_collect(0)[2], ops.prof_collect(2)[2]
    finally:
        ops.prof_enable(False)


def block_linears(case, joint):
    """Linear launches of the block stack: a double block is 4 joint, 8 apart (4 without a text stream), a single block 2"""
    return CFG.num_layers * (4 if joint or case[2] == 0 else 8) + CFG.num_single_layers * 2


# ----------------------------------------------------------------------------- bf16
@pytest.mark.parametrize("case", CASES, ids=cid)
def test_whole_forward_equals_the_chain_under_every_knob(ops, case):
    """ses.run(mod) == the chain's out under (ln_joint, gemm_group_streams) = (1, 1), (0, 1), (1, 0); the form that ran is OBSERVED
    through the launch profiler's GEMM count (x_embedder + the block Linears + proj_out): the two T % 256 == 0 cases take the joint
    form under the default knobs, every other case and gemm_group_streams 0 the apart form.  xin, ctx0 and mod keep their bits."""
    m, ses, inp, mod = setup("bf16", case)
    ref = reference("bf16", case, mod)
    ctx0, mod0 = ses.ctx0.clone(), mod.clone()
    try:
        for ln_joint, group in ((1, 1), (0, 1), (1, 0)):
            ops.set_option("ln_joint", ln_joint)
            ops.set_option("gemm_group_streams", group)
            out, n_bf16, n_fp8 = gemm_launches(ops, lambda: engine(ses, mod, inp["x"]))
            same(out, ref["out"], f"{case} ln_joint {ln_joint} gemm_group_streams {group}: out")
            assert (n_bf16, n_fp8) == (2 + block_linears(case, bool(group) and case in JOINT), 0), (case, ln_joint, group, n_bf16, n_fp8)
            assert torch.equal(ses.xin, inp["x"]) and torch.equal(ses.ctx0, ctx0) and torch.equal(mod, mod0)
    finally:
        ops.set_option("ln_joint", 1)
        ops.set_option("gemm_group_streams", 1)


@pytest.mark.parametrize("case", CASES, ids=cid)
def test_each_block_equals_the_chain(ops, case):
    """Block k alone on the CHAIN's hid before block k: a fault is named by its block, and cannot hide behind or be blamed on an
    earlier one."""
    m, ses, inp, mod = setup("bf16", case)
    ref = reference("bf16", case, mod)
    assert len(ref["hid"]) == NBLK + 1
    for k in range(NBLK):
        same(engine_block(ses, mod, ref["hid"][k], k), ref["hid"][k + 1], f"{case} block {k}: hid")
        assert torch.isnan(ses.out.float()).all()         # flags bit 1: the tail did not run


@pytest.mark.parametrize("case", CASES, ids=cid)
def test_flags_and_block_range(ops, case):
    m, ses, inp, mod = setup("bf16", case)
    ref = reference("bf16", case, mod)
    # flags = 1: hid preloaded, embedders skipped (xin is NaN: a read of it would show), blocks + tail run
    poison(ses, hid=False)
    ses.xin.fill_(float("nan"))
    ses.hid.copy_(ref["hid"][0])
    same(ses.run(mod, flags=1), ref["out"], f"{case} flags 1: out")
    # flags = 2: embedders + blocks run, out left untouched
    poison(ses)
    ses.xin.copy_(inp["x"])
    ses.out.fill_(SENTINEL)
    ses.run(mod, flags=2)
    assert (ses.out == SENTINEL).all()
    same(ses.hid, ref["hid"][-1], f"{case} flags 2: hid")
    # the embedders alone: an empty block range
    poison(ses)
    ses.run(mod, first_block=0, last_block=0, flags=2)
    same(ses.hid, ref["hid"][0], f"{case} embedders: hid")
    # first_block < 0 and last_block beyond the count clamp to the whole stack
    same(engine(ses, mod, inp["x"], first_block=-3, last_block=NBLK + 95), ref["out"], f"{case} clamped range: out")


def test_euler_gate_equals_the_scheduler_kernel_on_the_chains_output(ops):
    """euler=True: xin[:, :, :out_channels] == tfx_euler_step on the chain's stored model output, every sample with its own dsigma; the
    other columns of xin untouched; out keeps its sentinel."""
    from textflux_amd.transformer import EULER_PAD
    case = (2, 200, 57)
    m, ses, inp, mod = setup("bf16", case)
    ref = reference("bf16", case, mod)
    C, ds = CFG.out_channels, torch.tensor([-0.0371, -0.0123])
    modx = torch.empty(case[0], m.mod_len + EULER_PAD, dtype=BF, device="cuda")
    modx[:, :m.mod_len] = mod
    modx[:, m.mod_len:] = ds.to(BF).cuda()[:, None]
    same(pf.plain_forward(pf.HipBackend(pf.pack_weights(tiny_sd(), CFG), CFG, *case), modx, *pf.rope_rows(text_ids(case[2]), inp["img_ids"], CFG),
                          m.attn_score_bounds(), xin=inp["x"], prompt_embeds=inp["pe"])["out"], ref["out"], "chain on the wider mod rows")
    want = pf.euler_on_output(ops, ref["out"], inp["x"], ds)
    assert not torch.equal(want, inp["x"][:, :, :C])
    poison(ses)
    ses.xin.copy_(inp["x"])
    ses.out.fill_(SENTINEL)
    ses.run(modx, euler=True)
    same(ses.xin[:, :, :C], want, "euler: latent columns of xin")
    assert torch.equal(ses.xin[:, :, C:], inp["x"][:, :, C:]) and (ses.out == SENTINEL).all()


@pytest.mark.parametrize("case", FAULT_CASES, ids=cid)
def test_fused_qk_epilogue_rotates_every_row_with_its_own_table_row(ops, case):
    """The one offset of the forward the bit-for-bit tests cannot reach: qkn_pos0, the rotary row of a projection's first output row when
    q / k norm + RoPE ride in the GEMM's epilogue (fuse_qk_norm_rope, the default).  The epilogue differs from the separate pass by
    design, so this comparison is the one tests/test_model_gpu.py holds the two forms to: the normalised, rotated k columns of the
    first double block -- text rows with non-zero ids, image rows from table row T -- agree with the chain's to one bf16 step of their
    rotation pair, on all but 2 % of the elements; more than none differ, which shows the epilogue ran (MI355X: 2 of 332 544 and 3 of
    262 144 elements, 0.28 of a step at most; the launches are deterministic, so are the counts).  A table row off by one moves
    a text row by a rotation of 1 and 3 id steps: most of its elements, by far more than a step."""
    D = CFG.inner_dim
    m, ses, inp, mod = setup("fused", case)
    assert ses.desc.rope_cs
    r = chain("fused", case, mod, hid0=reference("bf16", case, setup("bf16", case)[3])["hid"][0], blocks=[0], tail=False)
    engine_block(ses, mod, r["hid"][0], 0)
    a, b = r["be"].y[:, :, :D].float(), ses.y[:, :, :D].float()
    assert torch.isfinite(a).all() and torch.isfinite(b).all()
    diff = (a - b).abs()
    pair = (a.view(*a.shape[:-1], -1, 2) ** 2).sum(-1).sqrt().repeat_interleave(2, dim=-1)
    frac = (diff > 0).float().mean().item()
    print(f"{case}: fused epilogue vs the chain's separate pass: {frac:.2e} of the k elements differ, worst {(diff / (2 ** -6 * pair + 1e-6)).max().item():.2f} steps")
    assert (diff <= 2 ** -6 * pair + 1e-6).all()
    assert 0 < frac < 2e-2
    # ... and the same comparison does see a text table shifted by one
    T = case[2]
    hid0 = r["hid"][0]
    bad = chain("fused", case, mod, fault="txt_rope_shift_one", hid0=hid0, blocks=[0], tail=False)["be"].y[:, :T, :D].float()
    off = ((bad - b[:, :T]).abs() > 2 ** -6 * pair[:, :T] + 1e-6).float().mean().item()
    print(f"{case}: with the text table shifted by one {off:.2f} of the text rows' k elements are more than a step away")
    # one id step on axis 1 and three on axis 2 turn a pair of frequency f by f and 3 f: more than a step (2^-6 of the pair) for the 13 and
    # 16 fastest of each axis's 28 pairs, 58 of a head's 128 elements; a quarter leaves room for elements near zero
    assert off > 0.25


# ----------------------------------------------------------------------------- fp8 linears
@pytest.mark.parametrize("fuse", (1, 0))
@pytest.mark.parametrize("case", FP8_CASES, ids=cid)
def test_fp8_forward_and_blocks_equal_the_fp8_chain(ops, case, fuse):
    """enable_fp8(): ln_modulate_fp8 / quantize_rows_fp8 + gemm_fp8 per Linear with w8 and K % 256 == 0 -- at D = 256 every block Linear
    (counted: no bf16 GEMM but x_embedder and proj_out), always the apart form."""
    m, ses, inp, mod = setup("fp8", case)
    assert ses.fp8 and len(m.w8) == CFG.num_layers * 8 + CFG.num_single_layers * 2
    ref = reference("fp8", case, mod)
    ops.set_option("fp8_fuse_qkn", fuse)
    try:
        out, n_bf16, n_fp8 = gemm_launches(ops, lambda: engine(ses, mod, inp["x"]))
        same(out, ref["out"], f"fp8 {case} fp8_fuse_qkn {fuse}: out")
        assert (n_bf16, n_fp8) == (2, block_linears(case, False)), (n_bf16, n_fp8)
        for k in range(NBLK):
            same(engine_block(ses, mod, ref["hid"][k], k), ref["hid"][k + 1], f"fp8 {case} fp8_fuse_qkn {fuse} block {k}: hid")
    finally:
        ops.set_option("fp8_fuse_qkn", 1)
    assert not torch.equal(ref["out"], reference("bf16", case, setup("bf16", case)[3])["out"])


# ----------------------------------------------------------------------------- runtime LoRA
@pytest.mark.parametrize("scale", (1.0, 0.5))
@pytest.mark.parametrize("case", LORA_CASES, ids=cid)
def test_runtime_lora_forward_and_blocks_equal_the_lora_chain(ops, case, scale):
    """The adapter of LORA_TARGETS (an image-stream q, a text-stream k, an image ff1, a text ff2, two single-block segments) at two
    call scales.  At D = 256 the q | k | v projections' T blocks do not fit a row of xn: the per-segment matrices (`planes`) of
    Gemm::run_lora; (2, 256, 256) takes the joint launches with lora_mask | mask2 << 8, (2, 200, 57) the apart form -- counted: the
    block Linears plus one column-scaled down projection per adapted segment (6)."""
    m, ses, inp, mod = setup("lora", case)
    assert m.get_active_adapters() == ["a"]
    try:
        m._write_scales(scale)
        ref = reference("lora", case, mod, scale)
        out, n_bf16, _ = gemm_launches(ops, lambda: engine(ses, mod, inp["x"]))
        same(out, ref["out"], f"lora {case} scale {scale}: out")
        assert n_bf16 == 2 + block_linears(case, case in JOINT) + 6, n_bf16
        for k in range(NBLK):
            same(engine_block(ses, mod, ref["hid"][k], k), ref["hid"][k + 1], f"lora {case} scale {scale} block {k}: hid")
    finally:
        m._write_scales(1.0)
    base = reference("bf16", case, setup("bf16", case)[3])
    assert not torch.equal(ref["out"], base["out"])
    if scale != 1.0:
        assert not torch.equal(ref["out"], reference("lora", case, mod, 1.0)["out"])


# ----------------------------------------------------------------------------- full width
def test_full_width_block_pair_equals_the_chain(ops, golden):
    """D = 3072, 24 heads, 1 + 1 blocks (the weights of test_full_width_blocks_match_reference_goldens), B = 2, S = 1152, T = 512: the
    joint row-split launches, K = 12288 and 15360 and the 2-q-tile attention at the production tile geometry."""
    heads, _, _, seed, _, _ = [int(v) for v in golden("g2_blocks")["d3072.meta"]]
    cfg = fo.FluxConfig(num_layers=1, num_single_layers=1, num_attention_heads=heads, joint_attention_dim=64, pooled_projection_dim=32)
    sd = fo.seeded_state_dict(cfg, seed)
    case = B, S, T = 2, 1152, 512
    m = build(cfg, sd, fuse=False)
    inp = inputs(cfg, *case)
    ses = m.session(*case)
    ses.set_conditioning(inp["pe"], text_ids(T), inp["img_ids"])
    assert not ses.desc.rope_cs
    mod = m.modulation(m.temb(inp["t"], inp["g"], inp["pooled"]))
    W = pf.pack_weights(sd, cfg)
    del sd
    be = pf.HipBackend(W, cfg, *case)
    ref = pf.plain_forward(be, mod, *pf.rope_rows(text_ids(T), inp["img_ids"], cfg), m.attn_score_bounds(), xin=inp["x"], prompt_embeds=inp["pe"])
    out, n_bf16, _ = gemm_launches(ops, lambda: engine(ses, mod, inp["x"]))
    same(out, ref["out"], "full width: out")
    assert n_bf16 == 2 + 4 + 2, n_bf16            # the joint form
    for k in range(2):
        same(engine_block(ses, mod, ref["hid"][k], k), ref["hid"][k + 1], f"full width block {k}: hid")


# ----------------------------------------------------------------------------- the tests can fail
def engine_results(case, zero_txt=False):
    def make():
        m, ses, inp, mod = setup("bf16", case, zero_txt)
        ref = chain("bf16", case, mod, zero_txt=zero_txt)
        out = engine(ses, mod, inp["x"])
        blocks = [engine_block(ses, mod, ref["hid"][k], k) for k in range(NBLK)]
        return dict(mod=mod, ref=ref, out=out, blocks=blocks)
    return cached(("engine", case, zero_txt), make)


@pytest.mark.parametrize("fault", sorted(pf.FAULTS))
@pytest.mark.parametrize("case", FAULT_CASES, ids=cid)
def test_every_named_fault_in_the_chain_is_seen(ops, case, fault):
    """The chain with one deliberate mistake of its own differs from the engine: in the whole forward, and in every block the mistake
    touches when that block runs alone from the unfaulted input."""
    e = engine_results(case)
    same(e["out"], e["ref"]["out"], "the unfaulted chain")
    bad = chain("bf16", case, e["mod"], fault=fault)
    assert torch.isfinite(bad["out"].float()).all() and not torch.equal(bad["out"], e["out"]), fault
    L = CFG.num_layers
    touched = dict(double=range(L), single=range(L, NBLK), both=range(NBLK), tail=())[pf.FAULTS[fault]]
    for k in touched:
        got = chain("bf16", case, e["mod"], fault=fault, hid0=e["ref"]["hid"][k], blocks=[k], tail=False)["hid"][-1]
        assert torch.isfinite(got.float()).all() and not torch.equal(got, e["blocks"][k]), (fault, k)


def test_zero_text_ids_hide_a_shifted_text_table(ops):
    """Why the text ids of this module are non-zero: with zero ids the text rows' rotary rows (and the first image row's, id (0, 0, 0))
    are the identity, and text rows rotated with the table one row further down give the engine's bits all the same."""
    case = (3, 333, 100)
    e = engine_results(case, zero_txt=True)
    same(e["out"], e["ref"]["out"], "zero text ids: the unfaulted chain")
    assert torch.equal(chain("bf16", case, e["mod"], fault="txt_rope_shift_one", zero_txt=True)["out"], e["out"])
    setup("bf16", case)       # the session back on this module's ids


# ----------------------------------------------------------------------------- anchor: the chain is not wrong the engine's way
def test_chain_matches_the_reference_goldens(golden):
    """The chain's out on the g3_model inputs, held to test_forward_matches_reference_goldens' criterion: relative MAE against out_f32
    <= 1.25 x, against out_bf16 <= 1.5 x the reference's own bf16-vs-fp32 distance."""
    from tests.test_model_gpu import G3_CFG, rel_mae
    g = golden("g3_model")
    inp = {k[3:]: v for k, v in g.items() if k.startswith("in.")}
    sd = fo.seeded_state_dict(G3_CFG, 7)
    m = build(G3_CFG, sd, fuse=False)
    x, pe = inp["hidden_states"].to(BF).cuda(), inp["encoder_hidden_states"].to(BF).cuda()
    B, S, T = x.shape[0], x.shape[1], pe.shape[1]
    t = (inp["timestep"].to(BF).cuda() * 1000).float().expand(B)          # transformer_flux.py:1088-1090
    gd = (inp["guidance"].cuda().to(BF) * 1000).float().expand(B)
    mod = m.modulation(m.temb(t, gd, inp["pooled_projections"].to(BF).cuda()))
    be = pf.HipBackend(pf.pack_weights(sd, G3_CFG), G3_CFG, B, S, T)
    out = pf.plain_forward(be, mod, *pf.rope_rows(inp["txt_ids"], inp["img_ids"], G3_CFG), m.attn_score_bounds(), xin=x, prompt_embeds=pe)["out"]
    assert out.shape == g["out_bf16"].shape and torch.isfinite(out.float()).all()
    ref_gap = rel_mae(g["out_bf16"], g["out_f32"])
    e_bf, e_f32 = rel_mae(out, g["out_bf16"]), rel_mae(out, g["out_f32"])
    print(f"chain rel MAE vs ref-bf16 {e_bf:.2e}, vs ref-f32 {e_f32:.2e}, ref-bf16 vs ref-f32 {ref_gap:.2e}")
    assert ref_gap < 2e-2
    assert e_f32 <= 1.25 * ref_gap and e_bf <= 1.5 * ref_gap
