"""The model walk of tests/helpers/model_walk.py, proven on the CPU: the emulated engine (every kernel in fp64, rounded at the documented
points) under the unchanged model code passes every node of every configuration tests/test_model_walk_gpu.py runs, and every named fault,
injected one at a time, is rejected AT THE NODE where it was injected.  Plus two host-only checks of the load-time code: the T5
relative-position table and the VAE's packed filters."""
import pytest
import torch

from oracle import text_oracle as to
from oracle import vae_oracle as vo
from tests.helpers import model_walk as mw

BF = torch.bfloat16


@pytest.fixture()
def emu():
    from textflux_amd import ops
    return lambda fault=None: mw.EmuOps(ops, fault)


def _vae_case(name):
    kw, xs, zs, chunk_bytes, plan = mw.VAE_CASES[name]
    cfg = vo.VaeConfig(**kw)
    return kw, cfg, vo.seeded_state_dict(cfg, 321), mw.image8(xs, 11), (mw.latent(zs, 12) if zs else None), chunk_bytes, plan


def _walk_vae(monkeypatch, engine, name, end, pair_convs=True):
    kw, cfg, sd, x8, z, chunk_bytes, plan = _vae_case(name)
    x = x8 if end == "encoder" else z
    trace, out = mw.run_vae(monkeypatch, engine, "cpu", kw, sd, end, x, chunk_bytes, pair_convs)
    got_plan = mw.walk_vae(trace, sd, cfg, end, x, out, pair_convs)
    return trace, got_plan, plan


# ------------------------------------------------------------------------------------------------------------------ the emulated engine passes
@pytest.mark.parametrize("name,end", [("even", "encoder"), ("even", "decoder"), ("odd", "encoder"), ("odd", "decoder"), ("chunks", "encoder")])
def test_emulated_vae_passes_every_node(monkeypatch, emu, name, end):
    trace, got_plan, plan = _walk_vae(monkeypatch, emu(), name, end)
    if end == "encoder":
        assert got_plan == [plan]
    kinds = {c.fn for c in trace}
    assert ("conv3x3_pair_nhwc" in kinds) and ("conv3x3_nhwc" in kinds)


def test_emulated_vae_without_pair_convs(monkeypatch, emu):
    trace, _, _ = _walk_vae(monkeypatch, emu(), "even", "encoder", pair_convs=False)
    assert not any(c.fn == "conv3x3_pair_nhwc" for c in trace)


@pytest.mark.parametrize("end", ["encoder", "decoder"])
def test_emulated_vae_tiled_passes(monkeypatch, emu, end):
    """Six tiles of three sizes through ONE model object.  This is the run that found `_attend` leaving an earlier, larger tile's softmax
    weights in the padded key columns of its reused buffer (the attend node asserts that padding zero): it needs no GPU to fail."""
    kw, sample_size, xs, zs = mw.VAE_TILED_CASE
    cfg = vo.VaeConfig(**kw)
    sd = vo.seeded_state_dict(cfg, 1300)
    x = mw.image8(xs, 21) if end == "encoder" else mw.latent(zs, 22)
    trace, out = mw.run_vae(monkeypatch, emu(), "cpu", kw, sd, end, x, tiling=sample_size)
    assert mw.walk_vae_tiled(trace, sd, cfg, end, x, out, sample_size) == 6            # a ragged 2 x 3 tile grid
    assert sum(c.fn == "blend_edge_nhwc_" for c in trace) == 7


@pytest.mark.parametrize("T", [40, 129])
def test_emulated_t5_passes_every_node(monkeypatch, emu, T):
    sd, ids = mw.t5_state_dict(), mw.t5_ids(T)
    trace, out = mw.run_t5(monkeypatch, emu(), "cpu", sd, ids)
    mw.walk_t5(trace, sd, mw.t5_oracle_cfg(), ids, out)


def test_emulated_clip_passes_every_node(monkeypatch, emu):
    sd, ids = mw.clip_state_dict(), mw.clip_ids()
    trace, last, pooled = mw.run_clip(monkeypatch, emu(), "cpu", sd, ids)
    mw.walk_clip(trace, sd, mw.clip_oracle_cfg(), ids, last, pooled)


# ------------------------------------------------------------------------------------------------------------------ named faults
E, D = "encoder.", "decoder."
VAE_FAULTS = [
    # (fault, label of the faulty call's weight, case, end, node that must reject it)
    ("border_column", "hw:encoder.down_blocks.2.resnets.0.conv1.weight", "odd", "encoder", E + "down_blocks.2.resnets.0.conv1"),
    ("border_column", "hw:encoder.down_blocks.0.resnets.0.conv1.pair[0]", "odd", "encoder", E + "down_blocks.0.resnets.0.conv1"),
    ("down_pad", "hw:encoder.down_blocks.0.downsamplers.0.conv.weight", "odd", "encoder", E + "down_blocks.0.downsamplers.0.conv"),
    ("up_after", "hw:decoder.up_blocks.0.upsamplers.0.conv.weight", "odd", "decoder", D + "up_blocks.0.upsamplers.0.conv"),
    ("bias_shifted", "hw:decoder.conv_out.weight", "odd", "decoder", D + "conv_out"),
    ("taps_transposed", "hw:encoder.down_blocks.0.resnets.0.conv1.pair[0]", "odd", "encoder", E + "down_blocks.0.resnets.0.conv1"),
    ("taps_transposed", "hw:encoder.mid_block.resnets.1.conv2.weight", "odd", "encoder", E + "mid_block.resnets.1.conv2"),
    ("res_before_shortcut", "hw:encoder.down_blocks.1.resnets.0.conv2.pair[0]", "odd", "encoder", E + "down_blocks.1.resnets.0.conv2"),
    ("gn_neighbour_stats", "sd:encoder.down_blocks.0.resnets.0.norm1.weight", "odd", "encoder", E + "down_blocks.0.resnets.0.norm1"),
    ("gn_no_silu", "sd:encoder.down_blocks.0.resnets.0.norm2.weight", "odd", "encoder", E + "down_blocks.0.resnets.0.norm2"),
    ("stale_ragged_weights", None, "chunks", "encoder", E + "mid_block.attentions.0.attend"),
    ("pad_weight", None, "odd", "encoder", E + "mid_block.attentions.0.attend"),
    ("softmax_scale", None, "odd", "decoder", D + "mid_block.attentions.0.attend"),
]


@pytest.mark.parametrize("fault,label,name,end,node", VAE_FAULTS, ids=[f"{f[0]}@{f[4]}" for f in VAE_FAULTS])
def test_vae_fault_is_rejected_at_its_node(monkeypatch, emu, fault, label, name, end, node):
    with pytest.raises(mw.NodeFailure) as e:
        _walk_vae(monkeypatch, emu((fault, label)), name, end)
    assert e.value.node == node, str(e.value)


def _t5_table_q_minus_k(t):
    return t.flip(-1).contiguous()                                       # bias(h, query - key)


def _t5_bucket_off_by_one(t):
    T = (t.shape[1] + 1) // 2
    t = t.clone()
    t[:, T - 1 + 17] = t[:, T - 1 + 23]                                  # distance 17 is in bucket 26 of 32, distance 23 in bucket 27
    return t


def test_the_off_by_one_fault_moves_distance_17_to_the_next_bucket():
    b = to.relative_position_bucket(torch.tensor([16, 17, 23]))
    assert b.tolist() == [26, 26, 27]


T5_FAULTS = [("wi_swapped", "w:0.wi", None, "t5.0.wi"), ("stream_not_rounded", "w:0.o", None, "t5.0.o"),
             (None, None, _t5_table_q_minus_k, "t5.0.attn"), (None, None, _t5_bucket_off_by_one, "t5.0.attn")]


@pytest.mark.parametrize("fault,label,table_fault,node", T5_FAULTS, ids=["wi_swapped", "stream_not_rounded", "bias_q_minus_k", "bucket_off_by_one"])
def test_t5_fault_is_rejected_at_its_node(monkeypatch, emu, fault, label, table_fault, node):
    sd, ids = mw.t5_state_dict(), mw.t5_ids(40)
    trace, out = mw.run_t5(monkeypatch, emu((fault, label) if fault else None), "cpu", sd, ids, table_fault=table_fault)
    with pytest.raises(mw.NodeFailure) as e:
        mw.walk_t5(trace, sd, mw.t5_oracle_cfg(), ids, out)
    assert e.value.node == node, str(e.value)


@pytest.mark.parametrize("fault,label,node", [("pos_shifted", "w:pos", "clip.pos"), ("causal_plus_one", None, "clip.0.attn"),
                                              ("pooled_eos_minus_one", None, "clip.pooled")])
def test_clip_fault_is_rejected_at_its_node(monkeypatch, emu, fault, label, node):
    sd, ids = mw.clip_state_dict(), mw.clip_ids()
    post = fault == "pooled_eos_minus_one"
    trace, last, pooled = mw.run_clip(monkeypatch, emu(None if post else (fault, label)), "cpu", sd, ids)
    if post:
        pooled = last[torch.arange(ids.shape[0]), ids.argmax(-1) - 1]
    with pytest.raises(mw.NodeFailure) as e:
        mw.walk_clip(trace, sd, mw.clip_oracle_cfg(), ids, last, pooled)
    assert e.value.node == node, str(e.value)


def test_a_missing_or_an_extra_launch_is_rejected(monkeypatch, emu):
    """The walk pins the launch sequence: a dropped call fails at the node it belonged to, a trailing one at the end."""
    sd, ids = mw.clip_state_dict(), mw.clip_ids()
    trace, last, pooled = mw.run_clip(monkeypatch, emu(), "cpu", sd, ids)
    cfg = mw.clip_oracle_cfg()
    with pytest.raises(mw.NodeFailure) as e:
        mw.walk_clip(trace[:3] + trace[4:], sd, cfg, ids, last, pooled)
    assert e.value.node == "clip.0.ln1"
    with pytest.raises(mw.NodeFailure) as e:
        mw.walk_clip(trace + trace[-1:], sd, cfg, ids, last, pooled)
    assert e.value.node == "end"


# ------------------------------------------------------------------------------------------------------------------ host-only checks
@pytest.mark.parametrize("buckets,max_distance", [(32, 128), (8, 20)])
def test_t5_rel_bias_table_equals_the_oracle_for_every_length(buckets, max_distance):
    from textflux_amd.text_encoders import T5EncoderModel
    sd = mw.t5_state_dict(buckets=buckets)
    extra = dict(relative_attention_num_buckets=buckets, relative_attention_max_distance=max_distance)
    m = T5EncoderModel({**mw.T5_CFG, **extra}).load_state_dict(sd, device="cpu")
    cfg = mw.t5_oracle_cfg(buckets, max_distance)
    sd16 = to.t5_state_dict_as_loaded(sd)
    for T in range(1, 513):
        table = m._rel_bias(T)
        assert table.shape == (mw.T5_CFG["num_heads"], 2 * T - 1) and table.dtype == torch.float32
        idx = torch.arange(T)[None, :] - torch.arange(T)[:, None] + T - 1                 # key - query + T - 1
        assert torch.equal(table[:, idx], to.t5_position_bias(sd16, cfg, T)[0].float()), T


@pytest.mark.parametrize("kw", [mw.VAE_KW, mw.VAE_TILED_KW], ids=["3-level", "4-level"])
def test_vae_packed_filters_unpack_to_the_state_dict(kw):
    """Every 3 x 3 weight of AutoencoderKL._prep, read back through the layouts include/textflux_hip.h and ops.pair_conv_weights document,
    is the state-dict filter exactly, and all padding is zero."""
    from textflux_amd.vae import AutoencoderKL, _narrow
    cfg = vo.VaeConfig(**kw)
    vae = AutoencoderKL(**kw).load_state_dict(vo.seeded_state_dict(cfg, 5), device="cpu")
    seen = 0
    for k, f in vae.sd.items():
        if not (k.endswith(".weight") and f.dim() == 4):
            continue
        name, (cout, cin) = k[:-7], f.shape[:2]
        w = vae.hw[k]
        if f.shape[2] == 1:
            assert torch.equal(w, f.view(cout, cin))
            continue
        seen += 1
        coutp = (cout + 7) // 8 * 8
        krsc = f.permute(0, 2, 3, 1)
        if cin % 64:
            cp = _narrow(cin)
            assert w.shape == (coutp, (9 * cp + 63) // 64 * 64)
            taps = w[:, :9 * cp].view(coutp, 3, 3, cp)
            assert not w[:, 9 * cp:].any() and not taps[..., cin:].any()
            taps = taps[..., :cin]
        else:
            assert w.shape == (coutp, 3, 3, cin)
            taps = w
        assert torch.equal(taps[:cout], krsc) and not taps[cout:].any()
        if coutp != cout:
            b = vae.hw[name + ".bias"]
            assert b.shape == (coutp,) and torch.equal(b[:cout], vae.sd[name + ".bias"]) and not b[cout:].any()
        else:
            assert name + ".bias" not in vae.hw
        pair = vae.hw.get(name + ".pair")
        assert (pair is not None) == (cin % 64 == 0 and cout % 8 == 0 and cout <= 128)
        if pair is not None:
            wp, bp = pair[0].view(2, cout, 3, 4, cin), pair[1]
            assert torch.equal(wp[0, :, :, 0:3], krsc) and not wp[0, :, :, 3].any()
            assert torch.equal(wp[1, :, :, 1:4], krsc) and not wp[1, :, :, 0].any()
            assert torch.equal(bp, torch.cat([vae.sd[name + ".bias"]] * 2))
    assert seen >= 20
