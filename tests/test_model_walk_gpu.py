"""Every layer output of the VAE and of the two text encoders, element by element: the engine's own kernel calls are recorded
(tests/helpers/model_walk.py) and walked against the graph of oracle/vae_oracle.py / oracle/text_oracle.py -- the wiring with torch.equal,
every node's value in fp64 from the device's own inputs and the original state-dict tensors, every element inside a derived window of bf16
values.  tests/test_model_walk_cpu.py proves on the CPU that this walk rejects eighteen named faults at their nodes.  The shapes are the
smallest at which each path of the composition is still taken; each test prints, per node kind, the nodes and elements it checked and how
much of the derived bound the device used (`room`, see model_walk.Walk)."""
import pytest
import torch

from oracle import vae_oracle as vo
from tests.helpers import model_walk as mw

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    from textflux_amd import ops as o
    return o


def _report(what, stats):
    print(f"\n{what}: {sum(s['nodes'] for s in stats.values())} nodes, {sum(s['elements'] for s in stats.values())} elements\n"
          + mw.format_stats(stats))


def _vae(monkeypatch, ops, name, pair_convs=True):
    kw, xs, zs, chunk_bytes, plan = mw.VAE_CASES[name]
    cfg = vo.VaeConfig(**kw)
    sd = vo.seeded_state_dict(cfg, 321)
    stats, traces = {}, []
    for end, x in (("encoder", mw.image8(xs, 11)), ("decoder", mw.latent(zs, 12) if zs else None)):
        if x is None:
            continue
        with monkeypatch.context() as mp:
            trace, out = mw.run_vae(mp, ops, "cuda", kw, sd, end, x, chunk_bytes, pair_convs)
        got_plan = mw.walk_vae(trace, sd, cfg, end, x, out, pair_convs, stats=stats)
        if end == "encoder":
            assert got_plan == [plan]
        traces.append(trace)
    _report(f"VAE {name}" + ("" if pair_convs else ", pair_convs off"), stats)
    return traces


def test_vae_even_widths_every_node(monkeypatch, ops):
    """Pair form at every <= 128-channel layer, the shortcut GEMMs, both narrow conv_in layers, the padded conv_out; 120 tokens in a
    256-row scratch (rows > N): the ragged path, one softmax launch per image."""
    enc, dec = _vae(monkeypatch, ops, "even")
    for trace in (enc, dec):
        assert sum(c.fn == "conv3x3_pair_nhwc" for c in trace) >= 4 and sum(c.fn == "conv3x3_nhwc" for c in trace) >= 2
    assert sum(c.fn == "row_softmax" for c in enc) == 2


def test_vae_odd_widths_every_node(monkeypatch, ops):
    """Level widths 20, 10, 5 (decoder 3, 6, 12): the plain form on layers that took the pair form at even widths."""
    enc, dec = _vae(monkeypatch, ops, "odd")
    plain = lambda trace: sum(c.fn == "conv3x3_nhwc" for c in trace)
    assert plain(enc) >= 7 and plain(dec) >= 7


def test_vae_attention_chunks_every_node(monkeypatch, ops):
    """300 tokens through 256-row chunks: a full chunk (ONE batched softmax launch) and a ragged chunk of 44 (a launch per image)."""
    enc, = _vae(monkeypatch, ops, "chunks")
    assert [tuple(c.args[0].shape) for c in enc if c.fn == "row_softmax"] == [(512, 300), (44, 300), (44, 300)]
    assert [tuple(c.out.shape) for c in enc if c.fn == "gemm_f32"] == [(2, 256, 300), (2, 44, 300)]


def test_vae_without_pair_convs_every_node(monkeypatch, ops):
    enc, dec = _vae(monkeypatch, ops, "even", pair_convs=False)
    assert not any(c.fn == "conv3x3_pair_nhwc" for c in enc + dec)


def test_vae_tiled_every_tile_blend_and_crop(monkeypatch, ops):
    kw, sample_size, xs, zs = mw.VAE_TILED_CASE
    cfg = vo.VaeConfig(**kw)
    sd = vo.seeded_state_dict(cfg, 1300)
    stats = {}
    for end, x in (("encoder", mw.image8(xs, 21)), ("decoder", mw.latent(zs, 22))):
        with monkeypatch.context() as mp:
            trace, out = mw.run_vae(mp, ops, "cuda", kw, sd, end, x, tiling=sample_size)
        assert mw.walk_vae_tiled(trace, sd, cfg, end, x, out, sample_size, stats=stats) == 6
        assert sum(c.fn == "blend_edge_nhwc_" for c in trace) == 7
    _report("VAE tiled", stats)


@pytest.mark.parametrize("T", [40, 129])
def test_t5_every_node(monkeypatch, ops, T):
    sd, ids = mw.t5_state_dict(), mw.t5_ids(T)
    trace, out = mw.run_t5(monkeypatch, ops, "cuda", sd, ids)
    stats = {}
    mw.walk_t5(trace, sd, mw.t5_oracle_cfg(), ids, out, stats=stats)
    _report(f"T5, {T} tokens", stats)


def test_clip_every_node(monkeypatch, ops):
    sd, ids = mw.clip_state_dict(), mw.clip_ids()
    trace, last, pooled = mw.run_clip(monkeypatch, ops, "cuda", sd, ids)
    stats = {}
    mw.walk_clip(trace, sd, mw.clip_oracle_cfg(), ids, last, pooled, stats=stats)
    _report("CLIP", stats)
