"""The forward chain helper's view of the layout (tests/helpers/plain_forward.py) held to the oracle on the CPU: the packed weights,
the modulation chunk order, the rotary rows and the runtime-LoRA operands.  The chain itself runs here on its plain-torch backend
in fp32 -- the same orchestration code that issues the HIP launches in tests/test_forward_chain_gpu.py -- and must give the
oracle's blocks to fp32 rounding: sums of at most 1280 products of O(1) terms in another order, 1e-5 absolute; the bound below is
1e-4, and a layout mistake is O(1)."""
import pytest
import torch

from oracle import flux_oracle as fo
from oracle import pipeline_oracle as po
from tests.helpers import plain_forward as pf
from tests.helpers import tiny_checkpoint as tc

CFG = tc.TR_CFG
B, S, T, GRID = 2, 12, 5, (3, 4)


def rnd(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def ids():
    txt = torch.zeros(T, 3)
    txt[:, 1], txt[:, 2] = torch.arange(T), 3 * torch.arange(T) + 1
    return txt, po.latent_image_ids(*GRID)


@pytest.fixture(scope="module")
def world():
    sd = fo.seeded_state_dict(CFG, 7)
    D = CFG.inner_dim
    w = dict(sd=sd, W=pf.pack_weights(sd, CFG), hidden=rnd((B, S, D), 1), enc=rnd((B, T, D), 2), temb=rnd((B, D), 3))
    w["mod"] = pf.reference_modulation(sd, CFG, w["temb"])
    w["txt_ids"], w["img_ids"] = ids()
    w["bounds"] = ([0.0] * CFG.num_layers, [0.0] * CFG.num_single_layers)
    return w


def close(got, ref):
    assert got.shape == ref.shape
    assert (got - ref).abs().max().item() <= 1e-4, (got - ref).abs().max().item()


def chain(w, blocks, fault=None, hid0=None):
    be = pf.TorchBackend(w["W"], CFG, B, S, T)
    cos, sin = pf.rope_rows(w["txt_ids"], w["img_ids"], CFG, fault)
    return pf.plain_forward(be, w["mod"], cos, sin, w["bounds"], hid0=torch.cat((w["enc"], w["hidden"]), 1) if hid0 is None else hid0,
                            blocks=blocks, tail=False, fault=fault)["hid"][-1]


def test_mod_len_and_chunk_order(world):
    assert world["mod"].shape == (B, pf.mod_len(CFG))
    m = pf.mod_slices(world["mod"], CFG)
    st = torch.nn.functional.silu(world["temb"])
    six = fo.linear(st, world["sd"], "transformer_blocks.1.norm1_context.linear").chunk(6, dim=1)
    for name, ref in zip(pf.SIX, six):
        assert torch.equal(m["double"][1]["txt"][name], ref), name
    scale, shift = fo.linear(st, world["sd"], "norm_out.linear").chunk(2, dim=1)
    assert torch.equal(m["out"]["scale"], scale) and torch.equal(m["out"]["shift"], shift)
    shift, scale, gate = fo.linear(st, world["sd"], "single_transformer_blocks.1.norm.linear").chunk(3, dim=1)
    assert torch.equal(m["single"][1]["shift"], shift) and torch.equal(m["single"][1]["gate"], gate)


@pytest.mark.parametrize("i", range(CFG.num_layers))
def test_double_block_through_packed_weights_is_the_oracles(world, i):
    cos, sin = fo.flux_pos_embed(torch.cat((world["txt_ids"], world["img_ids"])), CFG.axes_dims_rope)
    enc, hid = fo.double_block(world["sd"], f"transformer_blocks.{i}", CFG.num_attention_heads, world["hidden"], world["enc"],
                               world["temb"], cos, sin)
    close(chain(world, [i]), torch.cat((enc, hid), 1))


@pytest.mark.parametrize("j", range(CFG.num_single_layers))
def test_single_block_through_packed_weights_is_the_oracles(world, j):
    cos, sin = fo.flux_pos_embed(torch.cat((world["txt_ids"], world["img_ids"])), CFG.axes_dims_rope)
    ref = fo.single_block(world["sd"], f"single_transformer_blocks.{j}", CFG.num_attention_heads,
                          torch.cat((world["enc"], world["hidden"]), 1), world["temb"], cos, sin)
    close(chain(world, [CFG.num_layers + j]), ref)


def test_whole_chain_is_the_oracles_forward(world):
    sd = world["sd"]
    x, pe, pooled = rnd((B, S, CFG.in_channels), 4), rnd((B, T, CFG.joint_attention_dim), 5), rnd((B, CFG.pooled_projection_dim), 6)
    t, g = torch.tensor([0.9, 0.12]), torch.full((B,), 30.0)
    ref = fo.transformer_forward(sd, CFG, x, pe, pooled, t, world["img_ids"], world["txt_ids"], g)
    mod = pf.reference_modulation(sd, CFG, fo.time_text_embed(sd, t * 1000, g * 1000, pooled))
    cos, sin = pf.rope_rows(world["txt_ids"], world["img_ids"], CFG)
    got = pf.plain_forward(pf.TorchBackend(world["W"], CFG, B, S, T), mod, cos, sin, world["bounds"], xin=x, prompt_embeds=pe)
    assert len(got["hid"]) == 1 + CFG.num_layers + CFG.num_single_layers
    close(got["out"], ref)


def test_rope_rows_are_the_oracles_for_non_zero_text_ids(world):
    txt, img = world["txt_ids"], world["img_ids"]
    cos, sin = pf.rope_rows(txt, img, CFG)
    rc, rs = fo.flux_pos_embed(torch.cat((txt, img)), CFG.axes_dims_rope)
    assert cos.shape == (T + S, 128) and torch.equal(cos, rc) and torch.equal(sin, rs)
    assert not torch.equal(cos[:T], cos[:1].expand(T, -1))              # the text rows really are rotated
    c1, _ = pf.rope_rows(txt, img, CFG, "txt_rope_shift_one")
    assert torch.equal(c1[:T], rc[1:T + 1]) and torch.equal(c1[T:], rc[T:]) and not torch.equal(c1, rc)
    c2, _ = pf.rope_rows(txt, img, CFG, "img_rope_from_row0")
    assert torch.equal(c2[T:], rc[:S]) and torch.equal(c2[:T], rc[:T])
    # the blind spot of zero text ids: every text row and the first image row hold the identity, a shift by one shows nothing
    z = torch.zeros(T, 3)
    a, b = pf.rope_rows(z, img, CFG), pf.rope_rows(z, img, CFG, "txt_rope_shift_one")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("fault", sorted(f for f, where in pf.FAULTS.items() if where != "tail"))
def test_every_fault_moves_the_fp32_chain(world, fault):
    L = CFG.num_layers
    blocks = dict(double=[1], single=[L + 1], both=[1, L + 1])[pf.FAULTS[fault]]
    for k in blocks:
        d = (chain(world, [k], fault) - chain(world, [k])).abs().max().item()
        assert d > 1e-3, (fault, k, d)


def test_lora_operands_are_the_merged_update(world):
    """x W^T + (c * (x Acat_s^T)) Bcat^T == x (W + scale * alpha / r * B A)^T for every adapted reference Linear, nothing for the
    others: pack_lora against the definition (PEFT's lora.Linear, D/utils/peft_utils.py:103-120), in fp32."""
    sd, W = world["sd"], world["W"]
    g = torch.Generator().manual_seed(3)
    lora, r = {}, 8
    for i, t in enumerate(tc.LORA_TARGETS):
        o, k = sd[t + ".weight"].shape
        lora[f"transformer.{t}.lora_A.weight"] = (torch.randn(r, k, generator=g) * 0.2).to(pf.BF)
        lora[f"transformer.{t}.lora_B.weight"] = (torch.randn(o, r, generator=g) * 0.2).to(pf.BF)
        if i % 2:
            lora[f"transformer.{t}.alpha"] = torch.tensor(4.0)
    packs = pf.pack_lora(W, lora, call_scale=0.5)
    assert sorted(packs) == ["d0.ff1_img", "d0.qkv_img", "d1.ff2_txt", "d1.qkv_txt", "s0.qkv_mlp", "s1.qkv_mlp"]
    assert [packs[n]["mask"] for n in ("d0.qkv_img", "d1.qkv_txt", "s0.qkv_mlp", "s1.qkv_mlp", "d0.ff1_img")] == [4, 1, 2, 1, 1]
    for name, p in packs.items():
        N, K = W[name]["w"].shape
        R, nseg = p["R"], p["nseg"]
        assert R == 128 and p["wide"].shape == (N, K + R) and p["acat"].shape == (nseg * R, K) and p["seg_cols"] == (N if nseg == 1 else CFG.inner_dim)
        x = rnd((7, K), 9)
        merged = W[name]["w"].to(pf.BF).float().clone()
        for s, (key, r0, rows) in enumerate(W[name]["segs"]):
            if key in tc.LORA_TARGETS:
                alpha = float(lora.get(f"transformer.{key}.alpha", float(r)))
                merged[r0:r0 + rows] += 0.5 * alpha / r * (lora[f"transformer.{key}.lora_B.weight"].float() @ lora[f"transformer.{key}.lora_A.weight"].float())
        got = x @ p["wide"][:, :K].float().T
        for n0 in range(0, N, 256):
            s = min(n0 // p["seg_cols"], nseg - 1)
            t = p["c"][s * R:(s + 1) * R] * (x @ p["acat"][s * R:(s + 1) * R].float().T)
            got[:, n0:n0 + 256] += t @ p["wide"][n0:n0 + 256, K:].float().T
        close(got, x @ merged.T)
