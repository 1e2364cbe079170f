"""CPU-side checks of the runtime (unmerged) LoRA path: the packing of adapters into the operands of the GEMM tail (pure torch), the new
C-ABI surface (symbols, NULL rejection, the adapter-scratch arithmetic -- no GPU call), the CLI flags, and the emitted ISA of the tail
instantiations of the persistent GEMM (tests/test_isa_hazards.py then gates their K loops like every other instantiation's)."""
import ctypes as C
import os
import re

import pytest
import torch

from textflux_amd import _lib as L
from textflux_amd import lora

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 256


def fusion_map():
    """The fused layouts of the engine: [k; v; q] of both streams of a double block (an [img; txt] pair), single-target Linears,
    [k; v; q; mlp] of a single block -- and two Linears outside the blocks."""
    m = [("transformer_blocks.0.attn.to_k", "d0.qkv_img", 0), ("transformer_blocks.0.attn.to_v", "d0.qkv_img", D),
         ("transformer_blocks.0.attn.to_q", "d0.qkv_img", 2 * D),
         ("transformer_blocks.0.attn.add_k_proj", "d0.qkv_txt", 0), ("transformer_blocks.0.attn.add_v_proj", "d0.qkv_txt", D),
         ("transformer_blocks.0.attn.add_q_proj", "d0.qkv_txt", 2 * D),
         ("transformer_blocks.0.attn.to_out.0", "d0.out_img", 0), ("transformer_blocks.0.ff.net.2", "d0.ff2_img", 0),
         ("single_transformer_blocks.0.attn.to_k", "s0.qkv_mlp", 0), ("single_transformer_blocks.0.attn.to_v", "s0.qkv_mlp", D),
         ("single_transformer_blocks.0.attn.to_q", "s0.qkv_mlp", 2 * D), ("single_transformer_blocks.0.proj_mlp", "s0.qkv_mlp", 3 * D),
         ("single_transformer_blocks.0.proj_out", "s0.proj_out", 0),
         ("proj_out", "proj_out", 0), ("transformer_blocks.0.norm1.linear", "mod", 0)]
    shapes = {"d0.qkv_img": (3 * D, D), "d0.qkv_txt": (3 * D, D), "d0.out_img": (D, D), "d0.ff2_img": (D, 4 * D),
              "s0.qkv_mlp": (7 * D, D), "s0.proj_out": (D, 5 * D), "proj_out": (64, D), "mod": (6 * D, D)}
    return m, shapes


def rows_of(key, shapes, m):
    name, off = next((n, o) for k, n, o in m if k == key)
    offs = sorted(o for k, n, o in m if n == name)
    nxt = [o for o in offs if o > off]
    return name, off, (nxt[0] if nxt else shapes[name][0]) - off


def make_adapter(targets, rank, seed, alpha=None):
    m, shapes = fusion_map()
    g = torch.Generator().manual_seed(seed)
    sd, alphas = {}, {}
    for i, t in enumerate(targets):
        name, _, rows = rows_of(t, shapes, m)
        sd[f"transformer.{t}.lora_A.weight"] = torch.randn(rank, shapes[name][1], generator=g)
        sd[f"transformer.{t}.lora_B.weight"] = torch.randn(rows, rank, generator=g)
        if alpha is not None and i % 2:
            alphas[f"transformer.{t}.alpha"] = torch.tensor(float(alpha))
    return sd, alphas


def merged_reference(name, W, adapters, weights, scale):
    """fp64 W + sum c * bf16(B) @ bf16(A), c = fp32(scale * weight * alpha / r), over every (adapter, target) of the fused tensor `name`."""
    m, shapes = fusion_map()
    out = W.double().clone()
    for an, (sd, alphas) in adapters.items():
        for k in [k for k in sd if k.endswith(".lora_A.weight")]:
            t = k[len("transformer."):-len(".lora_A.weight")]
            n, off, rows = rows_of(t, shapes, m)
            if n != name:
                continue
            A, B = sd[k].bfloat16().double(), sd[k.replace("lora_A", "lora_B")].bfloat16().double()
            r = A.shape[0]
            al = float((alphas or {}).get(f"transformer.{t}.alpha", r))
            c = float(torch.tensor(scale * weights[an] * (al / r), dtype=torch.float32))     # c is an fp32 quantity (the device vector)
            out[off:off + rows] += c * (B @ A)
    return out


def adapted_linear(x, W, p, c):
    """the engine's formula in fp64 (no rounding of t): x W^T + sum_seg (c_seg * x Acat_seg^T) Bcat[seg rows]^T"""
    y = x @ W.double().T
    N = W.shape[0]
    for s in range(p.nseg):
        lo, hi = s * p.seg_cols, ((s + 1) * p.seg_cols if s + 1 < p.nseg else N)
        t = (x @ p.Acat[s * p.R:(s + 1) * p.R].double().T) * c[s * p.R:(s + 1) * p.R].double()
        if p.seg_mask >> s & 1:
            y[:, lo:hi] += t @ p.Bcat[lo:hi].double().T
        else:
            assert p.Bcat[lo:hi].abs().max() == 0 and p.Acat[s * p.R:(s + 1) * p.R].abs().max() == 0
    return y


QKV_IMG = ["transformer_blocks.0.attn.to_k", "transformer_blocks.0.attn.to_v", "transformer_blocks.0.attn.to_q"]
QKV_TXT = ["transformer_blocks.0.attn.add_k_proj", "transformer_blocks.0.attn.add_q_proj"]
SINGLE = ["single_transformer_blocks.0.attn.to_k", "single_transformer_blocks.0.attn.to_v", "single_transformer_blocks.0.attn.to_q"]
ONE = ["transformer_blocks.0.attn.to_out.0", "transformer_blocks.0.ff.net.2", "single_transformer_blocks.0.proj_out"]


@pytest.mark.parametrize("rank", [8, 16, 128, 192])
@pytest.mark.parametrize("targets", [QKV_IMG + QKV_TXT, SINGLE, SINGLE + ["single_transformer_blocks.0.proj_mlp"], ONE,
                                     ["transformer_blocks.0.attn.to_q"]], ids=["pair", "kvq_mlp_untargeted", "kvq_mlp", "single_target", "q_only"])
def test_packed_operands_restate_the_merged_linear(targets, rank):
    m, shapes = fusion_map()
    adapters = {"a": make_adapter(targets, rank, 1, alpha=8.0)}
    packs = lora.pack_runtime_adapter(adapters, m, shapes)
    assert sorted(packs) == sorted({rows_of(t, shapes, m)[0] for t in targets})
    g = torch.Generator().manual_seed(2)
    for name, p in packs.items():
        N, K = shapes[name]
        assert p.R == (rank + 127) // 128 * 128 and p.Acat.shape == (p.nseg * p.R, K) and p.Bcat.shape == (N, p.R)
        assert p.Acat.dtype == p.Bcat.dtype == torch.bfloat16
        assert p.Bcat[:, rank:].abs().sum() == 0 and p.Acat.view(p.nseg, p.R, K)[:, rank:].abs().sum() == 0     # padding
        assert p.nseg == sum(1 for _, n, _ in m if n == name) and p.seg_cols == (D if p.nseg > 1 else N)
        W, x = torch.randn(N, K, generator=g).bfloat16(), torch.randn(5, K, generator=g, dtype=torch.float64)
        for scale, w in ((1.0, 1.0), (0.5, 0.7)):
            c = p.scale_vector({"a": w}, scale)
            assert c.dtype == torch.float32 and c.view(p.nseg, p.R)[:, rank:].abs().sum() == 0
            got = adapted_linear(x, W, p, c)
            ref = x @ merged_reference(name, W, adapters, {"a": w}, scale).T
            assert (got - ref).abs().max() <= 1e-9 * ref.abs().max()
        assert p.scale_vector({}, 1.0).abs().max() == 0                     # an inactive adapter contributes nothing


def test_two_adapters_on_one_target_concatenate_along_the_rank_axis_and_the_cap_raises():
    m, shapes = fusion_map()
    adapters = {"a": make_adapter(QKV_IMG, 16, 1, alpha=8.0), "b": make_adapter(["transformer_blocks.0.attn.to_q", "transformer_blocks.0.attn.to_out.0"], 120, 2, alpha=30.0)}
    packs = lora.pack_runtime_adapter(adapters, m, shapes)
    p = packs["d0.qkv_img"]
    assert p.R == 256 and p.seg_mask == 0b111 and packs["d0.out_img"].R == 128          # 16 + 120 pads to 256
    assert sorted(e[:4] for e in p.entries) == [("a", 0, 0, 16), ("a", 1, 0, 16), ("a", 2, 0, 16), ("b", 2, 16, 136)]
    g = torch.Generator().manual_seed(3)
    W, x = torch.randn(3 * D, D, generator=g).bfloat16(), torch.randn(4, D, generator=g, dtype=torch.float64)
    w = {"a": 0.7, "b": 0.3}
    got = adapted_linear(x, W, p, p.scale_vector(w, 0.9))
    ref = x @ merged_reference("d0.qkv_img", W, adapters, w, 0.9).T
    assert (got - ref).abs().max() <= 1e-9 * ref.abs().max()
    adapters["c"] = make_adapter(["transformer_blocks.0.attn.to_q"], 128, 4)             # 16 + 120 + 128 > 256
    with pytest.raises(ValueError, match="256"):
        lora.pack_runtime_adapter(adapters, m, shapes)


def test_targets_the_runtime_path_does_not_take_are_refused_like_the_merged_path_refuses_them():
    m, shapes = fusion_map()
    with pytest.raises(ValueError, match="proj_out.*merged path"):
        lora.pack_runtime_adapter({"a": make_adapter(["proj_out"], 8, 1)}, m, shapes)
    with pytest.raises(ValueError, match="norm1.linear.*merged path"):
        lora.pack_runtime_adapter({"a": make_adapter(["transformer_blocks.0.norm1.linear"], 8, 1)}, m, shapes)
    with pytest.raises(KeyError, match="is not a Linear of FluxTransformer2DModel"):
        lora.pack_runtime_adapter({"a": ({"transformer.nope.lora_A.weight": torch.zeros(8, D), "transformer.nope.lora_B.weight": torch.zeros(D, 8)}, None)}, m, shapes)
    sd, _ = make_adapter(["transformer_blocks.0.attn.to_q"], 8, 1)
    sd["transformer.transformer_blocks.0.attn.to_q.lora_B.weight"] = torch.zeros(D + 8, 8)
    with pytest.raises(ValueError, match="do not match the target weight"):
        lora.pack_runtime_adapter({"a": (sd, None)}, m, shapes)
    with pytest.raises(NotImplementedError, match="Kohya"):
        lora.pack_runtime_adapter({"a": ({"lora_unet_x.lora_down.weight": torch.zeros(1)}, None)}, m, shapes)


# ---------------------------------------------------------------------------------------------------- C ABI
@pytest.fixture(scope="module")
def lib():
    L.build()
    return L.lib()


def test_new_entry_point_is_declared_bound_exported_and_rejects_null(lib):
    header = open(os.path.join(REPO, "include", "textflux_hip.h")).read()
    assert "tfx_gemm_bf16_lora" in header and "tfx_gemm_bf16_lora" in L.SIGNATURES and hasattr(lib, "tfx_gemm_bf16_lora")
    assert L.ABI_VERSION == L.header_abi_version() >= 9
    assert lib.tfx_gemm_bf16_lora(None, None, None, None) != 0 and b"null" in lib.tfx_last_error()
    g, l = L.GemmArgs(), L.LoraArgs()
    assert lib.tfx_gemm_bf16_lora(C.byref(g), None, C.byref(l), None) != 0 and b"null matrix pointer" in lib.tfx_last_error()
    g.A = g.W = g.C = 4096                                # never dereferenced: the adapter operands are checked first
    assert lib.tfx_gemm_bf16_lora(C.byref(g), None, C.byref(l), None) != 0 and b"T / Bm" in lib.tfx_last_error()
    # the ctypes mirrors carry the new fields
    assert [f for f, _ in L.GemmArgs._fields_][-1] == "cscale"
    assert {"ldw", "lora_a", "lora_r", "lora_nseg", "lora_mask", "lora_scale_off"} <= {f for f, _ in L.Linear._fields_}
    assert [f for f, _ in L.DitDesc._fields_][-3:] == ["lora_t_xn", "lora_t_y", "lora_scale"]


def test_adapter_scratch_is_appended_behind_the_existing_workspace_parts(lib):
    for (B, S, T, Dm) in ((8, 4096, 512, 3072), (1, 64, 16, 256)):
        N = S + T
        base, gws0 = (C.c_int64 * 6)(), C.c_int64()
        assert lib.tfx_workspace_layout(B, S, T, Dm, 0, base, C.byref(gws0)) == 0
        off, gws = (C.c_int64 * 8)(), C.c_int64()
        assert lib.tfx_workspace_layout(B, S, T, Dm, 8, off, C.byref(gws)) == 0
        assert list(off)[:6] == list(base) and gws.value == gws0.value                   # nothing that existed moves
        hid, y = B * N * Dm * 2, B * N * 7 * Dm * 2
        planes = 1 if Dm >= 1024 else 4
        assert off[6] == base[5] + gws0.value and off[7] == off[6] + planes * hid
        assert lib.tfx_workspace_bytes(B, S, T, Dm, 8) == off[7] + y
        assert lib.tfx_workspace_bytes(B, S, T, Dm, 0) == base[5] + gws0.value
        assert all(o % 256 == 0 for o in off if o >= 0)                                  # (q8 / q8_scale: -1 without the fp8 flag)
        # T above its input inside one 32-bit range: xn -> lora_t_xn (+ the per-segment matrices), y -> lora_t_y
        assert off[6] - off[1] + planes * hid < (1 << 32) - 65536 and off[7] - off[2] + y < (1 << 32) - 65536
    f8 = (C.c_int64 * 8)()
    assert lib.tfx_workspace_layout(8, 4096, 512, 3072, 4 | 8, f8, None) == 0 and f8[3] > 0 and f8[6] > f8[5]


# ---------------------------------------------------------------------------------------------------- CLIs
def test_lora_clis_parse_the_new_flags_and_default_to_the_merged_path():
    import sys
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "scripts"))
    import run_eval
    import run_inference_lora as rl
    a = rl.build_parser().parse_args(["--image", "i.png", "--mask", "m.png", "--words", "w"])
    assert a.lora_runtime is False and a.lora_scale == 1.0 and a.steps == 30 and a.seed == 42
    a = rl.build_parser().parse_args(["--image", "i.png", "--mask", "m.png", "--words", "w", "--lora_runtime", "--lora_scale", "0.6"])
    assert a.lora_runtime is True and a.lora_scale == 0.6
    e = run_eval.build_parser(lora=True).parse_args([])
    assert e.lora_runtime is False and e.lora_scale == 1.0 and e.scheduler == "overshoot"
    e = run_eval.build_parser(lora=True).parse_args(["--lora_runtime", "--lora_scale", "0.5"])
    assert e.lora_runtime is True and e.lora_scale == 0.5
    assert not hasattr(run_eval.build_parser(lora=False).parse_args([]), "lora_runtime")


# ---------------------------------------------------------------------------------------------------- ISA
def test_tail_instantiations_of_the_persistent_gemm_exist_without_scratch(tmp_path):
    from tests.test_isa_hazards import HIPCC, isa
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    asm = isa("gemm.hip", tmp_path)
    # gemm8pp_kernel<EPI, PLACE = 2, FP8 = false, SPLIT = false, QKN, LORA = true>: bias, bias + GELU, gated residual, residual, q / k norm
    want = {"bias": "Li0ELi2ELb0ELb0ELb0ELb1E", "bias_gelu": "Li1ELi2ELb0ELb0ELb0ELb1E", "gate_res": "Li2ELi2ELb0ELb0ELb0ELb1E",
            "res": "Li3ELi2ELb0ELb0ELb0ELb1E", "qkn": "Li1ELi2ELb0ELb0ELb1ELb1E"}
    for what, targs in want.items():
        name = f"_ZN3tfx14gemm8pp_kernelI{targs}EEvNS_10GemmParamsE"
        assert f".amdhsa_kernel {name}" in asm, what
        desc = asm[asm.index(".amdhsa_kernel " + name):]
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", desc).group(1)) == 0, what
        vgpr = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", desc).group(1))
        assert vgpr <= 256, (what, vgpr)
    # ... and the down projection's column-scale epilogue in the persistent kernel (whole tiles and K-sliced units)
    for targs in ("Li4ELi2ELb0ELb0ELb0ELb0E", "Li4ELi2ELb0ELb1ELb0ELb0E"):
        assert f".amdhsa_kernel _ZN3tfx14gemm8pp_kernelI{targs}EEvNS_10GemmParamsE" in asm
