"""LoRA load path: parse a diffusers/PEFT-format LoRA file and MERGE it into the fused transformer weights at load.

Reference call chain (arithmetic in third-party `peft`, absent here -- parity of that sub-path is "unpinned",
DESIGN.md): FluxLoraLoaderMixin.lora_state_dict D/loaders/lora_pipeline.py:1618-1743, load_lora_into_transformer
:1821-1861, PeftAdapterMixin.load_lora_adapter D/loaders/peft.py:111-287 (prefix strip :200-204, rank = lora_B.shape[1]
:217-220), get_peft_kwargs D/utils/peft_utils.py:150-192 (lora_alpha = alpha entry or rank).  File format
(D/loaders/lora_base.py:722-757): `transformer.<module path>.lora_A.weight [r, in]`, `.lora_B.weight [out, r]`,
optional `<module path>.alpha`.

PEFT adds B(A(x)) * (alpha / r) at every forward; this engine folds the same update into the weights once:
    W' = W + (alpha / r) * B @ A      (device GEMM through the C ABI, fp32 accumulate, one bf16 rounding of the update)
TextFlux trains alpha = r = 128 (scripts/train_lora.py:527-532), i.e. scale 1.
"""
from __future__ import annotations

import os
from typing import Dict, Optional, Tuple

import torch

from . import ops

BF16 = torch.bfloat16
LORA_WEIGHT_NAME_SAFE = "pytorch_lora_weights.safetensors"


def lora_state_dict(path_or_dict, return_alphas: bool = False, weight_name: Optional[str] = None):
    if isinstance(path_or_dict, dict):
        sd = dict(path_or_dict)
    else:
        from safetensors.torch import load_file
        p = path_or_dict
        if os.path.isdir(p):
            p = os.path.join(p, weight_name or LORA_WEIGHT_NAME_SAFE)
        sd = load_file(p)
    if any("dora_scale" in k for k in sd):  # lora_pipeline.py:1705-1712: DoRA scales are dropped with a warning
        sd = {k: v for k, v in sd.items() if "dora_scale" not in k}
    alphas = {}
    for k in list(sd.keys()):
        if k.endswith(".alpha"):
            alphas[k] = sd.pop(k)
    if any(".lora_down.weight" in k or "lora_unet_" in k or ".processor." in k for k in sd):
        raise NotImplementedError("Kohya / XLabs LoRA formats are out of scope (SURVEY.md §2.2); convert to the diffusers format")
    return (sd, alphas) if return_alphas else sd


def _target_index(transformer) -> Dict[str, Tuple[str, int, int]]:
    """reference module path -> (fused tensor name, row offset, out_features)."""
    D = transformer.inner_dim
    idx = {}
    for key, name, off in transformer._fusion_map():
        rows = transformer.w[name + ".w"].shape[0]
        idx[key] = (name, off, rows)
    # out_features of a target = distance to the next offset inside the fused tensor, or the tensor's end
    by_name: Dict[str, list] = {}
    for key, (name, off, rows) in idx.items():
        by_name.setdefault(name, []).append((off, key))
    out = {}
    for name, lst in by_name.items():
        lst.sort()
        total = transformer.w[name + ".w"].shape[0]
        for i, (off, key) in enumerate(lst):
            end = lst[i + 1][0] if i + 1 < len(lst) else total
            out[key] = (name, off, end - off)
    return out


@torch.no_grad()
def merge_lora_into_transformer(state_dict: Dict[str, torch.Tensor], network_alphas: Optional[Dict[str, torch.Tensor]],
                                transformer, scale: float = 1.0) -> int:
    """Returns the number of merged target modules."""
    prefix = "transformer."
    sd = {k[len(prefix):]: v for k, v in state_dict.items() if k.startswith(prefix)}
    if not sd:
        sd = dict(state_dict)  # already stripped
    alphas = {}
    for k, v in (network_alphas or {}).items():
        k2 = k[len(prefix):] if k.startswith(prefix) else k
        alphas[k2[: -len(".alpha")]] = float(v)
    targets = _target_index(transformer)
    merged = 0
    dev = transformer.device
    modules = sorted({k[: -len(".lora_A.weight")] for k in sd if k.endswith(".lora_A.weight")})
    for mod in modules:
        if mod not in targets:
            raise KeyError(f"LoRA target {mod} is not a Linear of FluxTransformer2DModel")
        A = sd[mod + ".lora_A.weight"].to(dev, BF16)          # [r, in]
        Bm = sd[mod + ".lora_B.weight"].to(dev, BF16)         # [out, r]
        r = Bm.shape[1]
        name, off, rows = targets[mod]
        W = transformer.w[name + ".w"][off:off + rows]
        if Bm.shape[0] != rows or A.shape[1] != W.shape[1] or A.shape[0] != r:
            raise ValueError(f"LoRA shapes for {mod} do not match the target weight {tuple(W.shape)}")
        s = scale * alphas.get(mod, float(r)) / r
        gate = torch.full((W.shape[1],), s, dtype=BF16, device=dev)
        # W[out, in] += s * (B[out, r] @ A[r, in]):   C = res + gate * (a @ w^T) with a = B, w = A^T [in, r]
        ops.gemm(Bm.contiguous(), A.t().contiguous(), None, out=W, epilogue=ops.EPI_BIAS_GATE_RES, gate=gate, res=W)
        merged += 1
    transformer._session = None
    if getattr(transformer, "_adapters", None):     # runtime adapters attached as well: their wide weight copies follow the merge
        transformer._build_lora(transformer._adapters)
    return merged


# ---------------------------------------------------------------------------------------------------- runtime (unmerged) adapters
# The merged path above is the default and costs nothing per step; what it cannot do is change the strength per call, unload or swap
# an adapter (the base value is rounded away in the bf16 sum).  The runtime form keeps the adapter next to the base weight and adds it
# inside the Linear's GEMM (ops.gemm_lora / tfx_gemm_bf16_lora):
#     t = bf16(c * (x @ Acat^T))        c = scale * adapter weight * alpha / r   (ops.gemm, epilogue EPI_COLSCALE, c read at run time)
#     y = epi(x @ W^T + t @ Bcat^T + bias)                                       (one fp32 accumulation, then the Linear's epilogue)
# PEFT rounds more often -- bf16(bf16(bf16(x A^T) B^T) * c) + bf16(x W^T + b) --; as for the merged path, parity with `peft` itself is
# unpinned (it is not installed here), the reference of the tests is the fp32 Linear with the update merged.
RUNTIME_MAX_RANK = 256            # padded rank per fused Linear the GEMM tail takes (ops.LORA_MAX_RANK)


class RuntimePack:
    """Operands of one adapted fused Linear.  Acat [nseg * R, K]: the segments' (zero-padded) A stacked; Bcat [N, R]: row n holds the B
    row of the target that owns output column n; seg_cols / nseg / seg_mask as tfx_lora_args wants them; entries: one
    (adapter name, segment, first column, last column, alpha / r) per (adapter, target) -- what scale_vector() turns into c."""

    def __init__(self, Acat, Bcat, R, seg_cols, nseg, seg_mask, entries):
        self.Acat, self.Bcat, self.R, self.seg_cols, self.nseg, self.seg_mask, self.entries = Acat, Bcat, R, seg_cols, nseg, seg_mask, entries

    def scale_vector(self, weights: Dict[str, float], scale: float = 1.0) -> torch.Tensor:
        """fp32 [nseg * R]: c of every T column at the given adapter weights (an adapter missing from `weights` is inactive: 0) and call
        scale; padded columns 0."""
        c = torch.zeros(self.nseg * self.R, dtype=torch.float32)
        for name, seg, c0, c1, base in self.entries:
            c[seg * self.R + c0:seg * self.R + c1] = scale * float(weights.get(name, 0.0)) * base
        return c


def _strip_prefix(state_dict, network_alphas):
    prefix = "transformer."
    sd = {k[len(prefix):]: v for k, v in state_dict.items() if k.startswith(prefix)}
    if not sd:
        sd = dict(state_dict)  # already stripped
    alphas = {}
    for k, v in (network_alphas or {}).items():
        k2 = k[len(prefix):] if k.startswith(prefix) else k
        alphas[k2[: -len(".alpha")]] = float(v)
    return sd, alphas


def pack_runtime_adapter(adapters, fusion_map, shapes: Dict[str, Tuple[int, int]], max_rank: int = RUNTIME_MAX_RANK) -> Dict[str, RuntimePack]:
    """Pure torch, runs on CPU tensors.  adapters: {adapter name: (lora state dict, alphas or None)} in the format lora_state_dict()
    returns; fusion_map: FluxTransformer2DModel._fusion_map(); shapes: fused tensor name -> (rows, in_features).  Returns
    {fused tensor name: RuntimePack} for every fused Linear that at least one adapter targets.  Several adapters on one target
    concatenate along the rank axis; R = the largest per-segment rank sum, padded to a multiple of 128, at most max_rank."""
    by_name: Dict[str, list] = {}
    where = {}
    for key, name, off in fusion_map:
        by_name.setdefault(name, []).append((off, key))
    for name, lst in by_name.items():
        lst.sort()
        total = shapes[name][0] if name in shapes else None
        for i, (off, key) in enumerate(lst):
            end = lst[i + 1][0] if i + 1 < len(lst) else total
            where[key] = (name, i, off, None if end is None else end - off)
    plan: Dict[str, list] = {}
    for aname, (state_dict, network_alphas) in adapters.items():
        sd, alphas = _strip_prefix(state_dict, network_alphas)
        if any(".lora_down.weight" in k or "lora_unet_" in k or ".processor." in k for k in sd):
            raise NotImplementedError("Kohya / XLabs LoRA formats are out of scope (SURVEY.md §2.2); convert to the diffusers format")
        for mod in sorted({k[: -len(".lora_A.weight")] for k in sd if k.endswith(".lora_A.weight")}):
            if mod not in where:
                raise KeyError(f"LoRA target {mod} is not a Linear of FluxTransformer2DModel")
            name, seg, off, rows = where[mod]
            if not (name[0] in "ds" and name[1:].split(".")[0].isdigit()):
                raise ValueError(f"LoRA target {mod} lies outside the double / single blocks: runtime adapters cover the block Linears "
                                 "only; load this file through the merged path (runtime=False)")
            A, Bm = sd[mod + ".lora_A.weight"], sd[mod + ".lora_B.weight"]
            r = Bm.shape[1]
            if Bm.shape[0] != rows or A.shape[1] != shapes[name][1] or A.shape[0] != r:
                raise ValueError(f"LoRA shapes for {mod} do not match the target weight {(rows, shapes[name][1])}")
            plan.setdefault(name, []).append((aname, seg, off, rows, A, Bm, alphas.get(mod, float(r)) / r, mod))
    packs = {}
    for name, items in plan.items():
        N, K = shapes[name]
        nseg = len(by_name[name])
        seg_cols = by_name[name][1][0] if nseg > 1 else N
        if nseg > 4 or seg_cols % 256 or any(off != i * seg_cols for i, (off, _) in enumerate(by_name[name])):
            raise ValueError(f"{name}: the GEMM tail takes up to 4 segments of equal width, a multiple of 256 columns (got {nseg} of {seg_cols})")
        used = [0] * nseg
        for _, seg, *_rest in items:
            used[seg] += _rest[3].shape[1]
        R = (max(used) + 127) // 128 * 128
        if R > max_rank:
            raise ValueError(f"{name}: rank sum {max(used)} pads to {R} > {max_rank}, the most the runtime path takes per Linear; "
                             "merge some of the adapters (fuse_lora / runtime=False)")
        Acat = torch.zeros(nseg * R, K, dtype=BF16)
        Bcat = torch.zeros(N, R, dtype=BF16)
        fill, entries, mask = [0] * nseg, [], 0
        for aname, seg, off, rows, A, Bm, base, _mod in items:
            r = Bm.shape[1]
            c0 = fill[seg]
            Acat[seg * R + c0:seg * R + c0 + r] = A.to(BF16)
            Bcat[off:off + rows, c0:c0 + r] = Bm.to(BF16)
            entries.append((aname, seg, c0, c0 + r, base))
            fill[seg] += r
            mask |= 1 << seg
        packs[name] = RuntimePack(Acat, Bcat, R, seg_cols, nseg, mask, entries)
    return packs
