"""Torch-tensor front end of the C-ABI kernels (device memory + stream plumbing only, no math here).

Every function enqueues HIP kernels from libtextflux_hip.so on torch's current stream and returns torch
tensors that alias / own the outputs.  Inputs must live on a ROCm device; bf16 unless stated.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import numpy as np
import torch

from . import _lib as L

EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_GATE_RES, EPI_BIAS_RES, EPI_COLSCALE = 0, 1, 2, 3, 4
DEFAULT_ATTENTION = 0      # tfx_set_option("attention_waves", 0): back to the library's default kernel (30 = attn_w4_kernel)
BF16 = torch.bfloat16


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _chk_dev(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("textflux_amd ops need tensors on the ROCm device (no CPU fallback exists)")


def _rows_view(t: torch.Tensor):
    """(ptr, ld, batch_stride, rows_per_batch, batch) of a [.., rows, cols] tensor with unit inner stride."""
    assert t.stride(-1) == 1
    if t.dim() == 2:
        return t.data_ptr(), t.stride(0), 0, t.shape[0], 1
    assert t.dim() == 3
    return t.data_ptr(), t.stride(1), t.stride(0), t.shape[1], t.shape[0]


def gemm(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
         epilogue: int = EPI_BIAS, gelu_from_col: int = 0, gate: Optional[torch.Tensor] = None,
         res: Optional[torch.Tensor] = None, variant: int = -1, workspace: Optional[torch.Tensor] = None,
         cscale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[b] = epi(a[b] @ w.T + bias).  a: [M,K] or [B,M,K] (row/batch strided views allowed), w: [N,K].
    workspace: optional device scratch tensor; lets the auto path split K when the GEMM has fewer tiles than CUs.
    cscale (EPI_COLSCALE): fp32 [N] on the device, out = bf16(cscale * (a @ w.T)), read when the kernel runs."""
    _chk_dev(a, w, bias, out, gate, res, workspace, cscale)
    assert a.dtype == BF16 and w.dtype == BF16 and w.dim() in (2, 3) and w.stride(-1) == 1
    ap, lda, abs_, M, batch = _rows_view(a)
    N, K = w.shape[-2:]
    assert a.shape[-1] == K and (w.dim() == 2 or (a.dim() == 3 and w.shape[0] == batch)), "w [N, K], or [B, N, K] with a [B, M, K]"
    if out is None:
        out = torch.empty(*a.shape[:-1], N, dtype=BF16, device=a.device)
    cp, ldc, cbs, M2, b2 = _rows_view(out)
    assert (M2, b2) == (M, batch) and out.shape[-1] == N
    g = L.GemmArgs()
    g.A, g.lda, g.a_bstride = ap, lda, abs_
    g.W, g.ldw, g.bias = w.data_ptr(), w.stride(-2), _p(bias)
    g.w_bstride = w.stride(0) if w.dim() == 3 else 0
    g.C, g.ldc, g.c_bstride = cp, ldc, cbs
    g.M, g.N, g.K, g.batch = M, N, K, batch
    g.epilogue, g.gelu_from_col = epilogue, gelu_from_col
    if epilogue in (EPI_BIAS_GATE_RES, EPI_BIAS_RES):
        assert res is not None
        if epilogue == EPI_BIAS_GATE_RES:
            assert gate is not None and gate.stride(-1) == 1
            g.gate = gate.data_ptr()
            g.gate_bstride = gate.stride(0) if gate.dim() == 2 else 0
        rp, ldr, rbs, _, _ = _rows_view(res)
        g.res, g.ldr, g.r_bstride = rp, ldr, rbs
    if workspace is not None:
        g.workspace, g.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    if epilogue == EPI_COLSCALE:
        assert cscale is not None and cscale.dtype == torch.float32 and cscale.is_contiguous() and cscale.numel() == N
        g.cscale = cscale.data_ptr()
    L.check(L.lib().tfx_gemm_bf16(C.byref(g), variant, _stream()), "gemm")
    return out


def gemm_qkn(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], norm_q: torch.Tensor, norm_k: torch.Tensor,
             rope_cs: torch.Tensor, q_range, k_range, out: Optional[torch.Tensor] = None, epilogue: int = EPI_BIAS,
             gelu_from_col: int = 0, pos0: int = 0, eps: float = 1e-6, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """tfx_gemm_bf16_qkn: the fused [k | v | q (| mlp)] projection of a FLUX block with the per-head RMSNorm + RoPE of the q / k column
    ranges applied in the GEMM's epilogue (what tfx_dit_forward launches).  rope_cs: fp32 [rows, 64, 2] (cos, sin) pairs."""
    _chk_dev(a, w, bias, out, norm_q, norm_k, rope_cs, workspace)
    assert a.dtype == BF16 and w.dtype == BF16 and w.dim() == 2 and w.stride(1) == 1
    assert norm_q.dtype == norm_k.dtype == BF16 and norm_q.numel() == norm_k.numel() == 128 and rope_cs.dtype == torch.float32 and rope_cs.is_contiguous()
    ap, lda, abs_, M, batch = _rows_view(a)
    N, K = w.shape
    assert a.shape[-1] == K and rope_cs.shape[-2:] == (64, 2)
    rope_bstride = 0
    if rope_cs.dim() == 4:      # [B, rows, 64, 2]: one table per batch sample (tfx_qkn_args.rope_bstride)
        assert rope_cs.shape[0] == batch and rope_cs.shape[1] >= pos0 + M
        rope_bstride = rope_cs.shape[1]
    else:
        assert rope_cs.shape[0] >= pos0 + M
    if out is None:
        out = torch.empty(*a.shape[:-1], N, dtype=BF16, device=a.device)
    cp, ldc, cbs, M2, b2 = _rows_view(out)
    assert (M2, b2) == (M, batch) and out.shape[-1] == N
    g = L.GemmArgs()
    g.A, g.lda, g.a_bstride = ap, lda, abs_
    g.W, g.ldw, g.bias = w.data_ptr(), w.stride(0), _p(bias)
    g.C, g.ldc, g.c_bstride = cp, ldc, cbs
    g.M, g.N, g.K, g.batch = M, N, K, batch
    g.epilogue, g.gelu_from_col = epilogue, gelu_from_col
    if workspace is not None:
        g.workspace, g.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    q = L.QknArgs()
    q.norm_q, q.norm_k, q.rope_cs = norm_q.data_ptr(), norm_k.data_ptr(), rope_cs.data_ptr()
    q.pos0, q.q0, q.q1, q.k0, q.k1, q.eps = pos0, q_range[0], q_range[1], k_range[0], k_range[1], eps
    q.rope_bstride = rope_bstride
    L.check(L.lib().tfx_gemm_bf16_qkn(C.byref(g), C.byref(q), _stream()), "gemm_qkn")
    return out


LORA_MAX_RANK = 256      # padded rank the tail of tfx_gemm_bf16_lora takes (128 or 256)


def lora_operands(x: torch.Tensor, t_cols: int):
    """One allocation [x | T] as tfx_gemm_bf16_lora wants its activations placed: returns (buf, x_view, t_view) with x copied into
    x_view [.., rows, K]; t_view [.., rows, t_cols] (zeros) shares x_view's row pitch max(K, t_cols) and batch stride and lies above it."""
    _chk_dev(x)
    assert x.dtype == BF16 and x.dim() in (2, 3) and t_cols % 8 == 0
    K = x.shape[-1]
    buf = torch.zeros(2, *x.shape[:-1], max(K, t_cols), dtype=BF16, device=x.device)
    buf[0][..., :K].copy_(x)
    return buf, buf[0][..., :K], buf[1][..., :t_cols]


def gemm_lora(a: torch.Tensor, t: torch.Tensor, wb: torch.Tensor, K: int, R: int, seg_cols: int, nseg: int, seg_mask: int,
              bias: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, epilogue: int = EPI_BIAS, gelu_from_col: int = 0,
              gate: Optional[torch.Tensor] = None, res: Optional[torch.Tensor] = None, qkn: Optional[dict] = None,
              split_row: int = 0, second: Optional[dict] = None, t_seg_stride: int = 0) -> torch.Tensor:
    """tfx_gemm_bf16_lora: out[b] = epi(a[b] @ W.T + t[b][:, seg block] @ B.T + bias) in one fp32 accumulation.  wb [N, >= K + R] holds
    W in columns [0, K) and the (zero-padded) up-projection rows B in [K, K + R); t [.., M, nseg * R] shares a's row pitch and batch
    stride and lies above it (lora_operands); t_seg_stride != 0: t [.., M, R] is segment 0's matrix, segment s's lies s * t_seg_stride
    elements above it.  qkn: dict(norm_q, norm_k, rope_cs, q_range, k_range, pos0=0, eps=1e-6) for the fused
    q / k RMSNorm + RoPE epilogue.  split_row / second = dict(wb, bias, gate, norm_q, norm_k): the rows below split_row take the second
    set, which must live above wb within 4 GiB (one allocation)."""
    _chk_dev(a, t, wb, bias, out, gate, res)
    assert a.dtype == BF16 and t.dtype == BF16 and wb.dtype == BF16 and wb.dim() == 2 and wb.stride(1) == 1 and wb.shape[1] >= K + R
    ap, lda, abs_, M, batch = _rows_view(a)
    tp, ldt, tbs, Mt, bt = _rows_view(t)
    assert (ldt, Mt, bt) == (lda, M, batch) and (tbs == abs_ or batch == 1) and a.shape[-1] == K and t.shape[-1] >= (R if t_seg_stride else nseg * R)
    N = wb.shape[0]
    if out is None:
        out = torch.empty(*a.shape[:-1], N, dtype=BF16, device=a.device)
    cp, ldc, cbs, M2, b2 = _rows_view(out)
    assert (M2, b2) == (M, batch) and out.shape[-1] == N
    g = L.GemmArgs()
    g.A, g.lda, g.a_bstride = ap, lda, abs_
    g.W, g.ldw, g.bias = wb.data_ptr(), wb.stride(0), _p(bias)
    g.C, g.ldc, g.c_bstride = cp, ldc, cbs
    g.M, g.N, g.K, g.batch = M, N, K, batch
    g.epilogue, g.gelu_from_col = epilogue, gelu_from_col
    if epilogue in (EPI_BIAS_GATE_RES, EPI_BIAS_RES):
        assert res is not None
        if epilogue == EPI_BIAS_GATE_RES:
            assert gate is not None and gate.stride(-1) == 1
            g.gate = gate.data_ptr()
            g.gate_bstride = gate.stride(0) if gate.dim() == 2 else 0
        rp, ldr, rbs, _, _ = _rows_view(res)
        g.res, g.ldr, g.r_bstride = rp, ldr, rbs
    q = None
    if qkn is not None:
        q = L.QknArgs()
        _chk_dev(qkn["norm_q"], qkn["norm_k"], qkn["rope_cs"])
        assert qkn["rope_cs"].dtype == torch.float32 and qkn["rope_cs"].is_contiguous() and qkn["rope_cs"].shape[0] >= qkn.get("pos0", 0) + M
        q.norm_q, q.norm_k, q.rope_cs = qkn["norm_q"].data_ptr(), qkn["norm_k"].data_ptr(), qkn["rope_cs"].data_ptr()
        q.pos0, q.eps = qkn.get("pos0", 0), qkn.get("eps", 1e-6)
        (q.q0, q.q1), (q.k0, q.k1) = qkn["q_range"], qkn["k_range"]
    l = L.LoraArgs()
    l.T, l.Bm, l.R, l.seg_cols, l.nseg, l.seg_mask, l.t_seg_stride = tp, wb.data_ptr() + 2 * K, R, seg_cols, nseg, seg_mask, t_seg_stride
    if split_row:
        w2 = second["wb"]
        _chk_dev(w2, second.get("bias"), second.get("gate"), second.get("norm_q"), second.get("norm_k"))
        assert w2.dtype == BF16 and w2.shape == wb.shape and w2.stride() == wb.stride()
        l.split_row, l.W2 = split_row, w2.data_ptr()
        l.bias2, l.gate2, l.norm_q2, l.norm_k2 = (_p(second.get(k)) for k in ("bias", "gate", "norm_q", "norm_k"))
    L.check(L.lib().tfx_gemm_bf16_lora(C.byref(g), C.byref(q) if q is not None else None, C.byref(l), _stream()), "gemm_lora")
    return out


def quantize_rows_fp8(x: torch.Tensor, out: Optional[torch.Tensor] = None, scale: Optional[torch.Tensor] = None):
    """Per-row absmax quantisation bf16 -> e4m3 bytes: returns (q uint8 [.., rows, K], scale f32 [.., rows]) with
    x ~= q * scale[..., None];  x [rows, K] or [B, rows, K] (row/batch strided views allowed)."""
    _chk_dev(x, out, scale)
    assert x.dtype == BF16
    xp, ldx, xbs, R, B = _rows_view(x)
    K = x.shape[-1]
    if out is None:
        out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    if scale is None:
        scale = torch.empty(x.shape[:-1], dtype=torch.float32, device=x.device)
    assert out.dtype == torch.uint8 and scale.dtype == torch.float32 and scale.is_contiguous() and out.shape == x.shape
    op, ldo, obs, _, _ = _rows_view(out)
    L.check(L.lib().tfx_quantize_rows_fp8(xp, ldx, xbs, op, ldo, obs, scale.data_ptr(), R if x.dim() == 3 else 0, R, B, K,
                                          _stream()), "quantize_rows_fp8")
    return out, scale


def gemm_fp8(a: torch.Tensor, a_scale: torch.Tensor, w: torch.Tensor, w_scale: torch.Tensor,
             bias: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, epilogue: int = EPI_BIAS,
             gelu_from_col: int = 0, gate: Optional[torch.Tensor] = None, res: Optional[torch.Tensor] = None,
             workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[b] = epi((a[b] @ w.T) * a_scale[b][:, None] * w_scale[None, :] + bias) on e4m3 operands (uint8 storage), bf16 out.
    workspace: optional scratch, enables split-K for few-tile shapes (see gemm)."""
    _chk_dev(a, a_scale, w, w_scale, bias, out, gate, res, workspace)
    assert a.dtype == torch.uint8 and w.dtype == torch.uint8 and w.dim() == 2 and w.stride(1) == 1
    assert a_scale.dtype == torch.float32 and w_scale.dtype == torch.float32 and a_scale.is_contiguous() and w_scale.is_contiguous()
    ap, lda, abs_, M, batch = _rows_view(a)
    N, K = w.shape
    assert a.shape[-1] == K and a_scale.numel() == M * batch and w_scale.numel() == N
    if out is None:
        out = torch.empty(*a.shape[:-1], N, dtype=BF16, device=a.device)
    cp, ldc, cbs, M2, b2 = _rows_view(out)
    assert (M2, b2) == (M, batch) and out.shape[-1] == N and out.dtype == BF16
    g = L.GemmArgs()
    g.A, g.lda, g.a_bstride = ap, lda, abs_
    g.W, g.ldw, g.bias = w.data_ptr(), w.stride(0), _p(bias)
    g.C, g.ldc, g.c_bstride = cp, ldc, cbs
    g.M, g.N, g.K, g.batch = M, N, K, batch
    g.epilogue, g.gelu_from_col = epilogue, gelu_from_col
    if epilogue in (EPI_BIAS_GATE_RES, EPI_BIAS_RES):
        assert res is not None
        if epilogue == EPI_BIAS_GATE_RES:
            assert gate is not None and gate.stride(-1) == 1
            g.gate = gate.data_ptr()
            g.gate_bstride = gate.stride(0) if gate.dim() == 2 else 0
        rp, ldr, rbs, _, _ = _rows_view(res)
        g.res, g.ldr, g.r_bstride = rp, ldr, rbs
    if workspace is not None:
        g.workspace, g.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    L.check(L.lib().tfx_gemm_fp8(C.byref(g), a_scale.data_ptr(), M if batch > 1 else 0, w_scale.data_ptr(), _stream()), "gemm_fp8")
    return out


def ln_modulate(x: torch.Tensor, shift: torch.Tensor, scale: torch.Tensor, out: Optional[torch.Tensor] = None,
                eps: float = 1e-6, split_row: Optional[int] = None, shift2: Optional[torch.Tensor] = None,
                scale2: Optional[torch.Tensor] = None) -> torch.Tensor:
    """LayerNorm(x) * (1 + scale[b]) + shift[b];  x [B,R,D], shift/scale [B,D] (row-strided views allowed).
    split_row: rows < split_row of every sample take (shift2, scale2) instead (tfx_ln_modulate_split: the joint [text | image] rows)."""
    _chk_dev(x, shift, scale, out, shift2, scale2)
    assert x.dim() == 3 and x.dtype == BF16
    if out is None:
        out = torch.empty_like(x)
    xp, ldx, xbs, R, B = _rows_view(x)
    op, ldo, obs, _, _ = _rows_view(out)
    assert shift.stride(-1) == 1 and scale.stride(-1) == 1 and shift.stride(0) == scale.stride(0)
    if split_row is None:
        assert shift2 is None and scale2 is None
        L.check(L.lib().tfx_ln_modulate(xp, ldx, xbs, op, ldo, obs, shift.data_ptr(), scale.data_ptr(), shift.stride(0),
                                        R, B, x.shape[-1], eps, _stream()), "ln_modulate")
        return out
    for t in (shift2, scale2):
        assert t is None or (t.stride(-1) == 1 and t.stride(0) == shift.stride(0))
    L.check(L.lib().tfx_ln_modulate_split(xp, ldx, xbs, op, ldo, obs, shift.data_ptr(), scale.data_ptr(), _p(shift2), _p(scale2),
                                          int(split_row), shift.stride(0), R, B, x.shape[-1], eps, _stream()), "ln_modulate_split")
    return out


def layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """nn.LayerNorm with elementwise affine over the last dim of x [.., D] bf16: one bf16 rounding.  x and out are contiguous, or
    2-D row-strided views [rows, D]."""
    _chk_dev(x, gamma, beta, out)
    assert x.dtype == BF16 and gamma.dtype == BF16 and beta.dtype == BF16
    D = x.shape[-1]
    assert gamma.numel() == D and beta.numel() == D
    if out is None:
        out = torch.empty(x.shape, dtype=BF16, device=x.device)
    assert out.dtype == BF16 and out.shape == x.shape
    ld = [D if t.is_contiguous() else t.stride(0) for t in (x, out)]
    assert all(t.is_contiguous() or (t.dim() == 2 and t.stride(1) == 1) for t in (x, out))
    L.check(L.lib().tfx_layernorm(x.data_ptr(), ld[0], out.data_ptr(), ld[1], gamma.data_ptr(), beta.data_ptr(), x.numel() // D, D, eps,
                                  _stream()), "layernorm")
    return out


def ln_modulate_fp8(x: torch.Tensor, shift: torch.Tensor, scale: torch.Tensor, eps: float = 1e-6,
                    out: Optional[torch.Tensor] = None, scale_out: Optional[torch.Tensor] = None):
    """ln_modulate followed by quantize_rows_fp8 in one pass: returns (q uint8 [B,R,D], scale f32 [B,R]).  out / scale_out: views to
    write them into (out row / batch strided, scale_out batch strided)."""
    _chk_dev(x, shift, scale, out, scale_out)
    assert x.dim() == 3 and x.dtype == BF16
    xp, ldx, xbs, R, B = _rows_view(x)
    D = x.shape[-1]
    q = torch.empty(B, R, D, dtype=torch.uint8, device=x.device) if out is None else out
    qs = torch.empty(B, R, dtype=torch.float32, device=x.device) if scale_out is None else scale_out
    assert q.dtype == torch.uint8 and q.shape == (B, R, D) and q.stride(2) == 1
    assert qs.dtype == torch.float32 and qs.shape == (B, R) and (R == 0 or qs.stride(1) == 1)
    assert shift.stride(-1) == 1 and scale.stride(-1) == 1 and shift.stride(0) == scale.stride(0)
    L.check(L.lib().tfx_ln_modulate_fp8(xp, ldx, xbs, q.data_ptr(), q.stride(1), q.stride(0), qs.data_ptr(), qs.stride(0), shift.data_ptr(),
                                        scale.data_ptr(), shift.stride(0), R, B, D, eps, _stream()), "ln_modulate_fp8")
    return q, qs


def rmsnorm_rope_(buf: torch.Tensor, q_off: int, k_off: int, H: int, T: int, wq_img, wk_img, wq_txt, wk_txt,
                  cos: torch.Tensor, sin: torch.Tensor, eps: float = 1e-6) -> torch.Tensor:
    """In place on buf [B,N,ld]: q at columns q_off.., k at k_off.. (H heads of 128).  cos / sin [N, 128], or [B, N, 128]: one table
    per batch sample (tfx_rmsnorm_rope_batched)."""
    _chk_dev(buf, wq_img, wk_img, wq_txt, wk_txt, cos, sin)
    assert buf.dim() == 3 and buf.dtype == BF16 and cos.dtype == torch.float32 and cos.is_contiguous() and sin.is_contiguous()
    B, N, _ = buf.shape
    if cos.dim() == 3:
        assert cos.shape == (B, N, 128) and sin.shape == cos.shape
        L.check(L.lib().tfx_rmsnorm_rope_batched(buf.data_ptr(), buf.stride(1), buf.stride(0), q_off, k_off, H, N, T, B,
                                                 wq_img.data_ptr(), wk_img.data_ptr(), wq_txt.data_ptr(), wk_txt.data_ptr(),
                                                 cos.data_ptr(), sin.data_ptr(), cos.stride(0), eps, _stream()), "rmsnorm_rope_batched")
        return buf
    assert cos.shape == (N, 128)
    L.check(L.lib().tfx_rmsnorm_rope(buf.data_ptr(), buf.stride(1), buf.stride(0), q_off, k_off, H, N, T, B,
                                     wq_img.data_ptr(), wk_img.data_ptr(), wq_txt.data_ptr(), wk_txt.data_ptr(),
                                     cos.data_ptr(), sin.data_ptr(), eps, _stream()), "rmsnorm_rope")
    return buf


def gate_residual(x: torch.Tensor, gate: torch.Tensor, res: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """res + bf16(gate[:, None, :] * x): x, res [B,R,D] (row / batch strides allowed), gate [B,D] -> out [B,R,D] (tfx_gate_residual;
    `hidden_states + gate.unsqueeze(1) * attn_output`, transformer_flux.py:733-735, 817-818)."""
    _chk_dev(x, gate, res, out)
    assert x.dim() == 3 and x.dtype == res.dtype == gate.dtype == BF16 and res.shape == x.shape
    B, R, D = x.shape
    assert gate.shape == (B, D) and x.stride(2) == res.stride(2) == gate.stride(1) == 1
    if out is None:
        out = torch.empty(B, R, D, dtype=BF16, device=x.device)
    assert out.shape == x.shape and out.dtype == BF16 and out.stride(2) == 1
    L.check(L.lib().tfx_gate_residual(x.data_ptr(), x.stride(1), x.stride(0), gate.data_ptr(), gate.stride(0), res.data_ptr(),
                                      res.stride(1), res.stride(0), out.data_ptr(), out.stride(1), out.stride(0), R, B, D,
                                      _stream()), "gate_residual")
    return out


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: Optional[torch.Tensor] = None,
              scale: Optional[float] = None, score_bound: float = 0.0, workspace: Optional[torch.Tensor] = None,
              seq_len: Optional[torch.Tensor] = None) -> torch.Tensor:
    """q,k,v: [B,N,H*128] (views with row/batch strides allowed) -> out [B,N,H*128].  score_bound: the caller's promise
    |scale * q . k| <= score_bound (0 = unknown), see tfx_attn_args.  workspace: optional device scratch (>= 69.2 MB) that lets the
    kernel deal (item, key tile) units to the CUs (stream-K, tfx_attn_args.workspace).  seq_len: optional device int32 [B], sample b's
    valid length (tfx_attn_args.seq_len): its first seq_len[b] queries attend to its first seq_len[b] keys, later rows of `out` are
    not written."""
    _chk_dev(q, k, v, out, workspace, seq_len)
    B, N, HD = q.shape
    H = HD // 128
    assert HD % 128 == 0 and q.dtype == BF16
    if out is None:
        out = torch.empty(B, N, HD, dtype=BF16, device=q.device)
    a = L.AttnArgs()
    a.q, a.k, a.v, a.o = q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr()
    a.ldq, a.ldk, a.ldv, a.ldo = q.stride(1), k.stride(1), v.stride(1), out.stride(1)
    a.q_bstride, a.k_bstride, a.v_bstride, a.o_bstride = q.stride(0), k.stride(0), v.stride(0), out.stride(0)
    a.B, a.H, a.N = B, H, N
    a.scale = scale if scale is not None else 128 ** -0.5
    a.score_bound = float(score_bound)
    if workspace is not None:
        a.workspace, a.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    if seq_len is not None:
        assert seq_len.dtype == torch.int32 and seq_len.is_contiguous() and seq_len.numel() == B
        a.seq_len = seq_len.data_ptr()
    L.check(L.lib().tfx_joint_attention(C.byref(a), _stream()), "joint_attention")
    return out


def euler_step_(v: torch.Tensor, x: torch.Tensor, coef: torch.Tensor, step: int = 0,
                step_ptr: Optional[torch.Tensor] = None, xin: Optional[torch.Tensor] = None) -> torch.Tensor:
    _chk_dev(v, x, coef, step_ptr, xin)
    if v.dtype != BF16 or x.dtype != BF16 or (xin is not None and xin.dtype != BF16):
        raise TypeError("euler_step_: the HIP scheduler kernels operate on bf16 latents / model outputs")
    assert v.is_contiguous() and x.is_contiguous() and coef.dtype == torch.float32
    Cc = x.shape[-1]
    rows = x.numel() // Cc
    L.check(L.lib().tfx_euler_step(v.data_ptr(), x.data_ptr(), _p(xin), xin.stride(-2) if xin is not None else 0, Cc,
                                   rows, coef.data_ptr(), _p(step_ptr), step, _stream()), "euler_step")
    return x


def amo_step_(v: torch.Tensor, x: torch.Tensor, coef: torch.Tensor, noise: torch.Tensor, step: int = 0,
              step_ptr: Optional[torch.Tensor] = None, xin: Optional[torch.Tensor] = None) -> torch.Tensor:
    _chk_dev(v, x, coef, noise, step_ptr, xin)
    if v.dtype != BF16 or x.dtype != BF16 or (xin is not None and xin.dtype != BF16):
        raise TypeError("amo_step_: the HIP scheduler kernels operate on bf16 latents / model outputs")
    assert v.is_contiguous() and x.is_contiguous() and noise.is_contiguous() and noise.dtype == torch.float32
    Cc = x.shape[-1]
    rows = x.numel() // Cc
    L.check(L.lib().tfx_amo_step(v.data_ptr(), x.data_ptr(), _p(xin), xin.stride(-2) if xin is not None else 0, Cc,
                                 rows, coef.data_ptr(), _p(step_ptr), step, noise.data_ptr(), _stream()), "amo_step")
    return x


def multistep_step_(v: torch.Tensor, x: torch.Tensor, coef: torch.Tensor, v_prev: torch.Tensor, step: int = 0,
                    step_ptr: Optional[torch.Tensor] = None, xin: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Second-order multistep update of x in place (tfx_multistep_step): coef fp32 [n, 2]; v_prev, the previous step's model
    output, is read from step 1 on and holds v afterwards."""
    _chk_dev(v, x, coef, v_prev, step_ptr, xin)
    if v.dtype != BF16 or x.dtype != BF16 or v_prev.dtype != BF16 or (xin is not None and xin.dtype != BF16):
        raise TypeError("multistep_step_: the HIP scheduler kernels operate on bf16 latents / model outputs")
    assert v.is_contiguous() and x.is_contiguous() and v_prev.is_contiguous() and coef.is_contiguous() and coef.dtype == torch.float32
    assert v.numel() == x.numel() == v_prev.numel()
    Cc = x.shape[-1]
    rows = x.numel() // Cc if Cc else 0
    if step_ptr is None and not 0 <= step < coef.numel() // 2:
        raise ValueError(f"multistep_step_: step {step} outside the coefficient table of {coef.numel() // 2} steps")
    L.check(L.lib().tfx_multistep_step(v.data_ptr(), x.data_ptr(), _p(xin), xin.stride(-2) if xin is not None else 0, Cc,
                                       rows, coef.data_ptr(), _p(step_ptr), step, v_prev.data_ptr(), _stream()), "multistep_step")
    return x


def _flat_rows(t: torch.Tensor, name: str):
    """(rows, pitch) of a [.., rows, C] tensor whose rows lie one pitch apart throughout (a contiguous tensor, or a column view of one)"""
    if t.dim() < 2 or t.stride(-1) != 1:
        raise ValueError(f"{name}: needs [.., rows, C] with unit inner stride")
    ld = t.stride(-2)
    rows = 1
    for d in range(t.dim() - 2, -1, -1):
        if t.shape[d] != 1 and t.stride(d) != rows * ld:
            raise ValueError(f"{name}: the rows are not one pitch ({ld}) apart in dimension {d}")
        rows *= t.shape[d]
    return rows, ld


def known_region_blend(x: torch.Tensor, x0: torch.Tensor, noise: torch.Tensor, mask: torch.Tensor, keep_sigma: torch.Tensor,
                       step: int = 0, step_ptr: Optional[torch.Tensor] = None, xin: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x <- (1 - mask) * scale_noise(x0, keep_sigma[step], noise) + mask * x in place, one bf16 rounding per op as the reference's
    tensor ops (tfx_known_region_blend).  x [.., rows, C] may be a column view (row pitch = stride(-2)); x0 / noise / mask contiguous
    of x's shape; keep_sigma fp32 [n], bf16-exact values, a negative entry = x0 itself; xin: the x_embedder input to mirror into."""
    _chk_dev(x, x0, noise, mask, keep_sigma, step_ptr, xin)
    if any(t.dtype != BF16 for t in (x, x0, noise, mask)) or (xin is not None and xin.dtype != BF16):
        raise TypeError("known_region_blend: bf16 latents, noise and mask")
    if keep_sigma.dtype != torch.float32 or not keep_sigma.is_contiguous() or keep_sigma.dim() != 1:
        raise TypeError("known_region_blend: keep_sigma is a contiguous fp32 vector")
    if not (x0.shape == noise.shape == mask.shape == x.shape) or not (x0.is_contiguous() and noise.is_contiguous() and mask.is_contiguous()):
        raise ValueError("known_region_blend: x0, noise and mask must be contiguous and of x's shape")
    Cc = x.shape[-1]
    rows, ldx = _flat_rows(x, "known_region_blend: x")
    ldxin = 0
    if xin is not None:
        rin, ldxin = _flat_rows(xin, "known_region_blend: xin")
        if rin != rows:
            raise ValueError(f"known_region_blend: xin has {rin} rows, x {rows}")
    if step_ptr is None and not 0 <= step < keep_sigma.numel():
        raise ValueError(f"known_region_blend: step {step} outside the sigma table of {keep_sigma.numel()} steps")
    L.check(L.lib().tfx_known_region_blend(x.data_ptr(), ldx, x0.data_ptr(), noise.data_ptr(), mask.data_ptr(), Cc, rows,
                                           keep_sigma.data_ptr(), _p(step_ptr), step, _p(xin), ldxin, _stream()), "known_region_blend")
    return x


def change_map_blend(x: torch.Tensor, x0: torch.Tensor, noise: torch.Tensor, hold: torch.Tensor, cut: torch.Tensor,
                     keep_sigma: torch.Tensor, step: int = 0, step_ptr: Optional[torch.Tensor] = None,
                     xin: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x <- p k + x (1 - k) in place with p = scale_noise(x0, keep_sigma[step], noise) and k = hold[row, col & 3] > cut[step], one bf16
    rounding per op as the reference's tensor ops (tfx_change_map_blend).  x [.., rows, C] may be a column view; x0 / noise contiguous
    of x's shape; hold uint8 [.., rows, 4] contiguous (change_map_pack); cut int32 [n] (schedulers.change_cut_table) and keep_sigma
    fp32 [n] of one length.  cut[step] >= 255 leaves x unwritten; xin, the x_embedder input, is mirrored into either way."""
    _chk_dev(x, x0, noise, hold, cut, keep_sigma, step_ptr, xin)
    if any(t.dtype != BF16 for t in (x, x0, noise)) or (xin is not None and xin.dtype != BF16):
        raise TypeError("change_map_blend: bf16 latents and noise")
    if keep_sigma.dtype != torch.float32 or not keep_sigma.is_contiguous() or keep_sigma.dim() != 1:
        raise TypeError("change_map_blend: keep_sigma is a contiguous fp32 vector")
    if cut.dtype != torch.int32 or not cut.is_contiguous() or cut.shape != keep_sigma.shape:
        raise TypeError("change_map_blend: cut is a contiguous int32 vector of keep_sigma's length")
    if not (x0.shape == noise.shape == x.shape) or not (x0.is_contiguous() and noise.is_contiguous()):
        raise ValueError("change_map_blend: x0 and noise must be contiguous and of x's shape")
    Cc = x.shape[-1]
    rows, ldx = _flat_rows(x, "change_map_blend: x")
    if hold.dtype != torch.uint8 or not hold.is_contiguous() or hold.numel() != rows * 4 or hold.shape[-1] != 4:
        raise ValueError(f"change_map_blend: hold must be contiguous uint8 [.., {rows}, 4]")
    ldxin = 0
    if xin is not None:
        rin, ldxin = _flat_rows(xin, "change_map_blend: xin")
        if rin != rows:
            raise ValueError(f"change_map_blend: xin has {rin} rows, x {rows}")
    if step_ptr is None and not 0 <= step < keep_sigma.numel():
        raise ValueError(f"change_map_blend: step {step} outside the tables of {keep_sigma.numel()} steps")
    L.check(L.lib().tfx_change_map_blend(x.data_ptr(), ldx, x0.data_ptr(), noise.data_ptr(), hold.data_ptr(), cut.data_ptr(), Cc, rows,
                                         keep_sigma.data_ptr(), _p(step_ptr), step, _p(xin), ldxin, _stream()), "change_map_blend")
    return x


def cfg_combine(v_neg: torch.Tensor, v_pos: torch.Tensor, scale: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out <- v_neg + scale * (v_pos - v_neg), one bf16 rounding per op as the reference's tensor ops with a Python float
    (tfx_cfg_combine; true CFG, pipeline_flux_with_cfg.py:808).  v_neg / v_pos bf16 [.., rows, C], contiguous and of one shape; scale:
    a DEVICE fp32 tensor of one element, read when the kernel runs; out: None (a new tensor), v_neg itself (in place) or a contiguous
    tensor of the same shape that overlaps neither input."""
    _chk_dev(v_neg, v_pos, scale, out)
    if out is None:
        out = torch.empty_like(v_neg)
    if any(t.dtype != BF16 for t in (v_neg, v_pos, out)):
        raise TypeError("cfg_combine: bf16 model outputs")
    if scale.dtype != torch.float32 or scale.numel() != 1:
        raise TypeError("cfg_combine: scale is a device fp32 tensor of one element")
    if v_neg.dim() < 1 or not (v_neg.shape == v_pos.shape == out.shape):
        raise ValueError("cfg_combine: v_neg, v_pos and out must be of one shape")
    if not (v_neg.is_contiguous() and v_pos.is_contiguous() and out.is_contiguous()):
        raise ValueError("cfg_combine: v_neg, v_pos and out must be contiguous")
    Cc = v_neg.shape[-1]
    rows = v_neg.numel() // Cc if Cc else 0
    L.check(L.lib().tfx_cfg_combine(v_neg.data_ptr(), v_pos.data_ptr(), out.data_ptr(), Cc, rows, scale.data_ptr(), _stream()), "cfg_combine")
    return out


def x0_predict(x: torch.Tensor, v: torch.Tensor, sigma: torch.Tensor, step: int = 0, step_ptr: Optional[torch.Tensor] = None,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out <- x - sigma[step] * v, one bf16 rounding per op as torch's `latents - sigma * noise_pred` on bf16 tensors with a Python
    float (tfx_x0_predict; DESIGN.md section 4 "Candidates").  x bf16 [.., rows, C] with unit inner stride and one row pitch (a
    contiguous tensor, or a column slice such as xin[:, :, :C] of one); v bf16, contiguous, of x's shape; sigma: a DEVICE fp32
    vector; the step index is step_ptr's word (a device int32 tensor of one element) when given, else `step`."""
    _chk_dev(x, v, sigma, step_ptr, out)
    if out is None:
        out = torch.empty(x.shape, dtype=BF16, device=x.device)
    if any(t.dtype != BF16 for t in (x, v, out)):
        raise TypeError("x0_predict: bf16 latents and model output")
    if sigma.dtype != torch.float32 or sigma.dim() != 1 or not sigma.is_contiguous():
        raise TypeError("x0_predict: sigma is a contiguous device fp32 vector")
    if step_ptr is not None and (step_ptr.dtype != torch.int32 or step_ptr.numel() != 1):
        raise TypeError("x0_predict: step_ptr is a device int32 tensor of one element")
    if x.dim() < 2 or not (x.shape == v.shape == out.shape):
        raise ValueError("x0_predict: x, v and out must be of one shape [.., rows, C]")
    if not (v.is_contiguous() and out.is_contiguous()):
        raise ValueError("x0_predict: v and out must be contiguous")
    Cc = x.shape[-1]
    rows = x.numel() // Cc if Cc else 0
    ldx = x.stride(-2)
    if x.stride(-1) != 1 or any(x.stride(d) != x.stride(d + 1) * x.shape[d + 1] for d in range(x.dim() - 2)):
        raise ValueError("x0_predict: x must have unit inner stride and one row pitch over all its rows")
    if step_ptr is None and not 0 <= int(step) < sigma.numel():
        raise ValueError(f"x0_predict: step {step} outside the table of {sigma.numel()} sigmas")
    L.check(L.lib().tfx_x0_predict(x.data_ptr(), ldx, v.data_ptr(), out.data_ptr(), Cc, rows, sigma.data_ptr(), _p(step_ptr), int(step),
                                   _stream()), "x0_predict")
    return out


def timestep_embedding(t: torch.Tensor) -> torch.Tensor:
    _chk_dev(t)
    t = t.contiguous().float()
    out = torch.empty(t.numel(), 256, dtype=BF16, device=t.device)
    L.check(L.lib().tfx_timestep_embedding(t.data_ptr(), out.data_ptr(), t.numel(), _stream()), "timestep_embedding")
    return out


def silu(a: torch.Tensor) -> torch.Tensor:
    _chk_dev(a)
    a = a.contiguous()
    out = torch.empty_like(a)
    L.check(L.lib().tfx_silu(a.data_ptr(), out.data_ptr(), a.numel(), _stream()), "silu")
    return out


def add(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    _chk_dev(a, b)
    a, b = a.contiguous(), b.contiguous()
    out = torch.empty_like(a)
    L.check(L.lib().tfx_add(a.data_ptr(), b.data_ptr(), out.data_ptr(), a.numel(), _stream()), "add")
    return out


def scatter_cols_(src: torch.Tensor, dst: torch.Tensor, col0: int) -> torch.Tensor:
    """dst[..., col0:col0+C] = src  (src [.., C] contiguous, dst [.., ld] contiguous)."""
    _chk_dev(src, dst)
    assert src.is_contiguous() and dst.is_contiguous()
    Cc = src.shape[-1]
    L.check(L.lib().tfx_scatter_cols(src.data_ptr(), dst.data_ptr(), src.numel() // Cc, Cc, dst.shape[-1], col0,
                                     _stream()), "scatter_cols")
    return dst


def copy_rows_(src: torch.Tensor, dst: torch.Tensor) -> torch.Tensor:
    _chk_dev(src, dst)
    sp, sld, sbs, R, B = _rows_view(src)
    dp, dld, dbs, R2, B2 = _rows_view(dst)
    assert (R, B) == (R2, B2) and src.shape[-1] == dst.shape[-1]
    L.check(L.lib().tfx_copy_rows(sp, sld, sbs, dp, dld, dbs, R, src.shape[-1], B, _stream()), "copy_rows")
    return dst


def select_step_(table: torch.Tensor, cur: torch.Tensor, step_ptr: torch.Tensor) -> None:
    L.check(L.lib().tfx_select_step(table.data_ptr(), cur.data_ptr(), cur.numel(), step_ptr.data_ptr(), _stream()),
            "select_step")


def advance_step_(step_ptr: torch.Tensor) -> None:
    L.check(L.lib().tfx_advance_step(step_ptr.data_ptr(), _stream()), "advance_step")


def prof_enable(on: bool) -> None:
    L.check(L.lib().tfx_prof_enable(1 if on else 0), "prof_enable")


def prof_collect(kind: int):
    """(total kernel ms, total algorithmic FLOPs, launches) of the profiled launches of kind 0 (GEMM) / 1 (attention)."""
    ms, fl, n = C.c_double(), C.c_double(), C.c_int()
    L.check(L.lib().tfx_prof_collect(kind, C.byref(ms), C.byref(fl), C.byref(n)), "prof_collect")
    return ms.value, fl.value, n.value


def mfma_peak_probe(operands: torch.Tensor, fp8: bool = False, seconds: float = 2.5) -> dict:
    """tfx_mfma_peak_probe timed over ~`seconds` with HIP events on the current stream: the rate of an MFMA-only kernel on `operands`
    (bf16, or uint8 holding e4m3 codes) at the board's power cap -- TFLOP/s of the LAST launch of a back-to-back series (the first ones run
    inside the power controller's averaging window at the uncapped clock)."""
    _chk_dev(operands)
    nbytes = operands.numel() * operands.element_size()
    st = _stream()
    fl = C.c_double()

    def launch(ktiles):
        L.check(L.lib().tfx_mfma_peak_probe(operands.data_ptr(), nbytes, 1 if fp8 else 0, ktiles, C.byref(fl), st), "mfma_peak_probe")

    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record(); launch(48 * 64); ev[1].record(); torch.cuda.synchronize()
    per_ktile_ms = ev[0].elapsed_time(ev[1]) / (48 * 64)
    kt = max(48, int(250.0 / max(per_ktile_ms, 1e-6)) // 48 * 48)          # ~0.25 s per launch
    n = max(3, int(seconds / 0.25))
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
    evs[0].record()
    for i in range(n):
        launch(kt)
        evs[i + 1].record()
    torch.cuda.synchronize()
    ms = [evs[i].elapsed_time(evs[i + 1]) for i in range(n)]
    tf = [fl.value / (m * 1e-3) / 1e12 for m in ms]
    return {"tflops": tf[-1], "tflops_first_launch": tf[0], "tflops_min": min(tf), "launches": n, "seconds": sum(ms) * 1e-3,
            "dtype": "e4m3" if fp8 else "bf16", "flops_per_launch": fl.value}


ATTENTION_MODES = ("w4_guarded", "w4_valu_rowsum", "w4_lazy_valu", "w4_lazy", "w4_reference_free", "hp", "w16", "other",
                   "streamk_tail")     # the last: launches (already counted under their kernel form) whose last round was dealt as (item, tile) units


def attention_mode_counts(reset: bool = False) -> dict:
    """Attention launches since the last reset by kernel form (tfx_attention_mode_counts): which stream the score bound selected."""
    c = (C.c_int64 * 9)()
    L.lib().tfx_attention_mode_counts(c, 9, 1 if reset else 0)
    return {name: int(c[i]) for i, name in enumerate(ATTENTION_MODES)}


def release_scratch() -> None:
    """Frees what the library allocated behind optional knobs (today: the attention tail-split partials, one buffer per stream that
    ran with attention_tail_split = 1).  Step graphs captured while the knob was on keep dangling pointers: drop them first."""
    L.check(L.lib().tfx_release_scratch(), "release_scratch")


def set_option(name: str, value: int) -> None:
    L.check(L.lib().tfx_set_option(name.encode(), int(value)), "set_option")


_ZERO_PAGE = {}


def zero_page(device) -> torch.Tensor:
    z = _ZERO_PAGE.get(str(device))
    if z is None:
        z = _ZERO_PAGE[str(device)] = torch.zeros(256, dtype=BF16, device=device)
    return z


def conv3x3_nhwc(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], stride: int = 1, up: int = 1,
                 pad_lo: int = 1, res: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                 variant: int = -1) -> torch.Tensor:
    """x [B, inH, inW, Cin] NHWC bf16, w [Cout, 3, 3, Cin] (KRSC) -> [B, H, W, Cout].  up = 2 folds a nearest 2x upsample
    into the gather; stride = 2, pad_lo = 0 is the VAE downsample (pad (0,1,0,1))."""
    _chk_dev(x, w, bias, res, out)
    assert x.is_contiguous() and w.is_contiguous() and x.dtype == BF16
    B, inH, inW, Cin = x.shape
    Cout = w.shape[0]
    if stride == 1:
        H, W = inH * up, inW * up
    else:
        H, W = (inH * up + pad_lo + 1 - 3) // stride + 1, (inW * up + pad_lo + 1 - 3) // stride + 1
    if out is None:
        out = torch.empty(B, H, W, Cout, dtype=BF16, device=x.device)
    L.check(L.lib().tfx_conv3x3_nhwc(x.data_ptr(), B, inH, inW, Cin, w.data_ptr(), _p(bias), out.data_ptr(), H, W, Cout,
                                     stride, up, pad_lo, _p(res), zero_page(x.device).data_ptr(), variant, _stream()),
            "conv3x3_nhwc")
    return out


def pair_conv_weights(w: torch.Tensor, bias: Optional[torch.Tensor]):
    """[Cout, 3, 3, Cin] (KRSC), [Cout] -> the pixel-pair form of tfx_conv3x3_pair_nhwc: [2 Cout, 3, 4, Cin], [2 Cout]."""
    Cout, _, _, Cin = w.shape
    wp = torch.zeros(2, Cout, 3, 4, Cin, dtype=w.dtype, device=w.device)
    wp[0, :, :, 0:3] = w
    wp[1, :, :, 1:4] = w
    return wp.view(2 * Cout, 3, 4, Cin).contiguous(), (torch.cat([bias, bias]).contiguous() if bias is not None else None)


def conv3x3_pair_nhwc(x: torch.Tensor, w_pair: torch.Tensor, bias_pair: Optional[torch.Tensor], res: Optional[torch.Tensor] = None,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """3 x 3 convolution, stride 1, pad 1, in pixel-pair form (pair_conv_weights): x [B, H, W, Cin], W even -> [B, H, W, Cout]."""
    _chk_dev(x, w_pair, bias_pair, res, out)
    assert x.is_contiguous() and w_pair.is_contiguous() and x.dtype == BF16
    B, H, W, Cin = x.shape
    Cout = w_pair.shape[0] // 2
    if out is None:
        out = torch.empty(B, H, W, Cout, dtype=BF16, device=x.device)
    # the kernel addresses res and out as dense [B, H, W, Cout] (no strides in tfx_conv3x3_pair_nhwc)
    assert out.shape == (B, H, W, Cout) and out.dtype == BF16 and out.is_contiguous()
    assert res is None or (res.shape == (B, H, W, Cout) and res.dtype == BF16 and res.is_contiguous())
    L.check(L.lib().tfx_conv3x3_pair_nhwc(x.data_ptr(), B, H, W, Cin, w_pair.data_ptr(), _p(bias_pair), out.data_ptr(), Cout, _p(res),
                                          zero_page(x.device).data_ptr(), _stream()), "conv3x3_pair_nhwc")
    return out


def blend_edge_nhwc_(a: torch.Tensor, b: torch.Tensor, extent: int, axis: int) -> torch.Tensor:
    """Seam blend of two VAE tiles, in place on b (AutoencoderKL.blend_v: axis 1 = rows, blend_h: axis 2 = columns; a, b NHWC bf16
    views [B, H, W, C]): the first `extent` rows / columns of b fade in from the LAST `extent` of a; extent is clamped to both tiles'
    sizes as the reference does, and the weights use the clamped value."""
    _chk_dev(a, b)
    assert a.dim() == 4 and b.dim() == 4 and a.dtype == b.dtype == BF16 and a.stride(3) == b.stride(3) == 1 and axis in (1, 2)
    other = 3 - axis
    extent = min(a.shape[axis], b.shape[axis], int(extent))
    assert a.shape[0] == b.shape[0] and a.shape[3] == b.shape[3] and a.shape[other] == b.shape[other], "tiles of one row / column line up"
    if extent <= 0:
        return b
    a0 = a.narrow(axis, a.shape[axis] - extent, extent)
    L.check(L.lib().tfx_blend_edge_nhwc(a0.data_ptr(), a0.stride(0), a0.stride(axis), a0.stride(other), b.data_ptr(), b.stride(0),
                                        b.stride(axis), b.stride(other), b.shape[0], extent, b.shape[other], b.shape[3], _stream()),
            "blend_edge_nhwc")
    return b


def groupnorm_nhwc(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, groups: int, silu: bool = True,
                   eps: float = 1e-6, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x [B, ..., C] NHWC bf16 -> GroupNorm(+SiLU)."""
    _chk_dev(x, gamma, beta, out)
    assert x.is_contiguous() and x.dtype == BF16
    B, C = x.shape[0], x.shape[-1]
    HW = x.numel() // (B * C)
    if out is None:
        out = torch.empty_like(x)
    ws = torch.empty(B * ((HW + 1023) // 1024 + 1) * groups * 2, dtype=torch.float32, device=x.device)
    L.check(L.lib().tfx_groupnorm_nhwc(x.data_ptr(), out.data_ptr(), gamma.data_ptr(), beta.data_ptr(), ws.data_ptr(), B,
                                       HW, C, groups, eps, 1 if silu else 0, _stream()), "groupnorm_nhwc")
    return out


# ---------------------------------------------------------------------------------------------------------------------
# pixel / latent layout steps around the VAE (imageops.hip)
_DT = {torch.float32: 0, torch.bfloat16: 1, torch.uint8: 2}


def _dt(t: torch.Tensor) -> int:
    if t.dtype not in _DT:
        raise TypeError(f"unsupported dtype {t.dtype} (float32, bfloat16 or uint8)")
    return _DT[t.dtype]


def any_negative(x: torch.Tensor, flag: Optional[torch.Tensor] = None) -> torch.Tensor:
    """int32 device flag, set when x has a negative element (no host sync)."""
    _chk_dev(x, flag)
    x = x.contiguous()
    if flag is None:
        flag = torch.zeros(1, dtype=torch.int32, device=x.device)
    L.check(L.lib().tfx_any_negative(x.data_ptr(), _dt(x), x.numel(), flag.data_ptr(), _stream()), "any_negative")
    return flag


def prep_image(img: torch.Tensor, mask: Optional[torch.Tensor] = None, norm_mode: int = 0, binarize: bool = True,
               neg_flag: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Encoder input [B, H, W, 8] bf16 NHWC = bf16(norm(img) * (1 - mask)).  img: [B, C, H, W] float32 / bfloat16, or
    [B, H, W, C] uint8 (value / 255); mask: [Bm, 1, H, W] / [Bm, H, W] float32 or uint8, Bm in {1, B}."""
    _chk_dev(img, mask, neg_flag)
    img = img.contiguous()
    if img.dtype == torch.uint8:
        B, H, W, Cc = img.shape
    else:
        B, Cc, H, W = img.shape
    mb = 1
    if mask is not None:
        mask = mask.contiguous()
        mb = mask.shape[0]
        assert mask.numel() == mb * H * W, "mask must be [Bm, 1, H, W] or [Bm, H, W] at the image size"
    out = torch.empty(B, H, W, 8, dtype=BF16, device=img.device)
    L.check(L.lib().tfx_prep_image(img.data_ptr(), _dt(img), _p(mask), _dt(mask) if mask is not None else 0, out.data_ptr(),
                                   B, Cc, H, W, mb, norm_mode, 1 if binarize else 0, _p(neg_flag), _stream()), "prep_image")
    return out


_RESAMPLE_TABLES = {}


def resample_u8(x: torch.Tensor, size) -> torch.Tensor:
    """PIL.Image.resize((W, H)) (BICUBIC, the default) of uint8 [B, H, W, C] images on the device, bit-identical to Pillow:
    horizontal pass, then vertical pass, each rounding to uint8 (tfx_resample_u8)."""
    from .image_processor import pil_resample_tables
    _chk_dev(x)
    assert x.dtype == torch.uint8 and x.dim() == 4 and x.is_contiguous()
    B, H, W, Cc = x.shape
    Ho, Wo = size
    for axis, (n_in, n_out) in ((2, (W, Wo)), (1, (H, Ho))):
        if n_in == n_out:
            continue
        key = (n_in, n_out, str(x.device))
        if key not in _RESAMPLE_TABLES:
            b, k = pil_resample_tables(n_in, n_out)
            _RESAMPLE_TABLES[key] = (torch.from_numpy(b).to(x.device), torch.from_numpy(k).to(x.device))
        b, k = _RESAMPLE_TABLES[key]
        Bc, Hc, Wc, _ = x.shape
        if axis == 2:
            out, outer, inner = torch.empty(Bc, Hc, n_out, Cc, dtype=torch.uint8, device=x.device), Bc * Hc, Cc
        else:
            out, outer, inner = torch.empty(Bc, n_out, Wc, Cc, dtype=torch.uint8, device=x.device), Bc, Wc * Cc
        L.check(L.lib().tfx_resample_u8(x.data_ptr(), out.data_ptr(), b.data_ptr(), k.data_ptr(), k.shape[1], outer, n_in, n_out,
                                        inner, _stream()), "resample_u8")
        x = out
    return x


def rgb_to_grey(x: torch.Tensor) -> torch.Tensor:
    """PIL convert("L") of uint8 [..., 3] -> uint8 [...]."""
    _chk_dev(x)
    assert x.dtype == torch.uint8 and x.shape[-1] == 3 and x.is_contiguous()
    out = torch.empty(x.shape[:-1], dtype=torch.uint8, device=x.device)
    L.check(L.lib().tfx_rgb_to_grey_u8(x.data_ptr(), out.data_ptr(), out.numel(), _stream()), "rgb_to_grey")
    return out


def compose_canvas(glyph: torch.Tensor, scene: torch.Tensor, scene_mask_rgb: torch.Tensor, horizontal: bool = False,
                   mask_rgb: bool = False):
    """uint8 [B, gh, gw, 3] glyph images + [B, sh, sw, 3] scenes + the scenes' RGB masks -> (canvas [B, H, W, 3] u8, mask
    [B, H, W] u8): glyph first (top / left), its mask black, PIL's "L" of the RGB mask elsewhere.  mask_rgb: the mask canvas
    keeps its three channels ([B, H, W, 3]) for a resize before the grey conversion."""
    _chk_dev(glyph, scene, scene_mask_rgb)
    for t in (glyph, scene, scene_mask_rgb):
        assert t.dtype == torch.uint8 and t.dim() == 4 and t.shape[-1] == 3 and t.is_contiguous()
    B, gh, gw, _ = glyph.shape
    _, sh, sw, _ = scene.shape
    assert scene.shape[0] == B and scene_mask_rgb.shape == scene.shape
    H, W = (sh, gw + sw) if horizontal else (gh + sh, sw)
    canvas = torch.empty(B, H, W, 3, dtype=torch.uint8, device=glyph.device)
    cmask = torch.empty((B, H, W, 3) if mask_rgb else (B, H, W), dtype=torch.uint8, device=glyph.device)
    L.check(L.lib().tfx_compose_canvas(glyph.data_ptr(), scene.data_ptr(), scene_mask_rgb.data_ptr(), canvas.data_ptr(),
                                       cmask.data_ptr(), B, gh, gw, sh, sw, 1 if horizontal else 0, 1 if mask_rgb else 0,
                                       _stream()), "compose_canvas")
    return canvas, cmask


def _chk_mask_u8(mask: torch.Tensor, radius: int, what: str):
    _chk_dev(mask)
    if mask.dtype != torch.uint8 or mask.dim() != 3 or not mask.is_contiguous() or mask.numel() == 0:
        raise ValueError(f"{what}: the mask must be a contiguous, non-empty uint8 [B, H, W] tensor, got {mask.dtype} {tuple(mask.shape)}")
    if not 0 <= int(radius) <= 255:
        raise ValueError(f"{what}: radius must be in [0, 255], got {radius}")


def mask_dilate(mask: torch.Tensor, radius: int) -> torch.Tensor:
    """Square max filter of a uint8 mask [B, H, W]: the maximum over the (2 radius + 1)^2 window, clipped at the image border
    (tfx_mask_dilate_u8).  radius 0 copies."""
    _chk_mask_u8(mask, radius, "mask_dilate")
    out, tmp = torch.empty_like(mask), torch.empty_like(mask)
    B, H, W = mask.shape
    L.check(L.lib().tfx_mask_dilate_u8(mask.data_ptr(), out.data_ptr(), tmp.data_ptr(), B, H, W, int(radius), _stream()), "mask_dilate")
    return out


def mask_feather(mask: torch.Tensor, radius: int) -> torch.Tensor:
    """Three box passes of width 2 radius + 1 along x, then three along y, over a uint8 mask [B, H, W]; edge replicated, every pass
    rounded to uint8 (tfx_mask_feather_u8).  radius 0 copies."""
    _chk_mask_u8(mask, radius, "mask_feather")
    out, tmp = torch.empty_like(mask), torch.empty_like(mask)
    B, H, W = mask.shape
    L.check(L.lib().tfx_mask_feather_u8(mask.data_ptr(), out.data_ptr(), tmp.data_ptr(), B, H, W, int(radius), _stream()), "mask_feather")
    return out


def overlay(orig: torch.Tensor, edit: torch.Tensor, alpha: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(orig (255 - alpha) + edit alpha + 127) // 255 of uint8 images [B, H, W, C] under a uint8 alpha [B, H, W] (tfx_overlay_u8).
    out: None (a new tensor) or `orig` itself."""
    _chk_dev(orig, edit, alpha, out)
    for t in (orig, edit, alpha):
        if t.dtype != torch.uint8 or not t.is_contiguous():
            raise ValueError("overlay: orig, edit and alpha must be contiguous uint8 tensors")
    if orig.dim() != 4 or orig.numel() == 0 or edit.shape != orig.shape or alpha.shape != orig.shape[:3]:
        raise ValueError(f"overlay: orig / edit [B, H, W, C] and alpha [B, H, W] must agree, got {tuple(orig.shape)}, {tuple(edit.shape)}, "
                         f"{tuple(alpha.shape)}")
    if out is None:
        out = torch.empty_like(orig)
    elif out.shape != orig.shape or out.dtype != torch.uint8 or not out.is_contiguous():
        raise ValueError("overlay: out must be a contiguous uint8 tensor of orig's shape")
    B, H, W, Cc = orig.shape
    L.check(L.lib().tfx_overlay_u8(orig.data_ptr(), edit.data_ptr(), alpha.data_ptr(), out.data_ptr(), B, H, W, Cc, _stream()), "overlay")
    return out


MASKED_MOMENTS_SCRATCH_BYTES = 34816     # include/textflux_hip.h: TFX_MASKED_MOMENTS_SCRATCH_BYTES, per sample


def masked_moments(a: torch.Tensor, b: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    """int64 [B, C, 5] = (n, sum a, sum b, sum a a, sum a b) per sample and channel over the pixels whose weight is not 0, of uint8 images
    a, b [B, H, W, C] (C in 1..4) under a uint8 weight [B, H, W] (tfx_masked_moments_u8).  Exact: integer sums, 64-bit throughout."""
    _chk_dev(a, b, weight)
    for t in (a, b, weight):
        if t.dtype != torch.uint8 or not t.is_contiguous():
            raise ValueError("masked_moments: a, b and weight must be contiguous uint8 tensors")
    if a.dim() != 4 or a.numel() == 0 or not 1 <= a.shape[3] <= 4 or b.shape != a.shape or weight.shape != a.shape[:3]:
        raise ValueError(f"masked_moments: a / b [B, H, W, C <= 4] and weight [B, H, W] must agree, got {tuple(a.shape)}, {tuple(b.shape)}, "
                         f"{tuple(weight.shape)}")
    B, H, W, Cc = a.shape
    out = torch.empty(B, Cc, 5, dtype=torch.int64, device=a.device)
    scratch = torch.empty(B * MASKED_MOMENTS_SCRATCH_BYTES // 8, dtype=torch.int64, device=a.device)
    L.check(L.lib().tfx_masked_moments_u8(a.data_ptr(), b.data_ptr(), weight.data_ptr(), out.data_ptr(), scratch.data_ptr(),
                                          scratch.numel() * 8, B, H, W, Cc, _stream()), "masked_moments")
    return out


def overlay_lut(orig: torch.Tensor, edit: torch.Tensor, alpha: torch.Tensor, lut: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ops.overlay with the edit sent through a per-sample, per-channel table first: (orig (255 - alpha) + lut[b, c, edit] alpha + 127) // 255
    of uint8 images [B, H, W, C] (C in 1..4) under a uint8 alpha [B, H, W], lut uint8 [B, C, 256] (tfx_overlay_lut_u8).
    out: None (a new tensor) or `orig` itself."""
    _chk_dev(orig, edit, alpha, lut, out)
    for t in (orig, edit, alpha, lut):
        if t.dtype != torch.uint8 or not t.is_contiguous():
            raise ValueError("overlay_lut: orig, edit, alpha and lut must be contiguous uint8 tensors")
    if orig.dim() != 4 or orig.numel() == 0 or not 1 <= orig.shape[3] <= 4 or edit.shape != orig.shape or alpha.shape != orig.shape[:3]:
        raise ValueError(f"overlay_lut: orig / edit [B, H, W, C <= 4] and alpha [B, H, W] must agree, got {tuple(orig.shape)}, "
                         f"{tuple(edit.shape)}, {tuple(alpha.shape)}")
    B, H, W, Cc = orig.shape
    if tuple(lut.shape) != (B, Cc, 256):
        raise ValueError(f"overlay_lut: lut must be [{B}, {Cc}, 256], got {tuple(lut.shape)}")
    if out is None:
        out = torch.empty_like(orig)
    elif out.shape != orig.shape or out.dtype != torch.uint8 or not out.is_contiguous():
        raise ValueError("overlay_lut: out must be a contiguous uint8 tensor of orig's shape")
    L.check(L.lib().tfx_overlay_lut_u8(orig.data_ptr(), edit.data_ptr(), alpha.data_ptr(), lut.data_ptr(), out.data_ptr(), B, H, W, Cc,
                                       _stream()), "overlay_lut")
    return out


def seamless_overlay(orig: torch.Tensor, ref: torch.Tensor, edit: torch.Tensor, alpha: torch.Tensor, covered: Optional[torch.Tensor] = None,
                     lut: Optional[torch.Tensor] = None, smooth: int = 8, max_shift: int = 32, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ops.overlay_lut (ops.overlay without a table) with a membrane added to the edit first (tfx_seamless_overlay_u8; DESIGN.md section 4
    "Seamless paste"): the difference ref - lut[edit], known where alpha == 0 (and covered != 0 when given), is interpolated across
    alpha's support by a pull-push pyramid, smoothed by `smooth` Jacobi sweeps and clamped to +- max_shift grey levels.  uint8 images
    orig, ref, edit [B, H, W, C] (C in 1..4; ref may be orig), uint8 alpha and covered [B, H, W], lut uint8 [B, C, 256].  Exact: integer
    arithmetic.  out: None (a new tensor) or `orig` itself."""
    _chk_dev(orig, ref, edit, alpha, covered, lut, out)
    for t in (orig, ref, edit, alpha, covered, lut):
        if t is not None and (t.dtype != torch.uint8 or not t.is_contiguous()):
            raise ValueError("seamless_overlay: orig, ref, edit, alpha, covered and lut must be contiguous uint8 tensors")
    if (orig.dim() != 4 or orig.numel() == 0 or not 1 <= orig.shape[3] <= 4 or edit.shape != orig.shape or ref.shape != orig.shape
            or alpha.shape != orig.shape[:3] or (covered is not None and covered.shape != alpha.shape)):
        raise ValueError(f"seamless_overlay: orig / ref / edit [B, H, W, C <= 4] and alpha / covered [B, H, W] must agree, got {tuple(orig.shape)}, "
                         f"{tuple(ref.shape)}, {tuple(edit.shape)}, {tuple(alpha.shape)}" + ("" if covered is None else f", {tuple(covered.shape)}"))
    B, H, W, Cc = orig.shape
    if lut is not None and tuple(lut.shape) != (B, Cc, 256):
        raise ValueError(f"seamless_overlay: lut must be [{B}, {Cc}, 256], got {tuple(lut.shape)}")
    if not (0 <= int(smooth) <= 255 and 0 <= int(max_shift) <= 255):
        raise ValueError(f"seamless_overlay: smooth and max_shift must be in [0, 255], got {smooth}, {max_shift}")
    if out is None:
        out = torch.empty_like(orig)
    elif out.shape != orig.shape or out.dtype != torch.uint8 or not out.is_contiguous():
        raise ValueError("seamless_overlay: out must be a contiguous uint8 tensor of orig's shape")
    need = L.lib().tfx_seamless_workspace_bytes(B, H, W, Cc)
    L.check(1 if need < 0 else 0, "seamless_overlay")
    ws = torch.empty((need + 7) // 8, dtype=torch.int64, device=orig.device)
    ptr = lambda t: None if t is None else t.data_ptr()
    L.check(L.lib().tfx_seamless_overlay_u8(orig.data_ptr(), ref.data_ptr(), edit.data_ptr(), alpha.data_ptr(), ptr(covered), ptr(lut),
                                            out.data_ptr(), ws.data_ptr(), ws.numel() * 8, B, H, W, Cc, int(smooth), int(max_shift),
                                            _stream()), "seamless_overlay")
    return out


HIGHPASS_BINS = 1024                     # include/textflux_hip.h: tfx_highpass_hist_u8's bins per (sample, channel)
GRAIN_SIGMA0 = math.sqrt(4 * (256 ** 2 - 1) / 12)      # standard deviation of tfx_grain_u8's n: the sum of four uniform bytes, 147.8005


def highpass_hist(img: torch.Tensor, sel: torch.Tensor, lo: int = 255, hi: int = 255, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """int32 [B, C, 1024]: per sample and channel the histogram of v = |16 p - sum w p'|, w = [1 2 1] x [1 2 1] over the edge-replicated
    3 x 3 neighbourhood, over the pixels of a uint8 image [B, H, W, C] (C in 1..4) whose uint8 sel [B, H, W] lies in [lo, hi]; v of 1023
    and above shares the last bin (tfx_highpass_hist_u8).  Exact: integer counts.  out: None (a new tensor) or an int32 [B, C, 1024]
    tensor, which the call zeroes itself."""
    out = _hist_args("highpass_hist", img, sel, lo, hi, 0, out)
    B, H, W, Cc = img.shape
    L.check(L.lib().tfx_highpass_hist_u8(img.data_ptr(), sel.data_ptr(), int(lo), int(hi), out.data_ptr(), B, H, W, Cc, _stream()),
            "highpass_hist")
    return out


def highpass_hist_step(img: torch.Tensor, sel: torch.Tensor, lo: int = 255, hi: int = 255, step: int = 1,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """int32 [B, C + 1, 1024] (tfx_highpass_hist_step_u8): rows 0..C-1 are highpass_hist's with the eight neighbours taken at distance
    `step` in 1..8 (the a-trous form; step 1: highpass_hist itself, bit for bit), row C is the histogram of |sum over the channels of the
    signed residuals| over the same pixels.  Exact: integer counts.  out: None (a new tensor) or an int32 [B, C + 1, 1024] tensor, which
    the call zeroes itself."""
    if int(step) != step or not 1 <= int(step) <= 8:
        raise ValueError(f"highpass_hist_step: step must be an integer in 1..8, got {step}")
    out = _hist_args("highpass_hist_step", img, sel, lo, hi, 1, out)
    B, H, W, Cc = img.shape
    L.check(L.lib().tfx_highpass_hist_step_u8(img.data_ptr(), sel.data_ptr(), int(lo), int(hi), int(step), out.data_ptr(), B, H, W, Cc,
                                              _stream()), "highpass_hist_step")
    return out


def _hist_args(name, img, sel, lo, hi, extra_rows, out):
    """The checks both histograms make before they launch -> out (made when None): int32 [B, C + extra_rows, 1024]."""
    _chk_dev(img, sel, out)
    for t in (img, sel):
        if t.dtype != torch.uint8 or not t.is_contiguous():
            raise ValueError(f"{name}: img and sel must be contiguous uint8 tensors")
    if img.dim() != 4 or img.numel() == 0 or not 1 <= img.shape[3] <= 4 or sel.shape != img.shape[:3]:
        raise ValueError(f"{name}: img [B, H, W, C <= 4] and sel [B, H, W] must agree, got {tuple(img.shape)}, {tuple(sel.shape)}")
    if not (0 <= int(lo) <= 255 and 0 <= int(hi) <= 255):
        raise ValueError(f"{name}: lo and hi must be in [0, 255], got {lo}, {hi}")
    B, rows = img.shape[0], img.shape[3] + extra_rows
    if out is None:
        out = torch.empty(B, rows, HIGHPASS_BINS, dtype=torch.int32, device=img.device)
    elif tuple(out.shape) != (B, rows, HIGHPASS_BINS) or out.dtype != torch.int32 or not out.is_contiguous():
        raise ValueError(f"{name}: out must be a contiguous int32 [{B}, {rows}, {HIGHPASS_BINS}] tensor")
    return out


def grain(img: torch.Tensor, alpha: torch.Tensor, gain, origin=None, seed: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Hashed white grain added to a uint8 image [B, H, W, C] (C in 1..4) under a uint8 alpha [B, H, W] (tfx_grain_u8): per byte
    clamp(img + floor((n gain[b, c] alpha + 255 * 32768) / (255 * 65536)), 0, 255), n in [-510, 510] a hash of the pixel's scene position,
    channel and seed with standard deviation GRAIN_SIGMA0.  gain: integers [B, C] (a host array or a tensor) = sigma / GRAIN_SIGMA0 in
    Q16, each in [0, 65536]; origin: None, (x, y), or integers [B, 2]: the scene position of the window's top-left pixel (taken modulo
    2^32); seed: taken modulo 2^32.  alpha == 0 leaves a byte unchanged and gain == 0 copies.  Exact: integer arithmetic.
    out: None (a new tensor) or `img` itself."""
    g, o, out = _grain_args("grain", img, alpha, gain, 65536, origin, out)
    B, H, W, Cc = img.shape
    gd = torch.from_numpy(g).to(img.device)
    L.check(L.lib().tfx_grain_u8(img.data_ptr(), alpha.data_ptr(), gd.data_ptr(), _p(o), int(seed) % 2 ** 32, out.data_ptr(), B, H, W, Cc,
                                 _stream()), "grain")
    return out


GRAIN_MAX_BLUR, GRAIN_MAX_GAIN = 64, 2 ** 18      # tfx_grain_shaped_u8: the largest s, and the largest gain (blurred grain is weaker)


def grain_shaped(img: torch.Tensor, alpha: torch.Tensor, gain, shape, origin=None, seed: int = 0,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """grain() with the noise correlated over neighbouring pixels and over the channels (tfx_grain_shaped_u8): per byte
    clamp(img + floor((f gain[b, c] alpha + 255 * 2^39) / (255 * 2^40)), 0, 255), f the [s, 256 - 2 s, s] x [s, 256 - 2 s, s] blur, over
    SCENE positions, of (256 - lam) n(x, y, c) + lam n(x, y, 255).  shape: integers [B, 2] or (s, lam), s in [0, 64] and lam in [0, 256];
    gain: as grain's, each in [0, 2^18]; origin, seed, out: as grain's.  (s, lam) = (0, 0) with gains up to 65536 is grain(), bit for
    bit; the grain of a scene pixel does not depend on the window.  Exact: integer arithmetic."""
    g, o, out = _grain_args("grain_shaped", img, alpha, gain, GRAIN_MAX_GAIN, origin, out)
    B, H, W, Cc = img.shape
    sh = np.asarray(shape.cpu() if isinstance(shape, torch.Tensor) else shape)
    if sh.dtype.kind not in "iu" or sh.shape not in ((2,), (B, 2)):
        raise ValueError(f"grain_shaped: shape must be integers (s, lam) or [{B}, 2], got {sh.dtype} {sh.shape}")
    sh = np.ascontiguousarray(np.broadcast_to(sh, (B, 2)).astype(np.int64))
    if sh.min() < 0 or sh[:, 0].max() > GRAIN_MAX_BLUR or sh[:, 1].max() > 256:
        raise ValueError(f"grain_shaped: s must be in [0, {GRAIN_MAX_BLUR}] and lam in [0, 256], got {sh.tolist()}")
    gd, sd = torch.from_numpy(g).to(img.device), torch.from_numpy(sh.astype(np.int32)).to(img.device)
    L.check(L.lib().tfx_grain_shaped_u8(img.data_ptr(), alpha.data_ptr(), gd.data_ptr(), sd.data_ptr(), _p(o), int(seed) % 2 ** 32,
                                        out.data_ptr(), B, H, W, Cc, _stream()), "grain_shaped")
    return out


def _grain_args(name, img, alpha, gain, max_gain, origin, out):
    """The checks both grains make before they launch -> (gain as a contiguous int32 host array [B, C], origin as an int32 device tensor
    [B, 2] or None, out (made when None))."""
    _chk_dev(img, alpha, out)
    for t in (img, alpha):
        if t.dtype != torch.uint8 or not t.is_contiguous():
            raise ValueError(f"{name}: img and alpha must be contiguous uint8 tensors")
    if img.dim() != 4 or img.numel() == 0 or not 1 <= img.shape[3] <= 4 or alpha.shape != img.shape[:3]:
        raise ValueError(f"{name}: img [B, H, W, C <= 4] and alpha [B, H, W] must agree, got {tuple(img.shape)}, {tuple(alpha.shape)}")
    B, H, W, Cc = img.shape
    g = np.asarray(gain.cpu() if isinstance(gain, torch.Tensor) else gain)
    if g.shape != (B, Cc) or g.dtype.kind not in "iu":
        raise ValueError(f"{name}: gain must be integers [{B}, {Cc}], got {g.dtype} {g.shape}")
    if g.min() < 0 or g.max() > max_gain:
        raise ValueError(f"{name}: every gain must be in [0, {max_gain}], got [{int(g.min())}, {int(g.max())}]")
    o = None
    if origin is not None:
        o = np.asarray(origin.cpu() if isinstance(origin, torch.Tensor) else origin)
        if o.dtype.kind not in "iu" or o.shape not in ((2,), (B, 2)):
            raise ValueError(f"{name}: origin must be integers (x, y) or [{B}, 2], got {o.dtype} {o.shape}")
        o = np.broadcast_to(o.astype(np.int64), (B, 2))
        o = torch.from_numpy((((o + 2 ** 31) % 2 ** 32) - 2 ** 31).astype(np.int32)).to(img.device)
    if out is None:
        out = torch.empty_like(img)
    elif out.shape != img.shape or out.dtype != torch.uint8 or not out.is_contiguous():
        raise ValueError(f"{name}: out must be a contiguous uint8 tensor of img's shape")
    return np.ascontiguousarray(g.astype(np.int32)), o, out


def change_metric(a: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 [B, H, W]: how much two uint8 images [B, H, W, C] (C in 1..4) differ around a pixel (tfx_change_metric_u8): the largest, over
    the channels, of (|s_c| + 8) >> 4 with s_c the [1 2 1] x [1 2 1] sum of a - b over the edge-replicated 3 x 3 neighbourhood.  0 where
    the images agree on the neighbourhood, |k| where they differ by the constant k.  Exact: integer arithmetic.  out: None (a new tensor)
    or a uint8 [B, H, W] tensor that is neither a nor b."""
    _chk_dev(a, b, out)
    for t in (a, b):
        if t.dtype != torch.uint8 or not t.is_contiguous():
            raise ValueError("change_metric: a and b must be contiguous uint8 tensors")
    if a.dim() != 4 or a.numel() == 0 or not 1 <= a.shape[3] <= 4 or b.shape != a.shape:
        raise ValueError(f"change_metric: a and b [B, H, W, C <= 4] must agree, got {tuple(a.shape)}, {tuple(b.shape)}")
    B, H, W, Cc = a.shape
    if out is None:
        out = torch.empty(B, H, W, dtype=torch.uint8, device=a.device)
    elif tuple(out.shape) != (B, H, W) or out.dtype != torch.uint8 or not out.is_contiguous():
        raise ValueError(f"change_metric: out must be a contiguous uint8 [{B}, {H}, {W}] tensor")
    L.check(L.lib().tfx_change_metric_u8(a.data_ptr(), b.data_ptr(), out.data_ptr(), B, H, W, Cc, _stream()), "change_metric")
    return out


def hysteresis(m: torch.Tensor, lo: int, hi: int, rounds: bool = False):
    """uint8 [B, H, W] in {0, 255} (tfx_hysteresis_u8): 255 exactly on the pixels of a uint8 field m [B, H, W] with m >= lo that an
    8-connected path of such pixels, inside the same sample, joins to a pixel with m >= hi; 0 <= lo <= hi <= 256 (hi = 256: all 0,
    hi = 0: all 255).  The launch is repeated until a round marks nothing: the call synchronises the current stream once per round and is
    refused while that stream is capturing.  rounds=True: (the result, the number of rounds, at least 1)."""
    _chk_dev(m)
    if m.dtype != torch.uint8 or m.dim() != 3 or not m.is_contiguous() or m.numel() == 0:
        raise ValueError(f"hysteresis: m must be a contiguous, non-empty uint8 [B, H, W] tensor, got {m.dtype} {tuple(m.shape)}")
    if int(lo) != lo or int(hi) != hi or not 0 <= int(lo) <= int(hi) <= 256:
        raise ValueError(f"hysteresis: lo and hi must be integers with 0 <= lo <= hi <= 256, got {lo}, {hi}")
    B, H, W = m.shape
    need = L.lib().tfx_hysteresis_workspace_bytes(B, H, W)
    L.check(1 if need < 0 else 0, "hysteresis")
    out = torch.empty_like(m)
    ws = torch.empty((need + 7) // 8, dtype=torch.int64, device=m.device)
    n = C.c_int32(0)
    L.check(L.lib().tfx_hysteresis_u8(m.data_ptr(), out.data_ptr(), int(lo), int(hi), ws.data_ptr(), ws.numel() * 8, C.byref(n), B, H, W,
                                      _stream()), "hysteresis")
    return (out, int(n.value)) if rounds else out


_WARP_TAPS = {}


def _warp_u8(name: str, x: torch.Tensor, out_size, coverage: bool, shape_map):
    """The line warps' common part: the checks of x and out_size, the tap table and the call of tfx_<name>.  shape_map(B, out_h, out_w)
    -> (the map as an int64 tensor whose leading axis is B, expanded where one map serves the batch; the arguments between the map
    and the tap table): the caller's own checks, the host-side magnitude check among them."""
    _chk_dev(x)
    if x.dtype != torch.uint8 or x.dim() != 4 or not x.is_contiguous() or x.numel() == 0 or not 1 <= x.shape[3] <= 4:
        raise ValueError(f"{name}: x must be a contiguous, non-empty uint8 [B, H, W, C <= 4] tensor, got {x.dtype} {tuple(x.shape)}")
    B, H, W, Cc = x.shape
    Ho, Wo = (int(v) for v in out_size)
    if Ho < 1 or Wo < 1:
        raise ValueError(f"{name}: out_size must be (out_h, out_w) with both at least 1, got {tuple(out_size)}")
    m, extra = shape_map(B, Ho, Wo)
    m = m.to(x.device).contiguous()
    key = str(x.device)
    if key not in _WARP_TAPS:
        from .rectify import catmull_rom_taps
        _WARP_TAPS[key] = torch.from_numpy(catmull_rom_taps()).to(x.device)
    taps = _WARP_TAPS[key]
    out = torch.empty(B, Ho, Wo, Cc, dtype=torch.uint8, device=x.device)
    cov = torch.empty(B, Ho, Wo, dtype=torch.uint8, device=x.device) if coverage else None
    L.check(getattr(L.lib(), "tfx_" + name)(x.data_ptr(), out.data_ptr(), _p(cov), B, H, W, Cc, Ho, Wo, m.data_ptr(), *extra,
                                            taps.data_ptr(), _stream()), name)
    return (out, cov) if coverage else out


def _warp_matrix_u8(name: str, n: int, x: torch.Tensor, m, out_size, coverage: bool, host_check=None):
    """warp_affine_u8 / warp_perspective_u8: _warp_u8 with n matrix entries per sample.  host_check(matrices [k, n] as a host array,
    out_h, out_w): applied when m arrives as a host array."""
    def shape_map(B, Ho, Wo):
        host, t = None, m
        if not isinstance(m, torch.Tensor):
            import numpy as np
            host = np.ascontiguousarray(m)
            t = torch.from_numpy(host)
        if t.dtype != torch.int64 or t.numel() not in (n, n * B) or t.shape[-1] != n:
            raise ValueError(f"{name}: m must be int64 [{B}, {n}] or [{n}], got {t.dtype} {tuple(t.shape)}")
        if host is not None and host_check is not None:
            host_check(host.reshape(-1, n), Ho, Wo)
        return t.reshape(-1, n).expand(B, n), ()
    return _warp_u8(name, x, out_size, coverage, shape_map)


def warp_affine_u8(x: torch.Tensor, m, out_size, coverage: bool = False):
    """uint8 [B, H, W, C] (C in 1..4) -> [B, out_h, out_w, C]: every destination pixel (i, j) is x[b] sampled at its Q16 affine image
    under m (int64 [B, 6] or [6], tensor or array: one matrix per sample, or one for all), 4 x 4 Catmull-Rom taps, edge replicated, in
    integer arithmetic (tfx_warp_affine_u8; include/textflux_hip.h has the arithmetic, rectify.matrices builds m).  out_size =
    (out_h, out_w).  coverage: also return uint8 [B, out_h, out_w], 255 where the sample position lies inside the image."""
    return _warp_matrix_u8("warp_affine_u8", 6, x, m, out_size, coverage)


GATHER_COLS = 10                    # warp_affine_gather_u8's table row: (b, m0..m5, out_h, out_w, byte offset)


def warp_affine_gather_u8(images: torch.Tensor, table, out: Optional[torch.Tensor] = None, refused: Optional[torch.Tensor] = None,
                          blocks_per_crop: int = 64):
    """Every crop of `table` in one launch (tfx_warp_affine_gather_u8; DESIGN.md section 4 "Candidates") -> (out, refused).  images uint8
    [B, H, W, C] (C in 1..4), contiguous.  table int64 [n, 10], a host array or a device tensor, one row per crop: (b, m0..m5 Q16, out_h,
    out_w, byte offset); crop k is warp_affine_u8(images[b], m, (out_h, out_w)) bit for bit, written as [out_h, out_w, C] at its byte
    offset of the packed uint8 vector `out` -- the layout ocr_resize_norm reads; offsets are byte-granular.  out: None = a new vector as
    long as the host table's furthest crop end (a device table needs `out`).  refused: a device int32 tensor of one element the kernel adds
    1 to for every row it cannot serve (b outside [0, B), a non-positive side, a byte range outside out) and then leaves unwritten; None =
    a fresh zero.  blocks_per_crop: the workgroups that share a crop's tiles; the bytes do not depend on it."""
    _chk_dev(images, out, refused)
    if images.dtype != torch.uint8 or images.dim() != 4 or not images.is_contiguous() or images.numel() == 0 or not 1 <= images.shape[3] <= 4:
        raise ValueError(f"warp_affine_gather_u8: images must be a contiguous, non-empty uint8 [B, H, W, C <= 4] tensor, got {images.dtype} "
                         f"{tuple(images.shape)}")
    B, H, W, Cc = images.shape
    host = None
    if not isinstance(table, torch.Tensor):
        import numpy as np
        host = np.ascontiguousarray(table)
        table = torch.from_numpy(host)
    if table.dtype != torch.int64 or table.dim() != 2 or table.shape[1] != GATHER_COLS:
        raise ValueError(f"warp_affine_gather_u8: table must be int64 [n, {GATHER_COLS}], got {table.dtype} {tuple(table.shape)}")
    n = table.shape[0]
    if out is None:
        if host is None:
            raise ValueError("warp_affine_gather_u8: a device table needs `out`")
        ends = [int(r[9]) + int(r[7]) * int(r[8]) * Cc for r in host.tolist() if r[7] > 0 and r[8] > 0 and r[9] >= 0]
        out = torch.empty(max(ends, default=0), dtype=torch.uint8, device=images.device)
    elif out.dtype != torch.uint8 or out.dim() != 1 or not out.is_contiguous():
        raise ValueError("warp_affine_gather_u8: out must be a contiguous uint8 vector")
    if refused is None:
        refused = torch.zeros(1, dtype=torch.int32, device=images.device)
    elif refused.dtype != torch.int32 or refused.numel() != 1:
        raise ValueError("warp_affine_gather_u8: refused must be a device int32 tensor of one element")
    if int(blocks_per_crop) != blocks_per_crop or not 1 <= int(blocks_per_crop) <= 65535:
        raise ValueError(f"warp_affine_gather_u8: blocks_per_crop must be an integer in 1..65535, got {blocks_per_crop!r}")
    table = table.to(images.device).contiguous()
    _chk_dev(table)
    key = str(images.device)
    if key not in _WARP_TAPS:
        from .rectify import catmull_rom_taps
        _WARP_TAPS[key] = torch.from_numpy(catmull_rom_taps()).to(images.device)
    if n and out.numel():
        L.check(L.lib().tfx_warp_affine_gather_u8(images.data_ptr(), out.data_ptr(), out.numel(), table.data_ptr(), n, refused.data_ptr(), B,
                                                  H, W, Cc, int(blocks_per_crop), _WARP_TAPS[key].data_ptr(), _stream()),
                "warp_affine_gather_u8")
    elif n:                              # an empty out has no address to hand over: every row is refused, as the kernel would
        refused += n
    return out, refused


def _perspective_magnitudes(m, out_h: int, out_w: int) -> None:
    """tfx_warp_perspective_u8's magnitude contract, in Python integers: the three forms are linear in (i, j), so over the destination
    their extremes lie at its four corner pixels.  D <= 0 is allowed (defined: the pixel is 0 and uncovered)."""
    lim = 1 << 54
    for row in m.tolist():
        for i, j in ((0, 0), (out_w - 1, 0), (0, out_h - 1), (out_w - 1, out_h - 1)):
            nx, ny, d = (row[k] * i + row[k + 1] * j + row[k + 2] for k in (0, 3, 6))
            if abs(nx) >= lim or abs(ny) >= lim or d >= lim:
                raise ValueError(f"warp_perspective_u8: |Nx|, |Ny| and D must stay below 2^54 over the destination; at pixel ({i}, {j}) "
                                 f"they are {nx}, {ny}, {d}")


def warp_perspective_u8(x: torch.Tensor, m, out_size, coverage: bool = False):
    """warp_affine_u8 under a homography: every destination pixel (i, j) is x[b] sampled at (Nx / D, Ny / D) with Nx = m0 i + m1 j + m2,
    Ny = m3 i + m4 j + m5, D = m6 i + m7 j + m8 (m int64 [B, 9] or [9], tensor or array), the quotients floored to 8 fractional bits;
    a pixel with D <= 0 is 0 and uncovered (tfx_warp_perspective_u8; include/textflux_hip.h has the arithmetic, perspective.matrices
    builds m).  A host array is checked against the magnitude contract (|Nx|, |Ny|, D < 2^54 at the destination's corners: ValueError);
    a device tensor is taken as it is, which is memory-safe but leaves such pixels undefined."""
    return _warp_matrix_u8("warp_perspective_u8", 9, x, m, out_size, coverage, _perspective_magnitudes)


GRID_NONE = -(1 << 63)               # warp_grid_u8: a node whose x is this marks "no source" (INT64_MIN)


def _grid_magnitudes(grid) -> None:
    """tfx_warp_grid_u8's magnitude contract on a host grid: every value is the marker or below 2^50 in magnitude."""
    bad = (grid != GRID_NONE) & ((grid >= 1 << 50) | (grid <= -(1 << 50)))
    if bad.any():
        raise ValueError(f"warp_grid_u8: every grid value must be the marker or below 2^50 in magnitude; {int(bad.sum())} are not")


def warp_grid_u8(x: torch.Tensor, grid, shift: int, out_size, coverage: bool = False):
    """warp_affine_u8 under a control grid, and the general remap (shift = 0): every destination pixel (i, j) is x[b] sampled at the
    bilinear blend of the four grid nodes around it.  grid: int64 [gh, gw, 2] (one grid for the batch) or [B, gh, gw, 2], a device tensor
    or a host array, gh = ((out_h - 1) >> shift) + 2, gw = ((out_w - 1) >> shift) + 2; node (r, q) is the Q16 source position (x, y) of
    destination pixel (q << shift, r << shift); shift in 0..5.  A pixel one of whose four nodes has x = GRID_NONE is 0 and uncovered
    (tfx_warp_grid_u8; include/textflux_hip.h has the arithmetic, curve.grids builds the grids).  A host grid is checked against the
    magnitude contract (every value the marker or below 2^50 in magnitude: ValueError); a device tensor is taken as it is, which is
    memory-safe but leaves such pixels undefined."""
    def shape_map(B, Ho, Wo):
        if isinstance(shift, bool) or int(shift) != shift or not 0 <= int(shift) <= 5:
            raise ValueError(f"warp_grid_u8: shift must be an integer in 0..5, got {shift!r}")
        sh = int(shift)
        gh, gw = ((Ho - 1) >> sh) + 2, ((Wo - 1) >> sh) + 2
        host, g = None, grid
        if not isinstance(grid, torch.Tensor):
            import numpy as np
            host = np.ascontiguousarray(grid)
            if host.dtype != np.int64:
                raise ValueError(f"warp_grid_u8: grid must be int64, got {host.dtype}")
            g = torch.from_numpy(host)
        if g.dtype != torch.int64 or tuple(g.shape) not in ((gh, gw, 2), (B, gh, gw, 2)):
            raise ValueError(f"warp_grid_u8: grid must be int64 [{gh}, {gw}, 2] or [{B}, {gh}, {gw}, 2] for out_size {(Ho, Wo)} at shift {sh}, "
                             f"got {g.dtype} {tuple(g.shape)}")
        if host is not None:
            _grid_magnitudes(host)
        return g.reshape(-1, gh, gw, 2).expand(B, gh, gw, 2), (sh,)
    return _warp_u8("warp_grid_u8", x, out_size, coverage, shape_map)


def pack_mask(mask: torch.Tensor, out: torch.Tensor, col0: int, B: int, H: int, W: int, binarize: bool = True) -> torch.Tensor:
    """out[b, :, col0 : col0 + 256] = packed mask (out: [B, S, ld] bf16)."""
    _chk_dev(mask, out)
    mask = mask.contiguous()
    mb = mask.shape[0]
    assert mask.numel() == mb * H * W and out.dtype == BF16 and out.is_contiguous()
    L.check(L.lib().tfx_pack_mask(mask.data_ptr(), _dt(mask), out.data_ptr(), B, H, W, mb, 1 if binarize else 0,
                                  out.shape[-1], col0, _stream()), "pack_mask")
    return out


KEEP_MODES = {"nearest": 0, "cover": 1}


def keep_mask_pack(mask_u8: torch.Tensor, C: int = 64, mode="nearest", grow: int = 0) -> torch.Tensor:
    """uint8 pixel mask [B, H, W] -> the packed latent mask of known-region sampling, bf16 [B, (H/16)(W/16), C] of 1.0 / 0.0
    (tfx_keep_mask_pack).  mode "nearest" (0): the reference's F.interpolate, grow must be 0; "cover" (1): a latent pixel is masked
    when anything >= 128 lies in its 8x8 block or in those of its `grow` neighbours (0..8)."""
    _chk_dev(mask_u8)
    if mask_u8.dtype != torch.uint8 or mask_u8.dim() != 3:
        raise TypeError("keep_mask_pack: the mask is uint8 [B, H, W]")
    mode = KEEP_MODES.get(mode, mode)
    mask_u8 = mask_u8.contiguous()
    B, H, W = mask_u8.shape
    if H % 16 or W % 16:
        raise ValueError(f"keep_mask_pack: H and W must be multiples of 16, got {H} x {W}")
    out = torch.empty(B, (H // 16) * (W // 16), C, dtype=BF16, device=mask_u8.device)
    L.check(L.lib().tfx_keep_mask_pack(mask_u8.data_ptr(), out.data_ptr(), B, H, W, C, int(mode), int(grow), _stream()), "keep_mask_pack")
    return out


def change_map_pack(map_u8: torch.Tensor, mode="nearest", grow: int = 0) -> torch.Tensor:
    """uint8 change map [B, H, W] (255 = free from the first step, 0 = never changes) -> the hold bytes of change-map sampling, uint8
    [B, (H/16)(W/16), 4] = 255 - map per latent pixel of each token's 2x2 patch (tfx_change_map_pack).  mode "nearest" (0): the map at
    every 8th pixel, the reference's F.interpolate, grow must be 0; "cover" (1): the maximum of the map over the latent pixel's 8x8
    block and those of its `grow` neighbours (0..8)."""
    _chk_dev(map_u8)
    if map_u8.dtype != torch.uint8 or map_u8.dim() != 3:
        raise TypeError("change_map_pack: the map is uint8 [B, H, W]")
    mode = KEEP_MODES.get(mode, mode)
    map_u8 = map_u8.contiguous()
    B, H, W = map_u8.shape
    if H % 16 or W % 16:
        raise ValueError(f"change_map_pack: H and W must be multiples of 16, got {H} x {W}")
    out = torch.empty(B, (H // 16) * (W // 16), 4, dtype=torch.uint8, device=map_u8.device)
    L.check(L.lib().tfx_change_map_pack(map_u8.data_ptr(), out.data_ptr(), B, H, W, int(mode), int(grow), _stream()), "change_map_pack")
    return out


def vae_sample_pack(moments: torch.Tensor, eps: Optional[torch.Tensor], out: torch.Tensor, col0: int, shift: float,
                    scale: float) -> torch.Tensor:
    """moments [B, h, w, 2L] NHWC bf16, eps [B, L, h, w] (None: the mode) -> out[b, :, col0 : col0 + 4L]."""
    _chk_dev(moments, eps, out)
    B, h, w, L2 = moments.shape
    assert moments.is_contiguous() and moments.dtype == BF16 and out.dtype == BF16 and out.is_contiguous()
    if eps is not None:
        eps = eps.contiguous()
        assert eps.shape == (B, L2 // 2, h, w)
    L.check(L.lib().tfx_vae_sample_pack(moments.data_ptr(), _p(eps), _dt(eps) if eps is not None else 1, out.data_ptr(), B, h,
                                        w, L2 // 2, shift, scale, out.shape[-1], col0, _stream()), "vae_sample_pack")
    return out


def unpack_latents(lat: torch.Tensor, h: int, w: int, shift: float, scale: float) -> torch.Tensor:
    """lat [B, (h/2)(w/2), 4L] bf16 -> z [B, h, w, L] NHWC bf16 = lat / scale + shift."""
    _chk_dev(lat)
    assert lat.dtype == BF16 and lat.stride(-1) == 1 and lat.dim() == 3
    B, S, C4 = lat.shape
    assert S == (h // 2) * (w // 2) and lat.stride(0) == S * lat.stride(1)
    out = torch.empty(B, h, w, C4 // 4, dtype=BF16, device=lat.device)
    L.check(L.lib().tfx_unpack_latents(lat.data_ptr(), lat.stride(1), out.data_ptr(), B, h, w, C4 // 4, shift, scale,
                                       _stream()), "unpack_latents")
    return out


def postprocess(x: torch.Tensor, C: int, mode: str, denorm: bool = True, crop=None) -> torch.Tensor:
    """x [B, H, W, Cs] NHWC bf16 -> "pt": [B, C, H, W] bf16 | "np": [B, H, W, C] f32 | "u8": [B, H, W, C] uint8 |
    "pt32": [B, C, H, W] f32; crop = (left, top, right, bottom) in pixels keeps only that window (PIL box convention)."""
    _chk_dev(x)
    assert x.is_contiguous() and x.dtype == BF16
    B, H, W, Cs = x.shape
    x0, y0, x1, y1 = crop if crop is not None else (0, 0, W, H)
    Hc, Wc = y1 - y0, x1 - x0
    code = {"pt": 0, "np": 1, "u8": 2, "pt32": 3}[mode]
    if code in (0, 3):
        out = torch.empty(B, C, Hc, Wc, dtype=BF16 if code == 0 else torch.float32, device=x.device)
    else:
        out = torch.empty(B, Hc, Wc, C, dtype=torch.float32 if code == 1 else torch.uint8, device=x.device)
    L.check(L.lib().tfx_postprocess(x.data_ptr(), out.data_ptr(), B, H, W, Cs, C, code, 1 if denorm else 0, y0, x0, Hc, Wc,
                                    _stream()), "postprocess")
    return out


def transpose(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[B, N, C] -> [B, C, N] (bf16)."""
    _chk_dev(x, out)
    assert x.dim() == 3 and x.dtype == BF16 and x.stride(-1) == 1
    B, N, Cc = x.shape
    if out is None:
        out = torch.empty(B, Cc, N, dtype=BF16, device=x.device)
    L.check(L.lib().tfx_transpose(x.data_ptr(), x.stride(1), x.stride(0), out.data_ptr(), out.stride(1), out.stride(0), N, Cc,
                                  B, _stream()), "transpose")
    return out


def row_softmax(s: torch.Tensor, scale: float, out: torch.Tensor) -> torch.Tensor:
    """out[:, :N] = bf16(softmax(scale * s)) over the last dim; s [R, N] fp32 (row-strided), out [R, >= N] bf16."""
    _chk_dev(s, out)
    assert s.dim() == 2 and s.dtype == torch.float32 and s.stride(1) == 1
    assert out.dim() == 2 and out.dtype == BF16 and out.stride(1) == 1 and out.shape[0] == s.shape[0] and out.shape[1] >= s.shape[1]
    L.check(L.lib().tfx_row_softmax(s.data_ptr(), s.stride(0), out.data_ptr(), out.stride(0), s.shape[0], s.shape[1], scale,
                                    _stream()), "row_softmax")
    return out


def gemm_f32(a: torch.Tensor, w: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[b] = a[b] @ w.T as fp32 raw accumulators (no bias / epilogue).  a [M, K] or [B, M, K] bf16, w [N, K] bf16,
    out [.., M, N] fp32 (row-strided views allowed)."""
    _chk_dev(a, w, out)
    assert a.dtype == BF16 and w.dtype == BF16 and w.dim() in (2, 3) and w.stride(-1) == 1
    ap, lda, abs_, M, batch = _rows_view(a)
    N, K = w.shape[-2:]
    assert a.shape[-1] == K and (w.dim() == 2 or (a.dim() == 3 and w.shape[0] == batch)), "w [N, K], or [B, N, K] with a [B, M, K]"
    if out is None:   # rows padded to a multiple of 4 floats (16-byte aligned vector stores)
        out = torch.empty(*a.shape[:-1], (N + 3) // 4 * 4, dtype=torch.float32, device=a.device)[..., :N]
    assert out.dtype == torch.float32
    cp, ldc, cbs, M2, b2 = _rows_view(out)
    assert (M2, b2) == (M, batch) and out.shape[-1] == N
    g = L.GemmArgs()
    g.A, g.lda, g.a_bstride = ap, lda, abs_
    g.W, g.ldw, g.bias = w.data_ptr(), w.stride(-2), None
    g.w_bstride = w.stride(0) if w.dim() == 3 else 0
    g.C, g.ldc, g.c_bstride = cp, ldc, cbs
    g.M, g.N, g.K, g.batch = M, N, K, batch
    g.epilogue = EPI_BIAS
    L.check(L.lib().tfx_gemm_bf16_f32(C.byref(g), _stream()), "gemm_f32")
    return out


# ---------------------------------------------------------------------------------------------------------------------
# text-encoder kernels (textenc.hip)
def attention64(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: float, rel_bias: Optional[torch.Tensor] = None,
                causal: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """q, k, v: [B, N, H*64] bf16 (row / batch strided views allowed), N <= 512 -> [B, N, H*64].  rel_bias: fp32 [H, 2N-1]
    indexed by key - query + N - 1 (T5); causal: keys after the query masked (CLIP)."""
    _chk_dev(q, k, v, rel_bias, out)
    B, N, HD = q.shape
    H = HD // 64
    assert HD % 64 == 0 and q.dtype == BF16
    if rel_bias is not None:
        assert rel_bias.dtype == torch.float32 and rel_bias.is_contiguous() and rel_bias.shape == (H, 2 * N - 1)
    if out is None:
        out = torch.empty(B, N, HD, dtype=BF16, device=q.device)
    a = L.AttnArgs()
    a.q, a.k, a.v, a.o = q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr()
    a.ldq, a.ldk, a.ldv, a.ldo = q.stride(1), k.stride(1), v.stride(1), out.stride(1)
    a.q_bstride, a.k_bstride, a.v_bstride, a.o_bstride = q.stride(0), k.stride(0), v.stride(0), out.stride(0)
    a.B, a.H, a.N, a.scale = B, H, N, scale
    L.check(L.lib().tfx_attention64(C.byref(a), _p(rel_bias), 1 if causal else 0, _stream()), "attention64")
    return out


def rmsnorm(x: torch.Tensor, w: torch.Tensor, eps: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """T5LayerNorm over the last dim of x [rows, D] (fp32 or bf16) -> bf16."""
    _chk_dev(x, w, out)
    assert x.dim() == 2 and x.stride(1) == 1 and w.dtype == BF16 and x.dtype in (torch.float32, BF16)
    if out is None:
        out = torch.empty(x.shape, dtype=BF16, device=x.device)
    L.check(L.lib().tfx_rmsnorm(x.data_ptr(), 0 if x.dtype == torch.float32 else 1, x.stride(0), w.data_ptr(), out.data_ptr(),
                                out.stride(0), x.shape[0], x.shape[1], eps, _stream()), "rmsnorm")
    return out


def gather_rows(table: torch.Tensor, ids: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _chk_dev(table, ids, out)
    assert table.dtype == BF16 and table.is_contiguous() and ids.dtype == torch.int64
    ids = ids.contiguous().view(-1)
    if out is None:
        out = torch.empty(ids.numel(), table.shape[1], dtype=BF16, device=table.device)
    assert out.dtype == BF16 and out.shape == (ids.numel(), table.shape[1]) and out.is_contiguous()
    L.check(L.lib().tfx_gather_rows(table.data_ptr(), ids.data_ptr(), out.data_ptr(), ids.numel(), table.shape[1],
                                    table.shape[0], _stream()), "gather_rows")
    return out


def add_into_f32_(x32: torch.Tensor, y: torch.Tensor, assign: bool = False) -> torch.Tensor:
    _chk_dev(x32, y)
    assert x32.dtype == torch.float32 and x32.is_contiguous() and y.is_contiguous() and y.numel() == x32.numel()
    mode = 2 if assign else (0 if y.dtype == BF16 else 1)
    assert y.dtype in (BF16, torch.float32) and not (assign and y.dtype != BF16)
    L.check(L.lib().tfx_add_into_f32(x32.data_ptr(), y.data_ptr(), x32.numel(), mode, _stream()), "add_into_f32")
    return x32


def _act_out(a: torch.Tensor, out: Optional[torch.Tensor]) -> torch.Tensor:
    if out is None:
        return torch.empty(a.shape, dtype=BF16, device=a.device)
    assert out.dtype == BF16 and out.shape == a.shape and out.stride(1) == 1
    return out


def mul(a: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """a * b for bf16 [rows, cols] row-strided views."""
    _chk_dev(a, b, out)
    assert a.dim() == 2 and a.shape == b.shape and a.stride(1) == 1 and b.stride(1) == 1 and a.dtype == BF16
    out = _act_out(a, out)
    L.check(L.lib().tfx_mul_act(a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), out.data_ptr(), out.stride(0), a.shape[0],
                                a.shape[1], 0, _stream()), "mul")
    return out


def quick_gelu(a: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _chk_dev(a, out)
    assert a.dim() == 2 and a.stride(1) == 1 and a.dtype == BF16
    out = _act_out(a, out)
    L.check(L.lib().tfx_mul_act(a.data_ptr(), a.stride(0), None, 0, out.data_ptr(), out.stride(0), a.shape[0], a.shape[1], 1,
                                _stream()), "quick_gelu")
    return out


# ---- read-back: the fp32 NHWC kernels of the text recogniser and the CTC decode / loss (ocr.hip) --------------------------------------
OCR_ACTS = {None: 0, "none": 0, "relu": 1, "hard_swish": 2, "hard_sigmoid": 3, "swish": 4}
F32 = torch.float32


def _chk_f32(*ts):
    _chk_dev(*ts)
    for t in ts:
        if t is not None and (t.dtype != F32 or not t.is_contiguous()):
            raise RuntimeError("the read-back kernels take contiguous fp32 tensors")


def ocr_resize_norm(packed: torch.Tensor, table: torch.Tensor, img_h: int, img_w: int) -> torch.Tensor:
    """packed u8 line crops ([h, w, 3] each) + table int32 [n, 4] = (byte offset, h, w, turn) -> fp32 [n, img_h, img_w, 3]."""
    _chk_dev(packed, table)
    assert packed.dtype == torch.uint8 and packed.dim() == 1 and packed.is_contiguous()
    assert table.dtype == torch.int32 and table.dim() == 2 and table.shape[1] == 4 and table.is_contiguous()
    n = table.shape[0]
    out = torch.empty(n, img_h, img_w, 3, dtype=F32, device=packed.device)
    L.check(L.lib().tfx_ocr_resize_norm(packed.data_ptr(), packed.numel(), table.data_ptr(), out.data_ptr(), n, img_h, img_w, _stream()),
            "ocr_resize_norm")
    return out


def _conv_out(size: int, k: int, s: int) -> int:
    return (size + 2 * (k // 2) - k) // s + 1


def ocr_conv_f32(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], stride=(1, 1), act=None, cin: Optional[int] = None,
                 out: Optional[torch.Tensor] = None, co_off: int = 0) -> torch.Tensor:
    """x [B, H, W, >= cin] fp32 (the first cin channels are read), w [Cout, k, k, cin], k in (1, 3) -> act(conv + bias) written to
    out[..., co_off : co_off + Cout] (a fresh [B, Ho, Wo, Cout] when out is None)."""
    _chk_f32(x, w, bias, out)
    assert x.dim() == 4 and w.dim() == 4 and w.shape[1] == w.shape[2]
    B, H, W, ldx = x.shape
    Cout, k, _, Cin = w.shape
    assert (cin or ldx) == Cin and Cin <= ldx and (bias is None or bias.shape == (Cout,))
    Ho, Wo = _conv_out(H, k, stride[0]), _conv_out(W, k, stride[1])
    if out is None:
        out = torch.empty(B, Ho, Wo, Cout, dtype=F32, device=x.device)
    assert out.shape[:3] == (B, Ho, Wo) and out.shape[3] >= co_off + Cout
    L.check(L.lib().tfx_ocr_conv_f32(x.data_ptr(), w.data_ptr(), _p(bias), out.data_ptr(), B, H, W, Cin, Cout, k, stride[0], stride[1],
                                     OCR_ACTS[act], ldx, out.shape[3], co_off, _stream()), "ocr_conv_f32")
    return out


def ocr_linear(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], act=None) -> torch.Tensor:
    """x [M, K] fp32, w [N, K] -> act(x w^T + bias) [M, N]: the 1 x 1 case of ocr_conv_f32."""
    assert x.dim() == 2 and w.dim() == 2
    M, K = x.shape
    return ocr_conv_f32(x.view(M, 1, 1, K), w.view(w.shape[0], 1, 1, K), bias, act=act).view(M, w.shape[0])


def ocr_conv_dw(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], stride=(1, 1), act=None) -> torch.Tensor:
    """depthwise: x [B, H, W, C] fp32, w [k, k, C], k in (3, 5) -> act(conv + bias), act None or 'hard_swish'."""
    _chk_f32(x, w, bias)
    assert x.dim() == 4 and w.dim() == 3 and w.shape[0] == w.shape[1] and w.shape[2] == x.shape[3]
    B, H, W, Cc = x.shape
    k = w.shape[0]
    out = torch.empty(B, _conv_out(H, k, stride[0]), _conv_out(W, k, stride[1]), Cc, dtype=F32, device=x.device)
    L.check(L.lib().tfx_ocr_conv_dw(x.data_ptr(), w.data_ptr(), _p(bias), out.data_ptr(), B, H, W, Cc, k, stride[0], stride[1],
                                    OCR_ACTS[act], _stream()), "ocr_conv_dw")
    return out


def ocr_pool_mean(x: torch.Tensor) -> torch.Tensor:
    """x [B, H, W, C] fp32 -> the mean over (H, W), [B, C]."""
    _chk_f32(x)
    B, H, W, Cc = x.shape
    out = torch.empty(B, Cc, dtype=F32, device=x.device)
    L.check(L.lib().tfx_ocr_pool(x.data_ptr(), out.data_ptr(), B, H, W, Cc, 0, Cc, _stream()), "ocr_pool")
    return out


def ocr_pool_2x2(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x [B, H, W, C] fp32 -> the 2 x 2 stride-2 average written to out[..., :C] (a fresh [B, H // 2, W // 2, C] when out is None)."""
    _chk_f32(x, out)
    B, H, W, Cc = x.shape
    if out is None:
        out = torch.empty(B, H // 2, W // 2, Cc, dtype=F32, device=x.device)
    assert out.shape[:3] == (B, H // 2, W // 2) and out.shape[3] >= Cc
    L.check(L.lib().tfx_ocr_pool(x.data_ptr(), out.data_ptr(), B, H, W, Cc, 1, out.shape[3], _stream()), "ocr_pool")
    return out


def ocr_scale_channels(x: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """x [B, H, W, C] * s [B, C] (fp32)."""
    _chk_f32(x, s)
    B, H, W, Cc = x.shape
    assert s.shape == (B, Cc)
    out = torch.empty_like(x)
    L.check(L.lib().tfx_ocr_scale_channels(x.data_ptr(), s.data_ptr(), out.data_ptr(), B, H * W, Cc, _stream()), "ocr_scale_channels")
    return out


def ocr_layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float) -> torch.Tensor:
    """nn.LayerNorm over the last dim of fp32 rows [rows, D]."""
    _chk_f32(x, gamma, beta)
    assert x.dim() == 2 and gamma.shape == beta.shape == (x.shape[1],)
    out = torch.empty_like(x)
    L.check(L.lib().tfx_ocr_layernorm(x.data_ptr(), x.shape[1], out.data_ptr(), x.shape[1], gamma.data_ptr(), beta.data_ptr(), x.shape[0],
                                      x.shape[1], eps, _stream()), "ocr_layernorm")
    return out


def ocr_add_(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """x += y on fp32 tensors (the residual add of the neck's blocks): the fp32 mode of tfx_add_into_f32."""
    _chk_f32(x, y)
    return add_into_f32_(x, y)


def ocr_attention(qkv: torch.Tensor, heads: int) -> torch.Tensor:
    """qkv fp32 [B, N, 3 * heads * d] -> softmax((q d^-0.5) k^T) v as [B, N, heads * d]."""
    _chk_f32(qkv)
    B, N, three = qkv.shape
    d = three // (3 * heads)
    assert three == 3 * heads * d
    out = torch.empty(B, N, heads * d, dtype=F32, device=qkv.device)
    L.check(L.lib().tfx_ocr_attention(qkv.data_ptr(), out.data_ptr(), B, N, heads, d, float(d) ** -0.5, _stream()), "ocr_attention")
    return out


def ctc_rows(logits: torch.Tensor):
    """logits fp32 [..., C] -> (max fp32, first argmax int32, log-sum-exp fp32), each of shape logits.shape[:-1]."""
    _chk_f32(logits)
    Cc = logits.shape[-1]
    rows = logits.numel() // Cc
    mx = torch.empty(logits.shape[:-1], dtype=F32, device=logits.device)
    arg = torch.empty(logits.shape[:-1], dtype=torch.int32, device=logits.device)
    lse = torch.empty_like(mx)
    L.check(L.lib().tfx_ctc_rows(logits.data_ptr(), Cc, rows, Cc, mx.data_ptr(), arg.data_ptr(), lse.data_ptr(), _stream()), "ctc_rows")
    return mx, arg, lse


def ctc_score(logits: torch.Tensor, row_arg: torch.Tensor, row_lse: torch.Tensor, targets=None):
    """logits fp32 [n, T, C] with ctc_rows' outputs -> (ids int32 [n, T], time_index int32 [n, T], count int32 [n], loss fp32 [n] or None);
    targets: one list of class ids per sample (None: decode only)."""
    _chk_f32(logits, row_lse)
    n, T, Cc = logits.shape
    assert row_arg.dtype == torch.int32 and row_arg.shape == (n, T) and row_arg.is_contiguous() and row_lse.shape == (n, T)
    dev = logits.device
    ids = torch.empty(n, T, dtype=torch.int32, device=dev)
    tix = torch.empty(n, T, dtype=torch.int32, device=dev)
    count = torch.empty(n, dtype=torch.int32, device=dev)
    loss = tg = off = None
    longest = 0
    if targets is not None:
        if len(targets) != n:
            raise ValueError(f"ctc_score: {len(targets)} targets for {n} samples")
        flat, offs = [], [0]
        for t in targets:
            t = [int(v) for v in t]
            if any(v < 0 or v >= Cc for v in t):
                raise ValueError(f"ctc_score: a target id lies outside [0, {Cc})")
            flat += t
            offs.append(len(flat))
            longest = max(longest, len(t))
        if longest > 127:
            raise ValueError("ctc_score: targets of at most 127 symbols")
        tg = torch.tensor(flat or [0], dtype=torch.int32, device=dev)
        off = torch.tensor(offs, dtype=torch.int32, device=dev)
        loss = torch.empty(n, dtype=F32, device=dev)
    L.check(L.lib().tfx_ctc_score(logits.data_ptr(), row_arg.data_ptr(), row_lse.data_ptr(), _p(tg), _p(off), longest, n, T, Cc,
                                  ids.data_ptr(), tix.data_ptr(), count.data_ptr(), _p(loss), _stream()), "ctc_score")
    return ids, tix, count, loss
