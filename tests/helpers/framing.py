"""Canary frames for the outputs and NaN frames for the inputs of the exact GPU tests (tests/test_exact_rows_gpu.py,
tests/test_exact_layout_gpu.py): every output is a view inside a canary-filled buffer, every input a view inside a NaN-filled (integer
types: zero-filled) one, so a write or a read outside the operands shows."""
import torch

BF = torch.bfloat16
CANARY = {BF: -2.0 ** 127, torch.float32: -2.0 ** 127, torch.uint8: 0xA5}       # values no kernel here produces


def framed(B, R, C, dtype=BF, pad_rows=3, pad_cols=16):
    """A [B, R, C] view inside a canary-filled [B, R + 2 pad_rows, C + pad_cols] buffer."""
    buf = torch.full((B, R + 2 * pad_rows, C + pad_cols), CANARY[dtype], dtype=dtype, device="cuda")
    return buf, buf[:, pad_rows:pad_rows + R, :C]


def flat_framed(shape, dtype=BF, pad=64):
    """A contiguous `shape` view with `pad` canary elements before and after it."""
    n = int(torch.Size(shape).numel())
    buf = torch.full((n + 2 * pad,), CANARY[dtype], dtype=dtype, device="cuda")
    return buf, buf[pad:pad + n].view(shape)


def check_frame(buf, view, what):
    """Everything of buf outside view still holds the canary, and no element of view does."""
    buf, view = buf.cpu(), view.cpu()
    if buf.dim() == 1:
        pad = (buf.numel() - view.numel()) // 2
        outside = torch.cat([buf[:pad], buf[pad + view.numel():]])
    else:
        mask = torch.ones(buf.shape, dtype=torch.bool)
        pr = (buf.shape[1] - view.shape[-2]) // 2
        mask[:, pr:pr + view.shape[-2], :view.shape[-1]] = False
        outside = buf[mask]
    c = CANARY[buf.dtype]
    assert bool((outside == c).all()), f"{what}: wrote outside its output"
    if buf.dtype != torch.uint8:
        assert bool((view != c).all()), f"{what}: left part of its output unwritten"


def strided(t, pad_cols=24, col0=8):
    """t [.., R, C] (CPU) as a row- and batch-strided device view inside a NaN-filled [.., R + 2, C + pad_cols] buffer, 16-byte aligned."""
    lead = t.shape[:-2]
    R, C = t.shape[-2:]
    fill = float("nan") if t.dtype.is_floating_point else 0
    buf = torch.full((*lead, R + 2, C + pad_cols), fill, dtype=t.dtype, device="cuda")
    view = buf[..., 1:R + 1, col0:col0 + C]
    view.copy_(t)
    return view


def flat_in(t, pad=64, fill=None):
    """t (CPU) as a contiguous device view with `pad` elements of NaN (integer types: zero, or `fill`) before and after it: the form of
    an operand the entry takes without strides."""
    if fill is None:
        fill = float("nan") if t.dtype.is_floating_point else 0
    buf = torch.full((t.numel() + 2 * pad,), fill, dtype=t.dtype, device="cuda")
    view = buf[pad:pad + t.numel()].view(t.shape)
    view.copy_(t)
    return view
