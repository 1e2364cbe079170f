"""Recorder, reference walk and emulated engine for the three models around the DiT (textflux_amd/vae.py, textflux_amd/text_encoders.py).

RECORDER.  `Recorder` stands in for the `ops` module those files import (install it with pytest's monkeypatch, per test).  Every kernel
call is forwarded; the function name, the arguments and a CLONE of the result (for `out=` calls: of the `out` view, which the ops return)
go to a trace.  Cloning matters: `_attend` reuses its score / weight buffers and the seam blend works in place.  An argument whose
data_ptr() is that of a tensor of the model's `sd` / `hw` / `w` dicts is recorded as a `Weight` carrying the dict labels, not as data.

WALK.  `walk_vae`, `walk_vae_tiled`, `walk_t5`, `walk_clip` visit the model's graph in the order oracle/vae_oracle.py and
oracle/text_oracle.py define it (the structure is restated from the oracles, not from the code under test; a residual add that the engine
fuses into a GEMM / conv epilogue is part of that node).  The walk consumes the trace in step: the next recorded call must be the kernel
the node should be, so the launch sequence is pinned as well.  At every node
  * the inputs are the DEVICE'S OWN recorded outputs of the node's graph predecessors, and torch.equal asserts that the call received exactly
    those tensors (the wiring); errors therefore never compound from node to node;
  * the node's value is computed in fp64 from those inputs and the ORIGINAL state-dict tensors (the [Cout, Cin, 3, 3] filter, the real bias,
    the separate q / k / v and wi_0 / wi_1 matrices), so the engine's weight packing is under test;
  * EVERY element of the device output must lie in a window [lo, hi] of bf16 values (exact_inputs.assert_in_window), or equal the
    reference bit for bit where the node is exact (gather_rows, add, mul, transpose, blend_edge, crop / concatenate, the pooled row).
A failure raises NodeFailure with the node's name.

WINDOWS: derived, never fitted.  u = 2^-23 bounds the relative error of ONE fp32 operation under any rounding mode (the matrix pipe's
internal adds need not round to nearest).  bf(.) is the fp64 -> fp32 -> bf16 rounding; it is monotone, so a device value t in [a, b]
stores bf(t) in [bf(a), bf(b)].
  linear / conv   v = sum_K a_i w_i + b, S = sum |a_i w_i| + |b| (one more fp64 conv / matmul on absolute values).  K products are
                  exact in fp32 (two bf16 factors), K additions (bias included) each err by at most u times a partial sum that S bounds:
                  the fp32 value lies in v +- (K + 1) u S.  Window: the epilogue chain on both ends -- bf(t) | bf(res + bf(t)) (torch's
                  bf16 add, monotone) | GELU-tanh of bf(t).
  GELU-tanh       not monotone: over [bf(lo), bf(hi)] the least value is the function's minimum (x = -0.7518, found on a grid in fp64)
                  where the interval contains it, else the smaller end.  common.h evaluates x * rcp(2^(z - 32) + 2^-32) * 2^-32 with
                  z = x (c0 + c1 x^2) from two fmas: the exponent is off by at most 2 u (32 + |z|), the exp2 / rcp units by one step
                  each, three products: a relative (72 + 2 |z|) u on the ends.
  GroupNorm       gn_partial_kernel: a lane adds 4 channels of at most ceil(1024 / (256 / (C / 8))) pixels, one lane per (group, statistic)
                  then adds at most 512 lane partials: no element passes through more than A = 4 P + 512 fp32 additions, so a chunk's
                  sum is off by at most A u sum|x| (squares: one more rounding).  gn_finalize_kernel adds the chunks in double and
                  forms mean = s * fp32(1 / count), var = q * inv - mean^2 in double, casts both to fp32 and adds eps in fp32:
                  |mean' - mean| <= em = (A + 2) u mean|x|, |var' - var| <= ev = (A + 3) u E[x^2] + 2 |mean| em + em^2 + 2 u (var + eps);
                  rstd in [rsqrt(var + eps + ev) (1 - 4u), rsqrt(var + eps - ev) (1 + 4u)] (rsqrtf within two steps, as
                  tests/test_exact_rows_gpu.py allows with X.nudge).  y = (x - mean) rstd gamma + beta is bilinear in (mean, rstd): its
                  range over the box is spanned by the four corners; four fp32 operations add 4 u (|(x - mean) rstd gamma| + |beta|).
                  One rounding bf(y) (X.groupnorm_chain), then SiLU of that bf16 value.
  SiLU            y / (1 + __expf(-y)) is not monotone either (minimum at y = -1.2785): as GELU, with a relative (2 |y| + 8) u for the
                  fp32 exponential (argument product, exp2 unit), the add and the division.
  LayerNorm       tfx_layernorm (X.layernorm_affine_chain): mean = sum / D, var = sum (x - mean)^2 / D in fp32 over D terms:
                  em = (D + 2) u mean|x|, ev = (D + 4) u var + em^2 + 2 u (var + eps); then as GroupNorm without the activation.
  T5 RMSNorm      tfx_rmsnorm (X.t5_rmsnorm_chain): r = rsqrt(sum x^2 / D + eps), the sum off by (D + 4) u, r by half of it + 4 u;
                  t = bf(x r) from both ends (+- u |t| for the product), out = w * t in torch's bf16 product, min / max of the ends.
  quick_gelu      X.quick_gelu_chain: bf(1.702 x) is exact arithmetic, sigmoid of that bf16 value +- (2 |arg| + 8) u then bf, then the
                  bf16 product with x: min / max of the two ends.
  attend (VAE)    P the fp64 softmax.  The device rounds each weight to bf16 (2^-8 covers truncation), sums Np products in fp32, K = C
                  products per score: P.v lies within (2^-8 + (Np + C + 4) u) sum_j P_ij |v_jc| of the fp64 result, then one bf16 rounding.
  attention64     attn64_kernel (X.attention64_graded_chain restates it): score s' = s + e, |e| <= es = 68 u (|scale| sum|q k| + |bias|)
                  (64 products, the scale, the bias add, the log2 e product); the exponent argument s' log2 e - m is off by u (|s| + |s - m|)
                  more, exp2 by a step; a weight is rounded to bf16 (2^-8), the row sum and the output add N terms and are rescaled N / 32
                  times in fp32, one reciprocal and one product finish.  A relative error rho in every weight and in the normaliser
                  moves the output by at most 2 rho sum_j P_ij |v_jd|.  With es_i and sm_i = max_j (|s_ij| + |s_ij - m_i|) over the
                  unmasked keys: rho_i = 2^-8 + 4 es_i + (4 sm_i + 4 N + 32) u, window bf(o -+ rho_i sum_j P_ij |v_jd|).

EMULATED ENGINE.  `EmuOps` implements the same calls on the CPU: every kernel in fp64 from the inputs it is handed and the PACKED weights
in the layouts include/textflux_hip.h documents, rounded at the documented points with torch's bf16 operators.  The model code runs
unchanged on top of it, which gives a trace without a GPU; `fault=(kind, target label)` makes one kernel (or, for the host-side faults,
the test makes one table / one result) wrong in a named way.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional

import torch
import torch.nn.functional as F

from oracle import text_oracle as to
from oracle import vae_oracle as vo
from tests.helpers import exact_inputs as X

BF = torch.bfloat16
U = 2.0 ** -23
EPI_PLAIN, EPI_GELU, EPI_RES = 0, 1, 3              # include/textflux_hip.h: tfx_gemm_args.epilogue
RECORDED = ("conv3x3_nhwc", "conv3x3_pair_nhwc", "groupnorm_nhwc", "gemm", "gemm_f32", "row_softmax", "transpose", "blend_edge_nhwc_",
            "rmsnorm", "layernorm", "attention64", "gather_rows", "add", "mul", "quick_gelu")


class NodeFailure(AssertionError):
    def __init__(self, node: str, msg: str):
        super().__init__(f"{node}: {msg}")
        self.node = node


# ------------------------------------------------------------------------------------------------------------------ recorder
class Weight:
    """A recorded argument that is one of the model's own tensors: the dict labels it is held under (a 1 x 1 filter's matrix view
    shares its state-dict tensor's storage, so there can be two)."""

    def __init__(self, names):
        self.names = frozenset(names)

    def __repr__(self):
        return f"Weight({sorted(self.names)})"


class Call:
    def __init__(self, fn, args, kwargs, workspace):
        self.fn, self.args, self.kwargs, self.workspace, self.out = fn, args, kwargs, workspace, None

    def arg(self, i, key, default=None):
        return self.args[i] if len(self.args) > i else self.kwargs.get(key, default)


class Recorder:
    def __init__(self, real, weights: Dict[str, torch.Tensor]):
        self._real, self.trace, self._names = real, [], {}
        for label, t in weights.items():
            self._names.setdefault(t.data_ptr(), set()).add(label)

    def labels(self, t) -> frozenset:
        return frozenset(self._names.get(t.data_ptr(), ())) if torch.is_tensor(t) else frozenset()

    def _snap(self, v):
        if not torch.is_tensor(v):
            return v
        names = self._names.get(v.data_ptr())
        return Weight(names) if names else v.detach().cpu().clone()

    def __getattr__(self, name):
        attr = getattr(self._real, name)
        if name not in RECORDED:
            return attr

        def wrapped(*args, **kwargs):
            c = Call(name, [self._snap(a) for a in args], {k: self._snap(v) for k, v in kwargs.items() if k != "workspace"},
                     kwargs.get("workspace") is not None)
            r = attr(*args, **kwargs)
            c.out = r.detach().cpu().clone()
            self.trace.append(c)
            return r
        return wrapped


def vae_weights(vae) -> Dict[str, torch.Tensor]:
    w = {f"sd:{k}": v for k, v in vae.sd.items()}
    for k, v in vae.hw.items():
        if isinstance(v, tuple):
            w.update({f"hw:{k}[{i}]": t for i, t in enumerate(v)})
        else:
            w[f"hw:{k}"] = v
    return w


def text_weights(model) -> Dict[str, torch.Tensor]:
    return {f"w:{k}": v for k, v in model.w.items()}


def install(monkeypatch, module, engine, weights) -> Recorder:
    """Put a Recorder over `engine` (the real ops module, or an EmuOps) in place of `module.ops`."""
    rec = Recorder(engine, weights)
    if isinstance(engine, EmuOps):
        engine.labels = rec.labels
    monkeypatch.setattr(module, "ops", rec)
    return rec


# ------------------------------------------------------------------------------------------------------------------ windows
def bf(t: torch.Tensor) -> torch.Tensor:
    return t.float().to(BF)


def _argmin_on_grid(f, a, b):
    xs = torch.linspace(a, b, 200001, dtype=torch.float64)
    return float(xs[f(xs).argmin()])


GELU_XMIN = _argmin_on_grid(X.gelu_tanh64, -0.76, -0.74)
SILU_XMIN = _argmin_on_grid(X.silu64, -1.29, -1.27)
assert abs(GELU_XMIN + 0.7518) < 1e-3 and abs(SILU_XMIN + 1.2785) < 1e-3


def _dip_window(f, xmin: float, rel, lo: torch.Tensor, hi: torch.Tensor):
    """Window of f over the bf16 interval [lo, hi] for a function with ONE minimum at xmin, evaluated in fp32 with relative error rel(x)."""
    a, b = f(lo), f(hi)
    mn, mx = torch.minimum(a, b), torch.maximum(a, b)
    inside = (lo.double() < xmin) & (hi.double() > xmin)
    mn = torch.where(inside, f(torch.tensor(xmin, dtype=torch.float64)).expand_as(mn), mn)
    r = torch.maximum(rel(lo.double()), rel(hi.double()))
    return bf(mn - r * mn.abs()), bf(mx + r * mx.abs())


def gelu_window(lo, hi):
    z = lambda x: (x * (2.3022081981443252 + 0.10294323958002349 * x * x)).abs()
    return _dip_window(X.gelu_tanh64, GELU_XMIN, lambda x: (72 + 2 * z(x)) * U, lo, hi)


def silu_window(lo, hi):
    return _dip_window(X.silu64, SILU_XMIN, lambda x: (2 * x.abs() + 8) * U, lo, hi)


def linear_window(v, d, epilogue=EPI_PLAIN, res=None, gelu_from_col=0):
    lo, hi = bf(v - d), bf(v + d)
    if epilogue == EPI_RES:
        return res + lo, res + hi
    if epilogue == EPI_GELU:
        lo, hi = lo.clone(), hi.clone()
        lo[..., gelu_from_col:], hi[..., gelu_from_col:] = gelu_window(lo[..., gelu_from_col:], hi[..., gelu_from_col:])
    return lo, hi


def matmul_bounds(a, w64, b64=None):
    """(v, (K + 1) u S) of a @ w^T + b; a bf16 [.., K], w64 fp64 [N, K]."""
    a64 = a.double()
    v, S = a64 @ w64.T, a64.abs() @ w64.abs().T
    if b64 is not None:
        v, S = v + b64, S + b64.abs()
    return v, (a.shape[-1] + 1) * U * S


def conv_bounds(x, w64, b64, stride=1, up=1):
    """(v, (9 Cin + 1) u S) [B, H, W, Cout] of the reference's 3 x 3 convolution of x NHWC bf16 with the [Cout, Cin, 3, 3] filter:
    F.interpolate(nearest) before an up = 2 conv, the asymmetric (0, 1, 0, 1) padding before a stride-2 one."""
    xi = x.double().permute(0, 3, 1, 2)
    if up == 2:
        xi = F.interpolate(xi, scale_factor=2.0, mode="nearest")
    pad = 1
    if stride == 2:
        xi, pad = F.pad(xi, (0, 1, 0, 1), mode="constant", value=0), 0
    v = F.conv2d(xi, w64, b64, stride=stride, padding=pad)
    S = F.conv2d(xi.abs(), w64.abs(), b64.abs(), stride=stride, padding=pad)
    return v.permute(0, 2, 3, 1), (9 * w64.shape[1] + 1) * U * S.permute(0, 2, 3, 1)


def _affine_window(x64, mlo, mhi, rlo, rhi, gamma, beta):
    g, b = gamma.double(), beta.double()
    ys = [(x64 - m) * r * g + b for m in (mlo, mhi) for r in (rlo, rhi)]
    ts = [(y - b).abs() for y in ys]
    slack = 4 * U * (torch.stack(ts).max(0).values + b.abs())
    ylo, yhi = torch.stack(ys).min(0).values - slack, torch.stack(ys).max(0).values + slack
    return bf(ylo), bf(yhi), (yhi - ylo) / 2


def _rstd_box(var, eps, ev):
    eps = float(torch.tensor(eps, dtype=torch.float32))
    return (var + eps + ev) ** -0.5 * (1 - 4 * U), (var + eps - ev).clamp(min=eps / 2) ** -0.5 * (1 + 4 * U)


def groupnorm_window(x, gamma, beta, groups: int, silu: bool, eps: float = 1e-6):
    """x [B, HW, C] bf16 -> (lo, hi, centre, half width before the rounding; None with SiLU: two roundings) of tfx_groupnorm_nhwc."""
    B, HW, C = x.shape
    cpg = C // groups
    xg = x.double().view(B, HW, groups, cpg)
    m, q, am = xg.mean((1, 3)), (xg ** 2).mean((1, 3)), xg.abs().mean((1, 3))
    var = (q - m * m).clamp(min=0)
    A = 4 * math.ceil(min(HW, 1024) / (256 // (C // 8))) + 512
    em = (A + 2) * U * am
    ev = (A + 3) * U * q + 2 * m.abs() * em + em * em + 2 * U * (var + eps)
    rlo, rhi = _rstd_box(var, eps, ev)
    ex = lambda t: t.repeat_interleave(cpg, 1)[:, None, :]
    lo, hi, half = _affine_window(x.double(), ex(m - em), ex(m + em), ex(rlo), ex(rhi), gamma, beta)
    centre = (x.double() - ex(m)) * ex((var + eps) ** -0.5) * gamma.double() + beta.double()
    if silu:
        lo, hi = silu_window(lo, hi)
        centre, half = X.silu64(bf(centre)), None
    return lo, hi, centre, half


def layernorm_window(x, gamma, beta, eps: float):
    D = x.shape[-1]
    x64 = x.double()
    m = x64.mean(-1, keepdim=True)
    var = ((x64 - m) ** 2).mean(-1, keepdim=True)
    em = (D + 2) * U * x64.abs().mean(-1, keepdim=True)
    ev = (D + 4) * U * var + em * em + 2 * U * (var + eps)
    rlo, rhi = _rstd_box(var, eps, ev)
    lo, hi, half = _affine_window(x64, m - em, m + em, rlo, rhi, gamma, beta)
    return lo, hi, (x64 - m) * (var + eps) ** -0.5 * gamma.double() + beta.double(), half


def rmsnorm_window(x, w, eps: float):
    D = x.shape[-1]
    x64 = x.double()
    ms = (x64 ** 2).mean(-1, keepdim=True)
    rlo, rhi = _rstd_box(ms, eps, (D + 4) * U * ms)
    t1, t2 = x64 * rlo, x64 * rhi
    tlo, thi = torch.minimum(t1, t2), torch.maximum(t1, t2)
    a, b = w * bf(tlo - U * tlo.abs()), w * bf(thi + U * thi.abs())
    lo = torch.minimum(a.float(), b.float()).to(BF)
    hi = torch.maximum(a.float(), b.float()).to(BF)
    return lo, hi, w.double() * bf(x64 * (ms + eps) ** -0.5).double()


def quick_gelu_window(a):
    arg = (torch.tensor(1.702, dtype=torch.float32).double() * a.double()).float().to(BF).double()
    sg = 1.0 / (1.0 + torch.exp(-arg))
    r = (2 * arg.abs() + 8) * U
    p, q = a * bf(sg * (1 - r)), a * bf(sg * (1 + r))
    return torch.minimum(p.float(), q.float()).to(BF), torch.maximum(p.float(), q.float()).to(BF)


def attend_window(q, k, v):
    """The VAE mid-block attention, one head of dim C: q, k, v [B, N, C] bf16 -> (lo, hi, o, d)."""
    B, N, C = q.shape
    Np = (N + 63) // 64 * 64
    P = torch.softmax(q.double() @ k.double().transpose(1, 2) * C ** -0.5, -1)
    o, d = P @ v.double(), (2.0 ** -8 + (Np + C + 4) * U) * (P @ v.double().abs())
    return bf(o - d), bf(o + d), o, d


def attention64_window(q, k, v, scale: float, bias=None, causal: bool = False):
    """q, k, v [B, N, H * 64] bf16; bias fp64 [H, N, N] (query, key) or None -> (lo, hi, o, d)."""
    B, N, HD = q.shape
    H = HD // 64
    qh, kh, vh = (t.double().view(B, N, H, 64).transpose(1, 2) for t in (q, k, v))
    s, sa = qh @ kh.transpose(-1, -2) * scale, qh.abs() @ kh.abs().transpose(-1, -2) * abs(scale)
    if bias is not None:
        s, sa = s + bias, sa + bias.abs()
    live = torch.ones(N, N, dtype=torch.bool)
    if causal:
        live = ~torch.ones(N, N, dtype=torch.bool).triu(1)
        s = s.masked_fill(~live, -math.inf)
    m = s.max(-1, keepdim=True).values
    es = (68 * U * sa).masked_fill(~live, 0).max(-1, keepdim=True).values
    sm = (s.abs() + (s - m).abs()).masked_fill(~live, 0).max(-1, keepdim=True).values
    rho = 2.0 ** -8 + 4 * es + (4 * sm + 4 * N + 32) * U
    P = torch.softmax(s, -1)
    o, d = P @ vh, rho * (P @ vh.abs())
    back = lambda t: t.transpose(1, 2).reshape(B, N, HD)
    return bf(back(o - d)), bf(back(o + d)), back(o), back(d)


# ------------------------------------------------------------------------------------------------------------------ the walk
class Walk:
    """Cursor over a trace, the checks of a node, and the statistics of a whole walk: per node kind the nodes and elements checked and,
    where the node has ONE final rounding, `room`: the largest distance of the fp64 value from the rounding cell of the stored bf16
    number in units of the node's bound (0: the stored value is the rounding of the fp64 value itself; 1: the edge of the window).
    `off` counts the elements that differ from `ideal`, the node's rounding chain applied to the fp64 value itself."""

    def __init__(self, trace: List[Call], stats: Optional[dict] = None):
        self.trace, self.i = trace, 0
        self.stats = stats if stats is not None else {}

    def take(self, node: str, *fns) -> Call:
        if self.i >= len(self.trace):
            raise NodeFailure(node, f"the trace ends after {self.i} calls; expected {' / '.join(fns)}")
        c = self.trace[self.i]
        if c.fn not in fns:
            raise NodeFailure(node, f"call {self.i} of the trace is {c.fn}, the node is {' / '.join(fns)}")
        self.i += 1
        return c

    def done(self):
        if self.i != len(self.trace):
            raise NodeFailure("end", f"{len(self.trace) - self.i} calls after the last node, the first is {self.trace[self.i].fn}")

    def _count(self, kind, n):
        s = self.stats.setdefault(kind, dict(nodes=0, elements=0, room=None, off=0))
        s["nodes"] += 1
        s["elements"] += n
        return s

    def same(self, node, what, got, want):
        """The call received exactly this tensor (a free reshape of a contiguous activation is the same tensor)."""
        ok = torch.is_tensor(got) and got.dtype == want.dtype and got.numel() == want.numel() and torch.equal(got.reshape(want.shape), want)
        if not ok:
            raise NodeFailure(node, f"argument `{what}` is not the recorded output of its graph predecessor")

    def value(self, node, what, got, want):
        if got != want:
            raise NodeFailure(node, f"argument `{what}` is {got!r}, the node takes {want!r}")

    def weight(self, node, what, arg, *labels):
        if not (isinstance(arg, Weight) and any(l in arg.names for l in labels)):
            raise NodeFailure(node, f"argument `{what}` is {arg if isinstance(arg, Weight) else type(arg).__name__}, expected the tensor {' / '.join(labels)}")

    def exact(self, node, kind, got, want):
        self._count(kind, want.numel())
        if got.shape != want.shape or got.dtype != want.dtype:
            raise NodeFailure(node, f"shape / dtype {tuple(got.shape)} {got.dtype}, expected {tuple(want.shape)} {want.dtype}")
        bad = got != want
        if bad.any():
            raise NodeFailure(node, f"{int(bad.sum())} of {got.numel()} elements differ from the exact value; first at {tuple(bad.nonzero()[0].tolist())}")

    def window(self, node, kind, got, lo, hi, centre=None, bound=None, ideal=None):
        s = self._count(kind, lo.numel())
        if got.shape != lo.shape or got.dtype != BF:
            raise NodeFailure(node, f"shape / dtype {tuple(got.shape)} {got.dtype}, expected {tuple(lo.shape)} bf16")
        try:
            X.assert_in_window(got.reshape(-1, got.shape[-1]), lo.reshape(-1, lo.shape[-1]), hi.reshape(-1, hi.shape[-1]), node)
        except AssertionError as e:
            bad = ~((got.float() >= lo.float()) & (got.float() <= hi.float()))
            raise NodeFailure(node, f"{e}; index {tuple(bad.nonzero()[0].tolist())} of {tuple(got.shape)}") from None
        if ideal is not None:
            s["off"] += int((got != ideal.reshape(got.shape)).sum())
        if centre is not None and bound is not None:
            g = got.double()
            half = torch.where(g == 0, torch.zeros_like(g), torch.exp2(torch.frexp(g.abs().clamp(min=1e-300)).exponent.double() - 9))   # half a bf16 step
            dist = ((g - centre).abs() - half).clamp(min=0)
            room = float((dist / bound.clamp(min=1e-300)).max())
            s["room"] = max(room, s["room"] or 0.0)


class _VaeWalk:
    def __init__(self, W: Walk, sd, cfg, pair_convs: bool, attend_rows: int):
        self.W, self.cfg, self.pair_convs, self.rows = W, cfg, pair_convs, attend_rows
        self.sd = {k: v.to(BF) for k, v in sd.items()}                    # what load_state_dict holds
        self.attend_plan = []

    # -- nodes
    def conv(self, name, x, stride=1, up=1, res=None):
        W = self.W
        w, b = self.sd[name + ".weight"], self.sd[name + ".bias"]
        Cout, Cin = w.shape[:2]
        pair = self.pair_convs and Cin % 64 == 0 and Cout % 8 == 0 and Cout <= 128 and x.shape[2] % 2 == 0 and stride == 1 and up == 1
        c = W.take(name, "conv3x3_pair_nhwc" if pair else "conv3x3_nhwc")
        W.same(name, "x", c.args[0], x)
        if x.shape[3] != Cin:                                            # a narrow input: the channels above Cin are padding
            if bool((x[..., Cin:] != 0).any()):
                raise NodeFailure(name, "padding channels of the narrow input are not zero")
            x = x[..., :Cin]
        if pair:
            W.weight(name, "w_pair", c.args[1], f"hw:{name}.pair[0]")
            W.weight(name, "bias_pair", c.args[2], f"hw:{name}.pair[1]")
        else:
            W.weight(name, "w", c.args[1], f"hw:{name}.weight")
            W.weight(name, "bias", c.args[2], f"hw:{name}.bias" if Cout % 8 else f"sd:{name}.bias")
            for key, want in (("stride", stride), ("up", up), ("pad_lo", 0 if stride == 2 else 1)):
                W.value(name, key, c.kwargs.get(key, 1), want)
        got_res = c.kwargs.get("res")
        if res is None:
            W.value(name, "res", got_res, None)
        else:
            W.same(name, "res", got_res, res)
        v, d = conv_bounds(x, w.double(), b.double(), stride, up)
        got = c.out
        if got.shape[-1] != Cout:                                        # conv_out: 3 filters padded to 8, zero filters and zero bias
            W.exact(name, "exact", got[..., Cout:], torch.zeros_like(got[..., Cout:]))
            got = got[..., :Cout]
        lo, hi = linear_window(v, d, EPI_RES if res is not None else EPI_PLAIN, res)
        W.window(name, "conv", got, lo, hi, *((v, d) if res is None else (None, None)), ideal=bf(v) if res is None else res + bf(v))
        return c.out

    def gn(self, name, x, silu):
        W = self.W
        c = W.take(name, "groupnorm_nhwc")
        W.same(name, "x", c.args[0], x)
        W.weight(name, "gamma", c.args[1], f"sd:{name}.weight")
        W.weight(name, "beta", c.args[2], f"sd:{name}.bias")
        W.value(name, "groups", c.args[3], self.cfg.norm_num_groups)
        W.value(name, "silu", c.kwargs.get("silu", True), silu)
        W.value(name, "eps", c.kwargs.get("eps", 1e-6), 1e-6)
        B, C = x.shape[0], x.shape[-1]
        lo, hi, centre, half = groupnorm_window(x.reshape(B, -1, C), self.sd[name + ".weight"], self.sd[name + ".bias"], self.cfg.norm_num_groups, silu)
        W.window(name, "groupnorm+silu" if silu else "groupnorm", c.out.reshape(B, -1, C), lo, hi, centre, half, ideal=bf(centre))
        return c.out

    def linear(self, name, a, res=None):
        W = self.W
        w, b = self.sd[name + ".weight"], self.sd[name + ".bias"]
        c = W.take(name, "gemm")
        W.same(name, "a", c.args[0], a)
        W.weight(name, "w", c.args[1], f"hw:{name}.weight", f"sd:{name}.weight")
        W.weight(name, "bias", c.args[2], f"sd:{name}.bias")
        W.value(name, "epilogue", c.kwargs.get("epilogue", EPI_PLAIN), EPI_RES if res is not None else EPI_PLAIN)
        if res is not None:
            W.same(name, "res", c.kwargs.get("res"), res)
        a2 = a.reshape(-1, a.shape[-1])
        v, d = matmul_bounds(a2, w.double().reshape(w.shape[0], -1), b.double())
        r2 = res.reshape(v.shape) if res is not None else None
        lo, hi = linear_window(v, d, EPI_RES if res is not None else EPI_PLAIN, r2)
        W.window(name, "linear", c.out.reshape(v.shape), lo, hi, *((v, d) if res is None else (None, None)), ideal=bf(v) if res is None else r2 + bf(v))
        return c.out

    def attend(self, name, q, k, v):
        """ONE node: q, k, v in, o out.  The calls inside are consumed as a group, their count and kinds against the chunk plan: a
        transpose; per chunk of `rows` query rows a score GEMM, ONE softmax launch for a full chunk or one per image for a ragged one,
        and the K-sliced P v GEMM.  The zero padding of the weights and of v^T to a multiple of 64 keys is asserted on the way."""
        W = self.W
        B, N, C = q.shape
        Np = (N + 63) // 64 * 64
        t = W.take(name, "transpose")
        W.same(name, "v", t.args[0], v)
        W.exact(name, "exact", t.out, v.transpose(1, 2).contiguous())
        vt = torch.zeros(B, C, Np, dtype=BF)
        vt[:, :, :N] = t.out
        parts, plan = [], []
        for r0 in range(0, N, self.rows):
            n = min(self.rows, N - r0)
            g = W.take(name, "gemm_f32")
            W.same(name, "q rows of the chunk", g.args[0], q[:, r0:r0 + n])
            W.same(name, "k", g.args[1], k)
            full = n == self.rows
            launches = 1 if full else B
            pw = []
            for b in range(launches):
                sm = W.take(name, "row_softmax")
                W.value(name, "softmax scale", sm.args[1], C ** -0.5)
                W.value(name, "softmax shape", tuple(sm.args[0].shape), (B * self.rows, N) if full else (n, N))
                if full:
                    W.same(name, "scores", sm.args[0].view(B, self.rows, N)[:, :n], g.out)
                else:
                    W.same(name, "scores", sm.args[0], g.out[b])
                pw.append(sm.out.view(B, self.rows, Np)[:, :n] if full else sm.out[None])
            pw = torch.cat(pw, 0)
            if bool((pw[:, :, N:] != 0).any()):
                raise NodeFailure(name, "a padded key column carries a non-zero softmax weight")
            pv = W.take(name, "gemm")
            W.same(name, "softmax weights", pv.args[0], pw)
            W.same(name, "v^T, zero-padded", pv.args[1], vt)
            if not pv.workspace:
                raise NodeFailure(name, "the P v product runs without its K-slicing workspace")
            parts.append(pv.out)
            plan.append((n, launches))
        o = torch.cat(parts, 1)
        lo, hi, o64, d = attend_window(q, k, v)
        W.window(name, "attend", o, lo, hi, o64, d, ideal=bf(o64))
        self.attend_plan.append(plan)
        return o

    # -- the graph, as oracle/vae_oracle.py has it
    def resnet(self, x, p):
        h = self.conv(p + ".conv1", self.gn(p + ".norm1", x, True))
        h = self.gn(p + ".norm2", h, True)
        if p + ".conv_shortcut.weight" in self.sd:
            x = self.linear(p + ".conv_shortcut", x)
        return self.conv(p + ".conv2", h, res=x.reshape(h.shape[0], h.shape[1], h.shape[2], -1))

    def mid_block(self, x, p):
        x = self.resnet(x, p + ".resnets.0")
        a = p + ".attentions.0"
        B, H, Wd, C = x.shape
        tok = x.reshape(B, H * Wd, C)
        h = self.gn(a + ".group_norm", tok, False)
        q, k, v = (self.linear(f"{a}.{n}", h) for n in ("to_q", "to_k", "to_v"))
        o = self.attend(a + ".attend", q, k, v)
        x = self.linear(a + ".to_out.0", o, res=tok).reshape(B, H, Wd, C)
        return self.resnet(x, p + ".resnets.1")

    def encoder(self, x):
        c = self.cfg
        h = self.conv("encoder.conv_in", x)
        n = len(c.block_out_channels)
        for i in range(n):
            for j in range(c.layers_per_block):
                h = self.resnet(h, f"encoder.down_blocks.{i}.resnets.{j}")
            if i != n - 1:
                h = self.conv(f"encoder.down_blocks.{i}.downsamplers.0.conv", h, stride=2)
        h = self.mid_block(h, "encoder.mid_block")
        return self.conv("encoder.conv_out", self.gn("encoder.conv_norm_out", h, True))

    def decoder(self, z):
        c = self.cfg
        h = self.conv("decoder.conv_in", z)
        h = self.mid_block(h, "decoder.mid_block")
        n = len(c.block_out_channels)
        for i in range(n):
            for j in range(c.layers_per_block + 1):
                h = self.resnet(h, f"decoder.up_blocks.{i}.resnets.{j}")
            if i != n - 1:
                h = self.conv(f"decoder.up_blocks.{i}.upsamplers.0.conv", h, up=2)
        return self.conv("decoder.conv_out", self.gn("decoder.conv_norm_out", h, True))


def walk_vae(trace, sd, cfg, end: str, x, result, pair_convs: bool = True, attend_rows: int = 256, stats=None):
    """One untiled encoder (`end` "encoder": x [B, H, W, 8] NHWC bf16 -> moments) or decoder ("decoder": z [B, h, w, L]) run.  Returns the
    chunk plans [(rows of the chunk, softmax launches), ..] of the mid-block attentions."""
    W = Walk(trace, stats)
    vw = _VaeWalk(W, sd, cfg, pair_convs, attend_rows)
    out = getattr(vw, end)(x)
    W.exact(end + ".result", "exact", result, out)
    W.done()
    return vw.attend_plan


def walk_vae_tiled(trace, sd, cfg, end: str, x, result, sample_size: int, pair_convs: bool = True, attend_rows: int = 256, stats=None):
    """A tiled run: every tile walked as its own model run, every seam blend torch.equal to the reference's blend_v / blend_h on the
    device's own tile outputs in the reference's in-place order, and the result equal to the reference's blend / crop / concatenate
    (vae_oracle._tiled) of those tile outputs."""
    W = Walk(trace, stats)
    vw = _VaeWalk(W, sd, cfg, pair_convs, attend_rows)
    ts, tl = vo.tile_sizes(cfg, sample_size)
    tile, out_tile = (ts, tl) if end == "encoder" else (tl, ts)
    step, extent = int(tile * 0.75), int(out_tile * 0.25)
    ys, xs = range(0, x.shape[1], step), range(0, x.shape[2], step)
    outs = {(r, c): getattr(vw, end)(x[:, y0:y0 + tile, x0:x0 + tile].contiguous()) for r, y0 in enumerate(ys) for c, x0 in enumerate(xs)}
    cur = {k: v.clone() for k, v in outs.items()}
    for r in range(len(ys)):
        for c in range(len(xs)):
            for on, nb, axis, blend in ((r, (r - 1, c), 1, vo._blend_v), (c, (r, c - 1), 2, vo._blend_h)):
                if not on:
                    continue
                node = f"{end}.tile[{r},{c}].blend_{'v' if axis == 1 else 'h'}"
                b = W.take(node, "blend_edge_nhwc_")
                W.same(node, "a", b.args[0], cur[nb])
                W.same(node, "b", b.args[1], cur[r, c])
                W.value(node, "extent", b.args[2], extent)
                W.value(node, "axis", b.arg(3, "axis"), axis)
                want = cur[r, c].clone()
                blend(cur[nb].permute(0, 3, 1, 2), want.permute(0, 3, 1, 2), extent)
                W.exact(node, "exact", b.out, want)
                cur[r, c] = b.out
    it = iter(outs[k].permute(0, 3, 1, 2).clone() for k in sorted(outs))
    want = vo._tiled(x.permute(0, 3, 1, 2), lambda _t: next(it), tile, out_tile, 0.25).permute(0, 2, 3, 1).contiguous()
    W.exact(end + ".result", "exact", result, want)
    W.done()
    return len(outs)


# -- text encoders
def _gemm_node(W, node, a, w64, b64, label, bias_label=None, epilogue=EPI_PLAIN, res=None, gelu_from_col=0):
    c = W.take(node, "gemm")
    W.same(node, "a", c.args[0], a)
    W.weight(node, "w", c.args[1], label)
    if bias_label is None:
        W.value(node, "bias", c.arg(2, "bias"), None)
    else:
        W.weight(node, "bias", c.arg(2, "bias"), bias_label)
    W.value(node, "epilogue", c.kwargs.get("epilogue", EPI_PLAIN), epilogue)
    if epilogue == EPI_GELU:
        W.value(node, "gelu_from_col", c.kwargs.get("gelu_from_col", 0), gelu_from_col)
    if epilogue == EPI_RES:
        W.same(node, "res", c.kwargs.get("res"), res)
    v, d = matmul_bounds(a.reshape(-1, a.shape[-1]), w64, b64)
    lo, hi = linear_window(v, d, epilogue, res.reshape(v.shape) if res is not None else None, gelu_from_col)
    ideal = X.chain(epilogue, bf(v), res=res.reshape(v.shape) if res is not None else None, gelu_from_col=gelu_from_col)
    W.window(node, "linear", c.out.reshape(v.shape), lo, hi, *((v, d) if epilogue == EPI_PLAIN else (None, None)), ideal=ideal)
    return c.out


def _attn_node(W, node, qkv, inner, scale, bias64=None, table=None, causal=False):
    c = W.take(node, "attention64")
    q, k, v = qkv[:, :, :inner], qkv[:, :, inner:2 * inner], qkv[:, :, 2 * inner:]
    for what, got, want in (("q", c.args[0], q), ("k", c.args[1], k), ("v", c.args[2], v)):
        W.same(node, what, got, want)
    W.value(node, "scale", c.args[3], scale)
    W.value(node, "causal", bool(c.kwargs.get("causal", False)), causal)
    got_table = c.kwargs.get("rel_bias")
    if table is None:
        W.value(node, "rel_bias", got_table, None)
    elif not (torch.is_tensor(got_table) and got_table.shape == table.shape and torch.equal(got_table, table)):
        raise NodeFailure(node, "rel_bias is not the reference's position bias as a table over key - query")
    lo, hi, o, d = attention64_window(q, k, v, scale, bias64, causal)
    W.window(node, "attention64", c.out, lo, hi, o, d, ideal=bf(o))
    return c.out


def walk_t5(trace, sd, cfg: to.T5Cfg, ids, result, stats=None):
    W = Walk(trace, stats)
    sd = to.t5_state_dict_as_loaded(sd)
    B, T = ids.shape
    D, inner, dff, eps = cfg.d_model, cfg.num_heads * 64, cfg.d_ff, cfg.layer_norm_epsilon
    c = W.take("t5.emb", "gather_rows")
    W.weight("t5.emb", "table", c.args[0], "w:embed")
    W.same("t5.emb", "ids", c.args[1], ids)
    W.exact("t5.emb", "exact", c.out, sd.get("shared.weight", sd.get("encoder.embed_tokens.weight"))[ids].reshape(B * T, D))
    x = c.out
    bias = to.t5_position_bias(sd, cfg, T)[0]                            # [H, T, T] (query, key), bf16
    table = torch.cat([bias[:, T - 1, :], bias[:, 0, 1:]], -1).float().contiguous()      # over key - query = -(T - 1) .. T - 1

    def norm(node, x, label, key):
        c = W.take(node, "rmsnorm")
        W.same(node, "x", c.args[0], x)
        W.weight(node, "w", c.args[1], label)
        W.value(node, "eps", c.args[2], eps)
        lo, hi, centre = rmsnorm_window(x, sd[key], eps)
        W.window(node, "rmsnorm", c.out, lo, hi, ideal=bf(centre))
        return c.out

    for i in range(cfg.num_layers):
        p, n = f"encoder.block.{i}.layer.", f"t5.{i}."
        a, f = p + "0.SelfAttention.", p + "1.DenseReluDense."
        h = norm(n + "ln0", x, f"w:{i}.ln0", p + "0.layer_norm.weight")
        w64 = torch.cat([sd[a + "q.weight"], sd[a + "k.weight"], sd[a + "v.weight"]], 0).double()
        qkv = _gemm_node(W, n + "qkv", h, w64, None, f"w:{i}.qkv")
        o = _attn_node(W, n + "attn", qkv.view(B, T, 3 * inner), inner, 1.0, bias.double(), table)
        x = _gemm_node(W, n + "o", o.reshape(B * T, inner), sd[a + "o.weight"].double(), None, f"w:{i}.o", epilogue=EPI_RES, res=x)
        h = norm(n + "ln1", x, f"w:{i}.ln1", p + "1.layer_norm.weight")
        w64 = torch.cat([sd[f + "wi_1.weight"], sd[f + "wi_0.weight"]], 0).double()      # the node's value: [wi_1 x | gelu(wi_0 x)]
        u = _gemm_node(W, n + "wi", h, w64, None, f"w:{i}.wi", epilogue=EPI_GELU, gelu_from_col=dff)
        c = W.take(n + "mul", "mul")
        W.same(n + "mul", "a", c.args[0], u[:, dff:])
        W.same(n + "mul", "b", c.args[1], u[:, :dff])
        W.exact(n + "mul", "exact", c.out, u[:, dff:] * u[:, :dff])
        x = _gemm_node(W, n + "wo", c.out, sd[f + "wo.weight"].double(), None, f"w:{i}.wo", epilogue=EPI_RES, res=x)
    out = norm("t5.final_ln", x, "w:final_ln", "encoder.final_layer_norm.weight")
    W.exact("t5.result", "exact", result, out.view(B, T, D))
    W.done()


def walk_clip(trace, sd, cfg: to.ClipCfg, ids, last, pooled, stats=None):
    W = Walk(trace, stats)
    sd = {k: v.to(BF) for k, v in sd.items()}
    pre = "text_model." if any(k.startswith("text_model.") for k in sd) else ""
    B, T = ids.shape
    D, eps = cfg.hidden_size, cfg.layer_norm_eps
    c = W.take("clip.tok", "gather_rows")
    W.weight("clip.tok", "table", c.args[0], "w:tok")
    W.same("clip.tok", "ids", c.args[1], ids)
    W.exact("clip.tok", "exact", c.out, sd[pre + "embeddings.token_embedding.weight"][ids].reshape(B * T, D))
    tok = c.out
    c = W.take("clip.pos", "gather_rows")
    W.weight("clip.pos", "table", c.args[0], "w:pos")
    W.same("clip.pos", "ids", c.args[1].view(B, T), torch.arange(T)[None].expand(B, T).contiguous())
    W.exact("clip.pos", "exact", c.out, sd[pre + "embeddings.position_embedding.weight"][:T][None].expand(B, T, D).reshape(B * T, D))
    pos = c.out
    c = W.take("clip.emb", "add")
    W.same("clip.emb", "a", c.args[0], tok)
    W.same("clip.emb", "b", c.args[1], pos)
    W.exact("clip.emb", "exact", c.out, tok + pos)
    x = c.out.view(B, T, D)

    def norm(node, x, label, key):
        c = W.take(node, "layernorm")
        W.same(node, "x", c.args[0], x)
        W.weight(node, "gamma", c.args[1], label + ".gamma")
        W.weight(node, "beta", c.args[2], label + ".beta")
        W.value(node, "eps", c.arg(3, "eps"), eps)
        lo, hi, centre, half = layernorm_window(x, sd[key + ".weight"], sd[key + ".bias"], eps)
        W.window(node, "layernorm", c.out, lo, hi, centre, half, ideal=bf(centre))
        return c.out

    for i in range(cfg.num_hidden_layers):
        l, n = f"{pre}encoder.layers.{i}.", f"clip.{i}."
        wb = lambda k: (sd[l + k + ".weight"].double(), sd[l + k + ".bias"].double())
        h = norm(n + "ln1", x, f"w:{i}.ln1", l + "layer_norm1")
        ws, bs = zip(*(wb(f"self_attn.{m}_proj") for m in "qkv"))
        qkv = _gemm_node(W, n + "qkv", h, torch.cat(ws, 0), torch.cat(bs, 0), f"w:{i}.qkv.w", f"w:{i}.qkv.b")
        o = _attn_node(W, n + "attn", qkv.view(B, T, 3 * D), D, 64 ** -0.5, causal=True)
        x = _gemm_node(W, n + "o", o, *wb("self_attn.out_proj"), f"w:{i}.o.w", f"w:{i}.o.b", epilogue=EPI_RES, res=x)
        h = norm(n + "ln2", x, f"w:{i}.ln2", l + "layer_norm2")
        u = _gemm_node(W, n + "fc1", h, *wb("mlp.fc1"), f"w:{i}.fc1.w", f"w:{i}.fc1.b")
        c = W.take(n + "act", "quick_gelu")
        W.same(n + "act", "a", c.args[0], u)
        lo, hi = quick_gelu_window(u.reshape(B * T, -1))
        W.window(n + "act", "quick_gelu", c.out.reshape(B * T, -1), lo, hi, ideal=X.quick_gelu_chain(u.reshape(B * T, -1)))
        x = _gemm_node(W, n + "fc2", c.out, *wb("mlp.fc2"), f"w:{i}.fc2.w", f"w:{i}.fc2.b", epilogue=EPI_RES, res=x).view(B, T, D)
    out = norm("clip.final_ln", x, "w:final", pre + "final_layer_norm").view(B, T, D)
    W.exact("clip.result", "exact", last, out)
    eos = ids.argmax(-1) if cfg.eos_token_id == 2 else (ids == cfg.eos_token_id).int().argmax(-1)
    W.exact("clip.pooled", "exact", pooled, out[torch.arange(B), eos])
    W.done()


# ------------------------------------------------------------------------------------------------------------------ emulated engine
class EmuOps:
    """The kernels of textflux_amd.ops on the CPU (see the module docstring).  fault = (kind, label): the kernel call whose weight
    argument carries `label` (or, for the attention faults, every call of that kind) goes wrong in the named way."""

    def __init__(self, real_ops, fault=None):
        self._real, self.fault, self.labels = real_ops, fault, (lambda t: frozenset())
        self._shortcut_in = None
        self._softmax_calls = 0

    def __getattr__(self, name):                                         # EPI_* constants, pair_conv_weights (torch only)
        if name.startswith("EPI_") or name == "pair_conv_weights":
            return getattr(self._real, name)
        raise AttributeError(f"the emulated engine has no {name}")

    def _hit(self, kind, *tensors):
        return self.fault is not None and self.fault[0] == kind and (self.fault[1] is None or any(self.fault[1] in self.labels(t) for t in tensors))

    @staticmethod
    def _put(out, r):
        if out is None:
            return r
        out.copy_(r)
        return out

    def _conv64(self, x, w4, bias, stride, up, taps_t=False, up_after=False, down_pad=False, border=False):
        xi, wf = x.double().permute(0, 3, 1, 2), w4.double().permute(0, 3, 1, 2)
        if taps_t:
            wf = wf.transpose(2, 3)
        if up == 2 and not up_after:
            xi = F.interpolate(xi, scale_factor=2.0, mode="nearest")
        if stride == 2:
            y = F.conv2d(F.pad(xi, (1, 0, 1, 0) if down_pad else (0, 1, 0, 1)), wf, bias.double(), stride=2)
        else:
            xp = F.pad(xi, (1, 1, 1, 1))
            if border:
                xp[:, :, :, 0] = xp[:, :, :, 1]
            y = F.conv2d(xp, wf, bias.double())
        if up == 2 and up_after:
            y = F.interpolate(y, scale_factor=2.0, mode="nearest")
        return y.permute(0, 2, 3, 1)

    def _res(self, y, res, w):
        if res is None:
            return y
        if self._hit("res_before_shortcut", w):
            a = self._shortcut_in
            res = a.repeat(*([1] * (a.dim() - 1)), y.shape[-1] // a.shape[-1]).view(y.shape)
        return res + y

    def conv3x3_nhwc(self, x, w, bias, stride=1, up=1, pad_lo=1, res=None, out=None, variant=-1):
        assert pad_lo == (0 if stride == 2 else 1) and x.dtype == BF
        cp = x.shape[3]
        w4 = w if w.dim() == 4 else w[:, :9 * cp].reshape(w.shape[0], 3, 3, cp)
        if self._hit("bias_shifted", w):
            bias = torch.cat([bias[1:], torch.zeros_like(bias[:1])])
        y = bf(self._conv64(x, w4, bias, stride, up, self._hit("taps_transposed", w), self._hit("up_after", w), self._hit("down_pad", w),
                            self._hit("border_column", w)))
        return self._put(out, self._res(y, res, w))

    def conv3x3_pair_nhwc(self, x, w_pair, bias_pair, res=None, out=None):
        B, H, Wd, Cin = x.shape
        Cout = w_pair.shape[0] // 2
        assert Wd % 2 == 0
        wf = w_pair.double().permute(0, 3, 1, 2)                          # [2 Cout, Cin, 3, 4]
        if self._hit("taps_transposed", w_pair):
            wf = torch.cat([F.pad(wf[:Cout, :, :, 0:3].transpose(2, 3), (0, 1)), F.pad(wf[Cout:, :, :, 1:4].transpose(2, 3), (1, 0))], 0)
        xp = F.pad(x.double().permute(0, 3, 1, 2), (1, 1, 1, 1))
        if self._hit("border_column", w_pair):
            xp[:, :, :, 0] = xp[:, :, :, 1]
        y = F.conv2d(xp, wf, bias_pair.double(), stride=(1, 2))           # [B, 2 Cout, H, W / 2]: pixel o of pair p at channel block o
        y = bf(y.view(B, 2, Cout, H, Wd // 2).permute(0, 3, 4, 1, 2).reshape(B, H, Wd, Cout))
        return self._put(out, self._res(y, res, w_pair))

    def groupnorm_nhwc(self, x, gamma, beta, groups, silu=True, eps=1e-6, out=None):
        B, C = x.shape[0], x.shape[-1]
        x3 = x.reshape(B, -1, C)
        cpg = C // groups
        xg = x3.double().view(B, -1, groups, cpg)
        m = xg.mean((1, 3))
        r = ((xg ** 2).mean((1, 3)) - m * m + float(torch.tensor(eps, dtype=torch.float32))) ** -0.5
        if self._hit("gn_neighbour_stats", gamma):
            m[:, 1], r[:, 1] = m[:, 0], r[:, 0]
        ex = lambda t: t.float().repeat_interleave(cpg, 1)[:, None, :]
        y = ((x3.float() - ex(m)) * ex(r) * gamma.float() + beta.float()).to(BF)
        if silu and not self._hit("gn_no_silu", gamma):
            y = bf(X.silu64(y))
        return self._put(out, y.view(x.shape))

    def gemm(self, a, w, bias=None, out=None, epilogue=0, gelu_from_col=0, gate=None, res=None, variant=-1, workspace=None, cscale=None):
        assert epilogue in (EPI_PLAIN, EPI_GELU, EPI_RES) and gate is None and cscale is None
        if "conv_shortcut" in "".join(self.labels(w)):
            self._shortcut_in = a
        w64 = w.double()
        if self._hit("wi_swapped", w):
            w64 = torch.cat([w64[gelu_from_col:], w64[:gelu_from_col]], 0)
        v = a.double() @ w64.transpose(-1, -2)
        if bias is not None:
            v = v + bias.double()
        if epilogue == EPI_RES and self._hit("stream_not_rounded", w):
            return self._put(out, bf(res.double() + v))
        return self._put(out, X.chain(epilogue, bf(v), res=res, gelu_from_col=gelu_from_col))

    def gemm_f32(self, a, w, out=None):
        return self._put(out, (a.double() @ w.double().transpose(-1, -2)).float())

    def row_softmax(self, s, scale, out):
        self._softmax_calls += 1
        if self._hit("stale_ragged_weights") and self._softmax_calls > 1:
            return out                                                   # the ragged chunk's launches do nothing: the buffer keeps the previous chunk's weights
        if self._hit("softmax_scale"):
            scale = scale * scale
        N = s.shape[1]
        out[:, :N] = X.softmax_rows64(s, scale)
        if self._hit("pad_weight") and out.shape[1] > N:
            out[0, N] = 2.0 ** -6
        return out

    def transpose(self, x, out=None):
        return self._put(out, x.transpose(1, 2).contiguous())

    def blend_edge_nhwc_(self, a, b, extent, axis):
        (vo._blend_v if axis == 1 else vo._blend_h)(a.permute(0, 3, 1, 2), b.permute(0, 3, 1, 2), extent)
        return b

    def rmsnorm(self, x, w, eps, out=None):
        r = ((x.double() ** 2).mean(-1, keepdim=True) + eps) ** -0.5
        return self._put(out, X.t5_rmsnorm_chain(x, w, r.float()))

    def layernorm(self, x, gamma, beta, eps=1e-5, out=None):
        m = x.double().mean(-1, keepdim=True)
        r = (((x.double() - m) ** 2).mean(-1, keepdim=True) + eps) ** -0.5
        return self._put(out, ((x.float() - m.float()) * r.float() * gamma.float() + beta.float()).to(BF))

    def attention64(self, q, k, v, scale, rel_bias=None, causal=False, out=None):
        B, N, HD = q.shape
        H = HD // 64
        qh, kh, vh = (t.double().view(B, N, H, 64).transpose(1, 2) for t in (q, k, v))
        s = qh @ kh.transpose(-1, -2) * scale
        if rel_bias is not None:
            idx = torch.arange(N)[None, :] - torch.arange(N)[:, None] + N - 1
            s = s + rel_bias.double()[:, idx]
        if causal:
            s = s + torch.full((N, N), -math.inf, dtype=torch.float64).triu(2 if self._hit("causal_plus_one") else 1)
        p = torch.exp(s - s.max(-1, keepdim=True).values)
        o = (p.float().to(BF).double() @ vh) / p.sum(-1, keepdim=True)
        return self._put(out, bf(o.transpose(1, 2).reshape(B, N, HD)))

    def gather_rows(self, table, ids, out=None):
        ids = ids.reshape(-1)
        if self._hit("pos_shifted", table):
            ids = (ids + 1).clamp(max=table.shape[0] - 1)
        return self._put(out, table[ids].clone())

    def add(self, a, b):
        return a + b

    def mul(self, a, b, out=None):
        return self._put(out, a * b)

    def quick_gelu(self, a, out=None):
        return self._put(out, X.quick_gelu_chain(a))


# ------------------------------------------------------------------------------------------------------------------ the cases of both test files
VAE_KW = dict(block_out_channels=(64, 128, 128), layers_per_block=1, latent_channels=16, norm_num_groups=16)
VAE_CHUNK_KW = dict(block_out_channels=(64, 128), layers_per_block=1, latent_channels=16, norm_num_groups=16)
VAE_TILED_KW = dict(block_out_channels=(64, 64, 128, 128), layers_per_block=1, latent_channels=16, norm_num_groups=16)
#            name: (config, x NCHW shape, z NCHW shape or None, ATTEND_CHUNK_BYTES or None, chunk plan of the encoder's attention)
VAE_CASES = {
    "even": (VAE_KW, (2, 3, 48, 40), (2, 16, 12, 10), None, [(120, 2)]),            # N = 120 < 256 rows: one ragged chunk, a launch per image
    "odd": (VAE_KW, (1, 3, 24, 20), (1, 16, 5, 3), None, [(30, 1)]),                # level widths 20, 10, 5
    "chunks": (VAE_CHUNK_KW, (2, 3, 40, 30), None, 1 << 20, [(256, 1), (44, 2)]),   # 300 tokens: a full chunk, then a ragged one
}
VAE_TILED_CASE = (VAE_TILED_KW, 32, (1, 3, 40, 56), (1, 16, 5, 7))
T5_CFG = dict(d_model=128, d_kv=64, num_heads=2, d_ff=192, num_layers=2, vocab_size=100, feed_forward_proj="gated-gelu")
CLIP_CFG = dict(vocab_size=120, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2,
                max_position_embeddings=77, hidden_act="quick_gelu", eos_token_id=2)
CLIP_EOS = (76, 40, 5)


def rnd(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def image8(shape, seed):
    """[B, H, W, 8] NHWC bf16: what tfx_prep_image hands the encoder (three image channels in [-1, 1], five of zeros)."""
    B, C, H, W = shape
    x8 = torch.zeros(B, H, W, 8, dtype=BF)
    x8[..., :C] = rnd(shape, seed).clamp(-1, 1).permute(0, 2, 3, 1).to(BF)
    return x8


def latent(shape, seed):
    return rnd(shape, seed).permute(0, 2, 3, 1).contiguous().to(BF)


def _seeded(shapes, seed, std=0.02):
    g = torch.Generator().manual_seed(seed)
    return {k: ((1.0 + 0.1 * r) if ("layer_norm" in k and k.endswith("weight")) else std * r)
            for k, s in shapes.items() for r in (torch.randn(s, generator=g),)}


def t5_state_dict(seed=5, buckets=32):
    c = T5_CFG
    D, inner, dff = c["d_model"], c["num_heads"] * 64, c["d_ff"]
    shapes = {"shared.weight": (c["vocab_size"], D), "encoder.final_layer_norm.weight": (D,),
              "encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight": (buckets, c["num_heads"])}
    for i in range(c["num_layers"]):
        p = f"encoder.block.{i}.layer."
        for n in "qkv":
            shapes[p + f"0.SelfAttention.{n}.weight"] = (inner, D)
        shapes[p + "0.SelfAttention.o.weight"] = (D, inner)
        shapes[p + "0.layer_norm.weight"] = shapes[p + "1.layer_norm.weight"] = (D,)
        shapes[p + "1.DenseReluDense.wi_0.weight"] = shapes[p + "1.DenseReluDense.wi_1.weight"] = (dff, D)
        shapes[p + "1.DenseReluDense.wo.weight"] = (D, dff)
    sd = _seeded(shapes, seed, std=0.05)
    sd["shared.weight"] = sd["shared.weight"] * 20                       # unit-scale embeddings
    sd["encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"] *= 20
    return sd


def clip_state_dict(seed=7):
    c = CLIP_CFG
    D, I, T = c["hidden_size"], c["intermediate_size"], c["max_position_embeddings"]
    shapes = {"text_model.embeddings.token_embedding.weight": (c["vocab_size"], D), "text_model.embeddings.position_embedding.weight": (T, D),
              "text_model.final_layer_norm.weight": (D,), "text_model.final_layer_norm.bias": (D,)}
    for i in range(c["num_hidden_layers"]):
        l = f"text_model.encoder.layers.{i}."
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            shapes[l + f"self_attn.{n}.weight"], shapes[l + f"self_attn.{n}.bias"] = (D, D), (D,)
        for n in ("layer_norm1", "layer_norm2"):
            shapes[l + n + ".weight"], shapes[l + n + ".bias"] = (D,), (D,)
        shapes[l + "mlp.fc1.weight"], shapes[l + "mlp.fc1.bias"] = (I, D), (I,)
        shapes[l + "mlp.fc2.weight"], shapes[l + "mlp.fc2.bias"] = (D, I), (D,)
    sd = _seeded(shapes, seed, std=0.05)
    sd["text_model.embeddings.token_embedding.weight"] *= 20
    return sd


def clip_ids(seed=8):
    V, T = CLIP_CFG["vocab_size"], CLIP_CFG["max_position_embeddings"]
    ids = torch.randint(0, V - 1, (len(CLIP_EOS), T), generator=torch.Generator().manual_seed(seed))
    for b, e in enumerate(CLIP_EOS):
        ids[b, e] = V - 1
    return ids


def t5_ids(T, seed=6):
    return torch.randint(0, T5_CFG["vocab_size"], (2, T), generator=torch.Generator().manual_seed(seed))


def t5_oracle_cfg(buckets=32, max_distance=128):
    c = T5_CFG
    return to.T5Cfg(d_model=c["d_model"], d_kv=64, num_heads=c["num_heads"], d_ff=c["d_ff"], num_layers=c["num_layers"],
                    relative_attention_num_buckets=buckets, relative_attention_max_distance=max_distance)


def clip_oracle_cfg():
    c = CLIP_CFG
    return to.ClipCfg(hidden_size=c["hidden_size"], num_attention_heads=c["num_attention_heads"], intermediate_size=c["intermediate_size"],
                      num_hidden_layers=c["num_hidden_layers"])


# -- one run + walk per model: shared by the CPU file (engine = an EmuOps, device "cpu") and the GPU file (engine = the real ops, "cuda")
def run_vae(monkeypatch, engine, device, kw, sd, end, x, chunk_bytes=None, pair_convs=True, tiling=None):
    import textflux_amd.vae as vae_mod
    vae = vae_mod.AutoencoderKL(**kw, **({"sample_size": tiling} if tiling else {}))
    vae.pair_convs = pair_convs
    vae.load_state_dict(sd, device=device)
    if chunk_bytes:
        vae.ATTEND_CHUNK_BYTES = chunk_bytes
    if tiling:
        vae.enable_tiling()
    rec = install(monkeypatch, vae_mod, engine, vae_weights(vae))
    fn = vae.encode_moments_nhwc if end == "encoder" else vae.decode_nhwc
    out = fn(x.to(device)).cpu()
    return rec.trace, out


def run_t5(monkeypatch, engine, device, sd, ids, cfg_extra=None, table_fault=None):
    import textflux_amd.text_encoders as te
    m = te.T5EncoderModel({**T5_CFG, **(cfg_extra or {})}).load_state_dict(sd, device=device)
    if table_fault is not None:
        m._bias_tables[ids.shape[1]] = table_fault(m._rel_bias(ids.shape[1]))
    rec = install(monkeypatch, te, engine, text_weights(m))
    return rec.trace, m(ids.to(device))[0].cpu()


def run_clip(monkeypatch, engine, device, sd, ids):
    import textflux_amd.text_encoders as te
    m = te.CLIPTextModel(CLIP_CFG).load_state_dict(sd, device=device)
    rec = install(monkeypatch, te, engine, text_weights(m))
    r = m(ids.to(device))
    return rec.trace, r.last_hidden_state.cpu(), r.pooler_output.cpu()


def format_stats(stats: dict) -> str:
    rows = [f"  {k:14s} nodes {s['nodes']:4d}  elements {s['elements']:9d}  off the ideal value {s['off']:7d}  room "
            + ("-" if s["room"] is None else f"{s['room']:.3f}") for k, s in sorted(stats.items())]
    return "\n".join(rows)
