"""Read-back on the device: the fp32 kernels of the text recogniser (ocr.hip), the CTC decode / loss, the whole model and the driver.

Three kinds of check, none with a fitted tolerance:
  * bit-exact against torch on the CPU on inputs whose every partial sum is an integer below 2^24 (activations in [-8, 8], weights and
    biases in [-4, 4], K <= 9216: 9216 * 32 < 2^24), so the summation order cannot matter;
  * derived windows (tests/helpers/ocr_ref.py: u = 2^-23 per operation through each kernel's stated operation order) around fp64
    computed from the device's own inputs;
  * exact integers (arg-max with planted ties, greedy ids, time indices, counts) against numpy on the device's own logits.
The whole model is additionally held to the reference: its logits on the five fixture crops lie within four times the reference's own
fp32-against-fp64 distance (tests/golden/g19_ocr.safetensors) of the reference's fp64 logits."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import ocr_ref as X

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EN_DICT = os.path.join(REPO, "tests", "golden", "en_dict.txt")
F32 = torch.float32
ACTS = {None: lambda t: t, "relu": F.relu, "hard_swish": lambda t: t * F.relu6(t + 3.0) / 6.0, "hard_sigmoid": lambda t: F.relu6(t + 3.0) / 6.0}


@pytest.fixture(scope="module")
def ops():
    from textflux_amd import ops as o
    return o


@pytest.fixture(scope="module")
def fx(golden):
    return golden("g19_ocr")


def ints(key, shape, lo, hi):
    return torch.from_numpy(X._ints(key, shape, lo, hi + 1)).float()


def inside(dev, y, e, what):
    d = (dev.detach().cpu().double() - y).abs()
    bad = d > e
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} outside the window, worst {float((d - e).max()):.3e} over it (|y| max {float(y.abs().max()):.3e})"


# --------------------------------------------------------------------------------------------------------------- bit-exact on integers
CONVS = [(3, 16, 3, (2, 2), 5, 7, 2), (16, 32, 1, (1, 1), 3, 5, 1), (512, 64, 3, (1, 1), 1, 5, 2), (1024, 64, 3, (1, 1), 1, 3, 2)]


@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("case", CONVS, ids=lambda c: f"{c[0]}-{c[1]}-k{c[2]}")
def test_conv_f32_is_bit_exact_on_integer_inputs(ops, case, act):
    cin, cout, k, stride, H, W, B = case
    x, w, b = ints(f"cx{case}", (B, H, W, cin), -8, 8), ints(f"cw{case}", (cout, k, k, cin), -4, 4), ints(f"cb{case}", (cout,), -4, 4)
    want = ACTS[act](F.conv2d(x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), b, stride=stride, padding=k // 2)).permute(0, 2, 3, 1)
    got = ops.ocr_conv_f32(x.cuda(), w.cuda(), b.cuda(), stride=stride, act=act)
    assert got.shape == want.shape and torch.equal(got.cpu(), want.contiguous())


@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("mnk", [(2, 64, 256), (10, 360, 120), (5, 97, 64), (3, 6625, 64)], ids=str)
def test_linear_is_bit_exact_on_integer_inputs(ops, mnk, act):
    M, N, K = mnk
    x, w, b = ints(f"lx{mnk}", (M, K), -8, 8), ints(f"lw{mnk}", (N, K), -4, 4), ints(f"lb{mnk}", (N,), -4, 4)
    got = ops.ocr_linear(x.cuda(), w.cuda(), b.cuda(), act=act)
    assert torch.equal(got.cpu(), ACTS[act](F.linear(x, w, b)))
    got = ops.ocr_linear(x.cuda(), w.cuda(), None, act=act)         # without a bias
    assert torch.equal(got.cpu(), ACTS[act](F.linear(x, w)))


def test_conv_writes_at_a_channel_offset_and_leaves_the_rest(ops):
    """the neck's free concat: Cout = 40 columns at offset 24 of a 72-wide buffer, read from the first 16 of 20 input channels"""
    B, H, W, cin, cout = 2, 3, 5, 16, 40
    x, w, b = ints("ox", (B, H, W, 20), -8, 8), ints("ow", (cout, 3, 3, cin), -4, 4), ints("ob", (cout,), -4, 4)
    buf = torch.full((B, H, W, 72), -777.0, device="cuda")
    out = ops.ocr_conv_f32(x.cuda(), w.cuda(), b.cuda(), act="relu", cin=cin, out=buf, co_off=24)
    assert out.data_ptr() == buf.data_ptr()
    want = F.relu(F.conv2d(x[..., :cin].permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), b, padding=1)).permute(0, 2, 3, 1)
    got = buf.cpu()
    assert torch.equal(got[..., 24:64], want.contiguous())
    assert bool((got[..., :24] == -777.0).all()) and bool((got[..., 64:] == -777.0).all())


@pytest.mark.parametrize("act", ["hard_swish", "hard_sigmoid"])
def test_knees_of_the_hard_activations(ops, act):
    """rows through an identity weight: -3 and 3 themselves, their fp32 neighbours, and values whose product is no multiple of 6"""
    v = [-3.0, 3.0, -4.0, 4.0, 0.0, -0.0, 1.0, -1.0, 2.5, -2.5, 0.1, 7.3]
    v += [float(np.nextafter(np.float32(s), np.float32(t))) for s in (-3.0, 3.0) for t in (-10.0, 10.0)]
    x = torch.tensor(v, dtype=F32).view(2, 8)
    got = ops.ocr_linear(x.cuda(), torch.eye(8).cuda(), None, act=act)
    assert torch.equal(got.cpu(), ACTS[act](x))


@pytest.mark.parametrize("C", [8, 260])
@pytest.mark.parametrize("k", [3, 5])
def test_conv_dw_is_bit_exact_on_integer_inputs(ops, k, C):
    """every stride pair at 3 x 5 (with k = 5 the padding is wider than the image) and 6 x 9, with and without hard-swish"""
    for H, W in ((3, 5), (6, 9)):
        x, w, b = ints(f"dx{H}{C}", (2, H, W, C), -8, 8), ints(f"dw{k}{C}", (k, k, C), -4, 4), ints(f"db{C}", (C,), -4, 4)
        xg, wg, bg = x.cuda(), w.cuda(), b.cuda()
        for stride in ((1, 1), (2, 1), (1, 2), (2, 2)):
            for act in (None, "hard_swish"):
                pre = F.conv2d(x.permute(0, 3, 1, 2), w.permute(2, 0, 1).unsqueeze(1), b, stride=stride, padding=k // 2, groups=C)
                want = ACTS[act](pre).permute(0, 2, 3, 1).contiguous()
                got = ops.ocr_conv_dw(xg, wg, bg, stride=stride, act=act)
                assert got.shape == want.shape and torch.equal(got.cpu(), want), (H, W, stride, act)


@pytest.mark.parametrize("hw", [(3, 5), (4, 6), (1, 1)])
def test_pools_and_channel_scale_are_bit_exact(ops, hw):
    H, W = hw
    x = ints(f"px{hw}", (2, H, W, 12), -8, 8)
    got = ops.ocr_pool_mean(x.cuda())
    assert torch.equal(got.cpu(), x.sum((1, 2)) / float(H * W))       # a fixed-order sum, then ONE division
    s = ints(f"ps{hw}", (2, 12), -4, 4)
    assert torch.equal(ops.ocr_scale_channels(x.cuda(), s.cuda()).cpu(), x * s[:, None, None, :])
    if H >= 2:
        want = F.avg_pool2d(x.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1).contiguous()
        assert torch.equal(ops.ocr_pool_2x2(x.cuda()).cpu(), want)
        buf = torch.full((2, H // 2, W // 2, 30), 5.0, device="cuda")
        ops.ocr_pool_2x2(x.cuda(), out=buf)
        assert torch.equal(buf[..., :12].cpu(), want) and bool((buf[..., 12:] == 5.0).all())


# --------------------------------------------------------------------------------------------------------------------- derived windows
def pack(crops, turns=None):
    table, off = [], 0
    for i, c in enumerate(crops):
        h, w = c.shape[:2]
        table.append((off, h, w, int(h > w * 1.2) if turns is None else turns[i]))
        off += h * w * 3
    return torch.from_numpy(np.concatenate([c.reshape(-1) for c in crops])).cuda(), torch.tensor(table, dtype=torch.int32).cuda()


def test_resize_norm_windows_on_the_fixture_crops(ops, fx):
    crops = X.fixture_crops()
    got = ops.ocr_resize_norm(*pack(crops), 48, 320)
    assert got.shape == (5, 48, 320, 3)
    for i, c in enumerate(crops):
        y, e = X.resize_norm_win(c, 48, 320)
        inside(got[i], y, e, f"crop {i} {c.shape}")
    assert bool((got[2, :, 48:] == 0.0).all()) and bool((got[0, :, -1].abs() > 0).any())     # 17 x 17 fills 48 columns; the wide one all 320
    # the reference's own fp32 batch (a strided sample is stored) lies in the same windows, so the two agree to twice the window
    flat = got.cpu().reshape(-1)
    step = max(1, flat.numel() // 2048)
    assert float((flat[::step][:2048] - fx["crops.norm"]).abs().max()) <= 2 * 2.0 * X.U * (2 * (300 + 90) + 10)


def test_resize_norm_edges(ops):
    """resized_w == 1 (the un-turned 96 x 2 crop), source size == target size (bit-exact: every weight is 0 or 1), a table entry that
    leaves the buffer (zeros, nothing read)"""
    thin = X._ints("thin", (96, 2, 3), 0, 256).astype(np.uint8)
    same = X._ints("same", (48, 64, 3), 0, 256).astype(np.uint8)
    buf, table = pack([thin, same], turns=[0, 0])
    got = ops.ocr_resize_norm(buf, table, 48, 64)
    a = torch.from_numpy(thin).double()
    ys = torch.arange(48, dtype=torch.float64) * (95 / 47)
    y0 = ys.floor().long()
    col = a[y0, 0] * (1 - (ys - y0)).view(-1, 1) + a[(y0 + 1).clamp(max=95), 0] * (ys - y0).view(-1, 1)
    inside(got[0, :, 0], (col / 255 - 0.5) / 0.5, torch.full((48, 3), 2 * X.U * (2 * 95 + 8) + 4 * X.U, dtype=torch.float64), "resized_w == 1")
    assert bool((got[0, :, 1:] == 0.0).all())
    s = torch.from_numpy(same).float()
    assert torch.equal(got[1].cpu(), (s / 255.0 - 0.5) / 0.5)
    bad = table.clone()
    bad[1, 0] = buf.numel() - 10
    assert bool((ops.ocr_resize_norm(buf, bad, 48, 64)[1] == 0.0).all())


def test_swish_window(ops):
    x = (ints("sw", (6, 8), -2000, 2000) / 100.0)
    got = ops.ocr_linear(x.cuda(), torch.eye(8).cuda(), None, act="swish")
    y, e = X.conv_win(x.view(6, 1, 1, 8), torch.eye(8).view(8, 1, 1, 8), None, act="swish")
    inside(got, y.view(6, 8), e.view(6, 8), "swish")


@pytest.mark.parametrize("eps", [1e-5, 1e-6])
def test_layernorm_window(ops, eps):
    x = ints("lnx", (7, 120), -3000, 3000) / 1000.0
    x[3] = x[3] * 1e-3 + 5.0                                            # a nearly constant row: eps matters
    g, b = ints("lng", (120,), 50, 150) / 100.0, ints("lnb", (120,), -50, 50) / 100.0
    got = ops.ocr_layernorm(x.cuda(), g.cuda(), b.cuda(), eps)
    inside(got, *X.layernorm_win(x, g, b, eps), f"layernorm eps {eps}")


@pytest.mark.parametrize("shape", [(2, 1, 8, 15), (2, 5, 8, 15), (2, 40, 8, 15), (1, 160, 8, 15), (1, 256, 2, 32)], ids=str)
def test_attention_window(ops, shape):
    B, N, H, d = shape
    qkv = ints(f"att{shape}", (B, N, 3 * H * d), -2000, 2000) / 1000.0
    if N > 1:                                                           # one row with one dominant score: the softmax is nearly one-hot
        qkv[0, 0, :d] = 6.0
        qkv[0, N - 1, H * d:H * d + d] = 6.0
    got = ops.ocr_attention(qkv.cuda(), H)
    inside(got, *X.attention_win(qkv, H), f"attention {shape}")


@pytest.mark.parametrize("C", [97, 6625])
def test_ctc_rows_exact_argmax_with_ties_and_lse_window(ops, C):
    x = ints(f"rows{C}", (7, C), -9000, 9000) / 1000.0
    x[0, 5] = x[0, 60] = 12.0                                           # ties: the first index wins ...
    x[1, 44] = x[1, min(C - 1, 300)] = 12.0                             # ... across the threads' strides
    x[2, C - 1] = 12.0
    x[3, 0] = x[3, C - 1] = 12.0
    x[4] = 0.25                                                         # all equal: index 0
    mx, arg, lse = ops.ctc_rows(x.cuda())
    wmx, warg, wlse, e = X.ctc_rows_win(x)
    assert torch.equal(mx.cpu().double(), wmx) and arg.cpu().tolist() == x.numpy().argmax(axis=1).tolist() == warg.tolist()
    assert arg.cpu().tolist()[:5] == [5, 44, C - 1, 0, 0]
    inside(lse, wlse, e, f"lse C {C}")


def score_case(T, C, key):
    return ints(key, (4, T, C), -6000, 6000) / 1000.0


def test_ctc_score_decode_is_numpy_on_the_device_logits(ops):
    logits = score_case(40, 97, "dec")
    logits[0, :, 0] += 20.0                                             # all blank: nothing decoded
    logits[1, 3:9, 7] += 20.0                                           # a run of one symbol
    logits[1, 9, 0] += 20.0
    logits[1, 10:12, 7] += 20.0                                         # the same symbol again after a blank
    lg = logits.cuda()
    _, arg, lse = ops.ctc_rows(lg)
    ids, tix, count, loss = ops.ctc_score(lg, arg, lse)
    assert loss is None
    am = lg.cpu().numpy().argmax(axis=2)
    assert torch.equal(arg.cpu(), torch.from_numpy(am).int())
    for i in range(4):
        a, b = X.greedy(am[i])
        n = int(count[i])
        assert n == len(a) and ids[i, :n].cpu().tolist() == a.tolist() and tix[i, :n].cpu().tolist() == b.tolist()
        assert bool((ids[i, n:] == 0).all()) and bool((tix[i, n:] == -1).all())
    assert int(count[0]) == 0


@pytest.mark.parametrize("T", [1, 40, 256])
def test_ctc_loss_window_and_cases(ops, T):
    """-log p inside the recursion's window; +inf, L = 0 and the repeated letter agree as cases with torch's CTCLoss on the CPU"""
    C = 97
    logits = score_case(T, C, f"loss{T}")
    long = min(127, T)
    # a run of one letter needs a blank between every two: [3, 3] cannot be emitted in 1 step, 21 of them not in 40; 127 fit into 256
    run = {1: [3, 3], 40: [3] * 21, 256: [3] * 127}[T]
    targets = [[8, 5, 12, 12, 15][:max(1, min(5, (T + 1) // 2))], [], run, [int(v) for v in X._ints("tg", (long,), 1, C)]]
    lg = logits.cuda()
    _, arg, lse = ops.ctc_rows(lg)
    _, _, _, loss = ops.ctc_score(lg, arg, lse, targets)
    loss = loss.cpu()
    lp = logits.double().log_softmax(-1).permute(1, 0, 2)
    want = F.ctc_loss(lp, torch.tensor(sum(targets, []), dtype=torch.long), torch.full((4,), T, dtype=torch.long),
                      torch.tensor([len(t) for t in targets]), reduction="none")
    for i, t in enumerate(targets):
        y, e = X.ctc_loss_win(logits[i], lse[i].cpu(), t)
        assert np.isinf(y) == bool(torch.isinf(want[i])), (i, y, float(want[i]))
        if np.isinf(y):
            assert torch.isinf(loss[i]) and loss[i] > 0                 # [3] * (T // 2 + 1) needs T + 1 steps
            continue
        exact = X.ctc_loss_win(logits[i], logits[i].double().logsumexp(-1), t)[0]
        assert abs(exact - float(want[i])) <= 1e-9 * max(1.0, abs(exact))       # the restatement and torch's fp64 recursion: the same quantity
        assert abs(float(loss[i]) - y) <= e, (T, i, float(loss[i]), y, e)
    assert bool(torch.isinf(loss[2])) == (T != 256) and torch.isfinite(loss[1])
    with pytest.raises(ValueError, match="127"):
        ops.ctc_score(lg, arg, lse, [[1] * 128, [], [], []])
    with pytest.raises(ValueError, match="outside"):
        ops.ctc_score(lg, arg, lse, [[C], [], [], []])


def test_entry_points_refuse_nulls_and_unsupported_shapes(ops):
    from textflux_amd import _lib as L
    lib = L.lib()
    assert lib.tfx_ocr_conv_f32(None, None, None, None, 1, 1, 1, 4, 4, 1, 1, 1, 0, 4, 4, 0, None) != 0 and b"null" in lib.tfx_last_error()
    x = torch.zeros(1, 4, 4, 8, device="cuda")
    p = x.data_ptr()
    assert lib.tfx_ocr_conv_f32(p, p, None, p, 1, 4, 4, 8, 8, 5, 1, 1, 0, 8, 8, 0, None) != 0 and b"1 x 1 or 3 x 3" in lib.tfx_last_error()
    assert lib.tfx_ocr_conv_f32(p, p, None, p, 1, 4, 4, 8, 8, 1, 1, 1, 0, 8, 8, 4, None) != 0 and b"ldo" in lib.tfx_last_error()
    assert lib.tfx_ocr_conv_dw(p, p, None, p, 1, 4, 4, 6, 3, 1, 1, 0, None) != 0 and b"multiple of 4" in lib.tfx_last_error()
    assert lib.tfx_ocr_conv_dw(p, p, None, p, 1, 4, 4, 8, 3, 3, 1, 0, None) != 0 and b"strides" in lib.tfx_last_error()
    assert lib.tfx_ocr_attention(p, p, 1, 257, 1, 8, 1.0, None) != 0 and lib.tfx_ocr_attention(p, p, 1, 4, 1, 33, 1.0, None) != 0
    assert lib.tfx_ocr_layernorm(p, 8, p, 8, p, p, 1, 513, 1e-5, None) != 0
    assert lib.tfx_ctc_score(p, p, p, p, p, 0, 1, 257, 4, p, p, p, p, None) != 0 and b"T <= 256" in lib.tfx_last_error()
    assert lib.tfx_ctc_rows(None, 4, 1, 4, p, p, p, None) != 0 and lib.tfx_ocr_pool(p, p, 1, 1, 4, 8, 1, 8, None) != 0
    assert lib.tfx_ocr_scale_channels(p, p, p, 1, 16, 6, None) != 0 and lib.tfx_ocr_resize_norm(p, 16, None, p, 1, 48, 64, None) != 0


# ------------------------------------------------------------------------------------------------------------------------ whole model
class Recorder:
    """textflux_amd.ops behind a recorder: every tensor a call is handed that an earlier call produced must still hold exactly what
    that call left there, and every output must lie inside the window computed in fp64 from the inputs the call was handed."""

    def __init__(self, ops):
        self.ops, self.made, self.calls = ops, {}, 0      # made: data_ptr -> (the output itself, its bits when the call returned)

    def _made(self, out):
        # the output is kept alive with its snapshot: a freed buffer's address would be handed out again, to a tensor no call produced
        self.made[out.data_ptr()] = (out, out.detach().clone())

    def _handed(self, t):
        if isinstance(t, torch.Tensor) and t.data_ptr() in self.made:
            kept = self.made[t.data_ptr()][1]
            assert kept.numel() == t.numel() and torch.equal(kept.reshape(-1), t.reshape(-1)), "a call was not handed its predecessor's output"

    def _run(self, name, win, args, kw):
        for t in list(args) + list(kw.values()):
            self._handed(t)
        host = [a.detach().cpu().clone() if isinstance(a, torch.Tensor) else a for a in args]
        hkw = {k: (v.detach().cpu().clone() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}
        out = getattr(self.ops, name)(*args, **kw)
        y, e = win(*host, **hkw)
        inside(out, y, e, f"call {self.calls} {name}")
        self._made(out)
        self.calls += 1
        return out

    def ocr_conv_f32(self, x, w, b, stride=(1, 1), act=None, cin=None, out=None, co_off=0):
        def win(x, w, b, out=None):
            y, e = X.conv_win(x, w, b, stride, act)
            if out is None:
                return y, e
            full, fe = out.double().clone(), torch.zeros(out.shape, dtype=torch.float64)       # the columns beside the result: unchanged
            full[..., co_off:co_off + y.shape[3]], fe[..., co_off:co_off + y.shape[3]] = y, e
            return full, fe
        for t in (x, out):
            self._handed(t)
        hx, hw, hb, hout = x.cpu().clone(), w.cpu(), b.cpu(), None if out is None else out.cpu().clone()
        res = self.ops.ocr_conv_f32(x, w, b, stride=stride, act=act, cin=cin, out=out, co_off=co_off)
        y, e = win(hx, hw, hb, out=hout)
        inside(res, y, e, f"call {self.calls} ocr_conv_f32")
        self._made(res)
        self.calls += 1
        return res

    def ocr_linear(self, x, w, b, act=None):
        return self._run("ocr_linear", lambda x, w, b, act=None: tuple(t.view(x.shape[0], w.shape[0]) for t in X.conv_win(
            x.view(x.shape[0], 1, 1, -1), w.view(w.shape[0], 1, 1, -1), b, act=act)), (x, w, b), dict(act=act))

    def ocr_conv_dw(self, x, w, b, stride=(1, 1), act=None):
        return self._run("ocr_conv_dw", X.dw_win, (x, w, b), dict(stride=stride, act=act))

    def ocr_pool_mean(self, x):
        return self._run("ocr_pool_mean", X.pool_mean_win, (x,), {})

    def ocr_pool_2x2(self, x, out=None):
        def win(x, out):
            y, e = X.pool_2x2_win(x)
            full, fe = out.double().clone(), torch.zeros(out.shape, dtype=torch.float64)
            full[..., :y.shape[3]], fe[..., :y.shape[3]] = y, e
            return full, fe
        return self._run("ocr_pool_2x2", win, (x,), dict(out=out))

    def ocr_scale_channels(self, x, s):
        return self._run("ocr_scale_channels", X.scale_win, (x, s), {})

    def ocr_layernorm(self, x, g, b, eps):
        return self._run("ocr_layernorm", X.layernorm_win, (x, g, b, eps), {})

    def ocr_add_(self, x, y):
        return self._run("ocr_add_", X.add_win, (x, y), {})

    def ocr_attention(self, qkv, heads):
        return self._run("ocr_attention", X.attention_win, (qkv, heads), {})


@pytest.fixture(scope="module")
def model(ops):
    from textflux_amd import ocr as O
    return O.RecModel(X.seeded_state(97), 97)


def test_whole_model_every_call_in_its_window_and_handed_its_predecessors(ops, model):
    from textflux_amd import ocr as O
    rec = Recorder(ops)
    traced = O.RecModel(X.seeded_state(97), 97, ops=rec)
    x = X.node_input().permute(0, 2, 3, 1).contiguous().cuda()
    out = traced(x)
    assert rec.calls == 1 + 13 + 13 + 2 * 4 + 1 + 5 + 2 * 9 + 1 + 1 and out["ctc"].shape == (2, 8, 97)
    again = model(x)
    assert torch.equal(again["ctc"], out["ctc"]) and torch.equal(again["ctc_neck"], out["ctc_neck"])     # the recorder changed nothing


@pytest.fixture(scope="module")
def reader(model):
    from textflux_amd import ocr as O
    return O.TextRecognizer(model, EN_DICT, (3, 48, 320), 6)


def test_whole_model_on_the_fixture_crops(ops, fx, reader):
    ctc, neck = reader.pred_imglist(X.fixture_crops())
    margin = 4 * float(fx["crops.ref_fp32_distance"])                   # the reference is the yardstick, not the code under test
    print(f"logit distance {float((ctc.cpu().double() - fx['crops.ctc']).abs().max()):.3e} of margin {margin:.3e}")
    assert ctc.shape == (5, 40, 97) and neck.shape == (5, 40, 64)
    assert float((ctc.cpu().double() - fx["crops.ctc"]).abs().max()) <= margin
    for i in range(5):
        ids, tix = reader.decode(ctc[i])
        n = int(fx["crops.count"][i])
        assert list(ids) == fx["crops.ids"][i, :n].tolist() and list(tix) == fx["crops.time_index"][i, :n].tolist()
    loss = reader.get_ctcloss(ctc, X.TARGETS, np.ones(5))
    _, _, lse = ops.ctc_rows(ctc.contiguous())
    for i, t in enumerate(X.TARGETS):
        y, e = X.ctc_loss_win(ctc[i].cpu(), lse[i].cpu(), reader.text_ids(t))
        if np.isinf(y):
            assert i == 3 and torch.isinf(loss[i]) and loss[i] > 0 and torch.isinf(fx["crops.ctcloss"][i])
        else:
            assert abs(float(loss[i]) * 40 - y) <= e + 2 * X.U * abs(y), (i, float(loss[i]), y / 40, e)      # / T and back: two roundings
            assert abs(float(loss[i]) - float(fx["crops.ctcloss"][i])) <= 2 * margin
    ctc2, neck2 = reader.pred_imglist(X.fixture_crops())
    assert torch.equal(ctc, ctc2) and torch.equal(neck, neck2)          # two runs, equal bits


# ----------------------------------------------------------------------------------------------------------------------------- driver
@pytest.fixture(scope="module")
def pipe(tmp_path_factory):
    import run_inference as ri
    from tests.helpers import tiny_checkpoint as tc
    root = str(tmp_path_factory.mktemp("flux_fill_dev_ocr"))
    tc.write_pipeline_dir(root)
    saved = ri.BASE, ri.TRANSFORMER, ri.PIPE
    ri.BASE, ri.TRANSFORMER, ri.PIPE = root, os.path.join(root, "transformer"), None
    p = ri.load_flux_pipeline()
    ri.BASE, ri.TRANSFORMER, ri.PIPE = saved
    return p


def test_run_items_reads_back_an_eval_item_with_two_annotations(pipe, tmp_path):
    """records of the stated schema for both annotations (the second one slanted), from the pipeline-size result and from the pasted
    scene; without the key the outputs are bit-equal and nothing about read-back appears in the result"""
    from PIL import Image
    from safetensors.torch import save_file
    from textflux_amd import batch_driver, glyph
    weights = str(tmp_path / "rec.safetensors")
    save_file(X.seeded_state(97), weights)
    item = dict(img_name="a.png", annotations=[dict(text="HELLO", polygon=[[40, 30], [200, 30], [200, 70], [40, 70]]),
                                               dict(text="to you", polygon=[[30, 90], [180, 100], [178, 125], [28, 115]])])
    scene = Image.fromarray(np.random.default_rng(7).integers(0, 256, (140, 250, 3), dtype=np.uint8))
    cfg = dict(original_images_dir="imgs", font=glyph.load_font(None), text_height_ratio=0.1667)

    def run(**kw):
        saved = {}
        res = batch_driver.run_items([item], pipe, None, batch_size=2, num_inference_steps=2, guidance_scale=30.0, seed=42,
                                     loader=lambda p: scene, eval_cfg=cfg, save_full=lambda w, full, crop: saved.update(full=np.array(full), crop=np.array(crop)), **kw)
        assert res["all_done"] == [0] and not res["failed"]
        return res, saved

    ocr = dict(weights=weights, lang="en", dict_path=EN_DICT)
    for paste in (None, dict(dilate=8, feather=2)):
        kw = {} if paste is None else dict(paste_back=paste)
        off, img_off = run(**kw)
        on, img_on = run(ocr=ocr, **kw)
        assert "ocr" not in off and (img_on["full"] == img_off["full"]).all() and (img_on["crop"] == img_off["crop"]).all()
        recs = on["ocr"][0]
        assert [r["text"] for r in recs] == ["HELLO", "to you"]
        for r in recs:
            assert set(r) == {"text", "pred", "seq_acc", "ned", "ctc_loss"} and isinstance(r["pred"], str)
            assert r["seq_acc"] in (0.0, 1.0) and r["ned"] <= 1.0 and r["ctc_loss"] > 0 and np.isfinite(r["ctc_loss"])
        again, _ = run(ocr=ocr, **kw)
        assert again["ocr"] == on["ocr"]                                # two runs, the same records
    with pytest.raises(ValueError, match="dict_path"):
        batch_driver.run_items([item], pipe, None, ocr=dict(weights=weights, lang="en"))


def test_crop_line_of_an_upright_rectangle_is_the_slice():
    """corners on whole pixels, unit axes: every sample position has a zero fraction, so the warp returns the scene's own bytes"""
    from textflux_amd import ocr as O
    img = torch.from_numpy(np.random.default_rng(3).integers(0, 256, (40, 120, 3), dtype=np.uint8))
    mask = np.zeros((40, 120), np.uint8)
    mask[10:20, 30:90] = 255
    crop = O.crop_line(img.cuda(), mask)
    assert crop.shape == (9, 59, 3) and torch.equal(crop.cpu(), img[10:19, 30:89])       # |tl - tr| = 59, |tl - bl| = 9, truncated as the reference's
    poly = np.array([[30.0, 10.0], [89.0, 10.0], [89.0, 19.0], [30.0, 19.0]])
    assert torch.equal(O.crop_line(img.cuda(), poly).cpu(), crop.cpu())
    with pytest.raises(ValueError, match="empty"):
        O.crop_line(img.cuda(), np.zeros((40, 120), np.uint8))
