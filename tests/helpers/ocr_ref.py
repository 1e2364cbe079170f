"""The read-back recogniser restated in fp64 (tests/test_ocr_cpu.py, tests/test_ocr_gpu.py, tests/golden/make_ocr_goldens.py).

Three things live here:
  * the seeded integer weight recipe (`seeded_state`) and the fixture inputs (`fixture_crops`, `node_input`, `TARGETS`): nothing of
    them is stored, the golden script and the tests call the same functions;
  * `forward64`: the whole model in fp64 on torch's CPU convolutions, node by node, with every trap of the reference available as a
    named wrong variant (`VARIANTS`);
  * the fp64 value AND first-order error window of every device op (`*_win`), from the op's own inputs, and `EmuOps`, an engine with
    the signatures of textflux_amd.ops' ocr_* / ctc_* functions that computes in fp64 on the host.

Windows.  u = 2^-23 per operation, pushed through the operation order each kernel states in include/textflux_hip.h: a sum of K
products with a bias is (K + 2) u sum|a w|; an activation multiplies the incoming error by its Lipschitz constant (hard-swish 1.5,
hard-sigmoid 1 / 6, swish 1.1, relu 1) and adds its own roundings.  None is fitted to what the device gives.
"""
import math
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from textflux_amd import ocr as O

U = 2.0 ** -23
F64 = torch.float64

VARIANTS = ("se_common_hsigmoid", "prenorm_true", "neck_gelu", "se_before_depthwise")
NODES = ["stem"] + [f"block{i}" for i in range(13)] + ["pool", "neck.conv1", "neck.conv2", "svtr0", "svtr1", "neck.norm", "neck.conv3",
                                                        "neck.conv4", "neck.conv1x1", "ctc"]
# where each variant first shows
VARIANT_NODE = {"se_common_hsigmoid": "block11", "prenorm_true": "svtr0", "neck_gelu": "neck.conv1", "se_before_depthwise": "block11"}

TARGETS = ["hello", "", "aéb", "x" * 45, "Zebra 42"]      # a repeated letter, the empty string, an unknown character, longer than T = 40


# ------------------------------------------------------------------------------------------------------------ seeded weights and inputs
def _ints(key: str, shape, lo: int, hi: int) -> np.ndarray:
    return np.random.RandomState(zlib.crc32(key.encode()) & 0x7fffffff).randint(lo, hi, size=shape)


def seeded_state(n_class: int) -> dict:
    """fp32 state dict from integers drawn per key: weights k / 127 * gain / sqrt(fan_in), BatchNorm gamma in [0.75, 1.25), beta, the
    running mean and every bias in [-1 / 16, 1 / 16), the running variance in [0.5, 1.5).  The gain 2.7 sits where the signal neither dies
    out nor blows up over the 28 convolutions (at 2.6 every image decodes alike, at 2.9 the logits reach the hundreds); the head is scaled
    up so that the logits follow the input."""
    sd = {}
    for key, shape in O.state_spec(n_class):
        if key.endswith("running_var"):
            v = 0.5 + _ints(key, shape, 0, 256) / 256.0
        elif key.endswith("running_mean") or (key.endswith(".bias") and len(shape) == 1):
            v = _ints(key, shape, -64, 64) / 1024.0
        elif len(shape) == 1:
            v = 0.75 + _ints(key, shape, 0, 128) / 256.0
        else:
            fan_in = math.prod(shape[1:])
            gain = 24.0 if key.startswith("head.") else (4.0 if ".mixer.qkv." in key else 2.7)
            v = _ints(key, shape, -127, 128) / 127.0 * gain / math.sqrt(fan_in)
        sd[key] = torch.from_numpy(np.asarray(v, dtype=np.float64)).float()
    return sd


def fixture_crops():
    """five uint8 [h, w, 3] line crops of random grey blocks (four pixels wide, a quarter of the height tall) under +-18 of noise: a wide
    one clamped to the full width, a tall one that gets turned, 17 x 17, and two ordinary."""
    sizes = [(24, 300), (90, 30), (17, 17), (32, 100), (48, 131)]
    out = []
    for i, (h, w) in enumerate(sizes):
        ch, cw = max(2, h // 4), 4
        g = _ints(f"crop{i}", ((h + ch - 1) // ch, (w + cw - 1) // cw, 1), 0, 256)
        base = np.kron(g, np.ones((ch, cw, 1)))[:h, :w]
        out.append(np.clip(base + _ints(f"noise{i}", (h, w, 3), -18, 19), 0, 255).astype(np.uint8))
    return out


def node_input(B: int = 2, W: int = 64) -> torch.Tensor:
    """fp32 NCHW [B, 3, 48, W] in [-1, 1]: the input of the per-node fixture."""
    v = _ints("node_input", (B, 3, 48, W), -255, 256) / 255.0
    yy, xx = np.mgrid[0:48, 0:W]
    return torch.from_numpy(0.5 * v + 0.5 * np.sin(xx * 0.4 + yy * 0.2)[None, None]).float()


# --------------------------------------------------------------------------------------------------------------------- fp64 restatement
def hswish(x):
    return (x * F.relu6(x + 3.0)) / 6.0


def hsigmoid(x):
    return F.relu6(x + 3.0) / 6.0


def swish(x):
    return x * torch.sigmoid(x)


def fold64(w, gamma, beta, mean, var, eps=1e-5):
    s = gamma.double() / torch.sqrt(var.double() + eps)
    return w.double() * s.view(-1, 1, 1, 1), beta.double() - mean.double() * s


def forward64(sd: dict, x: torch.Tensor, variant=None, round32: bool = False) -> dict:
    """{node: fp64 NCHW / [B, N, D] output} for x fp32 / fp64 NCHW.  round32: the folded weights are rounded to fp32 first, as the
    product's loader does.  variant: one of VARIANTS."""
    assert variant is None or variant in VARIANTS
    sd = {k: v.double() for k, v in sd.items()}
    rnd = (lambda t: t.float().double()) if round32 else (lambda t: t)

    def conv_bn(p, conv, bn, x, act, stride=1, groups=1):
        w, b = fold64(sd[f"{p}.{conv}.weight"], *(sd[f"{p}.{bn}.{n}"] for n in ("weight", "bias", "running_mean", "running_var")))
        k = w.shape[-1]
        return act(F.conv2d(x, rnd(w), rnd(b), stride=stride, padding=k // 2, groups=groups))

    def se(p, y):
        s = y.mean((2, 3), keepdim=True)
        s = F.relu(F.conv2d(s, sd[p + ".conv1.weight"], sd[p + ".conv1.bias"]))
        s = F.conv2d(s, sd[p + ".conv2.weight"], sd[p + ".conv2.bias"])
        s = F.relu6(1.2 * s + 3.0) / 6.0 if variant == "se_common_hsigmoid" else hsigmoid(s)
        return y * s

    out = {}
    y = out["stem"] = conv_bn("backbone.conv1", "_conv", "_batch_norm", x.double(), hswish, stride=2)
    for i, (c, co, k, stride, has_se) in enumerate(O.BLOCKS):
        p = f"backbone.block_list.{i}"
        if has_se and variant == "se_before_depthwise":
            y = se(p + "._se", y)
        y = conv_bn(p + "._depthwise_conv", "_conv", "_batch_norm", y, hswish, stride=stride, groups=c)
        if has_se and variant != "se_before_depthwise":
            y = se(p + "._se", y)
        y = out[f"block{i}"] = conv_bn(p + "._pointwise_conv", "_conv", "_batch_norm", y, hswish)
    h = out["pool"] = F.avg_pool2d(y, 2, 2)
    e = "neck.encoder"
    nact = (lambda t: F.gelu(t)) if variant == "neck_gelu" else swish
    z = out["neck.conv1"] = conv_bn(e + ".conv1", "conv", "norm", h, nact)
    z = out["neck.conv2"] = conv_bn(e + ".conv2", "conv", "norm", z, nact)
    B, C, H, W = z.shape
    t = z.flatten(2).permute(0, 2, 1)
    D = O.HIDDEN

    def ln(p, t, eps):
        return F.layer_norm(t, (D,), sd[p + ".weight"], sd[p + ".bias"], eps)

    def lin(p, t):
        return F.linear(t, sd[p + ".weight"], sd[p + ".bias"])

    def mixer(p, t):
        N = t.shape[1]
        qkv = lin(p + ".qkv", t).reshape(B, N, 3, O.HEADS, D // O.HEADS).permute(2, 0, 3, 1, 4)
        q, k, v = qkv[0] * (D // O.HEADS) ** -0.5, qkv[1], qkv[2]
        a = torch.softmax(q @ k.transpose(-1, -2), dim=-1)
        return lin(p + ".proj", (a @ v).permute(0, 2, 1, 3).reshape(B, N, D))

    def mlp(p, t):
        return lin(p + ".fc2", swish(lin(p + ".fc1", t)))

    for i in range(O.DEPTH):
        p = f"{e}.svtr_block.{i}"
        if variant == "prenorm_true":
            t = ln(p + ".norm1", t + mixer(p + ".mixer", t), 1e-5)
            t = ln(p + ".norm2", t + mlp(p + ".mlp", t), 1e-5)
        else:
            t = t + mixer(p + ".mixer", ln(p + ".norm1", t, 1e-5))
            t = t + mlp(p + ".mlp", ln(p + ".norm2", t, 1e-5))
        out[f"svtr{i}"] = t
    t = out["neck.norm"] = ln(e + ".norm", t, 1e-6)
    z = t.reshape(B, H, W, D).permute(0, 3, 1, 2)
    z = out["neck.conv3"] = conv_bn(e + ".conv3", "conv", "norm", z, nact)
    z = out["neck.conv4"] = conv_bn(e + ".conv4", "conv", "norm", torch.cat((h, z), dim=1), nact)
    z = out["neck.conv1x1"] = conv_bn(e + ".conv1x1", "conv", "norm", z, nact)
    feats = z.flatten(2).permute(0, 2, 1)
    out["ctc_neck"] = feats
    out["ctc"] = lin("head.fc", feats)
    return out


def resize_norm64(img: np.ndarray, img_h: int, img_w: int, with_pos: bool = False):
    """TextRecognizer's quarter turn + resize_norm_img in fp64 on a uint8 [h, w, 3] crop -> [img_h, img_w, 3] (and the source
    positions' sum fy + fx per pixel, for the window)."""
    a = torch.from_numpy(np.ascontiguousarray(img)).double()
    if a.shape[0] > a.shape[1] * 1.2:
        a = a.permute(2, 0, 1).transpose(1, 2).flip(dims=[1]).permute(1, 2, 0)
    h, w = a.shape[:2]
    rw = min(img_w, int(math.ceil(img_h * (w / float(h)))))
    ys = torch.arange(img_h, dtype=F64) * ((h - 1) / (img_h - 1) if img_h > 1 else 0.0)
    xs = torch.arange(rw, dtype=F64) * ((w - 1) / (rw - 1) if rw > 1 else 0.0)
    y0, x0 = ys.floor().long().clamp(max=h - 1), xs.floor().long().clamp(max=w - 1)
    y1, x1 = (y0 + 1).clamp(max=h - 1), (x0 + 1).clamp(max=w - 1)
    ly, lx = (ys - y0).view(-1, 1, 1), (xs - x0).view(1, -1, 1)
    top = a[y0][:, x0] * (1 - lx) + a[y0][:, x1] * lx
    bot = a[y1][:, x0] * (1 - lx) + a[y1][:, x1] * lx
    v = top * (1 - ly) + bot * ly
    out = torch.zeros(img_h, img_w, 3, dtype=F64)
    out[:, :rw] = (v / 255.0 - 0.5) / 0.5
    if not with_pos:
        return out
    pos = torch.zeros(img_h, img_w, 1, dtype=F64)
    pos[:, :rw] = (ys.view(-1, 1, 1) + xs.view(1, -1, 1))
    return out, pos, rw


def resize_norm_win(img: np.ndarray, img_h: int, img_w: int):
    """Two roundings on each source position (the scale, the product) move it by at most 2 u (fy + fx) pixels, worth at most 255 grey
    levels per pixel; eight more roundings in the weights and the blend; the normalisation doubles v / 255 and rounds twice.  The
    padding columns are exact."""
    y, pos, rw = resize_norm64(img, img_h, img_w, with_pos=True)
    e = 2.0 * U * (2.0 * pos + 8.0) + 4.0 * U
    e[:, rw:] = 0.0
    return y, e.expand_as(y)


# ---------------------------------------------------------------------------------------------------- per-op fp64 values and windows
def _act_win(pre, e, act):
    if act in (None, "none"):
        return pre, e
    if act == "relu":
        return F.relu(pre), e
    if act == "hard_swish":
        y = hswish(pre)
        return y, 1.5 * e + U * pre.abs() + 2 * U * y.abs()
    if act == "hard_sigmoid":
        return hsigmoid(pre), e / 6 + 2 * U
    if act == "swish":
        y = swish(pre)
        return y, 1.1 * e + 5 * U * y.abs()
    raise ValueError(act)


def conv_win(x, w, bias, stride=(1, 1), act=None, cin=None):
    """x [B, H, W, >= Cin], w [Cout, k, k, Cin] -> (fp64 NHWC output, window)."""
    Cout, k, _, Cin = w.shape
    xx = x.double()[..., :Cin].permute(0, 3, 1, 2)
    ww = w.double().permute(0, 3, 1, 2)
    b = None if bias is None else bias.double()
    pre = F.conv2d(xx, ww, b, stride=tuple(stride), padding=k // 2)
    mag = F.conv2d(xx.abs(), ww.abs(), None if b is None else b.abs(), stride=tuple(stride), padding=k // 2)
    y, e = _act_win(pre, (k * k * Cin + 2) * U * mag, act)
    return y.permute(0, 2, 3, 1).contiguous(), e.permute(0, 2, 3, 1).contiguous()


def dw_win(x, w, bias, stride=(1, 1), act=None):
    k, _, C = w.shape
    xx = x.double().permute(0, 3, 1, 2)
    ww = w.double().permute(2, 0, 1).unsqueeze(1)
    b = None if bias is None else bias.double()
    pre = F.conv2d(xx, ww, b, stride=tuple(stride), padding=k // 2, groups=C)
    mag = F.conv2d(xx.abs(), ww.abs(), None if b is None else b.abs(), stride=tuple(stride), padding=k // 2, groups=C)
    y, e = _act_win(pre, (k * k + 2) * U * mag, act)
    return y.permute(0, 2, 3, 1).contiguous(), e.permute(0, 2, 3, 1).contiguous()


def pool_mean_win(x):
    x = x.double()
    HW = x.shape[1] * x.shape[2]
    return x.mean((1, 2)), (HW + 1) * U * x.abs().mean((1, 2))


def pool_2x2_win(x):
    xx = x.double().permute(0, 3, 1, 2)
    return F.avg_pool2d(xx, 2, 2).permute(0, 2, 3, 1).contiguous(), (3 * U * F.avg_pool2d(xx.abs(), 2, 2)).permute(0, 2, 3, 1).contiguous()


def scale_win(x, s):
    y = x.double() * s.double()[:, None, None, :]
    return y, U * y.abs()


def layernorm_win(x, g, b, eps):
    x, g, b = x.double(), g.double(), b.double()
    D = x.shape[-1]
    mean = x.mean(-1, keepdim=True)
    em = (D + 1) * U * x.abs().mean(-1, keepdim=True)
    d = x - mean
    ed = em + U * d.abs()
    var = (d * d).mean(-1, keepdim=True)
    evar = (2 * (d.abs() * ed).sum(-1, keepdim=True) + (D + 2) * U * (d * d).sum(-1, keepdim=True)) / D
    r = 1.0 / torch.sqrt(var + eps)
    rel_r = 0.5 * (evar + U * (var + eps)) / (var + eps) + 2 * U
    y = d * r * g + b
    return y, g.abs() * r * (ed + d.abs() * (rel_r + 2 * U)) + U * ((d * r * g).abs() + y.abs())


def add_win(a, b):
    y = a.double() + b.double()
    return y, U * y.abs()


def attention_win(qkv, heads, scale32=True):
    """scale32: d^-0.5 as the fp32 number the kernel is handed (the fp64 engine keeps the fp64 one)"""
    B, N, three = qkv.shape
    d = three // (3 * heads)
    t = qkv.double().reshape(B, N, 3, heads, d).permute(2, 0, 3, 1, 4)
    scale = float(np.float32(float(d) ** -0.5)) if scale32 else float(d) ** -0.5
    q, k, v = t[0] * scale, t[1], t[2]
    s = q @ k.transpose(-1, -2)
    es = (d + 2) * U * (q.abs() @ k.abs().transpose(-1, -2))
    m, mi = s.max(-1, keepdim=True)
    ex = es + torch.gather(es, -1, mi) + U * (s - m).abs()            # of s - max
    e = torch.exp(s - m)
    rel_e = ex + 2 * U
    rel_p = rel_e + rel_e.max(-1, keepdim=True)[0] + 11 * U + U      # the sum: at most 4 + 6 additions deep; one division
    p = e / e.sum(-1, keepdim=True)
    y = p @ v
    ey = (p * (rel_p + (N / 2 + 3) * U)) @ v.abs()
    f = lambda z: z.permute(0, 2, 1, 3).reshape(B, N, heads * d)
    return f(y), f(ey)


def ctc_rows_win(x):
    """(max, first argmax, lse, lse window): max and argmax are exact."""
    x = x.double()
    C = x.shape[-1]
    m, arg = x.max(-1), None
    mx = m[0]
    arg = (x == mx.unsqueeze(-1)).to(torch.int64).argmax(-1)          # the first index of the maximum
    dx = x - mx.unsqueeze(-1)
    e = torch.exp(dx)
    ssum = e.sum(-1)
    rel = ((U * dx.abs() + U) * e).sum(-1) / ssum + (math.ceil(C / 256) + 8) * U
    lse = mx + torch.log(ssum)
    return mx, arg, lse, rel + U * torch.log(ssum).abs() + 2 * U + U * lse.abs()


def greedy(arg_row):
    """TextRecognizer.decode on one row of arg-max ids (numpy)."""
    t = np.asarray(arg_row)
    sel = np.ones(len(t), dtype=bool)
    sel[1:] = t[1:] != t[:-1]
    sel &= t != 0
    return t[sel], np.where(sel)[0]


def ctc_loss_win(logits, lse, target):
    """-log p(target | logits) by the forward recursion in fp64 over logits [T, C] and the row log-sum-exps the device used, and its
    window: the log-sum-exp of three is 1-Lipschitz in its inputs, so a step passes the incoming error on unchanged and adds its own
    roundings -- at most 4 u in log(sum exp), and u on each of |alpha|, |log(sum)|, |logit - lse| and the result."""
    lg, ls = logits.double(), lse.double()
    T = lg.shape[0]
    L = len(target)
    ext = [0] * (2 * L + 1)
    ext[1::2] = list(target)
    S = len(ext)
    NEG = float("-inf")
    lp = lg[:, ext] - ls.view(-1, 1)                                  # [T, S]
    alpha = torch.full((S,), NEG, dtype=F64)
    alpha[0] = lp[0, 0]
    if S > 1:
        alpha[1] = lp[0, 1]
    skip = torch.tensor([s >= 3 and s % 2 == 1 and ext[s] != ext[s - 2] for s in range(S)])
    err = U * float(alpha[torch.isfinite(alpha)].abs().max())
    for t in range(1, T):
        a1 = torch.cat([torch.tensor([NEG], dtype=F64), alpha[:-1]])
        a2 = torch.cat([torch.tensor([NEG, NEG], dtype=F64), alpha[:-2]])[:S]
        a2 = torch.where(skip, a2, torch.full_like(a2, NEG))
        l = torch.logsumexp(torch.stack([alpha, a1, a2]), dim=0)
        alpha = l + lp[t]
        fin = torch.isfinite(alpha)
        if fin.any():
            err += float((6 * U + U * (2 * l[fin].abs() + lp[t][fin].abs() + 2 * alpha[fin].abs())).max())
    tail = alpha[-2:] if S > 1 else alpha[-1:]
    tot = torch.logsumexp(tail, dim=0)
    if not torch.isfinite(tot):
        return float("inf"), 0.0
    return float(-tot), err + 6 * U + 2 * U * float(tot.abs())


# ------------------------------------------------------------------------------------------------------------------ the fp64 engine
class EmuOps:
    """textflux_amd.ops' read-back functions in fp64 on the host: textflux_amd.ocr runs over it unchanged."""

    def __init__(self):
        self.calls = []

    def _note(self, name):
        self.calls.append(name)

    def ocr_resize_norm(self, packed, table, img_h, img_w):
        self._note("ocr_resize_norm")
        buf = packed.numpy()
        out = []
        for off, h, w, turn in table.tolist():
            img = buf[off:off + h * w * 3].reshape(h, w, 3)
            assert bool(turn) == (h > w * 1.2)
            out.append(resize_norm64(img, img_h, img_w))
        return torch.stack(out)

    def ocr_conv_f32(self, x, w, bias, stride=(1, 1), act=None, cin=None, out=None, co_off=0):
        self._note("ocr_conv_f32")
        assert (cin or x.shape[3]) == w.shape[3]
        y = conv_win(x, w, bias, stride, act)[0]
        if out is None:
            return y
        out[..., co_off:co_off + y.shape[3]] = y
        return out

    def ocr_linear(self, x, w, bias, act=None):
        M, K = x.shape
        return self.ocr_conv_f32(x.view(M, 1, 1, K), w.view(w.shape[0], 1, 1, K), bias, act=act).view(M, w.shape[0])

    def ocr_conv_dw(self, x, w, bias, stride=(1, 1), act=None):
        self._note("ocr_conv_dw")
        return dw_win(x, w, bias, stride, act)[0]

    def ocr_pool_mean(self, x):
        self._note("ocr_pool_mean")
        return pool_mean_win(x)[0]

    def ocr_pool_2x2(self, x, out=None):
        self._note("ocr_pool_2x2")
        y = pool_2x2_win(x)[0]
        if out is None:
            return y
        out[..., :y.shape[3]] = y
        return out

    def ocr_scale_channels(self, x, s):
        self._note("ocr_scale_channels")
        return scale_win(x, s)[0]

    def ocr_layernorm(self, x, g, b, eps):
        self._note("ocr_layernorm")
        return layernorm_win(x, g, b, eps)[0]

    def ocr_add_(self, x, y):
        self._note("ocr_add_")
        x += y
        return x

    def ocr_attention(self, qkv, heads):
        self._note("ocr_attention")
        return attention_win(qkv, heads, scale32=False)[0]

    def ctc_rows(self, logits):
        self._note("ctc_rows")
        mx, arg, lse, _ = ctc_rows_win(logits)
        return mx, arg.to(torch.int32), lse

    def ctc_score(self, logits, row_arg, row_lse, targets=None):
        self._note("ctc_score")
        n, T, _ = logits.shape
        ids = torch.zeros(n, T, dtype=torch.int32)
        tix = torch.full((n, T), -1, dtype=torch.int32)
        count = torch.zeros(n, dtype=torch.int32)
        for i in range(n):
            a, b = greedy(row_arg[i].numpy())
            ids[i, :len(a)], tix[i, :len(a)], count[i] = torch.from_numpy(a.astype(np.int32)), torch.from_numpy(b.astype(np.int32)), len(a)
        loss = None
        if targets is not None:
            loss = torch.tensor([ctc_loss_win(logits[i], row_lse[i], list(targets[i]))[0] for i in range(n)], dtype=F64)
        return ids, tix, count, loss
