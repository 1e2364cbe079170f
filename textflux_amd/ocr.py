"""Read-back (DESIGN.md section 4 "Read-back"): a text recogniser on the library's fp32 kernels that reads what an edit wrote and
scores it against the text that was asked for.

It restates the reference's evaluation recogniser (eval/recognizer.py + eval/ocr_recog: PP-OCRv3 -- a MobileNetV1Enhance backbone at
scale 0.5 with last_conv_stride (1, 2) and an average last pool, a two-block SVTR neck with dims 64 / hidden 120 / use_guide, a CTC
head that also returns the neck's features) and the metrics of eval/eval_dgocr.py.  The state-dict keys are the reference's own, so
its checkpoint loads unchanged; BatchNorm is folded into the convolutions on the host.  Every launch is issued from here through
`ops` (ocr_* / ctc_*): there is no C-side forward, as for the VAE and the text encoders.

No recogniser checkpoint ships with this repository: what is tested is mechanism and arithmetic on seeded weights, and no accuracy
claim is made.
"""
from __future__ import annotations

import math
import os
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

N_CLASS = {"ch": 6625, "en": 97}
BN_EPS = 1e-5
HIDDEN, HEADS, DIMS, DEPTH = 120, 8, 64, 2
# (dw channels, pw out channels, dw size, stride, squeeze-excite) of the backbone's 13 depthwise-separable blocks at scale 0.5
BLOCKS = [(16, 32, 3, (1, 1), False), (32, 64, 3, (1, 1), False), (64, 64, 3, (1, 1), False), (64, 128, 3, (2, 1), False),
          (128, 128, 3, (1, 1), False), (128, 256, 3, (2, 1), False)] + [(256, 256, 5, (1, 1), False)] * 5 + \
         [(256, 512, 5, (2, 1), True), (512, 512, 5, (1, 2), True)]
C_BACKBONE = 512


def state_spec(n_class: int) -> List[Tuple[str, Tuple[int, ...]]]:
    """[(key, shape)] of RecModel(...).state_dict() in the fixed configuration, without the num_batches_tracked counters."""
    spec: List[Tuple[str, Tuple[int, ...]]] = []

    def conv_bn(prefix: str, conv: str, bn: str, cout: int, cin: int, k: int):
        spec.append((f"{prefix}.{conv}.weight", (cout, cin, k, k)))
        spec.extend((f"{prefix}.{bn}.{n}", (cout,)) for n in ("weight", "bias", "running_mean", "running_var"))

    conv_bn("backbone.conv1", "_conv", "_batch_norm", 16, 3, 3)
    for i, (c, co, k, _, se) in enumerate(BLOCKS):
        p = f"backbone.block_list.{i}"
        conv_bn(p + "._depthwise_conv", "_conv", "_batch_norm", c, 1, k)
        if se:
            spec += [(p + "._se.conv1.weight", (c // 4, c, 1, 1)), (p + "._se.conv1.bias", (c // 4,)),
                     (p + "._se.conv2.weight", (c, c // 4, 1, 1)), (p + "._se.conv2.bias", (c,))]
        conv_bn(p + "._pointwise_conv", "_conv", "_batch_norm", co, c, 1)
    e, C = "neck.encoder", C_BACKBONE
    conv_bn(e + ".conv1", "conv", "norm", C // 8, C, 3)
    conv_bn(e + ".conv2", "conv", "norm", HIDDEN, C // 8, 1)
    for i in range(DEPTH):
        b = f"{e}.svtr_block.{i}"
        spec += [(b + ".norm1.weight", (HIDDEN,)), (b + ".norm1.bias", (HIDDEN,)),
                 (b + ".mixer.qkv.weight", (3 * HIDDEN, HIDDEN)), (b + ".mixer.qkv.bias", (3 * HIDDEN,)),
                 (b + ".mixer.proj.weight", (HIDDEN, HIDDEN)), (b + ".mixer.proj.bias", (HIDDEN,)),
                 (b + ".norm2.weight", (HIDDEN,)), (b + ".norm2.bias", (HIDDEN,)),
                 (b + ".mlp.fc1.weight", (2 * HIDDEN, HIDDEN)), (b + ".mlp.fc1.bias", (2 * HIDDEN,)),
                 (b + ".mlp.fc2.weight", (HIDDEN, 2 * HIDDEN)), (b + ".mlp.fc2.bias", (HIDDEN,))]
    spec += [(e + ".norm.weight", (HIDDEN,)), (e + ".norm.bias", (HIDDEN,))]
    conv_bn(e + ".conv3", "conv", "norm", C, HIDDEN, 1)
    conv_bn(e + ".conv4", "conv", "norm", C // 8, 2 * C, 3)
    conv_bn(e + ".conv1x1", "conv", "norm", DIMS, C // 8, 1)
    spec += [("head.fc.weight", (n_class, DIMS)), ("head.fc.bias", (n_class,))]
    return spec


def seeded_state_dict(n_class: int, seed: int = 0) -> Dict[str, torch.Tensor]:
    """A state dict of the right shapes from a seeded generator (create_predictor(None, ...)): fan-in scaled weights, BatchNorm
    statistics near the identity.  It recognises nothing; it exists so that the mechanism runs without a checkpoint."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for key, shape in state_spec(n_class):
        if key.endswith("running_var"):
            t = 0.5 + torch.rand(shape, generator=g)
        elif key.endswith("running_mean") or (key.endswith(".bias") and len(shape) == 1):
            t = 0.1 * torch.randn(shape, generator=g)
        elif len(shape) == 1:
            t = 1.0 + 0.1 * torch.randn(shape, generator=g)
        else:
            t = torch.randn(shape, generator=g) * (2.0 / math.prod(shape[1:])) ** 0.5
        sd[key] = t.float()
    return sd


def fold_bn(w: torch.Tensor, gamma, beta, mean, var, eps: float = BN_EPS):
    """(w gamma / sqrt(var + eps), beta - mean gamma / sqrt(var + eps)) in fp64, rounded once to fp32."""
    s = gamma.double() / torch.sqrt(var.double() + eps)
    return (w.double() * s.view(-1, 1, 1, 1)).float(), (beta.double() - mean.double() * s).float()


class RecModel:
    """The recogniser's weights in the kernels' layouts (dense [Cout, k, k, Cin], depthwise [k, k, C]) and its forward."""

    def __init__(self, state_dict: Dict[str, torch.Tensor], n_class: int, device="cuda", ops=None):
        if ops is None:
            from . import ops
        self.ops, self.n_class, self.device = ops, n_class, torch.device(device)
        want = dict(state_spec(n_class))
        missing = [k for k in want if k not in state_dict]
        extra = [k for k in state_dict if k not in want and not k.endswith("num_batches_tracked")]
        if missing or extra:
            raise ValueError(f"recogniser state dict: missing {missing[:4]}{'...' if len(missing) > 4 else ''}, "
                             f"unexpected {extra[:4]}{'...' if len(extra) > 4 else ''}")
        for k, shape in want.items():
            if tuple(state_dict[k].shape) != shape:
                raise ValueError(f"recogniser state dict: {k} has shape {tuple(state_dict[k].shape)}, the model's is {shape}")
        sd = {k: state_dict[k].detach().cpu() for k in want}
        dev = lambda t: t.contiguous().to(self.device)

        def conv_bn(prefix, conv, bn):
            w, b = fold_bn(sd[f"{prefix}.{conv}.weight"], *(sd[f"{prefix}.{bn}.{n}"] for n in ("weight", "bias", "running_mean", "running_var")))
            return w, b

        def dense(prefix, conv="_conv", bn="_batch_norm"):
            w, b = conv_bn(prefix, conv, bn)
            return dev(w.permute(0, 2, 3, 1)), dev(b)

        def lin(prefix):                          # nn.Linear, a 1 x 1 nn.Conv2d with a bias, or a LayerNorm's (weight, bias)
            w = sd[prefix + ".weight"].float()
            return dev(w.reshape(w.shape[0], -1) if w.dim() > 1 else w), dev(sd[prefix + ".bias"].float())

        self.stem = dense("backbone.conv1")
        self.blocks = []
        for i, (c, co, k, stride, se) in enumerate(BLOCKS):
            p = f"backbone.block_list.{i}"
            w, b = conv_bn(p + "._depthwise_conv", "_conv", "_batch_norm")
            blk = dict(dw=(dev(w[:, 0].permute(1, 2, 0)), dev(b)), stride=stride, pw=dense(p + "._pointwise_conv"))
            if se:
                blk["se1"], blk["se2"] = lin(p + "._se.conv1"), lin(p + "._se.conv2")
            self.blocks.append(blk)
        e = "neck.encoder"
        self.conv1, self.conv2, self.conv3, self.conv4, self.conv1x1 = (dense(f"{e}.{n}", "conv", "norm") for n in ("conv1", "conv2", "conv3", "conv4", "conv1x1"))
        self.svtr = []
        for i in range(DEPTH):
            b = f"{e}.svtr_block.{i}"
            self.svtr.append({n: lin(f"{b}.{n}") for n in ("norm1", "mixer.qkv", "mixer.proj", "norm2", "mlp.fc1", "mlp.fc2")})
        self.norm = lin(e + ".norm")
        self.fc = lin("head.fc")

    def forward(self, x: torch.Tensor) -> Dict[str, torch.Tensor]:
        """x fp32 [B, H, W, 3] (NHWC, normalised) -> {'ctc': [B, T, n_class], 'ctc_neck': [B, T, 64]}."""
        o = self.ops
        y = o.ocr_conv_f32(x, *self.stem, stride=(2, 2), act="hard_swish")
        for blk in self.blocks:
            y = o.ocr_conv_dw(y, *blk["dw"], stride=blk["stride"], act="hard_swish")
            if "se1" in blk:                      # between the depthwise and the pointwise convolution; hard-sigmoid is relu6(x + 3) / 6
                s = o.ocr_pool_mean(y)
                s = o.ocr_linear(s, *blk["se1"], act="relu")
                s = o.ocr_linear(s, *blk["se2"], act="hard_sigmoid")
                y = o.ocr_scale_channels(y, s)
            y = o.ocr_conv_f32(y, *blk["pw"], act="hard_swish")
        B, H, W, C = y.shape
        H, W = H // 2, W // 2
        cat = torch.zeros(B, H, W, 2 * C, dtype=y.dtype, device=y.device)       # [pooled backbone | conv3's output]: the concat is free
        o.ocr_pool_2x2(y, out=cat)
        z = o.ocr_conv_f32(cat, *self.conv1, act="swish", cin=C)
        z = o.ocr_conv_f32(z, *self.conv2, act="swish")
        N = H * W
        t = z.view(B * N, HIDDEN)
        for blk in self.svtr:                     # prenorm=False in the reference's Block means x + mixer(norm1(x))
            n = o.ocr_layernorm(t, *blk["norm1"], 1e-5)
            qkv = o.ocr_linear(n, *blk["mixer.qkv"])
            a = o.ocr_attention(qkv.view(B, N, 3 * HIDDEN), HEADS)
            p = o.ocr_linear(a.view(B * N, HIDDEN), *blk["mixer.proj"])
            t = o.ocr_add_(p, t)
            n = o.ocr_layernorm(t, *blk["norm2"], 1e-5)
            h = o.ocr_linear(n, *blk["mlp.fc1"], act="swish")
            h = o.ocr_linear(h, *blk["mlp.fc2"])
            t = o.ocr_add_(h, t)
        t = o.ocr_layernorm(t, *self.norm, 1e-6)
        o.ocr_conv_f32(t.view(B, H, W, HIDDEN), *self.conv3, act="swish", out=cat, co_off=C)
        z = o.ocr_conv_f32(cat, *self.conv4, act="swish")
        z = o.ocr_conv_f32(z, *self.conv1x1, act="swish")
        feats = z.view(B * N, DIMS)
        logits = o.ocr_linear(feats, *self.fc)
        return {"ctc": logits.view(B, N, self.n_class), "ctc_neck": feats.view(B, N, DIMS)}

    __call__ = forward


def load_state_dict(path: str) -> Dict[str, torch.Tensor]:
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file
        return load_file(path)
    return torch.load(path, map_location="cpu", weights_only=True)


def create_predictor(model_dir: Optional[str] = None, model_lang: str = "ch", device="cuda", ops=None) -> RecModel:
    """The reference's create_predictor: 'ch' -> 6625 classes, 'en' -> 97; model_dir = a .pth / .safetensors state dict, or None for
    seeded weights."""
    if model_lang not in N_CLASS:
        raise ValueError(f"Unsupported OCR recog model_lang: {model_lang}")
    if model_dir is not None and not os.path.exists(model_dir):
        raise ValueError(f"not find model file path {model_dir}")
    n_class = N_CLASS[model_lang]
    sd = seeded_state_dict(n_class) if model_dir is None else load_state_dict(model_dir)
    return RecModel(sd, n_class, device=device, ops=ops)


def _as_u8_hwc(img) -> np.ndarray:
    if isinstance(img, torch.Tensor):
        img = img.detach().cpu().numpy()
    a = np.asarray(img)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"a line crop is a non-empty uint8 [h, w, 3] image, got {a.dtype} {a.shape}")
    return np.ascontiguousarray(a)


class TextRecognizer:
    """The reference's TextRecognizer on the device.  Line crops are uint8 [h, w, 3] images (tensors or arrays); the resize, the
    normalisation and the quarter turn of tall crops happen in tfx_ocr_resize_norm."""

    def __init__(self, predictor: RecModel, rec_char_dict_path: str, rec_image_shape=(3, 48, 320), rec_batch_num: int = 6):
        shape = [int(v) for v in rec_image_shape.split(",")] if isinstance(rec_image_shape, str) else [int(v) for v in rec_image_shape]
        if len(shape) != 3 or shape[0] != 3 or shape[1] != 48 or shape[2] < 32 or shape[2] % 32:
            raise ValueError(f"rec_image_shape must be (3, 48, W) with W a positive multiple of 32, got {tuple(shape)}")
        if rec_batch_num < 1:
            raise ValueError("rec_batch_num must be at least 1")
        self.rec_image_shape, self.rec_batch_num, self.predictor = shape, int(rec_batch_num), predictor
        self.chars = self.get_char_dict(rec_char_dict_path)
        if len(self.chars) != predictor.n_class:
            raise ValueError(f"the character list gives {len(self.chars)} classes ('sos' + {len(self.chars) - 2} lines + ' '), "
                             f"the model has {predictor.n_class}")
        self.char2id = {x: i for i, x in enumerate(self.chars)}

    @staticmethod
    def get_char_dict(character_dict_path: str) -> List[str]:
        with open(character_dict_path, "rb") as fin:
            lines = [line.decode("utf-8").strip("\n").strip("\r\n") for line in fin.readlines()]
        return ["sos"] + lines + [" "]           # eos is space

    def get_text(self, order) -> str:
        return "".join(self.chars[int(i)] for i in order)

    def text_ids(self, text: str) -> List[int]:
        """an unknown character maps to the last id"""
        return [self.char2id.get(c, len(self.chars) - 1) for c in text]

    def pred_imglist(self, img_list: Sequence[Any]):
        """(ctc [n, T, C], ctc_neck [n, T, 64]) in the order of img_list; batches of rec_batch_num, sorted by aspect ratio."""
        imgs = [_as_u8_hwc(i) for i in img_list]
        if not imgs:
            raise ValueError("pred_imglist: no images")
        o, dev = self.predictor.ops, self.predictor.device
        _, imgH, imgW = self.rec_image_shape
        imgW = int(imgH * (imgW / imgH))
        order = np.argsort(np.array([im.shape[1] / float(im.shape[0]) for im in imgs]))
        ctc, neck = [None] * len(imgs), [None] * len(imgs)
        for beg in range(0, len(imgs), self.rec_batch_num):
            idx = order[beg:beg + self.rec_batch_num]
            table, off = [], 0
            for i in idx:
                h, w = imgs[i].shape[:2]
                table.append((off, h, w, 1 if h > w * 1.2 else 0))
                off += h * w * 3
            packed = torch.from_numpy(np.concatenate([imgs[i].reshape(-1) for i in idx])).to(dev)
            x = o.ocr_resize_norm(packed, torch.tensor(table, dtype=torch.int32).to(dev), imgH, imgW)
            preds = self.predictor(x)
            for r, i in enumerate(idx):
                ctc[i], neck[i] = preds["ctc"][r], preds["ctc_neck"][r]
        return torch.stack(ctc, dim=0), torch.stack(neck, dim=0)

    def _score(self, preds: torch.Tensor, targets=None):
        o = self.predictor.ops
        preds = preds.contiguous()
        _, arg, lse = o.ctc_rows(preds)
        ids, tix, count, loss = o.ctc_score(preds, arg, lse, targets)
        count = count.cpu().numpy()
        ids, tix = ids.cpu().numpy(), tix.cpu().numpy()
        return [ids[i, :count[i]] for i in range(len(count))], [tix[i, :count[i]] for i in range(len(count))], loss

    def decode(self, mat: torch.Tensor):
        """mat [T, C] -> (ids, their time indices): arg-max per step, repeats collapsed, the blank 0 dropped."""
        ids, tix, _ = self._score(mat.unsqueeze(0))
        return ids[0], tix[0]

    def get_ctcloss(self, preds: torch.Tensor, gt_text: Sequence[str], weight) -> torch.Tensor:
        """-log p(text | preds) / T * weight per sample (torch.nn.CTCLoss(reduction='none') on log_softmax(preds), blank 0), on the host."""
        _, _, loss = self._score(preds, [self.text_ids(t) for t in gt_text])
        loss = loss.cpu() / preds.shape[1]
        w = weight if isinstance(weight, torch.Tensor) else torch.tensor(weight)
        return loss * w.cpu()

    def read(self, images: Sequence[Any], targets: Optional[Sequence[str]] = None) -> List[Dict[str, Any]]:
        """Per line: {'text', 'ids', 'ctc_loss'} (ctc_loss None without targets)."""
        if targets is not None and len(targets) != len(images):
            raise ValueError(f"read: {len(targets)} targets for {len(images)} images")
        preds, _ = self.pred_imglist(images)
        ids, _, loss = self._score(preds, None if targets is None else [self.text_ids(t) for t in targets])
        loss = None if loss is None else (loss.cpu() / preds.shape[1]).tolist()
        return [dict(text=self.get_text(ids[i]), ids=[int(v) for v in ids[i]], ctc_loss=None if loss is None else loss[i])
                for i in range(len(ids))]

    def read_device(self, images_u8: torch.Tensor, lines: Sequence[Tuple[int, Any]],
                    targets: Optional[Sequence[str]] = None) -> List[Dict[str, Any]]:
        """read() on lines that are cut on the device (DESIGN.md section 4 "Candidates"): images_u8 is a device uint8 [B, H, W, 3]
        tensor and `lines` a list of (b, polygon | mask), crop_line's shapes in image b's coordinates.  The minimum-area rectangles
        are computed on the host as crop_line does; then one table upload and ONE ops.warp_affine_gather_u8 launch cut every crop
        into one packed buffer, which ocr_resize_norm reads in batches of rec_batch_num in pred_imglist's aspect-ratio order.  No crop
        visits the host.  The records are read()'s, bit for bit those of read([crop_line(images_u8[b], shape) ...], targets)."""
        if not isinstance(images_u8, torch.Tensor) or images_u8.dtype != torch.uint8 or images_u8.dim() != 4 or images_u8.shape[3] != 3:
            raise ValueError("read_device: images_u8 is a device uint8 [B, H, W, 3] tensor")
        if targets is not None and len(targets) != len(lines):
            raise ValueError(f"read_device: {len(targets)} targets for {len(lines)} lines")
        if not lines:
            raise ValueError("read_device: no lines")
        o, dev = self.predictor.ops, self.predictor.device
        _, imgH, imgW = self.rec_image_shape
        imgW = int(imgH * (imgW / imgH))
        rows, off = [], 0
        for b, shape in lines:
            if not 0 <= int(b) < images_u8.shape[0]:
                raise ValueError(f"read_device: line of image {b}, the batch has {images_u8.shape[0]}")
            m6, h, w = line_matrix(shape)
            rows.append([int(b)] + [int(v) for v in m6] + [h, w, off])
            off += h * w * 3
        packed, refused = o.warp_affine_gather_u8(images_u8.contiguous(), np.array(rows, dtype=np.int64),
                                                  out=torch.empty(off, dtype=torch.uint8, device=dev))
        order = np.argsort(np.array([r[8] / float(r[7]) for r in rows]))
        table = torch.tensor([(rows[i][9], rows[i][7], rows[i][8], 1 if rows[i][7] > rows[i][8] * 1.2 else 0) for i in order],
                             dtype=torch.int32).to(dev)
        ctc = [None] * len(rows)
        for beg in range(0, len(rows), self.rec_batch_num):
            idx = order[beg:beg + self.rec_batch_num]
            preds = self.predictor(o.ocr_resize_norm(packed, table[beg:beg + len(idx)], imgH, imgW))
            for r, i in enumerate(idx):
                ctc[i] = preds["ctc"][r]
        preds = torch.stack(ctc, dim=0)
        ids, _, loss = self._score(preds, None if targets is None else [self.text_ids(t) for t in targets])
        if int(refused.item()):
            raise RuntimeError(f"read_device: the gather refused {int(refused.item())} of {len(rows)} crops")
        loss = None if loss is None else (loss.cpu() / preds.shape[1]).tolist()
        return [dict(text=self.get_text(ids[i]), ids=[int(v) for v in ids[i]], ctc_loss=None if loss is None else loss[i])
                for i in range(len(ids))]


# ---- line crops ------------------------------------------------------------------------------------------------------------------
def line_corners(points: np.ndarray) -> np.ndarray:
    """[tl, tr, br, bl] of the minimum-area rectangle around (x, y) points, ordered as the reference's min_bounding_rect orders them:
    the corners truncated to integers, the left two by x, each pair then by y."""
    from . import glyph
    box = glyph.box_points(glyph.min_area_rect(points)).astype(np.int64)
    xs = sorted((tuple(int(v) for v in p) for p in box), key=lambda p: p[0])
    (tl, bl), (tr, br) = sorted(xs[:2], key=lambda p: p[1]), sorted(xs[2:], key=lambda p: p[1])
    return np.array([tl, tr, br, bl], dtype=np.float64)


def crop_line(image_u8: torch.Tensor, polygon_or_mask, ops=None) -> torch.Tensor:
    """The upright crop (uint8 [h, w, 3], device) of the minimum-area rectangle around a line: polygon = [n, 2] (x, y) points, mask = a
    [H, W] or [H, W, 3] uint8 array whose pixels > 127 are the line.  The crop has the rectangle's own size and is sampled by
    ops.warp_affine_u8 (the reference's crop -- cv2 contours, a skimage similarity, grid_sample -- is not what is pinned)."""
    if ops is None:
        from . import ops
    m6, h, w = line_matrix(polygon_or_mask)
    if image_u8.dim() != 3 or image_u8.dtype != torch.uint8:
        raise ValueError("crop_line: image_u8 is a uint8 [H, W, 3] tensor")
    return ops.warp_affine_u8(image_u8.unsqueeze(0).contiguous(), m6, (h, w))[0]


def line_matrix(polygon_or_mask) -> Tuple[np.ndarray, int, int]:
    """(m int64 [6] Q16, h, w) of crop_line's warp: the minimum-area rectangle around the line, its own size, its upright frame."""
    a = np.asarray(polygon_or_mask)
    if a.ndim == 2 and a.shape[1] == 2 and a.shape[0] >= 3 and a.dtype != np.uint8:
        pts = a.astype(np.float64)
    else:
        m = a if a.ndim == 2 else a[..., 0]
        ys, xs = np.nonzero(m > 127)
        if len(xs) == 0:
            raise ValueError("crop_line: the mask is empty")
        pts = np.stack([xs, ys], axis=1).astype(np.float64)
    tl, tr, br, bl = line_corners(pts)
    width = max(np.linalg.norm(tl - tr), np.linalg.norm(br - bl))
    height = max(np.linalg.norm(tl - bl), np.linalg.norm(tr - br))
    w, h = max(1, int(width)), max(1, int(height))
    ux = (tr - tl) / max(np.linalg.norm(tr - tl), 1e-9) if np.linalg.norm(tr - tl) > 0 else np.array([1.0, 0.0])
    uy = (bl - tl) / max(np.linalg.norm(bl - tl), 1e-9) if np.linalg.norm(bl - tl) > 0 else np.array([0.0, 1.0])
    q = 1 << 16
    m6 = np.array([round(ux[0] * q), round(uy[0] * q), round(tl[0] * q), round(ux[1] * q), round(uy[1] * q), round(tl[1] * q)], dtype=np.int64)
    return m6, h, w


# ---- metrics (eval/eval_dgocr.py), host-side ---------------------------------------------------------------------------------------
def levenshtein(a: Sequence[Any], b: Sequence[Any]) -> int:
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i]
        for j, y in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (x != y)))
        prev = cur
    return prev[-1]


def get_ld(a: Sequence[Any], b: Sequence[Any]) -> float:
    """normalised edit distance score 1 - lev / (max(len) + 1e-5)"""
    return 1 - levenshtein(a, b) / (max(len(a), len(b)) + 1e-5)


def score_lines(rec: TextRecognizer, crops: Sequence[Any], texts: Sequence[str]) -> List[Dict[str, Any]]:
    """[{text, pred, seq_acc, ned, ctc_loss}] per line: the crop is read and compared with its text on id sequences."""
    out = []
    for text, r in zip(texts, rec.read(crops, texts)):
        gt = rec.text_ids(text)
        out.append(dict(text=text, pred=r["text"], seq_acc=1.0 if r["ids"] == gt else 0.0, ned=get_ld(r["ids"], gt), ctc_loss=r["ctc_loss"]))
    return out


def report(records: Sequence[Dict[str, Any]]) -> Dict[str, Any]:
    """ocr_report.json: the per-line records with the mean sentence accuracy, the mean NED and the line count."""
    n = len(records)
    return dict(lines=list(records), line_count=n, sen_acc=sum(r["seq_acc"] for r in records) / n if n else 0.0,
                ned=sum(r["ned"] for r in records) / n if n else 0.0)


# ---- the callers' side: run_items(ocr=...), the CLIs' --ocr_weights / --ocr_lang / --ocr_dict -----------------------------------------
OCR_KEYS = ("weights", "lang", "dict_path", "image_shape", "batch")


def ocr_cfg(ocr) -> Dict[str, Any]:
    """run_items' ocr argument with its defaults filled in: dict(weights=None, lang='ch', dict_path, image_shape=(3, 48, 320), batch=6).
    ValueError on anything else; nothing is loaded or launched here."""
    if not isinstance(ocr, dict):
        raise ValueError("ocr must be a dict(weights, lang, dict_path, image_shape, batch)")
    unknown = set(ocr) - set(OCR_KEYS)
    if unknown:
        raise ValueError(f"ocr: unknown keys {sorted(unknown)}")
    cfg = dict(weights=ocr.get("weights"), lang=ocr.get("lang") or "ch", dict_path=ocr.get("dict_path"),
               image_shape=tuple(ocr.get("image_shape") or (3, 48, 320)), batch=int(ocr.get("batch") or 6))
    if cfg["lang"] not in N_CLASS:
        raise ValueError(f"ocr: lang must be one of {sorted(N_CLASS)}, got {cfg['lang']!r}")
    if not cfg["dict_path"] or not os.path.exists(cfg["dict_path"]):
        raise ValueError(f"ocr: dict_path must name the character list of the model ({cfg['dict_path']!r} does not exist)")
    if cfg["weights"] is not None and not os.path.exists(cfg["weights"]):
        raise ValueError(f"ocr: weights {cfg['weights']!r} does not exist (None = seeded weights, which recognise nothing)")
    if len(cfg["image_shape"]) != 3 or cfg["batch"] < 1:
        raise ValueError("ocr: image_shape is (3, 48, W) and batch at least 1")
    return cfg


def make_reader(cfg: Dict[str, Any], device="cuda") -> TextRecognizer:
    """The TextRecognizer of an ocr_cfg dict: the first thing read-back constructs on the device."""
    return TextRecognizer(create_predictor(cfg["weights"], cfg["lang"], device=device), cfg["dict_path"], cfg["image_shape"], cfg["batch"])


def item_lines(item: Dict[str, Any], loader=None, eval_cfg: Optional[Dict[str, Any]] = None):
    """((W, H) of the item's scene, [(text, polygon [n, 2] float | line mask uint8 [H, W])]): every `annotations` entry of an eval item
    that has a text and a polygon, or every connected mask region of a plain item as per_line.split_lines pairs them with the text."""
    from PIL import Image
    load = loader or (lambda p: Image.open(p))
    if "img_name" in item:
        scene = load(os.path.join((eval_cfg or {}).get("original_images_dir", "."), item["img_name"]))
        return scene.size, [(a["text"], np.asarray(a["polygon"], dtype=np.float64)) for a in item.get("annotations") or []
                            if a.get("text") and a.get("polygon")]
    from . import glyph, per_line
    mask = load(item["mask"]).convert("L")
    return mask.size, [(text, lm) for _, text, lm in per_line.split_lines(mask, glyph.read_words_from_text(item["text"]))]


def read_lines(reader: TextRecognizer, image, size, lines, device="cuda") -> List[Dict[str, Any]]:
    """score_lines on the crops of `lines` (item_lines' pairs, in the coordinates of a scene of `size`) from the final image (PIL; the
    pasted scene, or the pipeline-size result -- shapes are scaled to it)."""
    from PIL import Image
    if not lines:
        return []
    img = image.convert("RGB")
    sx, sy = img.size[0] / float(size[0]), img.size[1] / float(size[1])
    dev_img = torch.from_numpy(np.ascontiguousarray(np.array(img))).to(device)
    crops = []
    for _, shape in lines:
        if shape.ndim == 2 and shape.shape[1] == 2 and shape.dtype != np.uint8:
            shape = shape * np.array([sx, sy])
        elif (sx, sy) != (1.0, 1.0):
            shape = np.array(Image.fromarray(shape).resize(img.size, Image.NEAREST))
        crops.append(crop_line(dev_img, shape))
    return score_lines(reader, crops, [t for t, _ in lines])
