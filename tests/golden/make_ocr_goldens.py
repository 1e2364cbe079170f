#!/usr/bin/env python3
"""Generate tests/golden/g19_ocr.safetensors by IMPORTING the reference's recogniser (build container only):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_ocr_goldens.py

eval/ocr_recog needs only torch; eval/recognizer.py imports once cv2, easydict and skimage are stubbed (prediction, decode and
get_ctcloss never touch them).  Weights are not stored: tests/helpers/ocr_ref.seeded_state builds them here and in the tests.  Data only:
  * node.<name> / node_max.<name>: the reference's fp64 output of every top-level module for 'en' on ocr_ref.node_input() ([2, 3, 48, 64]),
    as at most 2048 evenly strided elements of the flattened tensor (a whole tensor per node would be 10 MB) and its largest magnitude;
  * crops.*: for the five ocr_ref.fixture_crops() at 3,48,320 -- a strided sample of the reference's own normalised batch (the whole of it
    is compared with ocr_ref.resize_norm64 here), ctc / ctc_neck of the fp64 model on
    the fp64 resize of the crops, ctc of the reference end to end in fp32, the greedy decodes (ids, time indices, counts) and get_ctcloss for ocr_ref.TARGETS with weight 1;
  * crops.ref_fp32_distance: max |ctc fp32 - ctc fp64| of the reference itself on those inputs, and crops.max_logit.
"""
import os
import sys
import types

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REFERENCE = "/root/reference/eval"
sys.path.insert(0, REPO)
sys.path.insert(0, REFERENCE)
sys.dont_write_bytecode = True


class AttrDict(dict):
    """what the reference uses of EasyDict: attribute access on nested dicts, pop"""
    def __init__(self, **kw):
        super().__init__(**kw)

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)

    def __setattr__(self, k, v):
        self[k] = v


for name in ("cv2", "easydict", "skimage", "skimage.transform", "skimage.transform._geometric"):
    sys.modules[name] = types.ModuleType(name)
sys.modules["easydict"].EasyDict = AttrDict
sys.modules["skimage.transform._geometric"]._umeyama = None

import numpy as np
import torch
from safetensors.torch import save_file

import recognizer as R  # the reference

from tests.helpers import ocr_ref as X

OUT = os.path.dirname(os.path.abspath(__file__))
torch.set_grad_enabled(False)
torch.manual_seed(0)
KEEP = 2048


def strided(t):
    flat = t.reshape(-1)
    step = max(1, flat.numel() // KEEP)
    return flat[::step][:KEEP].clone()


def main():
    model = R.create_predictor(None, "en")
    want = {k: tuple(v.shape) for k, v in model.state_dict().items() if not k.endswith("num_batches_tracked")}
    sd = X.seeded_state(97)
    assert {k: tuple(v.shape) for k, v in sd.items()} == want, "textflux_amd.ocr.state_spec differs from RecModel(...).state_dict()"
    assert list(want)[0] == "backbone.conv1._conv.weight" and list(want)[-1] == "head.fc.bias"
    model.load_state_dict(sd, strict=False)
    model.eval()
    m64 = R.create_predictor(None, "en")
    m64.load_state_dict(sd, strict=False)
    m64 = m64.double().eval()

    out = {}
    # ---- every top-level node, fp64
    got = {}
    enc = m64.neck.encoder
    mods = {"stem": m64.backbone.conv1, "pool": m64.backbone.pool, "neck.conv1": enc.conv1, "neck.conv2": enc.conv2, "neck.norm": enc.norm,
            "neck.conv3": enc.conv3, "neck.conv4": enc.conv4, "neck.conv1x1": enc.conv1x1}
    mods.update({f"block{i}": m for i, m in enumerate(m64.backbone.block_list)})
    mods.update({f"svtr{i}": m for i, m in enumerate(enc.svtr_block)})
    hooks = [m.register_forward_hook(lambda _m, _i, o, n=n: got.__setitem__(n, o.detach().clone())) for n, m in mods.items()]
    res = m64(X.node_input().double())
    for h in hooks:
        h.remove()
    got["ctc"], got["ctc_neck"] = res["ctc"], res["ctc_neck"]
    assert sorted(got) == sorted(X.NODES + ["ctc_neck"])
    for n, t in got.items():
        out["node." + n] = strided(t)
        out["node_max." + n] = t.abs().max().reshape(1)
    # the restatement must agree before anything is written
    mine = X.forward64(sd, X.node_input())
    for n, t in got.items():
        assert mine[n].shape == t.shape and float((mine[n] - t).abs().max()) <= 2.0 ** -40 * float(t.abs().max()), n

    # ---- the five crops at 3,48,320
    args = AttrDict(rec_image_shape="3, 48, 320", rec_batch_num=6, rec_char_dict_path=os.path.join(REFERENCE, "ocr_recog", "en_dict.txt"), use_fp16=False)
    rec = R.TextRecognizer(args, model)
    crops = X.fixture_crops()
    as_chw = lambda: [torch.from_numpy(c).permute(2, 0, 1).float() for c in crops]
    batches = []

    class Tap(torch.nn.Module):
        def __init__(self, inner, cast):
            super().__init__()
            self.inner, self.cast = inner, cast

        def forward(self, x):
            batches.append(x.clone())
            return self.inner(x.to(self.cast))

    rec.predictor = Tap(model, torch.float32)
    ctc32, _ = rec.pred_imglist(as_chw())                           # the reference end to end in fp32: its resize, its model
    assert len(batches) == 1
    order = np.argsort(np.array([c.shape[1] / float(c.shape[0]) for c in crops]))
    norm = torch.empty_like(batches[0])
    norm[torch.from_numpy(order)] = batches[0]                      # back into the order of fixture_crops()
    norm = norm.permute(0, 2, 3, 1).contiguous()                    # NHWC fp32, what resize_norm_img made
    for i, c in enumerate(crops):                                   # the restatement of the resize agrees with it inside its own window
        y, e = X.resize_norm_win(c, 48, 320)
        assert bool(((norm[i].double() - y).abs() <= e).all()), f"crop {i}: resize_norm64 leaves the reference's fp32 result"
    out["crops.norm"] = strided(norm)
    # the reference in fp64 on the same u8 crops.  resize_norm_img writes into an fp32 buffer whatever it is given, so the fp64 run takes
    # the fp64 resize just compared with it; the distance below then holds what an fp32 resize costs, which every fp32 run pays
    res = m64(torch.stack([X.resize_norm64(c, 48, 320) for c in crops]).permute(0, 3, 1, 2))
    ctc64, neck64 = res["ctc"], res["ctc_neck"]
    out["crops.ctc"], out["crops.ctc_neck"], out["crops.ctc_fp32"] = ctc64, neck64, ctc32
    out["crops.ref_fp32_distance"] = (ctc32.double() - ctc64).abs().max().reshape(1)
    out["crops.max_logit"] = ctc64.abs().max().reshape(1)
    T = ctc64.shape[1]
    ids = torch.zeros(len(crops), T, dtype=torch.int32)
    tix = torch.full((len(crops), T), -1, dtype=torch.int32)
    count = torch.zeros(len(crops), dtype=torch.int32)
    texts = []
    for i in range(len(crops)):
        a, b = rec.decode(ctc64[i].softmax(dim=-1))
        a32, _ = rec.decode(ctc32[i].softmax(dim=-1))
        assert list(a) == list(a32), "the reference's fp32 and fp64 decodes differ: the fixture would pin a coin toss"
        assert len(a) >= 5, f"crop {i}: the greedy decode has {len(a)} symbols"
        ids[i, :len(a)], tix[i, :len(a)], count[i] = torch.from_numpy(a.astype(np.int32)), torch.from_numpy(b.astype(np.int32)), len(a)
        texts.append(rec.get_text(a))
    assert len(set(texts)) == len(texts), f"decodes repeat: {texts}"
    out["crops.ids"], out["crops.time_index"], out["crops.count"] = ids, tix, count
    loss = rec.get_ctcloss(ctc64, X.TARGETS, np.ones(len(crops)))
    assert torch.isinf(loss[3]) and torch.isfinite(loss[[0, 1, 2, 4]]).all()
    out["crops.ctcloss"] = loss.double()
    out["crops.ctcloss_fp32"] = rec.get_ctcloss(ctc32, X.TARGETS, np.ones(len(crops))).double()
    out = {k: v.contiguous() for k, v in out.items()}
    path = os.path.join(OUT, "g19_ocr.safetensors")
    save_file(out, path)
    print(path, os.path.getsize(path), "bytes; decodes", texts, "ref fp32 distance", float(out["crops.ref_fp32_distance"]),
          "max |logit|", float(out["crops.max_logit"]), "losses", loss.tolist())


if __name__ == "__main__":
    main()
