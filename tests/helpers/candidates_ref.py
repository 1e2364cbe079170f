"""Restatements for the candidates feature (DESIGN.md section 4 "Candidates"), written from include/textflux_hip.h:
tfx_warp_affine_gather_u8 in numpy on tests/helpers/rectify_ref.py's resampler, tfx_x0_predict in torch's own bf16 arithmetic on the
CPU, and the choice rule in plain Python."""
import math

import numpy as np
import torch

from tests.helpers import rectify_ref as rref

BF = torch.bfloat16
MAX_SIDE = 1 << 24


def gather(images, table, out):
    """images u8 [B, H, W, C]; table int64 [n, 10] = (b, m0..m5, out_h, out_w, byte offset); out u8 [out_bytes], the packed buffer as it
    is before the call -> (the buffer after the call, the number of rows refused).  A row that cannot be served writes nothing."""
    images, out = np.asarray(images), np.array(out, dtype=np.uint8, copy=True)
    B, H, W, C = images.shape
    refused = 0
    for row in np.asarray(table, np.int64).reshape(-1, 10).tolist():
        b, m, h, w, off = row[0], row[1:7], row[7], row[8], row[9]
        if not (0 <= b < B and 1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE and 0 <= off <= out.size and h * w * C <= out.size - off):
            refused += 1
            continue
        out[off:off + h * w * C] = rref.warp_affine(images[b], np.array(m, np.int64), (h, w))[0].reshape(-1)
    return out, refused


def pack_table(crops, C, guard=0):
    """[(b, m6, h, w)] -> (table int64 [n, 10], out_bytes): the crops packed one behind the other with `guard` bytes before, between
    and after them."""
    rows, off = [], guard
    for b, m, h, w in crops:
        rows.append([b] + [int(v) for v in m] + [h, w, off])
        off += h * w * C + guard
    return np.array(rows, dtype=np.int64).reshape(-1, 10), off


def x0_predict(x, v, sigma, step):
    """torch's `latents - sigma * noise_pred` on bf16 CPU tensors with the Python float float(sigma[step]): the product is rounded to
    bf16, then the difference (the Python float takes part as fp32: sigma is an fp32 table)."""
    s = float(torch.as_tensor(sigma, dtype=torch.float32)[step])
    x, v = x.detach().cpu().to(BF), v.detach().cpu().to(BF)
    return x - s * v


def same_bits(a, b):
    """bf16 tensors equal bit for bit, a NaN matching any NaN (the payload of a NaN is not pinned)."""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.shape != b.shape or a.dtype != BF or b.dtype != BF:
        return False
    na, nb = torch.isnan(a), torch.isnan(b)
    ia, ib = a.view(torch.int16), b.view(torch.int16)
    return bool(torch.equal(na, nb) and torch.equal(ia[~na], ib[~nb]))


def choice_key(records, k):
    """(lines not read exactly, sum of ctc_loss with a non-finite or missing loss as +inf, k)"""
    loss = 0.0
    for r in records:
        v = r.get("ctc_loss")
        loss += math.inf if v is None or not math.isfinite(v) else v
    return (sum(1 for r in records if r["seq_acc"] != 1.0), loss, k)


def choose(scored, keep=1):
    return sorted(range(len(scored)), key=lambda k: choice_key(scored[k], k))[:keep]
