"""Batched, multi-GPU batch driver: a list of work items -> one generated (and cropped) image per item.  Two item schemas:
the reference's `annos.json` entries {img_name, annotations: [{text, polygon}]} (scripts/run_eval.py:76-140: polygon -> mask,
strip height int(w * text_height_ratio), glyph strip stacked on top, `full_images/` + `cropped_images/` outputs) and the plain
{image, mask, text} triples of run_inference.py's rule.

Counterpart of the reference's scripts/run_eval.py:76-247.  The reference starts one worker process per GPU; every worker
holds a full replica (incl. the 9.5 GB T5 encoder), pulls ONE item at a time from a multiprocessing queue, encodes its own
prompts and calls the pipeline at batch 1.  Here (one process per GPU, launched by torchrun / `--gpus N`):

* the glyph image of every item is rendered on the host (font rasteriser); the canvas -- glyph and scene stacked, black mask
  over the glyph part, grey value of the RGB mask -- is composed ON THE DEVICE for a whole batch at once
  (`ops.compose_canvas`), including the callers' resize to a multiple of 32 (`ops.resample_u8`: Pillow's bicubic resampler
  in its own fixed-point arithmetic, bit-identical); items are grouped by pipeline geometry into batches of up to `batch_size` -- the engine's batch-8 rate is 13 % above its batch-1
  rate, and the captured step graph is reused across batches of one geometry;
* batches are dealt round-robin to the ranks.  The CLIP prompt is the one fixed template: its pooled embedding is encoded ONCE
  on rank 0 and broadcast (RCCL over xGMI).  The T5 prompts differ per image: when every rank holds a T5 encoder (9.5 GB of
  288 GB; the default) each rank encodes the prompts of ITS OWN batch -- 0.06 s per 8 prompts, no rank waits for another, the
  per-round critical path is the same on every rank.  Only when some rank has no T5 (`text_encoder_2 is None`) does rank 0
  encode for everybody and scatter, 4 MiB per prompt -- then rank 0 carries world x the encoding work on top of its own
  denoising and is the round's straggler by that much (3 % at world 8); an encoding failure on rank 0 marks that batch
  failed on its owner (a flag travels with the rows) instead of leaving the other ranks blocked in the collective;
* every rank denoises its batch with per-item generators seeded like the reference's single-image call (same noise per
  image as `run_inference.py --seed`), crops and writes its own results; a per-rank summary is gathered on rank 0.

The communication pattern (broadcast + scatter + gather, no per-step traffic) is exercised on CPU with the gloo backend
and a stub pipeline in tests/test_batch_driver_cpu.py.
"""
from __future__ import annotations

import os
from dataclasses import dataclass, field
from typing import Any, Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch
import torch.distributed as dist

from . import distributed as tdist
from . import glyph


@dataclass
class Work:
    index: int                       # position in the item list
    image: Any                       # composed PIL image at pipeline size (None when `parts` is set)
    mask: Any
    prompt: str                      # T5 prompt (generate_prompt(words))
    meta: Dict[str, Any]
    size: Tuple[int, int]            # (width, height) given to the pipeline
    parts: Any = None                # (glyph, scene, mask uint8 arrays, horizontal): composed on the device per batch
    name: Optional[str] = None       # eval schema: base file name written under full_images/ and cropped_images/
    orig_scene: Any = None           # paste-back only: the scene as loaded, uint8 [H, W, 3] ...
    orig_mask: Any = None            # ... its RGB mask, uint8 [H, W, 3] ...
    region: Any = None               # ... and the paste_back.Region of it that was edited (the whole image without `region`)
    parent: Optional[int] = None     # per-line editing only (per_line.py): the index of the item this line belongs to ...
    line: Optional[int] = None       # ... and the line's position in the item's split order
    rect: Any = None                 # rectified lines only (rectify.py): the oriented rectify.Rect that was edited upright; perspective lines
                                     # only (perspective.py): the perspective.Quad that was; curved lines only (curve.py): the curve.Ribbon.
                                     # `region` is then the scene window it is pasted into
    texts: Any = None                # the text lines the work writes: one for a strip edit, the item's words on the multi-line canvas
    seed: Optional[int] = None       # candidates only (candidates.py): the seed of this candidate's generator (None: the run's seed) ...
    cand: Optional[int] = None       # ... and its position k among the candidates of its work


@dataclass
class Batch:
    size: Tuple[int, int]            # (width, height) of the items; of the item with the most tokens when `mixed`
    items: List[Work] = field(default_factory=list)
    mixed: bool = False              # items of different sizes: one padded forward per step (FluxFillPipeline.call_mixed)


def eval_item_complete(item: Dict[str, Any]) -> bool:
    """The reference's filter (scripts/run_eval.py:229-231): first annotation with a non-empty text and polygon."""
    ann = item.get("annotations")
    return bool(ann) and bool(ann[0].get("text")) and bool(ann[0].get("polygon"))


class LinePath(NamedTuple):
    key: str                         # the paste_back cfg key
    module: str                      # the geometry module: plan(mask_grey, cfg) -> its shape or None, cfg(option)
    attr: str                        # the pipeline's warp
    keyword: str                     # the preparers' keyword that carries that warp
    verb: str                        # "only single-line edits are <verb>"


# The per-line paths that edit a line upright, in the order they are tried
LINE_PATHS = (LinePath("curve", "curve", "warp_grid", "warp_grid", "cut as ribbons"),
              LinePath("perspective", "perspective", "warp_perspective", "warp_quad", "cut as quads"),
              LinePath("rectify", "rectify", "warp_affine", "warp", "rectified"))


def _module(path: LinePath):
    import importlib
    return importlib.import_module("." + path.module, __package__)


def pipeline_warps(pipe, cfg: Dict[str, Any]) -> Dict[str, Optional[Callable]]:
    """{preparer keyword: the pipeline's warp for every line path the paste_back cfg asks for, None for the others}.  ValueError
    when the pipeline lacks one that is asked for."""
    warps = {}
    for path in reversed(LINE_PATHS):
        asked = bool(cfg.get(path.key))
        if asked and not hasattr(pipe, path.attr):
            raise ValueError(f"paste_back: {path.key} needs a pipeline with {path.attr} (FluxFillPipeline)")
        warps[path.keyword] = getattr(pipe, path.attr) if asked else None
    return warps


def _paste_back_option(paste_back: Dict[str, Any], key: str, make_cfg: Callable, needs_per_line: Optional[str] = None):
    """One option key of paste_back: None (absent) for None / False, make_cfg's dict for True or a dict, ValueError otherwise.
    needs_per_line: the reason the key is refused with, given when it needs per_line and per_line is off."""
    value = paste_back.get(key)
    if value is None or value is False:
        return None
    if value is not True and not isinstance(value, dict):
        raise ValueError(f"paste_back: {key} must be None, True or a dict")
    if needs_per_line:
        raise ValueError(f"paste_back: {key} needs per_line=True ({needs_per_line})")
    try:
        return make_cfg(value)
    except ValueError as e:
        raise ValueError(f"paste_back: {e}") from None


def _paste_back_cfg(paste_back: Dict[str, Any]) -> Dict[str, Any]:
    """run_items' paste_back argument with its defaults filled in: dict(dilate, feather, region: None | dict(pad, min_side, max_side)),
    and, only when the caller gave them, per_line: True (which implies a region: {} when absent) and color_match: paste_back.
    color_match_cfg's dict(ring, gain, max_shift, min_pixels), rectify: rectify.rectify_cfg's dict(min_angle, max_angle, min_aspect)
    perspective: perspective.perspective_cfg's dict(max_fit, max_taper, min_aspect, max_angle) and curve: curve.curve_cfg's
    dict(min_bend, max_squeeze, max_turn, min_aspect, min_fill, max_angle) (all three need per_line), seamless: paste_back.
    seamless_cfg's dict(smooth, max_shift) and grain: paste_back.grain_cfg's dict(ring, max_sigma, strength, min_pixels, seed) with, only
    when the caller gave it, spectrum: dict(max_blur, luma), and keyed: paste_back.keyed_cfg's dict(lo, hi, dilate, feather, noise, ring,
    min_pixels)."""
    from . import paste_back as pb
    unknown = set(paste_back) - {"dilate", "feather", "region", "per_line", "color_match", "rectify", "perspective", "curve", "seamless",
                                  "grain", "keyed"}
    region = paste_back.get("region")
    if region is not None:
        unknown |= {f"region.{k}" for k in set(region) - {"pad", "min_side", "max_side"}}
    if unknown:
        raise ValueError(f"paste_back: unknown keys {sorted(unknown)}")
    dilate, feather = paste_back.get("dilate"), paste_back.get("feather")
    cfg = dict(dilate=pb.DILATE if dilate is None else int(dilate), feather=pb.FEATHER if feather is None else int(feather), region=None)
    if not (0 <= cfg["dilate"] <= 255 and 0 <= cfg["feather"] <= 255):
        raise ValueError("paste_back: dilate and feather must be in [0, 255]")
    if region is not None:
        cfg["region"] = {k: v for k, v in region.items() if v is not None}
    per_line = paste_back.get("per_line")
    if per_line not in (None, False, True):
        raise ValueError("paste_back: per_line must be True or False")
    if per_line:
        cfg["per_line"] = True
        if cfg["region"] is None:
            cfg["region"] = {}
    options = [("color_match", pb.color_match_cfg, None), ("seamless", pb.seamless_cfg, None), ("grain", pb.grain_cfg, None),
               ("keyed", pb.keyed_cfg, None)]
    options += [(path.key, lambda v, path=path: _module(path).cfg(v), None if per_line else f"only single-line edits are {path.verb}")
                for path in reversed(LINE_PATHS)]
    for key, make_cfg, needs_per_line in options:
        got = _paste_back_option(paste_back, key, make_cfg, needs_per_line)
        if got is not None:
            cfg[key] = got
    return cfg


def _paste_back_inputs(scene, mask, cfg: Dict[str, Any]):
    """Paste-back: (scene, mask) PIL images handed to the usual preparation, and what the paste needs afterwards (the originals as
    arrays, the edited Region).  Without `region` the preparation sees the images as they are; with it, the region's crop, resized
    with PIL's bicubic to the region's editing size (tw, th) when that differs."""
    import numpy as np
    from PIL import Image
    from . import paste_back as pb
    so, mo = np.array(scene), np.array(mask)
    if cfg["region"] is None:
        return scene, mask, so, mo, pb.select_region(None, size=scene.size)
    reg = pb.select_region(pb.grey_of(mo), cfg["dilate"], cfg["feather"], **cfg["region"])
    box = (reg.x0, reg.y0, reg.x1, reg.y1)
    s, m = scene.crop(box), mask.crop(box)
    if s.size != (reg.tw, reg.th):
        s, m = s.resize((reg.tw, reg.th), Image.BICUBIC), m.resize((reg.tw, reg.th), Image.BICUBIC)
    return s, m, so, mo, reg


def _host_u8(x):
    """A warp's result (device tensor or array, with or without the batch axis of one) as a host uint8 array [H, W, C]."""
    import numpy as np
    a = x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return np.ascontiguousarray(a[0] if a.ndim == 4 else a)


def _warped_inputs(so, mo, warp: Callable, fwd, size, edit_size):
    """The scene and the RGB mask warped into an upright frame `size` = (w, h) by `warp` (the device kernel) under its arguments `fwd`,
    the mask binarised at >= 128, both resized to edit_size with PIL's bicubic when that differs -> (scene, mask) as PIL images."""
    import numpy as np
    from PIL import Image
    w, h = size
    s = _host_u8(warp(so, *fwd, (h, w)))
    m = np.where(_host_u8(warp(mo if mo.ndim == 3 else mo[:, :, None], *fwd, (h, w))) >= 128, 255, 0).astype(np.uint8)
    s, m = Image.fromarray(s), Image.fromarray(m if mo.ndim == 3 else m[:, :, 0])
    if s.size != tuple(edit_size):
        s, m = s.resize(tuple(edit_size), Image.BICUBIC), m.resize(tuple(edit_size), Image.BICUBIC)
    return s, m


def _upright_inputs(scene, mask, cfg: Dict[str, Any], path: LinePath, warp: Callable):
    """_paste_back_inputs for a line that is edited upright through `path` (DESIGN.md section 4 "Rectified lines", "Perspective
    lines", "Curved lines"), or None when the line stays on the other paths (the path's module's plan).  -> (scene, mask, originals,
    Region, shape): the scene and the RGB mask warped into the upright crop (rw, rh) of the shape -- a Rect, a Quad or a Ribbon -- by
    `warp` (the pipeline's warp of that path: the device kernel; nothing is resampled in a rotated frame on the host) under the shape's
    forward map, the mask binarised at >= 128, both resized to the editing size (tw, th) with PIL's bicubic when that differs.  The
    Region is the scene window the result is pasted into: the bounding box of the shape's footprint cut at the image."""
    import numpy as np
    from . import paste_back as pb
    so, mo = np.array(scene), np.array(mask)
    shape = _module(path).plan(pb.grey_of(mo), cfg)
    if shape is None:
        return None
    x0, y0, x1, y1 = shape.window(scene.size)
    s, m = _warped_inputs(so, mo, warp, shape.forward(), (shape.rw, shape.rh), (shape.tw, shape.th))
    return s, m, so, mo, pb.Region(x0, y0, x1, y1, shape.tw, shape.th), shape


def _edit_inputs(scene, mask, cfg: Dict[str, Any], warp: Optional[Callable], warp_quad: Optional[Callable] = None,
                 warp_grid: Optional[Callable] = None):
    """(scene, mask, the Work's paste-back fields): _upright_inputs through the first of LINE_PATHS that the cfg asks for, whose warp
    is at hand and for which the line qualifies; _paste_back_inputs otherwise."""
    warps = dict(warp=warp, warp_quad=warp_quad, warp_grid=warp_grid)
    for path in LINE_PATHS:
        if warps[path.keyword] is not None and cfg.get(path.key):
            got = _upright_inputs(scene, mask, cfg, path, warps[path.keyword])
            if got is not None:
                scene, mask, so, mo, reg, rect = got
                return scene, mask, dict(orig_scene=so, orig_mask=mo, region=reg, rect=rect)
    scene, mask, so, mo, reg = _paste_back_inputs(scene, mask, cfg)
    return scene, mask, dict(orig_scene=so, orig_mask=mo, region=reg)


def prepare_eval_item(index: int, item: Dict[str, Any], original_images_dir: str, font, text_height_ratio: float = 0.1667,
                      loader: Optional[Callable] = None, device_compose: bool = False, paste_back: Optional[Dict[str, Any]] = None,
                      annotation: int = 0, warp: Optional[Callable] = None, warp_quad: Optional[Callable] = None,
                      warp_grid: Optional[Callable] = None) -> Work:
    """One `annos.json` entry -> Work (scripts/run_eval.py:76-112): scene = original_images_dir / img_name; mask = the first
    annotation's polygon filled white on black; glyph strip of height int(w * text_height_ratio) -- a fraction of the image
    WIDTH -- with the annotation's text, stacked on top with a black mask; pipeline size ((w // 32) * 32,
    ((h + strip) // 32) * 32); T5 prompt generate_prompt([text]).  annotation: which entry of `annotations` (the reference, and
    every caller but per-line editing, reads the first).  warp: the pipeline's warp_affine, given by per-line editing when
    paste_back["rectify"] is set: a slanted line is then edited upright (_upright_inputs).  warp_quad: the pipeline's
    warp_perspective, given when paste_back["perspective"] is set: a line seen in perspective is then cut as a quad.
    warp_grid: the pipeline's warp_grid, given when paste_back["curve"] is set: a line along a bend is then cut as a ribbon."""
    import numpy as np
    from PIL import Image
    load = loader or (lambda p: Image.open(p))
    ann = item["annotations"][annotation]
    text = ann["text"]
    scene = load(os.path.join(original_images_dir, item["img_name"])).convert("RGB")
    w, h = scene.size
    m = glyph.fill_polygon(h, w, ann["polygon"])
    extra = {}
    if paste_back is not None:       # the strip, the stacking and the sizes below are then those of the edited region
        scene, mk, extra = _edit_inputs(scene, Image.fromarray(m), paste_back, warp, warp_quad, warp_grid)
        (w, h), m = scene.size, np.array(mk)
    strip = int(w * text_height_ratio)
    g = np.array(glyph.draw_glyph(font, text, w, strip))
    meta = dict(mode="singleline", direction="vertical", strip=strip, orig_h=h)
    size = ((w // 32) * 32, ((h + strip) // 32) * 32)
    prompt = glyph.generate_prompt([text])
    name = os.path.basename(item["img_name"])
    if device_compose:
        return Work(index, None, None, prompt, meta, size, parts=(g, np.array(scene), m, False), name=name, texts=[text], **extra)
    combined = Image.fromarray(np.vstack((g, np.array(scene))))
    cmask = Image.fromarray(np.vstack((np.zeros_like(g), m)))
    return Work(index, combined.resize(size), cmask.resize(size), prompt, meta, size, name=name, texts=[text], **extra)


def prepare_item(index: int, item: Dict[str, Any], loader: Optional[Callable] = None, device_compose: bool = False,
                 eval_cfg: Optional[Dict[str, Any]] = None, paste_back: Optional[Dict[str, Any]] = None) -> Work:
    """Host-side preparation of one item (run_inference.py:395-467 up to the pipeline call).  With device_compose the
    stacking is left to the device when no resize is involved.  Items in the reference's `annos.json` schema (an `img_name`
    key) go through prepare_eval_item with eval_cfg = dict(original_images_dir, font, text_height_ratio).
    paste_back (_paste_back_cfg's dict): the Work also keeps the scene and mask as loaded and the edited Region; with a `region` the
    preparation below runs on that region's crop instead of the whole scene."""
    from PIL import Image
    if "img_name" in item:
        c = eval_cfg or {}
        return prepare_eval_item(index, item, c.get("original_images_dir", "."), c.get("font") or glyph.load_font(c.get("font_path")),
                                 c.get("text_height_ratio", 0.1667), loader, device_compose, paste_back)
    load = loader or (lambda p: Image.open(p))
    scene, mask = load(item["image"]).convert("RGB"), load(item["mask"]).convert("RGB")
    return prepare_plain(index, scene, mask, glyph.read_words_from_text(item["text"]), device_compose, paste_back)


def prepare_plain(index: int, scene, mask, words: Sequence[str], device_compose: bool = False,
                  paste_back: Optional[Dict[str, Any]] = None, warp: Optional[Callable] = None,
                  warp_quad: Optional[Callable] = None, warp_grid: Optional[Callable] = None) -> Work:
    """prepare_item's rule for an {image, mask, text} item whose RGB scene and mask are loaded and whose text is split into words.
    warp, warp_quad, warp_grid: as in prepare_eval_item."""
    from PIL import Image
    extra = {}
    if paste_back is not None:
        scene, mask, extra = _edit_inputs(scene, mask, paste_back, warp, warp_quad, warp_grid)
    g, s_, m, horizontal, meta = glyph.compose_parts(scene, mask, words)
    H, W = (s_.shape[0], g.shape[1] + s_.shape[1]) if horizontal else (g.shape[0] + s_.shape[0], s_.shape[1])
    w, h = (W // 32) * 32, (H // 32) * 32
    prompt = glyph.generate_prompt(words)
    if device_compose:               # stacking, the resize to (w, h) and the grey mask happen on the device, per batch
        return Work(index, None, None, prompt, meta, (w, h), parts=(g, s_, m, horizontal), texts=list(words), **extra)
    import numpy as np
    stack = np.hstack if horizontal else np.vstack
    combined, cmask = Image.fromarray(stack((g, s_))), Image.fromarray(stack((np.zeros_like(g), m)))
    return Work(index, combined.resize((w, h)), cmask.resize((w, h)), prompt, meta, (w, h), texts=list(words), **extra)


def _batch_inputs(items: Sequence[Work], device):
    """(image, mask_image) arguments of the pipeline call for one batch: device-composed uint8 canvases when every item of
    the batch brought its parts and they agree in shape, else the PIL lists."""
    import numpy as np
    from . import ops
    if all(w.parts is not None for w in items):
        shapes = {(w.parts[0].shape, w.parts[1].shape, w.parts[3]) for w in items}
        if len(shapes) == 1:
            up = lambda k: torch.from_numpy(np.stack([w.parts[k] for w in items])).to(device)
            wh = items[0].size
            canvas, cmask = ops.compose_canvas(up(0), up(1), up(2), horizontal=items[0].parts[3], mask_rgb=True)
            if (canvas.shape[2], canvas.shape[1]) != wh:     # the callers' resize to a multiple of 32 (PIL bicubic, bit-exact)
                canvas, cmask = ops.resample_u8(canvas, (wh[1], wh[0])), ops.resample_u8(cmask, (wh[1], wh[0]))
            return canvas, ops.rgb_to_grey(cmask)
    from PIL import Image
    imgs, masks = [], []
    for w in items:
        if w.parts is None:
            imgs.append(w.image), masks.append(w.mask)
        else:
            g, s_, m, horizontal = w.parts
            stack = np.hstack if horizontal else np.vstack
            imgs.append(Image.fromarray(stack((g, s_))).resize(w.size))
            masks.append(Image.fromarray(stack((np.zeros_like(g), m))).resize(w.size))
    return imgs, masks


def _paste_into_original(pipe, w: Work, cropped, cfg: Dict[str, Any]):
    """The item's cropped result -> its original scene with the edited region pasted in (PIL image at the scene's size).  Only the
    region's crop of the scene and mask and the cropped result visit the device (pipe.paste_back); the insertion into the copy of
    the scene is a host slice assignment."""
    import numpy as np
    from PIL import Image
    from . import paste_back as pb
    reg = w.region
    oc = w.orig_scene[reg.y0:reg.y1, reg.x0:reg.x1]
    om = pb.grey_of(w.orig_mask[reg.y0:reg.y1, reg.x0:reg.x1])
    kw = dict(color_match=cfg["color_match"]) if cfg.get("color_match") else {}      # passed only then: older pipelines keep working
    if cfg.get("seamless"):
        kw["seamless"] = cfg["seamless"]
    if cfg.get("grain"):                             # the grain is anchored at scene positions: the region's own place in the scene
        kw.update(grain=cfg["grain"], origin=(reg.x0, reg.y0))
    if cfg.get("keyed"):
        kw["keyed"] = cfg["keyed"]
    pasted = pipe.paste_back(oc, cropped, om, dilate=cfg["dilate"], feather=cfg["feather"], **kw)
    pasted = pasted.cpu().numpy() if isinstance(pasted, torch.Tensor) else np.asarray(pasted)
    out = w.orig_scene.copy()
    out[reg.y0:reg.y1, reg.x0:reg.x1] = pasted.reshape(oc.shape)
    return Image.fromarray(out)


def image_tokens(size: Tuple[int, int]) -> int:
    """Image tokens of a (width, height) pipeline size: one per 16 x 16 pixels (8x VAE, 2 x 2 patches)."""
    return (size[0] // 16) * (size[1] // 16)


def pad_fraction(sizes: Sequence[Tuple[int, int]], text_tokens: int = 512) -> float:
    """Share of a batch's transformer rows that are padding: 1 - sum(L_b) / (B * N), L_b = text_tokens + image tokens of item b,
    N = the longest L_b rounded up to a multiple of 256 (call_mixed's launch length).  0 for a batch of one size: it runs unpadded on
    the uniform path."""
    if len(set(tuple(s) for s in sizes)) <= 1:
        return 0.0
    lens = [text_tokens + image_tokens(s) for s in sizes]
    n = (max(lens) + 255) // 256 * 256
    return 1.0 - sum(lens) / (len(lens) * n)


def plan_batches(works: Sequence[Work], batch_size: int, max_pad_fraction: float = 0.0, text_tokens: int = 512, group: int = 1) -> List[Batch]:
    """Same-geometry batches of up to batch_size items, deterministic (every rank computes the same plan): geometries in
    order of first appearance, items in list order.
    group > 1 (candidates with prune; candidates.py): the works come in runs of `group` adjacent works of one geometry, the candidates
    of one work, and no run straddles two batches -- a batch holds batch_size // group whole runs; group <= batch_size, not with
    max_pad_fraction > 0.
    max_pad_fraction > 0: items of different sizes may share a batch (Batch.mixed; FluxFillPipeline.call_mixed pads their rows to
    the longest).  Greedy over the items sorted by image token count (stable: ties keep list order): the next item joins the open
    batch unless the batch is full or pad_fraction of the batch with it would exceed the cap, in which case the batch is closed.
    text_tokens: the T5 sequence length every item carries (max_sequence_length)."""
    if max_pad_fraction < 0 or max_pad_fraction >= 1:
        raise ValueError("max_pad_fraction must be in [0, 1)")
    if group < 1 or group > batch_size or (group > 1 and max_pad_fraction > 0):
        raise ValueError(f"group must be in 1..batch_size = {batch_size} and 1 with max_pad_fraction > 0, got {group}")
    if max_pad_fraction > 0:
        out: List[Batch] = []
        cur: List[Work] = []
        close = lambda: out.append(Batch(cur[-1].size, list(cur), mixed=len({w.size for w in cur}) > 1))
        for w in sorted(works, key=lambda w: image_tokens(w.size)):
            if cur and (len(cur) >= batch_size or pad_fraction([x.size for x in cur] + [w.size], text_tokens) > max_pad_fraction):
                close()
                cur = []
            cur.append(w)
        if cur:
            close()
        return out
    by_size: Dict[Tuple[int, int], List[Work]] = {}
    for w in works:
        by_size.setdefault(w.size, []).append(w)
    out: List[Batch] = []
    per_batch = batch_size // group * group
    for size, ws in by_size.items():
        for i in range(0, len(ws), per_batch):
            out.append(Batch(size, list(ws[i:i + per_batch])))
    return out


def rank_plans(works: Sequence[Work], world: int, batch_size: int, max_pad_fraction: float = 0.0, text_tokens: int = 512,
               per_line: bool = False, group: int = 1) -> List[List[Batch]]:
    """plans[k][r] = the batch rank k runs in round r; deterministic, so every rank computes all of them.  Batches are dealt
    round-robin: plans[k] = plan_batches(works)[k::world], i.e. plans[k][r] = plan[r world + k].  per_line: ITEMS are dealt round-robin
    instead (in order of first appearance of Work.index) and each rank plans the lines of its own items, so all lines of an item run on
    the rank that pastes them together.  Candidates deal items whole in the same way (run_items passes per_line=True for them: all
    candidates of a work meet on the rank that chooses among them); group: plan_batches' group."""
    if not per_line:
        plan = plan_batches(works, batch_size, max_pad_fraction, text_tokens, group)
        return [plan[k::world] for k in range(world)]
    owner = {idx: n % world for n, idx in enumerate(dict.fromkeys(w.index for w in works))}
    return [plan_batches([w for w in works if owner[w.index] == k], batch_size, max_pad_fraction, text_tokens, group) for k in range(world)]


def _scatter(rows: Optional[List[torch.Tensor]], shape, dtype, device) -> torch.Tensor:
    """Rank 0 passes one tensor per rank, every rank receives its own."""
    world = dist.get_world_size() if dist.is_initialized() else 1
    if world == 1:
        return rows[0]
    out = torch.empty(shape, dtype=dtype, device=device)
    dist.scatter(out, [r.contiguous() for r in rows] if dist.get_rank() == 0 else None, src=0)
    return out


def _flag_min(v: int, device) -> int:
    """min over ranks of an int (1 rank: the value itself)."""
    if not dist.is_initialized() or dist.get_world_size() == 1:
        return v
    t = torch.tensor([v], dtype=torch.int32, device=device)
    dist.all_reduce(t, op=dist.ReduceOp.MIN)
    return int(t.item())


@torch.no_grad()
def run_items(items: Sequence[Dict[str, Any]], pipe, out_dir: Optional[str], batch_size: int = 8, num_inference_steps: int = 30,
              guidance_scale: float = 30.0, seed: int = 42, device="cuda", loader: Optional[Callable] = None,
              save: Optional[Callable] = None, max_sequence_length: int = 512, eval_cfg: Optional[Dict[str, Any]] = None,
              encode: str = "auto", save_full: Optional[Callable] = None, mixed_pad: float = 0.0,
              step_cache: Optional[Dict[str, Any]] = None, paste_back: Optional[Dict[str, Any]] = None, keep_known=None,
              strength: float = 1.0, change_map=None, true_cfg: float = 1.0, negative_prompt: Optional[str] = None,
              ocr: Optional[Dict[str, Any]] = None, candidates=None) -> Dict[str, Any]:
    """Runs the whole list; returns {"done": [indices this rank wrote], "failed": [...], "all_done": [...] on rank 0,
    "encode": "local" | "rank0"}.  `pipe` needs `encode_prompt(prompt, prompt_2, ...)` and the FluxFillPipeline `__call__`.
    encode: "local" = every rank encodes the T5 prompts of its own batches (needs a T5 on every rank), "rank0" = rank 0
    encodes for all and scatters, "auto" = local when every rank has `pipe.text_encoder_2`, else rank0.
    Outputs: eval-schema items (Work.name set) are written as out_dir/full_images/<name> and out_dir/cropped_images/<name>
    (or handed to save_full(work, full, cropped)); other items as out_dir/<index>.png (or save(index, cropped)).
    mixed_pad: plan_batches' max_pad_fraction -- > 0 lets items of different sizes share a batch (pipe.call_mixed) as long as at
    most that share of the batch's rows is padding; 0 (default) = same-geometry batches only.
    step_cache: None, or the keyword arguments of pipe.enable_step_cache (threshold, skip_steps, max_consecutive): the first-block step
    cache is switched on for the run (and off again afterwards); the result then carries "steps_skipped" / "steps_total" over this
    rank's batches.  Each rank decides alone from its own batch's metrics; not with mixed_pad > 0.
    paste_back: None (the outputs are the pipeline's own pixels at pipeline size), or dict(dilate, feather, region): every item's cropped
    result is blended back into its ORIGINAL scene under the dilated and feathered mask (pipe.paste_back), and the image that is saved /
    written as <index>.png / written under cropped_images/ / passed as `cropped` to save_full is that scene at its original size, changed
    only near the mask (full_images/ stays the raw canvas).  region: None = the whole scene goes through the pipeline as before;
    dict(pad, min_side, max_side) (paste_back.select_region) = only a region around the mask does, resized to at most max_side, so a
    large photo costs what its mask's neighbourhood costs.  Not with mixed_pad > 0.
    Two more keys, both opt-in (DESIGN.md section 4 "Per-line edits"): per_line=True (implies region, {} when absent) edits every text
    line of an item -- a connected region of the mask with its line of the text, or an entry of an eval item's `annotations` -- as a
    single-line item of its own, with its own region, and pastes all of them into the one scene in split order (per_line.py); items
    are then dealt to the ranks whole, and full_images/ holds line 0's raw canvas under <name>, line k >= 1 under <stem>_line<k><ext>
    (save_full receives line 0's Work and canvas).  A failing line fails its item.  color_match=True | dict(ring, gain, max_shift,
    min_pixels) matches each pasted edit's colours to the original's on a ring just outside the blend (paste_back.paste).
    rectify=True | dict(min_angle, max_angle, min_aspect) (with per_line; DESIGN.md section 4 "Rectified lines"): a line whose
    minimum-area rectangle is slanted by min_angle..max_angle degrees (defaults 5 and 45) and at least min_aspect (1.5) times as long
    as thick is cut as an oriented rectangle, warped upright on the device (pipe.warp_affine), edited upright and warped back into the
    scene under the same alpha; every other line is edited as without the key.
    perspective=True | dict(max_fit, max_taper, min_aspect, max_angle) (with per_line; DESIGN.md section 4 "Perspective lines"): a line
    whose outline is a tapering quadrilateral (perspective.is_perspective) is cut through the homography of that quad, warped upright on
    the device (pipe.warp_perspective), edited upright and warped back under the same alpha.  It is tried before rectify; both may be set.
    curve=True | dict(min_bend, max_squeeze, max_turn, min_aspect, min_fill, max_angle) (with per_line; DESIGN.md section 4 "Curved
    lines"): a line whose centre line bends (curve.is_curved) is cut as a ribbon around that centre line, warped upright on the device
    through a control grid (pipe.warp_grid), edited upright and warped back under the same alpha.  It is tried first; all three may be
    set.
    seamless=True | dict(smooth, max_shift) (DESIGN.md section 4 "Seamless paste"; with or without per_line, region and the three
    warps): the final blend of every paste adds a membrane to the edit first -- its difference to the original scene, known just outside
    the blend, interpolated across the blend's support by a pull-push pyramid, smoothed by `smooth` Jacobi sweeps (default 8) and clamped
    to +- max_shift grey levels (default 32) -- so that the edit meets the scene at the seam; with color_match the table is fitted as
    before and the membrane removes what it leaves.  The bytes outside the grown mask stay the original's.
    grain=True | dict(ring, max_sigma, strength, min_pixels, seed) (DESIGN.md section 4 "Grain match"; with or without the keys above):
    after the final blend of every paste the noise level of the original scene on a ring just outside the blend and that of the pasted
    pixels are estimated, and the missing variance -- at most max_sigma grey levels (default 6), times strength (default 1) -- is added
    as hashed white grain under the same alpha, anchored at scene positions.  The bytes outside the grown mask stay the original's.
    With grain=dict(spectrum=True | dict(max_blur, luma), ...) (DESIGN.md section 4 "Grain spectrum") the grain is blurred over
    neighbouring pixels (a 3-tap kernel whose side tap is at most max_blur / 256, default 64) and, with luma (default True), shared
    between the channels, as far as the scene's own noise on the ring is.
    keyed=True | dict(lo, hi, dilate, feather, noise, ring, min_pixels) (DESIGN.md section 4 "Keyed paste"; with or without the keys
    above): behind the blend of every paste and in front of its grain, the blend's difference to the scene is measured (a 3 x 3 weighted
    sum per channel), thresholded with hysteresis at lo / hi grey levels (defaults 10 and 28; the lower one stays `noise`, default 3,
    standard deviations of the scene's noise on the ring above zero), grown by `dilate` and feathered by `feather` (6 and 2) into a key,
    and the blend goes over the scene once more under that key: a pixel inside the mask that the edit did not change keeps the scene's
    byte.  The bytes outside the grown mask stay the original's.
    keep_known=True | dict(mode, grow) and strength (DESIGN.md section 4 "Known-region sampling"): handed to every pipeline call as
    they are -- the canvas outside the mask is then kept in the latents at every step, and the loop runs int(steps * strength) steps
    from the noised canvas.  Paste-back runs after decode, unchanged.  Not with mixed_pad > 0.
    change_map (DESIGN.md section 4 "Change-map sampling"): handed to every pipeline call as it is -- True or dict(dilate, feather, mode,
    grow, last) derives the map inside each call from that call's own mask, so it composes with paste_back, region, per_line and the
    warps with no further work (every line's call sees its own line's mask); an explicit map (an image, or dict(map=...)) must have the
    calls' size.  Not with keep_known, not with mixed_pad > 0.
    true_cfg, negative_prompt (DESIGN.md section 4 "True CFG"): one negative prompt string for all items and the guidance scale against
    it, handed to every pipeline call as they are (the calls behind paste_back, region and per_line included) when true_cfg > 1 and a
    negative prompt is given; every step then runs on twice the batch.  Not with mixed_pad > 0, not with step_cache.
    ocr (DESIGN.md section 4 "Read-back"): None, or dict(weights, lang='ch' | 'en', dict_path, image_shape=(3, 48, 320), batch=6): after an
    item's image is final -- the pasted scene with paste_back, else the pipeline-size result -- every line of it (ocr.item_lines) is
    cropped from that image, read by the recogniser and scored against its text; the result then carries "ocr": {item index: [{text,
    pred, seq_acc, ned, ctc_loss}]} for this rank's items.  Without the key nothing is constructed or launched.
    candidates (DESIGN.md section 4 "Candidates"; needs ocr): None, a count N, or dict(n, prune=None | dict(at, keep=1), seeds=None).
    Every work -- an item, or a line of an item with per_line -- is run as n candidates that differ in the seed (seed + k, or seeds[k]),
    adjacent in the plan; items are dealt to the ranks whole.  Every candidate is read on its own pipeline-size result (a device uint8
    tensor, TextRecognizer.read_device: one gather launch per batch) where the work's own pipeline mask says its lines are, and per work
    the smallest (lines not read exactly, sum of ctc_loss, k) wins.  Only the winner is converted, pasted and saved, by the code that
    serves a run without the key; the result carries "candidates": {item: [{line, seeds, chosen (the winner's position k), scores:
    [{seed, line, text, pred, seq_acc, ned, ctc_loss, stage}]}]}.  prune=dict(at=p, keep=K): a batch runs steps 0..p-1
    (step_window=(0, p)), the clean-image estimates (pipe.x0_preview) are decoded, read and ranked by the same rule (stage
    "preview"), and the K best of every work are finished on the smaller batch (step_window=(p, n)) and read again (stage "final").
    The n candidates of a work then share a batch (n <= batch_size), and what step_window refuses is refused here, up front.  None or
    n == 1 issues exactly the calls of a run without the key.  Not with mixed_pad > 0.  No quality claim is made: no real checkpoint
    or recogniser weights exist here, so there is no default n and no recommended prune step."""
    if ocr is not None:              # refused before anything is prepared or encoded
        from . import ocr as rb
        ocr = rb.ocr_cfg(ocr)
    cand = None
    if candidates is not None:       # refused before anything is prepared or encoded
        from . import candidates as cd
        cand = cd.candidates_cfg(candidates, seed, num_inference_steps, batch_size)
    if cand is not None:
        if ocr is None:
            raise ValueError("candidates needs ocr=dict(...): the reader and its dictionary choose among them")
        if mixed_pad > 0:
            raise NotImplementedError("candidates do not serve mixed-geometry batches (mixed_pad > 0)")
        if cand["prune"] is not None:
            from . import step_loop
            step_loop.refuse_step_window(getattr(pipe, "scheduler", None), strength, keep_known, change_map,
                                         negative_prompt is not None and true_cfg > 1, step_cache is not None)
            if not hasattr(pipe, "decode_latents"):
                raise ValueError("candidates with prune need a pipeline with step_window and decode_latents (FluxFillPipeline)")
    known = {}
    if negative_prompt is not None and not isinstance(negative_prompt, str):
        raise ValueError("negative_prompt is one string for all items")
    if negative_prompt is not None and true_cfg > 1:
        if mixed_pad > 0:
            raise NotImplementedError("true_cfg / negative_prompt (true CFG) do not serve mixed-geometry batches (mixed_pad > 0)")
        if step_cache is not None:
            raise NotImplementedError("true_cfg / negative_prompt (true CFG) do not run with step_cache")
        known["true_cfg"], known["negative_prompt"] = float(true_cfg), negative_prompt
    if change_map is not None and change_map is not False:
        if keep_known:
            raise ValueError("change_map and keep_known exclude each other")
        if mixed_pad > 0:
            raise NotImplementedError("change_map (change-map sampling) does not serve mixed-geometry batches (mixed_pad > 0)")
        known["change_map"] = change_map
    if keep_known:
        known["keep_known"] = keep_known
    if strength != 1.0:
        if strength < 0 or strength > 1:
            raise ValueError(f"The value of strength should in [0.0, 1.0] but is {strength}")
        known["strength"] = strength
    if known and mixed_pad > 0:
        raise NotImplementedError("keep_known / strength (known-region sampling) do not serve mixed-geometry batches (mixed_pad > 0)")
    if paste_back is not None:       # refused before anything is prepared or encoded
        if mixed_pad > 0:
            raise NotImplementedError("paste_back does not serve mixed-geometry batches (mixed_pad > 0)")
        if not hasattr(pipe, "paste_back"):
            raise ValueError("paste_back needs a pipeline with paste_back (FluxFillPipeline)")
        paste_back = _paste_back_cfg(paste_back)
        pipeline_warps(pipe, paste_back)
    if step_cache is not None:
        if mixed_pad > 0:
            raise NotImplementedError("step_cache does not serve mixed-geometry batches (mixed_pad > 0)")
        if not hasattr(pipe, "enable_step_cache"):
            raise ValueError("step_cache needs a pipeline with enable_step_cache (FluxFillPipeline)")
        pipe.enable_step_cache(**step_cache)
        try:
            return _run_items(items, pipe, out_dir, batch_size, num_inference_steps, guidance_scale, seed, device, loader, save,
                              max_sequence_length, eval_cfg, encode, save_full, mixed_pad, count_steps=True, paste_back=paste_back, known=known,
                              ocr=ocr, cand=cand)
        finally:
            pipe.disable_step_cache()
    return _run_items(items, pipe, out_dir, batch_size, num_inference_steps, guidance_scale, seed, device, loader, save,
                      max_sequence_length, eval_cfg, encode, save_full, mixed_pad, paste_back=paste_back, known=known, ocr=ocr, cand=cand)


def _run_items(items, pipe, out_dir, batch_size, num_inference_steps, guidance_scale, seed, device, loader, save, max_sequence_length,
               eval_cfg, encode, save_full, mixed_pad, count_steps: bool = False, paste_back: Optional[Dict[str, Any]] = None,
               known: Optional[Dict[str, Any]] = None, ocr: Optional[Dict[str, Any]] = None,
               cand: Optional[Dict[str, Any]] = None) -> Dict[str, Any]:
    steps_skipped = steps_total = 0
    read: Dict[int, Any] = {}       # ocr: item index -> its lines' records
    reader: List[Any] = []          # the recogniser, made when the first image is final

    def read_back(index, final):
        from . import ocr as rb
        if not reader:
            reader.append(rb.make_reader(ocr, device))
        size, item_ln = rb.item_lines(items[index], loader, eval_cfg)
        read[index] = rb.read_lines(reader[0], final, size, item_ln, device)
    if mixed_pad > 0:            # refused before anything is prepared or encoded, not batch by batch inside the loop
        if not hasattr(pipe, "call_mixed"):
            raise ValueError("mixed_pad > 0 needs a pipeline with call_mixed (FluxFillPipeline)")
        from .schedulers import FlowMatchMultistepScheduler, StochasticRFOvershotDiscreteScheduler
        if isinstance(getattr(pipe, "scheduler", None), StochasticRFOvershotDiscreteScheduler):
            raise NotImplementedError("mixed_pad > 0 needs the Euler sampler: mixed-geometry batches carry per-sample coefficients only "
                                      "in the fused Euler step (the AMO sampler's are per step); use mixed_pad=0")
        if isinstance(getattr(pipe, "scheduler", None), FlowMatchMultistepScheduler):
            raise NotImplementedError("mixed_pad > 0 needs the Euler sampler: mixed-geometry batches carry per-sample coefficients only "
                                      "in the fused Euler step (the multistep sampler's are per step); use mixed_pad=0")
    rank = dist.get_rank() if dist.is_initialized() else 0
    world = dist.get_world_size() if dist.is_initialized() else 1
    per_line = bool(paste_back and paste_back.get("per_line"))
    works, failed = [], []
    lines: Dict[int, List[Work]] = {}        # per_line: item index -> its lines in split order; results[item][line] = (canvas, crop)
    results: Dict[int, Dict[int, Any]] = {}
    for i, it in enumerate(items):
        try:
            device_compose = bool(getattr(pipe, "supports_device_compose", False))
            if per_line:
                from . import per_line as pl
                lines[i] = pl.prepare_lines(i, it, loader, device_compose, eval_cfg, paste_back, **pipeline_warps(pipe, paste_back))
                works.extend(lines[i])
            else:
                works.append(prepare_item(i, it, loader, device_compose=device_compose,
                                          eval_cfg=eval_cfg, **({} if paste_back is None else dict(paste_back=paste_back))))
        except Exception as e:       # per-item failures do not stop the run (reference :195-198)
            failed.append(i)
            if rank == 0:
                print(f"item {i} failed in preparation: {e}")
    if cand is None:
        plans = rank_plans(works, world, batch_size, mixed_pad, max_sequence_length, per_line)
    else:                        # every work becomes its n candidates, adjacent; items are dealt to the ranks whole, as per_line deals them
        from . import candidates as cd
        works = cd.expand(works, cand)
        plans = rank_plans(works, world, batch_size, mixed_pad, max_sequence_length, True, cand["n"] if cand["prune"] else 1)
    cand_pending: Dict[Any, Dict[int, Any]] = {}     # (item, line) -> {k: (line records, the pipeline-size result, device uint8)}
    cand_scores: Dict[Any, List[Any]] = {}          # (item, line) -> every record of the work's candidates, preview and final
    cand_report: Dict[int, List[Any]] = {}          # the result's "candidates"
    cand_lines: Dict[Any, Any] = {}                 # (item, line) -> where the work's lines are on its canvas

    def get_reader():
        from . import ocr as rb
        if not reader:
            reader.append(rb.make_reader(ocr, device))
        return reader[0]

    def cand_masks(mask_in):
        """the batch's pipeline masks as host grey arrays [H, W]"""
        import numpy as np
        if isinstance(mask_in, torch.Tensor):
            m = mask_in.cpu().numpy()
            return [m[j][..., 0] if m[j].ndim == 3 else m[j] for j in range(m.shape[0])]
        return [np.array(m.convert("L")) for m in mask_in]

    def cand_settle(batch_items, recs, images_u8):
        """files a batch's final records and results; -> [(the winning Work, its result as a PIL image)] of the works that are complete"""
        from PIL import Image
        won = []
        for w, r, u8 in zip(batch_items, recs, images_u8):
            key = cd.group_key(w)
            cand_pending.setdefault(key, {})[w.cand] = (w, r, u8)
            cand_scores.setdefault(key, []).extend(r)
        for key in dict.fromkeys(cd.group_key(w) for w in batch_items):
            got = cand_pending[key]
            want = cand["prune"]["keep"] if cand["prune"] else cand["n"]
            if len(got) < want:
                continue
            ks = sorted(got)
            k = ks[cd.choose([got[k][1] for k in ks])[0]]
            cand_report.setdefault(key[0], []).append(dict(line=key[1], seeds=list(cand["seeds"]), chosen=k, scores=cand_scores.pop(key)))
            won.append((got[k][0], Image.fromarray(got[k][2].cpu().numpy())))
            del cand_pending[key]
        return won

    def cand_batch(mine, call, gens, pe, pooled):
        """One batch of candidates -> cand_settle's winners.  call(**kw): the pipeline call of this batch with the arguments every call of
        it shares.  Without prune: one call, every result read at pipeline size.  With prune: steps 0..p-1, the estimates read and
        ranked, the survivors of every work finished on the smaller batch and read again."""
        img_in, mask_in = _batch_inputs(mine.items, device)
        masks = cand_masks(mask_in)
        size = dict(height=mine.size[1], width=mine.size[0])
        if cand["prune"] is None:
            images = call(image=img_in, mask_image=mask_in, generator=gens, prompt_embeds=pe, pooled_prompt_embeds=pooled, output_type="u8",
                          **size).images
            return cand_settle(mine.items, cd.score_batch(get_reader(), images, mine.items, masks, "final", cand_lines), images)
        p, keep = cand["prune"]["at"], cand["prune"]["keep"]
        lat = call(image=img_in, mask_image=mask_in, generator=gens, prompt_embeds=pe, pooled_prompt_embeds=pooled, output_type="latent",
                   step_window=(0, p), **size).images
        cond = pipe.window_conditioning
        previews = pipe.decode_latents(pipe.x0_preview, mine.size[1], mine.size[0], "u8")
        recs = cd.score_batch(get_reader(), previews, mine.items, masks, "preview", cand_lines)
        groups: Dict[Any, List[int]] = {}
        for j, w in enumerate(mine.items):
            groups.setdefault(cd.group_key(w), []).append(j)
            cand_scores.setdefault(cd.group_key(w), []).extend(recs[j])
        alive = sorted(js[o] for js in groups.values() for o in cd.choose([recs[j] for j in js], keep))    # batch order, so k order per work
        idx = torch.tensor(alive, dtype=torch.long, device=lat.device)
        images = call(masked_image_latents=cond[idx], latents=lat[idx], generator=[gens[j] for j in alive], prompt_embeds=pe[idx],
                      pooled_prompt_embeds=pooled[idx], output_type="u8", step_window=(p, num_inference_steps), **size).images
        items = [mine.items[j] for j in alive]
        return cand_settle(items, cd.score_batch(get_reader(), images, items, [masks[j] for j in alive], "final", cand_lines), images)
    rounds = max(len(p) for p in plans)
    if encode == "auto":
        has_t5 = 1 if (getattr(pipe, "text_encoder_2", None) is not None or getattr(pipe, "encodes_locally", False)) else 0
        encode = "local" if _flag_min(has_t5, device) == 1 else "rank0"
    if encode not in ("local", "rank0"):
        raise ValueError("encode must be 'auto', 'local' or 'rank0'")
    # ---- the CLIP prompt is one fixed template: pooled embedding encoded once on rank 0, broadcast once.  meta[0] < 0 is the
    # abort flag: a failure on rank 0 reaches every rank through the same broadcast the others are waiting in
    pooled1 = None
    err0 = None
    if rank == 0:
        try:
            pe1, pooled1, _ = pipe.encode_prompt(prompt=glyph.PROMPT_TEMPLATE2, prompt_2=glyph.PROMPT_TEMPLATE2, device=device,
                                                 max_sequence_length=max_sequence_length)
            meta = [pe1.shape[1], pe1.shape[2], pooled1.shape[1], {torch.bfloat16: 0, torch.float32: 1, torch.float16: 2}[pe1.dtype]]
        except Exception as e:
            err0, meta = e, [-1, 0, 0, 0]
    else:
        meta = [0, 0, 0, 0]
    grouped = dist.is_initialized()      # also at world size 1 under a launcher: a 1-GPU torchrun job runs the code of the 8-GPU job
    if grouped:
        mt = torch.tensor(meta, dtype=torch.int64, device=device)
        dist.broadcast(mt, src=0)
        tdist._ran("broadcast")
        meta = [int(v) for v in mt.tolist()]
    if meta[0] < 0:
        raise RuntimeError(f"rank 0 could not encode the prompt template: {err0}" if rank == 0 else
                           "rank 0 could not encode the prompt template (see its log)")
    T, J, P, dcode = meta
    dtype = {0: torch.bfloat16, 1: torch.float32, 2: torch.float16}[dcode]
    if rank != 0:
        pooled1 = torch.empty(1, P, dtype=dtype, device=device)
    if grouped:
        dist.broadcast(pooled1, src=0)
        tdist._ran("broadcast")
    done: List[int] = []
    for r in range(rounds):
        mine = plans[rank][r] if r < len(plans[rank]) else None
        pe_mine, enc_ok = None, True
        if encode == "rank0":
            # ---- rank 0 encodes the T5 prompts of every rank's batch of this round (padded to batch_size rows, one more row
            # whose first element is the ok flag) and scatters; a failed encode sends zero rows + flag 0 -- collectives stay matched
            rows = None
            if rank == 0:
                rows = []
                for k in range(world):
                    b = plans[k][r] if r < len(plans[k]) else None
                    buf = torch.zeros(batch_size + 1, T, J, dtype=dtype, device=device)
                    buf[batch_size, 0, 0] = 1
                    if b is not None:
                        try:
                            prompts = [w.prompt for w in b.items]
                            pe, _, _ = pipe.encode_prompt(prompt=[glyph.PROMPT_TEMPLATE2] * len(prompts), prompt_2=prompts,
                                                          device=device, max_sequence_length=max_sequence_length)
                            buf[:len(prompts)] = pe.to(dtype)
                        except Exception as e:
                            buf[batch_size, 0, 0] = 0
                            print(f"[rank 0] encoding the prompts of rank {k}'s batch of round {r} failed: {e}")
                    rows.append(buf)
            got = _scatter(rows, (batch_size + 1, T, J), dtype, device)
            pe_mine, enc_ok = got[:batch_size], bool(float(got[batch_size, 0, 0]) != 0)
        if mine is None:
            continue
        n = len(mine.items)
        try:
            if not enc_ok:
                raise RuntimeError("rank 0 failed to encode this batch's prompts")
            if encode == "local":   # this rank's own prompts, no collective: nobody waits for anybody
                prompts = [w.prompt for w in mine.items]
                pe_mine, _, _ = pipe.encode_prompt(prompt=[glyph.PROMPT_TEMPLATE2] * n, prompt_2=prompts, device=device,
                                                   max_sequence_length=max_sequence_length)
                pe_mine = pe_mine.to(dtype)
            # run_inference.py:76, per image; a candidate carries its own seed
            gens = [torch.Generator(device=device).manual_seed(int(seed if w.seed is None else w.seed)) for w in mine.items]
            boxes = [glyph.crop_box(w.size, w.meta) for w in mine.items]
            keep_full = any(w.name is not None for w in mine.items)   # eval schema: the uncropped result is an output too
            same_box = all(bx == boxes[0] for bx in boxes)      # one crop window for the whole batch: applied on the device
            kw = (dict(output_crop=boxes[0]) if same_box and not keep_full and not mine.mixed and getattr(pipe, "supports_output_crop", False)
                  else {})
            call_kw = dict(kw, **(known or {}))     # keep_known / strength / change_map: only when given, so that other pipelines' calls stay as they were
            finished = None
            if cand is not None:    # read at pipeline size, so no crop on the device; only the winners go on, through the code below
                kw = {}
                call = lambda **k: pipe(num_inference_steps=num_inference_steps, max_sequence_length=max_sequence_length,
                                        guidance_scale=guidance_scale, **k, **(known or {}))
                finished = [(w, img, glyph.crop_box(w.size, w.meta))
                            for w, img in cand_batch(mine, call, gens, pe_mine[:n], pooled1.expand(n, -1).contiguous())]
            elif mine.mixed:        # items of different sizes: one padded forward per step, every item at its own size
                img_in, mask_in = _batch_inputs(mine.items, device)
                images = pipe.call_mixed(image=img_in, mask_image=mask_in, sizes=[w.size for w in mine.items],
                                         num_inference_steps=num_inference_steps, generator=gens,
                                         max_sequence_length=max_sequence_length, guidance_scale=guidance_scale,
                                         prompt_embeds=pe_mine[:n], pooled_prompt_embeds=pooled1.expand(n, -1).contiguous()).images
            else:
                img_in, mask_in = _batch_inputs(mine.items, device)
                images = pipe(height=mine.size[1], width=mine.size[0], image=img_in,
                              mask_image=mask_in, num_inference_steps=num_inference_steps, generator=gens,
                              max_sequence_length=max_sequence_length, guidance_scale=guidance_scale,
                              prompt_embeds=pe_mine[:n], pooled_prompt_embeds=pooled1.expand(n, -1).contiguous(), **call_kw).images
            if count_steps:
                rep = getattr(pipe, "step_cache_report", None) or []
                steps_total += len(rep)
                steps_skipped += sum(1 for r_ in rep if r_["skipped"])
            for w, img, bx in (zip(mine.items, images, boxes) if finished is None else finished):
                cropped = img if kw else img.crop(bx)
                if per_line:         # kept until the item's last line is in; then all of them are pasted into the one scene
                    got = results.setdefault(w.index, {})
                    got[w.line] = (img, cropped)
                    if w.index in failed or len(got) < len(lines[w.index]):
                        continue
                    try:
                        from . import per_line as pl
                        ws = lines[w.index]
                        pasted = pl.compose_lines(pipe, ws, [got[x.line][1] for x in ws], paste_back)
                        if ocr is not None:
                            read_back(w.index, pasted)
                        pl.write_item(ws, [got[x.line][0] for x in ws], pasted, out_dir, save, save_full)
                        done.append(w.index)
                    except Exception as e:
                        failed.append(w.index)
                        print(f"[rank {rank}] pasting the {len(lines[w.index])} lines of item {w.index} failed: {e}")
                    finally:
                        del results[w.index]
                    continue
                if paste_back is not None:
                    cropped = _paste_into_original(pipe, w, cropped, paste_back)
                if ocr is not None:
                    read_back(w.index, cropped)
                if w.name is not None and (save_full is not None or (save is None and out_dir is not None)):
                    if save_full is not None:
                        save_full(w, img, cropped)
                    else:
                        img.save(os.path.join(out_dir, "full_images", w.name))
                        cropped.save(os.path.join(out_dir, "cropped_images", w.name))
                elif save is not None:
                    save(w.index, cropped)
                elif out_dir is not None:
                    cropped.save(os.path.join(out_dir, f"{w.index:06d}.png"))
                done.append(w.index)
        except Exception as e:
            failed.extend([i for i in dict.fromkeys(w.index for w in mine.items) if not (per_line and (i in failed or i in done))])
            print(f"[rank {rank}] batch of {n} at {mine.size} failed: {e}")
    # ---- summary on rank 0
    res: Dict[str, Any] = {"done": done, "failed": failed, "batches": sum(len(p) for p in plans), "rounds": rounds, "encode": encode}
    if count_steps:
        res["steps_skipped"], res["steps_total"] = steps_skipped, steps_total
    if ocr is not None:
        res["ocr"] = read
    if cand is not None:
        res["candidates"] = {i: sorted(v, key=lambda e: e["line"]) for i, v in cand_report.items()}
    if grouped:
        cnt = torch.zeros(len(items) + 1, dtype=torch.int32, device=device)
        for i in done:
            cnt[i] = 1
        dist.all_reduce(cnt)
        tdist._ran("all_reduce")
        res["all_done"] = [i for i in range(len(items)) if int(cnt[i]) > 0]
        tdist.barrier()
    else:
        res["all_done"] = sorted(done)
    return res
