"""Per-line region edits (DESIGN.md section 4 "Per-line edits"): a scene with K text lines is edited as K single-line items, each
through its own region around its own line and with a single-line glyph strip, and all K results are pasted into the ONE original
scene.  Opt-in (paste_back=dict(per_line=True)); the multi-line canvas of glyph.compose_parts stays the default.

No reference counterpart: the reference renders all lines onto one full-size glyph image and stacks it with the scene
(run_inference.py:330-376, 409-467), and its eval driver edits the first annotation only (scripts/run_eval.py:76-112).  What a
line is follows the reference's own rule (glyph.mask_regions: 8-connected regions of the mask, top-to-bottom then left-to-right, at
least min_area large; region i gets text i), so the pairing of texts and regions is the one render_multiline makes.
"""
from __future__ import annotations

import os
from typing import Any, Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import glyph


def split_lines(mask, texts: Sequence[str], min_area: int = 50) -> List[Tuple[int, str, np.ndarray]]:
    """[(region index, text, line mask)] in the reference's order: region i of glyph.mask_regions(mask, min_area) gets texts[i];
    regions beyond len(texts) and blank texts are dropped, as in glyph.render_multiline.  A line's mask has the mask's shape and
    dtype (PIL image or uint8 array, [H, W] or [H, W, 3]) and holds the mask's own values on the region's pixels, 0 elsewhere."""
    from PIL import Image
    img = mask if isinstance(mask, Image.Image) else Image.fromarray(np.asarray(mask))
    m = np.array(img)
    out = []
    for i, region in enumerate(glyph.mask_regions(img, min_area)):
        if i >= len(texts):
            break
        text = texts[i].strip()
        if not text:
            continue
        pts = region[4]
        lm = np.zeros_like(m)
        lm[pts[:, 1], pts[:, 0]] = m[pts[:, 1], pts[:, 0]]
        out.append((i, text, lm))
    return out


def prepare_scene_lines(index: int, scene, mask, texts: Sequence[str], cfg: Dict[str, Any], device_compose: bool = False,
                        warp: Optional[Callable] = None, warp_quad: Optional[Callable] = None,
                        warp_grid: Optional[Callable] = None) -> List[Any]:
    """The single-line Works of one {scene, mask, texts} item (PIL RGB images): per line of split_lines, batch_driver.prepare_plain on
    the line's mask alone with the line's one text -- the region of that mask (paste_back.select_region), its crop resized as
    _paste_back_inputs does, a glyph strip at the region's width (glyph.render_single_line), prompt generate_prompt([text]), meta of
    mode singleline.  Work.parent = index, Work.line = the position in the list.  No line at all: ValueError.
    warp (the pipeline's warp_affine; with cfg["rectify"]): a slanted line is cut as an oriented rectangle and prepared upright
    (batch_driver._upright_inputs); its Work then carries `rect`.  warp_quad (the pipeline's warp_perspective; with
    cfg["perspective"]): a line seen in perspective is cut as a quad instead; `rect` is then its Quad.
    warp_grid (the pipeline's warp_grid; with cfg["curve"]): a line along a bend is cut as a ribbon, which
    is tried first; `rect` is then its Ribbon."""
    from PIL import Image
    from . import batch_driver as bd
    works = []
    for _, text, lm in split_lines(mask, texts):
        w = bd.prepare_plain(index, scene, Image.fromarray(lm), [text], device_compose, cfg, warp=warp, warp_quad=warp_quad, warp_grid=warp_grid)
        w.parent, w.line = index, len(works)
        works.append(w)
    if not works:
        raise ValueError("per_line: no mask region with a text line")
    return works


def prepare_lines(index: int, item: Dict[str, Any], loader: Optional[Callable], device_compose: bool, eval_cfg: Optional[Dict[str, Any]],
                  cfg: Dict[str, Any], warp: Optional[Callable] = None, warp_quad: Optional[Callable] = None,
                  warp_grid: Optional[Callable] = None) -> List[Any]:
    """One item of batch_driver.run_items -> its lines as Works.  {image, mask, text} items: prepare_scene_lines.  `annos.json` items:
    every entry of `annotations` with a text and a polygon is a line (batch_driver.prepare_eval_item of that entry).  warp,
    warp_quad, warp_grid: as in prepare_scene_lines."""
    from PIL import Image
    from . import batch_driver as bd
    if "img_name" in item:
        c = eval_cfg or {}
        font = c.get("font") or glyph.load_font(c.get("font_path"))
        works = []
        for k, ann in enumerate(item["annotations"]):
            if not (ann.get("text") and str(ann["text"]).strip() and ann.get("polygon")):
                continue
            w = bd.prepare_eval_item(index, item, c.get("original_images_dir", "."), font, c.get("text_height_ratio", 0.1667), loader,
                                     device_compose, cfg, annotation=k, warp=warp, warp_quad=warp_quad, warp_grid=warp_grid)
            w.parent, w.line = index, len(works)
            works.append(w)
        if not works:
            raise ValueError("per_line: no annotation with a text and a polygon")
        return works
    load = loader or (lambda p: Image.open(p))
    scene, mask = load(item["image"]).convert("RGB"), load(item["mask"]).convert("RGB")
    return prepare_scene_lines(index, scene, mask, glyph.read_words_from_text(item["text"]), cfg, device_compose, warp, warp_quad, warp_grid)


def compose_lines(pipe, lines: Sequence[Any], crops: Sequence[Any], cfg: Dict[str, Any]):
    """The item's scene (PIL image at its original size) with every line's cropped result pasted in, in split order: starting from a
    copy of the scene, line by line pipe.paste_back(the CURRENT pixels of the line's region, the line's result, the line's mask in that
    region) is written back into the copy.  With cfg["color_match"] the call also gets color_match and color_ref = the ORIGINAL pixels
    of the region: each edit was generated from the original scene, so that is what its ring shows (another line's old text inside the
    ring appears in both; what was pasted in since does not).  The two are passed only then.  With cfg["seamless"] the call gets
    seamless and, for the same reason, the same color_ref (the membrane's difference is taken against the original region); passed
    only then.  With cfg["grain"] the call gets grain, origin = the region's top-left scene pixel (the grain is anchored at scene
    positions) and the same color_ref (the scene's noise level is measured on the original region, not on grain an earlier line's paste
    added); passed only then.  With cfg["keyed"] the call gets keyed and the same color_ref (the noise level that the key's thresholds
    stay above is the original region's); passed only then.  The key itself compares the blend with the CURRENT pixels, so what an
    earlier line pasted is kept like any other scene content.
    A rectified, perspective or curved line (Work.rect: a Rect, a Quad or a Ribbon) is pasted into its window `region`, the bounding box
    of the oriented rectangle or of the upright crop's footprint cut at the image: the call
    also gets rect and origin = the window's top-left scene pixel, and the pipeline warps the upright result into the window before
    the blend (paste_back.paste).  These two are passed only for such lines: a pipeline that predates them serves all others."""
    import torch
    from PIL import Image
    from . import paste_back as pb
    out = lines[0].orig_scene.copy()
    for w, cropped in zip(lines, crops):
        reg = w.region
        cur = np.ascontiguousarray(out[reg.y0:reg.y1, reg.x0:reg.x1])
        om = pb.grey_of(w.orig_mask[reg.y0:reg.y1, reg.x0:reg.x1])
        kw = {}
        if cfg.get("color_match"):
            kw = dict(color_match=cfg["color_match"], color_ref=np.ascontiguousarray(w.orig_scene[reg.y0:reg.y1, reg.x0:reg.x1]))
        if cfg.get("seamless"):
            kw.update(seamless=cfg["seamless"], color_ref=np.ascontiguousarray(w.orig_scene[reg.y0:reg.y1, reg.x0:reg.x1]))
        if cfg.get("grain"):
            kw.update(grain=cfg["grain"], origin=(reg.x0, reg.y0), color_ref=np.ascontiguousarray(w.orig_scene[reg.y0:reg.y1, reg.x0:reg.x1]))
        if cfg.get("keyed"):
            kw.update(keyed=cfg["keyed"], color_ref=np.ascontiguousarray(w.orig_scene[reg.y0:reg.y1, reg.x0:reg.x1]))
        if w.rect is not None:
            kw.update(rect=w.rect, origin=(reg.x0, reg.y0))
        pasted = pipe.paste_back(cur, cropped, om, dilate=cfg["dilate"], feather=cfg["feather"], **kw)
        pasted = pasted.cpu().numpy() if isinstance(pasted, torch.Tensor) else np.asarray(pasted)
        out[reg.y0:reg.y1, reg.x0:reg.x1] = pasted.reshape(cur.shape)
    return Image.fromarray(out)


def line_name(name: str, line: int) -> str:
    """File name of line k's raw canvas under full_images/: <name> for line 0, <stem>_line<k><ext> after it."""
    if line == 0:
        return name
    stem, ext = os.path.splitext(name)
    return f"{stem}_line{line}{ext}"


def write_item(lines: Sequence[Any], fulls: Sequence[Any], pasted, out_dir: Optional[str], save: Optional[Callable],
               save_full: Optional[Callable]) -> None:
    """batch_driver.run_items' output rule for an item edited line by line: `pasted` is what is saved / written as <index>.png / under
    cropped_images/<name>; full_images/ gets every line's raw canvas (line_name); save_full gets line 0's Work and canvas."""
    w0 = lines[0]
    if w0.name is not None and (save_full is not None or (save is None and out_dir is not None)):
        if save_full is not None:
            save_full(w0, fulls[0], pasted)
        else:
            for w, full in zip(lines, fulls):
                full.save(os.path.join(out_dir, "full_images", line_name(w.name, w.line)))
            pasted.save(os.path.join(out_dir, "cropped_images", w0.name))
    elif save is not None:
        save(w0.index, pasted)
    elif out_dir is not None:
        pasted.save(os.path.join(out_dir, f"{w0.index:06d}.png"))


def edit_scene(pipe, scene, mask, texts: Sequence[str], cfg: Dict[str, Any], num_inference_steps: int = 30, guidance_scale: float = 30.0,
               seed: int = 42, device=None, max_sequence_length: int = 512, call_kw: Optional[Dict[str, Any]] = None):
    """One scene outside the batch driver (run_inference.py): -> (the scene with all lines pasted in, [every line's raw canvas]).
    Lines of equal editing size go through one pipeline call each; every line has the generator of a single-image call.  call_kw:
    further keyword arguments of every pipeline call (keep_known, strength, change_map)."""
    import torch
    from . import batch_driver as bd
    device = device if device is not None else getattr(pipe, "_execution_device", "cuda")
    lines = prepare_scene_lines(0, scene.convert("RGB"), mask.convert("RGB"), texts, cfg, **bd.pipeline_warps(pipe, cfg))
    fulls: Dict[int, Any] = {}
    for batch in bd.plan_batches(lines, len(lines)):
        n = len(batch.items)
        gens = [torch.Generator(device=device).manual_seed(int(seed)) for _ in range(n)]
        images = pipe(height=batch.size[1], width=batch.size[0], image=[w.image for w in batch.items],
                      mask_image=[w.mask for w in batch.items], num_inference_steps=num_inference_steps, generator=gens,
                      max_sequence_length=max_sequence_length, guidance_scale=guidance_scale, prompt=[glyph.PROMPT_TEMPLATE2] * n,
                      prompt_2=[w.prompt for w in batch.items], **(call_kw or {})).images
        for w, img in zip(batch.items, images):
            fulls[w.line] = img
    crops = [fulls[w.line].crop(glyph.crop_box(w.size, w.meta)) for w in lines]
    return compose_lines(pipe, lines, crops, cfg), [fulls[w.line] for w in lines]
