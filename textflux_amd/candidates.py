"""Candidates (DESIGN.md section 4 "Candidates"): best of N seeds per work, chosen by on-device read-back.  The host side of it --
the option's parsing, the expansion of a work into its candidates, where a work's lines lie on its own pipeline canvas, the scoring of a
batch through TextRecognizer.read_device and the choice rule.  batch_driver.run_items drives it; nothing here launches anything but
`score_batch`, which makes the one read_device call of a batch.

No reference counterpart: the reference runs one seed per image.  No quality claim either: without a real checkpoint and real
recogniser weights only the mechanism is tested -- which candidate is kept follows exactly from the scores, and the kept candidate's
bytes are exactly those of a plain run with its seed.
"""
from __future__ import annotations

import dataclasses
import math
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

KEYS = ("n", "prune", "seeds")
PRUNE_KEYS = ("at", "keep")


def candidates_cfg(candidates, seed: int, num_inference_steps: Optional[int] = None, batch_size: Optional[int] = None):
    """run_items' candidates argument -> None (off: None, or n == 1) or dict(n, seeds: n ints, prune: None | dict(at, keep)).
    candidates: None | N | dict(n, prune=None | dict(at, keep=1), seeds=None).  seeds defaults to seed .. seed + n - 1.  With prune the
    candidates of a work share one batch: n <= batch_size; 0 < at < num_inference_steps and 1 <= keep <= n.  ValueError otherwise;
    nothing is loaded or launched here."""
    if candidates is None:
        return None
    if isinstance(candidates, bool):
        raise ValueError("candidates must be None, a count N or dict(n, prune, seeds)")
    if isinstance(candidates, int):
        candidates = dict(n=candidates)
    if not isinstance(candidates, dict):
        raise ValueError("candidates must be None, a count N or dict(n, prune, seeds)")
    unknown = set(candidates) - set(KEYS)
    if unknown:
        raise ValueError(f"candidates: unknown keys {sorted(unknown)}")
    n = candidates.get("n")
    if isinstance(n, bool) or not isinstance(n, int) or n < 1:
        raise ValueError(f"candidates: n must be an integer of at least 1, got {n!r}")
    seeds = candidates.get("seeds")
    if seeds is None:
        seeds = [int(seed) + k for k in range(n)]
    else:
        seeds = list(seeds)
        if len(seeds) != n or any(isinstance(s, bool) or not isinstance(s, int) for s in seeds) or len(set(seeds)) != n:
            raise ValueError(f"candidates: seeds must be {n} different integers, got {seeds!r}")
    prune = candidates.get("prune")
    if prune is not None:
        if not isinstance(prune, dict) or set(prune) - set(PRUNE_KEYS) or "at" not in prune:
            raise ValueError("candidates: prune must be None or dict(at, keep=1)")
        at, keep = prune["at"], prune.get("keep", 1)
        if any(isinstance(v, bool) or not isinstance(v, int) for v in (at, keep)):
            raise ValueError("candidates: prune's at and keep must be integers")
        if at < 1 or (num_inference_steps is not None and at >= num_inference_steps):
            raise ValueError(f"candidates: prune at={at} must lie inside the schedule, 0 < at < {num_inference_steps}")
        if not 1 <= keep <= n:
            raise ValueError(f"candidates: prune keep={keep} must be in 1..n = {n}")
        if batch_size is not None and n > batch_size:
            raise ValueError(f"candidates: with prune the {n} candidates of a work share one batch, batch_size is {batch_size}")
        prune = dict(at=at, keep=keep)
    if n == 1:
        if seeds != [int(seed)]:
            raise ValueError("candidates: n == 1 is the run without the key; give the seed as `seed`")
        return None
    return dict(n=n, seeds=seeds, prune=prune)


def expand(works: Sequence[Any], cfg: Dict[str, Any]) -> List[Any]:
    """Every Work -> its n candidates, adjacent and in seed order: copies that differ in `seed` and `cand` (the position k)."""
    return [dataclasses.replace(w, seed=s, cand=k) for w in works for k, s in enumerate(cfg["seeds"])]


def group_key(w) -> Tuple[int, int]:
    """What the candidates of one work share: (item index, line position; 0 for a work that is its whole item)."""
    return w.index, (w.line or 0)


# ---- the choice ---------------------------------------------------------------------------------------------------------------------
def choice_key(records: Sequence[Dict[str, Any]], k: int) -> Tuple[int, float, int]:
    """(number of lines not read exactly, sum of ctc_loss, k) of one candidate's line records; a loss that is missing or not finite
    counts as +inf, so does their sum."""
    loss = 0.0
    for r in records:
        v = r.get("ctc_loss")
        loss += float(v) if v is not None and math.isfinite(float(v)) else math.inf
    return sum(1 for r in records if r["seq_acc"] != 1.0), loss, k


def choose(scored: Sequence[Sequence[Dict[str, Any]]], keep: int = 1) -> List[int]:
    """The positions of the `keep` best candidates, best first: scored[k] = candidate k's line records; the smallest choice_key wins,
    ties go to the lowest k."""
    order = sorted(range(len(scored)), key=lambda k: choice_key(scored[k], k))
    return order[:keep]


# ---- where a work's lines are, and what reads them ------------------------------------------------------------------------------------
def work_lines(w, mask_grey: np.ndarray) -> List[Tuple[str, np.ndarray]]:
    """[(text, line mask uint8 [H, W])] of a work on its own pipeline canvas.  mask_grey: the work's pipeline mask (black over the
    glyph part).  A strip edit (one text) is one region, the whole mask; the multi-line canvas is split as per_line.split_lines pairs
    regions and texts.  ValueError when there is nothing to read."""
    from . import per_line
    texts = list(w.texts or [])
    if len(texts) == 1 and texts[0].strip():
        lines = [(texts[0].strip(), np.where(mask_grey > 127, 255, 0).astype(np.uint8))]
    else:
        lines = [(text, lm) for _, text, lm in per_line.split_lines(np.ascontiguousarray(mask_grey), texts)]
    lines = [(t, lm) for t, lm in lines if (lm > 127).any()]
    if not lines:
        raise ValueError(f"candidates: item {w.index} has no mask region with a text to read")
    return lines


def score_batch(reader, images_u8, works: Sequence[Any], masks: Sequence[np.ndarray], stage: str,
                cache: Optional[Dict[Any, Any]] = None) -> List[List[Dict[str, Any]]]:
    """One read_device call for all works of a batch: images_u8 device uint8 [B, H, W, 3] at pipeline size, works[j] is sample j and
    masks[j] its pipeline mask (grey, host).  -> per work its line records {seed, line, text, pred, seq_acc, ned, ctc_loss, stage}.
    cache: group_key -> the work's lines; the candidates of a work share a geometry, which is located once."""
    from . import ocr as rb
    lines, owner = [], []
    for j, (w, m) in enumerate(zip(works, masks)):
        key = group_key(w)
        if cache is None or key not in cache:
            got = work_lines(w, m)
            if cache is not None:
                cache[key] = got
        else:
            got = cache[key]
        for text, lm in got:
            lines.append((j, lm))
            owner.append((j, text))
    recs = reader.read_device(images_u8, lines, [t for _, t in owner])
    out: List[List[Dict[str, Any]]] = [[] for _ in works]
    for (j, text), r in zip(owner, recs):
        gt = reader.text_ids(text)
        out[j].append(dict(seed=works[j].seed, line=len(out[j]), text=text, pred=r["text"], seq_acc=1.0 if r["ids"] == gt else 0.0,
                           ned=rb.get_ld(r["ids"], gt), ctc_loss=r["ctc_loss"], stage=stage))
    return out


def pruned_steps(n: int, steps: int, at: int, keep: int) -> float:
    """Share of the unpruned candidates' steps that a pruned run issues: (n at + keep (steps - at)) / (n steps)."""
    return (n * at + keep * (steps - at)) / float(n * steps)
