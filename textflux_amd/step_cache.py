"""Host side of the first-block step cache ("Step cache"): the settings and the per-step decision.

No reference counterpart: the reference computes every block on every step (pipeline_flux_fill.py:2077-2116).  Per step the
engine runs the head (embedders + block 0) and measures how far the first block's residual moved since the last fully computed
step, per sample: metric[b] = sum |f - f_prev| / sum |f_prev|  (tfx_step_cache_metric).  The functions here turn those B numbers
into "run blocks 1 ... n" or "re-use the last computed step's residual".  Pure Python: importable and testable without a GPU.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import FrozenSet, Iterable, List, Optional, Sequence


@dataclass(frozen=True)
class StepCacheConfig:
    """threshold: a step is skipped when the LARGEST metric of the batch is below it (0 never skips, inf always does).  There is
    no default: a useful value is a property of the checkpoint -- run once with threshold=0 and read pipe.step_cache_report.
    skip_steps: an explicit schedule; a step listed here is skipped whatever its metric (and max_consecutive does not apply).
    max_consecutive: at most this many threshold skips in a row, then a computed step refreshes the residual (None = no cap).
    force_compute: steps that are always computed.  Step 0 always is."""
    threshold: float
    skip_steps: FrozenSet[int] = frozenset()
    max_consecutive: Optional[int] = None
    force_compute: FrozenSet[int] = frozenset()

    @staticmethod
    def make(threshold, skip_steps: Optional[Iterable[int]] = None, max_consecutive: Optional[int] = None,
             force_compute: Optional[Iterable[int]] = None) -> "StepCacheConfig":
        if threshold is None:
            raise ValueError("the step cache has no default threshold: it is a property of the checkpoint (run with threshold=0 "
                             "and read step_cache_report to choose one)")
        threshold = float(threshold)
        if math.isnan(threshold) or threshold < 0:
            raise ValueError(f"step cache threshold must be >= 0, got {threshold}")
        if max_consecutive is not None and int(max_consecutive) < 1:
            raise ValueError("max_consecutive must be >= 1 (or None)")
        return StepCacheConfig(threshold, frozenset(int(s) for s in (skip_steps or ())),
                               None if max_consecutive is None else int(max_consecutive),
                               frozenset(int(s) for s in (force_compute or ())))


def decide(cfg: StepCacheConfig, step: int, metric: Sequence[float], have_computed: bool, consecutive: int) -> bool:
    """True = skip blocks 1 ... n of step `step` (0-based).  metric: the head's per-sample values; have_computed: a computed
    step exists in this call (its residual is in the cache); consecutive: skipped steps directly in front of this one.  The
    maximum over the samples decides, so no sample is skipped beyond its own threshold; +inf (a zero reference residual) and NaN
    never pass the threshold."""
    if step < 1 or not have_computed or step in cfg.force_compute:
        return False
    if step in cfg.skip_steps:
        return True
    if cfg.max_consecutive is not None and consecutive >= cfg.max_consecutive:
        return False
    worst = max((float("inf") if math.isnan(float(m)) else float(m)) for m in metric)
    return worst < cfg.threshold


class Decider:
    """decide() with the loop's running state: call step(i, metric) once per step, in order."""

    def __init__(self, cfg: StepCacheConfig):
        self.cfg, self.have_computed, self.consecutive = cfg, False, 0
        self.report: List[dict] = []

    def step(self, i: int, metric: Sequence[float]) -> bool:
        skip = decide(self.cfg, i, metric, self.have_computed, self.consecutive)
        self.consecutive = self.consecutive + 1 if skip else 0
        self.have_computed = self.have_computed or not skip
        self.report.append(dict(metric=[float(m) for m in metric], skipped=bool(skip)))
        return skip


def replay(cfg: StepCacheConfig, metrics: Sequence[Sequence[float]]) -> List[bool]:
    """The skipped flags a loop over `metrics` (one row per step) produces."""
    d = Decider(cfg)
    return [d.step(i, m) for i, m in enumerate(metrics)]
