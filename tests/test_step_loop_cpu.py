"""The engine's step loop (textflux_amd/step_loop.py: run_steps) driven through its seam by a recorder: no GPU, no library.  Every
case asserts the exact sequence of device operations, callbacks and progress-bar updates."""
import warnings
from types import SimpleNamespace

import pytest

from textflux_amd.step_cache import Decider, StepCacheConfig, replay
from textflux_amd.step_loop import CaptureRefused, run_steps

KEY = (False, True)         # (is_amo, fuse) of the session's handle store


class Recorder:
    """The seam.  Handles are "g<phase>#<serial>"; `refuse`: the phase whose capture is refused; `metrics`: the head's values per step."""

    def __init__(self, refuse=None, metrics=None):
        self.ev, self.refuse, self.metrics, self.serial, self.heads = [], refuse, metrics, 0, 0

    def feed_noise(self, i):
        self.ev.append(("noise", i))

    def run(self, ph):
        self.ev.append(("run", ph))

    def replay(self, handle):
        self.ev.append(("replay", handle))

    def capture(self, ph):
        self.ev.append(("capture", ph))
        if ph == self.refuse:
            raise CaptureRefused("the runtime said no")
        self.serial += 1
        return f"g{ph}#{self.serial}"

    def destroy(self, handle):
        self.ev.append(("destroy", handle))

    def metric(self):
        self.ev.append(("metric",))
        self.heads += 1
        return self.metrics[self.heads - 1]

    def save(self):
        self.ev.append(("save",))
        return "state"

    def restore(self, saved):
        assert saved == "state"
        self.ev.append(("restore",))

    def update(self, n=1):          # the progress bar
        self.ev.append(("bar",))


def make_pipe():
    return SimpleNamespace(_interrupt=False, scheduler=SimpleNamespace(_step_index=0))


def drive(n, graphs, rec=None, pipe=None, **kw):
    rec, pipe = rec or Recorder(), pipe or make_pipe()
    pipe.scheduler._step_index = 0
    run_steps(rec, n, pipe, rec, graphs, KEY, **kw)
    return rec.ev, pipe


def step(i, *ops):
    return [("noise", i), *ops, ("bar",)]


def test_plain_eager():
    graphs = {}
    ev, pipe = drive(4, graphs)
    assert ev == sum((step(i, ("run", 0)) for i in range(4)), [])
    assert graphs == {} and pipe.scheduler._step_index == 4


def test_plain_with_graphs_captures_once_after_the_first_step_and_reuses_the_handle():
    graphs = {}
    ev, pipe = drive(4, graphs, use_graph=True)
    g = "g0#1"
    assert ev == step(0, ("run", 0), ("save",), ("capture", 0), ("restore",)) + sum((step(i, ("replay", g)) for i in (1, 2, 3)), [])
    assert graphs == {KEY: g} and pipe.scheduler._step_index == 4
    # the same session again: nothing is captured, and the first step is still the eager run
    ev, pipe = drive(4, graphs, use_graph=True)
    assert ev == step(0, ("run", 0)) + sum((step(i, ("replay", g)) for i in (1, 2, 3)), [])
    assert graphs == {KEY: g} and pipe.scheduler._step_index == 4


def test_one_step_is_never_captured():
    graphs = {}
    ev, _ = drive(1, graphs, use_graph=True)
    assert ev == step(0, ("run", 0)) and graphs == {}
    ev, _ = drive(1, graphs, Recorder(metrics=METRICS), decider=Decider(CFG), use_graph=True)
    assert ev == step(0, ("run", 1), ("metric",), ("run", 2)) and graphs == {}


def test_callback_keeps_the_loop_eager_and_runs_after_every_step():
    graphs, seen = {}, []
    rec = Recorder()
    ev, pipe = drive(3, graphs, rec, use_graph=True, callback=lambda i: (seen.append(i), rec.ev.append(("callback", i))))
    assert ev == sum((step(i, ("run", 0), ("callback", i)) for i in range(3)), [])
    assert seen == [0, 1, 2] and graphs == {} and not any(e[0] == "capture" for e in ev)


def test_refused_capture_warns_once_runs_eagerly_and_is_not_retried():
    graphs = {}
    with pytest.warns(UserWarning, match="capture of the denoising step failed .the runtime said no.; running the step loop eagerly") as w:
        ev, pipe = drive(4, graphs, Recorder(refuse=0), use_graph=True)
    assert len(w) == 1
    assert ev == step(0, ("run", 0), ("save",), ("capture", 0), ("restore",)) + sum((step(i, ("run", 0)) for i in (1, 2, 3)), [])
    assert graphs == {KEY: False} and pipe.scheduler._step_index == 4
    with warnings.catch_warnings():
        warnings.simplefilter("error")          # the cached False: no second attempt, no second warning
        ev, _ = drive(4, graphs, Recorder(refuse=0), use_graph=True)
    assert ev == sum((step(i, ("run", 0)) for i in range(4)), [])


INF = float("inf")
METRICS = [[INF, INF], [0.3, 0.01], [0.05, 0.02], [0.01, 0.01], [0.01, 0.01], [0.5, 0.01]]
CFG = StepCacheConfig.make(0.1, max_consecutive=2)
CACHE_KEYS = {ph: KEY + ("step_cache", ph) for ph in (1, 2, 3)}


def test_step_cache_phases_follow_the_decisions():
    skips = replay(CFG, METRICS)
    assert skips == [False, False, True, True, False, False]
    graphs, d = {}, Decider(CFG)
    ev, pipe = drive(6, graphs, Recorder(metrics=METRICS), decider=d)
    assert ev == sum((step(i, ("run", 1), ("metric",), ("run", 3 if skips[i] else 2)) for i in range(6)), [])
    assert [r["skipped"] for r in d.report] == skips and [r["metric"] for r in d.report] == METRICS
    assert graphs == {} and pipe.scheduler._step_index == 6


def test_step_cache_with_graphs_captures_three_phases_after_the_first_step():
    skips = replay(CFG, METRICS)
    graphs = {}
    ev, pipe = drive(6, graphs, Recorder(metrics=METRICS), decider=Decider(CFG), use_graph=True)
    h = {1: "g1#1", 2: "g2#2", 3: "g3#3"}
    first = step(0, ("run", 1), ("metric",), ("run", 2), ("save",), ("capture", 1), ("capture", 2), ("capture", 3), ("restore",))
    assert ev == first + sum((step(i, ("replay", h[1]), ("metric",), ("replay", h[3 if skips[i] else 2])) for i in range(1, 6)), [])
    assert graphs == {CACHE_KEYS[ph]: h[ph] for ph in (1, 2, 3)} and pipe.scheduler._step_index == 6
    # again: the handles are found after the first (eager) step, nothing is captured
    ev, _ = drive(6, graphs, Recorder(metrics=METRICS), decider=Decider(CFG), use_graph=True)
    assert ev == step(0, ("run", 1), ("metric",), ("run", 2)) + sum(
        (step(i, ("replay", h[1]), ("metric",), ("replay", h[3 if skips[i] else 2])) for i in range(1, 6)), [])
    # the plain loop's handle lives under its own key next to them
    drive(2, graphs, use_graph=True)
    assert set(graphs) == set(CACHE_KEYS.values()) | {KEY}


def test_step_cache_refusal_destroys_the_handles_already_made():
    graphs = {}
    with pytest.warns(UserWarning, match="running the step loop eagerly") as w:
        ev, _ = drive(3, graphs, Recorder(refuse=3, metrics=METRICS), decider=Decider(CFG), use_graph=True)
    assert len(w) == 1
    first = step(0, ("run", 1), ("metric",), ("run", 2), ("save",), ("capture", 1), ("capture", 2), ("capture", 3),
                 ("destroy", "g1#1"), ("destroy", "g2#2"), ("restore",))
    assert ev == first + step(1, ("run", 1), ("metric",), ("run", 2)) + step(2, ("run", 1), ("metric",), ("run", 3))
    assert graphs == {k: False for k in CACHE_KEYS.values()}


def test_noise_is_fed_before_every_step_replayed_ones_included():
    """feed_noise(i) is the loop's only per-step input: SessionSteps draws or copies the AMO noise there, outside any graph"""
    ev, _ = drive(5, {}, use_graph=True)
    assert [e for e in ev if e[0] in ("noise", "run", "replay")] == [
        ("noise", 0), ("run", 0), ("noise", 1), ("replay", "g0#1"), ("noise", 2), ("replay", "g0#1"), ("noise", 3), ("replay", "g0#1"),
        ("noise", 4), ("replay", "g0#1")]


def test_interrupt_from_the_callback_stops_issuing_and_the_bar():
    rec, pipe = Recorder(), make_pipe()

    def cb(i):
        rec.ev.append(("callback", i))
        if i == 1:
            pipe._interrupt = True

    ev, _ = drive(4, {}, rec, pipe, use_graph=True, callback=cb)
    assert ev == step(0, ("run", 0), ("callback", 0)) + step(1, ("run", 0), ("callback", 1))
    assert pipe.scheduler._step_index == 2


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("cached", [False, True])
def test_step_index_counts_every_step(use_graph, cached):
    n = 5
    kw = dict(decider=Decider(CFG)) if cached else {}
    _, pipe = drive(n, {}, Recorder(metrics=METRICS), use_graph=use_graph, **kw)
    assert pipe.scheduler._step_index == n
