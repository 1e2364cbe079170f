"""The engine's denoising loop, once: n steps of tfx_dit_step_run_ex3 -- or of the replay of the graph captured
from it -- for the plain loop (phase 0) and the step cache (phases 1, 2 / 3), the Euler, AMO, fused-Euler and multistep samplers (the
last by the history buffer in the step's tfx_step_extra), with or without a step callback, on uniform and mixed-geometry sessions; with
the known-region blend behind every sampler update (the tfx_step_extra's keep_* buffers) when the call keeps the known region, or the
change-map blend (a tfx_step_change beside it) when the call gives every latent pixel its own release step; with true CFG (a
tfx_step_cfg beside those) when the call carries a negative prompt: the session is then twice the loop state's batch.  Without a
tfx_step_cfg the _ex3 pair is exactly tfx_dit_step_run_ex2 / tfx_dit_step_capture_ex2.

`run_steps` is the control flow and touches no device: it drives a `steps` object with
    feed_noise(i)   run(phase)   replay(handle)   capture(phase) -> handle (raises CaptureRefused)   destroy(handle)
    metric() -> the head's B floats   save() -> state   restore(state)
`SessionSteps` binds those to a DitSession and the library; tests/test_step_loop_cpu.py binds them to a recorder.  `denoise` is
what the pipeline calls: buffers, side stream, run_steps, result.
"""
from __future__ import annotations

import ctypes as C
import warnings

import torch

from . import _lib as L
from . import ops
from .step_cache import Decider

BF16 = torch.bfloat16


class CaptureRefused(RuntimeError):
    """tfx_dit_step_capture returned an error (driver / runtime state); the message is the library's."""


def check_step_window(window, n=None):
    """(a, b) of a step_window as integers; ValueError unless 0 <= a < b (<= n when the schedule's length n is known)."""
    try:
        a, b = window
        ok = int(a) == a and int(b) == b and 0 <= a < b and (n is None or b <= n)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"step_window must be (a, b) with 0 <= a < b <= {'n' if n is None else n}, got {window!r}")
    return int(a), int(b)


def refuse_step_window(scheduler, strength=1.0, keep_known=None, change_map=None, true_cfg=False, step_cache=False, callback=False,
                       mixed=False):
    """NotImplementedError with the reason when a call with step_window (DESIGN.md section 4 "Candidates") cannot be served: a window
    carries the latents and nothing else from one call to the next, and every sampler state, blend buffer or decision beyond them would
    have to travel with it.  Touches no device: the pipeline and the batch driver both ask in front of everything else."""
    from .schedulers import FlowMatchEulerDiscreteScheduler, FlowMatchMultistepScheduler, StochasticRFOvershotDiscreteScheduler
    why = None
    if isinstance(scheduler, StochasticRFOvershotDiscreteScheduler):
        why = "the AMO sampler (its noise draws belong to the whole schedule)"
    elif isinstance(scheduler, FlowMatchMultistepScheduler):
        why = "the multistep sampler (its history, the previous model output, would have to travel with the latents)"
    elif not isinstance(scheduler, FlowMatchEulerDiscreteScheduler):
        why = f"a scheduler other than FlowMatchEulerDiscreteScheduler ({type(scheduler).__name__})"
    elif strength != 1.0:
        why = "strength (the window already names the steps that run)"
    elif keep_known:
        why = "keep_known (the blend's noise and original latents would have to travel with the latents)"
    elif change_map is not None and change_map is not False:
        why = "change_map (the blend's noise, original latents and hold bytes would have to travel with the latents)"
    elif true_cfg:
        why = "true CFG (negative_prompt / true_cfg > 1)"
    elif step_cache:
        why = "the step cache (its cached residual and decisions belong to one uninterrupted loop)"
    elif callback:
        why = "a step callback"
    elif mixed:
        why = "mixed-geometry batches (call_mixed / mixed_pad > 0)"
    if why is not None:
        raise NotImplementedError(f"step_window does not run with {why}")


def _graph_handles(steps, graphs, keys):
    """{phase: handle} for the phases of `keys`, captured now if the session holds none yet; False = eager (a refusal, now or cached).
    Capture does not execute, the state is kept explicit around it anyway."""
    have = {ph: graphs.get(k) for ph, k in keys.items()}
    if all(g is None for g in have.values()):
        saved = steps.save()
        try:
            for ph in keys:
                have[ph] = steps.capture(ph)
        except CaptureRefused as e:      # same kernels, launched eagerly
            warnings.warn(f"hipGraph capture of the denoising step failed ({e}); running the step loop eagerly")
            for g in have.values():
                if g:
                    steps.destroy(g)
            have = dict.fromkeys(have, False)
        steps.restore(saved)
        for ph, k in keys.items():
            graphs[k] = have[ph]
    return have if all(have.values()) else False


def run_steps(steps, n, pipe, progress_bar, graphs, key, decider=None, use_graph=False, callback=None):
    """n steps.  pipe: `_interrupt` is read and `scheduler._step_index` counted; graphs: the session's handle store, under `key` for
    the plain loop and key + ("step_cache", phase) for the cache; decider: the step cache's Decider (None: plain loop); callback(i):
    after step i.  use_graph, and then only without a callback and for n > 1: capture once the first step has run eagerly (a graph
    may only hold kernels that were launched before) and replay from then on."""
    use_graph = use_graph and callback is None and n > 1
    keys = {0: key} if decider is None else {ph: key + ("step_cache", ph) for ph in (1, 2, 3)}
    handles = None           # {phase: handle} once captured or found; False: eager phases

    def issue(ph):
        if handles:
            steps.replay(handles[ph])
        else:
            steps.run(ph)

    for i in range(n):
        if pipe._interrupt:
            continue
        steps.feed_noise(i)
        if decider is None:
            issue(0)
        else:
            issue(1)
            issue(3 if decider.step(i, steps.metric()) else 2)
        pipe.scheduler._step_index += 1
        if use_graph and handles is None:
            handles = _graph_handles(steps, graphs, keys)
        if callback is not None:
            callback(i)
        progress_bar.update()


class SessionSteps:
    """run_steps' device operations on a DitSession: its persistent step buffers `gb`, one tfx_step_desc per phase, stream `side`."""

    def __init__(self, ses, gb, side, phases, is_amo, fuse, amo_noise, multistep=False, keep=False, change=False, cfg=False):
        self.ses, self.gb, self.side, self.st, self.lib = ses, gb, side, side.cuda_stream, L.lib()
        self.sd = {ph: ses.step_desc(gb, is_amo, fuse, phase=ph) for ph in phases}
        self.is_amo, self.amo_noise = is_amo, amo_noise
        # One entry point serves every loop: an all-NULL tfx_step_extra is the plain step, v_prev alone the multistep sampler
        # (sampler 0's descriptor, the session's history buffer), keep_* all set the known-region blend; with a tfx_step_change
        # (hold bytes, cut table) keep_mask stays NULL and the blend is the change-map's.
        ptr = lambda name: gb[name].data_ptr()
        self.v_prev = ptr("v_prev") if multistep else None
        self.extra = L.StepExtra(v_prev=self.v_prev)
        self.change = None
        if keep or change:
            self.extra.keep_x0, self.extra.keep_noise, self.extra.keep_sigma = ptr("known_x0"), ptr("known_noise"), ptr("known_sigma")
        if keep:
            self.extra.keep_mask = ptr("known_mask")
        if change:
            self.change = L.StepChange(hold=ptr("known_hold"), cut=ptr("known_cut"))
        # true CFG: the scale's address (the value is rewritten every call); the per-sample buffers are then the first half of gb's
        self.cfg = L.StepCfg(scale=ptr("cfg_scale")) if cfg else None
        self.noise = gb["noise"][:ses.B // 2] if cfg else gb["noise"]
        self.args = {ph: (C.byref(sd), C.byref(self.extra), C.byref(self.change) if change else None, C.byref(self.cfg) if cfg else None)
                     for ph, sd in self.sd.items()}
        # what a failing step is reported as: the entry point of the C ABI that stands for this loop
        self.what = "dit_step_run" + ("_ex3" if cfg else "_ex2" if change else "_ex" if keep else "_multistep" if multistep else "")

    def feed_noise(self, i):
        if not self.is_amo:
            return
        if self.amo_noise is None:
            self.noise.normal_()            # global device RNG, as the reference's randn_tensor(generator=None); never captured
        else:
            self.noise.copy_(self.amo_noise[i].to(self.noise.device, torch.float32))

    def run(self, ph):
        L.check(self.lib.tfx_dit_step_run_ex3(*self.args[ph], self.st), self.what)

    def replay(self, handle):
        L.check(self.lib.tfx_dit_step_replay(handle, self.st), "dit_step_replay")

    def capture(self, ph):
        h = C.c_void_p()
        if self.lib.tfx_dit_step_capture_ex3(*self.args[ph], self.st, C.byref(h)) != 0:
            raise CaptureRefused(self.lib.tfx_last_error().decode())
        return h.value

    def destroy(self, handle):
        self.lib.tfx_graph_destroy(handle)

    def metric(self):
        c = self.ses.cache
        c["metric_host"].copy_(c["metric"], non_blocking=True)
        self.side.synchronize()
        return c["metric_host"].tolist()

    def save(self):
        self.side.synchronize()
        return [t.clone() for t in self._state()]

    def restore(self, saved):
        for t, s in zip(self._state(), saved):
            t.copy_(s)

    def _state(self):
        state = (self.gb["lat"], self.gb["step"], self.ses.xin)      # (xin also holds the latents when fused)
        return state + (self.gb["v_prev"],) if self.v_prev is not None else state


def denoise(pipe, ses, mod, latents, coef, n, progress_bar, is_amo=False, fuse=False, amo_noise=None, on_step=None, multistep=False,
            preview=None, cfg=None, keep=None, change=None):
    """The n steps of one engine call on session `ses`, whose xin holds [latents | masked_image_latents] and whose conditioning is
    set.  mod [n, B, mod_len (+ EULER_PAD when fuse)]: the modulation table.  latents [B, S, C] and coef, the sampler's coefficient
    table, may be None when fuse: the fused step reads the latents from xin and its coefficients from `mod`.  on_step(i, lat): the
    step callback, handed the live latent buffer after step i (it may write to it and to ses.xin).  multistep: the second-order
    multistep sampler -- unfused, coef its [n, 2] table, the history buffer gb["v_prev"] owned by the session; a callback that
    replaces the latents leaves the history (the previous model output) as it is.  keep: known-region sampling --
    dict(x0, noise, mask: bf16 [B, S, C]; sigma: fp32 [n], the scheduler's keep_sigma_table): after every sampler update the latents
    become (1 - mask) scale_noise(x0, sigma_{i+1}, noise) + mask latents (tfx_known_region_blend inside the step).  change:
    change-map sampling -- dict(x0, noise: bf16 [B, S, C]; hold: uint8 [B, S, 4]; sigma: fp32 [n]; cut: int32 [n],
    schedulers.change_cut_table): the same blend with the mask decided inside the step, held where hold > cut[step]
    (tfx_change_map_blend); not together with keep.  Either one's buffers live in the session next to v_prev, because captured graphs
    bake their addresses.  cfg: true CFG -- the scale g of noise_pred = neg + g (pos - neg); `ses` is then a session
    of 2B samples whose conditioning and modulation rows are [negative; positive] and whose xin holds the same rows in both halves, while
    latents, amo_noise, keep and change have B samples (they live in the first half of the session's buffers: the addresses are the
    same ones, whatever the call).  The scale lives in the session too and is rewritten every call: a captured graph serves every g.
    Unfused samplers only, not with the step cache, not on mixed sessions.  preview: dict(sigma: fp32 [..] on the device, step) of a
    window that ends early (DESIGN.md section 4 "Candidates") -- behind the last step, pipe.x0_preview becomes tfx_x0_predict of the
    final latents, that step's model output (ses.out: unfused samplers only) and sigma[step]; the launch is outside the step graph.
    Runs on the session's side stream (capture needs a non-NULL stream), fenced against the caller's current stream on both sides.  The step cache is on when
    pipe.enable_step_cache() is in force; graphs when pipe.enable_hip_graph(True), no callback and n > 1.  Returns the final
    latents and leaves pipe.step_cache_report set."""
    dev = ses.xin.device
    shape = (ses.B, ses.S, ses.model.out_channels)
    gb = ses.graph_buffers(n, 0 if coef is None else coef.numel(), shape)
    state = lambda t: t                     # the loop state's samples of a per-sample session buffer
    if cfg is not None:
        if fuse or ses.mixed or ses.B % 2:
            raise ValueError("true CFG needs an unfused sampler and a uniform session of 2B samples")
        if pipe._step_cache is not None:
            raise NotImplementedError("true CFG does not run with the step cache: the cache's metric would mix the two conditionings")
        state = lambda t: t[:ses.B // 2]
        if "cfg_scale" not in gb:           # lives and dies with gb: captured graphs bake its address
            gb["cfg_scale"] = torch.ones(1, dtype=torch.float32, device=dev)
    gb["mod_table"][:n, :, :mod.shape[2]].copy_(mod)
    if coef is not None:
        gb["coef"][:coef.numel()].copy_(coef.reshape(-1))
    if latents is not None:
        state(gb["lat"]).copy_(latents)
    gb["step"].zero_()
    if multistep:
        assert not is_amo and not fuse and latents is not None
        if "v_prev" not in gb:           # lives and dies with gb: captured graphs bake its address; step 0 never reads it
            gb["v_prev"] = torch.empty_like(gb["lat"])
    known = keep if keep is not None else change
    if known is not None:
        if ses.mixed:
            raise NotImplementedError(("known-region sampling" if keep is not None else "change_map (change-map sampling)")
                                      + " does not serve mixed-geometry sessions")
        if keep is not None and change is not None:
            raise ValueError("change_map and keep_known exclude each other")
        # one buffer family for both blends, living and dying with gb like v_prev: x0, noise and sigma, and the mask or the hold
        # bytes and the cut table
        for k in ("x0", "noise", "mask" if keep is not None else "hold"):             # per token
            if "known_" + k not in gb:
                gb["known_" + k] = torch.empty(*shape[:2], 4, dtype=torch.uint8, device=dev) if k == "hold" else torch.empty_like(gb["lat"])
            state(gb["known_" + k]).copy_(known[k])
        per_step = {"sigma": torch.float32} if keep is not None else {"sigma": torch.float32, "cut": torch.int32}
        for k, dtype in per_step.items():                                             # as long as the session's longest schedule
            assert known[k].numel() == n and known[k].dtype == dtype
            if "known_" + k not in gb:
                gb["known_" + k] = torch.zeros(gb["mod_table"].shape[0], dtype=dtype, device=dev)
            gb["known_" + k][:n].copy_(known[k])
    decider = None
    if pipe._step_cache is not None:
        ses.step_cache_reset()
        decider = Decider(pipe._step_cache)
    cur = torch.cuda.current_stream(dev)
    side = ses.graph_stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        if cfg is not None:
            gb["cfg_scale"].fill_(float(cfg))
        steps = SessionSteps(ses, gb, side, (0,) if decider is None else (1, 2, 3), is_amo, fuse, amo_noise, multistep, keep is not None,
                             change is not None, cfg is not None)
        ses._mod_keepalive = gb["mod_cur"]
        key = ("multistep", False) if multistep else (is_amo, fuse)
        if keep is not None:
            key += ("keep",)
        if change is not None:
            key += ("change",)
        if cfg is not None:
            key += ("cfg",)
        run_steps(steps, n, pipe, progress_bar, ses.graphs, key, decider, use_graph=pipe._use_hip_graph,
                  callback=None if on_step is None else lambda i: on_step(i, state(gb["lat"])))
        out = ops.copy_rows_(ses.xin[:, :, :shape[2]], torch.empty(shape, dtype=BF16, device=dev)) if fuse else state(gb["lat"]).clone()
        if preview is not None:
            if fuse or cfg is not None or pipe._interrupt:
                raise ValueError("the clean-image estimate needs the model output of the last step: an unfused, uninterrupted loop without true CFG")
            pipe.x0_preview = ops.x0_predict(out, ses.out, preview["sigma"], step=int(preview["step"]))
            pipe.x0_preview.record_stream(cur)
    out.record_stream(cur)
    cur.wait_stream(side)
    pipe.step_cache_report = decider.report if decider is not None else None
    return out
