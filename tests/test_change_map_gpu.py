"""Change-map sampling on the GPU (DESIGN.md section 4 "Change-map sampling"): tfx_change_map_blend and tfx_change_map_pack against the
restatement of helpers/change_map_ref.py (itself pinned to the reference by tests/test_change_map_cpu.py), bit for bit;
tfx_dit_step_run_ex2 inside the pipeline against the same loop issued from Python, for every sampler, eager and captured, with and
without `strength`, both `last` forms, an explicit and a derived map; and the pipeline's invariants.  Tiny model of
tests/helpers/tiny_checkpoint.py, B = 2, 128 x 96 pixels (48 tokens), 4 steps.  Every comparison is exact."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.helpers import change_map_ref as R
from tests.helpers import exact_inputs as X
from tests.helpers import paste_back_ref as PB
from tests.test_keep_known_gpu import B, GRID, H, N_STEPS, S, W, call, inputs, make_pipe

BF = torch.bfloat16


def bits(t):
    return t.contiguous().view(torch.int16)


def same(a, b):
    return torch.equal(bits(a.cpu()), bits(b.cpu()))


# ----------------------------------------------------------------------------- tfx_change_map_blend alone
CUTS = (-1, 0, 127, 254, 255)
SIGMAS = (0.90625, -1.0)                                                     # bf16-exact; the negative entry: "x0 itself"
# one table row per (cut, sigma) pair: row 2 ci + si
CUT_TABLE = torch.tensor([c for c in CUTS for _ in SIGMAS], dtype=torch.int32)
SIGMA_TABLE = torch.tensor([s for _ in CUTS for s in SIGMAS], dtype=torch.float32)


def blend_inputs(rows, C, seed):
    x, x0, noise = (X.arbitrary_bf16((rows, C), seed + k) for k in range(3))
    hold = torch.randint(0, 256, (rows, 4), generator=X.gen(seed + 3)).to(torch.uint8)
    hold[0] = torch.tensor([0, 255, 127, 128], dtype=torch.uint8)           # each cut of CUTS splits these four differently
    if rows > 1:
        hold[1] = torch.tensor([254, 255, 0, 1], dtype=torch.uint8)
    # signed zeros in row 0, columns 0..7 (columns j and j + 4 share a hold byte): both signs of x and of x0 under either decision
    for t, pattern in ((x, (0.0, -0.0, 0.0, -0.0, -0.0, 0.0, -0.0, 0.0)), (x0, (0.0, 0.0, -0.0, -0.0, -0.0, -0.0, 0.0, 0.0)),
                       (noise, (-0.0, 0.0, -0.0, 0.0, 0.0, -0.0, 0.0, -0.0))):
        t.view(-1)[:8] = torch.tensor(pattern, dtype=BF)
    return x, x0, noise, hold


@pytest.mark.parametrize("ldx", ["C", 384])
@pytest.mark.parametrize("C", [8, 64])
@pytest.mark.parametrize("rows", [1, 3, 33, 257])
def test_blend_equals_the_restatement(rows, C, ldx):
    """rows x C / 8 chunks: 1 .. 2056, below, across and not a multiple of a 256-thread block.  Per case: every cut x sigma, with the
    mirror and without, the step from the device cursor and as immediate."""
    from textflux_amd import ops
    ldx = C if ldx == "C" else ldx
    x, x0, noise, hold = blend_inputs(rows, C, 13 * rows + C)
    assert rows * C // 8 in (1, 3, 8, 24, 33, 257, 264, 2056)
    wants = [R.blend(x, x0, noise, hold, int(CUT_TABLE[t]), float(SIGMA_TABLE[t])) for t in range(len(CUT_TABLE))]
    assert sum(not same(w, x) for w in wants) == 8 and all(same(wants[t], x) for t in (8, 9))       # cut 255 leaves x, the others do not
    assert not same(wants[0], wants[1])
    x0d, nd, hd, sig, cut = x0.cuda(), noise.cuda(), hold.cuda(), SIGMA_TABLE.cuda(), CUT_TABLE.cuda()
    cursor = torch.zeros(1, dtype=torch.int32, device="cuda")
    pad_src, xin_src = X.arbitrary_bf16((rows, ldx), 77).cuda(), X.arbitrary_bf16((rows, C + 16), 78).cuda()
    for t in range(len(CUT_TABLE)):
        for mirror in (False, True):
            for device_step in (False, True):
                pad = pad_src.clone()
                pad[:, :C] = x.cuda()
                xd = pad[:, :C]                                              # a column view when ldx > C, the tensor itself otherwise
                pad0 = pad.clone()
                xin = xin_src.clone() if mirror else None
                cursor.fill_(t)
                got = ops.change_map_blend(xd, x0d, nd, hd, cut, sig, step=(len(CUT_TABLE) - 1 - t) if device_step else t,
                                           step_ptr=cursor if device_step else None, xin=xin)
                assert got is xd
                where = (int(CUT_TABLE[t]), float(SIGMA_TABLE[t]), mirror, device_step)
                assert same(pad[:, :C], wants[t]), where
                assert same(pad[:, C:], pad0[:, C:]), where
                if int(CUT_TABLE[t]) == 255:
                    assert same(pad, pad0), where                            # the bytes of x are untouched ...
                if mirror:                                                   # ... and the mirror is written either way
                    assert same(xin[:, :C], wants[t]) and same(xin[:, C:], xin_src[:, C:]), where


def test_blend_keeps_a_negative_zero_only_where_it_does_not_write():
    """e + d turns a free -0 into +0 (the reference's arithmetic); at cut 255 the kernel does not write, as the reference's last step"""
    x, x0, noise, hold = blend_inputs(3, 8, 5)
    free = R.blend(x, x0, noise, hold, 254, 0.90625)                         # column 1 held, the rest free
    assert bits(x)[0, 3] == -32768 and bits(free)[0, 3] == 0 and bits(R.blend(x, x0, noise, hold, 255, 0.90625))[0, 3] == -32768


@pytest.mark.parametrize("ldx", ["C", 384])
@pytest.mark.parametrize("C", [8, 64])
@pytest.mark.parametrize("rows", [1, 33, 257])
def test_a_binary_hold_is_the_known_region_blend_on_the_device(rows, C, ldx):
    """The two blends are one kernel frame with two mask sources: hold bytes of {0, 255} under any cut of 0..254 hold exactly the
    255s, and tfx_change_map_blend then equals tfx_known_region_blend with mask = 1 - k in every bit of x and of the mirror, for a
    positive sigma and a negative one (p = x0).  cut >= 255 is no part of this: there the change-map blend does not write."""
    from textflux_amd import ops
    ldx = C if ldx == "C" else ldx
    x, x0, noise = (X.arbitrary_bf16((rows, C), 29 * rows + C + k) for k in range(3))
    # the first chunk (all there is at rows 1, C 8) holds both zeros and both signs in every operand, under either decision
    for t, pattern in ((x, (0.0, -0.0, 1.5, -2.25, -0.0, 0.0, -3.0, 0.75)), (x0, (0.0, -0.0, -0.0, 0.0, 2.5, -1.25, 0.5, -4.0)),
                       (noise, (-0.0, 0.0, 1.0, -1.0, 0.0, -0.0, -0.5, 2.0))):
        t.view(-1)[:8] = torch.tensor(pattern, dtype=BF)
        assert (bits(t)[0, :8] == 0).any() and (bits(t)[0, :8] == -32768).any() and (t[0, :8] > 0).any() and (t[0, :8] < 0).any()
    hold = (torch.randint(0, 2, (rows, 4), generator=X.gen(rows + C)) * 255).to(torch.uint8)
    hold[0] = torch.tensor([0, 255, 255, 0], dtype=torch.uint8)
    k = (hold == 255).repeat(1, C // 4)                                     # column j reads byte j & 3
    mask = (1 - k.float()).to(BF).cuda()
    x0d, nd, hd = x0.cuda(), noise.cuda(), hold.cuda()
    pad_src, xin_src = X.arbitrary_bf16((rows, ldx), 79).cuda(), X.arbitrary_bf16((rows, C + 16), 80).cuda()
    for cut in (0, 127, 254):
        for sigma in SIGMAS:
            sig, ct = torch.tensor([sigma], dtype=torch.float32, device="cuda"), torch.tensor([cut], dtype=torch.int32, device="cuda")
            got = []
            for blend in (lambda xd, xin: ops.change_map_blend(xd, x0d, nd, hd, ct, sig, xin=xin),
                          lambda xd, xin: ops.known_region_blend(xd, x0d, nd, mask, sig, xin=xin)):
                pad, xin = pad_src.clone(), xin_src.clone()
                pad[:, :C] = x.cuda()
                blend(pad[:, :C], xin)
                got.append((pad, xin))
            (pc, ic), (pk, ik) = got
            assert same(pc, pk) and same(ic, ik), (cut, sigma)
            assert same(ic[:, :C], pc[:, :C]) and not same(pc[:, :C], x), (cut, sigma)


def test_blend_refusals():
    from textflux_amd import ops
    x, x0, noise, hold = (t.cuda() for t in blend_inputs(16, 64, 5))
    sig, cut = SIGMA_TABLE.cuda(), CUT_TABLE.cuda()
    keep = x.clone()
    ok = dict(x=x, x0=x0, noise=noise, hold=hold, cut=cut, keep_sigma=sig)
    for bad in (dict(x0=x), dict(noise=x)):
        with pytest.raises(RuntimeError, match="alias"):
            ops.change_map_blend(**dict(ok, **bad))
    big = torch.zeros(16 * 64 * 2 + 64, dtype=torch.uint8, device="cuda")
    xv = big[:16 * 64 * 2].view(BF).view(16, 64)
    with pytest.raises(RuntimeError, match="hold must not alias"):
        ops.change_map_blend(**dict(ok, x=xv, hold=big[16 * 64 * 2 - 32:16 * 64 * 2 + 32].view(16, 4)))
    with pytest.raises(RuntimeError, match="hold must not alias"):
        ops.change_map_blend(**dict(ok, xin=xv, hold=big[:64].view(16, 4)))
    with pytest.raises(RuntimeError, match="4-byte aligned"):
        ops.change_map_blend(**dict(ok, hold=big[2:66].view(16, 4)))
    with pytest.raises(RuntimeError, match="multiple of 8"):
        ops.change_map_blend(x[:, :12].contiguous(), x0[:, :12].contiguous(), noise[:, :12].contiguous(), hold, cut, sig)
    with pytest.raises(RuntimeError, match="ldxin"):
        ops.change_map_blend(**dict(ok, xin=torch.zeros(16, 56, dtype=BF, device="cuda")))
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        ops.change_map_blend(**dict(ok, x=torch.zeros(16, 72, dtype=BF, device="cuda")[:, 4:68]))
    with pytest.raises(ValueError, match="outside the tables"):
        ops.change_map_blend(**ok, step=len(CUT_TABLE))
    with pytest.raises(ValueError, match="hold must be contiguous uint8"):
        ops.change_map_blend(**dict(ok, hold=hold[:8]))
    with pytest.raises(TypeError, match="int32 vector of keep_sigma's length"):
        ops.change_map_blend(**dict(ok, cut=cut[:3]))
    with pytest.raises(TypeError, match="int32"):
        ops.change_map_blend(**dict(ok, cut=cut.long()))
    empty = torch.zeros(0, 64, dtype=BF, device="cuda")
    assert ops.change_map_blend(empty, empty.clone(), empty.clone(), torch.zeros(0, 4, dtype=torch.uint8, device="cuda"), cut, sig) is empty
    assert torch.equal(x, keep)                                              # nothing was launched


# ----------------------------------------------------------------------------- tfx_change_map_pack alone
def grey_map(Bm, Hm, Wm, seed):
    """random greys, with extremes at the corners of 8 x 8 blocks on and off the sampling lattice and at the image's borders"""
    m = torch.randint(0, 200, (Bm, Hm, Wm), generator=X.gen(seed)).to(torch.uint8)
    m[0, 0, 0], m[0, 7, 7], m[0, 8, 8], m[0, 15, 15] = 255, 254, 0, 253
    m[-1, Hm - 1, Wm - 1], m[-1, Hm - 8, Wm - 8], m[-1, 8, 0], m[-1, 0, Wm - 1] = 255, 0, 251, 252
    return m


@pytest.mark.parametrize("mode,grow", [(0, 0), (1, 0), (1, 1), (1, 8)], ids=["nearest", "cover0", "cover1", "cover8"])
@pytest.mark.parametrize("Bm", [1, 2])
@pytest.mark.parametrize("Hm,Wm", [(16, 16), (32, 48)], ids=["one_token", "32x48"])
def test_pack_equals_the_restatement(Hm, Wm, Bm, mode, grow):
    from textflux_amd import ops
    m = grey_map(Bm, Hm, Wm, Hm + Wm + Bm)
    want = R.pack(m, mode, grow)
    got = ops.change_map_pack(m.cuda(), mode, grow)
    assert got.shape == (Bm, (Hm // 16) * (Wm // 16), 4) and got.dtype == torch.uint8
    assert torch.equal(got.cpu(), want)
    assert torch.equal(ops.change_map_pack(m.cuda(), {0: "nearest", 1: "cover"}[mode], grow).cpu(), want)       # the mode by name
    if grow == 8:                                                            # larger than the image: every token sees the freest pixel
        assert Hm // 8 <= 8 and Wm // 8 <= 8 and (want == 255 - m.amax(dim=(1, 2))[:, None, None]).all()
    if mode == 1:
        assert (want <= R.pack(m, 0, 0)).all()                               # cover never holds longer than nearest


@pytest.mark.parametrize("mode,grow", [(0, 0), (1, 0), (1, 1), (1, 8)], ids=["nearest", "cover0", "cover1", "cover8"])
@pytest.mark.parametrize("Hm,Wm", [(16, 16), (32, 48)], ids=["one_token", "32x48"])
def test_a_binary_map_packs_to_the_keep_mask_on_the_device(Hm, Wm, mode, grow):
    """The two packers are one kernel frame with two reducers: on a map of {0, 255} the hold byte is 0 exactly where
    tfx_keep_mask_pack writes 1.0 (any byte >= 128 is the maximum being 255), and 255 elsewhere"""
    from textflux_amd import ops
    m = torch.zeros(2, Hm, Wm, dtype=torch.uint8)
    m[0, 8, 8] = m[1, Hm - 3, Wm - 5] = m[1, 5, 3] = 255                    # on the sampling lattice, and off it in two blocks
    hold = ops.change_map_pack(m.cuda(), mode, grow).cpu()
    mk = ops.keep_mask_pack(m.cuda(), 16, mode, grow).cpu()
    assert ((hold == 0) | (hold == 255)).all() and (hold[0] == 0).any()
    if (Hm, grow) == (32, 0) or (Hm, grow) == (32, 1):
        assert (hold[0] == 255).any()                                       # both values, where the window is smaller than the image
    want = (hold == 0).to(BF)[:, :, None, :].expand(2, hold.shape[1], 4, 4).reshape(2, hold.shape[1], 16)
    assert same(mk, want)


def test_pack_refusals():
    from textflux_amd import ops
    m = torch.zeros(1, 32, 48, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="grow must be 0"):
        ops.change_map_pack(m, "nearest", 1)
    with pytest.raises(RuntimeError, match="outside 0..8"):
        ops.change_map_pack(m, "cover", 9)
    with pytest.raises(RuntimeError, match="mode must be"):
        ops.change_map_pack(m, 2, 0)
    with pytest.raises(ValueError, match="multiples of 16"):
        ops.change_map_pack(m[:, :24])
    with pytest.raises(TypeError, match="uint8"):
        ops.change_map_pack(m.float())


# ----------------------------------------------------------------------------- the pipeline
_maps = {}


def maps():
    """the call's change maps and their hold bytes from the RESTATEMENT (not the device kernels): drawn once, never modified"""
    if not _maps:
        inp = inputs()
        g = X.gen(21)
        grey = (torch.arange(W) * 255 // (W - 1)).to(torch.uint8)[None, None, :].repeat(B, H, 1)         # a ramp over the width
        grey[1] = torch.randint(0, 256, (H, W), generator=g).to(torch.uint8)
        grey[0, :16, :16], grey[0, 16:32, :16] = 0, 255                     # one token that never changes, one free from step 0
        derived_cfg = dict(dilate=4, feather=3, mode="cover", grow=1)
        alpha = torch.from_numpy(PB.alpha_mask(inp["mask_u8"].numpy(), 4, 3))
        _maps.update(grey=grey, grey_hold=R.pack(grey, 0, 0), derived_cfg=derived_cfg, derived=alpha, derived_hold=R.pack(alpha, 1, 1))
        assert len(_maps["grey_hold"].unique()) > 16 and len(_maps["derived_hold"].unique()) > 2
    return _maps


def change_kw(change_map, **kw):
    inp = inputs()
    return dict(dict(change_map=change_map, image_latents=inp["x0"], mask_image=inp["mask_u8"]), **kw)


def python_loop(pipe, sname, hold, last, per_step=None):
    inp = inputs()
    c = inp["call"]
    return R.loop(pipe, inp["latents"], c["masked_image_latents"], c["prompt_embeds"], c["pooled_prompt_embeds"], GRID, inp["x0"],
                  inp["latents"], hold, last=last, sampler={"euler": "fused", "euler_unfused": "euler"}.get(sname, sname),
                  amo_noise=inp["amo_noise"], per_step=per_step)


@pytest.mark.parametrize("strength", [1.0, 0.6])
@pytest.mark.parametrize("sname", ["euler_unfused", "euler", "amo", "multistep"])
def test_step_run_ex2_equals_the_python_issued_loop(sname, strength):
    """eager and the captured graph (one for all steps and for every later call), both `last` forms, the explicit map and the derived
    one.  strength 0.6 of 4 steps runs 3 from step 1 (caller-given latents are both noise and start, as under keep_known); the cut
    table is that of the 3 steps that run."""
    pipe = make_pipe(sname)
    mp = maps()
    plain_extra = dict(amo_noise=inputs()["amo_noise"]) if sname == "amo" else {}
    extra = dict(plain_extra)
    if strength != 1.0:
        extra["strength"] = strength
        if sname == "amo":
            extra["amo_noise"] = inputs()["amo_noise"][:3]
    n_run = N_STEPS if strength == 1.0 else 3
    wants = {}
    pipe.enable_hip_graph(False)
    for last in ("keep", "free"):
        eager = call(pipe, **change_kw(dict(map=mp["grey"], last=last)), **extra)
        assert pipe.num_timesteps == n_run
        wants[last] = python_loop(pipe, sname, mp["grey_hold"], last)
        assert torch.equal(eager, wants[last]), last
    assert not torch.equal(wants["keep"], wants["free"])
    derived = call(pipe, **change_kw(mp["derived_cfg"]), **extra)
    wants["derived"] = python_loop(pipe, sname, mp["derived_hold"], "keep")
    assert torch.equal(derived, wants["derived"])
    assert torch.equal(call(pipe, **change_kw(mp["grey"]), **extra), wants["keep"])                    # the map given bare: last="keep"
    plain = call(pipe, **plain_extra)
    assert not torch.equal(plain, wants["keep"])
    ses = pipe.transformer._session
    assert not any(ses.graphs.values())
    pipe.enable_hip_graph(True)
    assert torch.equal(call(pipe, **change_kw(dict(map=mp["grey"], last="keep")), **extra), wants["keep"])
    keys = [k for k, g in ses.graphs.items() if g]
    assert len(keys) == 1 and keys[0][-1] == "change"                       # one graph, whatever the number of steps
    assert torch.equal(call(pipe, **change_kw(dict(map=mp["grey"], last="free")), **extra), wants["free"])
    assert torch.equal(call(pipe, **change_kw(mp["derived_cfg"]), **extra), wants["derived"])
    assert [k for k, g in ses.graphs.items() if g] == keys                  # ... and for every later call: tables and bytes are data
    assert torch.equal(call(pipe, **plain_extra), plain)                    # the plain call, on a graph of its own


def test_one_graph_serves_calls_of_different_lengths_and_the_step_cache_tails():
    pipe = make_pipe("euler").enable_hip_graph(True)
    mp = maps()
    want = None
    for kw, n in ((dict(), 4), (dict(strength=0.6), 3), (dict(strength=0.5), 2)):
        out = call(pipe, **change_kw(mp["grey"]), **kw)
        loop = python_loop(pipe, "euler", mp["grey_hold"], "keep")
        assert pipe.num_timesteps == n and torch.equal(out, loop), n
        want = loop if want is None else want                                # the 4-step call's
        keys = [k for k, g in pipe.transformer._session.graphs.items() if g]
        assert len(keys) == 1 and keys[0][-1] == "change", n
    for graph in (False, True):
        pipe.enable_hip_graph(graph)
        pipe.enable_step_cache(0.0)                                          # never skips: the computed tail ends in the same blend
        assert torch.equal(call(pipe, **change_kw(mp["grey"])), want), graph
        assert len(pipe.step_cache_report) == N_STEPS and not any(r["skipped"] for r in pipe.step_cache_report)
    pipe.enable_step_cache(0.0, skip_steps={2})                              # and the cached tail too
    skipped = call(pipe, **change_kw(mp["grey"]))
    assert [r["skipped"] for r in pipe.step_cache_report] == [False, False, True, False]
    assert torch.equal(call(pipe.enable_hip_graph(False), **change_kw(mp["grey"])), skipped)


def test_an_all_zero_map_returns_the_image_latents_and_an_all_255_map_the_plain_call():
    zeros = torch.zeros(B, H, W, dtype=torch.uint8)
    full = torch.full((B, H, W), 255, dtype=torch.uint8)
    for sname in ("euler", "euler_unfused", "multistep"):
        pipe = make_pipe(sname)
        plain = call(pipe)
        for graph in (False, True):
            pipe.enable_hip_graph(graph)
            assert same(call(pipe, **change_kw(dict(map=zeros, last="keep"))), inputs()["x0"]), (sname, graph)
            for last in ("keep", "free"):
                assert torch.equal(call(pipe, **change_kw(dict(map=full, last=last))), plain), (sname, graph, last)
            assert torch.equal(call(pipe, **change_kw(dict(map=full, mode="cover", grow=2))), plain)
    # last="free" with an all-zero map: the last step is the model's, so x0 is not what comes out
    assert not torch.equal(call(pipe, **change_kw(dict(map=zeros, last="free"))), inputs()["x0"])


@pytest.mark.parametrize("sname", ["euler_unfused", "euler", "amo", "multistep"])
def test_a_binary_map_is_keep_known_nearest(sname):
    inp = inputs()
    pipe = make_pipe(sname)
    extra = dict(amo_noise=inp["amo_noise"]) if sname == "amo" else {}
    for graph in (False, True):
        pipe.enable_hip_graph(graph)
        kept = call(pipe, keep_known=dict(mode="nearest"), image_latents=inp["x0"], mask_image=inp["mask_u8"], **extra)
        assert torch.equal(call(pipe, **change_kw(dict(map=inp["mask_u8"], last="keep")), **extra), kept), graph
        assert torch.equal(call(pipe, **change_kw(dict(dilate=0, feather=0)), **extra), kept), graph      # derived with no halo: the mask itself
    assert not torch.equal(call(pipe, **change_kw(dict(map=inp["mask_u8"], last="free")), **extra), kept)


def test_held_tokens_follow_the_noised_original_until_their_release_step():
    inp = inputs()
    mp = maps()
    pipe = make_pipe()
    seen = []
    out = call(pipe, **change_kw(mp["grey"]), callback_on_step_end=lambda p, i, t, kw: seen.append(kw["latents"].clone()) or {})
    assert len(seen) == N_STEPS and torch.equal(seen[-1], out)
    states = []
    assert torch.equal(out, python_loop(pipe, "euler_unfused", mp["grey_hold"], "keep", per_step=states))     # a callback: the unfused kernel
    tab, cut = R.keep_sigma(pipe.scheduler._sigmas_host), R.cut_table(N_STEPS, "keep")
    released = []
    for i in range(N_STEPS):
        assert torch.equal(seen[i], states[i]), i
        held = R.hold_mask(mp["grey_hold"], cut[i]).bool()
        proper = R.scale_noise(inp["x0"].cpu(), float(tab[i]), inp["latents"].cpu())
        assert torch.equal(bits(seen[i].cpu())[held], bits(proper)[held]), i
        released.append(int((~held).sum()))
    assert released == sorted(released) and released[0] < released[-1] and 0 < released[0]              # the held set only shrinks
    assert torch.equal(call(pipe, **change_kw(mp["grey"])), out)                                          # the fused form without the callback


def test_refusals_and_shapes():
    inp = inputs()
    pipe = make_pipe()
    mp = maps()
    with pytest.raises(ValueError, match="exclude each other"):
        call(pipe, **change_kw(mp["grey"]), keep_known=True)
    with pytest.raises(ValueError, match=r"the map is \(32, 48\), the call asks for"):
        call(pipe, **change_kw(torch.zeros(B, 32, 48, dtype=torch.uint8)))
    with pytest.raises(ValueError, match="must be uint8"):
        call(pipe, **change_kw(torch.zeros(B, H, W)))
    with pytest.raises(ValueError, match="needs `mask_image`"):
        call(pipe, change_map=True, image_latents=inp["x0"])
    with pytest.raises(ValueError, match="need `image`"):
        call(pipe, change_map=mp["grey"])
    with pytest.raises(ValueError, match="change_map packs to"):
        call(pipe, **change_kw(torch.zeros(3, H, W, dtype=torch.uint8)))
    one = call(pipe, **change_kw(mp["grey"][:1]))                            # one map for the whole batch
    assert torch.equal(one, python_loop(pipe, "euler", mp["grey_hold"][:1].repeat(B, 1, 1), "keep"))
    from PIL import Image
    pil = call(pipe, **change_kw(Image.fromarray(mp["grey"][0].numpy())))
    assert torch.equal(pil, one)
    with pytest.raises(NotImplementedError, match="call_mixed: change_map"):
        pipe.call_mixed(sizes=[(256, 256), (384, 256)], latents=[torch.zeros(1, 256, 64), torch.zeros(1, 384, 64)],
                        masked_image_latents=[torch.zeros(1, 256, 320), torch.zeros(1, 384, 320)], prompt_embeds=torch.zeros(2, 64, 64),
                        pooled_prompt_embeds=torch.zeros(2, 128), output_type="latent", change_map=True)


def test_the_derived_map_is_the_paste_backs_alpha():
    inp = inputs()
    pipe = make_pipe()
    mp = maps()
    cfg = dict(map=None, dilate=4, feather=3, mode="cover", grow=1, last="keep")
    got = pipe.change_map_u8(cfg, inp["mask_u8"], H, W, "cuda")
    assert got.dtype == torch.uint8 and torch.equal(got.cpu(), mp["derived"])
    from textflux_amd.paste_back import alpha_mask
    assert torch.equal(got, alpha_mask(inp["mask_u8"].cuda(), 4, 3))         # what paste_back blends under: the two halos agree
    assert torch.equal(pipe._change_hold(cfg, inp["mask_u8"], H, W, B, S, "cuda").cpu(), mp["derived_hold"])
