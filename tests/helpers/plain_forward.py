"""One FluxTransformer2DModel.forward restated from public pieces, one launch at a time: the independent composition
tfx_dit_forward (textflux_amd/csrc/dit_forward.cpp) is compared with, bit for bit (tests/test_forward_chain_gpu.py).  It follows
oracle/flux_oracle.py::double_block / single_block / transformer_forward, the project's restatement of the reference
(transformer_flux.py:715-739 FluxSingleTransformerBlock.forward, :794-841 FluxTransformerBlock.forward, :1086-1203 the model's
forward), on the engine's buffers hid / xn / y = [k | v | q | mlp...] of include/textflux_hip.h.

Independent of what it checks: the weights come from the REFERENCE-named state dict and are packed here (pack_weights), the
modulation rows are sliced here by the header's chunk order (mod_slices), the rotary tables come from the ids through
oracle.flux_oracle.flux_pos_embed (rope_rows), the runtime-LoRA operands from the adapter's own tensors (pack_lora).  Nothing of
FluxTransformer2DModel.w / _fusion_map, DitSession.desc / cos / sin / rope_cs is read.  temb and modulation are outside
tfx_dit_forward and stay the model's.

The chain (plain_forward) is written once against a small backend: HipBackend issues textflux_amd.ops launches -- one stream at a
time, never row-split, never with the fused q / k norm epilogue -- in buffers of its own; TorchBackend evaluates the same chain with
plain fp32 torch on the CPU, which is how tests/test_forward_chain_cpu.py holds the packing and the slicing to the oracle's blocks.

fault=: a deliberate, named mistake in THIS file's orchestration (FAULTS).  It exists only so that the tests can show their inputs
are sensitive to it."""
import torch
import torch.nn.functional as F

from oracle import flux_oracle as fo

BF = torch.bfloat16
EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_GATE_RES, EPI_COLSCALE = 0, 1, 2, 4      # include/textflux_hip.h: tfx_gemm_args.epilogue
SIX = ("shift_msa", "scale_msa", "gate_msa", "shift_mlp", "scale_mlp", "gate_mlp")

# fault -> the blocks whose output it changes: "double" / "single" / "both" ("tail": only the final norm_out + proj_out)
FAULTS = {
    "swap_shift_scale_mlp": "double",        # shift_mlp and scale_mlp swapped
    "gate_msa_for_gate_mlp": "double",       # gate_msa taken where gate_mlp belongs
    "mod_row0_for_all": "both",              # sample 0's modulation row used for every sample
    "txt_rows_img_qk_norm": "double",        # the text stream's rows normalised with the image stream's q / k norm weights
    "img_rope_from_row0": "both",            # image rows' rotary rows taken from 0 instead of T
    "txt_rope_shift_one": "both",            # text rows' rotary rows shifted by one
    "norm1_skips_last_txt_row": "double",    # the last text row left out of norm1
    "norm_out_shift_scale": "tail",          # norm_out's chunks read as [shift scale]
    "single_gelu_from_col0": "single",       # the single block's GELU starting at column 0 instead of 3D
    "to_out_reads_k": "double",              # the attention output read from the k columns by to_out
}


# ----------------------------------------------------------------------------- layout: pure torch, no device
def pack_weights(sd, cfg):
    """Reference state dict -> the fused Linears of include/textflux_hip.h ("Weight layout"): name -> dict(w [out, in], b [out],
    segs = [(reference key, first row, rows)]), and the q / k RMSNorm weights under their own names.  Dtype as given."""
    W = {}

    def put(name, keys):
        rows, segs = 0, []
        for k in keys:
            n = sd[k + ".weight"].shape[0]
            segs.append((k, rows, n))
            rows += n
        W[name] = dict(w=torch.cat([sd[k + ".weight"] for k in keys]), b=torch.cat([sd[k + ".bias"] for k in keys]), segs=segs)

    for n in ("x_embedder", "context_embedder", "proj_out"):
        put(n, [n])
    for i in range(cfg.num_layers):
        p = f"transformer_blocks.{i}"
        a = p + ".attn."
        put(f"d{i}.qkv_img", [a + "to_k", a + "to_v", a + "to_q"])
        put(f"d{i}.qkv_txt", [a + "add_k_proj", a + "add_v_proj", a + "add_q_proj"])
        put(f"d{i}.out_img", [a + "to_out.0"])
        put(f"d{i}.out_txt", [a + "to_add_out"])
        put(f"d{i}.ff1_img", [p + ".ff.net.0.proj"])
        put(f"d{i}.ff2_img", [p + ".ff.net.2"])
        put(f"d{i}.ff1_txt", [p + ".ff_context.net.0.proj"])
        put(f"d{i}.ff2_txt", [p + ".ff_context.net.2"])
        for n in ("norm_q", "norm_k", "norm_added_q", "norm_added_k"):
            W[f"d{i}.{n}"] = sd[a + n + ".weight"]
    for j in range(cfg.num_single_layers):
        p = f"single_transformer_blocks.{j}"
        a = p + ".attn."
        put(f"s{j}.qkv_mlp", [a + "to_k", a + "to_v", a + "to_q", p + ".proj_mlp"])
        put(f"s{j}.proj_out", [p + ".proj_out"])
        for n in ("norm_q", "norm_k"):
            W[f"s{j}.{n}"] = sd[a + n + ".weight"]
    return W


def mod_len(cfg):
    return (12 * cfg.num_layers + 3 * cfg.num_single_layers + 2) * cfg.inner_dim


def mod_slices(mod, cfg):
    """[B, >= mod_len] modulation rows -> column views [B, D] by the header's chunk order: double i [img: six | txt: six], single j
    [shift scale gate], norm_out [scale shift]."""
    D = cfg.inner_dim
    ch = lambda off: mod[:, off:off + D]
    dbl, sgl = [], []
    for i in range(cfg.num_layers):
        base = 12 * D * i
        dbl.append(dict(img={n: ch(base + k * D) for k, n in enumerate(SIX)}, txt={n: ch(base + 6 * D + k * D) for k, n in enumerate(SIX)}))
    base = 12 * D * cfg.num_layers
    for j in range(cfg.num_single_layers):
        sgl.append({n: ch(base + 3 * D * j + k * D) for k, n in enumerate(("shift", "scale", "gate"))})
    base += 3 * D * cfg.num_single_layers
    return dict(double=dbl, single=sgl, out=dict(scale=ch(base), shift=ch(base + D)))


def reference_modulation(sd, cfg, temb):
    """The [B, mod_len] rows the reference's own norm*.linear layers give for temb, stacked in the header's order (CPU tests)."""
    rows = []
    for i in range(cfg.num_layers):
        rows += [fo.linear(F.silu(temb), sd, f"transformer_blocks.{i}.norm1.linear"), fo.linear(F.silu(temb), sd, f"transformer_blocks.{i}.norm1_context.linear")]
    rows += [fo.linear(F.silu(temb), sd, f"single_transformer_blocks.{j}.norm.linear") for j in range(cfg.num_single_layers)]
    rows.append(fo.linear(F.silu(temb), sd, "norm_out.linear"))
    return torch.cat(rows, dim=1)


def rope_rows(txt_ids, img_ids, cfg, fault=None):
    """(cos, sin) fp32 [T + S, 128]: row r is the rotary row the chain applies to row r of the joint [text | image] stream."""
    T, S = txt_ids.shape[0], img_ids.shape[0]
    cos, sin = fo.flux_pos_embed(torch.cat((txt_ids.float(), img_ids.float()), dim=0), cfg.axes_dims_rope)
    t0 = 1 if fault == "txt_rope_shift_one" else 0
    i0 = 0 if fault == "img_rope_from_row0" else T
    pick = lambda tab: torch.cat((tab[t0:t0 + T], tab[i0:i0 + S]), dim=0).contiguous()
    return pick(cos), pick(sin)


def pack_lora(W, lora, call_scale=1.0, adapter_weight=1.0):
    """Runtime-LoRA operands as the header defines them (tfx_linear / tfx_lora_args), from a file-format adapter {"transformer.<target>
    .lora_A.weight" [r, in], ".lora_B.weight" [out, r], optional ".alpha"}: fused Linear name -> dict(acat [nseg * R, in]: the segments'
    zero-padded A stacked, wide [out, in + R] = [W | Bcat], c fp32 [nseg * R] = call scale * adapter weight * alpha / r, R, nseg,
    seg_cols, mask).  R: the rank padded to 128."""
    where = {k: (name, s, r0, n) for name, L in W.items() if isinstance(L, dict) for s, (k, r0, n) in enumerate(L["segs"])}
    out = {}
    for key in sorted(k for k in lora if k.endswith(".lora_A.weight")):
        t = key[len("transformer."):-len(".lora_A.weight")]
        A, Bm = lora[key].to(BF), lora[key.replace("lora_A", "lora_B")].to(BF)
        r = A.shape[0]
        alpha = float(lora.get(f"transformer.{t}.alpha", float(r)))
        name, seg, row0, rows = where[t]
        L = W[name]
        N, K = L["w"].shape
        nseg, R = len(L["segs"]), (r + 127) // 128 * 128
        p = out.setdefault(name, dict(acat=torch.zeros(nseg * R, K, dtype=BF), bcat=torch.zeros(N, R, dtype=BF),
                                      c=torch.zeros(nseg * R, dtype=torch.float32), R=R, nseg=nseg, mask=0,
                                      seg_cols=L["segs"][1][1] if nseg > 1 else N))
        assert p["R"] == R and not (p["mask"] >> seg) & 1
        p["acat"][seg * R:seg * R + r] = A
        p["bcat"][row0:row0 + rows, :r] = Bm
        p["c"][seg * R:seg * R + r] = call_scale * adapter_weight * (alpha / r)
        p["mask"] |= 1 << seg
    for name, p in out.items():
        p["wide"] = torch.cat((W[name]["w"].to(BF), p.pop("bcat")), dim=1).contiguous()
    return out


def is_block_linear(name):
    return name[0] in "ds" and name[1:].split(".")[0].isdigit()


# ----------------------------------------------------------------------------- backends
class TorchBackend:
    """The chain's launches as plain torch on the CPU in the dtype of the weights (fp32 in the tests): no device, no rounding scheme."""

    def __init__(self, W, cfg, B, S, T):
        self.W, self.cfg, self.B, self.S, self.T, self.N = W, cfg, B, S, T, S + T
        D = cfg.inner_dim
        dt = W["x_embedder"]["w"].dtype
        self.hid, self.xn, self.y = (torch.zeros(B, self.N, c, dtype=dt) for c in (D, D, 7 * D))
        self.out = torch.zeros(B, S, W["proj_out"]["w"].shape[0], dtype=dt)

    def tensor(self, t):
        return t

    def ln(self, r0, r1, shift, scale, consumer=None):
        if r1 > r0:
            self.xn[:, r0:r1] = fo.layer_norm(self.hid[:, r0:r1]) * (1 + scale[:, None]) + shift[:, None]

    def _epi(self, v, out, epi, gelu_from, gate):
        if epi == EPI_BIAS_GELU:
            v = torch.cat((v[..., :gelu_from], F.gelu(v[..., gelu_from:], approximate="tanh")), dim=-1)
        out.copy_(out + gate[:, None] * v if epi == EPI_BIAS_GATE_RES else v)

    def plain(self, name, x, out):
        out.copy_(F.linear(x, self.W[name]["w"], self.W[name]["b"]))

    def linear(self, name, src, r0, r1, c0, K, out, epi=EPI_BIAS, gelu_from=0, gate=None):
        if r1 > r0:
            x = (self.xn if src == "xn" else self.y)[:, r0:r1, c0:c0 + K]
            self._epi(F.linear(x, self.W[name]["w"], self.W[name]["b"]), out, epi, gelu_from, gate)

    def norm_rope(self, r0, r1, wq, wk, cos, sin):
        D, H = self.cfg.inner_dim, self.cfg.num_attention_heads
        for c0, w in ((2 * D, wq), (0, wk)):
            v = self.y[:, r0:r1, c0:c0 + D]
            h = fo.apply_rope(fo.rms_norm(v.reshape(self.B, r1 - r0, H, 128).transpose(1, 2), w), cos, sin)
            v.copy_(h.transpose(1, 2).reshape(self.B, r1 - r0, D))

    def attention(self, bound):
        D, H = self.cfg.inner_dim, self.cfg.num_attention_heads
        k, v, q = (self.y[:, :, c:c + D].reshape(self.B, self.N, H, 128).transpose(1, 2) for c in (0, D, 2 * D))
        self.y[:, :, 2 * D:3 * D] = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(self.B, self.N, D)

    def copy_rows(self, src, dst):
        dst.copy_(src)


class HipBackend:
    """The chain's launches as textflux_amd.ops calls in freshly allocated buffers.  fp8: block Linears with in % 256 == 0 (the
    header's rule for flags bit 2) run as ln_modulate_fp8 / quantize_rows_fp8 + gemm_fp8 on tfx_quantize_rows_fp8 of the same weights.
    lora: pack_lora()'s operands; an adapted Linear runs as the column-scaled down projection(s) into a T buffer that mirrors its
    input's, then gemm_lora."""

    def __init__(self, W, cfg, B, S, T, fp8=False, lora=None, device="cuda"):
        from textflux_amd import ops
        self.ops, self.cfg, self.B, self.S, self.T, self.N, self.fp8, self.dev = ops, cfg, B, S, T, S + T, fp8, device
        dev = lambda t: t.to(device, BF).contiguous()
        self.W = {n: (dict(w=dev(L["w"]), b=dev(L["b"])) if isinstance(L, dict) else dev(L)) for n, L in W.items()}
        if fp8:
            for n, L in self.W.items():
                if isinstance(L, dict) and is_block_linear(n) and L["w"].shape[1] % 256 == 0:
                    L["w8"], L["w8s"] = ops.quantize_rows_fp8(L["w"])
        self.lora = {n: {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in p.items()} for n, p in (lora or {}).items()}
        D, N = cfg.inner_dim, self.N
        nan = float("nan")
        # [0] the buffer itself, above it the T matrices of the adapted Linears that read it: xn's one per segment (up to 4), y's one
        self.xnT = torch.zeros(5 if lora else 1, B, N, D, dtype=BF, device=device)
        self.yT = torch.zeros(2 if lora else 1, B, N, 7 * D, dtype=BF, device=device)
        self.hid = torch.full((B, N, D), nan, dtype=BF, device=device)
        self.xn, self.y = self.xnT[0].fill_(nan), self.yT[0].fill_(nan)
        self.out = torch.full((B, S, W["proj_out"]["w"].shape[0]), nan, dtype=BF, device=device)
        self._q = {}

    def tensor(self, t):
        return t.to(self.dev)

    def _fp8_linear(self, name):
        return self.fp8 and "w8" in self.W[name]

    def ln(self, r0, r1, shift, scale, consumer=None):
        if r1 <= r0:
            return
        if consumer is not None and self._fp8_linear(consumer):
            self._q[(r0, r1)] = self.ops.ln_modulate_fp8(self.hid[:, r0:r1], shift, scale)
        else:
            self.ops.ln_modulate(self.hid[:, r0:r1], shift, scale, out=self.xn[:, r0:r1])

    def plain(self, name, x, out):
        self.ops.gemm(x, self.W[name]["w"], self.W[name]["b"], out=out)

    def linear(self, name, src, r0, r1, c0, K, out, epi=EPI_BIAS, gelu_from=0, gate=None):
        if r1 <= r0:
            return
        ops, L = self.ops, self.W[name]
        x = (self.xn if src == "xn" else self.y)[:, r0:r1, c0:c0 + K]
        kw = dict(out=out, epilogue=epi, gelu_from_col=gelu_from)
        if epi == EPI_BIAS_GATE_RES:
            kw.update(gate=gate, res=out)
        p = self.lora.get(name)
        if p is not None:
            R, nseg = p["R"], p["nseg"]
            tb = self.xnT if src == "xn" else self.yT
            if nseg * R > tb.shape[-1]:        # the segments' T blocks do not fit one row of the input's buffer: a matrix per segment
                for s in range(nseg):
                    if (p["mask"] >> s) & 1:
                        ops.gemm(x, p["acat"][s * R:(s + 1) * R], None, out=tb[1 + s][:, r0:r1, c0:c0 + R], epilogue=EPI_COLSCALE,
                                 cscale=p["c"][s * R:(s + 1) * R])
                t, stride = tb[1][:, r0:r1, c0:c0 + R], tb.stride(0)
            else:
                t, stride = tb[1][:, r0:r1, c0:c0 + nseg * R], 0
                ops.gemm(x, p["acat"], None, out=t, epilogue=EPI_COLSCALE, cscale=p["c"])
            ops.gemm_lora(x, t, p["wide"], K, R, p["seg_cols"], nseg, p["mask"], L["b"], t_seg_stride=stride, **kw)
        elif self._fp8_linear(name):
            q, qs = self._q.pop((r0, r1)) if src == "xn" else ops.quantize_rows_fp8(x)
            ops.gemm_fp8(q, qs, L["w8"], L["w8s"], L["b"], **kw)
        else:
            ops.gemm(x, L["w"], L["b"], **kw)

    def norm_rope(self, r0, r1, wq, wk, cos, sin):
        if r1 > r0:
            self.ops.rmsnorm_rope_(self.y[:, r0:r1], 2 * self.cfg.inner_dim, 0, self.cfg.num_attention_heads, 0, wq, wk, wq, wk,
                                   cos.contiguous(), sin.contiguous())

    def attention(self, bound):
        D, y = self.cfg.inner_dim, self.y
        self.ops.attention(y[:, :, 2 * D:3 * D], y[:, :, :D], y[:, :, D:2 * D], out=y[:, :, 2 * D:3 * D], score_bound=bound)

    def copy_rows(self, src, dst):
        self.ops.copy_rows_(src, dst)


# ----------------------------------------------------------------------------- the chain
def double_block(be, i, m, cos, sin, bound, fault=None):
    """FluxTransformerBlock.forward (transformer_flux.py:794-841), the image stream's rows [T, N) then the text stream's [0, T)."""
    D, T, N, W = be.cfg.inner_dim, be.T, be.N, be.W
    streams = [("img", T, N, m["img"], W[f"d{i}.norm_q"], W[f"d{i}.norm_k"]), ("txt", 0, T, m["txt"], W[f"d{i}.norm_added_q"], W[f"d{i}.norm_added_k"])]
    if fault == "txt_rows_img_qk_norm":
        streams[1] = streams[1][:4] + streams[0][4:]
    for s, r0, r1, ms, nq, nk in streams:      # norm1 -> [k | v | q] -> per-head RMSNorm + RoPE of q, k  (:799-806, attention_processor.py)
        skip = 1 if fault == "norm1_skips_last_txt_row" and s == "txt" else 0
        be.ln(r0, r1 - skip, ms["shift_msa"], ms["scale_msa"], consumer=None if skip else f"d{i}.qkv_{s}")
        if skip:                               # the row the faulty range misses keeps what was there: here, its un-normalised hidden state
            be.copy_rows(be.hid[:, r1 - 1:r1], be.xn[:, r1 - 1:r1])
        be.linear(f"d{i}.qkv_{s}", "xn", r0, r1, 0, D, be.y[:, r0:r1, :3 * D])
        be.norm_rope(r0, r1, nq, nk, cos[r0:r1], sin[r0:r1])
    be.attention(bound)
    for s, r0, r1, ms, _, _ in streams:        # hidden += gate_msa * to_out(attn)  (:817-818, 830-831)
        be.linear(f"d{i}.out_{s}", "y", r0, r1, 0 if fault == "to_out_reads_k" else 2 * D, D, be.hid[:, r0:r1], EPI_BIAS_GATE_RES, gate=ms["gate_msa"])
    for s, r0, r1, ms, _, _ in streams:        # norm2 * (1 + scale_mlp) + shift_mlp -> ff -> gated residual  (:820-826, 833-837)
        sh, sc = (ms["scale_mlp"], ms["shift_mlp"]) if fault == "swap_shift_scale_mlp" else (ms["shift_mlp"], ms["scale_mlp"])
        be.ln(r0, r1, sh, sc, consumer=f"d{i}.ff1_{s}")
        be.linear(f"d{i}.ff1_{s}", "xn", r0, r1, 0, D, be.y[:, r0:r1, 3 * D:], EPI_BIAS_GELU, gelu_from=0)
        be.linear(f"d{i}.ff2_{s}", "y", r0, r1, 3 * D, 4 * D, be.hid[:, r0:r1], EPI_BIAS_GATE_RES,
                  gate=ms["gate_msa" if fault == "gate_msa_for_gate_mlp" else "gate_mlp"])


def single_block(be, j, m, cos, sin, bound, fault=None):
    """FluxSingleTransformerBlock.forward (transformer_flux.py:715-739) on the joint [text | image] rows."""
    D, N, W = be.cfg.inner_dim, be.N, be.W
    be.ln(0, N, m["shift"], m["scale"], consumer=f"s{j}.qkv_mlp")
    be.linear(f"s{j}.qkv_mlp", "xn", 0, N, 0, D, be.y, EPI_BIAS_GELU, gelu_from=0 if fault == "single_gelu_from_col0" else 3 * D)
    be.norm_rope(0, N, W[f"s{j}.norm_q"], W[f"s{j}.norm_k"], cos, sin)
    be.attention(bound)
    be.linear(f"s{j}.proj_out", "y", 0, N, 2 * D, 5 * D, be.hid, EPI_BIAS_GATE_RES, gate=m["gate"])


def plain_forward(be, mod, cos, sin, bounds, xin=None, prompt_embeds=None, hid0=None, blocks=None, tail=True, fault=None):
    """The forward on backend `be`.  mod [B, >= mod_len]; cos / sin: rope_rows(); bounds: (double, single) score bounds per block
    (FluxTransformer2DModel.attn_score_bounds()).  xin [B, S, in_channels] and prompt_embeds [B, T, joint dim] feed the embedders
    (transformer_flux.py:1086, 1099) -- or hid0 [B, N, D] preloads the joint stream.  blocks: the block indices to run (all).
    Returns dict(hid = [the joint stream before block 0, after block 0, ...] as clones, out = the model output or None)."""
    cfg, T, N = be.cfg, be.T, be.N
    L = cfg.num_layers
    if fault == "mod_row0_for_all":
        mod = mod[:1].repeat(mod.shape[0], 1)
    m = mod_slices(mod, cfg)
    cos, sin = be.tensor(cos), be.tensor(sin)
    if hid0 is not None:
        be.hid.copy_(hid0)
    else:
        be.plain("x_embedder", xin, be.hid[:, T:])
        if T > 0:
            ctx0 = torch.empty(be.B, T, cfg.inner_dim, dtype=be.hid.dtype, device=be.hid.device)
            be.plain("context_embedder", prompt_embeds, ctx0)
            be.copy_rows(ctx0, be.hid[:, :T])
    hids = [be.hid.clone()]
    for k in (range(L + cfg.num_single_layers) if blocks is None else blocks):
        if k < L:
            double_block(be, k, m["double"][k], cos, sin, bounds[0][k], fault)
        else:
            single_block(be, k - L, m["single"][k - L], cos, sin, bounds[1][k - L], fault)
        hids.append(be.hid.clone())
    out = None
    if tail:       # norm_out (AdaLayerNormContinuous: chunks scale, shift) + proj_out on the image rows  (:1200-1203)
        sh, sc = (m["out"]["scale"], m["out"]["shift"]) if fault == "norm_out_shift_scale" else (m["out"]["shift"], m["out"]["scale"])
        be.ln(T, N, sh, sc)
        be.plain("proj_out", be.xn[:, T:], be.out)
        out = be.out.clone()
    return dict(hid=hids, out=out)


def euler_on_output(ops, out, xin, dsigma):
    """The latents after tfx_euler_step on the stored model output `out` [B, S, C], sample b with its own bf16-rounded dsigma[b]:
    what the fused Euler epilogue must leave in xin[:, :, :C]."""
    C = out.shape[-1]
    lat = xin[:, :, :C].clone().contiguous()
    coef = dsigma.to(BF).float().to(out.device).contiguous()
    for b in range(out.shape[0]):
        ops.euler_step_(out[b].contiguous(), lat[b], coef, step=b)
    return lat
