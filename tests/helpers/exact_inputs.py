"""Inputs on which the matrix-pipe kernels have ONE correct answer per output element, and that answer restated on the CPU.

Every generator draws from a seeded CPU torch.Generator and asserts its own exactness condition when called: operands whose
products and partial sums are small integers (or dyadic fractions) are summed exactly by fp32 in EVERY order, so a GEMM, a
convolution or an attention launch -- generic or MFMA, one tile or persistent, K-sliced or not, whole items or dealt units --
must store one definite bf16 bit pattern per element, and so must the plain fp64 / integer restatement here.  No tolerance is
budgeted for the summation order; assert_elementwise compares per element and names the tile of the first differences.

No expected value here comes from a restated kernel: they come from torch matmul / conv2d / softmax in fp64 (or fp32 on
integers, where fp32 is exact) and from torch's own bf16 operators for the rounding chains the C header documents.  Two host
restatements exist beside them: guarded_walk (the guarded attention kernel's reference policy, for the CPU tests that show the dyadic
cases drive it and for their fault injection -- the dyadic form's expected value is a plain weighted sum) and attention64_graded_chain
(attention64's rounding points, the one form whose expected value is a chain).
"""
import functools
import math

import torch

BF = torch.bfloat16
F8 = torch.float8_e4m3fn
GATES = (0.5, 0.75, 1.0, 1.5, 2.0)                      # epilogue 2: +- these
NORM_WEIGHTS = (0.5, 0.75, 1.0, 1.25, 1.5)              # q / k RMSNorm weights
NORM_SHIFTS = (0.125, 0.375, 0.625, 0.875, 1.125)       # GroupNorm beta: no magnitude of NORM_WEIGHTS, so +-gamma + beta never cancels
ROPE_PAIRS = ((1.0, 0.0), (-1.0, 0.0), (0.0, 1.0), (0.0, -1.0), (0.5, 0.5), (0.5, -0.5), (-0.5, 0.5), (-0.5, -0.5))   # (cos, sin)
ACC_LIMIT = 256                                         # every integer of magnitude <= 256 is a bf16 value


def gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def ternary(shape, seed: int, p_nonzero: float = 0.25) -> torch.Tensor:
    """fp32 entries in {-1, 0, 1}: P(non-zero) = p_nonzero, both signs equally likely."""
    u = torch.rand(shape, generator=gen(seed))
    return torch.where(u < p_nonzero / 2, -1.0, torch.where(u < p_nonzero, 1.0, 0.0))


def integers(shape, lo: int, hi: int, seed: int) -> torch.Tensor:
    return torch.randint(lo, hi + 1, shape, generator=gen(seed)).float()


def choice(values, shape, seed: int, signed: bool = False) -> torch.Tensor:
    t = torch.tensor(values, dtype=torch.float32)[torch.randint(0, len(values), shape, generator=gen(seed))]
    if signed:
        t = t * torch.where(torch.rand(shape, generator=gen(seed + 7919)) < 0.5, -1.0, 1.0)
    return t


def arbitrary_bf16(shape, seed: int, scale: float = 1.0) -> torch.Tensor:
    return (torch.randn(shape, generator=gen(seed)) * scale).to(BF)


# --------------------------------------------------------------------------------------------------------- comparison
def _ordered(t: torch.Tensor) -> torch.Tensor:
    """bf16 bit patterns as integers that count bf16 steps: neighbours differ by one, +0 and -0 are both 0."""
    bits = t.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
    mag = bits & 0x7FFF
    return torch.where((bits & 0x8000) != 0, -mag, mag)


def mismatches(got: torch.Tensor, want: torch.Tensor, ulps: int = 0) -> torch.Tensor:
    """bool mask of the elements of `got` more than `ulps` bf16 steps from `want` (fp32 tensors: any difference).  A NaN on either
    side is a mismatch; +0 and -0 are the same value (torch.equal's convention)."""
    assert got.shape == want.shape, (tuple(got.shape), tuple(want.shape))
    assert got.dtype == want.dtype, (got.dtype, want.dtype)
    if got.dtype == BF:
        bad = (_ordered(got) - _ordered(want)).abs() > ulps
    else:
        assert ulps == 0, "steps are counted for bf16 only"
        bad = got != want
    return bad | torch.isnan(got) | torch.isnan(want)


def assert_elementwise(got: torch.Tensor, want: torch.Tensor, what: str, ulps: int = 0, cap: float = None) -> int:
    """Every element of got [.., rows, cols] within `ulps` bf16 steps of want (0: the same value).  cap: only with ulps > 0 -- at most
    this share of the elements may differ from `want` at all.  Returns the number of elements that are not bit-equal.  The failure
    message lists the first sixteen offenders as (batch, row, column), their 256 x 256 tile and the position inside it."""
    got, want = got.detach().cpu(), want.detach().cpu()
    bad = mismatches(got, want, ulps)
    n_bad = int(bad.sum())
    n_diff = n_bad if ulps == 0 else int(mismatches(got, want, 0).sum())
    if n_bad == 0 and (cap is None or n_diff <= cap * got.numel()):
        return n_diff
    if n_bad == 0:
        raise AssertionError(f"{what}: every element is within {ulps} bf16 step(s), but {n_diff} of {got.numel()} differ "
                             f"({n_diff / got.numel():.3e}), more than the cap {cap:.3e}")
    idx = bad.reshape(-1, *bad.shape[-2:]) if bad.dim() >= 2 else bad.reshape(1, 1, -1)
    g3, w3 = got.reshape(idx.shape), want.reshape(idx.shape)
    lines = []
    for b, r, c in idx.nonzero()[:16].tolist():
        lines.append(f"  (batch {b}, row {r}, col {c})  tile ({r // 256}, {c // 256}) at ({r % 256}, {c % 256}): "
                     f"got {g3[b, r, c].item()!r}, want {w3[b, r, c].item()!r}")
    rows = idx.any(-1).sum().item()
    cols = idx.any(-2).sum().item() if idx.shape[-2] > 0 else 0
    raise AssertionError(f"{what}: {n_bad} of {got.numel()} elements differ by more than {ulps} bf16 step(s) "
                         f"({rows} rows and {cols} (batch, column) lines touched); first {len(lines)}:\n" + "\n".join(lines))


# --------------------------------------------------------------------------------------------------------- GEMM
def gemm_operands(B: int, M: int, N: int, K: int, seed: int, w_batched: bool = False, product: bool = True, p_nonzero: float = 0.25) -> dict:
    """a [B, M, K], w [N, K] (or [B, N, K]) ternary-sparse bf16, bias [N] integers in [-8, 8]; acc = a w^T as fp64 integers (None when
    product is False: shapes whose product the caller takes on the device).  Asserted: max|acc + bias| <= 256."""
    a = ternary((B, M, K), seed + 1, p_nonzero)
    w = ternary((B, N, K) if w_batched else (N, K), seed + 2, p_nonzero)
    bias = integers((N,), -8, 8, seed + 3)
    cs = dict(a=a.to(BF), w=w.to(BF), bias=bias.to(BF), acc=None)
    if product:
        acc = a.double() @ (w.double().transpose(-1, -2))
        check_accumulators(acc, bias)
        cs["acc"] = acc
    return cs


def check_accumulators(acc: torch.Tensor, bias: torch.Tensor = None) -> None:
    """The exactness condition of the integer GEMM / convolution: integers, |acc| and |acc + bias| <= 256 (bias along the last axis)."""
    assert bool((acc == acc.round()).all()), "accumulators must be integers"
    top = acc.abs().max().item()
    if bias is not None:
        top = max(top, (acc + bias.to(acc.dtype)).abs().max().item())
    assert top <= ACC_LIMIT, f"max|a w^T + bias| = {top} leaves the exact regime (<= {ACC_LIMIT})"


def gates(B: int, N: int, seed: int) -> torch.Tensor:
    return choice(GATES, (B, N), seed, signed=True).to(BF)


def pow2(shape, lo: int, hi: int, seed: int) -> torch.Tensor:
    return torch.exp2(torch.randint(lo, hi + 1, shape, generator=gen(seed)).float())


def gelu_tanh64(x: torch.Tensor) -> torch.Tensor:
    """F.gelu(x, approximate="tanh") in fp64 as x * sigmoid(2u), u = sqrt(2/pi) (x + 0.044715 x^3): the same function as
    0.5 x (1 + tanh u) without the cancelling 1 + tanh(u) for very negative x (fp64 would return 0 where the value is 1e-30)."""
    x = x.double()
    u = math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)
    return x / (1.0 + torch.exp(-2.0 * u))


def linear_bf16(acc: torch.Tensor, bias: torch.Tensor = None, row_scale: torch.Tensor = None, col_scale: torch.Tensor = None) -> torch.Tensor:
    """bf16(acc * row_scale * col_scale + bias): the Linear's stored output, rounded ONCE from the exact value.  The value is asserted
    to be an fp32 number, so the fp64 -> bf16 conversion rounds what the kernel's fp32 epilogue holds."""
    v = acc.double()
    if row_scale is not None:
        v = v * row_scale.double()[..., None]
    if col_scale is not None:
        v = v * col_scale.double()
    if bias is not None:
        v = v + bias.double()
    assert bool((v.float().double() == v).all()), "pre-rounding value must be exact in fp32"
    return v.float().to(BF)


def chain(epilogue: int, lin: torch.Tensor, res: torch.Tensor = None, gate: torch.Tensor = None, gelu_from_col: int = 0) -> torch.Tensor:
    """The epilogue chains of include/textflux_hip.h on the Linear's bf16 output `lin` [B, M, N], with torch's bf16 operators (each
    rounds once): 0 lin | 3 bf16(res + lin) | 2 bf16(res + bf16(gate * lin)) | 1 bf16(gelu_tanh(lin)) on columns >= gelu_from_col."""
    assert lin.dtype == BF
    if epilogue == 0:
        return lin
    if epilogue == 3:
        return res + lin
    if epilogue == 2:
        return res + gate[:, None, :] * lin
    if epilogue == 1:
        out = lin.clone()
        out[..., gelu_from_col:] = gelu_tanh64(lin[..., gelu_from_col:]).float().to(BF)
        return out
    raise ValueError(epilogue)


def gelu_exact_mask(lin: torch.Tensor, gelu_from_col: int) -> torch.Tensor:
    """Elements of an epilogue-1 output that must match bit for bit: the plain columns, and GELU columns whose value is 0 or x itself."""
    m = torch.ones(lin.shape, dtype=torch.bool)
    g = gelu_tanh64(lin[..., gelu_from_col:])
    x = lin[..., gelu_from_col:].double()
    m[..., gelu_from_col:] = (g == 0) | (g == x)
    return m


# --------------------------------------------------------------------------------------------------------- fp8
def fp8_bytes(t: torch.Tensor) -> torch.Tensor:
    """e4m3 bytes of values that e4m3 holds exactly (asserted)."""
    q = t.float().to(F8)
    assert bool((q.float() == t.float()).all()), "values must be e4m3 numbers"
    return q.view(torch.uint8)


def quantizable_rows(shape, seed: int, edge_peaks: bool = False):
    """bf16 rows whose quantisation is known exactly: row r = 2^e_r * integers in [-8, 8] with one entry +-448, so the scale is 2^e_r
    and the codes are the integers.  edge_peaks: the first row of every sample has its +-448 in the last column and the second row in
    the first, so a row maximum that misses the last (partly filled) round of a workgroup's lanes gives another scale.
    Returns (x bf16, codes uint8, scale fp32)."""
    ints = integers(shape, -8, 8, seed)
    pos = torch.randint(0, shape[-1], shape[:-1], generator=gen(seed + 1))
    if edge_peaks:
        pos[..., 0] = shape[-1] - 1
        pos[..., 1:2] = 0
    sign = torch.where(torch.rand(shape[:-1], generator=gen(seed + 2)) < 0.5, -448.0, 448.0)
    ints.scatter_(-1, pos[..., None], sign[..., None])
    scale = pow2(shape[:-1], -3, 3, seed + 3)
    x = ints * scale[..., None]
    assert bool((x.to(BF).float() == x).all())
    return x.to(BF), fp8_bytes(ints), scale


# --------------------------------------------------------------------------------------------------------- K-sliced launches
def plan_slices(T: int, per_batch: int, batch: int, nt: int, ws_bytes: int, grid: int):
    """gemm.hip::plan_slices restated: (slices, whole-tile units, sliced tiles per sample) of a persistent-kernel GEMM with T tiles of
    nt K-tiles (128 bytes of a row: 64 bf16 or 128 e4m3 values), a workspace and gemm_splitk = 2 (the default).  A slice keeps an even
    number >= 8 of K-tiles, a (tile, slice) unit takes 256 KiB of the workspace."""
    def ok(units, c):
        return units * c <= grid and nt % (2 * c) == 0 and nt // c >= 8 and units * c * 262144 <= ws_bytes
    if T < grid:
        for c in (8, 6, 4, 3, 2):
            if ok(T, c):
                return c, 0, per_batch
        return 1, 0, 0
    R = T % grid
    if R == 0 or T // grid >= 8 or R % batch:
        return 1, 0, 0
    for c in (4, 3, 2):
        if ok(R, c):
            return c, T - R, R // batch
    return 1, 0, 0


def gemm_tiles(B: int, M: int, N: int):
    """(T, tiles per sample) of 256 x 256 output tiles."""
    per_batch = ((M + 255) // 256) * ((N + 255) // 256)
    return B * per_batch, per_batch


def plan_slices_bf16(B: int, M: int, N: int, K: int, ws_bytes: int, grid: int):
    T, per_batch = gemm_tiles(B, M, N)
    return plan_slices(T, per_batch, B, K // 64, ws_bytes, grid)


def plan_slices_fp8(B: int, M: int, N: int, K: int, ws_bytes: int, grid: int):
    """gemm.hip::launch_fp8: K-tiles of 128 e4m3 bytes, and only a whole GEMM with fewer tiles than workgroups is sliced."""
    T, per_batch = gemm_tiles(B, M, N)
    return plan_slices(T, per_batch, B, K // 128, ws_bytes, grid) if T < grid else (1, 0, 0)


@functools.lru_cache(maxsize=None)
def fp8_sliced_case(B: int, M: int, N: int, K: int) -> dict:
    """One K-sliced fp8 case, shared by the GPU test and the CPU fault injection: gemm_operands' ternary values (as e4m3 bytes: aq, wq),
    power-of-two row scales sa [B, M] and channel scales sw [N], gate and res, and lin = bf16(acc * sa * sw + bias).  The accumulator
    bound max|acc + bias| <= 256 holds at the default density of a quarter for every K of GEMM_FP8_KSLICE (K = 15360: 4.5 standard
    deviations of sqrt(K / 16) = 31 are 140), so no case lowers it.  Callers must not modify what they get."""
    seed = shape_seed(B, M, N, K, 8)
    cs = gemm_operands(B, M, N, K, seed)
    cs.update(sa=pow2((B, M), -3, 3, seed + 5), sw=pow2((N,), -3, 3, seed + 6), gate=gates(B, N, seed + 11), res=arbitrary_bf16((B, M, N), seed + 12),
              aq=fp8_bytes(cs["a"]), wq=fp8_bytes(cs["w"]))
    cs["lin"] = linear_bf16(cs["acc"], cs["bias"].float(), row_scale=cs["sa"], col_scale=cs["sw"])
    return cs


def k_slice_products(cs: dict, slices: int) -> torch.Tensor:
    """fp64 [slices, B, M, N]: the contribution of each of `slices` equal K ranges to acc (their sum is acc, asserted)."""
    a, w = cs["a"].double(), cs["w"].double()
    K = a.shape[-1]
    assert K % slices == 0
    ks = K // slices
    parts = torch.stack([a[..., s * ks:(s + 1) * ks] @ w[:, s * ks:(s + 1) * ks].T for s in range(slices)])
    assert torch.equal(parts.sum(0), cs["acc"])
    return parts


# --------------------------------------------------------------------------------------------------------- q / k norm + RoPE
def rope_table(rows: int, seed: int, B: int = 0) -> torch.Tensor:
    """fp32 [rows, 64, 2] (or [B, rows, 64, 2]) of (cos, sin) pairs drawn per (row, pair) from the eight dyadic pairs."""
    shape = (B, rows, 64) if B else (rows, 64)
    return torch.tensor(ROPE_PAIRS, dtype=torch.float32)[torch.randint(0, 8, shape, generator=gen(seed))].contiguous()


def norm_weights(seed: int) -> torch.Tensor:
    return choice(NORM_WEIGHTS, (128,), seed).to(BF)


def qk_norm_rope(lin: torch.Tensor, ranges, weights, cs: torch.Tensor, eps: float = 1e-6, r_ulps: int = 0) -> torch.Tensor:
    """Per-head RMSNorm * weight, then the interleaved-pair rotation, on the column ranges `ranges` = ((lo, hi), ...) of lin
    [B, M, N] bf16 with `weights` = (w, ...) one bf16 [128] per range and cs [M, 64, 2] or [B, M, 64, 2]: the rounding points of
    tfx_rmsnorm_rope -- bf16(x * r), bf16(.* w), bf16(rotation) -- with r = rsqrt(sum x^2 / 128 + eps): the argument in fp32, the root
    in fp64 rounded once (torch.rsqrt in fp32 is asserted to lie within one step of it), so a device rsqrt that is accurate to one
    step returns r or a neighbour.  r_ulps: move every row factor by that many fp32 steps (the measurement of the comparison's cap).
    Asserted: |lin| <= 256, so the 128 squares sum exactly in fp32 (<= 2^23) in any order."""
    assert lin.dtype == BF and lin.dim() == 3
    out = lin.clone()
    B, M, _ = lin.shape
    cos, sin = cs[..., 0], cs[..., 1]
    if cs.dim() == 3:
        cos, sin = cos[None], sin[None]
    cos, sin = cos[:, :, None, :], sin[:, :, None, :]                              # [B | 1, M, 1, 64]
    for (lo, hi), w in zip(ranges, weights):
        x = lin[..., lo:hi].float().view(B, M, (hi - lo) // 128, 128)
        assert x.abs().max().item() <= ACC_LIMIT
        ss = (x.double() ** 2).sum(-1, keepdim=True)
        assert ss.max().item() <= 2 ** 23
        arg = ss.float() * (1.0 / 128.0) + eps                                      # fp32, as the kernels form it (ss / 128 is exact)
        r = (1.0 / torch.sqrt(arg.double())).float()                                # the correctly rounded fp32 factor ...
        t = torch.rsqrt(arg)                                                        # ... which torch.rsqrt (1 / sqrt, two roundings) is one step from at most
        assert bool(((r == t) | (torch.nextafter(r, t) == t)).all())
        for _ in range(abs(r_ulps)):
            r = torch.nextafter(r, torch.full_like(r, math.inf if r_ulps > 0 else 0.0))
        y = ((x * r).to(BF).float() * w.float()).to(BF).float()
        y0, y1 = y[..., 0::2], y[..., 1::2]
        o0, o1 = y0 * cos - y1 * sin, y1 * cos + y0 * sin
        for o, e in ((o0, y0.double() * cos.double() - y1.double() * sin.double()), (o1, y1.double() * cos.double() + y0.double() * sin.double())):
            assert bool((o.double() == e).all()), "the rotation must be exact in fp32"
        out[..., lo:hi] = torch.stack([o0, o1], -1).reshape(B, M, hi - lo).to(BF)
    return out


def expand_pairs(cs: torch.Tensor):
    """(cos, sin) [.., rows, 128] as tfx_rmsnorm_rope reads them (every value twice) from a pair table [.., rows, 64, 2]."""
    return cs[..., 0].repeat_interleave(2, -1).contiguous(), cs[..., 1].repeat_interleave(2, -1).contiguous()


# --------------------------------------------------------------------------------------------------------- attention
def _valid_lengths(B, N, lengths):
    L = [N] * B if lengths is None else [int(x) for x in lengths]
    assert len(L) == B and all(1 <= x <= N for x in L)
    return L


def _zero_sum_values(L: int, D: int, g: torch.Generator) -> torch.Tensor:
    """z [L, D] of +-128: every column sums to zero -- L // 2 rows of random signs, their negatives, one zero row when L is odd --
    with the rows in shuffled order."""
    h = L // 2
    s = torch.where(torch.rand(h, D, generator=g) < 0.5, -128.0, 128.0)
    z = torch.cat([s, -s, torch.zeros(L - 2 * h, D)], 0)
    return z[torch.randperm(L, generator=g)]


@functools.lru_cache(maxsize=None)
def uniform_attention(B: int, H: int, N: int, seed: int, lengths=None, D: int = 128, pad=float("nan"), nonzero_c: bool = False):
    """q = 0 (every weight exactly 1), k arbitrary, v = c + z with integer c[b, h, d] in [-3, 3] and z = +-128 summing to zero over each
    sample's valid keys.  Expected output: c in every valid row.  Rows >= lengths[b] of q / k / v hold `pad`.
    Returns (q, k, v, want) as bf16 [B, N, H * D]; want's padding rows are NaN (the caller checks its own sentinel there).
    Asserted: every value an integer bf16 holds, partial sums below 2^24, and one key more or less moves the result by more than a bf16 step."""
    g = gen(seed)
    L = _valid_lengths(B, N, lengths)
    c = torch.randint(-3, 4, (B, 1, H, D), generator=g).float()
    if nonzero_c:       # no value of v is 0 then (the zero row of an odd key count holds c): a selected v has a bf16 step to be exact within
        c = torch.where(c == 0, torch.where(torch.rand(c.shape, generator=g) < 0.5, -1.0, 1.0), c)
    q = torch.zeros(B, N, H, D)
    k = torch.randn(B, N, H, D, generator=g)
    v = torch.full((B, N, H, D), pad)
    want = torch.full((B, N, H, D), float("nan"))
    for b in range(B):
        for h in range(H):
            v[b, :L[b], h] = c[b, 0, h] + _zero_sum_values(L[b], D, g)
        want[b, :L[b]] = c[b]
        q[b, L[b]:], k[b, L[b]:] = pad, pad
        vb = v[b, :L[b]]
        assert bool((vb == vb.round()).all()) and vb.abs().max().item() <= 131 and bool((vb.to(BF).float() == vb).all())
        assert L[b] * 131 < 2 ** 24 and bool((vb.sum(0) == L[b] * c[b, 0]).all())
        assert 128.0 / L[b] > 2 ** -6, "a dropped key must move |c| <= 3 by more than one bf16 step (2^-6 in [2, 4))"
    return tuple(t.reshape(B, N, H * D).to(BF) for t in (q, k, v, want))


def selector_values(shape, g: torch.Generator) -> torch.Tensor:
    """bf16 values with every mantissa and both signs, 0.5 <= |v| < 2: any two differ by less than 4, and half a bf16 step of the
    smallest is 2^-10."""
    mant = 1.0 + torch.randint(0, 128, shape, generator=g).float() / 128.0
    e = torch.where(torch.rand(shape, generator=g) < 0.5, 0.5, 1.0)
    return mant * e * torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)


def selector_margin(qh: torch.Tensor, kh: torch.Tensor, pi: torch.Tensor, scale: float, causal: bool = False) -> float:
    """n_keys * exp(-(own score - largest other score)) of one (sample, head): qh, kh [L, D] fp32 with integer-valued products."""
    L = qh.shape[0]
    s = (qh @ kh.T) * scale
    own = s[torch.arange(L), pi].clone()
    s[torch.arange(L), pi] = -math.inf
    if causal:
        s = s + torch.full((L, L), -math.inf).triu(1)
    if L == 1:
        return 0.0
    gap = (own - s.max(-1).values).min().item()
    return L * math.exp(-gap)


@functools.lru_cache(maxsize=None)
def selector_attention(B: int, H: int, N: int, seed: int, lengths=None, D: int = 128, mult: float = 3.0, scale: float = None,
                       causal: bool = False, pad=float("nan")):
    """k[j] = a random +-1 code of D entries, q[i] = mult * k[pi(i)] with one permutation pi of the valid rows per (sample, head)
    (causal: a random map with pi(i) <= i), v = selector_values.  The chosen key's scaled score is mult * D * scale, the others are
    mult * N(0, 1) * sqrt(D) * scale.  Expected output: v[pi(i)].
    Asserted on the realised data, per (sample, head): n_keys * exp(-(own score - largest other score)) <= 2^-12.  The other keys
    then move an output by at most 4 * 2^-12 = 2^-10 (values differ by < 4), half a bf16 step of the smallest |v| = 0.5, before
    a softmax's own fp32 rounding (~2^-20): the stored bf16 is v[pi(i)].  Returns (q, k, v, want, max |scaled score|)."""
    g = gen(seed)
    scale = D ** -0.5 if scale is None else scale
    L = _valid_lengths(B, N, lengths)
    q, k, v = (torch.full((B, N, H, D), pad) for _ in range(3))
    want = torch.full((B, N, H, D), float("nan"))
    worst = 0.0
    for b in range(B):
        n = L[b]
        for h in range(H):
            code = torch.where(torch.rand(n, D, generator=g) < 0.5, -1.0, 1.0)
            if causal:
                pi = (torch.rand(n, generator=g) * (torch.arange(n) + 1)).long().clamp(max=n - 1)
                pi = torch.minimum(pi, torch.arange(n))
            else:
                pi = torch.randperm(n, generator=g)
            vals = selector_values((n, D), g)
            k[b, :n, h], q[b, :n, h], v[b, :n, h], want[b, :n, h] = code, mult * code[pi], vals, vals[pi]
            worst = max(worst, selector_margin(mult * code[pi], code, pi, scale, causal))
    assert worst <= 2 ** -12, f"selector margin {worst:.3e} > 2^-12 at B {B} H {H} N {N} (lengths {lengths})"
    return tuple(t.reshape(B, N, H * D).to(BF) for t in (q, k, v, want)) + (mult * D * scale,)


@functools.lru_cache(maxsize=None)
def bias_selector_attention(B: int, H: int, N: int, delta: int, seed: int, D: int = 64, peak: float = 24.0):
    """attention64's relative bias as the selector: q = 0, rel_bias [H, 2N - 1] zero except `peak` at index delta + N - 1, so query i
    puts weight 1 on key i + delta and exp(-peak) on every other one; v has uniform_attention's zero-sum structure with c != 0, so that
    no v is 0 (a selected 0 would have to come out as exactly 0, which a running-maximum kernel that rescales its early keys' weights
    by exp2 differences cannot promise and need not).  Expected: row i = v[i + delta] where that key exists (the others move it by
    < N * exp(-24) * 262 = 5e-6, far inside half a bf16 step of |v| >= 1, 2^-9), else the uniform answer c.
    Returns (q, k, v, rel_bias fp32, want)."""
    assert -(N - 1) <= delta <= N - 1 and N * math.exp(-peak) * 262 < 2.0 ** -12
    q, k, v, c = uniform_attention(B, H, N, seed, None, D, nonzero_c=True)
    assert v.float().abs().min().item() >= 1.0
    bias = torch.zeros(H, 2 * N - 1)
    bias[:, delta + N - 1] = peak
    want = c.clone()
    lo, hi = max(0, -delta), min(N, N - delta)                                   # queries whose target exists
    want[:, lo:hi] = v[:, lo + delta:hi + delta]
    return q, k, v, bias, want


def _softmax_times(s: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """softmax(s) v in fp64 as (exp(s - max) v) / sum exp(s - max): weights of exactly 1 then meet integer values in an exact sum
    (torch.softmax divides first, and n * (1 / n) * c is not c)."""
    p = torch.exp(s - s.max(-1, keepdim=True).values)
    return (p @ v) / p.sum(-1, keepdim=True)


def attention64_reference(q, k, v, scale, rel_bias=None, causal=False, D=64):
    """fp64 softmax(scale q k^T + bias) v of bf16 [B, N, H * D] operands, rounded once."""
    B, N, HD = q.shape
    H = HD // D
    qh, kh, vh = (t.double().view(B, N, H, D).transpose(1, 2) for t in (q, k, v))
    s = (qh @ kh.transpose(-1, -2)) * scale
    if rel_bias is not None:
        idx = torch.arange(N)[None, :] - torch.arange(N)[:, None] + N - 1
        s = s + rel_bias.double()[:, idx]
    if causal:
        s = s + torch.full((N, N), -math.inf, dtype=torch.float64).triu(1)
    return _softmax_times(s, vh).transpose(1, 2).reshape(B, N, HD).float().to(BF)


def attention_reference(q, k, v, lengths=None, D=128, scale=None):
    """fp64 softmax attention over each sample's valid rows, rounded once; rows beyond a sample's length are NaN."""
    B, N, HD = q.shape
    H = HD // D
    L = _valid_lengths(B, N, lengths)
    out = torch.full((B, N, HD), float("nan"), dtype=torch.float64)
    for b in range(B):
        qh, kh, vh = (t[b, :L[b]].double().view(L[b], H, D).transpose(0, 1) for t in (q, k, v))
        s = (qh @ kh.transpose(-1, -2)) * (D ** -0.5 if scale is None else scale)
        out[b, :L[b]] = _softmax_times(s, vh).transpose(0, 1).reshape(L[b], HD)
    return out.float().to(BF)


# --------------------------------------------------------------------------------------------------------- attention, dyadic form
# Every softmax weight an exact power of two, every row sum a power of two, v integer: the scores and the reference offset, exp2f of an
# integer, the bf16 packing of the weights, P.V and the row sums, the exp2f(-d) rescale of a reference move, the merge weights and
# inv = 1 / l all have exactly representable fp32 results, and the one rounding is the final bf16 pack of o * inv, whose argument is exact.
# attention_w4.hip passes a.scale * 1.4426950408889634f to its kernels, which pre-scale q with it: DYADIC_SCALE = 0.125 ln 2 rounded to
# fp32 makes that product exactly 0.125f, so q = 8.0 at one head-dim index d and 0 elsewhere gives the exp2-domain score k[j][d] itself.
DYADIC_SCALE = float.fromhex("0x1.62e43p-4")            # 0.08664339780807495
DYADIC_DEPTH = 16                                       # no weight below 2^-16 of its column's sum
DYADIC_FAMILIES = ("bounded", "far")                    # |score| <= 50 (both streams) | also columns near -200 and near +250 (guarded only)
DYADIC_KINDS = ("ascending", "descending", "shuffled", "spike", "block")    # key order of a column's weights, see dyadic_attention
DYADIC_SETS = 8                                         # exponent multisets per key count; a column takes one of them
W4_TILE, W4_UNIT, W4_ROWS, W4_THR = 64, 32, 32, 4.0     # attention_w4.hip: keys per tile (W4_KV) | per pipeline step (a 32 x 32 MFMA block) |
#                                                         query rows of a q-block (one wave's any-row vote) | W4_THR


def _split_multiset(n: int, g: torch.Generator, root: int = 0, floor: int = 0) -> list:
    """n exponents e with sum 2^-e = 2^-root exactly: start from {root}, replace one e by two e + 1, n - 1 times, never beyond
    DYADIC_DEPTH.  The leaf to split is uniform among those that may split, except that leaves above `floor` go first (shallowest first):
    with n >= 2^(floor - root) every exponent ends at `floor` or deeper.  Returned sorted ascending."""
    cnt = [0] * (DYADIC_DEPTH + 1)
    cnt[root] = 1
    assert 1 <= n <= 2 ** (DYADIC_DEPTH - root)
    u = torch.rand(max(n - 1, 1), generator=g).tolist()
    for i in range(n - 1):
        shallow = next((e for e in range(root, floor) if cnt[e]), None)
        if shallow is None:
            t = u[i] * sum(cnt[:DYADIC_DEPTH])
            for e in range(DYADIC_DEPTH):
                t -= cnt[e]
                if t < 0:
                    break
            else:
                e = max(e for e in range(DYADIC_DEPTH) if cnt[e])
        else:
            e = shallow
        cnt[e] -= 1
        cnt[e + 1] += 2
    out = [e for e in range(DYADIC_DEPTH + 1) for _ in range(cnt[e])]
    assert len(out) == n and sum(2 ** (DYADIC_DEPTH - e) for e in out) == 2 ** (DYADIC_DEPTH - root)
    return out


def dyadic_column(h: int, rows: torch.Tensor) -> torch.Tensor:
    """d(h, i): the head-dim index query row i of head h selects -- (2h + 1) i + 5h mod 128: all 128 indices over any 128 consecutive
    rows, and neighbouring rows differ."""
    return ((2 * h + 1) * rows + 5 * h) % 128


def dyadic_offsets(b: int, h: int, family: str) -> torch.Tensor:
    """c_d [128] integers: a column's scores are c_d - e, e in [0, 16].  bounded: c_d in [-34, 50], so |score| <= 50 (50 ln 2 = 34.7 <= 35,
    the score_bound the reference-free stream is given).  far: every third column near -200 (the first tile must pin), every third near
    +250, the rest as bounded."""
    d = torch.arange(128)
    c = (d * 29 + h * 13 + b * 7) % 85 - 34
    if family == "far":
        c = torch.where(d % 3 == 0, -184 - (d + h) % 7, torch.where(d % 3 == 1, 256 - (d + b) % 21, c))
    else:
        assert family == "bounded"
    return c


def dyadic_kind(h: int, d: torch.Tensor) -> torch.Tensor:
    return (d + h) % len(DYADIC_KINDS)


def _dyadic_exponents(L: int, b: int, h: int, g: torch.Generator, pool, spikes) -> torch.Tensor:
    """E [128, L] int64: column d's exponents along the keys, in the order its kind asks for."""
    d = torch.arange(128)
    sets = torch.tensor(pool)[(d * 3 + h + b) % DYADIC_SETS]                    # [128, L] sorted ascending (weights descending)
    kind = dyadic_kind(h, d)
    perm = torch.rand(128, L, generator=g).argsort(1)
    E = torch.gather(sets, 1, perm)                                              # shuffled
    E = torch.where((kind == 0)[:, None], sets.flip(1), E)                       # weights ascending along the keys
    E = torch.where((kind == 1)[:, None], sets, E)
    ustart = W4_UNIT * ((L - 1) // W4_UNIT)                                      # the last 32-key step of the last tile
    for c in d[kind == 3].tolist():                                              # the one large weight sits in the last step
        rest = torch.tensor(spikes[c % len(spikes)])[perm[c][perm[c] < L - 1]] if L > 1 else torch.empty(0, dtype=torch.long)
        pos = ustart + (c * 7) % (L - ustart)
        E[c] = torch.cat([rest[:pos], torch.tensor([1 if L > 1 else 0]), rest[pos:]])
    G = max(1, L // 8)
    for c in d[kind == 4].tolist():                                              # the G largest weights as one run, its place by column
        rest = sets[c, G:][perm[c][perm[c] < L - G] if L > G else slice(0, 0)]
        pos = ((c * 37 + 11 * h + 5 * b) % 97) * (L - G) // 96 if L > G else 0
        pos = min(pos, L - G)
        E[c] = torch.cat([rest[:pos], sets[c, :G].flip(0), rest[pos:]])
    return E


@functools.lru_cache(maxsize=None)
def _dyadic_parts(B: int, H: int, N: int, seed: int, lengths):
    """What the families share: the valid lengths, the exponents E[(b, h)] int8 [128, L_b] and the values [B, N, H, 128]."""
    g = gen(seed)
    L = _valid_lengths(B, N, lengths)
    pools = {n: [_split_multiset(n, g) for _ in range(DYADIC_SETS)] for n in sorted(set(L))}
    spikes = {n: [_split_multiset(n - 1, g, 1, 6) for _ in range(2)] if n > 1 else [[]] for n in sorted(set(L))}
    vals = torch.randint(1, 65, (B, N, H, 128), generator=g).float() * torch.where(torch.rand(B, N, H, 128, generator=g) < 0.5, -1.0, 1.0)
    E = {(b, h): _dyadic_exponents(L[b], b, h, g, pools[L[b]], spikes[L[b]]).to(torch.int8) for b in range(B) for h in range(H)}
    return L, E, vals


@functools.lru_cache(maxsize=None)
def dyadic_attention(B: int, H: int, N: int, seed: int, lengths=None, family: str = "bounded", D: int = 128, pad=float("nan")):
    """q[i] = 8.0 at index d(h, i) (dyadic_column), k[j][d] = c_d - e[j][d], v non-zero integers in [-64, 64] (every head its own): with
    scale = DYADIC_SCALE query i's exp2-domain scores are column d(h, i) of k, its weights 2^-e[j][d] up to the common 2^c_d.
    Every column's exponents are a multiset with sum 2^-e = 1 exactly (_split_multiset; DYADIC_SETS of them per key count, built over each
    sample's own L keys), laid along the keys by the column's kind (d + h) mod 5:
      ascending   the weights grow along the keys: the guarded kernel's reference has to move again and again
      descending  the first unit holds the maximum: the reference never moves
      shuffled
      spike       one weight of 1/2 in the last 32-key step of the last (ragged) tile, every other at most 2^-6 (given >= 33 keys): every
                  earlier tile's maximum is >= 5 below it, more than W4_THR.  (An exponent of 0 beside other keys would make the sum 2.)
      block       the L / 8 largest weights as one run at a place that depends on the column, so that the key ranges of a tail split or a
                  stream-K deal end with different references
    and offset by c_d (dyadic_offsets, by `family`; the families share exponents and values).  Expected output: sum_j 2^-e[j][d(i)] v[j]
    in fp64 (exact), rounded to bf16 once.
    Returns (q, k, v, want) bf16 [B, N, H * D]; rows >= lengths[b] of q / k / v hold `pad`, of want NaN.
    Asserted: every score an integer of magnitude <= 256 (<= 50 in the bounded family); every column sums to 1; for every row
    sum_j 2^(16 - e_j) |v_j| < 2^24, so every partial sum, in any order and against any reference, is an fp32 number; the expected value
    is an fp32 number."""
    assert D == 128
    L, Es, vals = _dyadic_parts(B, H, N, seed, lengths)
    q, k, v = (torch.full((B, N, H, D), pad) for _ in range(3))
    want = torch.full((B, N, H, D), float("nan"))
    for b in range(B):
        n = L[b]
        rows = torch.arange(n)
        for h in range(H):
            E = Es[b, h].long()
            c = dyadic_offsets(b, h, family)
            w = torch.exp2(-E.double())                                          # [128, n]
            s = c[:, None] - E
            assert bool((w.sum(1) == 1.0).all()) and int(E.min()) >= 0 and int(E.max()) <= DYADIC_DEPTH
            assert int(s.abs().max()) <= (50 if family == "bounded" else ACC_LIMIT)
            vh = vals[b, :n, h].double()
            assert float((torch.exp2(16.0 - E.double()) @ vh.abs()).max()) < 2 ** 24
            col = w @ vh                                                         # [128, D], exact
            assert bool((col.float().double() == col).all())
            dm = dyadic_column(h, rows)
            qh = torch.zeros(n, D)
            qh[rows, dm] = 8.0
            q[b, :n, h], k[b, :n, h], v[b, :n, h], want[b, :n, h] = qh, s.T.float(), vals[b, :n, h], col[dm].float()
    out = tuple(t.reshape(B, N, H * D).to(BF) for t in (q, k, v, want))
    assert all(bool((t.float().nan_to_num(0.0) == r.reshape(B, N, H * D).nan_to_num(0.0)).all()) for t, r in zip(out[:3], (q, k, v)))
    return out


def dyadic_scores(k: torch.Tensor, b: int, h: int, L: int, rows: torch.Tensor = None) -> torch.Tensor:
    """fp64 [rows, L]: the exp2-domain scores of head h of sample b of a dyadic_attention k -- q.k * scale log2 e = k[j][d(h, i)]."""
    rows = torch.arange(L) if rows is None else rows
    return k[b, :L, h * 128:(h + 1) * 128].double()[:, dyadic_column(h, rows)].T.contiguous()


def guarded_walk(s: torch.Tensor, v: torch.Tensor = None, fault: dict = None) -> dict:
    """attn_w4_kernel<0>'s reference policy and arithmetic restated on the host in fp64 (exact on dyadic inputs): s [R, K] exp2-domain
    scores of R consecutive query rows that start a q-block (W4_ROWS rows: one wave's vote) over the K keys of one key range, v [K, D].
    Keys go by units of W4_UNIT (two per W4_TILE-key tile).  The first unit pins every row's reference m to the unit's maximum.  A later
    unit moves the references of a q-block when ANY of its rows has a maximum more than W4_THR above its reference: every row of the block
    then moves by max(excess, 0) = d, rescales what it has accumulated by 2^-d and shifts the unit's scores by d.  Weights are 2^(s - m).
    Returns o [R, D], l [R], m [R] (un-normalised, as a tail-split / stream-K piece leaves them), moves [R] (moves with d != 0),
    late [R] (those inside the last tile) and events [(unit, q-block)] of the moves.
    fault (the tests' fault injection, one unit `unit` and q-block `block`): kind "skip_rescale" the rescale left out | "rescale_other"
    applied to the neighbouring q-block's rows instead | "no_shift" the unit's scores not shifted | "double" (tile, row): the weights of
    one row doubled in one tile."""
    R, K = s.shape
    s = s.double()
    grp = torch.arange(R) // W4_ROWS
    ng = int(grp[-1]) + 1
    m, l, moves, late = torch.zeros(R, dtype=torch.float64), torch.zeros(R, dtype=torch.float64), torch.zeros(R, dtype=torch.long), torch.zeros(R, dtype=torch.long)
    o = None if v is None else torch.zeros(R, v.shape[1], dtype=torch.float64)
    events = []
    nu = (K + W4_UNIT - 1) // W4_UNIT
    last_tile = (K - 1) // W4_TILE
    kind = fault["kind"] if fault else None
    for u in range(nu):
        su = s[:, u * W4_UNIT:min(K, (u + 1) * W4_UNIT)]                         # keys >= K are masked: they are not there
        mx = (su - m[:, None]).max(1).values
        if u == 0:
            d = mx
        else:
            take = torch.zeros(ng, dtype=torch.bool)
            take[grp[mx > W4_THR]] = True
            d = torch.where(take[grp], mx.clamp(min=0.0), torch.zeros_like(mx))
            moved = d != 0
            moves += moved
            if u // 2 == last_tile:
                late += moved
            events += [(u, int(x)) for x in grp[moved].unique()]
        m_old = m
        m = m + d
        assert bool((m.float().to(BF).double() == m).all()), "a reference must be a bf16 number"
        f = torch.exp2(-d) if u else torch.ones_like(d)
        shift = m
        if fault and fault.get("unit") == u and kind in ("skip_rescale", "rescale_other", "no_shift"):
            mine = grp == fault["block"]
            if kind == "no_shift":
                shift = torch.where(mine, m_old, m)
            else:
                if kind == "rescale_other":
                    other = grp == (fault["block"] ^ 1)
                    assert int(mine.sum()) == W4_ROWS and int(other.sum()) == W4_ROWS
                    g2 = torch.ones_like(f)
                    g2[other] = f[mine]
                    f = torch.where(mine, torch.ones_like(f), f) * g2
                else:
                    f = torch.where(mine, torch.ones_like(f), f)
        p = torch.exp2(su - shift[:, None])
        if kind == "double" and u // 2 == fault["tile"]:
            p[fault["row"]] *= 2.0
        l = l * f + p.sum(1)
        if o is not None:
            o = o * f[:, None] + p @ v[u * W4_UNIT:u * W4_UNIT + su.shape[1]].double()
    return dict(o=o, l=l, m=m, moves=moves, late=late, events=events)


def merge_pieces(pieces, wrong=None) -> torch.Tensor:
    """attn_w4_merge_kernel / attn_w4_merge_sk_kernel: O = sum_r o_r 2^(m_r - m) / sum_r l_r 2^(m_r - m), m = max_r m_r, rounded to bf16
    once.  wrong = (r, r2): piece r weighted with piece r2's reference (fault injection)."""
    m = torch.stack([p["m"] for p in pieces]).max(0).values
    acc, l = 0.0, 0.0
    for r, p in enumerate(pieces):
        w = torch.exp2(pieces[wrong[1]]["m"] - m) if wrong and wrong[0] == r else torch.exp2(p["m"] - m)
        acc, l = acc + p["o"] * w[:, None], l + p["l"] * w
    return finish_rows(acc, l)


def finish_rows(o: torch.Tensor, l: torch.Tensor) -> torch.Tensor:
    """bf16(o * (1 / l)) of exact fp64 accumulators."""
    return (o * (1.0 / l)[:, None]).float().to(BF)


def sk_bound(c: int, group: int, share: int, nkv: int, total: int) -> int:
    """attention_w4.hip::w4_sk_bound: boundary c of a sample's dealt tail units, snapped to the item boundary when it would leave a piece
    shorter than four tiles."""
    if c >= group:
        return total
    p = c * share
    if p >= total:
        return total
    r = p % nkv
    if r < 4:
        p -= r
    elif r > nkv - 4:
        p += nkv - r
    return min(p, total)


def streamk_pieces(H: int, N: int, B: int, cus: int, item: int):
    """Key-tile ranges [(t0, t1), ...] of tail item `item` (an index among the dealt items of one sample) of a stream-K launch on `cus`
    CUs (a multiple of eight), or None when attention_w4.hip::joint_attention_w4 would not deal this shape there."""
    group, nkv, Tp = cus // B, (N + W4_TILE - 1) // W4_TILE, H * ((N + 255) // 256)
    R = Tp - (Tp // group) * group
    share = (R * nkv + group - 1) // group if R else 0
    if not (R > 0 and nkv >= 16 and share * 6 >= nkv and share >= 8):
        return None
    total = R * nkv
    cuts = sorted({sk_bound(c, group, share, nkv, total) for c in range(group + 1)} | {item * nkv, (item + 1) * nkv})
    cuts = [p - item * nkv for p in cuts if item * nkv <= p <= (item + 1) * nkv]
    return list(zip(cuts[:-1], cuts[1:]))


# --------------------------------------------------------------------------------------------------------- attention64, graded form
# tfx_attention64 multiplies by `scale`, adds the bias and only then multiplies by log2 e in fp32: its exp2-domain scores are no integers
# for any scale, so the dyadic form is not available.  The graded form gives it small-integer NATURAL scores that grow along the keys, so
# that the running maximum moves (alpha != 1) in most 32-key blocks, and a restatement that follows the kernel's rounding points.
# ATTN64_GRADED_SHARE: the share of the output elements of all the cases whose bf16 value changes when every exponential (weights and
# alpha) and the row sum of the restatement move by one fp32 step either way; tests/test_exact_inputs_cpu.py measures it, the GPU test
# compares with ulps=1 and allows 4 * ATTN64_GRADED_SHARE of all elements to differ at all.
ATTN64_GRADED_MODES = ("plain", "causal", "bias")
ATTN64_GRADED_SHARE = 243 / 4080384


@functools.lru_cache(maxsize=None)
def graded_attention64(B: int, H: int, N: int, seed: int, mode: str = "plain", D: int = 64):
    """q[i] = 8.0 at index (2h + 1) i + 5h mod 64 (scale 0.125: the natural score is k[j][d]), k[j][d] = j // g_d + ((7 j + d) mod 3) - 1 -
    top_d with g_d in (8, 16, 24, 32) by column: integers that rise by a unit every g_d keys, so the maximum of nearly every 32-key block
    exceeds the one before, jittered so that a block's weights are not monotone; top_d keeps |k| <= 72.
    v: integers of magnitude 1 .. 64, one sign per column.  mode "bias": an integer rel_bias [H, 2N - 1] in [-3, 3] (fp32) is returned as well, else None.
    Returns (q, k, v, rel_bias); the expected value comes from attention64_graded_chain."""
    assert mode in ATTN64_GRADED_MODES
    g = gen(seed)
    j, d = torch.arange(N)[:, None], torch.arange(D)[None, :]
    gd = torch.tensor((8, 16, 24, 32))[(d + d // 4) % 4]
    q, k = torch.zeros(B, N, H, D), torch.zeros(B, N, H, D)
    for b in range(B):
        for h in range(H):
            kk = j // gd + (7 * j + d + h + b) % 3 - 1
            k[b, :, h] = (kk - (kk.max(0, keepdim=True).values - (d + h) % 9)).float()
            q[b, torch.arange(N), h, ((2 * h + 1) * torch.arange(N) + 5 * h) % D] = 8.0
    assert k.abs().max().item() <= 72
    # one sign per (sample, head, column): an output is then a weighted mean of values of one sign, |out| >= 1.  With mixed signs some of
    # the 4 million outputs cancel to 1e-5 of the sum of |p v|, and the fp32 roundings of the accumulation (2^-24 of THAT sum) are more
    # than a bf16 step of such a result: no tolerance counted in bf16 steps would describe a correct kernel there
    v = torch.randint(1, 65, (B, N, H, D), generator=g).float() * torch.where(torch.rand(B, 1, H, D, generator=g) < 0.5, -1.0, 1.0)
    bias = torch.randint(-3, 4, (H, 2 * N - 1), generator=g).float() if mode == "bias" else None
    return tuple(t.reshape(B, N, H * D).to(BF) for t in (q, k, v)) + (bias,)


def attention64_graded_chain(q, k, v, scale: float, rel_bias=None, causal: bool = False, exp_ulps: int = 0, sum_ulps: int = 0, D: int = 64):
    """attn64_kernel (textenc.hip) restated with its rounding points, everything between them in fp64.  Per query row and 32-key block:
    s = fp32((scale q.k + bias) * fp32(log2 e)) (the natural score must be an integer: asserted), keys >= N or beyond a causal row -inf;
    m = the running maximum after the block; alpha = fp32(exp2(fp32(m_before - m))); p = fp32(exp2(fp32(s - m))); l = l * alpha + sum p
    (the UNROUNDED weights); o = o * alpha + bf16(p) . v.  At the end inv = fp32(1 / fp32(l)), out = bf16(fp32(fp32(o) * inv)).
    exp_ulps / sum_ulps: every exponential (p and alpha) / the final row sum moved by that many fp32 steps (the cap's measurement)."""
    B, N, HD = q.shape
    H = HD // D
    log2e = torch.tensor(1.4426950408889634, dtype=torch.float32)
    qh, kh, vh = (t.double().view(B, N, H, D).transpose(1, 2) for t in (q, k, v))       # [B, H, N, D]
    nat = (qh @ kh.transpose(-1, -2)) * scale
    if rel_bias is not None:
        idx = torch.arange(N)[None, :] - torch.arange(N)[:, None] + N - 1
        nat = nat + rel_bias.double()[:, idx]
    assert bool((nat == nat.round()).all()) and nat.abs().max().item() < 2 ** 10
    s = nat.float() * log2e                                                               # one fp32 rounding
    if causal:
        s = s + torch.full((N, N), -math.inf).triu(1)
    m = torch.full((B, H, N), -math.inf)
    l = torch.zeros(B, H, N, dtype=torch.float64)
    o = torch.zeros(B, H, N, D, dtype=torch.float64)

    def ex(x):                                                                            # fp32 exp2 of an fp32 argument, moved by exp_ulps
        r = torch.exp2(x.double()).float()
        return nudge(r, exp_ulps) if exp_ulps else r
    for kb in range((N + 31) // 32):
        sb = s[..., kb * 32:(kb + 1) * 32]
        m_new = torch.maximum(m, sb.max(-1).values)
        m_use = torch.where(m_new == -math.inf, torch.zeros_like(m_new), m_new)
        alpha = ex(m - m_use).double()
        p = ex(sb - m_use[..., None])
        l = l * alpha + p.double().sum(-1)
        o = o * alpha[..., None] + p.to(BF).double() @ vh[:, :, kb * 32:(kb + 1) * 32]
        m = m_new
    lf = l.float()
    if sum_ulps:
        lf = nudge(lf, sum_ulps)
    inv = (1.0 / lf.double()).float()
    out = (o.float().double() * inv.double()[..., None]).float().to(BF)
    return out.transpose(1, 2).reshape(B, N, HD)


def attention64_graded_cases():
    return [(N, H, mode) for N in ATTN64_NS for H in ATTN64_HS for mode in ATTN64_GRADED_MODES]


# --------------------------------------------------------------------------------------------------------- convolution
def conv_operands(B, H, W, Cin, Cout, seed, stride=1, up=1, with_res=False):
    """x [B, Cin, H, W], w [Cout, Cin, 3, 3] ternary-sparse, integer bias; `want` = F.conv2d in fp64 on the NCHW view (nearest 2x
    upsample first when up == 2; stride 2 pads (0, 1, 0, 1) as the VAE's downsample does), rounded once, then bf16(res + .) with a
    residual.  Asserted: max|conv + bias| <= 256 before the residual.  Returns NHWC / KRSC bf16 operands and want [B, H', W', Cout]."""
    F = torch.nn.functional
    x, w, bias = ternary((B, Cin, H, W), seed + 1), ternary((Cout, Cin, 3, 3), seed + 2), integers((Cout,), -8, 8, seed + 3)
    xin = F.interpolate(x.double(), scale_factor=2.0, mode="nearest") if up == 2 else x.double()
    if stride == 2:
        acc = F.conv2d(F.pad(xin, (0, 1, 0, 1)), w.double(), None, stride=2, padding=0)
    else:
        acc = F.conv2d(xin, w.double(), None, stride=1, padding=1)
    acc = acc.permute(0, 2, 3, 1).contiguous()
    check_accumulators(acc, bias)
    lin = linear_bf16(acc, bias)
    res = arbitrary_bf16(lin.shape, seed + 4) if with_res else None
    return dict(x=x.permute(0, 2, 3, 1).contiguous().to(BF), w=w.permute(0, 2, 3, 1).contiguous().to(BF), bias=bias.to(BF), res=res,
                acc=acc, want=(res + lin) if with_res else lin)


# --------------------------------------------------------------------------------------------------------- rows with exact statistics
def zero_sum_rows(shape, D: int, seed: int, amp: int, offset: int = 0) -> torch.Tensor:
    """fp32 [*shape, D] of integers: every row is D / 2 draws from [-amp, amp] and their negatives in a shuffled order, plus the integer
    `offset`, so a row's sum is exactly offset * D.  Asserted: every value is a bf16 number, amp * D + |offset| * D < 2^24 (every partial
    sum of a row is an integer fp32 holds) and sum (x - offset)^2 < 2^24, and so is sum x^2.  Then the mean (= offset), the centred values
    and either sum of squares are exact in fp32 in EVERY summation order: the one freedom left to a kernel is the fp32 row factor."""
    assert D % 2 == 0 and amp * D + abs(offset) * D < 2 ** 24
    g = gen(seed)
    rows = int(torch.Size(shape).numel())
    h = torch.randint(-amp, amp + 1, (rows, D // 2), generator=g).float()
    z = torch.cat([h, -h], 1)
    z = torch.gather(z, 1, torch.rand(rows, D, generator=g).argsort(1))
    x = (z + float(offset)).view(*shape, D)
    assert bool((x.to(BF).float() == x).all()), "every value must be a bf16 number"
    assert bool((x.double().sum(-1) == offset * D).all())
    assert ((x.double() - offset) ** 2).sum(-1).max().item() < 2 ** 24 and (x.double() ** 2).sum(-1).max().item() < 2 ** 24
    return x


def zero_sum_groups(B: int, HW: int, C: int, groups: int, seed: int, offset: int = 0) -> torch.Tensor:
    """fp32 [B, HW, C] (NHWC): the HW * C / groups values of every (sample, group) are a zero_sum_rows row (+ offset) whose amplitude
    is 2, 4 or 8 by (sample, group), so that neighbouring groups have clearly different statistics."""
    cpg = C // groups
    n = HW * cpg
    x = torch.empty(B, HW, C)
    for i, amp in enumerate((2, 4, 8)):
        rows = zero_sum_rows((B, groups), n, seed + i, amp, offset)                     # [B, groups, n]
        pick = (torch.arange(B)[:, None] * 5 + torch.arange(groups)[None, :]) % 3 == i
        blk = rows.view(B, groups, HW, cpg).permute(0, 2, 1, 3)                         # [B, HW, groups, cpg]
        x.view(B, HW, groups, cpg)[:] = torch.where(pick[:, None, :, None], blk, x.view(B, HW, groups, cpg)) if i else blk
    return x


def nudge(r: torch.Tensor, ulps: int) -> torch.Tensor:
    """r (fp32, positive) moved by `ulps` fp32 steps (negative: towards zero)."""
    for _ in range(abs(ulps)):
        r = torch.nextafter(r, torch.full_like(r, math.inf if ulps > 0 else 0.0))
    return r


def row_factor(arg: torch.Tensor) -> torch.Tensor:
    """rsqrt(arg) of an fp32 argument: the root in fp64 rounded once, asserted to lie within one fp32 step of torch.rsqrt -- a device
    rsqrt that is accurate to one step returns it or a neighbour."""
    assert arg.dtype == torch.float32 and bool((arg > 0).all())
    r = (1.0 / torch.sqrt(arg.double())).float()
    t = torch.rsqrt(arg)
    assert bool(((r == t) | (torch.nextafter(r, t) == t)).all())
    return r


def layernorm_factor(x: torch.Tensor, eps: float):
    """(mean, r) [.., 1] fp32 of zero_sum_rows rows as the LayerNorm kernels form them: mean = sum / D, r = rsqrt(sum (x - mean)^2 / D +
    eps) with the quotient and the sum each rounded to fp32 once.  Asserted: the mean and the sum of squares are integers below 2^24."""
    D = x.shape[-1]
    mean = x.double().mean(-1, keepdim=True)
    ss = ((x.double() - mean) ** 2).sum(-1, keepdim=True)
    assert bool((mean == mean.round()).all()) and bool((ss == ss.round()).all()) and ss.max().item() < 2 ** 24
    return mean.float(), row_factor(ss.float() / float(D) + eps)


def ln_modulate_chain(x, shift, scale, mean, r, split_row: int = 0, shift2=None, scale2=None) -> torch.Tensor:
    """tfx_ln_modulate on x [B, R, D] with shift / scale bf16 [B, D] and the row statistics mean, r [B, R, 1] fp32, with torch's operators
    and the kernel's rounding points: xn = bf16((x - mean) * r), t = bf16(1 + scale), out = bf16(bf16(xn * t) + shift).  Rows below
    split_row of every sample take (shift2, scale2)."""
    assert shift.dtype == BF and scale.dtype == BF
    xn = ((x.float() - mean) * r).to(BF)
    out = xn * (1 + scale)[:, None, :] + shift[:, None, :]
    if split_row > 0:
        out[:, :split_row] = xn[:, :split_row] * (1 + scale2)[:, None, :] + shift2[:, None, :]
    return out


def cancels(x, gamma, beta, mean, r) -> bool:
    """True when some (x - mean) * r * gamma + beta nearly cancels.  Two steps of r and the rounding of the product move the sum by under
    2^-21 |t gamma|; that has to stay inside a bf16 step (2^-8) of the result, or no tolerance counted in bf16 steps describes what a
    correct kernel may store (a row whose variance is a square integer has a rational-looking r, and k * r * gamma == -beta happens)."""
    tg = (x.float() - mean) * r * gamma.float()
    return bool(((tg + beta.float()).abs() < 2.0 ** -12 * tg.abs()).any())


def layernorm_affine_chain(x, gamma, beta, mean, r, fused: bool = False) -> torch.Tensor:
    """tfx_layernorm: bf16((x - mean) * r * gamma + beta), fp32 and ONE bf16 rounding.  fused: the last multiply-add as one fma (the
    compiler may contract it): t * gamma + beta is exact in fp64 (24 + 8 bits against a dyadic beta), rounded to fp32 once."""
    t = (x.float() - mean) * r
    assert not cancels(x, gamma, beta, mean, r), "t * gamma + beta cancels"
    if fused:
        v = t.double() * gamma.double() + beta.double()
        assert bool(((v - beta.double()) == t.double() * gamma.double()).all())
        return v.float().to(BF)
    return (t * gamma.float() + beta.float()).to(BF)


def groupnorm_stats(x: torch.Tensor, groups: int, eps: float):
    """fp64 (mean, var, rstd) [B, groups] of x [B, HW, C] NHWC.  Asserted: a group's sum and sum of squares are integers below 2^24."""
    B, HW, C = x.shape
    v = x.double().view(B, HW, groups, C // groups).permute(0, 2, 1, 3).reshape(B, groups, -1)
    s, q = v.sum(-1), (v ** 2).sum(-1)
    assert q.max().item() < 2 ** 24 and s.abs().max().item() < 2 ** 24
    mean = s / v.shape[-1]
    var = q / v.shape[-1] - mean ** 2
    return mean, var, 1.0 / torch.sqrt(var.clamp(min=0) + torch.tensor(eps, dtype=torch.float32).double())     # eps as the fp32 number the kernel adds


def silu64(y: torch.Tensor) -> torch.Tensor:
    return y.double() / (1.0 + torch.exp(-y.double()))


def groupnorm_chain(x, gamma, beta, mean, rstd, groups: int, silu: bool, fused: bool = False) -> torch.Tensor:
    """tfx_groupnorm_nhwc on x [B, HW, C] with the statistics mean, rstd fp32 [B, groups]: y = bf16((x - mean) * rstd * gamma + beta),
    fp32 and one rounding (fused: as layernorm_affine_chain), then bf16(silu(y)) from fp64."""
    B, HW, C = x.shape
    cpg = C // groups
    m = mean.float().repeat_interleave(cpg, 1)[:, None, :]
    r = rstd.float().repeat_interleave(cpg, 1)[:, None, :]
    y = layernorm_affine_chain(x, gamma, beta, m, r, fused)
    return silu64(y).float().to(BF) if silu else y


def settled(v64: torch.Tensor, rel: float) -> torch.Tensor:
    """Elements of an fp64 result whose bf16 rounding does not change when the value moves by `rel` of itself either way."""
    return (v64 * (1 - rel)).float().to(BF) == (v64 * (1 + rel)).float().to(BF)


def t5_factor(x: torch.Tensor, eps: float) -> torch.Tensor:
    """r [rows, 1] fp32 of T5LayerNorm as the kernel forms it: rsqrt(sum x^2 / D + eps).  Asserted: the sum is an integer below 2^24."""
    ss = (x.double() ** 2).sum(-1, keepdim=True)
    assert bool((ss == ss.round()).all()) and ss.max().item() < 2 ** 24
    return row_factor(ss.float() / float(x.shape[-1]) + eps)


def t5_rmsnorm_chain(x, w, r) -> torch.Tensor:
    """tfx_rmsnorm: bf16(w * bf16(x * r)), x fp32 or bf16."""
    return w * (x.float() * r).to(BF)


def quick_gelu_chain(a: torch.Tensor) -> torch.Tensor:
    """CLIP's x * sigmoid(1.702 x) on bf16 op by op -- bf16(1.702 x), bf16(sigmoid(.)), bf16(x * .) -- each step from fp64."""
    u = (torch.tensor(1.702, dtype=torch.float32).double() * a.double()).float().to(BF)     # 1.702 as the fp32 constant of the product
    sg = (1.0 / (1.0 + torch.exp(-u.double()))).float().to(BF)
    return (a.double() * sg.double()).float().to(BF)


def euler_chain(v, x, dsigma: float) -> torch.Tensor:
    """FlowMatchEulerDiscreteScheduler.step on bf16 tensors: bf16(f32(x) + bf16(dsigma * v))."""
    return (x.float() + torch.tensor(dsigma, dtype=BF) * v).to(BF)


def amo_chain(v, x, noise, dt: float, a: float, b: float) -> torch.Tensor:
    """StochasticRFOvershotDiscreteScheduler.step on bf16 tensors: bf16((f32(x) + bf16(dt * (-v))) * a + noise * b), a, b, noise fp32."""
    x_over = x.float() + torch.tensor(dt, dtype=BF) * (-v)
    return (x_over * torch.tensor(a, dtype=torch.float32) + noise * torch.tensor(b, dtype=torch.float32)).to(BF)


def softmax_rows64(s: torch.Tensor, scale: float) -> torch.Tensor:
    return torch.softmax(s.double() * float(torch.tensor(scale, dtype=torch.float32)), -1).float().to(BF)


# The caps of tests/test_exact_rows_gpu.py.  Each *_SHARE is the share of the output elements of that file's cases whose stored bits change
# when the row factor moves within what a correct kernel may return; tests/test_exact_inputs_cpu.py measures each and asserts it equal to the
# constant.  The GPU tests compare with ulps=1 and cap = 4 * SHARE (the factor the q / k norm test argues for); a cap of 0 is bit-equality.
#   LayerNorm + modulation, affine LayerNorm, T5 RMSNorm: the argument of the root -- an exact integer sum, one correctly rounded division
#     by D, one correctly rounded + eps -- is the same fp32 number in every summation order, so r = rsqrt(arg) from a root accurate to one
#     step is row_factor(arg) or a neighbour: ONE step either way.
#   GroupNorm: TWO steps.  The kernel multiplies the exact sums by inv_count = fp32(1 / count), a rounded float unless count is a power of
#     two (relative error <= 2^-24 in var, half of it in rstd: up to one step where the mantissa of rstd is near 2), and rsqrtf adds a step
#     of its own.
#   The two one-rounding forms (affine LayerNorm, GroupNorm) also count the elements on which the fused and the unfused evaluation of the
#     final multiply-add differ: the compiler may contract it.
LN_DS = (8, 504, 512, 520, 1544, 3064, 3072)            # 1 chunk | 63 of 64 lanes | one full round | round 1 with one lane | round 3 partly | round 5 short of one lane | all full
LN_ROWS = (1, 3, 4, 5, 37)                              # below, at and above the four rows of a workgroup
LN_OFFSETS = (0, 3)
LN_AMP = 8
LN_SPLIT_DS, LN_SPLIT_ROWS, LN_SPLIT_R = (520, 3072), (0, 1, 5, 37), 37
LNA_DS, LNA_ROWS = (8, 520, 768, 3064), (1, 5, 77)
GN_CASES = [(128, 32, 1), (128, 32, 1023), (128, 32, 1024), (128, 32, 1025), (256, 64, 8193), (512, 32, 300), (64, 4, 2100)]   # (C, groups, HW)
GN_OFFSET_CASE = (128, 32, 1024)                        # count 4096, a power of two: mean = s * inv_count is exact with the offset 3
T5_DS, T5_ROWS = (8, 100, 4096), (1, 5)
LN_SHARE = 0.0
LN_AFFINE_SHARE = 35 / 361880
GN_SHARE = 167 / 5557504
T5_SHARE = 0.0


def ln_case(B: int, R: int, D: int, offset: int) -> dict:
    """One LayerNorm + modulation case of the GPU file: x, the [B, 6 * D] modulation table its shift / scale (and shift2 / scale2) are
    slices of, and the row statistics."""
    seed = shape_seed(B, R, D, offset)
    x = zero_sum_rows((B, R), D, seed, LN_AMP, offset)
    mean, r = layernorm_factor(x, 1e-6)
    return dict(x=x, mod=arbitrary_bf16((B, 6 * D), seed + 1, 0.5), mean=mean, r=r)


def mod_slices(mod: torch.Tensor, D: int):
    """(shift, scale, shift2, scale2): chunks 0, 1, 3, 4 of the six of an AdaLayerNormZero table."""
    return mod[:, :D], mod[:, D:2 * D], mod[:, 3 * D:4 * D], mod[:, 4 * D:5 * D]


def lna_case(rows: int, D: int) -> dict:
    """x rows (offset 3 at 5 rows), dyadic gamma / beta; the first of sixteen seeds whose outputs do not cancel (see cancels)."""
    for attempt in range(16):
        seed = shape_seed(rows, D, 77 + attempt)
        x = zero_sum_rows((rows,), D, seed, LN_AMP, 3 if rows == 5 else 0)
        mean, r = layernorm_factor(x, 1e-5)
        gamma, beta = choice(NORM_WEIGHTS, (D,), seed + 1, signed=True).to(BF), choice(NORM_WEIGHTS, (D,), seed + 2, signed=True).to(BF)
        if not cancels(x, gamma, beta, mean, r):
            return dict(x=x, gamma=gamma, beta=beta, mean=mean, r=r)
    raise AssertionError(f"no seed without a cancelling output at rows {rows} D {D}")


def gn_case(C: int, groups: int, HW: int, B: int = 2) -> dict:
    """x [B, HW, C] zero-sum per (sample, group) (offset 3 at GN_OFFSET_CASE), dyadic gamma / beta, and the fp64 statistics."""
    cpg = C // groups
    for attempt in range(16):
        seed = shape_seed(C, groups, HW, attempt)
        x = zero_sum_groups(B, HW, C, groups, seed, 3 if (C, groups, HW) == GN_OFFSET_CASE else 0)
        mean, var, rstd = groupnorm_stats(x, groups, 1e-6)
        # a group of four values of one magnitude (HW = 1) normalises to +-1 / sqrt(1 + eps / a^2): with |beta| == |gamma| the output would be
        # the rounding residue of gamma - gamma; beta's magnitudes are not gamma's, and a seed that still cancels somewhere is passed over
        gamma, beta = choice(NORM_WEIGHTS, (C,), seed + 11, signed=True).to(BF), choice(NORM_SHIFTS, (C,), seed + 12, signed=True).to(BF)
        if not cancels(x, gamma, beta, mean.float().repeat_interleave(cpg, 1)[:, None, :], rstd.float().repeat_interleave(cpg, 1)[:, None, :]):
            return dict(x=x, gamma=gamma, beta=beta, mean=mean, rstd=rstd)
    raise AssertionError(f"no seed without a cancelling output at C {C} groups {groups} HW {HW}")


def t5_case(rows: int, D: int, f32: bool) -> dict:
    """x integers (|x| <= 60 as fp32, <= 8 as bf16), w arbitrary bf16 near 1."""
    seed = shape_seed(rows, D, int(f32))
    x = zero_sum_rows((rows,), D, seed, 60 if f32 else LN_AMP)
    w = (1 + 0.25 * torch.randn(D, generator=gen(seed + 1))).to(BF)
    return dict(x=x if f32 else x.to(BF), w=w, r=t5_factor(x, 1e-6))


# --------------------------------------------------------------------------------------------------------- the shapes of tests/test_exact_gpu.py
# (tests/test_exact_inputs_cpu.py runs every generator at every one of them: a condition that fails must fail without a GPU)
GEMM_EPI_SHAPES = [(2, 300, 264, 128), (3, 37, 72, 192), (1, 8, 64, 128), (2, 513, 520, 384)]          # (B, M, N, K)
GEMM_WS_BYTES = 64 << 20                                # the workspace of every K-slicing test: the engine's scratch, 256 units of 256 KiB
GEMM_KSLICE_BMN = (1, 300, 520)                         # 6 tiles, ragged both ways (row tiles of 256 and 44 rows, column tiles of 256, 256 and 8)
GEMM_KSLICE = {1024: 2, 1536: 3, 2048: 4, 3072: 6, 4096: 8}                                            # bf16 K: slices at grids 256 and 304
GEMM_KSLICE_KS = tuple(GEMM_KSLICE)                                                                    # (1, 300, 520, K)
# fp8 K: slices.  Every slice count tail_reduce_kernel has a case for, and the production depths 3072, 12288, 15360 (16 .. 120 K-tiles)
GEMM_FP8_KSLICE = {2048: 2, 3072: 3, 4096: 4, 6144: 6, 8192: 8, 12288: 8, 15360: 6}
GEMM_FP8_BATCH2, GEMM_FP8_BATCH2_SLICES = (2, 300, 520, 3072), 3                                       # 12 tiles
# quantize_rows_fp8 (B, rows, K): 256 lanes take 8 values each per round -- quant_rows_fp8_kernel<2> up to K = 4096, <6> up to 12288, <8> up
# to 16384.  4104: the first K of <6>, one lane in its third round | 12288: <6> full | 12296: the first K of <8> | 16384: the limit
QUANT_SHAPES = [(2, 37, 256), (1, 300, 512), (2, 5, 4104), (1, 3, 12288), (1, 3, 12296), (1, 2, 16384)]
QUANT_K_LIMIT = 16384
GEMM_TAIL_SHAPE = (1, 4096, 9216, 1024)
# |lin| <= 71 at K <= 3072, and gate * lin is then a bf16 number for every gate of GATES: epilogue 2's intermediate rounding cannot be
# seen.  At K = 12288 (std 28) a couple of dozen elements of this launch have a |lin| whose product with +-0.75 / +-1.5 needs a ninth bit.
GEMM_ROUNDING_SHAPE = (1, 300, 264, 12288)
QKN_SHARE_ONE_ULP = 0.0     # measured (tests/test_exact_inputs_cpu.py): q / k elements whose bits change when r moves one fp32 step
GEMM_F32_SHAPES = [(1, 300, 520, 128), (2, 1015, 1015, 256)]
GEMM_COLSCALE_SHAPES = [(1, 300, 264, 192), (2, 80, 384, 256)]
GEMM_FP8_SHAPES = [(1, 512, 512, 256), (2, 1000, 3136, 512)]
LORA_MS, LORA_NK, LORA_RS = (80, 1664), (768, 256), (128, 256)
QKN_M, QKN_K, QKN_POS0, QKN_D = 2344, 256, 7, 3072
ATTN_SHAPES = [(1, 1, 1), (2, 3, 8), (1, 2, 33), (1, 1, 64), (1, 1, 65), (2, 2, 96), (1, 3, 300), (2, 2, 1664)]      # (B, H, N)
ATTN_PERSISTENT_SHAPES = [(16, 24, 50), (3, 24, 1100)]
ATTN_STREAMK_SHAPE = (2, 5, 2304)
ATTN_TAIL_SHAPE = (1, 24, 3100)
ATTN_SEQ_LEN_CASES = [((4, 24, 1024), (1024, 777, 257, 64)), ((2, 2, 512), (512, 130))]
ATTN64_NS, ATTN64_HS, ATTN64_MULT = (1, 40, 77, 129, 512), (2, 12), 6.0
# (B, H, W, Cin, Cout, stride, up, pad_lo, with_res): the smallest rows of tests/test_vae_kernels_gpu.py's parametrisations
CONV_CASES = [(2, 12, 20, 64, 64, 1, 1, 1, False), (1, 9, 7, 128, 72, 1, 1, 1, True), (2, 8, 6, 64, 128, 1, 2, 1, False),
              (1, 16, 12, 64, 64, 2, 1, 0, False)]
CONV_NARROW_CASES = [(2, 20, 24, 3, 64), (1, 9, 13, 16, 128)]                                           # (B, H, W, Cin, Cout)
CONV_PAIR_CASES = [(2, 12, 20, 64, 128, False), (1, 9, 14, 128, 128, True)]                             # (B, H, W, Cin, Cout, with_res)


def shape_seed(*shape) -> int:
    s = 17
    for x in shape:
        s = (s * 1000003 + int(x)) % (2 ** 31 - 1)
    return s


def lora_case(M: int, N: int, K: int, R: int, B: int, nseg: int, seed: int, sets: int = 1) -> dict:
    """Operands of tfx_gemm_bf16_lora in the exact regime: x [B, M, K], T [nseg][B, M, R] (one block per segment, its own seed), and per
    weight set W [N, K] | Bm [N, R] with the rows of segment s drawn from that segment's seed.  acc[set][B, M, N] per segment mask is
    taken with lora_acc.  Every operand is ternary-sparse: ONE exact accumulation over K + R."""
    x = ternary((B, M, K), seed + 1)
    T = torch.stack([ternary((B, M, R), seed + 100 + s) for s in range(nseg)])
    W = torch.stack([ternary((N, K), seed + 200 + i) for i in range(sets)])
    Bm = torch.stack([torch.cat([ternary((N // nseg, R), seed + 300 + 10 * i + s) for s in range(nseg)]) for i in range(sets)])
    bias = torch.stack([integers((N,), -8, 8, seed + 400 + i) for i in range(sets)])
    return dict(x=x, T=T, W=W, Bm=Bm, bias=bias, nseg=nseg, seg_cols=N // nseg)


def lora_acc(cs: dict, mask: int, which: int = 0) -> torch.Tensor:
    """x W^T + T_seg Bm^T over the segments of `mask`, fp64 integers [B, M, N], of weight set `which`; asserted <= 256 with the bias."""
    acc = cs["x"].double() @ cs["W"][which].double().T
    sc = cs["seg_cols"]
    for s in range(cs["nseg"]):
        if mask >> s & 1:
            acc[..., s * sc:(s + 1) * sc] += cs["T"][s].double() @ cs["Bm"][which][s * sc:(s + 1) * sc].double().T
    check_accumulators(acc, cs["bias"][which])
    return acc


# --------------------------------------------------------------------------------------------------------- tests/test_exact_layout_gpu.py
# rmsnorm_rope on its own: integer x (the 128 squares sum exactly in any order), four non-dyadic weights, real rotary tables.  That leaves a
# kernel the row factor (one fp32 step of row_factor either way) and the evaluation of y_i * c + (-y_{i+1}) * s: two rounded products, or a
# fused multiply-add with either product inside.  ROPE_SHARE is the share of q / k elements of ALL the cases below whose bits change under
# any of these; tests/test_exact_inputs_cpu.py measures it, the GPU file compares with ulps=1 and cap = 4 * ROPE_SHARE over all cases.
ROPE_HS = (1, 3, 5, 13, 24)         # 2H head rows over four lane groups: two empty | 2 each | 3, 3 (across q/k), 3, 1 | 7, 7, 7, 5 (a second round of six) | 12 each
ROPE_TOKENS = ((1, 1), (2, 5), (1, 37))     # (B, Ntok): one token | a workgroup's four tokens span both samples | ten workgroups, the last with one token
ROPE_AMP = 16
ROPE_SHARE = 14 / 2037248


def rope_ts(Ntok: int):
    """Text-row counts of a case: none | the switch inside a workgroup's four tokens | all (Ntok = 1: the same as 2, run once)."""
    return tuple(sorted({0, 2, Ntok} if Ntok > 1 else {0, 2}))


def rope_tables(B: int, Ntok: int, per_sample: bool):
    """(cos, sin) fp32 [Ntok, 128] (per_sample: [B, Ntok, 128], the samples' tables differ) from the reference's FluxPosEmbed on the ids
    of an image grid: windows of the 8 x 8 latent grid's row-major (0, row, column) ids."""
    from oracle import flux_oracle as fo
    from oracle import pipeline_oracle as po
    ids = po.latent_image_ids(8, 8)
    tabs = [fo.flux_pos_embed(ids[3 + 19 * b:3 + 19 * b + Ntok]) for b in range(B if per_sample else 1)]
    cos, sin = (torch.stack([t[i] for t in tabs]).contiguous() for i in (0, 1))
    assert cos.dtype == torch.float32 and cos.shape[-2:] == (Ntok, 128)
    assert not per_sample or B == 1 or not torch.equal(cos[0], cos[1])
    return (cos, sin) if per_sample else (cos[0], sin[0])


@functools.lru_cache(maxsize=None)
def rope_case(H: int, B: int, Ntok: int, T: int, per_sample: bool) -> dict:
    """x [B, Ntok, 2H, 128] integers in [-16, 16] (head rows: q heads, then k heads), the four weights (wq_img, wk_img, wq_txt, wk_txt),
    the tables, the per-row weight w [B, Ntok, 2H, 128] the kernel is to pick (text below T, k from head row H) and the row factor r."""
    seed = shape_seed(H, B, Ntok, T, int(per_sample))
    x = integers((B, Ntok, 2 * H, 128), -ROPE_AMP, ROPE_AMP, seed)
    ws = tuple((1 + 0.1 * torch.randn(128, generator=gen(seed + 1 + i))).to(BF) for i in range(4))
    assert len({tuple(w.tolist()) for w in ws}) == 4
    cos, sin = rope_tables(B, Ntok, per_sample)
    ss = (x.double() ** 2).sum(-1, keepdim=True)
    assert ss.max().item() <= 2 ** 23 and ss.min().item() > 0
    r = row_factor(ss.float() * (1.0 / 128.0) + 1e-6)           # ss / 128 is exact, so a contracted ss * (1 / 128) + eps is the same number
    return dict(x=x, ws=ws, cos=cos, sin=sin, r=r, w=rope_pick_weights(ws, B, Ntok, H, T))


def rope_pick_weights(ws, B: int, Ntok: int, H: int, T: int) -> torch.Tensor:
    """w [B, Ntok, 2H, 128] from ws = (wq_img, wk_img, wq_txt, wk_txt): rows n < T take the text pair, head rows >= H the k weight."""
    txt = (torch.arange(Ntok) < T)[None, :, None, None]
    is_k = (torch.arange(2 * H) >= H)[None, None, :, None]
    img_w = torch.where(is_k, ws[1].float(), ws[0].float())
    txt_w = torch.where(is_k, ws[3].float(), ws[2].float())
    return torch.where(txt, txt_w, img_w).expand(B, Ntok, 2 * H, 128).to(BF)


def _exact_sum(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """a + b of fp64 tensors, asserted exact in fp64 (so that rounding it to fp32 rounds the true sum once)."""
    s = a + b
    assert bool(((s - a) == b).all()) and bool(((s - b) == a).all()), "the fp64 sum of the two terms must be exact"
    return s


def _mul_add(a, b, c, d, order: int) -> torch.Tensor:
    """fp32 a * b + c * d of bf16-valued a, c and fp32 b, d (fp64 tensors; every product is exact in fp64).  order 0: both products
    rounded to fp32, then added; 1: fma(a, b, fp32(c * d)); 2: fma(c, d, fp32(a * b))."""
    p, q = a * b, c * d
    if order == 0:
        return p.float() + q.float()
    if order == 1:
        return _exact_sum(p, q.float().double()).float()
    return _exact_sum(q, p.float().double()).float()


def rms_rope_chain(x, w, cos, sin, r, order: int = 0) -> torch.Tensor:
    """tfx_rmsnorm_rope on head rows x [B, Ntok, R, 128] with the per-row weight w (bf16, same shape), tables [Ntok, 128] or [B, Ntok, 128]
    as the kernel reads them and the row factor r [B, Ntok, R, 1]: y = bf16(bf16(x * r) * w), then per pair (i, i + 1)
    o_i = y_i * cos_i + (-y_{i+1}) * sin_i, o_{i+1} = y_{i+1} * cos_{i+1} + y_i * sin_{i+1} in fp32, rounded to bf16 once.  order: how the
    fp32 expression is evaluated, see _mul_add (a compiler may contract either product into the add)."""
    assert w.dtype == BF and cos.dtype == torch.float32 and r.dtype == torch.float32
    y = ((x.float() * r).to(BF).float() * w.float()).to(BF).double()
    c, s = (t.double()[None, :, None, :] if t.dim() == 2 else t.double()[:, :, None, :] for t in (cos, sin))
    y0, y1 = y[..., 0::2], y[..., 1::2]
    o0 = _mul_add(y0, c[..., 0::2], -y1, s[..., 0::2], order)
    o1 = _mul_add(y1, c[..., 1::2], y0, s[..., 1::2], order)
    return torch.stack([o0, o1], -1).flatten(-2).to(BF)


def rope_cases():
    """Every (H, B, Ntok, T, per_sample) of the GPU file (each is run in both column orders: the same arithmetic)."""
    return [(H, B, N, T, ps) for H in ROPE_HS for B, N in ROPE_TOKENS for T in rope_ts(N) for ps in ((False, True) if B > 1 else (False,))]


# --- timestep embedding
TIMESTEPS = (0.0, 1e-3, 0.5, 1.0, 17.25, 999.0, 1000.0)


def timestep_window(t: torch.Tensor):
    """(lo, hi) bf16 [n, 256] a correct tfx_timestep_embedding row lies between, elementwise: e_j the reference's fp32 exponent (the
    operations of oracle.flux_oracle.timestep_embedding in their order), f_j = fp32(exp64(e_j)), a = fp32(t * f_j), want = cos64(a) |
    sin64(a), lo / hi = bf16(want -+ delta) with delta = |a| * 2^-20 + 2^-22: sixteen fp32 steps of the frequency, where a working expf,
    the product and sinf / cosf need one or two."""
    half = 128
    e = -math.log(10000) * torch.arange(0, half, dtype=torch.float32) / half
    f = torch.exp(e.double()).float()
    a = (t.float()[:, None] * f[None, :]).double()
    want = torch.cat([torch.cos(a), torch.sin(a)], -1)
    delta = torch.cat([a.abs(), a.abs()], -1) * 2.0 ** -20 + 2.0 ** -22
    return (want - delta).float().to(BF), (want + delta).float().to(BF)


def assert_in_window(got: torch.Tensor, lo: torch.Tensor, hi: torch.Tensor, what: str) -> None:
    got = got.detach().cpu()
    assert got.dtype == BF and got.shape == lo.shape
    bad = ~((got.float() >= lo.float()) & (got.float() <= hi.float()))              # a NaN is outside
    if bad.any():
        i, j = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.numel()} elements outside their window; first (row {i}, col {j}): got "
                             f"{got[i, j].item()!r}, window [{lo[i, j].item()!r}, {hi[i, j].item()!r}]")


# --- sample_pack
SAMPLE_PACK_CASES = ((1, 2, 2, 2), (2, 6, 10, 16))                                       # (B, h, w, L)
SAMPLE_PACK_LOGVARS = (-40.0, -30.0, 20.0, 25.0)


def sample_pack_case(B: int, h: int, w: int, L: int) -> dict:
    """mean, logvar bf16 [B, L, h, w] (NCHW; logvar holds the four values around the clamp and ordinary ones), eps bf16, and an fp32 eps
    that bf16 does not hold."""
    seed = shape_seed(B, h, w, L)
    mean, eps = arbitrary_bf16((B, L, h, w), seed), arbitrary_bf16((B, L, h, w), seed + 1)
    logvar = (torch.randn(B, L, h, w, generator=gen(seed + 2)) * 2.0 - 1.0).to(BF)
    flat = logvar.view(-1)
    flat[torch.randperm(flat.numel(), generator=gen(seed + 3))[:4]] = torch.tensor(SAMPLE_PACK_LOGVARS, dtype=BF)
    eps32 = torch.randn(B, L, h, w, generator=gen(seed + 4))
    assert not torch.equal(eps32.to(BF).float(), eps32)
    return dict(mean=mean, logvar=logvar, eps=eps, eps32=eps32)


def sample_pack_std64(logvar: torch.Tensor) -> torch.Tensor:
    """exp64(bf16(0.5 * clamp(logvar, -30, 20))): the one transcendental of the chain (0.5 * lv is exact)."""
    return torch.exp((0.5 * torch.clamp(logvar, -30.0, 20.0)).double())


def sample_pack_chain(mean, std, eps, shift: float, scale: float) -> torch.Tensor:
    """[B, S, 4L] bf16 = pack(bf16(bf16(z - shift) * scale)), z = bf16(mean + bf16(std * eps)) with torch's bf16 operators (eps None: the
    mode, z = mean); the two scalars as the reference's device kernels apply them (dev_scalar of tests/test_imageops_gpu.py)."""
    from oracle import pipeline_oracle as po
    from tests.test_imageops_gpu import dev_scalar
    assert mean.dtype == BF and (eps is None or (std.dtype == BF and eps.dtype == BF))
    z = mean if eps is None else mean + std * eps
    return po.pack_latents(dev_scalar(dev_scalar(z, "sub", shift), "mul", scale))


def bf16_neighbour(t: torch.Tensor, d: int) -> torch.Tensor:
    """The bf16 value d steps away in magnitude (positive finite t)."""
    return (t.contiguous().view(torch.int16) + d).view(BF)
