r"""Input families, float64 references, the error bound and the launch-rule predictors for the normalisation kernels' tests
(test_norm_cases_host.py checks all of it on the CPU, test_gpu_norm.py runs the kernels).  Plain module, no test in it; it
imports nothing from azula_amd.

The older norm tests draw ``randn * 1.7 + 0.9``: mean / std is O(1), so a naive E[x^2] - E[x]^2, a Chan merge without its cross
term or a missing pivot all pass their absolute 2e-5.  The families here are chosen for what the algorithm of csrc/norm.hip finds
hard (mean / std up to 1e5, variance exactly 0 or far below eps, chunk means far apart, a spike on the pivot positions).

The bound.  The apply kernel computes x S + T with S = rstd w (1 + a), T = (b - mean rstd w)(1 + a) + sh: its forward error scales
with the cancelling terms, not with |y|.  Per element, before the activation, with the reference's float64 statistics,

    cond    = (|x| + |mean|) rstd |w (1 + a)| + |b (1 + a)| + |sh|
    allowed = M 2^-24 cond            (x 1.1 after SiLU, its Lipschitz constant; pooled outputs: the window's mean of allowed)

Row norms use the same cond with b = 0.  2-byte outputs add half an ulp of the output type (2^-9 |y| bf16, 2^-12 |y| f16) and their
reference reads the rounded input (``half_ulp``: the exact half spacing at the reference value, which is 2^-9 |y| only at the top of
a binade and 2^-8 |y| at its bottom).  M is not chosen: ``M_REF`` is the largest ratio |restatement - ref| / (2^-24 cond) of the fp32
restatement below (two-pass fp32 statistics, S and T in fp32, x S + T without a fused multiply-add; for the row norms
(x - mean) rstd w (1 + a) + sh) over every case of the GPU test, measured on the CPU; the host test re-derives it.  The device
bound is M = 4 M_REF: the kernels' statistics come from another reduction order (pivoted per-thread sums, Chan merges, chunked
finalize) than the restatement's, and their mean and rstd each add at most one more term of the size M_REF already measures; the
factor 4 is those two terms, the restatement's own, and one of slack."""

from __future__ import annotations

from collections import namedtuple

import torch
import torch.nn.functional as F

EPS = 1e-5
U32 = 2.0 ** -24
HALF_ULP = {torch.bfloat16: 2.0 ** -9, torch.float16: 2.0 ** -12}  # half an ulp relative to |y|, at the top of a binade (half_ulp)
# Largest |fp32 restatement - ref| / (2^-24 cond) over GN_CASES and ROW_CASES: every case of test_gpu_norm.py whose input the
# test controls (the producer cases normalise what a convolution stored).  Measured 90.32, rounded up; the host test re-derives it
# and asserts measured <= M_REF <= 1.25 measured.  It is this large because cond has no floor where mean, bias and shift are all
# ~0: the zero-mean families without affine / modulation hold elements with |x| + |mean| ~ 1e-4 std, at which the rounding of
# the mean alone (~2^-24 std) is tens of 2^-24 cond.  The families with an offset sit at 1 - 8.
M_REF = 91.0
M_DEVICE = 4.0 * M_REF

FAMILIES = ("unit", "offset10", "offset1e2", "offset1e3", "offset1e4", "tight", "scaled1e4", "scaled1e-3", "constant_group",
            "channel_steps", "ramp", "spike", "pivot_spike")
LARGE_FAMILIES = ("offset1e3", "ramp", "pivot_spike", "constant_group")
ROW_FAMILIES = ("unit", "offset1e3", "tight", "scaled1e-3", "constant_group", "zero_row", "spike")
HALF_GN_FAMILIES = ("offset1e2", "constant_group", "ramp")
CONSTANTS = (3.25, 1000.1)
SPIKE = 1e4


# ------------------------------------------------------------------------------------------------ launch rules, restated
def pad4(c):
    return (c + 3) // 4 * 4


def gn_nchunks(HW, cs):
    r"""Builder.group_norm: about 64 KB of x per statistics workgroup, at most 512 chunks."""
    return int(min(512, max(1, (HW * cs * 4) // 65536)))


def gn_stats_path(C, cs, groups):
    r"""az_groupnorm_stats_f32: ("vector", qs) or ("generic", 0).  qs = float4 chunks per slice: the largest divisor of cs / 4,
    at most 256, that holds whole groups; a padded stride runs as one slice."""
    Cg, q, qs = C // groups, cs // 4, 0
    if Cg % 4 == 0 and C == cs:
        for d in range(min(q, 256), Cg // 4 - 1, -1):
            if d >= 1 and q % d == 0 and (4 * d) % Cg == 0:
                qs = d
                break
    elif Cg % 4 == 0 and q <= 256:
        qs = q
    fast = qs >= 32 or (qs > 0 and qs == q)
    return ("vector", qs) if fast else ("generic", 0)


def gn_chunk_ranges(HW, nchunks):
    r"""[p0, p1) of every chunk (p1 <= p0: an empty chunk)."""
    ppc = (HW + nchunks - 1) // nchunks
    return [(k * ppc, min(k * ppc + ppc, HW)) for k in range(nchunks)]


def gn_chunks_ragged_or_empty(HW, nchunks):
    r"""(some chunk shorter than the others, some chunk empty)."""
    lens = [max(0, p1 - p0) for p0, p1 in gn_chunk_ranges(HW, nchunks)]
    return min(lens) < max(lens), min(lens) == 0


def gn_pivot_pixels(HW, C, cs, groups):
    r"""The pixels from which a statistics thread takes its pivot (its first element): the first pixel lanes of every chunk --
    256 / qs lanes in the vector kernel, ceil(256 / Cg) pixels in the generic one."""
    path, qs = gn_stats_path(C, cs, groups)
    lanes = 256 // qs if path == "vector" else -(-256 // (C // groups))
    px = set()
    for p0, p1 in gn_chunk_ranges(HW, gn_nchunks(HW, cs)):
        px.update(range(p0, min(p0 + lanes, p1)))
    return sorted(px)


def finalize_items(nchunks, quads_per_group=0):
    r"""gn_finalize_kernel: partials per (sample, group) -- pixel chunks of the separate pass, or chunks x the group's channel
    quads of the moments a convolution left."""
    return nchunks * quads_per_group if quads_per_group > 0 else nchunks


def finalize_branch(items):
    return "le64" if items <= 64 else ("le256" if items <= 256 else "gt256")


def fused_chunks(kind, H, W, cout=0):
    r"""Partials per image of the producers: the F(2x2) / piece-form Winograd epilogue (64-tile blocks), the stem (8 x 32 pixel
    tiles), the split-K combine (Builder.conv's rule)."""
    if kind == "wino":
        return ((H // 2) * (W // 2)) // 64
    if kind == "stem":
        return ((H + 7) // 8) * ((W + 31) // 32)
    hw = H * W
    cpix = 2 * max(1, 256 // (cout // 4))
    chunks = max(1, min(128, (hw + cpix - 1) // cpix))
    while (hw + chunks - 1) // chunks * (chunks - 1) >= hw:
        chunks -= 1
    return chunks


def rownorm_path(C, cs, aligned=True):
    r"""az_rownorm_mod_f32: "register" (C % 4 == 0, C == cs, C <= 2048, 16-byte aligned weight / modulation rows), else
    "loop_vector" (C % 4 == 0) or "scalar"."""
    if C % 4 == 0 and C == cs and C <= 2048 and aligned:
        return "register"
    return "loop_vector" if C % 4 == 0 else "scalar"


def rownorm_waves(rows):
    r"""One wave per row, four per workgroup, at most 4096 workgroups: rows beyond 16384 go round the grid-stride loop."""
    return 4 * min(4096, (rows + 3) // 4)


def rownorm_h16_ok(C, cs, bstride=0):
    r"""az_rownorm_mod_h16 takes the row (else AZ_E_UNSUPPORTED): whole 8-value loads, no pad, at most 8 per lane."""
    return C % 8 == 0 and C == cs and C <= 4096 and bstride % 4 == 0


# ------------------------------------------------------------------------------------------------ input families
def family(name, B, C, HW, groups, seed=0, pivots=()):
    r"""(B, C, HW) float32.  A normalisation unit is a (sample, group); a row norm passes (rows, C, 1) with one group."""
    g = torch.Generator().manual_seed(1000 * seed + FAMILY_SEED[name])
    x = torch.randn(B, C, HW, generator=g)
    Cg = C // groups
    if name.startswith("offset"):
        x += float(name[6:])
    elif name == "tight":
        x = 1e-2 * x + 1e3
    elif name.startswith("scaled"):
        x *= float(name[6:])
    elif name == "constant_group":
        xv = x.view(B, groups, Cg, HW)
        n = B * groups
        for i, cval in zip((n // 3, n - 1) if n > 1 else (0,), CONSTANTS):
            xv[i // groups, i % groups] = cval
    elif name == "zero_row":
        x.zero_()
    elif name == "channel_steps":
        x += 10.0 * torch.arange(C, dtype=torch.float32)[None, :, None]
    elif name == "ramp":
        x += torch.linspace(0.0, 200.0, HW)[None, None, :]
    elif name == "spike":
        xv = x.view(B, groups, Cg * HW)
        idx = torch.randint(0, Cg * HW, (B, groups, 1), generator=g)
        # (channels of a group are contiguous along C: (B, groups, Cg, HW) flattens to (B, groups, Cg * HW))
        xv.scatter_(2, idx, SPIKE)
    elif name == "pivot_spike":
        x[:, :, list(pivots) if len(pivots) else [0]] = SPIKE
    elif name != "unit":
        raise ValueError(name)
    return x.contiguous()


FAMILY_SEED = {n: i + 1 for i, n in enumerate(FAMILIES + ("zero_row",))}


def round_to(x, dtype):
    return x if dtype is None else x.to(dtype).float()


# ------------------------------------------------------------------------------------------------ references (float64)
def _pool(t, H, W, pool):
    r"""(B, C, HW) -> pooled (B, C, HW'): 1 = 2 x 2 average, 2 = 1 x 2 (along the width)."""
    if not pool:
        return t
    B, C, _ = t.shape
    k = (2, 2) if pool == 1 else (1, 2)
    return F.avg_pool2d(t.reshape(B, C, H, W), k, k).reshape(B, C, -1)


def _chan(v, B, C, dtype, default):
    if v is None:
        return torch.full((1, C, 1), default, dtype=dtype)
    return v.to(dtype).reshape(-1, C, 1)


def groupnorm_ref(x, groups, H, W, weight=None, bias=None, scale=None, shift=None, act=0, pool=0, eps=EPS):
    r"""x (B, C, HW) -> (y, unit) in float64: y = pool(act((GN(x) w + b)(1 + a) + sh)) with the biased variance, and ``unit`` =
    2^-24 cond (x 1.1 under SiLU, averaged over the pooling window): the bound is M x unit."""
    B, C, HW = x.shape
    xd = x.double()
    xg = xd.reshape(B, groups, -1)
    mean = xg.mean(-1, keepdim=True)
    var = (xg - mean).pow(2).mean(-1, keepdim=True)
    rstd = torch.rsqrt(var + eps)
    Cg = C // groups
    mean_c, rstd_c = (t.expand(B, groups, Cg).reshape(B, C, 1) for t in (mean, rstd))
    w, b = _chan(weight, B, C, torch.float64, 1.0), _chan(bias, B, C, torch.float64, 0.0)
    a1, sh = 1.0 + _chan(scale, B, C, torch.float64, 0.0), _chan(shift, B, C, torch.float64, 0.0)
    y = ((xd - mean_c) * rstd_c * w + b) * a1 + sh
    cond = (xd.abs() + mean_c.abs()) * rstd_c * (w * a1).abs() + (b * a1).abs() + sh.abs()
    unit = U32 * cond
    if act == 1:
        y, unit = F.silu(y), 1.1 * unit
    return _pool(y, H, W, pool), _pool(unit, H, W, pool)


def rownorm_ref(x, kind, weight=None, scale=None, shift=None, rows_per_batch=None, eps=EPS):
    r"""x (rows, C); scale / shift (B, C), sample b = row // rows_per_batch.  kind 0: LayerNorm with the unbiased variance
    (oracle/nets.py: layer_norm_unbiased), kind 1: RMSNorm (rms_norm), then w, (1 + a), sh.  -> (y, unit) in float64."""
    rows, C = x.shape
    xd = x.double()
    if kind == 0:
        mean = xd.mean(-1, keepdim=True)
        rstd = torch.rsqrt((xd - mean).pow(2).sum(-1, keepdim=True) / (C - 1) + eps)
    else:
        mean = torch.zeros(rows, 1, dtype=torch.float64)
        rstd = torch.rsqrt(xd.pow(2).mean(-1, keepdim=True) + eps)
    w = torch.ones(1, C, dtype=torch.float64) if weight is None else weight.double()[None]
    bidx = torch.arange(rows) // (rows_per_batch or rows)
    a1 = 1.0 if scale is None else 1.0 + scale.double()[bidx]
    sh = 0.0 if shift is None else shift.double()[bidx]
    y = (xd - mean) * rstd * w * a1 + sh
    cond = (xd.abs() + mean.abs()) * rstd * (w * a1).abs() + (sh.abs() if shift is not None else 0.0)
    return y, U32 * cond


def half_ulp(ref, dtype):
    r"""Half the spacing of ``dtype`` at ``ref``: 2^(floor(log2 |ref|) - 8) for bfloat16 (8 significand bits), - 11 for IEEE half
    (11 bits, exponents from -14).  Between 2^-9 |ref| and 2^-8 |ref| (2^-12 .. 2^-11): round-to-nearest of the exact result
    already errs by this much, so nothing smaller can be asked of a kernel that stores the type."""
    e = torch.frexp(ref.abs())[1].double() - 1.0
    if dtype == torch.float16:
        e = e.clamp_min(-14.0)
    h = torch.exp2(e - (8.0 if dtype == torch.bfloat16 else 11.0))
    return torch.where(ref == 0, torch.zeros_like(h), h)


def worst_ratio(got, ref, unit, out_dtype=None):
    r"""max over elements of (|got - ref| - half an ulp of a 2-byte output) / unit -- to be compared with M; and max |got - ref|."""
    err = (got.double() - ref).abs()
    slack = half_ulp(ref, out_dtype) if out_dtype is not None else 0.0
    ratio = ((err - slack).clamp_min(0.0) / unit.clamp_min(1e-300))
    return ratio.max().item(), err.max().item()


# ------------------------------------------------------------------------------------------------ fp32 restatements
def _mul_add(x, S, T):
    return x * S + T  # (torch: two roundings, no fused multiply-add)


def _tree_sum(x):
    r"""Sum over the last axis as a balanced binary tree of elementwise fp32 additions: the same bits on every machine and
    thread count (torch.sum's order follows the vector width and the thread pool), so that M_REF can be re-derived."""
    n = x.shape[-1]
    p = 1 << max(0, (n - 1).bit_length())
    if p != n:
        x = F.pad(x, (0, p - n))
    while p > 1:
        p //= 2
        x = x[..., :p] + x[..., p:]
    return x


def groupnorm_fp32(x, groups, H, W, weight=None, bias=None, scale=None, shift=None, act=0, pool=0, eps=EPS, fault=None, nchunks=8):
    r"""The operation in the kernels' documented form, in fp32 on the CPU: two-pass statistics, S and T formed in fp32, x S + T.
    ``fault`` plants an error the bound must catch: "naive" = E[x^2] - E[x]^2, "no_cross" = per-chunk (n, mean, M2) merged
    without the n d^2 term (``nchunks`` pixel chunks)."""
    B, C, HW = x.shape
    Cg = C // groups
    xg = x.reshape(B, groups, Cg, HW)
    if fault == "naive":
        mean = xg.mean((2, 3), keepdim=True)
        var = (xg * xg).mean((2, 3), keepdim=True) - mean * mean
        var = var.clamp_min(0.0)
    elif fault == "no_cross":
        parts = torch.tensor_split(xg, min(nchunks, HW), dim=3)
        n = torch.tensor([p.shape[2] * p.shape[3] for p in parts], dtype=torch.float32)
        means = torch.stack([p.mean((2, 3)) for p in parts], -1)  # (B, groups, chunks)
        m2 = torch.stack([(p - p.mean((2, 3), keepdim=True)).pow(2).sum((2, 3)) for p in parts], -1)
        mean = ((means * n).sum(-1) / n.sum())[..., None, None]
        var = (m2.sum(-1) / n.sum())[..., None, None]
    else:
        n = float(Cg * HW)
        mean = (_tree_sum(xg.reshape(B, groups, -1)) / n)[..., None]
        var = (_tree_sum((xg - mean).pow(2).reshape(B, groups, -1)) / n)[..., None]
    rstd = torch.rsqrt(var + eps)
    mean_c, rstd_c = (t.expand(B, groups, Cg, 1).reshape(B, C, 1) for t in (mean, rstd))
    w, b = _chan(weight, B, C, torch.float32, 1.0), _chan(bias, B, C, torch.float32, 0.0)
    a1, sh = 1.0 + _chan(scale, B, C, torch.float32, 0.0), _chan(shift, B, C, torch.float32, 0.0)
    S = rstd_c * w * a1
    T = (b - mean_c * rstd_c * w) * a1 + sh
    y = _mul_add(x, S, T)
    if act == 1:
        y = F.silu(y)
    return _pool(y, H, W, pool)


def groupnorm_torch_fp32(x, groups, H, W, weight=None, bias=None, scale=None, shift=None, act=0, pool=0, eps=EPS):
    r"""torch.nn.functional.group_norm in fp32, then the modulation: the implementation the old tests took as reference."""
    B, C, HW = x.shape
    y = F.group_norm(x, groups, weight, bias, eps)
    if scale is not None:
        y = y * (1.0 + scale.reshape(B, C, 1)) + shift.reshape(B, C, 1)
    if act == 1:
        y = F.silu(y)
    return _pool(y, H, W, pool)


def rownorm_fp32(x, kind, weight=None, scale=None, shift=None, rows_per_batch=None, eps=EPS, fault=None):
    r"""(x - mean) rstd w (1 + a) + sh in fp32, two-pass variance.  ``fault`` "biased": LayerNorm dividing by C."""
    rows, C = x.shape
    if kind == 0:
        mean = _tree_sum(x) / C
        rstd = torch.rsqrt(_tree_sum((x - mean).pow(2)) / (C if fault == "biased" else C - 1) + eps)
    else:
        mean = torch.zeros(rows, 1)
        rstd = torch.rsqrt(_tree_sum(x * x) / C + eps)
    y = (x - mean) * rstd
    if weight is not None:
        y = y * weight[None]
    bidx = torch.arange(rows) // (rows_per_batch or rows)
    if scale is not None:
        y = y * (1.0 + scale[bidx])
    if shift is not None:
        y = y + shift[bidx]
    return y


# ------------------------------------------------------------------------------------------------ the GPU test's case lists
GNCase = namedtuple("GNCase", "family B C H W groups cs c1 affine mod act pool half")
RowCase = namedtuple("RowCase", "family kind B rpb C cs weight mod half")  # mod: 0 none, 1 aligned, 2 misaligned (scale_off odd)

SMALL_SHAPES = [  # (B, C, H, W, groups, cs)
    (2, 32, 16, 16, 8, 32),
    (1, 12, 9, 7, 3, 16),       # vector statistics on a padded stride (one slice; the pad quad is not live)
    (1, 10, 9, 7, 2, 12),       # generic statistics (groups of 5 channels), padded
    (1, 1048, 4, 4, 131, 1048),  # generic statistics: groups of 8 whose widest legal slice is 2 quads of 262
    (2, 768, 16, 16, 32, 768),  # 192-quad slices
    (1, 1280, 8, 8, 32, 1280),  # 160-quad slices
    (1, 2048, 8, 8, 8, 2048),   # groups of 256 channels: the finalize kernel's tail loop
]
LARGE_SHAPES = [
    (1, 64, 200, 200, 32, 64),    # 156 chunks of 257 pixels, the last ragged
    (1, 64, 256, 256, 32, 64),    # 256 chunks
    (1, 128, 256, 256, 32, 128),  # 512 chunks: the finalize kernel's loop from item 256 on
    (1, 128, 160, 161, 32, 128),  # 201 chunks of 129 pixels: the last one empty, the one before ragged
]
OPTIONS = [(0, 1, 1), (1, 1, 1), (1, 0, 0), (0, 0, 0)]  # (affine, modulation, SiLU)


def _gn_cases():
    cases, i = [], 0
    for shape in SMALL_SHAPES:
        for fam in FAMILIES:
            cases.append(GNCase(fam, *shape, 0, *OPTIONS[i % 4], 0, None))
            i += 1
    for shape in LARGE_SHAPES:
        for fam in LARGE_FAMILIES:
            cases.append(GNCase(fam, *shape, 0, *OPTIONS[i % 4], 0, None))
            i += 1
    for fam in FAMILIES:  # two sources: [x | x1] read in place
        cases.append(GNCase(fam, 2, 768, 8, 8, 32, 768, 256, *OPTIONS[i % 4], 0, None))
        i += 1
    for fam in LARGE_FAMILIES:
        cases.append(GNCase(fam, 1, 128, 128, 128, 8, 128, 64, *OPTIONS[i % 4], 0, None))
        i += 1
    for pool in (1, 2):  # pooled apply kernels, with and without a second source and SiLU
        for c1 in (0, 32):
            for act in (0, 1):
                for fam in ("offset1e2", "ramp"):
                    cases.append(GNCase(fam, 2, 64 + c1, 16, 16, 8, 64 + c1, c1, 1, 1, act, pool, None))
    for half in (torch.bfloat16, torch.float16):  # the 2-byte statistics / apply passes
        for fam in HALF_GN_FAMILIES:
            cases.append(GNCase(fam, 2, 64, 12, 16, 8, 64, 0, 1, 1, 1, 0, half))
            cases.append(GNCase(fam, 2, 96, 12, 16, 8, 96, 32, 1, 0, 0, 1, half))
    return cases


ROW_WIDTHS = (4, 5, 252, 256, 260, 1000, 1024, 2048, 2052, 4096, 4099)
ROW_WIDTHS_HALF = (8, 200, 768, 4096)


def _row_cases():
    cases, i = [], 0
    for kind in (0, 1):
        for C in ROW_WIDTHS:
            for fam in ROW_FAMILIES:
                weight, mod = (i % 2, (i // 2) % 3)
                cases.append(RowCase(fam, kind, 2, 15, C, pad4(C), weight, mod, None))
                i += 1
        for mod in (1, 2):  # the register form and, with misaligned modulation rows, the looping vector form at one width
            for fam in ("offset1e3", "spike"):
                cases.append(RowCase(fam, kind, 2, 15, 1024, 1024, 1, mod, None))
        for fam in ("unit", "offset1e3", "constant_group"):  # 18000 rows: the grid-stride loop, samples change inside a wave's stride
            cases.append(RowCase(fam, kind, 3, 6000, 64, 64, 1, 1, None))
        for half in (torch.bfloat16, torch.float16):
            for C in ROW_WIDTHS_HALF:
                for fam in ROW_FAMILIES:
                    cases.append(RowCase(fam, kind, 2, 15, C, C, i % 2, (i // 2) % 2, half))
                    i += 1
            cases.append(RowCase("offset1e3", kind, 3, 6000, 64, 64, 1, 1, half))
    return cases


GN_CASES = _gn_cases()
ROW_CASES = _row_cases()


def gn_inputs(c):
    r"""-> dict(x (B, C, HW) fp32 (rounded to ``half``), weight, bias, scale, shift) of a GNCase.  ``C`` counts both sources:
    the second holds the last ``c1`` channels."""
    HW = c.H * c.W
    pivots = gn_pivot_pixels(HW, c.C, c.cs, c.groups) if c.family == "pivot_spike" else ()
    seed = (c.C * 31 + c.H) % 997
    x = round_to(family(c.family, c.B, c.C, HW, c.groups, seed, pivots), c.half)
    g = torch.Generator().manual_seed(seed + 7)
    w, b = (1.0 + 0.5 * torch.randn(c.C, generator=g), torch.randn(c.C, generator=g)) if c.affine else (None, None)
    a, sh = (0.5 * torch.randn(c.B, c.C, generator=g), torch.randn(c.B, c.C, generator=g)) if c.mod else (None, None)
    return dict(x=x, weight=w, bias=b, scale=a, shift=sh)


def gn_kwargs(c, inp):
    return dict(groups=c.groups, H=c.H, W=c.W, weight=inp["weight"], bias=inp["bias"], scale=inp["scale"], shift=inp["shift"],
                act=c.act, pool=c.pool)


def row_inputs(c):
    rows = c.B * c.rpb
    seed = (c.C * 17 + c.kind) % 991
    x = round_to(family(c.family, rows, c.C, 1, 1, seed).reshape(rows, c.C), c.half)
    g = torch.Generator().manual_seed(seed + 3)
    w = 1.0 + 0.5 * torch.randn(c.C, generator=g) if c.weight else None
    a, sh = (0.5 * torch.randn(c.B, c.C, generator=g), torch.randn(c.B, c.C, generator=g)) if c.mod else (None, None)
    return dict(x=x, weight=w, scale=a, shift=sh)


def case_id(c):
    return "-".join(str(v).replace("torch.", "") for v in c)
