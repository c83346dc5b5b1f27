r"""Data, element counts and fp64 references of the nonlinear-operator tests, shared by the host and the GPU file.  Test
infrastructure: nothing here imports the package except :func:`trip_floats`, which asks the built library for a constant."""

import ctypes as C
import functools
import math

import torch

F32, F64 = torch.float32, torch.float64
U = 2.0**-24  # the unit roundoff of fp32

SCALES = (-60, 0, 60)  # the exact data at 2^k
COUNTS = (1, 3, 4, 5, 1023, 1024, 1025)  # floats per sample: a partial item, the scalar tail, whole items, either side of a block
BATCHES = (1, 3)
GUARD = 64  # guard words before, between and behind strided destinations

# (H, W), pad = int or (top, bottom, left, right): widths that are no multiple of 4 and one case of the 16-byte form
PAD_CASES = [((5, 7), (1, 2, 0, 1)), ((5, 7), (0, 0, 3, 0)), ((5, 7), (0, 0, 0, 0)), ((8, 8), 4)]
PAD_PLANES = (2, 3)  # (B, C)


def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------------------------ exact
@functools.lru_cache(maxsize=None)
def pythagorean_pairs() -> torch.Tensor:
    r"""Every integer pair 0 < p < q with p^2 + q^2 = h^2 and h < 4096, as an int64 (n, 3) tensor of (p, q, h).  h^2 < 2^24, so
    p^2, q^2 and their sum are exact fp32 numbers."""
    rows = []
    for q in range(2, 4096):
        p = torch.arange(1, q, dtype=torch.int64)
        h2 = p * p + q * q
        h = h2.double().sqrt().round().long()  # (h2 < 2^25: the fp64 root is within 1e-9 of an integer root)
        keep = (h * h == h2) & (h < 4096)
        rows.append(torch.stack([p[keep], torch.full_like(p[keep], q), h[keep]], dim=1))
    return torch.cat(rows)


@functools.lru_cache(maxsize=None)
def exact_data():
    r"""(re, im, hyp) fp32 vectors on which ``|z|`` is exact: every Pythagorean pair at the scales 2^k, k in SCALES, in both orders
    and the four sign combinations in turn, then pairs with a zero part (|z| is the other part) and z = 0 with both signs."""
    t = pythagorean_pairs().double()
    p, q, h = t[:, 0], t[:, 1], t[:, 2]
    re, im, hyp = [], [], []
    for k in SCALES:
        s = 2.0**k
        idx = torch.arange(p.numel())
        sr = torch.where(idx % 2 == 0, 1.0, -1.0).double()
        si = torch.where(idx // 2 % 2 == 0, 1.0, -1.0).double()
        re += [sr * p * s, si * q * s]
        im += [si * q * s, sr * p * s]
        hyp += [h * s, h * s]
        edge = torch.tensor([0.0, -0.0, 3.0, -3.0, 0.0, -0.0, 4095.0], dtype=F64) * s
        other = torch.tensor([0.0, 0.0, 0.0, -0.0, 5.0, -5.0, -0.0], dtype=F64) * s
        re += [edge, other]
        im += [other, edge]
        hyp += [(edge.abs() + other.abs())] * 2
    re, im, hyp = (torch.cat(v).to(F32) for v in (re, im, hyp))
    return re, im, hyp


def emulate_cmag(re: torch.Tensor, im: torch.Tensor) -> torch.Tensor:
    r"""The arithmetic of ``az_op_cmag_f32`` restated on the CPU for fp32 vectors: the part of larger magnitude scaled into
    [0.5, 1), the smaller by the same power of two, ``sqrt(fma(a, a, b b))`` with ``b b`` rounded to fp32 on its own, scaled back.
    The fma is an fp64 sum of the exact fp64 square and the rounded fp32 product, rounded to fp32: exact wherever the sum is an
    fp32 number (all of the exact data), else within a double rounding of the fused operation."""
    ar, ai = re.abs(), im.abs()
    h, l = torch.maximum(ar, ai), torch.minimum(ar, ai)
    _, e = torch.frexp(h)
    a, b = torch.ldexp(h, -e), torch.ldexp(l, -e)
    bb = (b.double() * b.double()).to(F32)
    s = (a.double() * a.double() + bb.double()).to(F32).sqrt()
    return torch.ldexp(s, e)


# --------------------------------------------------------------------------------------------------------------- accuracy
def accuracy_data(count: int, squared: bool, seed: int = 0):
    r"""(re, im, g, t_re, t_im) fp32 vectors of ``count`` elements: randn parts with independent per-element scales 2^e, e in
    [-60, 60] ([-30, 30] for the squared form, whose result has twice the exponent), the imaginary part another 2^d, d in
    [-12, 12], away; g and t are randn."""
    g = _gen(77 + seed + int(squared))
    top = 30 if squared else 60
    e = torch.randint(-top, top + 1, (count,), generator=g)
    d = torch.randint(-12, 13, (count,), generator=g)
    re = torch.ldexp(torch.randn(count, generator=g), e)
    im = torch.ldexp(torch.randn(count, generator=g), e + d)
    return re, im, torch.randn(count, generator=g), torch.randn(count, generator=g), torch.randn(count, generator=g)


def ref_cmag(re, im, squared: bool) -> torch.Tensor:
    re, im = re.double(), im.double()
    return re * re + im * im if squared else torch.hypot(re, im)


def ref_vjp(re, im, g, squared: bool):
    re, im, g = re.double(), im.double(), g.double()
    if squared:
        return 2 * g * re, 2 * g * im
    m = torch.hypot(re, im)
    inv = torch.where(m != 0, 1 / torch.where(m != 0, m, torch.ones_like(m)), torch.zeros_like(m))
    return g * re * inv, g * im * inv


def ref_jvp(re, im, t_re, t_im, squared: bool):
    r"""(reference, the sum of the absolute values of its two terms): the sum may cancel, so bounds are on the terms."""
    re, im, t_re, t_im = re.double(), im.double(), t_re.double(), t_im.double()
    if squared:
        return 2 * (re * t_re + im * t_im), 2 * ((re * t_re).abs() + (im * t_im).abs())
    m = torch.hypot(re, im)
    inv = torch.where(m != 0, 1 / torch.where(m != 0, m, torch.ones_like(m)), torch.zeros_like(m))
    return (re * t_re + im * t_im) * inv, ((re * t_re).abs() + (im * t_im).abs()) * inv


# ------------------------------------------------------------------------------------------------------- clip and quantize
CLIP = (2.0, -1.0, 1.0)  # gain, lo, hi: the HDR task
LEVELS = (2, 4, 256)


def clip_data(count: int, gain: float, lo: float, hi: float, seed: int = 0) -> torch.Tensor:
    r"""randn with, in front, elements whose product with ``gain`` is exactly ``lo`` and ``hi``, their fp32 neighbours on both
    sides, +-0 and NaN."""
    x = torch.randn(count, generator=_gen(5 + seed))
    on = torch.tensor([lo / gain, hi / gain], dtype=F32)
    assert torch.equal(on * gain, torch.tensor([lo, hi], dtype=F32))  # (the bounds are hit exactly)
    up, down = torch.nextafter(on, torch.full_like(on, math.inf)), torch.nextafter(on, torch.full_like(on, -math.inf))
    special = torch.cat([on, up, down, torch.tensor([0.0, -0.0, math.nan])])
    x[:special.numel()] = special
    return x


def step_of(levels: int, lo: float, hi: float) -> float:
    return float(torch.tensor((hi - lo) / (levels - 1), dtype=F32))


def quantize_data(count: int, levels: int, lo: float, hi: float, seed: int = 0) -> torch.Tensor:
    r"""randn that leaves [lo, hi] on both sides with, in front, the bounds, every half-way point between two levels that is an
    fp32 number (the ties: round half to even), +-0 and NaN."""
    x = torch.randn(count, generator=_gen(9 + seed + levels))
    step = step_of(levels, lo, hi)
    ties = (torch.arange(min(levels - 1, 64), dtype=F64) + 0.5) * step + lo
    special = torch.cat([torch.tensor([lo, hi, 0.0, -0.0, math.nan], dtype=F64), ties]).to(F32)
    x[:special.numel()] = special
    return x


def quantize_ref(x: torch.Tensor, levels: int, lo: float, hi: float) -> torch.Tensor:
    r"""The written-out torch sequence, in ``x``'s dtype on the CPU."""
    step = step_of(levels, lo, hi)
    return torch.round((torch.clamp(x, lo, hi) - lo) / step) * step + lo


# ---------------------------------------------------------------------------------------------------------- launch forms
def trip_floats() -> int:
    r"""The floats that one trip of the kernels' capped grid covers, from the library's own constants (host arithmetic)."""
    from azula_amd import _lib

    floats = C.c_int64(0)
    _lib.call("az_op_nonlinear_trip", C.byref(floats))
    return floats.value


def beyond_one_trip() -> int:
    r"""An element count that needs one more grid-stride trip than the capped grid covers, and ends in a partial item."""
    return trip_floats() + 4 * 256 * 3 + 5
