r"""Input families, masks and the fp64 reference for the attention kernels' tests (test_attention_cases_host.py checks the
families on the CPU, test_gpu_attention.py runs the kernels on them).  Plain module, no test in it.

The existing attention tests draw randn q, k, v: every score is O(1), the running maximum of the online softmax settles in the
first 32-key sub-tile and the rescale factor is 1 ever after.  The families here put the score *profile* along the key axis
under control, in log2 units (what the kernels' softmax sees after folding log2 e into the query scale):

* grid inputs (``grid_inputs``): every element on a coarse binary grid, so that q, k, v are exact in bf16, f16, the three-bf16
  split and the two-half split, and every product and fp32 partial sum of q k^T is exact.  Channel 0 carries the profile
  (q_0 = 15, k_0 = profile / (15 scale log2 e) rounded to multiples of 1/2), the other channels small noise that makes the lanes
  of a wave differ.  With D in (16, 64) the scale 1 / sqrt(D) is a power of two and the scores are exact in every entry.
* generic inputs (``rms_inputs``): random rows, RMS-normalised by the kernel, learned gains, a scale above 1 / sqrt(D): the route
  production takes to ``az_attention_f16x2_f32``.  The key rows are solved so that the *normalised, gained* scores follow the profile.
* ``lazy_trace`` emulates the lazy running maximum documented in ``attention_x3_kernel`` (sub-tile 32, threshold 8) in float64
  and tells how often a query jumps after its first sub-tile and how large its probabilities grow: the host test asserts with it
  that each family reaches the branch it was written for.
"""

from __future__ import annotations

import math

import torch
import torch.nn.functional as F

LOG2E = 1.4426950408889634
SUB = 32  # keys per softmax step (one S^T tile) in all three kernel templates
TILE = 64  # keys per LDS tile
LAZY = 8.0  # attention_x3_kernel: the running maximum moves when a sub-tile's maximum exceeds it by more than 2^8

PROFILES = ("ramp_small", "ramp_big", "threshold", "descend", "spike_last", "spike_first")
STEP = {"ramp_small": 4.0, "ramp_big": 12.0, "threshold": 8.0, "descend": -12.0}
MASKS = ("causal", "anticausal", "band", "blocks", "bernoulli", "lone_tail", "masked_spike", "dead_rows")
MASK_SHAPES = ("LL", "B1LL", "1HLL", "BHLL")
GRID_DIMS = (16, 64)  # head sizes whose 1 / sqrt(D) is a power of two
SPIKE = 60.0
MASKED_SPIKE = 100.0


# ------------------------------------------------------------------------------------------------ references
def effective_qk(q, k, rms=None, gains=None):
    r"""q, k as the softmax sees them: RMS norm over the head channels (``rms``: True = eps 1e-5, or the eps) and (D,) gains."""
    if rms:
        eps = 1e-5 if rms is True else float(rms)
        q = q * torch.rsqrt(q.pow(2).mean(-1, keepdim=True) + eps)
        k = k * torch.rsqrt(k.pow(2).mean(-1, keepdim=True) + eps)
    if gains is not None:
        q, k = q * gains[0].to(q.dtype), k * gains[1].to(k.dtype)
    return q, k


def _attention(q, k, v, scale, mask, rms, gains, dtype):
    q, k, v = q.to(dtype), k.to(dtype), v.to(dtype)
    q, k = effective_qk(q, k, rms, gains)
    B, H, T, _ = q.shape
    if mask is not None:
        mask = mask if mask.ndim == 4 else mask[None, None]
    out = torch.empty_like(v)
    rows = max(1, int(1e9 // (H * T * T * q.element_size())))  # batch rows per chunk: no temporary above ~1 GB
    for b0 in range(0, B, rows):
        s = (q[b0:b0 + rows] @ k[b0:b0 + rows].transpose(-1, -2)) * scale
        if mask is not None:
            s = s.masked_fill(~(mask if mask.shape[0] == 1 else mask[b0:b0 + rows]), -math.inf)
        out[b0:b0 + rows] = torch.softmax(s, dim=-1) @ v[b0:b0 + rows]  # a row with no live key: softmax over -inf = NaN
    return out


def reference(q, k, v, scale, mask=None, rms=None, gains=None):
    r"""softmax(masked_fill(q k^T scale, ~mask, -inf)) v in float64 on the CPU, (B, H, T, D) -> (B, H, T, D)."""
    return _attention(q, k, v, scale, mask, rms, gains, torch.float64)


def reference_fp32(q, k, v, scale, mask=None, rms=None, gains=None):
    r"""The same in float32.  Only to measure the tolerance: e32 = max |reference_fp32 - reference| on the same inputs."""
    return _attention(q, k, v, scale, mask, rms, gains, torch.float32)


def max_abs_err(got, ref):
    r"""max |got - ref| over the entries where ``ref`` is finite (dead rows are compared as NaN by the caller)."""
    d = (got.double() - ref).abs()
    return d[torch.isfinite(ref)].max().item()


def lazy_trace(q, k, scale, mask=None):
    r"""float64 emulation of the lazy running maximum (attention_x3_kernel: per 32-key sub-tile ``jump = mt > m_run + 8``) on the
    effective q, k -> (late jumps per query: those from a finite m_run; the largest 2^(s - m_run) per query), both (B, H, T)."""
    s = (q.double() @ k.double().transpose(-1, -2)) * (scale * LOG2E)
    if mask is not None:
        s = s.masked_fill(~(mask if mask.ndim == 4 else mask[None, None]), -math.inf)
    T = s.shape[-1]
    m = torch.full(s.shape[:-1], -math.inf, dtype=torch.float64)
    late = torch.zeros(s.shape[:-1], dtype=torch.int64)
    pmax = torch.zeros(s.shape[:-1], dtype=torch.float64)
    for k0 in range(0, T, SUB):
        st = s[..., k0:k0 + SUB]
        mt = st.max(-1).values
        jump = mt > m + LAZY
        late += (jump & (m > -math.inf)).long()
        m = torch.where(jump, mt, m)
        p = torch.exp2(st - torch.where(m == -math.inf, torch.zeros_like(m), m)[..., None])
        pmax = torch.maximum(pmax, p.max(-1).values)
    return late, pmax


# ------------------------------------------------------------------------------------------------ score profiles
def profile(name: str, T: int) -> torch.Tensor:
    r"""(T,) float64 target scores along the key axis in log2 units, centred on 0."""
    t = (torch.arange(T) // SUB).double()
    if name in STEP:
        p = STEP[name] * t
    elif name in ("flat", "spike_last", "spike_first"):
        p = torch.zeros(T, dtype=torch.float64)
        if name != "flat":
            p[T - 1 if name == "spike_last" else 0] = SPIKE
    else:
        raise ValueError(name)
    return p - (p.max() + p.min()) / 2


def _grid(g, shape, lim: int, step: float) -> torch.Tensor:
    return torch.randint(-lim, lim + 1, shape, generator=g).float() * step


def grid_inputs(name: str, B: int, H: int, T: int, D: int, seed: int = 0, spike: torch.Tensor | None = None):
    r"""-> (q, k, v, scale) float32 (B, H, T, D).  q, v and the noise channels of k: multiples of 2^-3, k_0: multiples of 2^-1;
    |q_0| = 15, |q_d|, |k_d| <= 1/2 elsewhere, |v| <= 2.  ``spike``: (B, H, T) keys that carry MASKED_SPIKE on top (masked_spike).
    For D outside GRID_DIMS the scale is not a power of two and the scores are exact only up to the rounding of q * scale."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * T + D + sum(map(ord, name)))
    scale = 1.0 / math.sqrt(D)
    q, k, v = _grid(g, (B, H, T, D), 4, 0.125), _grid(g, (B, H, T, D), 4, 0.125), _grid(g, (B, H, T, D), 16, 0.125)
    p = profile(name, T).expand(B, H, T).clone()
    if spike is not None:
        p[spike] += MASKED_SPIKE
    q[..., 0] = 15.0
    # rounded from the profile's own origin, then centred on the grid: the step between sub-tiles does not depend on T
    k0 = torch.round((p - p.min()) / (15.0 * scale * LOG2E) * 2) / 2
    k[..., 0] = (k0 - torch.round(k0.max() + k0.min()) / 2).float()
    return q, k, v, scale


def grid_is_exact(q, k, v) -> bool:
    r"""Every element survives bfloat16 and float16, and the float32 q k^T equals the float64 one bit for bit."""
    same = all(bool((t.bfloat16().float() == t).all()) and bool((t.half().float() == t).all()) for t in (q, k, v))
    s32, s64 = q @ k.transpose(-1, -2), q.double() @ k.double().transpose(-1, -2)
    return same and bool((s32.double() == s64).all())


def s_abs(q, k, scale) -> float:
    r"""max_ij sum_d |q_d k_d| scale log2 e: what a relative error of the q elements multiplies (the q_term of the bound)."""
    return ((q.abs().double() @ k.abs().double().transpose(-1, -2)).max() * scale * LOG2E).item()


# ------------------------------------------------------------------------------------------------ generic RMS-normed family
RMS_SCALE = {32: 1.0, 64: 1.0, 80: 0.5, 128: 0.5}  # all above 1 / sqrt(D): scores up to +- scale D between aligned rows
RMS_EPS = 1e-5  # Builder.attention's default


def rms_inputs(name: str, B: int, H: int, T: int, D: int, seed: int = 0):
    r"""-> (q, k, v, scale, gains): raw randn-like rows of random length whose RMS-normalised, gained scores follow ``profile(name)``.

    With gains gq, gk the kernel's scores are scale D (A_i . B_j) / (|A_i / gq| |B_j / gk|) for raw rows q_i ~ A_i / gq,
    k_j ~ B_j / gk.  A_i = u + small noise; B_j = c_j u + n_j with n_j a unit vector orthogonal to u, and c_j solved (bisection, the
    map is monotone on the bracket) so that the score of key j is the profile's.  Where the profile's range exceeds what
    aligned rows can reach (|cos| <= 0.8) its step is compressed; test_attention_cases_host.py asserts what is left."""
    g = torch.Generator().manual_seed(2000 * seed + 7 * T + D + sum(map(ord, name)))
    scale = RMS_SCALE[D]
    gq, gk = (1 + 0.2 * torch.randn(D, generator=g, dtype=torch.float64) for _ in range(2))
    u = torch.randn(B, H, 1, D, generator=g, dtype=torch.float64)
    u = u / u.norm(dim=-1, keepdim=True)

    def ortho(n):
        n = n - (n * u).sum(-1, keepdim=True) * u
        return n / n.norm(dim=-1, keepdim=True)

    sq = 0.4 / (LOG2E * scale * math.sqrt(D))  # per (query, key) noise of ~0.4 log2 units
    A = u + sq * ortho(torch.randn(B, H, T, D, generator=g, dtype=torch.float64))
    n = ortho(torch.randn(B, H, T, D, generator=g, dtype=torch.float64))
    top = scale * D * LOG2E / (A / gq).norm(dim=-1).mean().item()  # log2 score of a key with c / |B / gk| = 1
    fmax = 0.8 / (u / gk).norm(dim=-1).max().item()
    p = profile(name, T)
    if p.abs().max() > top * fmax:
        p = p * (top * fmax / p.abs().max())
    target = (p / top).expand(B, H, T)
    lo, hi = torch.full((B, H, T), -8.0, dtype=torch.float64), torch.full((B, H, T), 8.0, dtype=torch.float64)
    for _ in range(60):
        mid = (lo + hi) / 2
        f = mid / ((mid[..., None] * u + n) / gk).norm(dim=-1)
        below = f < target
        lo, hi = torch.where(below, mid, lo), torch.where(below, hi, mid)
    Bk = ((lo + hi) / 2)[..., None] * u + n
    qlen, klen = (0.5 + torch.rand(B, H, T, 1, generator=g, dtype=torch.float64) * 2 for _ in range(2))
    q, k = (A / gq * qlen).float(), (Bk / gk * klen).float()
    v = torch.randn(B, H, T, D, generator=g)
    return q, k, v, scale, (gq.float(), gk.float())


# ------------------------------------------------------------------------------------------------ masks
def _base_mask(family: str, T: int, g, slice_index: int) -> torch.Tensor:
    r"""(T, T) boolean, True = attend.  Every family but dead_rows keeps a live key in every row."""
    i, j = torch.arange(T)[:, None], torch.arange(T)[None, :]
    eye = i == j
    thin = torch.rand(T, T, generator=g) < 0.9  # a different draw per batch and head on top of the deterministic patterns
    if family == "causal":
        return (j <= i) & (thin | eye)
    if family == "anticausal":  # late queries: every leading tile dead
        return (j >= i) & (thin | eye)
    if family == "band":  # dead tiles on both sides
        return ((i - j).abs() <= 20) & (thin | eye)
    if family == "blocks":  # block-diagonal, block 48: boundaries off the 32 / 64 grid
        return (i // 48 == j // 48) & (thin | eye)
    if family == "bernoulli":
        return (torch.rand(T, T, generator=g) < 0.5) | eye
    if family == "lone_tail":  # each query sees only the last key
        return (j == T - 1).expand(T, T).clone()
    if family == "masked_spike":  # a set of keys dead for every query (they carry the spike), the others thinned
        deadkeys = torch.rand(T, generator=g) < 0.3
        deadkeys[(5 + slice_index) % T] = True
        deadkeys[(T - 1 - slice_index) % T] = False
        m = (thin | eye) & ~deadkeys[None, :]
        m[:, (T - 1 - slice_index) % T] = True  # (a live key for the rows whose diagonal is dead)
        return m
    if family == "dead_rows":
        m = (torch.rand(T, T, generator=g) < 0.5) | eye
        m[dead_rows(T, slice_index)] = False
        return m
    raise ValueError(family)


def dead_rows(T: int, slice_index: int) -> list[int]:
    r"""The queries without a live key in slice ``slice_index``: first, middle and last query blocks, shifted per slice."""
    s = slice_index
    return sorted({s % T, (31 + s) % T, (T // 2 + s) % T, (T - 1 - s) % T})


def make_mask(family: str, kind: str, B: int, H: int, T: int, seed: int = 0) -> torch.Tensor:
    r"""Boolean mask of broadcast shape ``kind``: (L, L), (B, 1, L, L), (1, H, L, L) or (B, H, L, L), each slice its own draw."""
    g = torch.Generator().manual_seed(3000 * seed + 11 * T + sum(map(ord, family + kind)))
    if kind == "LL":
        return _base_mask(family, T, g, 0)
    nb, nh = {"B1LL": (B, 1), "1HLL": (1, H), "BHLL": (B, H)}[kind]
    return torch.stack([torch.stack([_base_mask(family, T, g, b * nh + h) for h in range(nh)]) for b in range(nb)])


def expand_mask(mask: torch.Tensor, B: int, H: int) -> torch.Tensor:
    return (mask if mask.ndim == 4 else mask[None, None]).expand(B, H, *mask.shape[-2:])


# ------------------------------------------------------------------------------------------------ layouts and bounds
def pack_qkv(q, k, v, order: str) -> torch.Tensor:
    r"""(B, H, T, D) x 3 -> the fused (B, T, 3 H D) token tensor in '(n H C)' ("nHC", "3HC") or '(H n C)' ("H3C") order."""
    B, H, T, D = q.shape
    if order in ("nHC", "3HC"):
        return torch.stack((q, k, v), dim=0).permute(1, 3, 0, 2, 4).reshape(B, T, 3 * H * D).contiguous()
    return torch.stack((q, k, v), dim=2).permute(0, 3, 1, 2, 4).reshape(B, T, 3 * H * D).contiguous()


FP32_CLASS = {"az_attention_f32": (4, 2.0 ** -24), "az_attention_x3_f32": (4, 2.0 ** -24), "az_attention_f16x2_f32": (16, 2.0 ** -22)}
HALF_UNIT = {"az_attention_bf16_f32": 2.0 ** -8, "az_attention_f16_f32": 2.0 ** -11}
ENTRIES = tuple(FP32_CLASS) + tuple(HALF_UNIT)


def bound_fp32_class(entry: str, e32: float, vmax: float, sabs: float | None = None) -> float:
    r"""max(M e32, 2^-20 max|v|) + q_term.  M = 4 for the entries whose operands are exact to fp32 (another summation order, the
    hardware exp2); M = 16 for the f16x2 entry (operands carry 22 of fp32's 24 bits: x 4, three sources, rounded up to a power of
    two).  The floor is 4 x the 22-bit operand precision on a convex combination of v.  ``sabs`` (grid inputs only, where the
    fp32 reference has exact scores but the kernel rounds q * scale * log2 e once per element): a relative error eps_q of the q
    elements moves a log2 score by at most eps_q S_abs, a probability by the factor ln 2 eps_q S_abs and the normalised output
    by at most twice that times max|v|."""
    M, eps_q = FP32_CLASS[entry]
    q_term = 0.0 if sabs is None else 2 * math.log(2) * eps_q * sabs * vmax
    return max(M * e32, 2.0 ** -20 * vmax) + q_term


def bound_half_grid(entry: str, e32: float, vmax: float) -> float:
    r"""2-byte entries on grid inputs: exact scores; P is rounded to the type before the second contraction while l sums the
    unrounded p: at most u max|v| (u = 2^-8 bf16, 2^-11 f16).  Bound 2 u max|v| + 4 e32."""
    return 2 * HALF_UNIT[entry] * vmax + 4 * e32


def sdpa_check(q, k, v, scale, mask):
    r"""torch's own float64 SDPA on the same inputs (the host test compares ``reference`` with it)."""
    return F.scaled_dot_product_attention(q.double(), k.double(), v.double(), attn_mask=mask, scale=scale)
