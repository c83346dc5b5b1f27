r"""Case lists, input builders, float64 references and error bounds for the token-side, embedding and small-linear kernels
(test_token_cases_host.py checks all of it on the CPU, test_gpu_token_kernels.py runs the kernels).  Plain module, no test in it; it
imports nothing from azula_amd.

Two kinds of check.

Exact.  Patchify / unpatchify, the token-window copy and fills, the row gathers, the CFG combination and a linear layer fed one-hot
or small-integer rows have one right answer in fp32 (a permutation, one rounded operation per element, or a sum whose every
partial sum is representable): the GPU test compares bits.  The references here are independent restatements (reshape / permute,
torch's fp32 arithmetic, torch's cast).

fp64-bounded, with u = 2^-24.  The bounds are derived from the code, not measured:

* SiLU as the library evaluates it (csrc/common.h, ``az_silu``: v * rcp(1 + exp2(v * -log2 e))):
      e_silu(p) = (|p| + 6) u |silu(p)| + 1e-37
  -- the fp32 rounding of p log2 e moves the exponent by |p| u (relative, in the exponential); v_exp_f32 and v_rcp_f32 are within
  one ulp (2 u each), the add and the two multiplies are one rounding each; 1e-37 admits the flush of results whose reciprocal is
  subnormal.
* the small linears (csrc/linear.hip), with a = x or silu(x) and S = sum_k |a_k| |w_k|:
      allowed = 1.05 [ (ceil(K / 64) + 12) u (S + |b|) + sum_k e_silu(x_k) |w_k| ]
  -- a lane accumulates ceil(K / 64) products (ceil(K / 256) quads in the vector form) with fused multiply-adds, the wave butterfly
  adds six more roundings, the bias one; the rest is slack.  An output SiLU multiplies this by 1.1 (its Lipschitz constant) and
  adds e_silu at the pre-activation.
* SwiGLU: |x_2c| e_silu(x_2c+1) + u |ref|.
* the timestep embedding.  The exponent is reproduced exactly, e32 = fl(fl(-fl(ln P) j) / half) in fp32 (the kernel's order and
  the host table's), the rest is bounded: f = exp(e32), arg = t f in float64 and
      allowed = 3 u |arg| + 2 u
  -- one ulp of expf and half an ulp of the product move the argument, cosf / sinf of values <= 1 are within one ulp.

``PLANTED_FAULTS`` names the errors the restatements below can be given; the host test asserts per name that a case catches it."""

from __future__ import annotations

import math
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
GRID_CAP = 2048 * 256  # az_stream_grid: work items of one trip of a grid-stride loop
PLANTED_FAULTS = ("last k-quad dropped", "one k counted twice", "exponent in the other order", "cos and sin swapped",
                  "truncating 2-byte store", "pad lanes unwritten", "index clamp missing")


def pad4(c):
    return (c + 3) // 4 * 4


def bits(t):
    r"""The bit patterns of a tensor (equal NaNs compare equal, -0 differs from +0)."""
    return t.contiguous().view({4: torch.int32, 2: torch.int16}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a), bits(b)))


# ------------------------------------------------------------------------------------------------ SiLU and SwiGLU
def silu64(p):
    p = p.double()
    return p * torch.sigmoid(p)


def e_silu(p):
    p = p.double()
    return (p.abs() + 6.0) * U * silu64(p).abs() + 1e-37


SILU_SIZES = (1, 1027, GRID_CAP + 1027)
SILU_SPECIALS = (0.0, -0.0, 90.0, -90.0)


def silu_points(n, seed=0):
    r"""n values over +-30 with magnitudes log-uniform in [1e-6, 30]; the ends of both ranges come first."""
    g = torch.Generator().manual_seed(seed)
    mag = torch.exp(torch.empty(n, dtype=torch.float64).uniform_(math.log(1e-6), math.log(30.0), generator=g))
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0).double()
    p = (mag * sign).clamp(-30.0, 30.0)
    edge = torch.tensor([30.0, -30.0, 1e-6, -1e-6], dtype=torch.float64)[: min(n, 4)]
    p[: len(edge)] = edge
    return p.float()


SwigluCase = namedtuple("SwigluCase", "rows cout xs ys")
SWIGLU_CASES = [SwigluCase(7, cout, 2 * cout + dx, ys) for cout in (1, 9, 10, 64) for dx in (0, 2, 8) for ys in (cout, pad4(cout) + 4)]
SWIGLU_LARGE = SwigluCase(8200, 62, 128, 64)  # rows * ys just past GRID_CAP, two pad lanes


def swiglu_inputs(c, seed=0):
    r"""x (rows, xs): values of magnitudes 1e-3 / 1 / 1e3 in the even columns, gates from ``silu_points`` in the odd ones, NaN in the
    columns past 2 cout (which the kernel must not read into the result)."""
    g = torch.Generator().manual_seed(seed + 31 * c.cout + c.xs)
    x = torch.full((c.rows, c.xs), float("nan"))
    val = torch.randn(c.rows, c.cout, generator=g) * torch.tensor([1e-3, 1.0, 1e3])[torch.arange(c.cout) % 3]
    x[:, 0 : 2 * c.cout : 2] = val
    x[:, 1 : 2 * c.cout : 2] = silu_points(c.rows * c.cout, seed + c.cout).reshape(c.rows, c.cout)
    return x


def swiglu_ref(x, cout):
    r"""-> (ref, allowed), both (rows, cout) float64."""
    v, gate = x[:, 0 : 2 * cout : 2].double(), x[:, 1 : 2 * cout : 2]
    ref = v * silu64(gate)
    return ref, v.abs() * e_silu(gate) + U * ref.abs()


def swiglu_fp32(x, cout):
    return x[:, 0 : 2 * cout : 2] * F.silu(x[:, 1 : 2 * cout : 2])


# ------------------------------------------------------------------------------------------------ small linears
LIN_SHAPES = [(5, 7, 40), (3, 9, 4096), (2, 5, 1030), (1, 3, 3), (300, 6, 64)]  # (M, N, K)
LIN_ACTS = [(0, 0), (1, 0), (0, 1)]  # (in_act, out_act)
LIN_FORMS = ("plain", "ldx", "ldy", "offset")  # ldx = K + 4; ldy = N + 3; x one float past a 16-byte boundary (the scalar kernel)


def linear_vector_path(K, ldx, x_off_floats=0):
    r"""az_linear_small_f32's choice, for 16-byte aligned allocations of x and W."""
    return K % 4 == 0 and ldx % 4 == 0 and x_off_floats % 4 == 0


def linear_inputs(M, N, K, in_act, out_act, seed=0):
    r"""x (M, K) with column magnitudes cycling 1e-3 / 1 / 1e3 (within +-30 under an input SiLU), W (N, K), b (N).  Row 0 of W is
    orthogonal to a[0] (a = x or silu(x)) up to its fp32 rounding and b[0] = 0, so y[0, 0] is a cancellation to ~1e-8 of S.  Under
    an output SiLU W is scaled by a power of two so that |pre-activation| <= 30."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * M + 13 * N + K)
    x = torch.randn(M, K, generator=g) * torch.tensor([1e-3, 1.0, 1e3])[torch.arange(K) % 3]
    if in_act:
        x = x.clamp(-30.0, 30.0)
    W = torch.randn(N, K, generator=g) / math.sqrt(K)
    b = torch.randn(N, generator=g)
    a = silu64(x) if in_act else x.double()
    w0 = W[0].double()
    W[0] = (w0 - (w0 @ a[0]) / (a[0] @ a[0]) * a[0]).float()
    b[0] = 0.0
    if out_act:
        s = (a.abs() @ W.double().abs().T).max().item()
        if s > 20.0:
            W = W * 2.0 ** math.floor(math.log2(20.0 / s))
    return x.contiguous(), W.contiguous(), b


def linear_ref(x, W, b, in_act, out_act):
    r"""-> (ref, allowed, S) in float64, (M, N) each."""
    K = x.shape[1]
    a = silu64(x) if in_act else x.double()
    Wd = W.double()
    bd = torch.zeros(W.shape[0], dtype=torch.float64) if b is None else b.double()
    S = a.abs() @ Wd.abs().T
    pre = a @ Wd.T + bd
    allowed = (math.ceil(K / 64) + 12) * U * (S + bd.abs())
    if in_act:
        allowed = allowed + e_silu(x) @ Wd.abs().T
    if out_act:
        return silu64(pre), 1.05 * (1.1 * allowed + e_silu(pre)), S
    return pre, 1.05 * allowed, S


def linear_fp32(x, W, b, in_act=0, out_act=0, fault=None):
    r"""torch's own fp32 evaluation.  ``fault``: "last k-quad dropped" (the last, possibly partial, group of four k), "one k counted
    twice" (k = K // 2)."""
    a = F.silu(x) if in_act else x
    K = a.shape[1]
    if fault == "last k-quad dropped":
        keep = 4 * ((K - 1) // 4)
        a, W = a[:, :keep], W[:, :keep]
    elif fault == "one k counted twice":
        k = K // 2
        a, W = torch.cat((a, a[:, k : k + 1]), 1), torch.cat((W, W[:, k : k + 1]), 1)
    elif fault is not None:
        raise ValueError(fault)
    y = F.linear(a, W, b) if a.shape[1] else (torch.zeros(x.shape[0], W.shape[0]) + (0.0 if b is None else b))
    return F.silu(y) if out_act else y


ONEHOT_CASES = [(K, N) for K in (3, 40, 260, 300) for N in (1, 7)]  # x = identity: M = K (M > 256 loops over grid.y)


def onehot_inputs(K, N, seed=0):
    r"""(x = I_K, W (N, K) with magnitudes 1e-3 .. 1e3 and no zero, b (N)): y = W^T, or fl(W^T + b), bit for bit -- every partial
    sum of a row is 0 or the one weight, so no order of accumulation rounds."""
    g = torch.Generator().manual_seed(seed + 17 * K + N)
    W = torch.randn(N, K, generator=g) * 10.0 ** torch.randint(-3, 4, (N, K), generator=g).float()
    W = torch.where(W == 0, torch.ones_like(W), W)
    return torch.eye(K), W.contiguous(), torch.randn(N, generator=g)


GROUPED_M = 6
GROUPED_GROUPS = [(64, 12, True), (256, 256, False), (8, 5, True)]  # (K, N, has bias); the groups share M, not K


def grouped_inputs(seed=0):
    r"""Per group (x (6, K), W (N, K), b or None, expected (6, N) fp32).  Rows 0-2 are one-hot at k = 0, K - 1 and K // 2 - 1
    against random weights; rows 3-5 hold integers in [-8, 8] against integer weights on the same range: every partial sum is an
    integer below 2^24, so the fp32 result is exact in any order and a dropped, duplicated or misplaced k changes it."""
    out = []
    g = torch.Generator().manual_seed(seed + 5)
    for K, N, has_bias in GROUPED_GROUPS:
        x = torch.zeros(GROUPED_M, K)
        for m, k in enumerate((0, K - 1, K // 2 - 1)):
            x[m, k] = 1.0
        x[3:] = torch.randint(-8, 9, (3, K), generator=g).float()
        Wi = torch.randint(-8, 9, (N, K), generator=g).float()
        Wr = torch.randn(N, K, generator=g)
        b = torch.randint(-8, 9, (N,), generator=g).float() if has_bias else None
        # rows 0-2 meet Wr, rows 3-5 meet Wi: one W serves both if the one-hot columns of Wi are replaced by random values and
        # the integer rows are zero there
        W = Wi.clone()
        for k in (0, K - 1, K // 2 - 1):
            W[:, k] = Wr[:, k]
            x[3:, k] = 0.0
        want = (x.double() @ W.double().T)
        if has_bias:
            want[:3] = (want[:3].float() + b).double()  # one rounding
            want[3:] = want[3:] + b.double()  # exact
        assert (want[3:].abs() < 2 ** 24).all()
        out.append((x, W.contiguous(), b, want.float()))
    return out


# ------------------------------------------------------------------------------------------------ timestep embedding
EMB_DIMS = (6, 256, 320, 1024)
EMB_T = (0.0, 1e-4, 0.5, 1.0, 17.0, 250.25, 999.0, 999.999, 1e4)
EMB_ROWS = (1, 5)
EMB_LARGE = (2100, 512)  # (rows, dim): rows * dim / 2 just past GRID_CAP
MAX_PERIOD = 10000.0


def embedding_e32(half, max_period=MAX_PERIOD):
    r"""fl(fl(-fl(ln P) j) / half), j < half, as numpy float32 (each operation rounded once)."""
    lnp = np.float32(math.log(max_period))
    j = np.arange(half, dtype=np.float32)
    return ((-lnp) * j).astype(np.float32) / np.float32(half)


def embedding_ref(t, half, max_period=MAX_PERIOD):
    r"""t (rows,) float32 -> (ref, allowed), (rows, 2 half) float64: cos block, then sin block."""
    f = torch.from_numpy(np.exp(embedding_e32(half, max_period).astype(np.float64)))
    arg = t.double()[:, None] * f[None]
    allowed = arg.abs() * 3 * U + 2 * U
    return torch.cat((torch.cos(arg), torch.sin(arg)), 1), torch.cat((allowed, allowed), 1)


def embedding_fp32(t, half, max_period=MAX_PERIOD, fault=None):
    r"""torch's fp32 evaluation in the kernel's order.  ``fault``: "exponent in the other order" = -ln P (j / half); "cos and sin
    swapped"."""
    lnp = torch.tensor(math.log(max_period), dtype=torch.float32)
    j = torch.arange(half, dtype=torch.float32)
    h = torch.tensor(float(half), dtype=torch.float32)
    e = (-lnp) * (j / h) if fault == "exponent in the other order" else ((-lnp) * j) / h
    arg = t.float()[:, None] * torch.exp(e)[None]
    blocks = (torch.sin(arg), torch.cos(arg)) if fault == "cos and sin swapped" else (torch.cos(arg), torch.sin(arg))
    return torch.cat(blocks, 1)


def embedding_large_t(rows, seed=0):
    return torch.rand(rows, generator=torch.Generator().manual_seed(seed)) * 1000.0


# ------------------------------------------------------------------------------------------------ patchify
PATCH_Z, PATCH_P, PATCH_B = (1, 3, 4), (1, 2, 3, 4), (1, 3)
PATCH_SCALE = 0.37
PATCH_LARGE = (3, 3, 244, 244, 4, 52)  # (B, Z, H, W, p, cs): B Z H W and B L cs just past GRID_CAP, cs = F + 4


def patch_hw(p):
    return (9, 15) if p == 3 else (8, 12)


def patch_strides(Z, p):
    Fq = Z * p * p
    return sorted({Fq, pad4(Fq), Fq + 8})


def patchify_ref(x, p, cs, scale=None, prefill=0.0, fault=None):
    r"""(B, Z, H, W) -> (B, H/p W/p, cs): feature z p p + a p + b, pad lanes zero; ``scale`` a float32 scalar tensor (one rounded
    multiply).  ``fault`` "pad lanes unwritten": the pad lanes keep ``prefill``."""
    B, Z, H, W = x.shape
    t = x.reshape(B, Z, H // p, p, W // p, p).permute(0, 2, 4, 1, 3, 5).reshape(B, (H // p) * (W // p), Z * p * p)
    if scale is not None:
        t = scale * t
    out = torch.full((B, t.shape[1], cs), prefill if fault == "pad lanes unwritten" else 0.0)
    out[..., : Z * p * p] = t
    return out


def unpatchify_ref(tok, Z, H, W, p):
    r"""(B, L, cs) -> (B, Z, H, W); lanes past Z p p are not read."""
    B = tok.shape[0]
    t = tok[..., : Z * p * p].reshape(B, H // p, W // p, Z, p, p).permute(0, 3, 1, 4, 2, 5)
    return t.reshape(B, Z, H, W).contiguous()


# ------------------------------------------------------------------------------------------------ token windows
CopyCase = namedtuple("CopyCase", "name B cs dst_tokens dst_off src_tokens src_off n")
COPY_CASES = [
    CopyCase("front", 3, 24, 14, 0, 10, 0, 10),
    CopyCase("back", 3, 24, 14, 4, 10, 0, 10),
    CopyCase("middle", 3, 24, 14, 2, 10, 3, 5),
    CopyCase("source_tail", 2, 4, 6, 0, 10, 4, 6),
    CopyCase("interleave_even", 40, 24, 2, 0, 1, 0, 1),  # nn/unet3d.py: x1u[:, 0::2] = x1
    CopyCase("interleave_odd", 40, 4, 2, 1, 1, 0, 1),
    CopyCase("strided_pick", 40, 24, 1, 0, 3, 0, 1),  # nn/unet3d.py: out = full[:, 0::s]
    CopyCase("grid_cap", 2, 96, 11003, 2, 11001, 1, 11000),  # B n cs / 4 just past GRID_CAP
]
FillCase = namedtuple("FillCase", "B cs n dst_tokens dst_off row_bstride")  # row_bstride in units of cs


def fill_cases(cs):
    return [FillCase(3, cs, n, 9, off, rb) for n in (1, 4) for off in (0, 2, 9 - n) for rb in (1, 2, 0)]


FILL_LARGE = FillCase(2, 96, 11000, 11003, 2, 1)


def token_copy_ref(dst, src, c):
    out = dst.clone()
    out[:, c.dst_off : c.dst_off + c.n] = src[:, c.src_off : c.src_off + c.n]
    return out


def fill_inputs(c, seed=0):
    r"""(rows buffer (B, max(rb, 1) cs), pos (n, cs)) with magnitudes 1e-3 .. 1e3: the sums round."""
    g = torch.Generator().manual_seed(seed + c.n + c.cs)
    rb = max(c.row_bstride, 1)
    row = torch.randn(c.B, rb * c.cs, generator=g) * 10.0 ** torch.randint(-3, 4, (c.B, rb * c.cs), generator=g).float()
    pos = torch.randn(c.n, c.cs, generator=g) * 10.0 ** torch.randint(-3, 4, (c.n, c.cs), generator=g).float()
    return row, pos


def token_fill_sum(row, pos, c):
    r"""(B, n, cs) fp32: row[b * row_bstride : + cs] + pos[j]."""
    r = row[:1, : c.cs].expand(c.B, c.cs) if c.row_bstride == 0 else row[:, : c.cs]
    return r[:, None, :] + pos[None, :, :]


H16_DTYPES = {1: torch.bfloat16, 2: torch.float16}
H16_EXTRA = {torch.bfloat16: 16, torch.float16: 13}  # fp32 significand bits the type drops (normal range)


def _from_bits(v):
    r"""Integer bit patterns (any integer dtype; taken modulo 2^32) -> the float32 values with those bits."""
    v = v.to(torch.int64) & 0xFFFFFFFF
    return torch.where(v >= 2 ** 31, v - 2 ** 32, v).to(torch.int32).view(torch.float32)


def h16_special_sums(dtype, seed=0):
    r"""name -> float32 values the SUM row + pos must take: the rounding decisions of a 2-byte store.  All normal or zero."""
    extra = H16_EXTRA[dtype]
    g = torch.Generator().manual_seed(seed)
    base = (torch.randn(64, generator=g) * 10.0 ** torch.randint(-2, 3, (64,), generator=g).float()).to(dtype).float()
    base = torch.where(base.abs() < 1e-3, torch.ones_like(base), base)
    b = bits(base).to(torch.int64) & 0xFFFFFFFF
    lsb, half = 1 << extra, 1 << (extra - 1)
    even, odd = b & ~lsb, b | lsb  # (the sign-magnitude pattern: adding to it moves away from zero for either sign)
    out = {
        "tie_to_even_down": _from_bits(even + half),  # rounds back to the even neighbour below (in magnitude)
        "tie_to_even_up": _from_bits(odd + half),  # rounds away, to the even neighbour above
        "tie_plus_ulp": _from_bits(torch.cat((even, odd)) + half + 1),
        "tie_minus_ulp": _from_bits(torch.cat((even, odd)) + half - 1),
        "zeros": torch.tensor([-0.0, 0.0]),
    }
    if dtype == torch.float16:
        top = torch.tensor([65504.0, 65520.0], dtype=torch.float32)
        tb = bits(top).to(torch.int64)
        edge = _from_bits(torch.stack((tb[0], tb[1] - 1, tb[1], tb[1] + 1)))  # max finite, below the tie, the tie (-> inf), above
        k = torch.tensor([0, 1, 2, 3, 510, 511, 512, 1022, 1023], dtype=torch.float64)
        tie = ((k + 0.5) * 2.0 ** -24).float()  # halfway between two subnormal halves (spacing 2^-24); exact in fp32
        tbit = bits(tie).to(torch.int64)
        sub = torch.cat((tie, _from_bits(tbit + 1), _from_bits(tbit - 1), ((k + 1) * 2.0 ** -24).float()))
        out["half_subnormal"] = torch.cat((sub, -sub))
    else:
        edge = _from_bits(torch.tensor([0x7F7F0000, 0x7F7F7FFF, 0x7F7F8000, 0x7F7F8001]))
    out["overflow_edge"] = torch.cat((edge, -edge))
    return out


def h16_split(s):
    r"""s (float32) -> (row, pos) float32 with row + pos == s exactly: pos = +-2^(floor(log2 |s|) - 2) (or -0 / +-1 at a zero)."""
    e = torch.frexp(s.abs().double())[1].double()
    d = torch.copysign(torch.exp2(e - 3.0), s.double())
    row, pos = (s.double() - d).float(), d.float()
    zero = s == 0
    neg = zero & torch.signbit(s)
    row = torch.where(zero, torch.where(neg, -torch.zeros_like(row), torch.ones_like(row)), row)
    pos = torch.where(zero, torch.where(neg, -torch.zeros_like(pos), -torch.ones_like(pos)), pos)
    return row, pos


def h16_inputs(dtype, seed=0):
    r"""-> (row (cs,), pos (cs,), names): all special sums of ``dtype`` in one token row, cs a multiple of 8 (filled with 1.5)."""
    sums = h16_special_sums(dtype, seed)
    s = torch.cat(list(sums.values()))
    s = torch.cat((s, torch.full(((-len(s)) % 8,), 1.5)))
    row, pos = h16_split(s)
    return row, pos, sums


def truncate_to(x, dtype):
    r"""The planted fault: the 2-byte store keeps the top bits (round toward zero) instead of rounding to nearest even."""
    if dtype == torch.bfloat16:
        return _from_bits(bits(x) & ~0xFFFF).to(dtype)
    small = x.abs() < 2.0 ** -14  # (subnormal halves: chop to the fixed spacing)
    chopped = _from_bits(bits(x) & ~0x1FFF)
    sub = torch.trunc(x.double() * 2.0 ** 24) * 2.0 ** -24
    y = torch.where(small, sub.float(), chopped)
    y = torch.where(y.abs() > 65504.0, torch.copysign(torch.tensor(65504.0), y), y)
    return y.to(dtype)


# ------------------------------------------------------------------------------------------------ gathers and CFG
GATHER_NCOLS = (8, 300, 1000)
GATHER_TABLE_ROWS = 6


def gather_indices(table_rows):
    return torch.tensor([-5, 0, table_rows - 1, table_rows + 2, 1, table_rows - 1, 0, -1], dtype=torch.int64)


def gather_ref(table, idx, fault=None, guard=8):
    r"""table[clamp(idx)].  ``fault`` "index clamp missing": the row at the raw index of the table's surroundings (sentinel rows)."""
    if fault == "index clamp missing":
        fence = torch.full((guard, table.shape[1]), -777.0)
        return torch.cat((fence, table, fence))[idx + guard]
    return table[idx.clamp(0, table.shape[0] - 1)]


CFG_SIZES = (1, 1027, GRID_CAP + 77)
CFG_GUIDANCE = (0.0, 7.5, -1.0)


def cfg_inputs(n, seed=0):
    g = torch.Generator().manual_seed(seed + n)
    mk = lambda: torch.randn(n, generator=g) * 10.0 ** torch.empty(n).uniform_(-3.0, 3.0, generator=g)  # noqa: E731
    return mk(), mk()


def cfg_ref(pos, neg, gdn):
    r"""pos + g (pos - neg) with every operation rounded to fp32 (torch's eager arithmetic)."""
    return pos + torch.tensor(gdn, dtype=torch.float32) * (pos - neg)
