r"""Case lists, input families, references and error bounds for the four covariance entries of csrc/covariance.hip
(``az_cov_scale``, ``az_cov_project``, ``az_cov_expand``, ``az_cov_mode``).  test_covariance_host.py checks all of it on the CPU
(the cases can fail, the bound can be met), test_gpu_covariance_kernels.py runs the kernels.  Plain module, no test in it; it
imports nothing from azula_amd and nothing that needs a GPU.

The shapes sit just below, on and just above every tile constant of the kernels: 64 features and 64 rank columns per LDS tile,
32 rows per pass, 512 features per segment of the projection, the ``inner >= 64`` switch of the mode kernel's staging order, and
the grid caps of the scale kernel (65535 row blocks, 65536 feature blocks).

Two input families.

``exact`` -- the indexing check.  Every operand is a small integer held in fp32 or fp64: factors (W, Q) in {-3..3} with no zero
in the last feature, the last column, the last row and the first element; x and P in {-4..4} with no zero at the last contracted
index; c, a, d, g in {-2, -1, 1, 2}.  Every product, partial sum and result is then an integer far below 2^24 (the largest sum of
absolute values over all cases is 1100 * 3 * 2 * 4 = 26400), so any fp32 or fp64 evaluation in any order, fused or not, is exact
and the device must EQUAL the integer reference.  The scale entry's ``e`` is drawn so that h(e) is exact too: {-2, -1, 1, 2}
for e and 1 / e, {1, 4, 9, 16} under the square root, {1, 3} with rho = 1 for e / (e + rho) (1/2 and 3/4).  Q is not symmetric
and W differs in every row and column, so neither a transposition nor a tile shift can cancel; ``FAULTS`` are five such slips
applied to the reference, and the host test asserts that each changes the result of every case it can occur in.

``hard`` -- the arithmetic check.  Magnitudes 10 ** (3 (rand - 0.5)) with random signs (three decades), the rows of x carry an
offset of a few units each.  Operands are rounded to their storage dtype first; the reference reads what is stored.

The reference.  The expression of include/azula_amd.h, evaluated by numpy in ``REF`` = long double (64 significand bits where
the platform has them; fp64 otherwise) on the stored operands.  For an fp32 output plain fp64 would do.  For an fp64 output an
fp64 reference carries the same n 2^-53 S of round-off that the bound allows the device, so the comparison would not be
rigorous; eleven more bits put the reference's own error at 2^-11 of the bound.  S below is summed in fp64.

The bound (hard family).  Every output is a dot product with a few roundings around it; with u = 2^-24 for an fp32 output and
2^-53 for fp64, S the sum of the absolute values of the output's terms (all factors included), and k = terms + extra,

    |out - ref| <= gamma_k S,   gamma_k = k u / (1 - k u)     (the forward bound of a recursive sum; Higham, ASNA, 3.1)

``terms`` is the longest chain of dependent roundings of the accumulation as covariance.hip states it, ``extra`` the other
roundings on an output's path.  Read off the kernels:

  * conversion on load (``cld``): out_dtype is the promotion of the operand dtypes, so every conversion widens and is exact:
    0 roundings.  The reference therefore reads each stored operand as it is.  (The scalars are the exception: a host double or
    an fp64 device scalar is narrowed to an fp32 output type.  The cases' host scalars are fp32 numbers; the reference rounds an
    fp64 device scalar to fp32 exactly as ``cld<float>`` does.)
  * cov_project_kernel: ``acc = fma(W, Xs, acc)`` once per feature of the segment: min(n, 512) roundings (the zero fill of a
    ragged tile adds fma(0, 0, acc) = acc, exact).  Xs = c * x is rounded when it is staged: +1 with c.  With more than one
    segment, cov_project_reduce_kernel adds the partials, lane-strided and then through the butterfly; additions of an exact 0
    are exact, and a partial passes through at most ceil(nseg / 64) + 6 others, never more than nseg: + nseg.  The error of a
    segment's partial is gamma of its own S, and those sum to S.
        terms = min(n, 512) + (nseg if nseg > 1 else 0),  extra = [c]
  * cov_expand_kernel: ``acc = fma(W, Ps, acc)`` once per rank column: r roundings.  Ps = g * P is rounded when staged: +1 with
    g.  ``s * acc`` is written, but s is +1 or -1 in the contract and in every case: exact, 0.  ``dv * x + v`` is a product and
    a sum (one rounding if the compiler fuses them, two as written): +2 with x.  ``av * v``: +1 with a.  Each of these acts on a
    value bounded by S = |a| (|d x| + sum_j |W g P|).
        terms = r,  extra = [g] + 2 [x] + [a]
  * cov_mode_kernel: ``acc = fma(M, x, acc)`` once per m: n roundings, nothing else.
        terms = n,  extra = 0
  * cov_scale_kernel is elementwise; with t1 = k x, t2 = t1 - u, t3 = t2 h, y = t3 + v each written operation rounds its result
    once and passes the earlier errors on, multiplied by |h| where they go through the product:
        |out - ref| <= u' ([k] |t1| |h| + [u] |t2| |h| + (n_h + [e]) |t3| + [v] |y|),   u' = u / (1 - 6 u)
    n_h counts the roundings inside h: 0 for e, 1 for sqrt(e) (``__fsqrt_rn``), 1 for 1 / e, 2 for e / (e + rho) (the sum and
    the IEEE division); at most 6 roundings in all, whose second-order terms u' covers.  Without k, u, e and v the entry copies
    (or widens) x and the bound is 0.

On the CPU torch's evaluation in the output dtype sits at 0.4 to 13 percent of the dot-product bounds from 63 terms on, and at up
to 0.75 of them where an output has one or two terms and the bound is a handful of roundings (test_covariance_host.py prints
the ratios); the elementwise bound of the scale entry is met at 0.3 to 0.97.  So for the dot products the bound guards against
lost precision -- a product formed in a narrower type, a partial sum kept in a narrower type, an operand staged through
a narrower type, an operand rounded twice -- and not against indexing, which is the exact family's job."""

from __future__ import annotations

import functools
import zlib
from collections import namedtuple

import numpy as np
import torch

F32, F64 = torch.float32, torch.float64
DT = {"f32": F32, "f64": F64}
CODE = {F32: 0, F64: 1}  # the C ABI's dtype codes
U = {F32: 2.0 ** -24, F64: 2.0 ** -53}
REF = np.longdouble
SEG, TILE, PASS = 512, 64, 32
H_IDENTITY, H_SQRT, H_INV, H_POSTERIOR = 0, 1, 2, 3
H_ROUNDINGS = {H_IDENTITY: 0, H_SQRT: 1, H_INV: 1, H_POSTERIOR: 2}
FAMILIES = ("exact", "hard")

Project = namedtuple("Project", "n r rows c xd fd")
Expand = namedtuple("Expand", "n r rows x a g s xd fd")  # x: "none" | "d" (a d vector) | "d0" (the constant)
Mode = namedtuple("Mode", "n inner outer transpose xd fd")
Scale = namedtuple("Scale", "n rows h e u v k rho sd alias xd fd")  # e: "n" | "1" | "none"; k: "one" | "host" | "dev"; rho: "host" | "dev"

PROJECT_CASES = [
    Project(1, 1, 1, 0, "f32", "f32"),
    Project(63, 63, 31, 1, "f32", "f32"),
    Project(64, 64, 32, 0, "f32", "f32"),
    Project(65, 65, 33, 1, "f32", "f32"),
    Project(511, 1, 70, 1, "f32", "f32"),
    Project(512, 130, 1, 0, "f32", "f32"),
    Project(513, 65, 33, 1, "f32", "f32"),
    Project(1100, 130, 70, 1, "f32", "f32"),
    Project(1100, 65, 33, 0, "f64", "f64"),
    Project(511, 65, 1, 1, "f64", "f64"),
    Project(513, 63, 31, 1, "f32", "f64"),
    Project(64, 1, 33, 1, "f32", "f64"),
    Project(65, 130, 70, 0, "f64", "f32"),
    Project(1100, 64, 32, 1, "f64", "f32"),
]
EXPAND_CASES = [
    Expand(1, 1, 1, "none", 0, 0, 1, "f32", "f32"),
    Expand(63, 64, 32, "d", 1, 1, -1, "f32", "f32"),
    Expand(64, 65, 33, "d0", 1, 1, 1, "f32", "f32"),
    Expand(65, 200, 70, "d", 0, 1, -1, "f32", "f32"),
    Expand(130, 1, 33, "d0", 1, 0, 1, "f32", "f32"),
    Expand(130, 200, 70, "none", 1, 1, -1, "f32", "f32"),
    Expand(65, 65, 1, "none", 0, 1, 1, "f32", "f32"),
    Expand(130, 64, 32, "d", 1, 0, 1, "f64", "f64"),
    Expand(64, 1, 1, "none", 1, 0, -1, "f64", "f64"),
    Expand(63, 200, 33, "d0", 0, 1, -1, "f32", "f64"),
    Expand(1, 200, 33, "d", 1, 1, 1, "f32", "f64"),
    Expand(65, 65, 70, "d", 1, 1, -1, "f64", "f32"),
    Expand(130, 64, 32, "none", 0, 1, 1, "f64", "f32"),
]
MODE_CASES = [
    Mode(1, 1, 1, 0, "f32", "f32"),
    Mode(5, 7, 3, 1, "f32", "f32"),
    Mode(63, 63, 1, 0, "f32", "f32"),
    Mode(64, 64, 1, 1, "f32", "f32"),
    Mode(65, 70, 3, 0, "f32", "f32"),    # 210 columns: ragged, inner >= 64
    Mode(100, 7, 10, 1, "f32", "f32"),   # 70 columns: ragged, inner < 64
    Mode(130, 64, 3, 1, "f32", "f32"),
    Mode(130, 70, 1, 0, "f32", "f32"),
    Mode(65, 1, 10, 1, "f32", "f32"),
    Mode(100, 63, 3, 0, "f64", "f64"),   # 189 columns: ragged, inner < 64
    Mode(64, 70, 3, 1, "f64", "f64"),
    Mode(65, 64, 10, 0, "f32", "f64"),
    Mode(5, 64, 1, 0, "f32", "f64"),
    Mode(130, 7, 3, 1, "f64", "f32"),
    Mode(63, 70, 3, 1, "f64", "f32"),
]
SCALE_CASES = [
    Scale(1, 1, H_IDENTITY, "n", 0, 0, "one", "host", "f32", 0, "f32", "f32"),
    Scale(255, 3, H_SQRT, "n", 1, 1, "host", "host", "f32", 0, "f32", "f32"),
    Scale(256, 1, H_INV, "1", 1, 0, "dev", "host", "f32", 0, "f32", "f32"),
    Scale(257, 3, H_POSTERIOR, "n", 0, 1, "one", "host", "f32", 0, "f32", "f32"),
    Scale(257, 1, H_POSTERIOR, "1", 1, 1, "dev", "dev", "f64", 0, "f32", "f32"),  # fp64 device scalars, fp32 x
    Scale(256, 3, H_IDENTITY, "none", 1, 1, "host", "host", "f32", 1, "f32", "f32"),
    Scale(255, 1, H_INV, "n", 0, 0, "one", "host", "f32", 1, "f32", "f32"),
    Scale(257, 1, H_IDENTITY, "1", 0, 0, "one", "host", "f32", 0, "f32", "f32"),  # the isotropic apply
    Scale(1, 3, H_SQRT, "1", 0, 1, "dev", "host", "f32", 0, "f32", "f32"),
    Scale(256, 1, H_POSTERIOR, "n", 1, 0, "host", "dev", "f32", 1, "f32", "f32"),
    Scale(3, 65537, H_SQRT, "n", 1, 1, "host", "host", "f32", 0, "f32", "f32"),   # two rows past the 65535 row blocks
    Scale(257, 3, H_POSTERIOR, "n", 1, 1, "dev", "dev", "f64", 1, "f64", "f64"),
    Scale(256, 3, H_IDENTITY, "n", 1, 1, "host", "host", "f32", 0, "f32", "f64"),
    Scale(255, 3, H_SQRT, "1", 1, 0, "dev", "host", "f32", 0, "f64", "f32"),
    Scale(257, 1, H_INV, "n", 0, 1, "host", "host", "f32", 1, "f64", "f32"),
]
STRIDE_X_N = 256 * 65536 + 5  # five features past the 65536 feature blocks of 256 (built on the device by the GPU test)
CASES = {"project": PROJECT_CASES, "expand": EXPAND_CASES, "mode": MODE_CASES, "scale": SCALE_CASES}
INVARIANCE_ROWS = (31, 32, 33, 70)


def entry_of(case) -> str:
    return type(case).__name__.lower()


def case_id(case) -> str:
    return entry_of(case) + "-" + "-".join(str(v) for v in case)


def out_dtype(case) -> torch.dtype:
    return torch.promote_types(DT[case.xd], DT[case.fd])


def segments(n: int) -> int:
    return (n + SEG - 1) // SEG


# ------------------------------------------------------------------------------------------------------------- inputs
def _gen(case, family, salt=0):
    return torch.Generator().manual_seed(zlib.crc32(repr((case_id(case), family, salt)).encode()))


def _pick(g, shape, values):
    v = torch.tensor(values, dtype=F64)
    return v[torch.randint(0, len(values), tuple(shape), generator=g)]


def _ints(g, shape, bound, nonzero_last=()):
    r"""Integers in [-bound, bound]; no zero at the last index of each axis in ``nonzero_last`` nor at the first element."""
    t = torch.randint(-bound, bound + 1, tuple(shape), generator=g).double()
    mask = torch.zeros(tuple(shape), dtype=torch.bool)
    for ax in nonzero_last:
        mask.select(ax, shape[ax] - 1).fill_(True)
    mask.reshape(-1)[0] = True
    fix = _pick(g, shape, [v for v in range(-bound, bound + 1) if v])
    return torch.where(mask & (t == 0), fix, t)


def _mag(g, shape):
    r"""Three decades of magnitude around 1, random signs."""
    shape = tuple(shape)
    sign = 1.0 - 2.0 * torch.randint(0, 2, shape, generator=g).double()
    return sign * 10.0 ** (3.0 * (torch.rand(shape, generator=g, dtype=F64) - 0.5))


def _rows_with_offset(g, rows, rest):
    off = 5.0 * torch.randn((rows,) + (1,) * len(rest), generator=g, dtype=F64)
    return _mag(g, (rows, *rest)) + off


SMALL = (-2, -1, 1, 2)


def _vec(g, family, n, dtype):
    return (_pick(g, (n,), SMALL) if family == "exact" else _mag(g, (n,))).to(dtype)


def _fp32(v: float) -> float:
    return float(np.float32(v))


def inputs(case, family: str, rows: int | None = None) -> dict:
    r"""The operands of ``case`` on the CPU in their storage dtypes (tensors; absent operands None; host scalars floats).  Cached:
    treat the result as read-only.  ``rows`` overrides the case's row count (``outer`` for a Mode) for the invariance tests."""
    assert family in FAMILIES
    return _inputs(entry_of(case), case, family, rows)  # (namedtuples of two types with the same fields compare equal)


@functools.lru_cache(maxsize=None)
def _inputs(entry, case, family, rows):
    exact = family == "exact"
    g = _gen(case, family)
    xd, fd, od = DT[case.xd], DT[case.fd], out_dtype(case)
    if isinstance(case, Project):
        n, r, b = case.n, case.r, rows or case.rows
        return dict(
            W=(_ints(g, (n, r), 3, (0, 1)) if exact else _mag(g, (n, r))).to(fd),
            x=(_ints(g, (b, n), 4, (1,)) if exact else _rows_with_offset(g, b, (n,))).to(xd),
            c=_vec(g, family, n, fd) if case.c else None)
    if isinstance(case, Expand):
        n, r, b = case.n, case.r, rows or case.rows
        return dict(
            W=(_ints(g, (n, r), 3, (0, 1)) if exact else _mag(g, (n, r))).to(fd),
            P=(_ints(g, (b, r), 4, (1,)) if exact else _rows_with_offset(g, b, (r,))).to(od),
            x=None if case.x == "none" else (_ints(g, (b, n), 4, (1,)) if exact else _rows_with_offset(g, b, (n,))).to(xd),
            d=_vec(g, family, n, fd) if case.x == "d" else None,
            d0=(-2.0 if exact else 0.375) if case.x == "d0" else 0.0,
            a=_vec(g, family, n, fd) if case.a else None,
            g=_vec(g, family, r, fd) if case.g else None,
            s=float(case.s))
    if isinstance(case, Mode):
        n, o, k = case.n, rows or case.outer, case.inner
        return dict(
            Q=(_ints(g, (n, n), 3, (0, 1)) if exact else _mag(g, (n, n))).to(fd),
            x=(_ints(g, (o, n, k), 4, (1,)) if exact else _rows_with_offset(g, o, (n, k))).to(xd))
    assert isinstance(case, Scale)
    n, b, sd = case.n, rows or case.rows, DT[case.sd]
    en = {"n": n, "1": 1, "none": 0}[case.e]
    if exact:
        e_values = {H_IDENTITY: SMALL, H_SQRT: (1, 4, 9, 16), H_INV: SMALL, H_POSTERIOR: (1, 3)}[case.h]
        e = _pick(g, (en,), e_values)
        k, rho = -2.0, 1.0
    else:
        e = _mag(g, (en,))
        if case.h in (H_SQRT, H_POSTERIOR):
            e = e.abs()
        k, rho = 0.73, 0.3
    if case.k == "one":
        k = 1.0
    # a host scalar is an fp32 number (the entry narrows its double to the output type); a device scalar holds the raw value in
    # ``sd`` and scale_ref narrows it as the kernel does
    return dict(
        x=(_ints(g, (b, n), 4) if exact else _rows_with_offset(g, b, (n,))).to(xd),
        e=e.to(fd) if en else None,
        u=(_ints(g, (n,), 3) if exact else _mag(g, (n,))).to(fd) if case.u else None,
        v=(_ints(g, (n,), 3) if exact else _mag(g, (n,))).to(fd) if case.v else None,
        k=_fp32(k), rho=_fp32(rho),
        k_dev=torch.tensor([k], dtype=sd) if case.k == "dev" else None,
        rho_dev=torch.tensor([rho], dtype=sd) if case.rho == "dev" else None)


# --------------------------------------------------------------------------------------------------------- references
def _np(t, dt, absolute=False):
    if t is None:
        return None
    a = t.double().numpy().astype(dt)  # (every stored operand is exact in fp64)
    return np.abs(a) if absolute else a


FAULTS = ("last_feature", "last_column", "pass_shift", "transposed", "segment_twice")


def fault_applies(case, fault: str, rows: int | None = None) -> bool:
    r"""Whether the slip exists for this case: a second 32-row pass (a second 64-column tile for a Mode), a second segment, a
    factor with more than one row and column."""
    if isinstance(case, Scale):
        return False
    if fault == "pass_shift":
        return (case.outer * case.inner > TILE) if isinstance(case, Mode) else (rows or case.rows) > PASS
    if fault == "segment_twice":
        return isinstance(case, Project) and case.n > SEG
    if fault == "transposed":
        return case.n > 1 and (isinstance(case, Mode) or case.r > 1)
    return True


def _misread(W):
    r"""W (n, r) read with its indices swapped: element (f, j) taken from offset j n + f."""
    n, r = W.shape
    return W.reshape(-1).reshape(r, n).T


def _shift_rows(y, width):
    r"""The rows of the second ``width``-row pass taken from the first."""
    y = y.copy()
    m = min(2 * width, y.shape[0]) - width
    y[width : width + m] = y[:m]
    return y


def project_ref(inp, dt=REF, fault=None, absolute=False):
    r"""P[b, j] = sum_f W[f, j] c_f x[b, f]."""
    W, x, c = (_np(inp[k], dt, absolute) for k in ("W", "x", "c"))
    xc = x if c is None else x * c
    n = W.shape[0]
    if fault == "transposed":
        W = _misread(W)
    if fault == "last_feature":
        return xc[:, : n - 1] @ W[: n - 1]
    P = xc @ W
    if fault == "last_column":
        P[:, -1] = 0
    if fault == "pass_shift":
        P = _shift_rows(P, PASS)
    if fault == "segment_twice":
        P = P + xc[:, SEG : 2 * SEG] @ W[SEG : 2 * SEG]
    return P


def project_partials(inp, dt=np.float64):
    r"""(segments, rows, r): the sums over each 512-feature segment, as the entry leaves them in ``partial``."""
    W, x, c = (_np(inp[k], dt) for k in ("W", "x", "c"))
    xc = x if c is None else x * c
    return np.stack([xc[:, s : s + SEG] @ W[s : s + SEG] for s in range(0, W.shape[0], SEG)])


def expand_ref(inp, dt=REF, fault=None, absolute=False):
    r"""y[b, f] = a_f (d_f x[b, f] + s sum_j W[f, j] g_j P[b, j])."""
    W, P, x, d, a, g = (_np(inp[k], dt, absolute) for k in ("W", "P", "x", "d", "a", "g"))
    s, d0 = (1.0, abs(inp["d0"])) if absolute else (inp["s"], inp["d0"])
    if fault == "transposed":
        W = _misread(W)
    if fault == "last_feature":
        W = W.copy()
        W[-1] = 0
    gP = P if g is None else P * g
    if fault == "last_column":
        W, gP = W[:, :-1], gP[:, :-1]
    y = dt(s) * (gP @ W.T)
    if x is not None:
        y = (d if d is not None else dt(d0)) * x + y
    if a is not None:
        y = a * y
    if fault == "pass_shift":
        y = _shift_rows(y, PASS)
    return y


def mode_ref(inp, transpose, dt=REF, fault=None, absolute=False):
    r"""y[o, i, k] = sum_m M[i, m] x[o, m, k], M = Q or Q^T."""
    Q, x = _np(inp["Q"], dt, absolute), _np(inp["x"], dt, absolute)
    M = Q.T if bool(transpose) != (fault == "transposed") else Q
    if fault == "last_feature":
        M, x = M[:, :-1], x[:, :-1]
    y = np.matmul(M, x)  # (o, i, k)
    if fault == "last_column":
        y[-1, :, -1] = 0
    if fault == "pass_shift":  # the second 64-column tile of the flattened (o, k) takes the first's
        o, n, k = y.shape
        y = _shift_rows(y.transpose(0, 2, 1).reshape(o * k, n), TILE).reshape(o, k, n).transpose(0, 2, 1)
    return y


def _narrow(v, dt_out):
    return float(np.float32(v)) if dt_out == F32 else float(v)


def scale_ref(inp, case, dt=REF, want_bound=False):
    r"""y = (k x - u) h(e) + v; with ``want_bound`` also the sum of magnitudes that multiplies u' in the bound."""
    od = out_dtype(case)
    x, e, u, v = (_np(inp[k], dt) for k in ("x", "e", "u", "v"))
    k = _narrow(inp["k_dev"].item(), od) if inp["k_dev"] is not None else inp["k"]
    rho = _narrow(inp["rho_dev"].item(), od) if inp["rho_dev"] is not None else inp["rho"]
    scaled = inp["k_dev"] is not None or k != 1.0
    B = np.zeros(x.shape, dtype=np.float64)
    h = None
    with np.errstate(all="ignore"):
        if e is not None:
            h = {H_IDENTITY: lambda: e, H_SQRT: lambda: np.sqrt(e), H_INV: lambda: dt(1) / e,
                 H_POSTERIOR: lambda: e / (e + dt(rho))}[case.h]()
        ah = 1.0 if h is None else np.abs(h).astype(np.float64)
        t = x
        if scaled:
            t = dt(k) * t
            B = B + np.abs(t).astype(np.float64) * ah
        if u is not None:
            t = t - u
            B = B + np.abs(t).astype(np.float64) * ah
        if h is not None:
            t = t * h
            B = B + (H_ROUNDINGS[case.h] + 1) * np.abs(t).astype(np.float64)
        if v is not None:
            t = t + v
            B = B + np.abs(t).astype(np.float64)
    return (t, B) if want_bound else t


def reference(case, inp, fault=None, absolute=False, dt=REF):
    if isinstance(case, Project):
        return project_ref(inp, dt, fault, absolute)
    if isinstance(case, Expand):
        return expand_ref(inp, dt, fault, absolute)
    if isinstance(case, Mode):
        return mode_ref(inp, case.transpose, dt, fault, absolute)
    assert fault is None and not absolute
    return scale_ref(inp, case, dt)


# -------------------------------------------------------------------------------------------------------------- bounds
def roundings(case) -> tuple[int, int]:
    r"""(terms, extra) of the module docstring."""
    if isinstance(case, Project):
        nseg = segments(case.n)
        return min(case.n, SEG) + (nseg if nseg > 1 else 0), int(bool(case.c))
    if isinstance(case, Expand):
        return case.r, int(bool(case.g)) + 2 * int(case.x != "none") + int(bool(case.a))
    assert isinstance(case, Mode)
    return case.n, 0


def gamma(k: int, u: float) -> float:
    return k * u / (1.0 - k * u)


def magnitude(case, inp):
    r"""S: the sum of the absolute values of each output's terms, in fp64."""
    return reference(case, inp, absolute=True, dt=np.float64)


def bound(case, inp, dtype=None):
    r"""The allowed |out - ref| per output, for an output of ``dtype`` (the case's own by default)."""
    u = U[dtype or out_dtype(case)]
    if isinstance(case, Scale):
        return scale_ref(inp, case, np.float64, want_bound=True)[1] * (u / (1.0 - 6.0 * u))
    return gamma(sum(roundings(case)), u) * magnitude(case, inp)


def worst_ratio(out: torch.Tensor, ref, allowed) -> tuple[float, float]:
    r"""(max err / allowed, max err); an output whose allowance is 0 must be exact (ratio inf otherwise)."""
    err = np.abs(out.detach().cpu().numpy().astype(REF) - ref).astype(np.float64)
    assert err.shape == allowed.shape, (err.shape, allowed.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / allowed)
    return float(ratio.max()), float(err.max())


# ------------------------------------------------------------------------------------------- torch's own evaluation
def torch_eval(case, inp, dtype):
    r"""The same expression by torch on the CPU with every operand in ``dtype``: what the host test holds against the integer
    reference (exact family) and against the bound (hard family)."""
    t = lambda k: None if inp[k] is None else inp[k].to(dtype)  # noqa: E731
    if isinstance(case, Project):
        x = t("x") if inp["c"] is None else t("x") * t("c")
        return x @ t("W")
    if isinstance(case, Expand):
        P = t("P") if inp["g"] is None else t("P") * t("g")
        y = inp["s"] * (P @ t("W").T)
        if inp["x"] is not None:
            y = (t("d") if inp["d"] is not None else inp["d0"]) * t("x") + y
        return y if inp["a"] is None else t("a") * y
    if isinstance(case, Mode):
        Q = t("Q")
        return torch.matmul(Q.T if case.transpose else Q, t("x"))
    return scale_eval(case, dtype, **{k: (v.to(dtype) if torch.is_tensor(v) else v) for k, v in inp.items()})


def scale_eval(case, dtype, *, x, e, u, v, k, rho, k_dev, rho_dev):
    r"""(k x - u) h(e) + v by torch, on whatever device the operands are; also the model of the special values."""
    kk = k_dev.to(dtype) if k_dev is not None else k
    rr = rho_dev.to(dtype) if rho_dev is not None else rho
    y = x.to(dtype)
    if k_dev is not None or k != 1.0:
        y = kk * y
    if u is not None:
        y = y - u
    if e is not None:
        h = {H_IDENTITY: lambda: e, H_SQRT: lambda: torch.sqrt(e), H_INV: lambda: 1.0 / e, H_POSTERIOR: lambda: e / (e + rr)}[case.h]()
        y = y * h
    if v is not None:
        y = y + v
    return y
