r"""The oracle of the ``RadonOperator`` tests: a restatement of the operator's definition, written for these tests.

The weights are fp32 BY DEFINITION and are restated here in numpy ``float32``, one rounded operation at a time:

    x = j - (W - 1) / 2,  y = i - (H - 1) / 2                        (half-integers: exact)
    p = fadd(fmul(fadd(fmul(x, c), fmul(y, s)), 1 / d), (D - 1) / 2)
    w(a, k, i, j) = max(0, fsub(1, |fsub(p, float(k))|))

with ``(c, s)`` the fp32 rounding of the cosine and sine that :func:`cos_sin` takes from the angle reduced into its octant.
``dense`` is the matrix ``M32`` from that definition literally (every bin of every pixel); :class:`Geometry` holds the same
weights as a per-angle scatter of the two bins ``floor(p)`` and ``floor(p) + 1`` -- all that can be nonzero, which
``test_operators_radon_host.py`` checks against ``dense`` -- so that it scales past dense sizes.  Everything applied to data
runs in fp64 ON those fp32 weights.
"""

import functools
import math

import numpy as np
import torch

f32 = np.float32
EPS = 2.0 ** -24


def cos_sin(deg: float) -> tuple:
    r"""(cos, sin) of an angle in degrees as fp32: reduced modulo 360 in fp64, evaluated within the octant, rotated by
    quadrants.  Multiples of 90 give exactly 0 / +-1, and 45 gives c == s."""
    r = math.fmod(float(deg), 360.0)
    if r < 0:
        r += 360.0
    q, r = divmod(r, 90.0)
    if r == 45.0:
        c = s = math.sqrt(0.5)
    elif r < 45.0:
        c, s = math.cos(math.radians(r)), math.sin(math.radians(r))
    else:
        c, s = math.sin(math.radians(90.0 - r)), math.cos(math.radians(90.0 - r))
    for _ in range(int(q) % 4):
        c, s = -s, c
    return f32(c + 0.0), f32(s + 0.0)  # (+ 0.0: no negative zero)


def table(thetas) -> np.ndarray:
    return np.array([cos_sin(t) for t in thetas], dtype=f32).reshape(-1, 2)


def default_det_count(H: int, W: int, d: float = 1.0) -> int:
    return 2 * math.ceil(math.hypot(H, W) / d / 2) + 1


def positions(H: int, W: int, D: int, c, s, d: float) -> np.ndarray:
    r"""p of every pixel, (H, W) fp32."""
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    x, y = (j - f32((W - 1) / 2)).astype(f32), (i - f32((H - 1) / 2)).astype(f32)
    u = ((x * f32(c)).astype(f32) + (y * f32(s)).astype(f32)).astype(f32)
    u = (u * f32(1.0 / d)).astype(f32)
    return (u + f32((D - 1) / 2)).astype(f32)


def weight(p: np.ndarray, k) -> np.ndarray:
    r"""w of fp32 positions ``p`` on bin(s) ``k`` (an int or an integer array of p's shape), fp32."""
    kf = np.asarray(k).astype(f32)
    return np.maximum(f32(0), (f32(1) - np.abs((p - kf).astype(f32))).astype(f32)).astype(f32)


def dense(thetas, H: int, W: int, D: int, d: float = 1.0) -> np.ndarray:
    r"""M32 as a dense (A D, H W) fp64 array of the fp32 weights: the definition, bin by bin."""
    M = np.zeros((len(thetas), D, H, W))
    for a, t in enumerate(thetas):
        c, s = cos_sin(t)
        p = positions(H, W, D, c, s, d)
        for k in range(D):
            M[a, k] = weight(p, k)
    return M.reshape(len(thetas) * D, H * W)


class Geometry:
    r"""The weights of one operator as a per-angle scatter: for angle a, ``pix`` (pixel numbers), ``bins`` (detector bins) and
    ``w`` (fp64 copies of the nonzero fp32 weights)."""

    def __init__(self, thetas, H: int, W: int, D: int | None = None, d: float = 1.0) -> None:
        self.thetas = [float(t) for t in thetas]
        self.H, self.W, self.d = H, W, float(d)
        self.A, self.D = len(self.thetas), default_det_count(H, W, d) if D is None else D
        self.angles = []
        for t in self.thetas:
            c, s = cos_sin(t)
            p = positions(H, W, self.D, c, s, d).ravel()
            k0 = np.floor(p).astype(np.int64)
            pix, bins, w = [], [], []
            for k in (k0, k0 + 1):
                wk = weight(p, k)
                keep = (k >= 0) & (k < self.D) & (wk > 0)
                pix.append(np.nonzero(keep)[0])
                bins.append(k[keep])
                w.append(wk[keep].astype(np.float64))
            self.angles.append(tuple(torch.from_numpy(np.concatenate(v)) for v in (pix, bins, w)))

    # -- M and M^T on fp64 data ------------------------------------------------------------------------------------------
    def apply(self, x: torch.Tensor) -> torch.Tensor:
        r"""(..., H, W) -> (..., A, D) in fp64."""
        lead = x.shape[:-2]
        xf = x.double().reshape(-1, self.H * self.W)
        out = torch.zeros(xf.shape[0], self.A, self.D, dtype=torch.float64)
        for a, (pix, bins, w) in enumerate(self.angles):
            out[:, a].index_add_(1, bins, xf[:, pix] * w)
        return out.reshape(*lead, self.A, self.D)

    def adjoint(self, v: torch.Tensor) -> torch.Tensor:
        r"""(..., A, D) -> (..., H, W) in fp64."""
        lead = v.shape[:-2]
        vf = v.double().reshape(-1, self.A, self.D)
        out = torch.zeros(vf.shape[0], self.H * self.W, dtype=torch.float64)
        for a, (pix, bins, w) in enumerate(self.angles):
            out.index_add_(1, pix, vf[:, a][:, bins] * w)
        return out.reshape(*lead, self.H, self.W)

    @functools.cached_property
    def nnz_rows(self) -> torch.Tensor:
        r"""(A, D): the nonzero weights of each sinogram bin."""
        out = torch.zeros(self.A, self.D, dtype=torch.float64)
        for a, (_, bins, w) in enumerate(self.angles):
            out[a].index_add_(0, bins, torch.ones_like(w))
        return out

    @functools.cached_property
    def nnz_cols(self) -> torch.Tensor:
        r"""(H, W): the nonzero weights of each pixel."""
        out = torch.zeros(self.H * self.W, dtype=torch.float64)
        for pix, _, w in self.angles:
            out.index_add_(0, pix, torch.ones_like(w))
        return out.reshape(self.H, self.W)

    def dense(self) -> torch.Tensor:
        r"""(A D, H W) fp64, from the scatter."""
        M = torch.zeros(self.A * self.D, self.H * self.W, dtype=torch.float64)
        for a, (pix, bins, w) in enumerate(self.angles):
            M.index_put_((a * self.D + bins, pix), w, accumulate=True)
        return M

    # -- the rule's bounds -----------------------------------------------------------------------------------------------
    def bound_apply(self, x: torch.Tensor) -> torch.Tensor:
        r"""(nnz + 2) 2^-24 (|M32| |x|) per output of ``apply``: nnz fused multiply-adds, each rounded once, and two to spare."""
        return (self.nnz_rows + 2) * EPS * self.apply(x.double().abs())

    def bound_adjoint(self, v: torch.Tensor) -> torch.Tensor:
        return (self.nnz_cols + 2) * EPS * self.adjoint(v.double().abs())

    # -- filtered back-projection ----------------------------------------------------------------------------------------
    @functools.cached_property
    def taps(self) -> torch.Tensor:
        return ramlak(self.D, self.d)

    @property
    def fbp_scale(self) -> float:
        return float(f32(math.pi / self.A))  # (the factor the kernel multiplies by is an fp32 number)

    def filter(self, y: torch.Tensor) -> torch.Tensor:
        return y.double() @ toeplitz(self.taps)

    def bound_filter(self, y: torch.Tensor) -> torch.Tensor:
        t = toeplitz(self.taps)
        return ((t != 0).double().sum(0) + 2) * EPS * (y.double().abs() @ t.abs())

    def fbp(self, y: torch.Tensor) -> torch.Tensor:
        return self.fbp_scale * self.adjoint(self.filter(y))

    def bound_fbp(self, y: torch.Tensor) -> torch.Tensor:
        r"""The two stages composed: the filter's error e1 goes through the (non-negative) back-projection, and the
        back-projection's own rule applies to what it is given, at most |q| + e1."""
        q, e1 = self.filter(y), self.bound_filter(y)
        return self.fbp_scale * (self.adjoint(e1) + (self.nnz_cols + 2) * EPS * self.adjoint(q.abs() + e1))

    def fbp_t(self, g: torch.Tensor) -> torch.Tensor:
        return self.fbp_scale * self.filter(self.apply(g))


def ramlak(D: int, d: float = 1.0) -> torch.Tensor:
    r"""The D Ram-Lak taps h[0] = 1 / (4 d^2), h[n odd] = -1 / (pi n d)^2, h[n even] = 0: fp64 values, rounded to fp32."""
    n = np.arange(D, dtype=np.float64)
    h = np.zeros(D)
    h[0] = 1.0 / (4.0 * d * d)
    h[1::2] = -1.0 / (np.pi * n[1::2] * d) ** 2
    return torch.from_numpy(h.astype(f32))


def toeplitz(taps: torch.Tensor) -> torch.Tensor:
    r"""The symmetric (D, D) fp64 matrix T[k, s] = taps[|s - k|]."""
    D = taps.numel()
    idx = (torch.arange(D)[:, None] - torch.arange(D)[None, :]).abs()
    return taps.double()[idx]


@functools.lru_cache(maxsize=64)
def geometry(thetas: tuple, H: int, W: int, D: int | None = None, d: float = 1.0) -> Geometry:
    r"""One shared, unchanged Geometry per case."""
    return Geometry(thetas, H, W, D, d)
