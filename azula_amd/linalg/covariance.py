r"""Covariance matrices -- drop-in for ``azula.linalg.covariance``.

Seven classes with the reference's constructors, attributes, ``shape`` / ``rank``, ``from_data``, algebra (``+`` / ``*``
with the same ``NotImplemented`` rules, so that ``Isotropic + Diagonal`` resolves through ``__radd__``), ``@`` / ``__call__``,
``color``, ``inv``, ``logdet``, ``to`` and ``is_floating_point``.

* Host tensors: the reference's op sequence.
* Device tensors: setup stays in torch (``from_data``, the capacitance ``K``, the ``r x r`` ``eigh`` of ``inv`` / ``color``,
  ``logdet``).  The applies -- ``@`` and ``color`` of every class, Kronecker's inner ``L`` included -- run on the kernels of
  ``csrc/covariance.hip`` when ``x`` and the factors are fp32 or fp64 and the factors are contiguous; the output dtype is
  torch's promotion of ``x`` and the factors.  Anything else on the device (half types, non-contiguous factors, a graph
  through the operands) takes the torch sequence, as :func:`azula_amd.linalg.solve.cg` does.
"""

from __future__ import annotations

import abc
import ctypes as C
import math
import string
from collections.abc import Sequence

import torch
from torch import Tensor

from .. import _lib

__all__ = [
    "Covariance",
    "IsotropicCovariance",
    "DiagonalCovariance",
    "FullCovariance",
    "DPLRCovariance",
    "DMLRCovariance",
    "KroneckerCovariance",
]

_CODE = {torch.float32: 0, torch.float64: 1}
H_IDENTITY, H_SQRT, H_INV, H_POSTERIOR = 0, 1, 2, 3  # AZ_COV_H_*


class Covariance(abc.ABC):
    r"""Abstract covariance matrix."""

    @property
    @abc.abstractmethod
    def shape(self) -> Sequence[int]:
        pass

    @abc.abstractmethod
    def __add__(self, other: Covariance) -> Covariance:
        pass

    def __radd__(self, other: Covariance) -> Covariance:
        return self.__add__(other)

    @abc.abstractmethod
    def __mul__(self, other: Covariance) -> Covariance:
        pass

    def __rmul__(self, other: Covariance) -> Covariance:
        return self.__mul__(other)

    @abc.abstractmethod
    def __matmul__(self, x: Tensor) -> Tensor:
        pass

    def __call__(self, x: Tensor) -> Tensor:
        return self.__matmul__(x)

    @abc.abstractmethod
    def color(self, x: Tensor) -> Tensor:
        pass

    @property
    @abc.abstractmethod
    def inv(self) -> Covariance:
        pass

    @abc.abstractmethod
    def logdet(self) -> Tensor:
        pass

    def to(self, *args, **kwargs) -> Covariance:
        r"""A copy whose tensors (and those of its tensor lists, nested covariances included) are moved by ``.to``."""
        new = object.__new__(type(self))
        for name, value in self.__dict__.items():
            if hasattr(value, "to"):
                value = value.to(*args, **kwargs)
            elif isinstance(value, (list, tuple)):
                value = type(value)(w.to(*args, **kwargs) if hasattr(w, "to") else w for w in value)
            new.__dict__[name] = value
        return new

    def cuda(self, device=None) -> Covariance:  # used by `nn.Module.cuda`
        return self.to(torch.device("cuda") if device is None else torch.device("cuda", device) if isinstance(device, int) else device)

    def is_floating_point(self) -> bool:  # used by `nn.Module.to(dtype)`
        return True


# ---------------------------------------------------------------------------------------------------------- kernels
def _kernels_take(x: Tensor, *factors: Tensor) -> bool:
    r"""Device ``x`` (fp32 / fp64, any layout) and contiguous fp32 / fp64 factors of ONE dtype on its device, no gradient
    wanted through any of them."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype in _CODE and x.numel() > 0):
        return False
    dtypes = set()
    for f in factors:
        if not (torch.is_tensor(f) and f.device == x.device and f.dtype in _CODE and f.is_contiguous() and f.numel() > 0):
            return False
        dtypes.add(f.dtype)
    if len(dtypes) > 1:
        return False
    return not (torch.is_grad_enabled() and (x.requires_grad or any(f.requires_grad for f in factors)))


def _out_dtype(x: Tensor, f: Tensor | None) -> torch.dtype:
    return x.dtype if f is None else torch.promote_types(x.dtype, f.dtype)


def _ptr(t: Tensor | None) -> int | None:
    return None if t is None else t.data_ptr()


def _scale(x: Tensor, n: int, *, e: Tensor | None = None, h: int = H_IDENTITY, u: Tensor | None = None,
           v: Tensor | None = None, k: float = 1.0, k_dev: Tensor | None = None, rho: float = 0.0,
           rho_dev: Tensor | None = None, out: Tensor | None = None, f_dtype: torch.dtype | None = None) -> Tensor:
    r"""``(k x - u) h(e) + v`` over rows of ``n`` (``az_cov_scale``); ``x`` contiguous, ``e`` of ``n`` or 1 elements."""
    fd = f_dtype or next((t.dtype for t in (e, u, v) if t is not None), x.dtype)
    od = torch.promote_types(x.dtype, fd)
    y = torch.empty(x.shape, dtype=od, device=x.device) if out is None else out
    scal = k_dev if k_dev is not None else rho_dev
    a = _lib.AzCovScaleArgs(
        x=x.data_ptr(), e=_ptr(e), u=_ptr(u), v=_ptr(v), k_dev=_ptr(k_dev), rho_dev=_ptr(rho_dev), y=y.data_ptr(),
        k=float(k), rho=float(rho), rows=x.numel() // n, n=n, e_len=1 if e is None else e.numel(), h=h,
        x_dtype=_CODE[x.dtype], f_dtype=_CODE[fd], out_dtype=_CODE[od],
        scalar_dtype=_CODE[scal.dtype] if scal is not None else 0,
    )
    with torch.cuda.device(x.device):  # x's stream, whatever device is current
        _lib.call("az_cov_scale", C.byref(a), _lib.stream_ptr())
    return y


def _project(x: Tensor, W: Tensor, n: int, r: int, c: Tensor | None = None) -> Tensor:
    r"""``P = (c * x) @ W`` over rows of ``n`` (``az_cov_project``)."""
    od = torch.promote_types(x.dtype, W.dtype)
    rows = x.numel() // n
    P = torch.empty(rows, r, dtype=od, device=x.device)
    nseg = _lib.lib().az_cov_segments(n)
    partial = torch.empty(nseg, rows, r, dtype=od, device=x.device) if nseg > 1 else None
    a = _lib.AzCovLowRankArgs(x=x.data_ptr(), W=W.data_ptr(), c=_ptr(c), P=P.data_ptr(), partial=_ptr(partial), rows=rows,
                              n=n, r=r, x_dtype=_CODE[x.dtype], f_dtype=_CODE[W.dtype], out_dtype=_CODE[od])
    with torch.cuda.device(x.device):
        _lib.call("az_cov_project", C.byref(a), _lib.stream_ptr())
    return P


def _expand(P: Tensor, W: Tensor, n: int, r: int, *, x: Tensor | None = None, a: Tensor | None = None,
            d: Tensor | None = None, d0: float = 0.0, g: Tensor | None = None, s: float = 1.0) -> Tensor:
    r"""``y = a * (d * x + s (g * P) @ W^T)`` (``az_cov_expand``); ``P`` holds the output dtype."""
    rows = P.numel() // r
    xd = x.dtype if x is not None else P.dtype
    y = torch.empty(rows, n, dtype=P.dtype, device=P.device)
    args = _lib.AzCovLowRankArgs(x=_ptr(x), W=W.data_ptr(), a=_ptr(a), d=_ptr(d), g=_ptr(g), P=P.data_ptr(), y=y.data_ptr(),
                                 d0=float(d0), s=float(s), rows=rows, n=n, r=r, x_dtype=_CODE[xd], f_dtype=_CODE[W.dtype],
                                 out_dtype=_CODE[P.dtype])
    with torch.cuda.device(P.device):
        _lib.call("az_cov_expand", C.byref(args), _lib.stream_ptr())
    return y


def _modes(y: Tensor, Qs: Sequence[Tensor], transpose: bool) -> Tensor:
    r"""``y`` of shape ``(rows, *n)`` contracted with ``Q_i`` (``transpose``: ``Q_i^T``) over every axis, one
    ``az_cov_mode`` each."""
    shape = [Q.shape[0] for Q in Qs]
    outer = y.numel() // math.prod(shape)
    for i, Q in enumerate(Qs):
        od = torch.promote_types(y.dtype, Q.dtype)
        z = torch.empty(y.shape, dtype=od, device=y.device)
        a = _lib.AzCovModeArgs(x=y.data_ptr(), Q=Q.data_ptr(), y=z.data_ptr(), outer=outer * math.prod(shape[:i]), n=shape[i],
                               inner=math.prod(shape[i + 1:]), transpose=int(transpose), x_dtype=_CODE[y.dtype],
                               f_dtype=_CODE[Q.dtype], out_dtype=_CODE[od])
        with torch.cuda.device(y.device):
            _lib.call("az_cov_mode", C.byref(a), _lib.stream_ptr())
        y = z
    return y


def _isotropic_factor(lmbda, x: Tensor) -> tuple[Tensor | None, float]:
    r"""An isotropic ``lmbda`` as the kernels read it: a device tensor in ``x``'s dtype (a 0-d tensor does not promote) or
    a host float."""
    if torch.is_tensor(lmbda):
        if lmbda.is_cuda:
            return lmbda.to(device=x.device, dtype=x.dtype).reshape(1).contiguous(), 1.0
        return None, float(lmbda)
    return None, float(lmbda)


# ------------------------------------------------------------------------------------------------------------ classes
class IsotropicCovariance(Covariance):
    r"""Isotropic covariance matrix.

    .. math:: C = \lambda I
    """

    lmbda: Tensor | float

    def __init__(self, lmbda: Tensor | float) -> None:
        self.lmbda = lmbda.reshape(()) if torch.is_tensor(lmbda) else lmbda

    @property
    def shape(self) -> Sequence[int]:
        raise NotImplementedError("IsotropicCovariance's shape is ambiguous.")

    @staticmethod
    @torch.no_grad()
    def from_data(X: Tensor) -> IsotropicCovariance:
        return IsotropicCovariance(torch.var(X))

    def __add__(self, other: Covariance) -> IsotropicCovariance:
        if isinstance(other, IsotropicCovariance):
            return IsotropicCovariance(self.lmbda + other.lmbda)
        return NotImplemented

    def __mul__(self, other: Covariance) -> IsotropicCovariance:
        if isinstance(other, IsotropicCovariance):
            return IsotropicCovariance(self.lmbda * other.lmbda)
        return NotImplemented

    def _apply_kernels(self, x: Tensor, h: int) -> Tensor | None:
        lam = self.lmbda
        if not _kernels_take(x, *([lam] if torch.is_tensor(lam) and lam.is_cuda else [])):
            return None
        if torch.is_tensor(lam) and lam.device.type == "cpu" and lam.requires_grad and torch.is_grad_enabled():
            return None
        e, k = _isotropic_factor(lam, x)
        if e is None and h == H_SQRT:
            k = math.sqrt(k)
        xc = x.contiguous()
        y = _scale(xc, xc.numel(), e=e, h=h if e is not None else H_IDENTITY, k=k, f_dtype=x.dtype)
        return y.view(x.shape)

    def __matmul__(self, x: Tensor) -> Tensor:
        y = self._apply_kernels(x, H_IDENTITY)
        return self.lmbda * x if y is None else y

    def color(self, x: Tensor) -> Tensor:
        y = self._apply_kernels(x, H_SQRT)
        if y is not None:
            return y
        if torch.is_tensor(self.lmbda):
            return torch.sqrt(self.lmbda) * x
        return math.sqrt(self.lmbda) * x

    @property
    def inv(self) -> IsotropicCovariance:
        return IsotropicCovariance(1 / self.lmbda)

    def logdet(self) -> Tensor:
        raise NotImplementedError("IsotropicCovariance's log determinant is ambiguous.")


class DiagonalCovariance(Covariance):
    r"""Diagonal covariance matrix.

    .. math:: C = \mathrm{diag}(D)
    """

    D: Tensor

    def __init__(self, D: Tensor) -> None:
        self.D = D

    @property
    def shape(self) -> Sequence[int]:
        return self.D.shape

    @staticmethod
    @torch.no_grad()
    def from_data(X: Tensor) -> DiagonalCovariance:
        return DiagonalCovariance(torch.var(X, dim=0))

    def __add__(self, other: Covariance) -> DiagonalCovariance:
        if isinstance(other, IsotropicCovariance):
            return DiagonalCovariance(self.D + other.lmbda)
        if isinstance(other, DiagonalCovariance):
            return DiagonalCovariance(self.D + other.D)
        return NotImplemented

    def __mul__(self, other: Covariance) -> DiagonalCovariance:
        if isinstance(other, IsotropicCovariance):
            return DiagonalCovariance(self.D * other.lmbda)
        if isinstance(other, DiagonalCovariance):
            return DiagonalCovariance(self.D * other.D)
        return NotImplemented

    def _apply(self, x: Tensor, h: int) -> Tensor:
        y = x.reshape(-1, *self.shape)  # (raises, as the reference does, unless x holds whole rows of D's shape)
        if _kernels_take(x, self.D):
            return _scale(y.contiguous(), self.D.numel(), e=self.D, h=h).view(x.shape)
        y = (self.D if h == H_IDENTITY else torch.sqrt(self.D)) * y
        return y.reshape_as(x)

    def __matmul__(self, x: Tensor) -> Tensor:
        return self._apply(x, H_IDENTITY)

    def color(self, x: Tensor) -> Tensor:
        return self._apply(x, H_SQRT)

    @property
    def inv(self) -> DiagonalCovariance:
        return DiagonalCovariance(1 / self.D)

    def logdet(self) -> Tensor:
        return torch.log(self.D).sum()


class FullCovariance(Covariance):
    r"""Full covariance matrix.

    .. math:: C = Q \mathrm{diag}(L) Q^\top

    where :math:`Q` is an orthonormal matrix.
    """

    Q: Tensor
    L: Tensor

    def __init__(self, Q: Tensor, L: Tensor) -> None:
        self.Q, self.L = Q, L

    @property
    def shape(self) -> Sequence[int]:
        return self.Q.shape[:-1]

    @staticmethod
    @torch.no_grad()
    def from_data(X: Tensor) -> FullCovariance:
        samples, *shape = X.shape
        features = math.prod(shape)
        assert features < samples
        C_ = torch.cov(X.flatten(1).T).reshape(features, features)
        L, Q = torch.linalg.eigh(C_)
        return FullCovariance(Q.reshape(*shape, features), L)

    def __add__(self, other: Covariance) -> FullCovariance:
        if isinstance(other, IsotropicCovariance):
            return FullCovariance(self.Q, self.L + other.lmbda)
        return NotImplemented

    def __mul__(self, other: Covariance) -> FullCovariance:
        if isinstance(other, IsotropicCovariance):
            return FullCovariance(self.Q, self.L * other.lmbda)
        return NotImplemented

    def __matmul__(self, x: Tensor) -> Tensor:
        if _kernels_take(x, self.Q, self.L):
            r = self.Q.shape[-1]
            n = self.Q.numel() // r
            P = _project(x.contiguous(), self.Q, n, r)
            return _expand(P, self.Q, n, r, g=self.L).view(x.shape)
        y = x.reshape(-1, *self.shape)
        y = torch.einsum("...i,n...->ni", self.Q, y)
        y = self.L * y
        y = torch.einsum("...i,ni->n...", self.Q, y)
        return y.reshape_as(x)

    def color(self, x: Tensor) -> Tensor:
        if _kernels_take(x, self.Q, self.L):
            r = self.Q.shape[-1]
            n = self.Q.numel() // r
            P = x.to(_out_dtype(x, self.Q)).contiguous().view(-1, r)
            return _expand(P, self.Q, n, r, g=torch.sqrt(self.L)).view(x.shape)
        y = x.reshape(-1, self.Q.shape[-1])
        y = torch.sqrt(self.L) * y
        y = torch.einsum("...i,ni->n...", self.Q, y)
        return y.reshape_as(x)

    @property
    def inv(self) -> FullCovariance:
        return FullCovariance(self.Q, 1 / self.L)

    def logdet(self) -> Tensor:
        return torch.log(self.L).sum()


class _LowRank(Covariance):
    r"""``diag(D) + sign V V^T``: what DPLR (sign +1) and DMLR (sign -1) share."""

    SIGN = 1.0
    D: Tensor
    V: Tensor

    def __init__(self, D: Tensor, V: Tensor) -> None:
        self.D, self.V = D, V

    @property
    def shape(self) -> Sequence[int]:
        return self.D.shape

    @property
    def rank(self) -> int:
        return self.V.shape[-1]

    def __add__(self, other: Covariance) -> Covariance:
        if isinstance(other, IsotropicCovariance):
            return type(self)(self.D + other.lmbda, self.V)
        if isinstance(other, DiagonalCovariance):
            return type(self)(self.D + other.D, self.V)
        if isinstance(other, type(self)):
            return type(self)(self.D + other.D, torch.cat((self.V, other.V), dim=-1))
        return NotImplemented

    def __mul__(self, other: Covariance) -> Covariance:
        if isinstance(other, IsotropicCovariance):
            return type(self)(self.D * other.lmbda, self.V * torch.sqrt(other.lmbda))
        return NotImplemented

    def __matmul__(self, x: Tensor) -> Tensor:
        if _kernels_take(x, self.D, self.V):
            n, r = self.D.numel(), self.rank
            xc = x.contiguous()
            P = _project(xc, self.V, n, r)
            return _expand(P, self.V, n, r, x=xc, d=self.D, s=self.SIGN).view(x.shape)
        y = x.reshape(-1, *self.shape)
        low = torch.einsum("...i,ni->n...", self.V, torch.einsum("...i,n...->ni", self.V, y))
        y = self.D * y + low if self.SIGN > 0 else self.D * y - low
        return y.reshape_as(x)

    def _color_factors(self) -> tuple[Tensor, Tensor]:
        r"""``U`` and ``L`` of ``diag(D)^-1/2 V V^T diag(D)^-1/2 = U diag(L) U^T`` (setup: an ``r x r`` ``eigh``)."""
        W = torch.einsum("...,...i->...i", torch.rsqrt(self.D), self.V)
        L, Q = torch.linalg.eigh(torch.einsum("...i,...j->ij", W, W))
        U = torch.einsum("...i,ij,j->...j", W, Q, torch.rsqrt(L))
        return U, L

    def color(self, x: Tensor) -> Tensor:
        U, L = self._color_factors()
        U = U.contiguous()
        g = torch.sqrt(1 + L) - 1 if self.SIGN > 0 else torch.sqrt(1 - L) - 1
        if _kernels_take(x, self.D, U, g):
            n, r = self.D.numel(), self.rank
            xc = x.contiguous()
            P = _project(xc, U.contiguous(), n, r)
            return _expand(P, U, n, r, x=xc, a=torch.sqrt(self.D), d0=1.0, g=g).view(x.shape)
        y = x.reshape(-1, *self.shape)
        y = y + torch.einsum("...i,i,ni->n...", U, g, torch.einsum("...i,n...->ni", U, y))
        y = torch.sqrt(self.D) * y
        return y.reshape_as(x)

    @property
    def K(self) -> Tensor:  # capacitance
        eye = torch.eye(self.rank, dtype=self.D.dtype, device=self.D.device)
        VDV = torch.einsum("...i,...,...j->ij", self.V, 1 / self.D, self.V)
        return eye + VDV if self.SIGN > 0 else eye - VDV

    def _inverse(self, cls: type) -> Covariance:
        D = 1 / self.D
        L, Q = torch.linalg.eigh(self.K)
        return cls(D, torch.einsum("...,...i,ij,j->...j", D, self.V, Q, torch.rsqrt(L)))

    def logdet(self) -> Tensor:
        return torch.log(self.D).sum() + torch.linalg.slogdet(self.K).logabsdet


class DPLRCovariance(_LowRank):
    r"""Diagonal plus low-rank (DPLR) covariance matrix.

    .. math:: \mathrm{diag}(D) + V V^\top

    Wikipedia:
        https://wikipedia.org/wiki/Low-rank_approximation
    """

    SIGN = 1.0

    def __init__(self, D: Tensor, V: Tensor) -> None:
        self.D, self.V = D, V

    @staticmethod
    @torch.no_grad()
    def from_data(X: Tensor, rank: int = 1, iterations: int = 0) -> DPLRCovariance:
        r"""PCA initialisation, then ``iterations`` EM steps of factor analysis (Ghahramani & Hinton, 1996,
        https://mlg.eng.cam.ac.uk/zoubin/papers/tr-96-1.pdf)."""
        samples, *shape = X.shape
        features = math.prod(shape)
        assert 0 < rank < min(features, samples)
        X = X.flatten(1)
        X = X - X.mean(dim=0)
        wide = samples < features
        # the smaller of the two Gram matrices
        C_ = (torch.einsum("if,jf->ij", X, X) if wide else torch.einsum("ni,nj->ij", X, X)) / (samples - 1)
        if 3 * rank < min(samples, features):
            L, Q = torch.lobpcg(C_, k=rank)
        else:
            L, Q = torch.linalg.eigh(C_)
            L, Q = L[-rank:], Q[:, -rank:]
        if wide:
            Q = torch.einsum("ni,nj->ij", X, Q)
            Q = Q / torch.linalg.norm(Q, dim=0, keepdim=True)
        V = Q * torch.sqrt(L)
        D = torch.var(X, dim=0) - torch.einsum("fi,fi->f", V, V)
        for _ in range(iterations):
            B = DPLRCovariance(D, V).inv(V.T)
            Ez = torch.einsum("if,nf->ni", B, X)
            Ezz = (
                torch.eye(V.shape[-1], dtype=D.dtype, device=D.device)
                - torch.einsum("if,fj->ij", B, V)
                + torch.einsum("ni,nj->ij", Ez, Ez) / (samples - 1)
            )
            Ezz_inv = torch.cholesky_inverse(torch.linalg.cholesky(Ezz))
            V = torch.einsum("nf,ni,ij->fj", X, Ez, Ezz_inv) / (samples - 1)
            D = torch.var(X, dim=0) - torch.einsum("fi,ni,nf->f", V, Ez, X) / (samples - 1)
        return DPLRCovariance(D.reshape(shape), V.reshape(*shape, -1))

    @property
    def inv(self) -> DMLRCovariance:
        return self._inverse(DMLRCovariance)


class DMLRCovariance(_LowRank):
    r"""Diagonal minus low-rank (DMLR) covariance matrix.

    .. math:: \mathrm{diag}(D) - V V^\top
    """

    SIGN = -1.0

    def __init__(self, D: Tensor, V: Tensor) -> None:
        self.D, self.V = D, V

    @property
    def inv(self) -> DPLRCovariance:
        return self._inverse(DPLRCovariance)


class KroneckerCovariance(Covariance):
    r"""Kronecker-factorized covariance matrix.

    .. math:: C = (Q_1 \otimes \dots \otimes Q_n) \, L \, (Q_1 \otimes \dots \otimes Q_n)^\top

    where :math:`Q_i` are orthonormal matrices for each dimension and :math:`\otimes` denotes the Kronecker product.

    Wikipedia:
        https://wikipedia.org/wiki/Kronecker_product
    """

    Qs: Sequence[Tensor]
    L: Covariance

    def __init__(self, Qs: Sequence[Tensor], L: Covariance) -> None:
        self.Qs = tuple(Qs)
        self.L = L

    @property
    def shape(self) -> Sequence[int]:
        return tuple(Q.shape[0] for Q in self.Qs)

    @staticmethod
    def _einsum(transpose: bool, n: int) -> str:
        abc = string.ascii_lowercase[:n]
        return f"...{abc}," + ",".join(f"{i.upper()}{i}" if transpose else f"{i}{i.upper()}" for i in abc)

    @staticmethod
    @torch.no_grad()
    def from_data(X: Tensor, rank: int = 0, iterations: int = 0) -> KroneckerCovariance:
        Qs = []
        for i in range(1, X.ndim):
            _, Qi = torch.linalg.eigh(torch.cov(X.movedim(i, 0).flatten(1)))
            Qs.append(Qi)
        X = torch.einsum(KroneckerCovariance._einsum(False, len(Qs)), X, *Qs)
        if rank > 0 and len(Qs) > 1:
            L = DPLRCovariance.from_data(X, rank=rank, iterations=iterations)
        else:
            L = DiagonalCovariance.from_data(X)
        return KroneckerCovariance(Qs, L)

    def __add__(self, other: Covariance) -> KroneckerCovariance:
        if isinstance(other, IsotropicCovariance):
            return KroneckerCovariance(self.Qs, self.L + other)
        return NotImplemented

    def __mul__(self, other: Covariance) -> KroneckerCovariance:
        if isinstance(other, IsotropicCovariance):
            return KroneckerCovariance(self.Qs, self.L * other)
        return NotImplemented

    def __matmul__(self, x: Tensor) -> Tensor:
        y = x.reshape(-1, *self.shape)
        if _kernels_take(x, *self.Qs):
            y = _modes(y.contiguous(), self.Qs, transpose=True)  # (Q_1 x Q_2 ...)^T x
            y = self.L @ y
            y = _modes(y.contiguous(), self.Qs, transpose=False)
            return y.view(x.shape)
        y = torch.einsum(self._einsum(False, len(self.Qs)), y, *self.Qs)
        y = self.L @ y
        y = torch.einsum(self._einsum(True, len(self.Qs)), y, *self.Qs)
        return y.reshape_as(x)

    def color(self, x: Tensor) -> Tensor:
        y = x.reshape(-1, *self.shape)
        y = self.L.color(y)
        if _kernels_take(y, *self.Qs):
            return _modes(y.contiguous(), self.Qs, transpose=False).view(x.shape)
        y = torch.einsum(self._einsum(True, len(self.Qs)), y, *self.Qs)
        return y.reshape_as(x)

    @property
    def inv(self) -> KroneckerCovariance:
        return KroneckerCovariance(self.Qs, self.L.inv)

    def logdet(self) -> Tensor:
        return self.L.logdet()
