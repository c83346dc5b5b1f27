r"""Linear system solvers -- drop-in for ``azula.linalg.solve`` (reference ``solve.py:13-185``).

:func:`cg` and :func:`gmres` run a fixed number of iterations with no convergence test, so nothing waits on the device.  The
dot products reduce over the last dimension only: every leading index of ``b`` is an independent system (a row).

* Host tensors, and device cases the kernels do not take: the reference's op sequence.
* Device ``b`` (fp32 or fp64, contiguous) with fp32 or fp64 state (fp64 ``b`` with fp64 state only), an ``x0`` of ``b``'s
  shape and dtype, no gradient wanted through ``b`` / ``x0``, and for GMRES at most :data:`GMRES_MAX` iterations: the state
  lives in the kernels' buffers and every iteration is one ``az_cg_step`` or ``az_gmres_arnoldi`` after the caller's
  operator call (``csrc/krylov.hip``).  Rows up to 1024 elements take one fused pass per entry, longer rows a few passes
  with a fixed-order reduction; a row's result does not depend on the batch it is solved in.
"""

from __future__ import annotations

import ctypes as C
from collections.abc import Callable

import torch
from torch import Tensor

from .. import _lib

__all__ = ["cg", "gmres"]

GMRES_MAX = 32  # AZ_KRYLOV_GMRES_MAX
_CODE = {torch.float32: 0, torch.float64: 1}


def cg(
    A: Callable[[Tensor], Tensor],
    b: Tensor,
    x0: Tensor | None = None,
    iterations: int = 1,
    dtype: torch.dtype | None = None,
) -> Tensor:
    r"""Solves :math:`Ax = b` (:math:`A` symmetric positive semi-definite) with ``iterations`` conjugate gradient steps.

    Arguments:
        A: The linear operator :math:`x \mapsto Ax`.
        b: The right-hand side, with shape :math:`(*, D)`.
        x0: An initial guess, with shape :math:`(*, D)`, or :py:`None` for zeros.
        iterations: The number of iterations.
        dtype: The data type of the intermediate computations (default :class:`torch.float64`).

    Returns:
        The last iterate, with ``b``'s shape and dtype.
    """
    dtype = torch.float64 if dtype is None else dtype
    if iterations >= 1 and _kernels_take(b, x0, dtype):
        with torch.cuda.device(b.device):
            return _cg_kernels(A, b, x0, iterations, dtype)
    return _cg_ops(A, b, x0, iterations, dtype)


def gmres(
    A: Callable[[Tensor], Tensor],
    b: Tensor,
    x0: Tensor | None = None,
    iterations: int = 1,
    dtype: torch.dtype | None = None,
) -> Tensor:
    r"""Solves :math:`Ax = b` (any non-singular :math:`A`) with ``iterations`` generalized minimal residual steps.

    Arguments:
        A: The linear operator :math:`x \mapsto Ax`.
        b: The right-hand side, with shape :math:`(*, D)`.
        x0: An initial guess, with shape :math:`(*, D)`, or :py:`None` for zeros.
        iterations: The number of iterations (the Krylov subspace dimension).
        dtype: The data type of the intermediate computations (default :class:`torch.float64`).

    Returns:
        The last iterate, with ``b``'s shape and dtype.
    """
    dtype = torch.float64 if dtype is None else dtype
    if 1 <= iterations <= GMRES_MAX and _kernels_take(b, x0, dtype):
        with torch.cuda.device(b.device):
            return _gmres_kernels(A, b, x0, iterations, dtype)
    return _gmres_ops(A, b, x0, iterations, dtype)


# ---------------------------------------------------------------------------------------------------------- op sequences
def _dot(u: Tensor, v: Tensor) -> Tensor:
    return torch.einsum("...i,...i", u, v)


def _cg_ops(A, b: Tensor, x0: Tensor | None, iterations: int, dtype: torch.dtype) -> Tensor:
    r"""The reference's tensor op sequence (``solve.py:47-75``)."""
    eps = torch.finfo(dtype).eps
    if x0 is None:
        x, r = torch.zeros_like(b), b
    else:
        x, r = x0, b - A(x0)
    x, r = x.to(dtype), r.to(dtype)
    rr = _dot(r, r)
    p = r
    for _ in range(iterations):
        Ap = A(p.to(b)).to(dtype)
        alpha = (rr / torch.clip(_dot(p, Ap), min=eps))[..., None]
        x = x + alpha * p
        r_next = r - alpha * Ap
        rr_next = _dot(r_next, r_next)
        p = r_next + (rr_next / torch.clip(rr, min=eps))[..., None] * p
        r, rr = r_next, rr_next
    return x.to(b)


def _gmres_ops(A, b: Tensor, x0: Tensor | None, iterations: int, dtype: torch.dtype) -> Tensor:
    r"""The reference's tensor op sequence (``solve.py:109-185``): Arnoldi with modified Gram-Schmidt, Givens rotations of
    the Hessenberg columns, then ``(H + eps I) y = B`` and ``x = x0 + V y``."""
    eps = torch.finfo(dtype).eps
    n = iterations

    def unit(v: Tensor) -> tuple[Tensor, Tensor]:
        norm = torch.linalg.vector_norm(v, dim=-1)
        return v / torch.clip(norm[..., None], min=eps), norm

    r = (b if x0 is None else b - A(x0)).to(dtype)
    v0, b0 = unit(r)
    V, Bv = [v0], [b0]
    H = [[None] * n for _ in range(n + 1)]
    cs, ss = [], []
    for j in range(n):
        w = A(V[j].to(b)).to(dtype)
        for i in range(j + 1):
            H[i][j] = _dot(w, V[i])
            w = w - H[i][j][..., None] * V[i]
        v, H[j + 1][j] = unit(w)
        V.append(v)
        for i in range(j):
            hi, hn = H[i][j], H[i + 1][j]
            H[i][j], H[i + 1][j] = cs[i] * hi - ss[i] * hn, cs[i] * hn + ss[i] * hi
        hj, hn = H[j][j], H[j + 1][j]
        c = torch.clip(torch.sqrt(hj * hj + hn * hn), min=eps)
        cs.append(hj / c)
        ss.append(-hn / c)
        H[j][j] = cs[j] * hj - ss[j] * hn
        Bv.append(ss[j] * Bv[j])
        Bv[j] = cs[j] * Bv[j]
        for i in range(j + 1, n + 1):
            H[i][j] = torch.zeros_like(H[j][j])

    Vm = torch.stack(V[:n], dim=-2)
    Hm = torch.stack([torch.stack(H[i], dim=-1) for i in range(n)], dim=-2)
    rhs = torch.stack(Bv[:n], dim=-1)[..., None]
    y = torch.linalg.solve_triangular(Hm + eps * torch.eye(n, dtype=dtype, device=Hm.device), rhs, upper=True)[..., 0]
    x = torch.einsum("...ij,...i", Vm, y)
    if x0 is not None:
        x = x0 + x
    return x.to(b)


# ---------------------------------------------------------------------------------------------------------- kernels
def _kernels_take(b: Tensor, x0: Tensor | None, dtype: torch.dtype) -> bool:
    if not (torch.is_tensor(b) and b.is_cuda and b.dtype in _CODE and dtype in _CODE and b.ndim >= 1 and b.numel() > 0):
        return False
    if not b.is_contiguous() or (b.dtype == torch.float64 and dtype == torch.float32):
        return False
    if x0 is not None and not (torch.is_tensor(x0) and x0.shape == b.shape and x0.dtype == b.dtype
                               and x0.device == b.device and x0.is_contiguous()):
        return False
    # the kernels are not differentiable: a graph through b or x0 takes the op sequence
    return not (torch.is_grad_enabled() and (b.requires_grad or (x0 is not None and x0.requires_grad)))


def _operand(y: Tensor, b: Tensor, dtype: torch.dtype) -> tuple[Tensor, int]:
    r"""An operator output (or ``b - A(x0)``) as the kernels read it: ``b``'s shape, fp32 or fp64 (``.to(dtype)`` of any
    other floating type, as the reference converts it), contiguous."""
    if not torch.is_tensor(y) or y.shape != b.shape or y.device != b.device:
        what = tuple(y.shape) if torch.is_tensor(y) else type(y).__name__
        raise ValueError(f"the operator must map tensors of shape {tuple(b.shape)} on {b.device} to the same shape, got {what}")
    if y.dtype not in _CODE:
        y = y.to(dtype)
    return y.contiguous(), _CODE[y.dtype]


def _ptr(t: Tensor | None) -> int | None:
    return None if t is None else t.data_ptr()


def _cg_kernels(A, b: Tensor, x0: Tensor | None, iterations: int, dtype: torch.dtype) -> Tensor:
    dim = b.shape[-1]
    rows = b.numel() // dim
    dev = b.device
    r0, in_code = (b, _CODE[b.dtype]) if x0 is None else _operand(b - A(x0), b, dtype)
    nseg = _lib.lib().az_krylov_segments(dim)
    x, r, p = (torch.empty(rows, dim, dtype=dtype, device=dev) for _ in range(3))
    rr, rr_next = torch.empty(rows, dtype=dtype, device=dev), torch.empty(rows, dtype=dtype, device=dev)
    partial = torch.empty(2 * rows * nseg, dtype=dtype, device=dev) if nseg > 1 else None
    p_io = torch.empty_like(b)
    a = _lib.AzCgArgs(r0=r0.data_ptr(), x0=_ptr(x0), x=x.data_ptr(), r=r.data_ptr(), p=p.data_ptr(), rr_out=rr.data_ptr(),
                      p_io=p_io.data_ptr(), partial=_ptr(partial), rows=rows, dim=dim, state_dtype=_CODE[dtype],
                      io_dtype=_CODE[b.dtype], in_dtype=in_code)
    _lib.call("az_cg_init", C.byref(a), _lib.stream_ptr())
    out = torch.empty_like(b)
    for k in range(iterations):
        Ap, a.in_dtype = _operand(A(p_io), b, dtype)
        last = k == iterations - 1
        p_io = None if last else torch.empty_like(b)  # a fresh operator input per call, as p.to(b) is
        a.Ap, a.rr, a.rr_out = Ap.data_ptr(), rr.data_ptr(), rr_next.data_ptr()
        a.p_io, a.out = _ptr(p_io), out.data_ptr() if last else None
        _lib.call("az_cg_step", C.byref(a), _lib.stream_ptr())
        rr, rr_next = rr_next, rr
    return out


def _gmres_kernels(A, b: Tensor, x0: Tensor | None, iterations: int, dtype: torch.dtype) -> Tensor:
    dim = b.shape[-1]
    rows = b.numel() // dim
    dev, n = b.device, iterations
    r0, in_code = (b, _CODE[b.dtype]) if x0 is None else _operand(b - A(x0), b, dtype)
    nseg = _lib.lib().az_krylov_segments(dim)
    V = torch.empty(n, rows, dim, dtype=dtype, device=dev)
    H = torch.zeros(rows, n + 1, n, dtype=dtype, device=dev)
    cs, ss = torch.empty(rows, n, dtype=dtype, device=dev), torch.empty(rows, n, dtype=dtype, device=dev)
    Bv = torch.empty(rows, n + 1, dtype=dtype, device=dev)
    work = torch.empty(rows, dim, dtype=dtype, device=dev) if nseg > 1 else None
    partial = torch.empty((n + 2) * rows * nseg, dtype=dtype, device=dev) if nseg > 1 else None
    v_io = torch.empty_like(b)
    a = _lib.AzGmresArgs(r0=r0.data_ptr(), V=V.data_ptr(), work=_ptr(work), H=H.data_ptr(), cs=cs.data_ptr(),
                         ss=ss.data_ptr(), B=Bv.data_ptr(), v_io=v_io.data_ptr(), partial=_ptr(partial), rows=rows, dim=dim,
                         iterations=n, state_dtype=_CODE[dtype], io_dtype=_CODE[b.dtype], in_dtype=in_code)
    _lib.call("az_gmres_init", C.byref(a), _lib.stream_ptr())
    for j in range(n):
        w, a.in_dtype = _operand(A(v_io), b, dtype)
        v_io = torch.empty_like(b) if j + 1 < n else None
        a.w, a.j, a.v_io = w.data_ptr(), j, _ptr(v_io)
        _lib.call("az_gmres_arnoldi", C.byref(a), _lib.stream_ptr())
    out = torch.empty_like(b)
    a.x0, a.out = _ptr(x0), out.data_ptr()
    _lib.call("az_gmres_finish", C.byref(a), _lib.stream_ptr())
    return out
