r"""Oracle: the Krylov solvers and DiffPIR (torch, the reference's op order) -- TEST INFRASTRUCTURE.

A functional restatement of ``azula/linalg/solve.py`` (``cg``, ``gmres``) and of ``DiffPIRDenoiser.forward``
(``azula/guidance/diffpir.py:80-99``) over a posterior-mean function, plus the DDIM loop of ``oracle.sampling`` with DiffPIR
in it.  ``tools/make_golden_diffpir.py`` asserts that it is bit-identical to the reference on CPU before it writes
``tests/golden/g26_diffpir.npz``; the GPU tests run it on the host against the device.
"""

from __future__ import annotations

from typing import Callable

import torch
from torch import Tensor

from oracle.sampling import time_pairs, transition, vp_schedule

Op = Callable[[Tensor], Tensor]


def _inner(a: Tensor, c: Tensor) -> Tensor:
    return torch.einsum("...i,...i", a, c)


def _floor(v: Tensor, eps: float) -> Tensor:
    return torch.clip(v, min=eps)


def solve_cg(A: Op, b: Tensor, x0: Tensor | None = None, iterations: int = 1, dtype: torch.dtype | None = None) -> Tensor:
    r"""Conjugate gradients, every iteration run (``solve.py:47-75``)."""
    dtype = dtype or torch.float64
    eps = torch.finfo(dtype).eps
    x = (torch.zeros_like(b) if x0 is None else x0).to(dtype)
    r = (b if x0 is None else b - A(x0)).to(dtype)
    p, rho = r, _inner(r, r)
    for _ in range(iterations):
        q = A(p.to(b)).to(dtype)
        step = rho / _floor(_inner(p, q), eps)
        x, r_new = x + step[..., None] * p, r - step[..., None] * q
        rho_new = _inner(r_new, r_new)
        p = r_new + (rho_new / _floor(rho, eps))[..., None] * p
        r, rho = r_new, rho_new
    return x.to(b)


def solve_gmres(A: Op, b: Tensor, x0: Tensor | None = None, iterations: int = 1, dtype: torch.dtype | None = None) -> Tensor:
    r"""GMRES with modified Gram-Schmidt and Givens rotations, every iteration run (``solve.py:78-185``).  The Hessenberg
    matrix is kept as a dict of columns; the entries below the first sub-diagonal are zero, as the reference fills them."""
    dtype = dtype or torch.float64
    eps = torch.finfo(dtype).eps
    m = iterations
    r = (b if x0 is None else b - A(x0)).to(dtype)

    def normalised(v: Tensor) -> tuple[Tensor, Tensor]:
        n = torch.linalg.vector_norm(v, dim=-1)
        return v / _floor(n[..., None], eps), n

    basis, g0 = normalised(r)
    basis = [basis]
    g = {0: g0}
    col: dict[tuple[int, int], Tensor] = {}
    rot: list[tuple[Tensor, Tensor]] = []
    for j in range(m):
        w = A(basis[j].to(b)).to(dtype)
        for i in range(j + 1):
            col[i, j] = _inner(w, basis[i])
            w = w - col[i, j][..., None] * basis[i]
        v, col[j + 1, j] = normalised(w)
        basis.append(v)
        for i, (c, s) in enumerate(rot):
            top, bottom = col[i, j], col[i + 1, j]
            col[i, j] = c * top - s * bottom
            col[i + 1, j] = c * bottom + s * top
        a, z = col[j, j], col[j + 1, j]
        h = _floor(torch.sqrt(a * a + z * z), eps)
        c, s = a / h, -z / h
        rot.append((c, s))
        col[j, j] = c * a - s * z
        g[j + 1] = s * g[j]
        g[j] = c * g[j]
        for i in range(j + 1, m + 1):
            col[i, j] = torch.zeros_like(col[j, j])
    Hm = torch.stack([torch.stack([col[i, j] for j in range(m)], dim=-1) for i in range(m)], dim=-2)
    gm = torch.stack([g[i] for i in range(m)], dim=-1)
    y = torch.linalg.solve_triangular(Hm + eps * torch.eye(m, dtype=dtype, device=Hm.device), gm.unsqueeze(-1), upper=True)
    x = torch.einsum("...ij,...i", torch.stack(basis[:m], dim=-2), y.squeeze(-1))
    return x.to(b) if x0 is None else (x0 + x).to(b)


SOLVERS = {"cg": solve_cg, "gmres": solve_gmres}


def diffpir_mean(mean: Tensor, alpha_t: Tensor, sigma_t: Tensor, y: Tensor, A: Op, var_y, lmbda: float = 10.0,
                 solver: str = "gmres", iterations: int = 1) -> Tensor:
    r"""DiffPIR's corrected mean from the inner denoiser's mean (``diffpir.py:80-99``)."""
    rho = (sigma_t / alpha_t) ** 2
    with torch.enable_grad():
        xh = mean.detach().requires_grad_()
        Axh = A(xh)

    def AT(v: Tensor) -> Tensor:
        return torch.autograd.grad(Axh, xh, v, retain_graph=True)[0]

    def system(v: Tensor) -> Tensor:
        return AT(A(v) / var_y) + lmbda * v / rho

    delta = SOLVERS[solver](system, AT((y - Axh) / var_y), iterations=iterations)
    return xh + delta


def diffpir_fn(mean_fn: Callable[..., Tensor], y: Tensor, A: Op, var_y, schedule=vp_schedule, **kw) -> Callable[..., Tensor]:
    r"""``mean_fn`` wrapped as a DiffPIR denoiser's mean (``kw``: lmbda, solver, iterations)."""

    def fn(x_t: Tensor, t: Tensor, **kwargs) -> Tensor:
        alpha_t, sigma_t = schedule(t)
        with torch.no_grad():
            mean = mean_fn(x_t, t, **kwargs)
        return diffpir_mean(mean, alpha_t, sigma_t, y, A, var_y, **kw).detach()

    return fn


# ------------------------------------------------------------------------------------------------------------- operators
def pixel_mask(mask: Tensor) -> Op:
    return lambda x: x * mask


def avg_pool2(x: Tensor) -> Tensor:
    return torch.nn.functional.avg_pool2d(x, 2)


def row_matrix(M: Tensor) -> Op:
    r"""x -> x M^T along the last dimension (one matrix for every row)."""
    return lambda x: x @ M.to(x).mT
