r"""DiffPIR plug-and-play restoration -- drop-in for ``azula.guidance.diffpir`` (reference ``diffpir.py:24-99``).

The posterior mean of the inner denoiser is corrected by a few Krylov iterations on the regularised normal equations of the
observation ``y ~ N(A x, var_y)`` (Zhu et al., 2023, https://arxiv.org/abs/2305.08995):

    x = x_hat + (A^T A / var_y + lmbda / rho_t)^-1 A^T (y - A x_hat) / var_y,    rho_t = (sigma_t / alpha_t)^2

It needs no gradient through the denoiser: the network runs once, without a graph, on its own HIP path, and ``A^T`` is
torch autograd of the user's ``A`` at ``x_hat``.  The solve is :mod:`azula_amd.linalg` (device tensors: the Krylov kernels).
The user's ``A`` and its adjoint run outside the engine's tape, so a sampler always runs DiffPIR on the generic loop.
"""

from __future__ import annotations

from collections.abc import Callable
from functools import partial
from typing import Literal

import torch
from torch import Tensor

from ..denoise import Denoiser, DiracPosterior
from ..linalg.solve import cg, gmres
from ..noise import Schedule

__all__ = ["DiffPIRDenoiser"]


class DiffPIRDenoiser(Denoiser):
    r"""Creates a DiffPIR denoiser module.

    Arguments:
        denoiser: A denoiser :math:`q_\phi(X \mid X_t)`.
        y: An observation :math:`y \sim \mathcal{N}(A x, \Sigma_y)`, with shape :math:`(*, D)`.
        A: The forward operator :math:`x \mapsto A x`.
        var_y: The noise variance :math:`\Sigma_y`.
        lmbda: The regularization strength :math:`\lambda \in \mathbb{R}_+`.
        solver: The linear solver name, ``"cg"`` or ``"gmres"``.
        iterations: The number of solver iterations.

    ``y``, ``A`` and ``var_y`` are read on every call: a re-assignment takes effect on the next call.
    """

    def __init__(
        self,
        denoiser: Denoiser,
        y: Tensor,
        A: Callable[[Tensor], Tensor],
        var_y: float | Tensor,
        lmbda: float = 10.0,
        solver: Literal["cg", "gmres"] = "gmres",
        iterations: int = 1,
    ) -> None:
        super().__init__()
        self.denoiser = denoiser
        self.y = y
        self.A = A
        self.var_y = var_y
        self.lmbda = lmbda
        solvers = {"cg": cg, "gmres": gmres}
        if solver not in solvers:
            raise ValueError(f"Unknown solver '{solver}'.")
        self.solve = partial(solvers[solver], iterations=iterations)

    @property
    def schedule(self) -> Schedule:
        return self.denoiser.schedule

    @torch.no_grad()
    def forward(self, x_t: Tensor, t: Tensor, **kwargs) -> DiracPosterior:
        alpha_t, sigma_t = self.schedule(t)
        rho_t = (sigma_t / alpha_t) ** 2
        q = self.denoiser(x_t, t, **kwargs)
        with torch.enable_grad():
            x_hat = q.mean.detach().requires_grad_()
            y_hat = self.A(x_hat)

        def adjoint(v: Tensor) -> Tensor:  # v -> A^T v at x_hat
            return torch.autograd.grad(y_hat, x_hat, v, retain_graph=True)[0]

        def normal(v: Tensor) -> Tensor:  # (A^T A / var_y + lmbda / rho_t) v, in the reference's op order
            return adjoint(self.A(v) / self.var_y) + self.lmbda * v / rho_t

        rhs = adjoint((self.y - y_hat) / self.var_y)
        return DiracPosterior(mean=x_hat + self.solve(A=normal, b=rhs))
