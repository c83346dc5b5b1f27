r"""Moment matching posterior sampling -- drop-in for ``azula.guidance.mmps`` (reference ``mmps.py:24-92``).

The posterior mean is corrected with ``gamma_t J^T A^T (cov_y + A gamma_t J^T A^T)^-1 (y - A x_hat)``,
``J = d x_hat / d x_t``, ``gamma_t = sigma_t^2 / alpha_t``.  ``A`` is ``torch.func.jvp`` of the user's operator at a detached
``x_hat`` and ``A^T`` torch autograd of it, as in :mod:`azula_amd.guidance.jfps`; every product with ``J^T`` inside the Krylov
operator is the HIP pullback of the inner denoiser (``Denoiser._az_vjp``), run once per solver iteration after ONE forward;
the solve is :mod:`azula_amd.linalg.solve`.
"""

from __future__ import annotations

from collections.abc import Callable
from functools import partial

import torch
from torch import Tensor

from .. import _lib
from ..denoise import Denoiser, DiracPosterior
from ..linalg.covariance import Covariance
from ..linalg.solve import cg, gmres
from ..noise import Schedule
from ._vjp import mean_and_pullback

__all__ = ["MMPSDenoiser"]


class MMPSDenoiser(Denoiser):
    r"""Creates a MMPS denoiser module.

    Arguments:
        denoiser: A denoiser :math:`q_\phi(X \mid X_t)`.
        y: An observation :math:`y \sim \mathcal{N}(A(x), \Sigma_y)`, with shape :math:`(*, D)`.
        A: The forward operator :math:`x \mapsto A(x)`.
        cov_y: The noise covariance :math:`\Sigma_y`.
        solver: The linear solver name (``"cg"`` or ``"gmres"``).
        iterations: The number of solver iterations.
    """

    def __init__(self, denoiser: Denoiser, y: Tensor, A: Callable[[Tensor], Tensor], cov_y: Covariance, solver: str = "gmres",
                 iterations: int = 1) -> None:
        super().__init__()
        self.denoiser = denoiser
        self.y = y
        self.A = A
        self.cov_y = cov_y
        if solver == "cg":
            self.solve = partial(cg, iterations=iterations)
        elif solver == "gmres":
            self.solve = partial(gmres, iterations=iterations)
        else:
            raise ValueError(f"Unknown solver '{solver}'.")

    @property
    def schedule(self) -> Schedule:
        return self.denoiser.schedule

    @torch.no_grad()
    @_lib.on_device
    def forward(self, x_t: Tensor, t: Tensor, **kwargs) -> DiracPosterior:
        alpha_t, sigma_t = self.schedule(t)
        gamma_t = sigma_t**2 / alpha_t

        x_hat, pullback = mean_and_pullback(self.denoiser, x_t, t, kwargs)
        with torch.enable_grad():
            x_hat = x_hat.detach().requires_grad_()
            y_hat = self.A(x_hat)

        def A(v: Tensor) -> Tensor:
            return torch.func.jvp(self.A, (x_hat.detach(),), (v,))[1]

        def At(v: Tensor) -> Tensor:
            return torch.autograd.grad(y_hat, x_hat, v, retain_graph=True)[0]

        def cov_x(v: Tensor) -> Tensor:
            return gamma_t * pullback(v)

        def cov_y(v: Tensor) -> Tensor:
            return self.cov_y(v) + A(cov_x(At(v)))

        grad = self.y - y_hat.detach()
        grad = self.solve(A=cov_y, b=grad)
        grad = gamma_t * pullback(At(grad))

        return DiracPosterior(mean=x_hat.detach() + grad)
