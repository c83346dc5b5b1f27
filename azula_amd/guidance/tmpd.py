r"""Tweedie moment projected diffusion -- drop-in for ``azula.guidance.tmpd`` (reference ``tmpd.py:21-73``).

The posterior mean is corrected with ``gamma_t J^T A^T ((y - A x_hat) / (var_y + A gamma_t J^T A^T 1))``,
``J = d x_hat / d x_t``, ``gamma_t = sigma_t^2 / alpha_t``.  ``A^T`` is torch autograd of the user's operator at a detached
``x_hat``; every product with ``J^T`` is the HIP pullback of the inner denoiser (``Denoiser._az_vjp``), called twice after one
forward.
"""

from __future__ import annotations

from collections.abc import Callable

import torch
from torch import Tensor

from .. import _lib
from ..denoise import Denoiser, DiracPosterior
from ..noise import Schedule
from ._vjp import mean_and_pullback

__all__ = ["TMPDenoiser"]


class TMPDenoiser(Denoiser):
    r"""Creates a TMPD denoiser module.

    Arguments:
        denoiser: A denoiser :math:`q_\phi(X \mid X_t)`.
        y: An observation :math:`y \sim \mathcal{N}(A x, \Sigma_y)`.
        A: The forward operator :math:`x \mapsto A x`.
        var_y: The noise variance :math:`\Sigma_y`.
    """

    def __init__(self, denoiser: Denoiser, y: Tensor, A: Callable[[Tensor], Tensor], var_y: float | Tensor) -> None:
        super().__init__()
        self.denoiser = denoiser
        self.y = y
        self.A = A
        self.var_y = var_y

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

        def At(v: Tensor) -> Tensor:
            return torch.autograd.grad(y_hat, x_hat, v, retain_graph=True)[0]

        def cov_x(v: Tensor) -> Tensor:
            return gamma_t * pullback(v)

        var_Ax = self.A(cov_x(At(torch.ones_like(y_hat))))

        grad = (self.y - y_hat.detach()) / (self.var_y + var_Ax)
        grad = gamma_t * pullback(At(grad))

        return DiracPosterior(mean=x_hat.detach() + grad)
