r"""Pseudo-inverse guided diffusion -- drop-in for ``azula.guidance.pgdm`` (reference ``pgdm.py:21-70``).

A DDIM step corrected with ``alpha_s alpha_t J^T (A^+ y - A^+ A x_hat)``, ``J = d x_hat / d x_t``.  The product with ``J^T``
is the HIP pullback of the denoiser (``Denoiser._az_vjp``); ``A`` and ``A_inv`` are the user's callables on device tensors.
The sampler runs on the generic loop.
"""

from __future__ import annotations

from collections.abc import Callable

import torch
from torch import Tensor

from .. import _lib
from ..denoise import Denoiser
from ..sample import DDIMSampler
from ._vjp import mean_and_pullback

__all__ = ["PGDMSampler"]


class PGDMSampler(DDIMSampler):
    r"""Creates a PGDM sampler.

    Arguments:
        denoiser: A denoiser :math:`q_\phi(X \mid X_t)`.
        y: An observation :math:`y \sim \mathcal{N}(A(x), \Sigma_y)`.
        A: The forward operator :math:`x \mapsto A(x)`.
        A_inv: The pseudo-inverse operator :math:`y \mapsto A^\dagger(y)`, such that :math:`A(A^\dagger(A(x))) = A(x)`.
        kwargs: Keyword arguments passed to :class:`azula_amd.sample.DDIMSampler`.
    """

    def __init__(self, denoiser: Denoiser, y: Tensor, A: Callable[[Tensor], Tensor], A_inv: Callable[[Tensor], Tensor],
                 **kwargs) -> None:
        super().__init__(denoiser, **kwargs)
        self.y = y
        self.A = A
        self.A_inv = A_inv

    @torch.no_grad()
    @_lib.on_device
    def step(self, x_t: Tensor, t: Tensor, s: Tensor, **kwargs) -> Tensor:
        alpha_s, sigma_s = self.denoiser.schedule(s)
        alpha_t, sigma_t = self.denoiser.schedule(t)

        tau = 1 - (alpha_t / alpha_s * sigma_s / sigma_t) ** 2
        tau = torch.clip(self.eta * tau, min=0, max=1)
        eps = torch.randn_like(x_t)

        x_hat, pullback = mean_and_pullback(self.denoiser, x_t, t, kwargs)

        x_s = alpha_s * x_hat
        x_s = x_s + sigma_s * torch.sqrt(1 - tau) / sigma_t * (x_t - alpha_t * x_hat)
        x_s = x_s + sigma_s * torch.sqrt(tau) * eps

        grad = self.A_inv(self.y) - self.A_inv(self.A(x_hat))
        grad = pullback(grad)

        return x_s + alpha_s * alpha_t * grad
