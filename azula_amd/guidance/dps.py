r"""Diffusion posterior sampling -- drop-in for ``azula.guidance.dps`` (reference ``dps.py:21-70``).

A DDPM step whose result is corrected with the gradient of the observation error norm ``|y - A(x_hat(x_t))|`` with respect
to ``x_t``.  The reference differentiates through the network with torch autograd; here the operator part
``d |y - A(x_hat)| / d x_hat`` is torch autograd of the user's ``A`` at a detached ``x_hat`` and the network part is the HIP
pullback of the denoiser (``Denoiser._az_vjp``).  The user's operator runs outside the engine's tape, so the sampler runs on
the generic loop.
"""

from __future__ import annotations

from collections.abc import Callable

import torch
from torch import Tensor

from .. import _lib
from ..denoise import Denoiser
from ..sample import DDPMSampler
from ._vjp import mean_and_pullback

__all__ = ["DPSSampler"]


class DPSSampler(DDPMSampler):
    r"""Creates a DPS sampler.

    Arguments:
        denoiser: A denoiser :math:`q_\phi(X \mid X_t)`.
        y: An observation :math:`y \sim \mathcal{N}(A(x), \Sigma_y)`.
        A: The forward operator :math:`x \mapsto A(x)`.
        zeta: The guidance strength :math:`\zeta`.
        kwargs: Keyword arguments passed to :class:`azula_amd.sample.DDPMSampler`.
    """

    def __init__(self, denoiser: Denoiser, y: Tensor, A: Callable[[Tensor], Tensor], zeta: float = 1.0, **kwargs) -> None:
        super().__init__(denoiser, **kwargs)
        self.y = y
        self.A = A
        self.zeta = zeta

    @torch.no_grad()
    @_lib.on_device
    def step(self, x_t: Tensor, t: Tensor, s: Tensor, **kwargs) -> Tensor:
        alpha_s, sigma_s = self.denoiser.schedule(s)
        alpha_t, sigma_t = self.denoiser.schedule(t)

        tau = 1 - (alpha_t / alpha_s * sigma_s / sigma_t) ** 2
        eps = torch.randn_like(x_t)  # (before the denoiser call, as the reference: dps.py:53)

        x_hat, pullback = mean_and_pullback(self.denoiser, x_t, t, kwargs)

        x_s = alpha_s * x_hat
        x_s = x_s + sigma_s * torch.sqrt(1 - tau) / sigma_t * (x_t - alpha_t * x_hat)
        x_s = x_s + sigma_s * torch.sqrt(tau) * eps

        with torch.enable_grad():
            x_hat = x_hat.detach().requires_grad_()
            error = self.y - self.A(x_hat)
            norm = torch.linalg.vector_norm(error)
        grad = pullback(torch.autograd.grad(norm, x_hat)[0])

        return x_s - self.zeta * grad
