r"""Jacobian-free posterior sampling -- drop-in for ``azula.guidance.jfps`` (reference ``jfps.py:22-103``).

The posterior mean of the inner denoiser is corrected with the observation ``y ~ N(A(x), cov_y)`` and the signal covariance
``cov_x``, without a gradient through the network:

    cov_x|t = (cov_x^-1 + (sigma_t / alpha_t)^-2 I)^-1
    x = x_hat + cov_x|t A^T (cov_y + A cov_x|t A^T)^-1 (y - A(x_hat))

The network runs once, without a graph, on its own HIP path.  ``A`` is ``torch.func.jvp`` of the user's operator at
``x_hat`` and ``A^T`` is torch autograd of it.  ``cov_x|t`` comes from the covariance algebra of
:mod:`azula_amd.linalg.covariance`, whose applies inside the Krylov operator run on its kernels for device tensors, and the
solve is :mod:`azula_amd.linalg.solve`.  The user's operator runs outside the engine's tape, so a sampler always runs JFPS on
the generic loop.
"""

from __future__ import annotations

from collections.abc import Callable
from functools import partial
from typing import Literal

import torch
from torch import Tensor

from .. import _lib
from ..denoise import Denoiser, DiracPosterior
from ..linalg.covariance import Covariance, IsotropicCovariance
from ..linalg.solve import cg, gmres
from ..noise import Schedule

__all__ = ["JFPSDenoiser"]


class JFPSDenoiser(Denoiser):
    r"""Creates a JFPS denoiser module.

    Arguments:
        denoiser: A denoiser :math:`q_\phi(X \mid X_t)`.
        y: An observation :math:`y \sim \mathcal{N}(A(x), \Sigma_y)`, with shape :math:`(*, D)`.
        A: The forward operator :math:`x \mapsto A(x)`.
        cov_y: The noise covariance :math:`\Sigma_y`.
        cov_x: The signal covariance :math:`\Sigma_x`.
        solver: The linear solver name, ``"cg"`` or ``"gmres"``.
        iterations: The number of solver iterations.

    ``y``, ``A``, ``cov_y`` and ``cov_x`` are read on every call: a re-assignment takes effect on the next call.
    """

    def __init__(
        self,
        denoiser: Denoiser,
        y: Tensor,
        A: Callable[[Tensor], Tensor],
        cov_y: Covariance,
        cov_x: Covariance,
        solver: Literal["cg", "gmres"] = "cg",
        iterations: int = 1,
    ) -> None:
        super().__init__()
        self.denoiser = denoiser
        self.y = y
        self.A = A
        self.cov_y = cov_y
        self.cov_x = cov_x
        solvers = {"cg": cg, "gmres": gmres}
        if solver not in solvers:
            raise ValueError(f"Unknown solver '{solver}'.")
        self.solve = partial(solvers[solver], iterations=iterations)

    @property
    def schedule(self) -> Schedule:
        return self.denoiser.schedule

    @torch.no_grad()
    @_lib.on_device
    def forward(self, x_t: Tensor, t: Tensor, **kwargs) -> DiracPosterior:
        alpha_t, sigma_t = self.schedule(t)
        q = self.denoiser(x_t, t, **kwargs)
        with torch.enable_grad():
            x_hat = q.mean.detach().requires_grad_()
            y_hat = self.A(x_hat)

        def forward_op(v: Tensor) -> Tensor:  # v -> A v at x_hat
            return torch.func.jvp(self.A, (x_hat.detach(),), (v,))[1]

        def adjoint(v: Tensor) -> Tensor:  # v -> A^T v at x_hat
            return torch.autograd.grad(y_hat, x_hat, v, retain_graph=True)[0]

        cov_t = IsotropicCovariance(sigma_t**2 / alpha_t**2)
        cov_x = (self.cov_x.inv + cov_t.inv).inv

        def normal(v: Tensor) -> Tensor:  # (cov_y + A cov_x|t A^T) v, in the reference's op order
            return self.cov_y(v) + forward_op(cov_x(adjoint(v)))

        w = self.solve(A=normal, b=self.y - y_hat)
        w = torch.autograd.grad(y_hat, x_hat, w)[0]
        return DiracPosterior(mean=x_hat + cov_x(w))
