r"""Oracle: DPS, PGDM, TMPD and MMPS (torch, the reference's op order) -- TEST INFRASTRUCTURE.

A functional restatement of ``DPSSampler.step`` (``azula/guidance/dps.py:45-70``), ``PGDMSampler.step`` (``pgdm.py:48-70``),
``TMPDenoiser.forward`` (``tmpd.py:49-73``) and ``MMPSDenoiser.forward`` (``mmps.py:63-92``) over a posterior-mean function
that torch can differentiate, with explicit ``autograd.grad`` calls and the noise handed in.
``tools/make_golden_guidance_vjp.py`` asserts that it is bit-identical to the reference's classes on the CPU before it writes
``tests/golden/g28_guidance_vjp.npz``; the GPU tests run it on the host (in fp64) against the device.
"""

from __future__ import annotations

from typing import Callable

import torch
from torch import Tensor

from diffpir_oracle import SOLVERS
from oracle.sampling import time_pairs, vp_schedule

Op = Callable[[Tensor], Tensor]


def _ddpm_part(x_hat, x_t, eps, alpha_t, sigma_t, alpha_s, sigma_s, tau):
    x_s = alpha_s * x_hat
    x_s = x_s + sigma_s * torch.sqrt(1 - tau) / sigma_t * (x_t - alpha_t * x_hat)
    x_s = x_s + sigma_s * torch.sqrt(tau) * eps
    return x_s


@torch.no_grad()
def dps_step(mean_fn, x_t: Tensor, t: Tensor, s: Tensor, eps: Tensor, y: Tensor, A: Op, zeta: float = 1.0,
             schedule=vp_schedule) -> Tensor:
    alpha_s, sigma_s = schedule(s)
    alpha_t, sigma_t = schedule(t)
    tau = 1 - (alpha_t / alpha_s * sigma_s / sigma_t) ** 2
    with torch.enable_grad():
        x_t = x_t.detach().requires_grad_()
        x_hat = mean_fn(x_t, t)
    x_s = _ddpm_part(x_hat, x_t, eps, alpha_t, sigma_t, alpha_s, sigma_s, tau)
    with torch.enable_grad():
        error = y - A(x_hat)
        norm = torch.linalg.vector_norm(error)
    grad = torch.autograd.grad(norm, x_t)[0]
    return x_s - zeta * grad


@torch.no_grad()
def pgdm_step(mean_fn, x_t: Tensor, t: Tensor, s: Tensor, eps: Tensor, y: Tensor, A: Op, A_inv: Op, eta: float = 0.0,
              schedule=vp_schedule) -> Tensor:
    alpha_s, sigma_s = schedule(s)
    alpha_t, sigma_t = schedule(t)
    tau = 1 - (alpha_t / alpha_s * sigma_s / sigma_t) ** 2
    tau = torch.clip(eta * tau, min=0, max=1)
    with torch.enable_grad():
        x_t = x_t.detach().requires_grad_()
        x_hat = mean_fn(x_t, t)
    x_s = _ddpm_part(x_hat, x_t, eps, alpha_t, sigma_t, alpha_s, sigma_s, tau)
    grad = A_inv(y) - A_inv(A(x_hat))
    grad = torch.autograd.grad(x_hat, x_t, grad)[0]
    return x_s + alpha_s * alpha_t * grad


def loop(step_fn, x: Tensor, eps: list, steps: int, **kw) -> Tensor:
    r"""``Sampler.__call__`` over ``steps`` steps with the noise of step k handed in as ``eps[k]``."""
    for (t, s), e in zip(time_pairs(steps=steps).to(x.dtype if x.dtype == torch.float64 else torch.float32), eps):
        x = step_fn(x_t=x, t=t, s=s, eps=e, **kw)
    return x


@torch.no_grad()
def tmpd_mean(mean_fn, x_t: Tensor, t: Tensor, y: Tensor, A: Op, var_y, schedule=vp_schedule) -> Tensor:
    alpha_t, sigma_t = schedule(t)
    gamma_t = sigma_t**2 / alpha_t
    with torch.enable_grad():
        x_t = x_t.detach().requires_grad_()
        x_hat = mean_fn(x_t, t)
        y_hat = A(x_hat)

    def At(v):
        return torch.autograd.grad(y_hat, x_hat, v, retain_graph=True)[0]

    def cov_x(v):
        return gamma_t * torch.autograd.grad(x_hat, x_t, v, retain_graph=True)[0]

    var_Ax = A(cov_x(At(torch.ones_like(y_hat))))
    grad = (y - y_hat) / (var_y + var_Ax)
    grad = gamma_t * torch.autograd.grad(y_hat, x_t, grad)[0]
    return x_hat + grad


@torch.no_grad()
def mmps_mean(mean_fn, x_t: Tensor, t: Tensor, y: Tensor, A: Op, cov_y: Op, solver: str = "gmres", iterations: int = 1,
              schedule=vp_schedule) -> Tensor:
    alpha_t, sigma_t = schedule(t)
    gamma_t = sigma_t**2 / alpha_t
    with torch.enable_grad():
        x_t = x_t.detach().requires_grad_()
        x_hat = mean_fn(x_t, t)
        y_hat = A(x_hat)

    def Av(v):
        return torch.func.jvp(A, (x_hat.detach(),), (v,))[1]

    def At(v):
        return torch.autograd.grad(y_hat, x_hat, v, retain_graph=True)[0]

    def cov_x(v):
        return gamma_t * torch.autograd.grad(x_hat, x_t, v, retain_graph=True)[0]

    def system(v):
        return cov_y(v) + Av(cov_x(At(v)))

    grad = y - y_hat
    grad = SOLVERS[solver](system, grad, iterations=iterations)
    grad = gamma_t * torch.autograd.grad(y_hat, x_t, grad)[0]
    return x_hat + grad


# ------------------------------------------------------------------------------------------------------------- operators
def mask_op(mask: Tensor):
    r"""(A, A_inv) of a pixel mask with the observation flattened to (B, D): A^+ = A^T (a projector)."""
    shape = mask.shape[1:]
    return (lambda x: (x * mask.to(x)).flatten(1)), (lambda y: y.unflatten(1, (-1, *shape[1:])) * mask.to(y))


def pool_op(H: int, W: int):
    r"""(A, A_inv) of 2x average pooling with the observation flattened: A^+ repeats every value over its 2 x 2 window."""
    A = lambda x: torch.nn.functional.avg_pool2d(x, 2).flatten(1)  # noqa: E731
    A_inv = lambda y: y.unflatten(1, (-1, H // 2, W // 2)).repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)  # noqa: E731
    return A, A_inv
