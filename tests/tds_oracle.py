r"""Oracle: the twisted diffusion sampler (torch, the reference's op order) -- TEST INFRASTRUCTURE.

A functional restatement of ``TDSSampler.step`` (``azula/guidance/tds.py:57-104``) over a posterior-mean function that torch
can differentiate, written from the mathematics of Wu et al. (2023) and the reference's behaviour: the twist's score through
the network, softmax weights, multinomial resampling, the twisted DDPM proposal and the importance weight as the difference of
two summed Gaussian log-densities.  It works in the dtype of its inputs (fp32 for the host tests, fp64 as the reference of
the GPU tests).  ``ancestors`` and ``eps`` are used when given; when not, the step draws with ``torch.multinomial`` and
``torch.normal`` exactly where the reference does, so that under one CPU seed it is bit-identical to the reference
(``tools/make_golden_tds.py`` asserts it before it writes ``tests/golden/g29_tds.npz``).
"""

from __future__ import annotations

import math
from typing import Callable

import torch
from torch import Tensor

from oracle.sampling import time_pairs, vp_schedule

Op = Callable[[Tensor], Tensor]


def gaussian_twist(y: Tensor, A: Op, var_y: float):
    r"""``log p(y | x_hat, lam) = -(y - A(x_hat))^2 / (2 (var_y + lam^2))``, un-summed: shape (K, D)."""

    def twist(x_hat: Tensor, lam: Tensor) -> Tensor:
        return -((y - A(x_hat)) ** 2) / (2 * (var_y + lam**2))

    return twist


def _per_particle(v: Tensor) -> Tensor:
    return v.sum(dim=tuple(range(1, v.ndim))) if v.ndim > 1 else v


def _normal_log_prob(x: Tensor, loc: Tensor, scale: Tensor) -> Tensor:
    r"""log N(x; loc, scale^2) = -(x - loc)^2 / (2 scale^2) - log scale - log sqrt(2 pi)."""
    scale = scale.expand(loc.shape)
    return -((x - loc) ** 2) / (2 * scale**2) - scale.log() - math.log(math.sqrt(2 * math.pi))


@torch.no_grad()
def tds_step(mean_fn, twist, x_t: Tensor, t: Tensor, s: Tensor, carry: dict, ancestors: Tensor | None = None,
             eps: Tensor | None = None, schedule=vp_schedule) -> Tensor:
    r"""One step; ``carry`` holds ``log_w`` between steps and, after the step, what the step chose (``ancestors``, ``w``,
    ``log_p``: the summed twist before the gather)."""
    alpha_s, sigma_s = schedule(s)
    alpha_t, sigma_t = schedule(t)
    with torch.enable_grad():
        x_t = x_t.detach().requires_grad_()
        x_hat = mean_fn(x_t, t)
        log_p_y = twist(x_hat, sigma_t / alpha_t)
        score_y = torch.autograd.grad(log_p_y.sum(), x_t)[0]
    x_t, x_hat, log_p_y = x_t.detach(), x_hat.detach(), log_p_y.detach()

    # resample
    log_p_y = _per_particle(log_p_y)
    log_w = log_p_y + carry["log_w"] if "log_w" in carry else log_p_y
    w = torch.softmax(log_w, dim=0)
    k = torch.multinomial(w, len(w), replacement=True) if ancestors is None else ancestors
    carry["ancestors"], carry["w"], carry["log_p"] = k, w, log_p_y
    x_t, x_hat, log_p_y, score_y = x_t[k], x_hat[k], log_p_y[k], score_y[k]

    # twisted DDPM proposal
    tau = (alpha_t / alpha_s * sigma_s / sigma_t) ** 2
    scale = sigma_s * torch.sqrt(1 - tau)

    def loc_of(x: Tensor) -> Tensor:
        e = (x_t - alpha_t * x) / sigma_t
        return alpha_s * x + sigma_s * torch.sqrt(tau) * e

    loc = loc_of(x_hat)
    loc_y = loc_of(x_hat + sigma_t**2 / alpha_t * score_y)
    if eps is None:
        x_s = torch.normal(loc_y, scale.expand(loc_y.shape))
    else:
        x_s = loc_y + scale * eps

    # reweight
    log_q = _per_particle(_normal_log_prob(x_s, loc, scale))
    log_q_y = _per_particle(_normal_log_prob(x_s, loc_y, scale))
    carry["log_w"] = log_q - log_q_y - log_p_y
    return x_s


def tds_loop(mean_fn, twist, x: Tensor, steps: int, ancestors: list | None = None, eps: list | None = None):
    r"""``TDSSampler.__call__`` over ``steps`` steps: ``(x, [per-step dict of x_s, log_w, ancestors, w, log_p])``."""
    carry: dict = {}
    trace = []
    pairs = time_pairs(steps=steps).to(x.dtype if x.dtype == torch.float64 else torch.float32)
    for n, (t, s) in enumerate(pairs):
        x = tds_step(mean_fn, twist, x, t, s, carry, None if ancestors is None else ancestors[n], None if eps is None else eps[n])
        trace.append({"x_s": x, "log_w": carry["log_w"], "ancestors": carry["ancestors"], "w": carry["w"], "log_p": carry["log_p"]})
    return x, trace


def inverse_cdf(log_w: Tensor, u: Tensor):
    r"""fp64 ``(ancestors, w, cdf)`` of multinomial resampling by inverse CDF: ``ancestors[j] = min{ i : c_i > u_j }``."""
    w = torch.softmax(log_w.double(), dim=0)
    c = torch.cumsum(w, dim=0)
    k = torch.searchsorted(c, u.double(), right=True).clamp(max=len(w) - 1)
    return k, w, c


def cdf_margin(c: Tensor, u: Tensor) -> Tensor:
    r"""Per uniform: its distance to the nearest CDF value."""
    return (u.double()[:, None] - c[None, :]).abs().min(dim=1).values
