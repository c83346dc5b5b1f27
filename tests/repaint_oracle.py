r"""Oracle: the RePaint sampling loop (torch, the reference's op order) -- TEST INFRASTRUCTURE.

A functional restatement of ``RePaintSampler.step`` (azula/guidance/repaint.py:47-63) over the DDIM transition of
``oracle.sampling``: per step ``iterations`` times a DDIM step t -> s, the masked replacement of the observed pixels and the
re-noising back to t.  ``tools/make_golden_repaint.py`` asserts that it is bit-identical to the reference on CPU before it
writes ``tests/golden/g25_repaint.npz``; the GPU tests feed it the noise the device drew.
"""

from __future__ import annotations

from typing import Callable

import torch
from torch import Tensor

from oracle.sampling import time_pairs, transition, vp_schedule


def repaint_scalars(schedule, t: Tensor, s: Tensor) -> tuple[Tensor, Tensor, Tensor, Tensor]:
    r"""[alpha_s, sigma_s, alpha_t / alpha_s, alpha_t sqrt((sigma_t / alpha_t)^2 - (sigma_s / alpha_s)^2)] of one step."""
    alpha_s, sigma_s = schedule(s)
    alpha_t, sigma_t = schedule(t)
    return alpha_s, sigma_s, alpha_t / alpha_s, alpha_t * torch.sqrt((sigma_t / alpha_t) ** 2 - (sigma_s / alpha_s) ** 2)


def scalar_table(schedule=vp_schedule, steps: int = 64, start: float = 1.0, stop: float = 0.0, dtype=None) -> Tensor:
    r"""(steps, 4) of :func:`repaint_scalars`, in the time grid's dtype."""
    return torch.stack([torch.stack(repaint_scalars(schedule, t, s)) for t, s in time_pairs(start, stop, steps, dtype).unbind()])


def sample_repaint(
    mean_fn: Callable[..., Tensor],
    x: Tensor,
    y: Tensor,
    mask: Tensor,
    schedule=vp_schedule,
    steps: int = 64,
    iterations: int = 3,
    eta: float = 0.0,
    start: float = 1.0,
    stop: float = 0.0,
    dtype: torch.dtype | None = None,
    noise: list[Tensor] | None = None,
    record: list | None = None,
    **kwargs,
) -> Tensor:
    r"""The reverse loop of ``RePaintSampler`` (``azula/sample.py:139-161`` with ``repaint.py:47-63``).

    Generator calls per iteration, in order: the DDIM step's ``randn_like(x_t)`` (drawn even when eta = 0), ``randn_like(y)``,
    ``randn_like(x_s)`` (the last iteration's too, whose result is discarded).  ``noise`` replays such a sequence instead of
    drawing; ``record`` collects what was used."""
    feed = iter(noise) if noise is not None else None

    def draw(like: Tensor) -> Tensor:
        e = torch.randn_like(like) if feed is None else next(feed).to(like)
        if record is not None:
            record.append(e)
        return e

    x_t = x
    for t, s in time_pairs(start, stop, steps, dtype).unbind():
        alpha_s, sigma_s = schedule(s)
        alpha_t, sigma_t = schedule(t)
        for _ in range(iterations):
            mean = mean_fn(x_t, t, **kwargs)
            x_s = transition(x_t, mean, draw(x_t), alpha_t, sigma_t, alpha_s, sigma_s, eta)
            x_s = torch.where(mask, alpha_s * y + sigma_s * draw(y), x_s)
            x_t = alpha_t / alpha_s * x_s + alpha_t * torch.sqrt((sigma_t / alpha_t) ** 2 - (sigma_s / alpha_s) ** 2) * draw(x_s)
        x_t = x_s
    return x_t
