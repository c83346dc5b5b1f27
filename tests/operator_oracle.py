r"""Oracle: the measurement operators of ``azula_amd.guidance.operators`` restated as torch ops -- TEST INFRASTRUCTURE.

Written for the tests and sharing no code with the package: the mask is a multiplication, the pooling a reshape and a sum, the
blur a two-dimensional shift-and-add over the outer product of the tap vectors.  Adjoints come from torch autograd of these.
Usable in fp64 on the host (the reference of every comparison) and in fp32 on the device (what a user would write)."""

from __future__ import annotations

import torch
from torch import Tensor


def mask(x: Tensor, m: Tensor) -> Tensor:
    return x * m.to(x)


def pool(x: Tensor, fh: int, fw: int) -> Tensor:
    B, C, H, W = x.shape
    return x.reshape(B, C, H // fh, fh, W // fw, fw).sum(dim=(3, 5)) * (1.0 / (fh * fw))


def unpool(y: Tensor, fh: int, fw: int) -> Tensor:
    r"""Nearest up-sampling: every value repeated over its window (the pseudo-inverse of ``pool``)."""
    return y.repeat_interleave(fh, dim=2).repeat_interleave(fw, dim=3)


def blur(x: Tensor, taps_h: Tensor, taps_w: Tensor, circular: bool) -> Tensor:
    r"""y[i, j] = sum_{a, b} taps_h[a] taps_w[b] x~[i + a - rh, j + b - rw], one shifted copy of x per tap pair."""
    H, W = x.shape[2:]
    nh, nw = taps_h.numel(), taps_w.numel()
    rh, rw = nh // 2, nw // 2
    K = torch.outer(taps_h.to(x), taps_w.to(x))
    if not circular:
        xp = torch.zeros(*x.shape[:2], H + 2 * rh, W + 2 * rw, dtype=x.dtype, device=x.device)
        xp[:, :, rh:rh + H, rw:rw + W] = x
    y = torch.zeros_like(x)
    for a in range(nh):
        for b in range(nw):
            shifted = torch.roll(x, (rh - a, rw - b), (2, 3)) if circular else xp[:, :, a:a + H, b:b + W]
            y = y + K[a, b] * shifted
    return y


def adjoint(fn, x_shape, w: Tensor) -> Tensor:
    r"""``fn``'s transpose at ``w`` by autograd (``fn`` linear on tensors of ``x_shape``)."""
    with torch.enable_grad():
        x = torch.zeros(x_shape, dtype=w.dtype, device=w.device, requires_grad=True)
        return torch.autograd.grad(fn(x), x, w)[0]
