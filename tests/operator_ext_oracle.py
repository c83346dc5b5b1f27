r"""Oracle: the PSF, decimation and channel-mix operators of ``azula_amd.guidance.operators`` restated as torch ops -- TEST
INFRASTRUCTURE.

Written for the tests and sharing no code with the package: the PSF is a shift-and-add with one shifted copy of x per tap (as
``operator_oracle.blur``), the decimation a strided slice, the channel mix an einsum.  Adjoints come from
``operator_oracle.adjoint`` (torch autograd of these).  Usable in fp64 on the host (the reference of every comparison) and in fp32
on the device (what a user would write)."""

from __future__ import annotations

import torch
from torch import Tensor


def psf(x: Tensor, k: Tensor, circular: bool) -> Tensor:
    r"""y[b, c, i, j] = sum_{a, b'} k[b, c, a, b'] x~[b, c, i + a - rh, j + b' - rw]; ``k`` broadcastable to (B, C, kh, kw)."""
    H, W = x.shape[2:]
    k = k.to(x)
    k = k.reshape((1,) * (4 - k.ndim) + tuple(k.shape))
    kh, kw = k.shape[2:]
    rh, rw = kh // 2, kw // 2
    y = torch.zeros_like(x)
    for a in range(kh):
        for b in range(kw):
            if circular:
                shifted = torch.roll(x, (rh - a, rw - b), (2, 3))
            elif abs(rh - a) >= H or abs(rw - b) >= W:
                continue  # (the image shifted out of its own frame: this tap meets zeros only)
            else:  # x moved down by rh - a and right by rw - b, zeros moving in (a negative pad crops)
                shifted = torch.nn.functional.pad(x, (rw - b, b - rw, rh - a, a - rh))
            y = y + k[:, :, a:a + 1, b:b + 1] * shifted
    return y


def decimate(x: Tensor, fh: int, fw: int, oh: int, ow: int) -> Tensor:
    return x[:, :, oh::fh, ow::fw]


def zero_stuff(y: Tensor, fh: int, fw: int, oh: int, ow: int) -> Tensor:
    r"""The values of ``y`` at (i fh + oh, j fw + ow) of a grid of zeros."""
    B, C, h, w = y.shape
    out = torch.zeros(B, C, h * fh, w * fw, dtype=y.dtype, device=y.device)
    out[:, :, oh::fh, ow::fw] = y
    return out


def mix(x: Tensor, M: Tensor) -> Tensor:
    return torch.einsum("oc,bchw->bohw", M.to(x), x)
