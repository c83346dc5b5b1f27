r"""What the gradient-based guidance methods share: the denoiser's posterior mean with its HIP pullback."""

from __future__ import annotations

from torch import Tensor

from ..denoise import Denoiser


def mean_and_pullback(denoiser: Denoiser, x_t: Tensor, t: Tensor, kwargs: dict):
    r"""``(x_hat, pullback)`` with ``pullback(v) = (d x_hat / d x_t)^T v`` through the denoiser's ``_az_vjp`` protocol (the
    backbone's backward tape of HIP kernels).  The reference takes this product from ``torch.autograd``; the backbones here
    are kernel tapes without an autograd graph, so a denoiser without the protocol is an error, never an eager fallback."""
    vjp = getattr(denoiser, "_az_vjp", None)
    if vjp is None:
        raise NotImplementedError(
            f"{type(denoiser).__name__} has no input-gradient path (_az_vjp): KarrasDenoiser / SimpleDenoiser around an "
            "azula_amd.nn.UNet or DiT, the ADM plugin's AblatedDenoiser, the JiT plugin's JITDenoiser, and CFGDenoiser around the "
            "last two, provide it")
    return vjp(x_t, t, **kwargs)
