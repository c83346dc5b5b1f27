r"""Velocity diffusion model (VDM) plugin -- drop-in for ``azula.plugins.vdm`` (Katherine Crowson's v-diffusion models).

    from azula_amd.plugins import vdm
    denoiser = vdm.load_model("imagenet_128x128").to("cuda")     # needs the checkpoint in the hub cache
    denoiser = vdm.make_model("imagenet_128").to("cuda")         # random init

``VelocityDenoiser`` wraps a network that predicts the velocity v = alpha eps - sigma x (reference
``azula/plugins/vdm/__init__.py:32-77``):

    mu(x_t) = c_skip x_t + c_out F(c_in x_t, c_time),   r = rsqrt(alpha_t^2 + sigma_t^2),
    c_in = r,  c_out = -sigma_t r,  c_skip = alpha_t r,  c_time = atan2(sigma_t, alpha_t) 2 / pi

In a fused sampler this is the transition kernel's Karras form; the backbone is :class:`VDMModel` compiled onto the convolution,
attention and pooling kernels (``model.VDMPlan``), its time planes written per step from ``AzStepCoef.c_time``.

Out of scope: ``cc12m_1`` / ``cc12m_1_cfg`` (CLIP-conditioned, no card), half-precision backbones, the input gradient
(``_az_vjp``: the gradient-guidance samplers raise their usual error on a ``VelocityDenoiser``).
"""

from __future__ import annotations

import math

import torch
import torch.nn as nn
from torch import Tensor

from ... import _lib
from ...denoise import (Denoiser, DiracPosterior, _expand_like, axpby_wide, is_wide, postcondition, precondition, precondition_wide,
                        require_f32_cuda)
from ...hub import download
from ...nn.utils import get_module_dtype, skip_init
from ...noise import Schedule, VPSchedule
from ..utils import load_cards
from .model import ARCHITECTURES, VDMModel

__all__ = ["VelocityDenoiser", "VDMModel", "load_model", "make_model", "load_cards"]


def velocity_coefficients(alpha_t: Tensor, sigma_t: Tensor):
    r"""(c_in, c_out, c_skip, c_time) in the reference's op order (``plugins/vdm/__init__.py:61-64``)."""
    c_in = torch.rsqrt(alpha_t**2 + sigma_t**2)
    c_out = -sigma_t * torch.rsqrt(alpha_t**2 + sigma_t**2)
    c_skip = alpha_t * torch.rsqrt(alpha_t**2 + sigma_t**2)
    c_time = torch.atan2(sigma_t, alpha_t).flatten() / math.pi * 2
    return c_in, c_out, c_skip, c_time


class VelocityDenoiser(Denoiser):
    r"""Velocity denoiser.  ``schedule=None`` selects ``VPSchedule(alpha_min=1e-2, sigma_min=1e-2)``."""

    def __init__(self, backbone: nn.Module, schedule: Schedule | None = None) -> None:
        super().__init__()
        self.backbone = backbone
        self.schedule = VPSchedule(alpha_min=1e-2, sigma_min=1e-2) if schedule is None else schedule

    @torch.no_grad()
    @_lib.on_device
    def forward(self, x_t: Tensor, t: Tensor, **kwargs) -> DiracPosterior:
        alpha_t, sigma_t = self.schedule(t)
        alpha_t, sigma_t = _expand_like(alpha_t, x_t.ndim), _expand_like(sigma_t, x_t.ndim)
        c_in, c_out, c_skip, c_time = velocity_coefficients(alpha_t, sigma_t)
        dtype = get_module_dtype(self.backbone) or x_t.dtype
        if not x_t.is_cuda:
            raise RuntimeError("azula_amd VDM denoisers execute only on an AMD GPU (no CPU fallback)")
        dev = x_t.device
        if is_wide(x_t, alpha_t):  # fp64 time grid / latents: fp64 elementwise path around the fp32 backbone
            x_in = precondition_wide(x_t, c_in)
            output = self.backbone(x_in.to(dtype), c_time.to(device=dev, dtype=dtype), **kwargs).to(x_t.dtype)
            return DiracPosterior(mean=axpby_wide(c_skip, x_t, c_out, output))
        require_f32_cuda(x_t, "VelocityDenoiser")
        x_t = x_t.contiguous()
        x_in = precondition(x_t, c_in.to(dev))
        output = self.backbone(x_in.to(dtype), c_time.to(device=dev, dtype=dtype), **kwargs).to(x_t).contiguous()
        return DiracPosterior(mean=postcondition(x_t, output, c_skip.to(dev), c_out.to(dev)))

    # -- fused sampling -------------------------------------------------------------------------
    def host_coefficients(self, alpha_t: Tensor, sigma_t: Tensor) -> dict:
        c_in, c_out, c_skip, c_time = velocity_coefficients(alpha_t, sigma_t)
        return {"c_in": c_in, "c_out": c_out, "c_skip": c_skip, "c_time": c_time.reshape(())}

    def _az_programs(self, x: Tensor, kwargs_list: list[dict], cur_coef: Tensor):
        r"""One compiled backbone program: the transition kernel leaves ``c_in' x_s`` in channels 0..2 of the stem's NHWC input,
        the program's first launch fills the time planes from the current step's ``c_time``."""
        bb = self.backbone
        if not isinstance(bb, VDMModel) or x.ndim != 4 or x.shape[1] != 3 or get_module_dtype(bb) != torch.float32:
            return None
        if len(kwargs_list) != 1 or kwargs_list[0]:
            return None  # (the six public models are unconditional: keyword arguments run the generic loop, which rejects them)
        B, _, H, W = x.shape
        plan = bb.plan(B, H, W, x.device, coef_ptr=cur_coef.data_ptr())
        # wide = True: under an fp64 clock the loop converts the fp64 latent into this fp32 input itself and still fills the
        # fp32 coefficient row the time planes read
        return [plan.program(bb.out_channels, wide=True)]

    def _az_fused(self, x: Tensor, kwargs: dict, cur_coef: Tensor):
        from ...sample import FusedDenoiser

        programs = self._az_programs(x, [kwargs], cur_coef)
        if programs is None:
            return None
        return FusedDenoiser(coefficients=self.host_coefficients, programs=programs)


def load_model(name: str, **kwargs) -> Denoiser:
    r"""A pre-trained VDM denoiser by card name, in eval mode (counterpart of the reference's ``plugins/vdm/__init__.py:80-100``).
    The checkpoint must already be in the hub cache: ``azula_amd.hub.download`` resolves an existing entry or raises, it never
    downloads.  ``kwargs`` go to ``torch.load`` (defaults: CPU tensors, ``weights_only``)."""
    cards = load_cards(__name__)
    if name not in cards:
        raise KeyError(f"vdm: no card {name!r}; one of {sorted(cards)}")
    card = cards[name]
    path = download(card.url, hash_prefix=card.hash)
    state = torch.load(path, **{"map_location": "cpu", "weights_only": True, **kwargs})
    with skip_init():  # (every parameter is overwritten by the checkpoint)
        denoiser = make_model(**card.config)
    denoiser.backbone.load_state_dict(state, strict=True)
    denoiser.eval()
    return denoiser


def make_model(model: str = "imagenet_128", **kwargs) -> Denoiser:
    r"""Initialises a VDM denoiser (reference ``plugins/vdm/__init__.py:103-110``).  ``base_channels=...`` narrows the network."""
    return VelocityDenoiser(VDMModel(model, **kwargs))
