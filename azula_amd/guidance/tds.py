r"""Twisted diffusion sampler -- drop-in for ``azula.guidance.tds`` (reference ``tds.py:23-104``; Wu et al., 2023).

A sequential Monte Carlo sampler over ``K`` particles (the batch): every step weights the particles by the twisting function
``log p(y | x_hat, t)``, resamples them, proposes ``x_s`` from the twisted DDPM transition and reweights.  The reference
differentiates the twist through the network with torch autograd; here the twist's gradient with respect to ``x_hat`` is torch
autograd of the user's function at a detached ``x_hat`` and the network part is the HIP pullback of the denoiser
(``Denoiser._az_vjp``), as in :mod:`azula_amd.guidance.dps`.  Everything behind it -- the reference's four gathers by ancestor,
two ``Normal`` objects, one ``sample``, two ``log_prob`` and three per-particle reductions (``tds.py:70-102``) -- is two
kernels: ``az_tds_resample_f32`` (softmax weights and inverse-CDF multinomial resampling in one workgroup) and
``az_tds_propose_f32`` (one pass that gathers, proposes, samples and reweights, with the importance weight in a form that does
not cancel).  The sampler runs on the generic loop, with no captured plan.

Random stream: a step draws, in this order and nothing else, ``torch.rand(K)`` (the resampling uniforms) and
``torch.randn_like(x_t)`` (the proposal noise) from the device's default generator.  Resampling is multinomial with
replacement, as in the reference, but by inverse CDF on those uniforms: it does not reproduce ``torch.multinomial``'s stream.
"""

from __future__ import annotations

import ctypes as C
from collections.abc import Callable

import torch
from torch import Tensor

from .. import _lib
from ..denoise import Denoiser
from ..sample import Sampler
from ._vjp import mean_and_pullback

__all__ = ["TDSSampler"]

MAX_PARTICLES = 65536  # az_tds_resample_f32 keeps the whole CDF in one workgroup


class TDSSampler(Sampler):
    r"""Creates a TDS sampler.

    Arguments:
        denoiser: A denoiser :math:`q_\phi(X \mid X_t)`.
        twist: A twisting function :math:`\log p(y \mid \hat{x}, t)`, called as ``twist(x_hat, sigma_t / alpha_t)``.
        kwargs: Keyword arguments passed to :class:`azula_amd.sample.Sampler`.

    ``step`` keeps the log-weights of the proposal in ``carry["log_w"]`` as the reference does.  Additions of this port:
    ``carry["ancestors"]`` (int64, ``K``) and ``carry["w"]`` (float32, ``K``) hold the last resampling's ancestor indices and
    normalised weights (the effective sample size is ``1 / (w ** 2).sum()``).  If every weight is ``-inf`` or one is NaN the
    reference raises inside ``torch.multinomial``; here ``w`` is NaN and every particle keeps itself.
    """

    def __init__(self, denoiser: Denoiser, twist: Callable[[Tensor], Tensor], **kwargs) -> None:
        super().__init__(**kwargs)
        self.denoiser = denoiser
        self.twist = twist

    @torch.no_grad()
    def __call__(self, x: Tensor, **kwargs) -> Tensor:
        r"""Simulates the reverse process from :math:`t_T` to :math:`t_0` for the :math:`K` particles ``x`` (shape
        :math:`(K, *)`)."""
        return super().__call__(x, carry={}, **kwargs)

    @torch.no_grad()
    @_lib.on_device
    def step(self, x_t: Tensor, t: Tensor, s: Tensor, carry: dict, **kwargs) -> Tensor:
        who = type(self).__name__
        if self.shard is not None:
            raise NotImplementedError(f"{who}: the particles are coupled across the batch (resampling); a sharded batch is not supported")
        K = x_t.shape[0]
        if K > MAX_PARTICLES:
            raise ValueError(f"{who}: at most {MAX_PARTICLES} particles (got {K})")
        if getattr(self.denoiser, "_az_vjp", None) is None:
            mean_and_pullback(self.denoiser, x_t, t, kwargs)  # (raises: no input-gradient path)
        if not x_t.is_cuda or x_t.dtype != torch.float32:
            raise NotImplementedError(
                f"{who}: the resample / proposal kernels take fp32 device tensors only; got {x_t.dtype} on {x_t.device} and "
                "there is no eager fallback")

        alpha_s, sigma_s = self.denoiser.schedule(s)
        alpha_t, sigma_t = self.denoiser.schedule(t)

        x_t = x_t.detach().contiguous()
        x_hat, pullback = mean_and_pullback(self.denoiser, x_t, t, kwargs)

        with torch.enable_grad():
            x_hat = x_hat.detach().requires_grad_()
            log_p_y = self.twist(x_hat, sigma_t / alpha_t)
            grad = torch.autograd.grad(log_p_y.sum(), x_hat)[0]
        score_y = pullback(grad).contiguous()
        x_hat = x_hat.detach().contiguous()
        log_p_y = log_p_y.detach().reshape(K, -1).sum(dim=1).to(torch.float32).contiguous()

        dev = x_t.device
        u = torch.rand(K, dtype=torch.float32, device=dev)
        z = torch.randn_like(x_t)

        # Resample (tds.py:70-78)
        log_w = carry.get("log_w")
        ancestors = torch.empty(K, dtype=torch.int64, device=dev)
        w = torch.empty(K, dtype=torch.float32, device=dev)
        stream = _lib.stream_ptr()
        _lib.call("az_tds_resample_f32", _lib.ptr(log_p_y), None if log_w is None else _lib.ptr(log_w.contiguous()), _lib.ptr(u),
                  _lib.ptr(ancestors), _lib.ptr(w), K, stream)

        # Proposal and reweight (tds.py:80-102)
        tau = (alpha_t / alpha_s * sigma_s / sigma_t) ** 2
        scale = sigma_s * torch.sqrt(1 - tau)
        coef = torch.stack([alpha_t, alpha_s, sigma_t**2 / alpha_t, sigma_s * torch.sqrt(tau) / sigma_t, scale, 1 / scale])
        coef = coef.to(device=dev, dtype=torch.float32).contiguous()
        N = x_t.numel() // K
        chunks = _lib.lib().az_tds_chunks(K, N)
        x_s = torch.empty_like(x_t)
        log_w_next = torch.empty(K, dtype=torch.float32, device=dev)
        work = torch.empty(K * chunks, dtype=torch.float64, device=dev)
        a = _lib.AzTdsProposeArgs(
            x_t=_lib.ptr(x_t), x_hat=_lib.ptr(x_hat), score=_lib.ptr(score_y), z=_lib.ptr(z), ancestors=_lib.ptr(ancestors),
            log_p=_lib.ptr(log_p_y), coef=_lib.ptr(coef), x_s=_lib.ptr(x_s), log_w_next=_lib.ptr(log_w_next),
            workspace=work.data_ptr(), K=K, N=N, chunks=chunks,
        )
        _lib.call("az_tds_propose_f32", C.byref(a), stream)

        carry["log_w"] = log_w_next
        carry["ancestors"] = ancestors
        carry["w"] = w
        return x_s
