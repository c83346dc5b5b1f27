r"""Classifier-free guidance -- drop-in for ``azula.guidance.cfg`` (reference ``cfg.py:19-65``).

mu = mu(x_t | c+) + g * (mu(x_t | c+) - mu(x_t | c-)).  The reference makes two sequential,
un-batched denoiser calls and three elementwise passes; inside a fused sampler the two backbone
programs run back to back in the step graph and the combine is folded into the transition kernel
(``az_transition_f32`` with ``F_neg``), so guidance adds no pass over the latent.
"""

from __future__ import annotations

from typing import Any

import torch
from torch import Tensor

from .. import _lib
from ..denoise import Denoiser, DiracPosterior
from ..noise import Schedule

__all__ = ["CFGDenoiser"]


class CFGDenoiser(Denoiser):
    r"""Creates a CFG denoiser module around ``denoiser``."""

    def __init__(self, denoiser: Denoiser) -> None:
        super().__init__()
        self.denoiser = denoiser

    @property
    def schedule(self) -> Schedule:
        return self.denoiser.schedule

    @torch.no_grad()
    @_lib.on_device
    def forward(
        self,
        x_t: Tensor,
        t: Tensor,
        positive: dict[str, Any],
        negative: dict[str, Any] = {},  # noqa: B006
        guidance: float | Tensor = 1.0,
        **kwargs,
    ) -> DiracPosterior:
        q_pos = self.denoiser(x_t, t, **positive, **kwargs)
        q_neg = self.denoiser(x_t, t, **negative, **kwargs)
        if not x_t.is_cuda:  # host tensors: reference op sequence
            return DiracPosterior(mean=q_pos.mean + guidance * (q_pos.mean - q_neg.mean))
        if q_pos.mean.dtype == torch.float64:  # fp64 means (Sampler(dtype=float64)): pos + g * (pos - neg) in fp64
            from ..denoise import axpby_wide

            one = torch.ones((), dtype=torch.float64)
            diff = axpby_wide(one, q_pos.mean, -one, q_neg.mean)
            g64 = torch.as_tensor(guidance, dtype=torch.float64).reshape(())
            return DiracPosterior(mean=axpby_wide(one, q_pos.mean, g64, diff))
        pos, neg = q_pos.mean.contiguous(), q_neg.mean.contiguous()
        g = torch.as_tensor(guidance, dtype=torch.float32, device=x_t.device).reshape(1)
        mean = torch.empty_like(pos)
        _lib.call("az_cfg_combine_f32", mean.data_ptr(), pos.data_ptr(), neg.data_ptr(), g.data_ptr(), pos.numel(), _lib.stream_ptr())
        return DiracPosterior(mean=mean)

    # -- input gradient (azula_amd internal: the guidance classes that need d mean / d x_t) --------------------------
    @torch.no_grad()
    @_lib.on_device
    def _az_vjp(self, x_t: Tensor, t: Tensor, positive: dict[str, Any] | None = None, negative: dict[str, Any] = {},  # noqa: B006
                guidance: float | Tensor = 1.0, **kwargs):
        r"""``(mean, pullback)`` of the guided mean ``m = (1 + g) m+ - g m-``, evaluated the way the fused sampler evaluates it:
        ONE call of the inner denoiser's ``_az_vjp`` on the stacked batch ``[x_t ; x_t]`` with the labels ``[c+ ; c-]`` (one
        gradient plan, one forward-keep tape, one backward tape).  The halves of the mean meet in ``az_cfg_combine_f32``; the
        pullback is ``az_cfg_split_f32`` (``[(1 + g) v ; -g v]``), the inner pullback, and ``az_axpby_f32`` over the halves.
        ``positive`` / ``negative`` may hold only ``label`` (the rule of the fused CFG path); ``AZ_CFG_BATCHED`` does not apply."""
        from ..plugins.adm import AblatedDenoiser
        from ..plugins.jit import JITDenoiser

        if not x_t.is_cuda:
            raise NotImplementedError("CFGDenoiser: the input-gradient path of classifier-free guidance (CFG) runs on device tensors only")
        if positive is None:
            raise NotImplementedError("CFGDenoiser: the input-gradient path of classifier-free guidance (CFG) needs `positive`")
        inner = self.denoiser
        inner_vjp = getattr(inner, "_az_vjp", None)
        if inner_vjp is None:
            raise NotImplementedError(f"CFGDenoiser: the inner {type(inner).__name__} has no input-gradient path (_az_vjp) for "
                                      "classifier-free guidance (CFG) to stack")
        if kwargs or set(positive) - {"label"} or set(negative) - {"label"}:
            raise NotImplementedError("CFGDenoiser: the input-gradient path of classifier-free guidance (CFG) stacks the two "
                                      "evaluations on the labels alone: `positive` / `negative` may hold only `label`, and no "
                                      "further keyword arguments")
        B, dev = x_t.shape[0], x_t.device
        labels = [positive.get("label"), negative.get("label")]
        if isinstance(inner, JITDenoiser):  # a missing label is the null class
            labels = [torch.as_tensor(inner.num_classes) if lab is None else lab for lab in labels]
        elif isinstance(inner, AblatedDenoiser) and getattr(inner.backbone, "num_classes", None) is not None:
            if any(lab is None for lab in labels):
                raise NotImplementedError("CFGDenoiser: classifier-free guidance (CFG) on a class-conditional AblatedDenoiser needs "
                                          "a label in both `positive` and `negative`")
        else:
            raise NotImplementedError(f"CFGDenoiser: no stacked (CFG) input-gradient path around {type(inner).__name__}: a "
                                      "JITDenoiser or a class-conditional AblatedDenoiser provides it")
        label2 = torch.cat([torch.as_tensor(lab).to(device=dev, dtype=torch.int64).reshape(-1).expand(B) for lab in labels])
        x_t = x_t.detach().contiguous()
        t2 = t if t.numel() == 1 else torch.cat((t.reshape(-1), t.reshape(-1)))
        mean2, pull2 = inner_vjp(torch.cat((x_t, x_t)), t2, label=label2)
        mean2 = mean2.contiguous()
        n = mean2.numel() // 2
        g = torch.as_tensor(guidance, dtype=torch.float32, device=dev).reshape(1)
        mean = torch.empty_like(mean2[:B])
        _lib.call("az_cfg_combine_f32", mean.data_ptr(), mean2.data_ptr(), mean2.data_ptr() + 4 * n, g.data_ptr(), n, _lib.stream_ptr())
        one = torch.ones(1, dtype=torch.float32, device=dev)

        def pullback(v: Tensor) -> Tensor:
            v = v.detach().to(torch.float32).contiguous()
            assert v.shape == mean.shape
            with torch.cuda.device(dev):
                v2 = torch.empty_like(mean2)
                _lib.call("az_cfg_split_f32", v2.data_ptr(), v.data_ptr(), g.data_ptr(), n, _lib.stream_ptr())
                d2 = pull2(v2).contiguous()
                dx = torch.empty_like(x_t)
                m = dx.numel()
                _lib.call("az_axpby_f32", dx.data_ptr(), one.data_ptr(), d2.data_ptr(), one.data_ptr(), d2.data_ptr() + 4 * m, 1, m, 0,
                          _lib.stream_ptr())
            return dx

        return mean, pullback

    # -- fused sampling ---------------------------------------------------------------------------
    def _az_fused(self, x: Tensor, kwargs: dict, cur_coef: Tensor):
        from ..sample import FusedDenoiser

        inner = self.denoiser
        make = getattr(inner, "_az_programs", None)
        if make is None or set(kwargs) - {"positive", "negative", "guidance"} or "positive" not in kwargs:
            return None
        guidance = kwargs.get("guidance", 1.0)
        if torch.is_tensor(guidance):
            if guidance.numel() != 1:
                return None
            guidance = float(guidance)
        pos, neg = dict(kwargs["positive"]), dict(kwargs.get("negative", {}))
        programs = make(x, [pos, neg], cur_coef)
        if programs is None:
            return None
        # each program's prepare() looks up its own label set
        for i, p in enumerate(programs):
            orig = p.prepare

            def prepare(call_kwargs: dict, orig=orig, i=i) -> None:
                labels = {0: call_kwargs["positive"].get("label"), 1: call_kwargs.get("negative", {}).get("label")}
                orig({"_az_labels": labels})

            p.prepare = prepare
        return FusedDenoiser(
            coefficients=inner.host_coefficients, programs=programs, guidance=float(guidance), clip=inner._clip()
        )
