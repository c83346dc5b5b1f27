r"""Denoisers and posteriors -- drop-in for ``azula.denoise`` on the sampling path.

``Denoiser.forward(x_t, t, **kwargs) -> Posterior`` with ``.mean`` shaped like ``x_t`` and an
attribute/property ``schedule`` (reference ``azula/denoise.py:97-114``).

Device tensors: the preconditioning arithmetic runs in HIP kernels through the C ABI
(``az_scale_f32``, ``az_axpby_f32``); inside a sampler it is fused with the transition
(``az_transition_f32``) and never exists as separate passes.  Host tensors (the reference's
CPU-runnable README configuration) take the reference's own op sequence in torch.
"""

from __future__ import annotations

import abc
import ctypes as C
import math

import torch
import torch.nn as nn
from torch import Tensor

from . import _lib
from .nn.utils import get_module_dtype
from .noise import Schedule

__all__ = [
    "Posterior", "DiracPosterior", "GaussianPosterior", "Denoiser", "GaussianDenoiser", "SimpleDenoiser", "KarrasDenoiser",
]


class Posterior(abc.ABC):
    r"""Abstract posterior q(X | x_t) (reference ``azula/denoise.py:50-53``)."""

    mean: Tensor


class DiracPosterior(Posterior):
    r"""Dirac delta at ``mean`` (reference ``azula/denoise.py:56-66``)."""

    def __init__(self, mean: Tensor) -> None:
        self.mean = mean


class GaussianPosterior(Posterior):
    r"""N(mean, var) with elementwise variance (reference ``azula/denoise.py:69-94``)."""

    def __init__(self, mean: Tensor, var: Tensor) -> None:
        self.mean = mean
        self.var = var

    def log_prob(self, x: Tensor) -> Tensor:
        return -((x - self.mean) ** 2 / self.var + torch.log(self.var) + math.log(2 * math.pi)) / 2


class Denoiser(nn.Module):
    r"""Abstract denoiser module (reference ``azula/denoise.py:97-114``)."""

    schedule: Schedule

    @abc.abstractmethod
    def forward(self, x_t: Tensor, t: Tensor, **kwargs) -> Posterior:
        r"""x_t: (B, *), t: () or (B) -> posterior."""

    # -- fused sampling protocol (azula_amd internal) ---------------------------------------------
    def _az_fused(self, x: Tensor, kwargs: dict, cur_coef: Tensor):
        r"""Returns a :class:`azula_amd.sample.FusedDenoiser` if this denoiser can run inside the
        captured per-step graph, else ``None`` (generic step-by-step path)."""
        return None

    def _az_fused_key(self) -> tuple:
        r"""Identity of the state a compiled program reads that is neither a parameter nor a buffer (part of the sampler's
        plan key)."""
        return ()


def _expand_like(a: Tensor, ndim: int) -> Tensor:
    while a.ndim < ndim:
        a = a[..., None]
    return a


def require_f32_cuda(x: Tensor, who: str) -> None:
    if x.dtype != torch.float32:
        raise NotImplementedError(
            f"{who}: the gfx950 kernels are fp32; got a {x.dtype} device tensor and there is no eager fallback"
        )


def karras_coefficients(alpha_t: Tensor, sigma_t: Tensor):
    r"""(c_in, c_out, c_skip, c_time) in the reference's op order (``azula/denoise.py:309-312``)."""
    c_in = torch.rsqrt(alpha_t**2 + sigma_t**2)
    c_out = sigma_t * torch.rsqrt(alpha_t**2 + sigma_t**2)
    c_skip = alpha_t / (alpha_t**2 + sigma_t**2)
    c_time = torch.log(sigma_t / alpha_t)
    return c_in, c_out, c_skip, c_time


def is_wide(*tensors: Tensor) -> bool:
    r"""True if torch's type promotion makes the elementwise path fp64: a DIMENSIONED fp64 tensor takes part (0-d
    tensors do not promote).  ``Sampler(dtype=float64)`` gets there through the schedule scalars, which the denoisers
    expand to shape (1, ..., 1) before multiplying them into x_t (reference ``azula/denoise.py:306-322``)."""
    return any(t.dtype == torch.float64 and t.ndim > 0 for t in tensors)


def _dev64(c: Tensor, device) -> Tensor:
    return c.reshape(-1).to(device=device, dtype=torch.float64).contiguous()


def precondition_wide(x_t: Tensor, c_in: Tensor) -> Tensor:
    r"""``(c_in * x_t).to(float32)`` with the product taken in fp64 (``az_scale_f64_to_f32``)."""
    x64 = x_t.to(torch.float64).contiguous()
    c = _dev64(c_in, x_t.device)
    rows = x_t.shape[0] if c.numel() > 1 else 1
    y = torch.empty(x_t.shape, dtype=torch.float32, device=x_t.device)
    _lib.call("az_scale_f64_to_f32", y.data_ptr(), x64.data_ptr(), c.data_ptr(), rows, x64.numel() // rows,
              1 if c.numel() > 1 else 0, _lib.stream_ptr())
    return y


def axpby_wide(a: Tensor, x: Tensor, b: Tensor, z: Tensor) -> Tensor:
    r"""a * x + b * z in fp64 (``az_axpby_f64``); ``z`` may be fp32 (widened element by element, as torch does)."""
    x64 = x.to(torch.float64).contiguous()
    z = z.contiguous() if z.dtype in (torch.float32, torch.float64) else z.to(torch.float32).contiguous()
    a64, b64 = _dev64(a, x.device), _dev64(b, x.device)
    rows = x.shape[0] if a64.numel() > 1 else 1
    y = torch.empty_like(x64)
    _lib.call("az_axpby_f64", y.data_ptr(), a64.data_ptr(), x64.data_ptr(), b64.data_ptr(), z.data_ptr(),
              int(z.dtype == torch.float32), rows, x64.numel() // rows, 1 if a64.numel() > 1 else 0, _lib.stream_ptr())
    return y


def precondition(x_t: Tensor, c_in: Tensor) -> Tensor:
    r"""c_in * x_t on the device (reference ``azula/denoise.py:317``); c_in is () or (B,)."""
    B = x_t.shape[0] if c_in.numel() > 1 else 1
    y = torch.empty_like(x_t)
    c = c_in.reshape(-1).to(torch.float32).contiguous()
    zero = torch.zeros_like(c)
    # y = c * x + 0 * x  (exact: adding a signed zero leaves every finite value unchanged)
    _lib.call(
        "az_axpby_f32", y.data_ptr(), c.data_ptr(), x_t.data_ptr(), zero.data_ptr(), x_t.data_ptr(),
        B, x_t.numel() // B, 1 if c.numel() > 1 else 0, _lib.stream_ptr(),
    )
    return y


def postcondition(x_t: Tensor, out: Tensor, c_skip: Tensor, c_out: Tensor) -> Tensor:
    r"""c_skip * x_t + c_out * out on the device (reference ``azula/denoise.py:322``)."""
    B = x_t.shape[0] if c_skip.numel() > 1 else 1
    y = torch.empty_like(x_t)
    a = c_skip.reshape(-1).to(torch.float32).contiguous()
    b = c_out.reshape(-1).to(torch.float32).contiguous()
    _lib.call(
        "az_axpby_f32", y.data_ptr(), a.data_ptr(), x_t.data_ptr(), b.data_ptr(), out.data_ptr(),
        B, x_t.numel() // B, 1 if a.numel() > 1 else 0, _lib.stream_ptr(),
    )
    return y


def _vjp_preconditioned(den: "Denoiser", x_t: Tensor, c_in: Tensor, c_out: Tensor | None, c_skip: Tensor | None, c_time: Tensor,
                        kwargs: dict):
    r"""mean = c_skip x_t + c_out F(c_in x_t, c_time) and its pullback v -> c_skip v + c_in c_out J_F^T v (``c_out`` /
    ``c_skip`` None: mean = F(c_in x_t, c_time)).  ``F``'s pullback is the backbone's ``vjp`` (HIP tapes); the elementwise parts
    are the preconditioning kernels of the forward.  No torch fallback: a backbone without ``vjp`` is an error."""
    backbone = den.backbone
    if not x_t.is_cuda:
        raise NotImplementedError(f"{type(den).__name__}: the input-gradient path runs on device tensors only")
    vjp = getattr(backbone, "vjp", None)
    if vjp is None:
        raise NotImplementedError(
            f"{type(den).__name__}: the backbone {type(backbone).__name__} has no input-gradient (vjp) path on the HIP kernels "
            "(available: azula_amd.nn.UNet, UNetBlock, DiT, DiTBlock, MultiheadSelfAttention and TimeModulated around them, the ADM "
            "plugin's UNetModel and the JiT plugin's JiT, also under CFGDenoiser); "
            "there is no torch fallback on device tensors")
    if get_module_dtype(backbone) not in (None, torch.float32):
        raise NotImplementedError(f"{type(den).__name__}: the input-gradient path takes fp32 backbones only")
    require_f32_cuda(x_t, type(den).__name__)
    x_t = x_t.detach().contiguous()
    x_in = precondition(x_t, c_in)
    output, pull = vjp(x_in, c_time.to(device=x_t.device, dtype=torch.float32), **kwargs)
    output = output.contiguous()
    mean = output if c_out is None else postcondition(x_t, output, c_skip, c_out)
    scale = c_in if c_out is None else c_in * c_out

    def pullback(v: Tensor) -> Tensor:
        v = v.detach().to(torch.float32).contiguous()
        jv = pull(v).contiguous()
        if c_skip is None:
            return precondition(jv, scale)
        return postcondition(v, jv, c_skip, scale)

    return mean, pullback


class KarrasDenoiser(Denoiser):
    r"""EDM-style preconditioned denoiser (reference ``azula/denoise.py:263-324``).

    mu(x_t) = c_skip x_t + c_out F(c_in x_t, c_time),  with
    c_in = rsqrt(a^2 + s^2), c_out = s c_in, c_skip = a / (a^2 + s^2), c_time = log(s / a).
    """

    def __init__(self, backbone: nn.Module, schedule: Schedule) -> None:
        super().__init__()
        self.backbone = backbone
        self.schedule = schedule

    @torch.no_grad()
    @_lib.on_device
    def forward(self, x_t: Tensor, t: Tensor, **kwargs) -> DiracPosterior:
        alpha_t, sigma_t = self.schedule(t)
        alpha_t, sigma_t = _expand_like(alpha_t, x_t.ndim), _expand_like(sigma_t, x_t.ndim)
        c_in, c_out, c_skip, c_time = karras_coefficients(alpha_t, sigma_t)
        c_time = c_time.reshape_as(t)
        dtype = get_module_dtype(self.backbone) or x_t.dtype

        if not x_t.is_cuda:  # host tensors: the reference's op sequence (README CPU configuration)
            output = self.backbone((c_in * x_t).to(dtype), c_time.to(dtype), **kwargs).to(x_t)
            return DiracPosterior(mean=c_skip * x_t + c_out * output)

        if is_wide(x_t, alpha_t):  # fp64 time grid and / or fp64 latents: the elementwise path is fp64 (see is_wide)
            x_in = precondition_wide(x_t, c_in)
            output = self.backbone(x_in.to(dtype), c_time.to(device=x_t.device, dtype=dtype), **kwargs)
            output = output.to(x_t.dtype)  # .to(x_t): the latents' dtype, before the fp64 scalars promote the sum
            return DiracPosterior(mean=axpby_wide(c_skip, x_t, c_out, output))
        require_f32_cuda(x_t, "KarrasDenoiser")
        x_t = x_t.contiguous()
        x_in = precondition(x_t, c_in.to(x_t.device))
        output = self.backbone(x_in.to(dtype), c_time.to(device=x_t.device, dtype=dtype), **kwargs)
        output = output.to(x_t).contiguous()
        return DiracPosterior(mean=postcondition(x_t, output, c_skip.to(x_t.device), c_out.to(x_t.device)))

    # -- input gradient (azula_amd internal: the guidance classes that need d mean / d x_t) ------------------
    @torch.no_grad()
    @_lib.on_device
    def _az_vjp(self, x_t: Tensor, t: Tensor, **kwargs):
        r"""``(mean, pullback)`` with ``pullback(v) = (d mean / d x_t)^T v = c_skip v + c_in c_out J_F^T v``: the backbone's
        HIP pullback between the preconditioning kernels.  A backbone without ``vjp`` raises ``NotImplementedError``."""
        alpha_t, sigma_t = self.schedule(t)
        alpha_t, sigma_t = _expand_like(alpha_t, x_t.ndim), _expand_like(sigma_t, x_t.ndim)
        c_in, c_out, c_skip, c_time = karras_coefficients(alpha_t, sigma_t)
        return _vjp_preconditioned(self, x_t, c_in.to(x_t.device), c_out.to(x_t.device), c_skip.to(x_t.device), c_time.reshape_as(t), kwargs)

    # -- fused sampling -------------------------------------------------------------------------
    def host_coefficients(self, alpha_t: Tensor, sigma_t: Tensor) -> dict:
        r"""Per-step scalars for the device table, from 0-d HOST tensors (reference op order)."""
        c_in, c_out, c_skip, c_time = karras_coefficients(alpha_t, sigma_t)
        return {"c_in": c_in, "c_out": c_out, "c_skip": c_skip, "c_time": c_time}

    def _az_fused(self, x: Tensor, kwargs: dict, cur_coef: Tensor):
        compile_ = getattr(self.backbone, "_az_compile", None)
        if compile_ is None or get_module_dtype(self.backbone) not in (None, torch.float32, torch.float16, torch.bfloat16):
            return None
        program = compile_(x, kwargs, cur_coef)
        if program is None:
            return None
        from .sample import FusedDenoiser

        return FusedDenoiser(coefficients=self.host_coefficients, programs=[program])


class SimpleDenoiser(Denoiser):
    r"""Denoiser whose backbone predicts the mean directly (reference ``azula/denoise.py:177-230``):
    mu(x_t) = F(c_in x_t, c_time) with c_in = rsqrt(a^2 + s^2), c_time = log(s / a).  In the fused step it
    is the Karras form with c_skip = 0, c_out = 1 (0 * x + 1 * F is exact in fp32)."""

    def __init__(self, backbone: nn.Module, schedule: Schedule) -> None:
        super().__init__()
        self.backbone = backbone
        self.schedule = schedule

    @torch.no_grad()
    @_lib.on_device
    def forward(self, x_t: Tensor, t: Tensor, **kwargs) -> DiracPosterior:
        alpha_t, sigma_t = self.schedule(t)
        alpha_t, sigma_t = _expand_like(alpha_t, x_t.ndim), _expand_like(sigma_t, x_t.ndim)
        c_in = torch.rsqrt(alpha_t**2 + sigma_t**2)
        c_time = torch.log(sigma_t / alpha_t).reshape_as(t)
        dtype = get_module_dtype(self.backbone) or x_t.dtype
        if not x_t.is_cuda:
            return DiracPosterior(mean=self.backbone((c_in * x_t).to(dtype), c_time.to(dtype), **kwargs).to(x_t))
        if is_wide(x_t, alpha_t):
            x_in = precondition_wide(x_t, c_in)
            output = self.backbone(x_in.to(dtype), c_time.to(device=x_t.device, dtype=dtype), **kwargs)
            return DiracPosterior(mean=output.to(x_t))
        require_f32_cuda(x_t, "SimpleDenoiser")
        x_in = precondition(x_t.contiguous(), c_in.to(x_t.device))
        output = self.backbone(x_in.to(dtype), c_time.to(device=x_t.device, dtype=dtype), **kwargs)
        return DiracPosterior(mean=output.to(x_t))

    @torch.no_grad()
    @_lib.on_device
    def _az_vjp(self, x_t: Tensor, t: Tensor, **kwargs):
        r"""``(mean, pullback)`` with ``pullback(v) = c_in J_F^T v`` (the Karras form with c_skip = 0, c_out = 1)."""
        alpha_t, sigma_t = self.schedule(t)
        alpha_t, sigma_t = _expand_like(alpha_t, x_t.ndim), _expand_like(sigma_t, x_t.ndim)
        c_in = torch.rsqrt(alpha_t**2 + sigma_t**2).to(x_t.device)
        c_time = torch.log(sigma_t / alpha_t).reshape_as(t)
        return _vjp_preconditioned(self, x_t, c_in, None, None, c_time, kwargs)

    def host_coefficients(self, alpha_t: Tensor, sigma_t: Tensor) -> dict:
        c_in = torch.rsqrt(alpha_t**2 + sigma_t**2)
        return {"c_in": c_in, "c_out": torch.ones_like(c_in), "c_skip": torch.zeros_like(c_in),
                "c_time": torch.log(sigma_t / alpha_t)}

    _az_fused = KarrasDenoiser._az_fused


# --------------------------------------------------------------------------------------------------------- Gaussian
def _cov_key(obj) -> tuple:
    r"""(type, address / version / shape / dtype of every tensor, value of every number) of a covariance, recursively."""
    if torch.is_tensor(obj):
        return ("T", obj.data_ptr(), obj._version, tuple(obj.shape), str(obj.dtype), str(obj.device))
    if isinstance(obj, (int, float)):
        return ("v", obj)
    if isinstance(obj, (list, tuple)):
        return ("seq", *(_cov_key(v) for v in obj))
    return (type(obj).__name__, *((k, _cov_key(v)) for k, v in sorted(getattr(obj, "__dict__", {}).items())))


def _device_scalar(v, device) -> tuple[float, Tensor | None]:
    r"""A 0-d schedule value as the covariance kernels read it: a host float when it lives on the host (no sync), else a
    one-element fp32 / fp64 device tensor."""
    if not torch.is_tensor(v):
        return float(v), None
    if v.device.type == "cpu":
        return float(v), None
    v = v.reshape(1).to(device)
    return 1.0, (v if v.dtype in (torch.float32, torch.float64) else v.to(torch.float64)).contiguous()


class GaussianDenoiser(Denoiser):
    r"""Analytical denoiser of a Gaussian prior :math:`X \sim \mathcal{N}(\mu_x, \Sigma_x)` (reference
    ``azula/denoise.py:117-172``): with :math:`X_t \sim \mathcal{N}(\alpha_t X, \sigma_t^2 I)`,

    .. math:: \mathbb{E}[X \mid x_t] = \mu_x + \Sigma_x (\Sigma_x + \rho_t I)^{-1} (z - \mu_x), \quad
        z = x_t / \alpha_t, \quad \rho_t = (\sigma_t / \alpha_t)^2

    Arguments:
        mean: The mean vector :math:`\mu_x`, with shape :math:`(N_1, ..., N_d)`.
        cov: The covariance matrix :math:`\Sigma_x` (an :class:`azula_amd.linalg.covariance.Covariance`).
        schedule: The noise schedule.

    Host tensors take the reference's op sequence.  Device tensors take the form above: the covariance applies run on the
    kernels of ``csrc/covariance.hip`` (see :mod:`azula_amd.linalg.covariance`).  For the spectral covariances (Isotropic,
    Diagonal, Full, Kronecker with a Diagonal ``L``) with fp32 latents and factors, a sampler runs the whole denoiser inside
    its captured step graph: ``z - mu``, the projection, ``e / (e + rho)``, the expansion and ``+ mu``, with ``rho`` read
    from the step's coefficient row.  ``mean`` and ``cov`` are plain attributes: a re-assignment or an in-place edit of
    their tensors rebuilds that plan.
    """

    def __init__(self, mean: Tensor, cov, schedule: Schedule) -> None:
        super().__init__()
        self.mean = mean
        self.cov = cov
        self.schedule = schedule

    def _apply(self, fn, recurse: bool = True):
        super()._apply(fn, recurse=recurse)
        self.mean = fn(self.mean)
        self.cov = fn(self.cov)
        return self

    @_lib.on_device
    def forward(self, x_t: Tensor, t: Tensor, **kwargs) -> DiracPosterior:
        from .linalg.covariance import IsotropicCovariance

        alpha_t, sigma_t = self.schedule(t)
        if not x_t.is_cuda:  # host tensors: the reference's op sequence
            mean_t = alpha_t * self.mean
            cov_t = IsotropicCovariance(alpha_t**2) * self.cov + IsotropicCovariance(sigma_t**2)
            return DiracPosterior(mean=(x_t + sigma_t**2 * cov_t.inv(mean_t - x_t)) / alpha_t)

        # The reference's (x_t + sigma^2 cov_t^-1 (alpha mu - x_t)) / alpha is the same quantity, but it cancels
        # catastrophically in fp32 as t -> 1: z = x_t / alpha grows like 1 / alpha while the mean stays O(1).
        rho = (sigma_t / alpha_t) ** 2
        mu = self.mean
        d = self._centered(x_t, alpha_t)
        y = self.cov @ ((self.cov + IsotropicCovariance(rho)).inv @ d)
        if d.is_cuda and self._kernel_mean(x_t) and y.dtype in (torch.float32, torch.float64):
            from .linalg.covariance import _scale

            y = y.contiguous()
            return DiracPosterior(mean=_scale(y, mu.numel(), v=mu))
        return DiracPosterior(mean=y + mu)

    def _kernel_mean(self, x_t: Tensor) -> bool:
        mu = self.mean
        return (torch.is_tensor(mu) and mu.device == x_t.device and mu.dtype in (torch.float32, torch.float64)
                and x_t.dtype in (torch.float32, torch.float64) and mu.is_contiguous() and mu.numel() > 0
                and x_t.numel() % mu.numel() == 0 and tuple(x_t.shape[x_t.ndim - mu.ndim:]) == tuple(mu.shape)
                and not (torch.is_grad_enabled() and (x_t.requires_grad or mu.requires_grad)))

    def _centered(self, x_t: Tensor, alpha_t: Tensor) -> Tensor:
        r"""``x_t / alpha_t - mu`` (one ``az_cov_scale`` pass where the kernels take the operands)."""
        if alpha_t.numel() == 1 and self._kernel_mean(x_t):
            from .linalg.covariance import _scale

            k, k_dev = _device_scalar(1 / alpha_t, x_t.device)
            return _scale(x_t.contiguous(), self.mean.numel(), u=self.mean, k=k, k_dev=k_dev)
        return x_t / alpha_t - self.mean

    # -- fused sampling ---------------------------------------------------------------------------------------------
    def host_coefficients(self, alpha_t: Tensor, sigma_t: Tensor) -> dict:
        r"""The program's input is ``z = x_t / alpha_t`` (``c_in``), its output the mean itself (``c_skip = 0``,
        ``c_out = 1``); ``rho = (sigma_t / alpha_t)^2`` travels in the ``c_time`` word."""
        c_in = 1 / alpha_t
        return {"c_in": c_in, "c_out": torch.ones_like(c_in), "c_skip": torch.zeros_like(c_in),
                "c_time": (sigma_t / alpha_t) ** 2}

    def _az_fused_key(self) -> tuple:
        return (_cov_key(self.mean), _cov_key(self.cov))

    def _az_fused(self, x: Tensor, kwargs: dict, cur_coef: Tensor):
        from .linalg import covariance as cv

        mu, cov = self.mean, self.cov
        f32 = lambda *ts: all(torch.is_tensor(t) and t.dtype == torch.float32 and t.device == x.device and t.is_contiguous()  # noqa: E731
                              for t in ts)
        if x.dtype != torch.float32 or x.ndim < 2 or not f32(mu) or mu.numel() != x[0].numel():
            return None
        n = mu.numel()
        B = x.numel() // n
        rho_ptr = cur_coef.data_ptr() + 4 * _lib.COEF_FIELDS.index("c_time")
        tape_ops: list = []
        keep: list = []
        x_in, out = torch.empty_like(x), torch.empty_like(x)

        def scale(src: Tensor, dst: Tensor, cols: int, e: Tensor | None = None, u: Tensor | None = None,
                  v: Tensor | None = None) -> None:
            a = _lib.AzCovScaleArgs(x=src.data_ptr(), e=None if e is None else e.data_ptr(), u=None if u is None else u.data_ptr(),
                                    v=None if v is None else v.data_ptr(), rho_dev=rho_ptr if e is not None else None,
                                    y=dst.data_ptr(), k=1.0, rows=src.numel() // cols, n=cols,
                                    e_len=0 if e is None else e.numel(), h=cv.H_POSTERIOR if e is not None else cv.H_IDENTITY)
            tape_ops.append(("az_cov_scale", a))

        if isinstance(cov, cv.IsotropicCovariance):
            lam = cov.lmbda
            if torch.is_tensor(lam):
                if not (lam.dtype == torch.float32 and lam.device in (x.device, torch.device("cpu"))):
                    return None
                e = lam.detach().to(device=x.device).reshape(1).clone()
            else:
                e = torch.tensor([float(lam)], dtype=torch.float32, device=x.device)
            keep.append(e)
            scale(x_in, out, n, e=e, u=mu, v=mu)
        elif isinstance(cov, cv.DiagonalCovariance):
            if not (f32(cov.D) and cov.D.numel() == n):
                return None
            scale(x_in, out, n, e=cov.D, u=mu, v=mu)
        elif isinstance(cov, cv.FullCovariance):
            Q, L = cov.Q, cov.L
            r = Q.shape[-1]
            if not (f32(Q, L) and Q.numel() == n * r and L.numel() == r):
                return None
            d, y = torch.empty_like(x), torch.empty_like(x)
            P, P2 = (torch.empty(B, r, dtype=torch.float32, device=x.device) for _ in range(2))
            nseg = _lib.lib().az_cov_segments(n)
            partial = torch.empty(nseg, B, r, dtype=torch.float32, device=x.device) if nseg > 1 else None
            keep += [d, y, P, P2, partial]
            scale(x_in, d, n, u=mu)
            tape_ops.append(("az_cov_project", _lib.AzCovLowRankArgs(
                x=d.data_ptr(), W=Q.data_ptr(), P=P.data_ptr(), partial=None if partial is None else partial.data_ptr(),
                rows=B, n=n, r=r)))
            scale(P, P2, r, e=L)
            tape_ops.append(("az_cov_expand", _lib.AzCovLowRankArgs(W=Q.data_ptr(), P=P2.data_ptr(), y=y.data_ptr(), s=1.0,
                                                                    rows=B, n=n, r=r)))
            scale(y, out, n, v=mu)
        elif isinstance(cov, cv.KroneckerCovariance) and isinstance(cov.L, cv.DiagonalCovariance):
            Qs, D = cov.Qs, cov.L.D
            shape = [Q.shape[0] for Q in Qs]
            if not (f32(D, *Qs) and math.prod(shape) == n and D.numel() == n and all(Q.shape == (m, m) for Q, m in zip(Qs, shape))):
                return None
            bufs = [torch.empty_like(x) for _ in range(2)]
            keep += bufs
            scale(x_in, bufs[0], n, u=mu)
            cur = 0
            for transpose, core in ((1, True), (0, False)):
                for i, Q in enumerate(Qs):
                    tape_ops.append(("az_cov_mode", _lib.AzCovModeArgs(
                        x=bufs[cur].data_ptr(), Q=Q.data_ptr(), y=bufs[1 - cur].data_ptr(), outer=B * math.prod(shape[:i]),
                        n=shape[i], inner=math.prod(shape[i + 1:]), transpose=transpose)))
                    cur = 1 - cur
                if core:
                    scale(bufs[cur], bufs[1 - cur], n, e=D)
                    cur = 1 - cur
            scale(bufs[cur], out, n, v=mu)
        else:
            return None  # the DPLR family (and anything else): the generic loop

        from .engine import Tape
        from .sample import BackboneProgram, FusedDenoiser

        tape = Tape()
        for name, a in tape_ops:
            tape.add(name, C.byref(a), keep=[a])
        tape.keep += [mu, cov, *keep]
        Cc = x.shape[1] if x.ndim > 2 else 1
        program = BackboneProgram(tape=tape, x_in=x_in, x_in_cs=0, out=out, f_channels=Cc, f_nhwc=False, wide=False)
        return FusedDenoiser(coefficients=self.host_coefficients, programs=[program])
