r"""RePaint inpainting -- drop-in for ``azula.guidance.repaint`` (reference ``repaint.py:20-63``).

A step is ``iterations`` DDIM steps t -> s, each followed by a masked replacement of the observed pixels and a re-noising
back to t (Lugmayr et al., 2022, https://arxiv.org/abs/2201.09865).  It needs no gradient through the denoiser, so it runs on
all three paths of the samplers:

* host tensors: the reference's op sequence (bit for bit, generator calls included);
* the captured loop (fp32 latents and clock, a fused-capable denoiser, ``y`` of x's shape and dtype, a bool ``mask`` that
  broadcasts to x's shape): ``iterations`` table rows per step, each one evaluation + ``az_transition_f32`` +
  ``az_repaint_f32`` + the next evaluation's input relayout, one hipGraph replay per step;
* otherwise the generic loop: ``DDIMSampler.step`` on the device followed by ``az_repaint_f32`` (fp32), or the reference's
  torch op sequence with its type promotion (``Sampler(dtype=float64)``).
"""

from __future__ import annotations

import ctypes as C

import torch
from torch import Tensor

from .. import _lib
from ..denoise import Denoiser
from ..engine import Tape
from ..sample import DDIMSampler, _attr_key

__all__ = ["RePaintSampler"]


class RePaintSampler(DDIMSampler):
    r"""Creates a RePaint sampler.

    Arguments:
        denoiser: A denoiser :math:`q_\phi(X \mid X_t)`.
        y: An observation :math:`y = m \odot x`.
        mask: The observation mask :math:`m` (bool).
        iterations: The number of RePaint iterations per step.
        kwargs: Keyword arguments passed to :class:`azula_amd.sample.DDIMSampler`.

    ``y`` and ``mask`` are read on every call, as in the reference: an in-place edit or a re-assignment takes effect on the
    next call.  Under ``parallel.sample_sharded`` they are the rank's slice of the batch, like per-sample keyword arguments.
    """

    def __init__(self, denoiser: Denoiser, y: Tensor, mask: Tensor, iterations: int = 3, **kwargs) -> None:
        super().__init__(denoiser, **kwargs)
        self.y = y
        self.mask = mask
        self.iterations = iterations

    def _repaint_scalars(self, t: Tensor, s: Tensor) -> tuple[Tensor, Tensor, Tensor, Tensor]:
        r"""The 0-d values of one step in the reference's op order (``repaint.py:48-49,55,59-61``):
        [alpha_s, sigma_s, alpha_t / alpha_s, alpha_t * sqrt((sigma_t / alpha_t)^2 - (sigma_s / alpha_s)^2)]."""
        alpha_s, sigma_s = self.denoiser.schedule(s)
        alpha_t, sigma_t = self.denoiser.schedule(t)
        return alpha_s, sigma_s, alpha_t / alpha_s, alpha_t * torch.sqrt((sigma_t / alpha_t) ** 2 - (sigma_s / alpha_s) ** 2)

    def _repaint_table(self) -> Tensor:
        r"""(steps, 4) fp32: ``_repaint_scalars`` of every step, from 0-d CPU tensors (the captured loop's per-step row)."""
        ts = torch.linspace(self.start, self.stop, self.steps + 1, dtype=self.dtype)
        return torch.stack([torch.stack(self._repaint_scalars(t, s)).to(torch.float32) for t, s in ts.unfold(0, 2, 1).unbind()])

    @torch.no_grad()
    @_lib.on_device
    def step(self, x_t: Tensor, t: Tensor, s: Tensor, **kwargs) -> Tensor:
        if self.iterations < 1:
            raise ValueError(f"iterations must be >= 1, got {self.iterations}")
        alpha_s, sigma_s, ratio, kick = self._repaint_scalars(t, s)
        coef = None
        for k in range(self.iterations):
            last = k == self.iterations - 1
            x_s = super().step(x_t, t, s, **kwargs)
            if self._kernel_applies(x_s):
                if coef is None:
                    coef = torch.stack((alpha_s, sigma_s, ratio, kick)).to(device=x_s.device, dtype=torch.float32)
                x_s, x_t = self._device_repaint(x_s, coef, last)
            else:  # host tensors, an fp64 clock or fp64 latents: the reference's op sequence and type promotion
                x_s = torch.where(self.mask, alpha_s * self.y + sigma_s * self._draw_noise(self.y), x_s)
                if not last:
                    x_t = ratio * x_s + kick * self._draw_noise(x_s)
                elif self.rng_parity:
                    self._draw_noise(x_s)  # (the reference re-noises after the last iteration too and discards the result)
        return x_s

    # -- generic device loop ------------------------------------------------------------------------------------------
    def _kernel_applies(self, x_s: Tensor) -> bool:
        y, m = self.y, self.mask
        if not (x_s.is_cuda and x_s.dtype == torch.float32 and torch.is_tensor(y) and torch.is_tensor(m)):
            return False
        if y.dtype != torch.float32 or m.dtype != torch.bool or y.device != x_s.device or m.device != x_s.device:
            return False
        return _broadcasts_to(y.shape, x_s.shape) and _broadcasts_to(m.shape, x_s.shape)

    def _device_repaint(self, x_s: Tensor, coef: Tensor, last: bool) -> tuple[Tensor, Tensor | None]:
        r"""``az_repaint_f32`` on one iteration.  The noise of the observation is drawn in ``y``'s shape (as the reference's
        ``randn_like(y)``) and, like ``y`` and ``mask``, expanded to x's shape."""
        shape = x_s.shape
        n_y = _aligned(self._draw_noise(self.y).expand(shape).contiguous(), 16)
        n_x = self._draw_noise(x_s) if (not last or self.rng_parity) else None
        y = _aligned(self.y.expand(shape).contiguous(), 16)
        mask = _aligned(self.mask.expand(shape).contiguous(), 4)
        x_s = _aligned(x_s.contiguous(), 16)
        x_t = None if last else torch.empty_like(x_s)
        a = _lib.AzRepaintArgs(
            x_s=x_s.data_ptr(), y=y.data_ptr(), mask=mask.data_ptr(), n_y=n_y.data_ptr(),
            n_x=None if last else n_x.data_ptr(), x_s_out=x_s.data_ptr() if last else None,
            x_t_out=None if last else x_t.data_ptr(), coef=coef.data_ptr(), n=x_s.numel(),
        )
        _lib.call("az_repaint_f32", C.byref(a), _lib.stream_ptr())
        return x_s, x_t

    # -- captured loop ------------------------------------------------------------------------------------------------
    def _fusable(self, x: Tensor) -> bool:
        if type(self).step is not RePaintSampler.step:
            return False  # a subclass overrides step: generic loop
        if x.ndim < 2 or self._clock(x) != "f32" or self.iterations < 1:
            return False  # (the fp64 clock runs the generic loop: the masked replacement has no fp64 kernel)
        y, m = self.y, self.mask
        if not (torch.is_tensor(y) and torch.is_tensor(m)):
            return False
        return (y.shape == x.shape and y.dtype == x.dtype and y.device == x.device and m.dtype == torch.bool
                and m.device == x.device and _broadcasts_to(m.shape, x.shape))

    def _hyper(self) -> tuple:
        # (y and mask are copied into the plan on every call: their values never key the coefficient table)
        return _attr_key({k: v for k, v in vars(self).items() if k not in ("y", "mask")})

    def _noise_draws(self) -> int:
        # per iteration: the DDIM step's noise (read only if eta != 0), randn_like(y), and randn_like(x_s) except after the last
        return self.iterations * (2 + int(self.eta != 0)) - 1

    def _fused_structure(self) -> tuple:
        return (*super()._fused_structure(), self.iterations, tuple(self.y.shape), tuple(self.mask.shape))

    def _fused_rows(self, t, s, fused):
        return super()._fused_rows(t, s, fused) * self.iterations  # every iteration evaluates the denoiser at t

    def _fused_step_tapes(self, loop):
        it, dev, n = self.iterations, loop.x.device, loop.x.numel()
        noise = list(loop.noise)
        loop.rp_eps = [noise.pop(0) for _ in range(it)] if self.eta != 0 else [None] * it
        loop.rp_ny = [noise.pop(0) for _ in range(it)]
        loop.rp_nx = [noise.pop(0) for _ in range(it - 1)] + [None]
        assert not noise
        loop.rp_dummy = torch.empty_like(loop.x) if self.rng_parity else None  # draws nothing reads (eta = 0, the last re-noise)
        loop.rp_y = torch.empty_like(loop.x)
        loop.rp_mask = torch.empty(loop.x.shape, dtype=torch.bool, device=dev)
        loop.rp_table = torch.zeros(self.steps, 4, dtype=torch.float32, device=dev)
        loop.rp_row = torch.zeros(4, dtype=torch.float32, device=dev)
        loop.keep += [loop.rp_dummy, loop.rp_y, loop.rp_mask, loop.rp_table, loop.rp_row]
        tape = Tape()
        for k in range(it):
            last = k == it - 1
            loop.add_evaluation(tape)
            if k == 0:  # this step's [alpha_s, sigma_s, alpha_t / alpha_s, kick] (every row of a step carries its step number)
                tape.add("az_gather_step_row_f32", loop.rp_row.data_ptr(), loop.rp_table.data_ptr(), loop.cur.data_ptr(), 1, 4,
                         self.steps)
            # the DDIM step in place: x_t is not read again once x_s exists
            loop.add_transition(tape, x_t=loop.x, x_s=loop.x, eps=loop.rp_eps[k], write_xin=False)
            a = _lib.AzRepaintArgs(
                x_s=loop.x.data_ptr(), y=loop.rp_y.data_ptr(), mask=loop.rp_mask.data_ptr(), n_y=loop.rp_ny[k].data_ptr(),
                n_x=None if last else loop.rp_nx[k].data_ptr(), x_s_out=loop.x.data_ptr() if last else None,
                x_t_out=None if last else loop.x.data_ptr(), coef=loop.rp_row.data_ptr(), n=n,
            )
            tape.add("az_repaint_f32", C.byref(a), keep=[a])
            # the next evaluation's backbone input: c_in(t) between iterations, c_in(s) after the last (_host_table's chaining)
            loop.add_input_relayout(tape, loop.x, loop.coef_ptr("c_in_next"))
        return [tape]

    def _fused_draws(self, loop) -> list[Tensor]:
        out = []
        for k in range(self.iterations):
            e = loop.rp_eps[k] if loop.rp_eps[k] is not None else loop.rp_dummy
            nx = loop.rp_nx[k] if loop.rp_nx[k] is not None else loop.rp_dummy
            out += [b for b in (e, loop.rp_ny[k], nx) if b is not None]
        return out

    def _fused_upload_extra(self, loop) -> None:
        loop.rp_table.copy_(self._repaint_table())

    def _fused_reset(self, loop) -> None:
        loop.rp_y.copy_(self.y)
        loop.rp_mask.copy_(self.mask.expand(loop.x.shape))


def _broadcasts_to(shape, target) -> bool:
    try:
        return tuple(torch.broadcast_shapes(tuple(shape), tuple(target))) == tuple(target)
    except RuntimeError:
        return False


def _aligned(t: Tensor, align: int) -> Tensor:
    return t if t.data_ptr() % align == 0 else t.clone()
