r"""The two tapes of an input-gradient (vjp) plan and their static buffers, shared by every backbone's gradient plan
(``nn/unet.py``, ``nn/vit.py``, ``plugins/adm``, ``plugins/jit``)."""

from __future__ import annotations

import torch
from torch import Tensor

from .engine import Act, Builder, Tape
from .plan import mod_buffer, with_mod_front


def vjp_scope(module: torch.nn.Module, x: Tensor, name: str, who: str | None = None) -> None:
    r"""The input-gradient tapes of every backbone take fp32 parameters and fp32 device tensors (``who``: the backbone's name in
    the forward's own device check).  What else a backbone leaves out (volumes, circular padding, head sizes) is its own check."""
    from .nn.utils import backbone_io_dtype

    if x.dtype != torch.float32 or any(p.dtype != torch.float32 for p in module.parameters()):
        raise NotImplementedError(f"{name}.vjp: fp32 parameters and tensors only (half-precision modules have no input-gradient plan)")
    if not x.is_cuda:
        raise NotImplementedError(f"{name}.vjp: device tensors only (CPU tensors have no input-gradient path)")
    backbone_io_dtype(module, x, who or f"azula_amd.nn.{name}")


def row_pullback(result: tuple) -> tuple:
    r"""``(out, pullback)`` of a 1-D network from those of the one-row images (B, C, 1, L) it runs as."""
    out, pullback = result
    return out[:, :, 0], lambda v: pullback(v[:, :, None])[:, :, 0]


class _GradTapes:
    r"""The two tapes of a gradient plan and their static planar buffers.  *forward-keep* (``fwd``): ``x_in`` (planar) ->
    ``out`` (planar) with every tensor the pullback reads kept alive; *backward* (``bwd``): ``v_in`` (the cotangent of the
    output, planar) -> ``dx`` (the cotangent of the input, planar).  The backward tape only writes temporaries of its own, so it
    runs any number of times after one forward-keep run.  Plain ``Tape.run`` on the current stream: no graph capture."""

    def __init__(self, device, B: int, cin: int, cout: int, H: int, W: int, mod_rows: int, D: int, tokens: bool = False) -> None:
        self.bld = Builder(device)
        if tokens:  # (B, L, C) token plans: the four buffers are views of the plan's own activations (_TokenGradTapes)
            self.x_in = self.out = self.v_in = self.dx = None
        else:
            self.x_in = torch.empty(B, cin, H, W, dtype=torch.float32, device=device)
            self.out = torch.empty(B, cout, H, W, dtype=torch.float32, device=device)
            self.v_in = torch.empty(B, cout, H, W, dtype=torch.float32, device=device)
            self.dx = torch.empty(B, cin, H, W, dtype=torch.float32, device=device)
        self.mod = mod_buffer(device, mod_rows, D)
        self.mod_rows, self.D = mod_rows, D
        self.fwd = self.bld.tape  # (the builder records onto it until end_forward)
        self.bwd: Tape | None = None
        self.serial = 0  # forward-keep runs so far: a pullback belongs to one of them

    def end_forward(self, mod_jobs: list) -> None:
        self.fwd = with_mod_front(self.bld, self.fwd, mod_jobs, self.mod, self.mod_rows, self.D)
        self.bld.tape = Tape()

    def end_backward(self) -> None:
        self.bld.finish()  # (one split-K workspace for both tapes)
        self.bwd = self.bld.tape
        self.bwd.keep.append(self.fwd)

    @property
    def saved_bytes(self) -> int:
        return self.bld.pool.bytes

    def run(self, x: Tensor, mod: Tensor | None):
        self.x_in.copy_(x)
        if self.mod_rows:
            self.mod.copy_(mod.to(torch.float32).reshape(self.mod_rows, -1))
        self.fwd.run()
        self.serial += 1
        serial = self.serial

        @torch.no_grad()
        def pullback(v: Tensor) -> Tensor:
            if serial != self.serial:
                raise RuntimeError("this pullback belongs to an earlier vjp call on the same module and shapes: its saved "
                                   "tensors have been overwritten")
            if not v.is_cuda or v.dtype != torch.float32 or tuple(v.shape) != tuple(self.out.shape):
                raise ValueError(f"pullback: expected an fp32 device tensor of shape {tuple(self.out.shape)}")
            with torch.cuda.device(self.v_in.device):
                self.v_in.copy_(v)
                self.bwd.run()
                return self.dx.clone()

        return self.out.clone(), pullback


class _TokenGradTapes(_GradTapes):
    r""":class:`_GradTapes` on (B, L, C) token tensors: ``x_in`` / ``out`` / ``v_in`` / ``dx`` are views of the plan's own
    (channel-padded) activations, so nothing is rearranged on the way in or out."""

    def __init__(self, device, B: int, L: int, cin: int, mod_rows: int, D: int) -> None:
        super().__init__(device, B, cin, cin, L, 1, mod_rows, D, tokens=True)
        self.B, self.L = B, L

    def _pinned(self, channels: int) -> Act:
        a = self.bld.new_act(self.B, self.L, 1, channels, pinned=True)
        a.buf.zero_()  # (the pad lanes stay zero: only the real channels are ever copied in)
        return self.bld.wrote(a, bounded=False)

    def _view(self, a: Act) -> Tensor:
        return a.buf.view(self.B, self.L, a.cs)[..., : a.C]

    def token_input(self, channels: int) -> Act:
        a = self._pinned(channels)
        self.x_in = self._view(a)
        return a

    def cotangent(self, channels: int) -> Act:
        a = self._pinned(channels)
        self.v_in = self._view(a)
        return a

    def set_output(self, out: Act) -> None:
        out.pinned = True
        self.out = self._view(out)

    def set_dx(self, dx: Act) -> None:
        dx.pinned = True
        self.dx = self._view(dx)
        self.end_backward()

    def run(self, x: Tensor, mod: Tensor | None):
        lead = tuple(x.shape[:-2])  # (standalone modules take (*, L, C))
        out, pull = super().run(x.reshape(self.B, self.L, -1), mod)
        if lead == (self.B,):
            return out, pull
        return out.reshape(*lead, self.L, -1), lambda v: pull(v.reshape(self.B, self.L, -1)).reshape(*lead, self.L, -1)
