r"""The forward plan of every backbone: its builder, its modulation buffer and front, its input in one of four layouts, how it is
run and how it is handed to the captured sampling loop.  The backbones (``nn/unet.py``, ``nn/unet3d.py``, ``nn/vit.py``,
``plugins/adm``, ``plugins/jit``, ``plugins/vdm``) subclass :class:`ForwardPlan` and emit their walk; the gradient twin is
``gradplan.py``."""

from __future__ import annotations

import math

import torch
from torch import Tensor

from . import _lib, engine
from .engine import Act, Builder, Tape, mod_front_tape


def mod_buffer(device, mod_rows: int, D: int) -> Tensor:
    r"""The (rows, D) fp32 buffer the modulation front reads (one element where there is no modulation)."""
    return torch.empty(max(mod_rows, 1), max(D, 1), dtype=torch.float32, device=device)


def with_mod_front(bld: Builder, tape: Tape, mod_jobs: list, mod: Tensor, mod_rows: int, D: int) -> Tape:
    r"""``tape`` behind the modulation front of the queued jobs (``engine.ada_zero_triple``): h_i = silu(W0_i mod + b0_i) for all
    blocks as ONE GEMV, abc_i = W2_i h_i + b2_i as ONE grouped GEMV.  No job: ``tape`` itself, nothing prepended."""
    if not mod_jobs:
        return tape
    pre = mod_front_tape(bld, mod_jobs, mod, mod_rows, D)
    pre.extend(tape)
    return pre


def copy_tape(tape: Tape, front: Tape | None = None) -> Tape:
    r"""A tape of its own with the launches of ``front`` (if any), then those of ``tape``: extending it leaves both alone."""
    c = Tape()
    for t in (front, tape):
        if t is not None:
            c.extend(t)
    return c


class ForwardPlan:
    r"""Compiled forward of one backbone for one signature.  A subclass makes the input with one of ``latent_input`` /
    ``planar_input`` / ``nhwc_input`` / ``token_input`` / ``nchw_input``, emits its walk on ``bld`` (queueing modulation MLPs on
    ``mod_jobs``), sets ``out`` (planar) or ``out_tokens`` and calls :meth:`end`.  Inputs of its own (time indices, labels) are
    the subclass's: the backbone fills them before :meth:`run`."""

    planar = False  # x_in is the planar latent, read by Builder.conv_stem
    x_in: Act | None = None  # planar / NHWC / token input
    x_nchw: Tensor | None = None  # (B, Z, H, W) input of a patchify launch
    tokens: Act | None = None
    out: Tensor | None = None
    out_tokens: Act | None = None

    def __init__(self, device, *, half=None, half_act: bool = False, mod_rows: int = 0, D: int = 0) -> None:
        self.bld = Builder(device, half=half, half_act=half_act)
        self.mod = mod_buffer(device, mod_rows, D)
        self.mod_rows, self.D = mod_rows, D
        self.mod_jobs: list[tuple] = []  # queued modulation MLPs (ada_zero_triple), emitted together at the tape front
        self.tape: Tape | None = None

    # -- the input, in its four forms ---------------------------------------------------------------------------------
    def _input(self, form: str, x_in: Act | None, loop_in: tuple | None) -> Act | None:
        self._form, self.x_in, self._loop_in = form, x_in, loop_in  # loop_in: (buffer, channel stride) of BackboneProgram
        return x_in

    def planar_input(self, B: int, C: int, H: int, W: int) -> Act:
        r"""The latent in the sampling loop's own (B, C, H, W) layout: channel stride 0 in the fused protocol."""
        self.planar = True
        a = Act(torch.empty(B * C * H * W, dtype=torch.float32, device=self.bld.device), B, H, W, C, 0, True)
        return self._input("planar", a, (a.buf, 0))

    def nhwc_input(self, B: int, H: int, W: int, C: int, *, zero: bool = True, pool: bool = False, shared: Act | None = None) -> Act:
        r"""The channel-padded NHWC image (volumes: B = all planes): a zero-filled (``zero=False``: uninitialised) buffer of its
        own, a pinned activation of the pool, or the input of another plan (``shared``)."""
        if shared is not None:
            a = shared
        elif pool:
            a = self.bld.new_act(B, H, W, C, pinned=True)
        else:
            cs = self.bld.pad(C)
            a = Act((torch.zeros if zero else torch.empty)(B * H * W * cs, dtype=torch.float32, device=self.bld.device), B, H, W, C, cs, True)
        return self._input("nhwc", a, (a.buf, a.cs))

    def latent_input(self, B: int, H: int, W: int, C: int, stem_3x3: bool, *, planes: int = 1, shared: Act | None = None) -> Act:
        r"""The input of an image network: at most 4 channels into a 3 x 3 first convolution (``stem_3x3``, the caller's check
        of that layer) of an fp32 module are read PLANAR (``Builder.conv_stem``), anything else as padded NHWC planes.  A
        ``shared`` input (the second program of classifier-free guidance) is planar only if it was made so."""
        if engine.STEM_PLANAR and C <= 4 and stem_3x3 and self.bld.half is None and (shared is None or shared.cs == 0):
            if shared is None:
                return self.planar_input(B, C, H, W)
            self.planar = True
            return self._input("planar", shared, (shared.buf, 0))
        return self.nhwc_input(B * planes, H, W, C, shared=shared)

    def token_input(self, B: int, L: int, C: int, f32: bool = False) -> Act:
        r"""(B, L, C) tokens in a pinned activation; :meth:`run` keeps the pad lanes zero."""
        self.tokens = self.bld.new_act(B, L, 1, C, pinned=True, f32=f32)
        return self._input("tokens", self.tokens, None)

    def nchw_input(self, B: int, Z: int, H: int, W: int) -> Tensor:
        r"""The (B, Z, H, W) buffer a patchify launch of the walk reads: again the loop's own layout."""
        self.x_nchw = torch.empty(B, Z, H, W, dtype=torch.float32, device=self.bld.device)
        self._input("nchw", None, (self.x_nchw, 0))
        return self.x_nchw

    # -- the end of emission -------------------------------------------------------------------------------------------
    def end(self) -> None:
        self.bld.finish()
        self.tape = with_mod_front(self.bld, self.bld.tape, self.mod_jobs, self.mod, self.mod_rows, self.D)

    # -- running -------------------------------------------------------------------------------------------------------
    def run(self, x: Tensor, mod: Tensor | None = None, *, cond: Tensor | None = None, out_dtype=torch.float32) -> Tensor:
        r"""Stages ``x`` (and ``cond``, behind its channels) for the plan's input form, copies the modulation, runs the tape on
        the current stream and returns the output as a tensor of the caller's own."""
        s = _lib.stream_ptr()
        form = self._form
        if form == "nchw":  # (the channel concatenation, written in place)
            Z = x.shape[1]
            self.x_nchw[:, :Z].copy_(x)
            if cond is not None:
                self.x_nchw[:, Z:].copy_(cond)
        else:
            if cond is not None:
                x = torch.cat((x, cond), dim=-1 if form == "tokens" else 1)
            x = x.to(torch.float32).contiguous()
            t = self.x_in
            if form == "planar":
                t.buf.copy_(x.reshape(-1))
            elif form == "nhwc":
                _lib.call("az_nchw_to_nhwc_f32", t.ptr, x.data_ptr(), None, x.shape[0], x.shape[1], math.prod(x.shape[2:]), t.cs, s)
            else:
                rows = x.reshape(t.B * t.H, -1)
                if t.cs == rows.shape[1]:
                    t.buf.copy_(rows.reshape(-1))
                else:
                    t.buf.zero_()
                    t.buf.view(t.B * t.H, t.cs)[:, : rows.shape[1]].copy_(rows)
        if self.mod_rows:
            self.mod.copy_(mod.to(torch.float32).reshape(self.mod_rows, -1))
        self.tape.run(s)
        if self.out is not None:
            return self.out.to(out_dtype, copy=True)
        o = self.out_tokens
        return o.buf.view(o.B, o.H, o.cs)[..., : o.C].to(out_dtype, copy=True).reshape(*x.shape[:-1], o.C)

    # -- the captured sampling loop ------------------------------------------------------------------------------------
    def program(self, f_channels: int, *, front: Tape | None = None, **kw):
        r"""The ``BackboneProgram`` of this plan: a copy of its tape (behind ``front``) that keeps the plan alive, the input the
        transition kernel writes and the planar output.  The plan itself stays as it is."""
        from .sample import BackboneProgram

        tape = copy_tape(self.tape, front)
        tape.keep.append(self)
        x_in, cs = self._loop_in
        return BackboneProgram(**{**dict(tape=tape, x_in=x_in, x_in_cs=cs, out=self.out, f_channels=f_channels, f_nhwc=False), **kw})
