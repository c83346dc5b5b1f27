r"""U-Net backbone executed by hand-written gfx950 kernels.

Drop-in for ``azula.nn.unet`` (reference ``azula/nn/unet.py:18-259``): same constructor
arguments, same ``state_dict`` keys (``descent.{l}.{j}...``, ``ascent.{k}.{j}...``),
same ``forward(x, mod, cond)`` semantics for 2-D inputs.  The modules below only HOLD the
parameters; the forward is a compiled tape of C-ABI kernels on a channel-padded NHWC layout:

* every conv is the MFMA implicit GEMM (``az_conv2d_f32``); SiLU, bias, the gated residual
  ``x + c*y`` (``unet.py:93``), the skip concat ``cat((y, x))`` (``unet.py:257``), nearest x2
  upsampling (``unet.py:187``), ``narrow`` (``unet.py:253-255``) and zero padding are folded into
  its gather / epilogue and never touch HBM as separate passes;
* normalisation + AdaZero modulation ``(a + 1) * norm(x) + b`` (``unet.py:91``) is one stats pass
  + one fused scale/shift pass;
* the first conv reads the NHWC input written by the sampler's transition kernel and the last
  conv writes planar NCHW directly.
"""

from __future__ import annotations

import math
from collections.abc import Sequence

import torch
import torch.nn as nn
from torch import Tensor

from ..engine import Act, Builder, PlanCache, Tape, ada_zero_triple, mod_rows, pad4
from ..gradplan import _GradTapes, row_pullback, vjp_scope
from ..plan import ForwardPlan
from .. import _lib, engine

__all__ = ["UNet", "UNetBlock"]


def _conv_holder(cin: int, cout: int, kernel_size, stride=1, identity_init: bool = False) -> nn.Module:
    r"""Parameter holder with the reference's shapes: ``Conv1d`` / ``Conv2d`` / ``Conv3d`` for spatial = 1 / 2 / 3 (``ConvNd``,
    ``azula/nn/layers.py:25-68``); ``len(kernel_size)`` is the number of spatial dimensions."""
    Conv = {1: nn.Conv1d, 2: nn.Conv2d, 3: nn.Conv3d}[len(kernel_size)]
    conv = Conv(cin, cout, kernel_size=tuple(kernel_size), stride=stride, padding=tuple(k // 2 for k in kernel_size))
    if identity_init:  # azula/nn/layers.py:53-66: near-identity down/up-sampling convolutions
        center = [k // 2 for k in conv.weight.shape[2:]]
        eye = torch.zeros_like(conv.weight.data[:cin])
        for i in range(min(cin, cout)):
            eye[(i, i, *center)] = 1.0
        conv.weight.data[:cin].mul_(1e-2)
        conv.weight.data[:cin].add_(eye)
    return conv


class UNetBlock(nn.Module):
    r"""Parameter holder of a modulated U-Net block (reference ``azula/nn/unet.py:18-116``).

    ``ada_zero`` = Linear(D, D) -> SiLU -> Linear(D, 3C) (last weight x 1e-2), or a raw
    ``(3, C, 1, 1)`` parameter when ``mod_features == 0``;  ``ffn`` = conv -> SiLU -> conv.
    """

    def __init__(
        self,
        channels: int,
        mod_features: int = 0,
        norm: str = "layer",
        groups: int = 16,
        ffn_factor: int = 1,
        spatial: int = 2,
        dropout: float | None = None,
        checkpointing: bool = False,
        kernel_size: Sequence[int] = (3, 3),
        **kwargs,
    ) -> None:
        super().__init__()
        if spatial not in (1, 2, 3):
            raise NotImplementedError("azula_amd.nn.UNet implements spatial = 1, 2 and 3")
        if isinstance(kernel_size, int):  # standalone use passes ConvNd's keyword arguments (reference unet.py:76-83)
            kernel_size = (kernel_size,) * spatial
        kernel_size = tuple(kernel_size)[:spatial] if len(kernel_size) >= spatial else tuple(kernel_size)
        if any(k % 2 == 0 for k in kernel_size) or kwargs.get("stride", 1) not in (1, (1,), [1], (1, 1), [1, 1], (1, 1, 1), [1, 1, 1]):
            raise NotImplementedError("odd kernel sizes with stride 1 only")
        pad = kwargs.get("padding", tuple(k // 2 for k in kernel_size))
        if tuple([pad] * len(kernel_size) if isinstance(pad, int) else pad) != tuple(k // 2 for k in kernel_size):
            raise NotImplementedError("'same' padding (kernel_size // 2) only")
        if norm not in ("layer", "rms", "group"):
            raise NotImplementedError(norm)
        self.periodic = kwargs.get("padding_mode", "zeros") == "circular"
        if kwargs.get("padding_mode", "zeros") not in ("zeros", "circular"):
            raise NotImplementedError(f"padding_mode {kwargs['padding_mode']!r}: zeros and circular only")
        self.channels, self.mod_features, self.spatial = channels, mod_features, spatial
        self.norm_kind, self.groups = norm, min(groups, channels)
        self.ffn_factor = ffn_factor
        if mod_features > 0:
            self.ada_zero = nn.Sequential(
                nn.Linear(mod_features, mod_features), nn.SiLU(), nn.Linear(mod_features, 3 * channels), nn.Identity()
            )
            self.ada_zero[-2].weight.data.mul_(1e-2)
        else:
            self.ada_zero = nn.Parameter(torch.randn(3, channels, *(1,) * spatial))
            self.ada_zero.data.mul_(1e-2)
        self.ffn = nn.Sequential(
            _conv_holder(channels, ffn_factor * channels, kernel_size),
            nn.SiLU(),
            nn.Identity() if dropout is None else nn.Dropout(dropout),
            _conv_holder(ffn_factor * channels, channels, kernel_size),
        )

        self._plans = PlanCache()

    def _emit(self, bld: Builder, x: Act, D: int, mod_rows: int, mod_jobs: list, keep_input: bool = False,
              saved: dict | None = None) -> Act:
        r"""y = (a + 1) norm(x) + b;  y = conv(silu(conv(y)));  out = x + c y   (reference ``unet.py:85-95``): one
        statistics + one scale/shift pass, two convolutions with SiLU / gate / residual in their epilogues.

        ``saved``: a dict that receives what :meth:`_emit_bwd` reads, kept alive -- the input ``x``, the GroupNorm statistics and
        the PRE-activation ``h``.  The forward-keep form takes no lazy norm and no epilogue moments, runs the first convolution
        without its SiLU epilogue and SiLU as a pass of its own behind it, and hands neither ``x`` nor ``h`` back to the pool."""
        keep = saved is not None
        Cc, cs = self.channels, pad4(self.channels)
        abc, bstride = ada_zero_triple(bld, self.ada_zero, Cc, D, mod_rows, mod_jobs)
        gn = {} if keep else None
        if self.norm_kind == "group":
            n_ = bld.group_norm(x, self.groups, scale=abc, shift=abc, scale_off=0, shift_off=cs, bstride=bstride, lazy=not keep, saved=gn)
        else:
            n_ = bld.row_norm(x, 0 if self.norm_kind == "layer" else 1, scale=abc, shift=abc, scale_off=0, shift_off=cs, bstride=bstride)
        c0, c3 = self.ffn[0], self.ffn[3]
        # (its moments bound the maximum of SiLU(conv) for the second convolution's f16x2 scale: no pass over the hidden tensor)
        h = bld.conv(n_, bld.pack_conv(c0.weight, c0.bias), c0.out_channels, act=0 if keep else 1, periodic=self.periodic,
                     gn_stats=not keep and engine.moments_for_scale())
        bld.free(n_)
        a1 = bld.silu(h) if keep else h
        y = bld.conv(a1, bld.pack_conv(c3.weight, c3.bias), c3.out_channels, gate=abc, gate_off=2 * cs, gate_bstride=bstride,
                     res=x, periodic=self.periodic, gn_stats=not keep and self.norm_kind == "group")  # feeds the next block's norm
        bld.free(a1)
        if keep:
            saved.update(x=x, abc=abc, bstride=bstride, gn=gn, h=h)
        elif not keep_input:
            bld.free(x)
        return y

    # -- input gradient (vector-Jacobian product) -------------------------------------------------------------------
    def _emit_bwd(self, bld: Builder, g: Act, saved: dict, cache: dict) -> Act:
        r"""Cotangent of the block's output -> cotangent of its input: g2 = c g; g3 = dgrad(conv2)(g2); g4 = g3 silu'(h);
        g5 = dgrad(conv1)(g4); dx = g + norm_bwd(x, gamma = 1 + a, g5)."""
        cs = pad4(self.channels)
        abc, bstride, x = saved["abc"], saved["bstride"], saved["x"]
        g2 = bld.channel_scale(g, abc, 2 * cs, bstride)
        g3 = bld.conv_dgrad(g2, self.ffn[3], cache=cache)
        bld.free(g2)
        bld.silu_bwd(g3, saved["h"])
        g5 = bld.conv_dgrad(g3, self.ffn[0], cache=cache)
        bld.free(g3)
        if self.norm_kind == "group":
            dx = bld.group_norm_bwd(x, g5, saved["gn"], scale=abc, scale_off=0, bstride=bstride, res=g)
        else:
            dx = bld.row_norm_bwd(x, g5, 0 if self.norm_kind == "layer" else 1, scale=abc, scale_off=0, bstride=bstride, res=g)
        bld.free(g5)
        bld.free(g)
        return dx

    @torch.no_grad()
    @_lib.on_device
    def vjp(self, x: Tensor, mod: Tensor | None = None):
        r"""``(out, pullback)``: ``out = self(x, mod)`` and ``pullback(v) = (d out / d x)^T v`` (like ``x``), both on the HIP
        tapes of a gradient plan (``mod`` is a constant of the pullback).  The pullback may be called any number of times
        until the next ``vjp`` of this module with the same shapes.  fp32, spatial = 1 / 2, zero padding."""
        if self.spatial == 3 or self.periodic:
            raise NotImplementedError("UNetBlock.vjp: spatial = 1 / 2 with zero padding only")
        vjp_scope(self, x, "UNetBlock")
        one_d = self.spatial == 1
        if one_d:
            assert x.ndim == 3
            x = x[:, :, None]
        assert x.ndim == 4 and x.shape[1] == self.channels
        B, Cc, H, W = x.shape
        D = self.mod_features

        def make(rows: int) -> _GradTapes:
            plan = _GradTapes(x.device, B, Cc, Cc, H, W, rows, D)
            bld = plan.bld
            xin = bld.new_act(B, H, W, Cc, pinned=True)
            plan.fwd.add("az_nchw_to_nhwc_f32", xin.ptr, plan.x_in.data_ptr(), None, B, Cc, H * W, xin.cs)
            bld.wrote(xin, bounded=False)
            jobs: list = []
            saved: dict = {}
            out = self._emit(bld, xin, D, rows, jobs, saved=saved)
            bld.tape.add("az_nhwc_to_nchw_f32", plan.out.data_ptr(), out.ptr, B, Cc, H * W, out.cs)
            plan.end_forward(jobs)
            g = bld.new_act(B, H, W, Cc, pinned=True)
            bld.tape.add("az_nchw_to_nhwc_f32", g.ptr, plan.v_in.data_ptr(), None, B, Cc, H * W, g.cs)
            bld.wrote(g, bounded=False)
            dx = self._emit_bwd(bld, g, saved, {})
            bld.tape.add("az_nhwc_to_nchw_f32", plan.dx.data_ptr(), dx.ptr, B, Cc, H * W, dx.cs)
            plan.end_backward()
            return plan

        res = self._cached_plan(x, mod, make, vjp=True)[0].run(x, mod)
        return row_pullback(res) if one_d else res

    def _cached_plan(self, x: Tensor, mod: Tensor | None, make, vjp: bool = False):
        r"""(plan, modulation rows) of this block for ``x`` (B, C, *dims) and ``mod``: the cached plan, else ``make(rows)``.  A
        gradient plan lives beside the forward ones under a ``"vjp"`` key."""
        rows = mod_rows(mod, x.shape[0], self.mod_features, "block")
        key = (*(("vjp",) if vjp else ()), x.shape[0], *x.shape[2:], rows, str(x.device))
        return self._plans.get(key, lambda: make(rows), self), rows

    @torch.no_grad()
    @_lib.on_device
    def forward(self, x: Tensor, mod: Tensor | None = None) -> Tensor:
        r"""x: (B, C, H, W) [(B, C, L) for spatial = 1, (B, C, D, H, W) for spatial = 3]; mod: (D) or (B, D) -> like x
        (reference ``unet.py:97-116``)."""
        from .utils import backbone_io_dtype

        out_dtype = backbone_io_dtype(self, x, "azula_amd.nn.UNetBlock")
        one_d = self.spatial == 1
        if one_d:  # (B, C, L): the same kernels and the same plan cache on a one-row image (no module state is touched)
            assert x.ndim == 3
            x = x[:, :, None]
        assert x.ndim == (5 if self.spatial == 3 else 4) and x.shape[1] == self.channels
        plan, _ = self._cached_plan(x, mod, lambda rows: _BlockPlan(self, x.shape[0], tuple(x.shape[2:]), rows, x.device))
        out = plan.run(x, mod, out_dtype=out_dtype)
        return out[:, :, 0] if one_d else out


class _BlockPlan(ForwardPlan):
    r"""One-block plan on (B, C, H, W) images, or (B, C, D, H, W) volumes as B D planes on the volume form (see ``unet3d.py``)."""

    def __init__(self, blk: UNetBlock, B: int, dims: tuple, rows: int, device) -> None:
        super().__init__(device, half=next(blk.parameters()).dtype, mod_rows=rows, D=blk.mod_features)
        vol = blk.spatial == 3
        planes, (H, W) = (dims[0] if vol else 1), dims[-2:]
        Cc, D, bld = blk.channels, blk.mod_features, self.bld
        xin = self.nhwc_input(B * planes, H, W, Cc, pool=True)
        if vol:
            from .unet3d import Vol, block3d

            out = block3d(blk, bld, Vol(xin, B, planes), D, rows, self.mod_jobs, keep_input=True)
        else:
            out = blk._emit(bld, xin, D, rows, self.mod_jobs, keep_input=True)
        self.out = torch.empty(B, Cc, *dims, dtype=torch.float32, device=device)
        bld.tape.add("az_nhwc_to_nchw_f32", self.out.data_ptr(), out.buf.data_ptr(), B, Cc, math.prod(dims), out.cs)
        self.end()


class UNetPlan(ForwardPlan):
    r"""Compiled forward for one (batch, H, W, modulation-rows) signature."""

    def __init__(self, net: "UNet", B: int, H: int, W: int, mod_rows: int, device: torch.device) -> None:
        self.B, self.H, self.W = B, H, W
        # a network cast to half precision keeps its activations in HBM in its own type (engine.HALF_ACT) when every kernel on its
        # tape has the typed form: channel counts in multiples of 8, whole GroupNorm groups in 4-channel chunks, power-of-two strides
        sv0 = (net.stride, net.stride) if isinstance(net.stride, int) else tuple(net.stride)
        blocks = [m for m in net.modules() if isinstance(m, UNetBlock)]
        half_act = (net.spatial == 2 and all(c % 8 == 0 for c in net.hid_channels) and all(v in (1, 2, 4, 8, 16) for v in sv0)
                    and all(b.norm_kind != "group" or (b.channels // b.groups) % 4 == 0 for b in blocks)
                    and all(b.ffn[0].out_channels % 8 == 0 and b.channels <= 4096 for b in blocks))
        super().__init__(device, half=next(net.parameters()).dtype, half_act=half_act, mod_rows=mod_rows, D=net.mod_features)
        first = net.descent[0][0]
        stem = net.spatial == 2 and tuple(first.weight.shape[2:]) == (3, 3) and first.out_channels % 4 == 0
        x_in = self.latent_input(B, H, W, net.in_channels + net.cond_channels, stem)
        self.out = torch.empty(B, net.out_channels, H, W, dtype=torch.float32, device=device)
        _walk(net, self.bld, x_in, self.out, mod_rows, self.mod_jobs, planar=self.planar)
        self.end()


def _walk(net: "UNet", bld: Builder, cur: Act, out: Tensor, mod_rows: int, mod_jobs: list, *, planar: bool = False,
          keep: bool = False) -> tuple:
    r"""The network from the input Act ``cur`` to the planar output ``out``: descent with the skip list (reference
    unet.py:226-230), ascent with the merge convolutions reading ``cat((skip, upsampled))`` in place.  ``planar``: ``cur`` is the
    planar latent, read by ``Builder.conv_stem``.  ``keep``: the forward-keep tape of a gradient plan -- blocks in their keep form
    (``UNetBlock._emit(saved=)``), no convolution-epilogue moments, the last block's output not released.  Returns what the
    backward walk reads: per level the (block, record) pairs of descent and ascent and the map sizes, and the last convolution."""
    L, D, stride = len(net.hid_blocks), net.mod_features, net.stride
    # power-of-two strides (<= 16): the decoder's nearest upsampling is a right shift inside the merge convolution's gather;
    # any other stride: a nearest-upsampling pass of its own in front of the merge convolution (reference unet.py:186,250-254)
    sv = (stride, stride) if isinstance(stride, int) else tuple(stride)
    pow2 = all(v in (1, 2, 4, 8, 16) for v in sv)
    up = 0
    if pow2:
        up = stride.bit_length() - 1 if isinstance(stride, int) else tuple(v.bit_length() - 1 for v in stride)
    per = net.periodic
    gn = not keep and any(isinstance(m, UNetBlock) and m.norm_kind == "group" for m in net.modules())

    def blocks(mods, x: Act) -> tuple[Act, list]:
        recs = []
        for blk in mods:
            saved = {} if keep else None
            x = blk._emit(bld, x, D, mod_rows, mod_jobs, saved=saved)
            recs.append((blk, saved))
        return x, recs

    skips: list[Act] = []
    down, upr, sizes = [], {}, []
    for i in range(L):
        first = net.descent[i][0]
        if i > 0:
            skips.append(cur)  # output of level i-1 = memory entry (unet.py:226-230)
        if i == 0 and planar:
            cur = bld.conv_stem(cur.buf, cur.B, cur.C, cur.H, cur.W, bld.pack_conv(first.weight, first.bias), first.out_channels,
                                periodic=per, gn_stats=gn)
        else:
            cur = bld.conv(cur, bld.pack_conv(first.weight, first.bias), first.out_channels, stride=stride if i > 0 else 1,
                           periodic=per, gn_stats=gn)
        sizes.append((cur.H, cur.W))
        cur, recs = blocks(net.descent[i][1 : 1 + net.hid_blocks[i]], cur)
        down.append(recs)
    for k in range(L):
        i = L - 1 - k
        mods = net.ascent[k]
        idx = 0
        if i + 1 < L:
            y = skips[i]
            conv = mods[0]
            if not pow2:
                wide = bld.upsample_nearest(cur, sv[0], sv[1], y.H, y.W)
                bld.free(cur)
                cur = wide
            merged = bld.conv(
                y, bld.pack_conv(conv.weight, conv.bias, cin0=y.C), conv.out_channels, src1=cur, up1=up,
                hin=y.H, win=y.W, periodic=per, gn_stats=gn,
            )
            bld.free(cur)  # (outputs of a level's last block: no pullback reads them)
            bld.free(y)
            cur = merged
            idx = 1
        cur, upr[i] = blocks(mods[idx : idx + net.hid_blocks[i]], cur)
        # i > 0: nearest upsampling is folded into the next level's merge conv (up1 = log2 stride)
    last = net.ascent[L - 1][idx + net.hid_blocks[0]]
    bld.conv(cur, bld.pack_conv(last.weight, last.bias), last.out_channels, dst_nchw=out, periodic=per)
    if not keep:
        bld.free(cur)
    return down, upr, sizes, last


class UNetGradPlan(_GradTapes):
    r"""Gradient plan of a :class:`UNet` for one (batch, H, W, modulation-rows) signature: the forward-keep and backward tapes
    (see :class:`_GradTapes`).  The forward-keep tape is :class:`UNetPlan`'s walk in its keep form (:func:`_walk`), a different
    tape from that plan's, whose launches it leaves untouched: no lazy normalisation, no convolution-epilogue moments, SiLU as a
    pass of its own behind the kept pre-activation."""

    def __init__(self, net: "UNet", B: int, H: int, W: int, mod_rows: int, device: torch.device) -> None:
        cin, D = net.in_channels, net.mod_features
        super().__init__(device, B, cin, net.out_channels, H, W, mod_rows, D)
        bld = self.bld
        L = len(net.hid_blocks)
        sv = (net.stride, net.stride) if isinstance(net.stride, int) else tuple(net.stride)
        mod_jobs: list[tuple] = []

        # ---- forward-keep: the walk of UNetPlan, nothing the pullback reads is released
        cur = bld.new_act(B, H, W, cin, pinned=True)
        bld.tape.add("az_nchw_to_nhwc_f32", cur.ptr, self.x_in.data_ptr(), None, B, cin, H * W, cur.cs)
        bld.wrote(cur, bounded=False)
        down, upr, sizes, last = _walk(net, bld, cur, self.out, mod_rows, mod_jobs, keep=True)
        self.end_forward(mod_jobs)

        # ---- backward: the same graph walked from the output to the input
        cache: dict = {}
        v = bld.new_act(B, H, W, net.out_channels, pinned=True)
        bld.tape.add("az_nchw_to_nhwc_f32", v.ptr, self.v_in.data_ptr(), None, B, net.out_channels, H * W, v.cs)
        bld.wrote(v, bounded=False)
        g = bld.conv_dgrad(v, last, cache=cache)
        g_skip: dict[int, Act] = {}  # level -> the skip connection's share of that level's output cotangent
        for i in range(L):
            for blk, rec in reversed(upr[i]):
                g = blk._emit_bwd(bld, g, rec, cache)
            if i + 1 < L:
                conv = net.ascent[L - 1 - i][0]
                c0 = net.hid_channels[i]
                g_skip[i] = bld.conv_dgrad(g, conv, cin_lo=0, cin_hi=c0, cache=cache)
                g_up = bld.conv_dgrad(g, conv, cin_lo=c0, cache=cache)  # on the skip's grid: the narrowed, upsampled map
                bld.free(g)
                g = bld.upsample_nearest_bwd(g_up, sv[0], sv[1], *sizes[i + 1])
                bld.free(g_up)
        for i in range(L - 1, -1, -1):
            for blk, rec in reversed(down[i]):
                g = blk._emit_bwd(bld, g, rec, cache)
            first = net.descent[i][0]
            if i > 0:
                wide = bld.zero_stuff(g, sv[0], sv[1], *sizes[i - 1])
                bld.free(g)
                g = bld.conv_dgrad(wide, first, res=g_skip[i - 1], cache=cache)  # (the level's output is consumed twice: its cotangents add)
                bld.free(wide)
                bld.free(g_skip[i - 1])
            else:
                bld.conv_dgrad(g, first, dst_nchw=self.dx, cache=cache)
                bld.free(g)
        self.end_backward()


class UNet(nn.Module):
    r"""Modulated U-Net (reference ``azula/nn/unet.py:119-259``), gfx950-native forward.

    Arguments are those of ``azula.nn.unet.UNet``: ``spatial`` 1 (one-row images), 2 or 3 (volumes: every 3-D convolution
    as depth taps of the 2-D kernels, ``unet3d.py``), zero or circular padding, odd kernels, any integer stride per axis (powers of
    two: the upsampling is folded into the merge convolution; others: ``az_upsample_nearest_f32``; volumes: the same in-plane + a gather of whole planes along the depth axis).
    """

    def __init__(
        self,
        in_channels: int,
        out_channels: int,
        cond_channels: int = 0,
        hid_channels: Sequence[int] = (64, 128, 256),
        hid_blocks: Sequence[int] = (3, 3, 3),
        kernel_size: int | Sequence[int] = 3,
        stride: int | Sequence[int] = 2,
        spatial: int = 2,
        periodic: bool = False,
        identity_init: bool = False,
        **kwargs,
    ) -> None:
        super().__init__()
        assert len(hid_blocks) == len(hid_channels)
        if spatial not in (1, 2, 3):
            raise NotImplementedError("azula_amd.nn.UNet implements spatial = 1, 2 and 3")
        self.spatial = spatial
        if isinstance(kernel_size, int):
            kernel_size = [kernel_size] * spatial
        if isinstance(stride, int):
            stride = [stride] * spatial
        assert len(kernel_size) == len(stride) == spatial
        if any(k % 2 == 0 for k in kernel_size):
            raise NotImplementedError("odd kernel sizes only (anisotropic allowed)")
        if any(int(s_) != s_ or s_ < 1 for s_ in stride):
            raise ValueError("integer strides >= 1 only")
        self.in_channels, self.out_channels, self.cond_channels = in_channels, out_channels, cond_channels
        self.hid_channels, self.hid_blocks = tuple(hid_channels), tuple(hid_blocks)
        self.stride = stride[0] if len(set(stride)) == 1 else tuple(stride)  # int (isotropic) or one per axis
        self.mod_features = kwargs.get("mod_features", 0)
        self.periodic = bool(periodic)
        if periodic:  # reference unet.py:175-180: every convolution pads circularly
            kwargs["padding_mode"] = "circular"
        ks = tuple(kernel_size)

        self.descent, self.ascent = nn.ModuleList(), nn.ModuleList()
        for i, num_blocks in enumerate(hid_blocks):
            do, up = nn.ModuleList(), nn.ModuleList()
            for _ in range(num_blocks):
                do.append(UNetBlock(hid_channels[i], kernel_size=ks, spatial=spatial, **kwargs))
                up.append(UNetBlock(hid_channels[i], kernel_size=ks, spatial=spatial, **kwargs))
            if i > 0:
                do.insert(0, _conv_holder(hid_channels[i - 1], hid_channels[i], ks, stride=tuple(stride), identity_init=identity_init))
                up.append(nn.Upsample(scale_factor=tuple(float(s) for s in stride), mode="nearest"))
            else:
                do.insert(0, _conv_holder(in_channels + cond_channels, hid_channels[i], ks))
                up.append(_conv_holder(hid_channels[i], out_channels, ks))
            if i + 1 < len(hid_blocks):
                up.insert(0, _conv_holder(hid_channels[i] + hid_channels[i + 1], hid_channels[i], ks, identity_init=identity_init))
            self.descent.append(do)
            self.ascent.insert(0, up)
        self._plans = PlanCache()

    # -- plan management -----------------------------------------------------------------------
    def plan3d(self, B: int, D: int, H: int, W: int, mod_rows: int, device: torch.device):
        from .unet3d import UNet3DPlan

        return self._plans.get((B, D, H, W, mod_rows, str(device)), lambda: UNet3DPlan(self, B, D, H, W, mod_rows, device), self)

    def plan(self, B: int, H: int, W: int, mod_rows: int, device: torch.device) -> UNetPlan:
        return self._plans.get((B, H, W, mod_rows, str(device)), lambda: UNetPlan(self, B, H, W, mod_rows, device), self)

    # -- input gradient --------------------------------------------------------------------------------------------
    def grad_plan(self, B: int, H: int, W: int, mod_rows: int, device: torch.device) -> UNetGradPlan:
        return self._plans.get(("vjp", B, H, W, mod_rows, str(device)), lambda: UNetGradPlan(self, B, H, W, mod_rows, device), self)

    @torch.no_grad()
    @_lib.on_device
    def vjp(self, x: Tensor, mod: Tensor | None = None):
        r"""``(out, pullback)``: ``out = self(x, mod)`` and ``pullback(v) = (d out / d x)^T v`` (like ``x``): the input
        gradient that ``azula.guidance`` takes from ``torch.autograd``, on HIP tapes (``UNetGradPlan``).  ``mod`` is a
        constant of the pullback; it may be called any number of times until the next ``vjp`` with the same shapes.
        Scope: spatial = 1 / 2, zero padding, fp32 parameters and tensors, no ``cond_channels``; anything else raises
        ``NotImplementedError`` (the forward is not affected)."""
        if self.spatial == 3 or self.periodic or self.cond_channels:
            raise NotImplementedError("UNet.vjp: spatial = 1 / 2, zero padding, no cond_channels")
        vjp_scope(self, x, "UNet")
        one_d = self.spatial == 1
        if one_d:
            assert x.ndim == 3, "spatial = 1: expected (B, C, L)"
            x = x[:, :, None]
        B, Cin, H, W = x.shape
        assert Cin == self.in_channels
        rows = mod_rows(mod, B, self.mod_features, "UNet")
        res = self.grad_plan(B, H, W, rows, x.device).run(x, mod)
        return row_pullback(res) if one_d else res

    def _check_device(self, x: Tensor) -> torch.dtype:
        from .utils import backbone_io_dtype

        return backbone_io_dtype(self, x, "azula_amd.nn.UNet")

    # -- fused sampling (see azula_amd.sample.BackboneProgram) --------------------------------------
    def _program(self, x: Tensor, mod_rows: int):
        self._check_device(x)
        if self.cond_channels or x.ndim != (5 if self.spatial == 3 else 4):
            return None, None
        if self.spatial == 3:  # the loop's layouts only know (B, C, inner): a volume is an image of D H x W pixels
            B, _, Dd, H, W = x.shape
            p = self.plan3d(B, Dd, H, W, mod_rows, x.device)
            # The loop hands over the pre-scaled input in the latent's OWN (planar) layout, so that it launches the flat
            # transition form (every stream read / written once, 16 B per element: 0.72 - 0.76 of the HBM roofline) instead of
            # the image form with its channel-padded second output (0.59 on volumes); one layout pass in front of
            # the first convolution makes the (B, D, H, W, cs) planes the depth-tap launches read.
            x_planar = torch.empty(B * self.in_channels * Dd * H * W, dtype=torch.float32, device=x.device)
            front = Tape()
            front.add("az_nchw_to_nhwc_f32", p.x_in.ptr, x_planar.data_ptr(), None, B, self.in_channels, Dd * H * W, p.x_in.cs, keep=[x_planar])
            return p.program(self.out_channels, front=front, x_in=x_planar, x_in_cs=0), p.mod
        B, _, H, W = x.shape
        p = self.plan(B, H, W, mod_rows, x.device)
        return p.program(self.out_channels), p.mod

    def _az_compile_modulated(self, x: Tensor, mod_rows: int = 1):
        r"""(program, mod buffer): the caller's tape must fill the (mod_rows, D) buffer first."""
        if self.mod_features == 0:
            return None
        return self._program(x, mod_rows)

    def _az_compile(self, x: Tensor, kwargs: dict, cur_coef: Tensor):
        r"""Bare UNet as a KarrasDenoiser backbone: only meaningful without modulation (the
        second positional argument, c_time, is then ignored exactly as in the reference)."""
        if self.mod_features > 0 or kwargs:
            return None
        return self._program(x, 0)[0]

    @torch.no_grad()
    @_lib.on_device
    def forward(self, x: Tensor, mod: Tensor | None = None, cond: Tensor | None = None) -> Tensor:
        r"""x: (B, C_i, H, W); mod: (D) or (B, D); cond: (B, C_c, H, W) -> (B, C_o, H, W).  With ``spatial = 1`` the
        tensors are (B, C, L): a one-row image through the same kernels (the 1-D filters sit in the middle row of
        3 x 3 ones, the other rows only ever meet the padding); with ``spatial = 3`` they are (B, C, D, H, W) volumes, every
        3-D convolution as depth taps of the 2-D kernels (``unet3d.py``)."""
        out_dtype = self._check_device(x)
        assert x.ndim == self.spatial + 2, f"spatial = {self.spatial}: expected a {self.spatial + 2}-d input"
        assert x.shape[1] + (cond.shape[1] if cond is not None else 0) == self.in_channels + self.cond_channels
        if self.spatial == 1:
            x, cond = x[:, :, None], (cond[:, :, None] if cond is not None else None)
        rows = mod_rows(mod, x.shape[0], self.mod_features, "UNet")
        p = (self.plan3d if self.spatial == 3 else self.plan)(x.shape[0], *x.shape[2:], rows, x.device)
        out = p.run(x, mod, cond=cond, out_dtype=out_dtype)
        return out[:, :, 0] if self.spatial == 1 else out
