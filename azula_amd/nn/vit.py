r"""DiT / ViT backbones executed by gfx950 kernels -- drop-ins for ``azula.nn.dit`` / ``azula.nn.vit``.

Same constructors and ``state_dict`` keys as the reference (``azula/nn/dit.py:24-218``,
``azula/nn/vit.py:22-108``, ``azula/nn/attention.py:17-108``).  Note the reference's
block is NOT the standard two-branch DiT: ONE (a, b, c) AdaLN-zero triple per block,

    y = (a + 1) * RMSNorm(x) + b;   y = y + MSA(y);   y = FFN(y);   out = x + c * y   (dit.py:102-110)

Compiled forward (token tensors are "NHWC" images of width 1, so every linear is the MFMA
implicit GEMM with ksize = 1):

* patchify is an index remap fused with the ``c_in`` pre-scale; ``in_proj`` adds the
  (batch-shared, precomputed) positional embedding in its epilogue;
* RMSNorm + modulation is one row-norm pass; q/k RMSNorm and the 1/sqrt(C) scale are folded
  into the attention kernel's operand loads; ``y + y_proj(att)``, SiLU and ``x + c * ffn`` are
  GEMM epilogues.

Input gradient (``vjp``): forward-keep and backward tapes on the attention backward kernels (``csrc/attention_bwd.hip``),
:class:`DiTGradPlan`; DESIGN.md section 9.
"""

from __future__ import annotations

import math
from collections.abc import Sequence

import torch
import torch.nn as nn
from torch import Tensor

from .. import _lib, engine
from ..engine import Act, Builder, LinearView, PlanCache, SharedResidual, ada_zero_triple, content_key, mod_rows, pad4
from ..gradplan import _TokenGradTapes, vjp_scope
from ..plan import ForwardPlan

__all__ = ["DiT", "DiTBlock", "MultiheadSelfAttention", "ViT"]


class MultiheadSelfAttention(nn.Module):
    r"""Parameter holder (reference ``azula/nn/attention.py:17-70``): fused ``qkv_proj`` and
    bias-free ``y_proj``; per-head q/k RMSNorm has no parameters."""

    def __init__(
        self,
        channels: int,
        pos_channels: int = 1,
        attention_heads: int = 1,
        qkv_bias: bool = True,
        qk_norm: bool = True,
        rope: bool = False,
        dropout: float | None = None,
    ) -> None:
        super().__init__()
        assert channels % attention_heads == 0
        self.qkv_proj = nn.Linear(channels, 3 * channels, bias=qkv_bias)
        self.y_proj = nn.Linear(channels, channels, bias=False)
        if rope:  # learned rotary axes (reference attention.py:60-68): random directions, log-uniform magnitudes
            magnitude = torch.exp(math.log(1e-1) * torch.rand(channels // 2, 1))
            direction = torch.randn(channels // 2, pos_channels)
            direction = direction / torch.linalg.norm(direction, dim=-1, keepdim=True)
            self.theta_proj = nn.Linear(pos_channels, channels // 2, bias=False)
            self.theta_proj.weight.data.copy_(magnitude * direction)
        else:
            self.theta_proj = None
        self.heads = attention_heads
        self.qk_norm = qk_norm
        self._plans = PlanCache()

    def _emit(self, bld: Builder, y: Act, pos_h: Tensor | None, mask: Tensor | None, res: Act | None = None,
              saved: dict | None = None) -> Act:
        r"""qkv projection -> attention (q/k RMS norm, RoPE, mask in the kernel) -> y_proj (+ ``res``).  A head size the kernels are
        not instantiated for runs zero-padded to the next one (engine.ATTN_HEAD_DIMS; G24).

        ``saved``: a dict that receives what :meth:`_emit_bwd` reads, kept alive -- the raw ``qkv``, q^ | k^ and the attention
        output in front of ``y_proj`` (``Builder.attention_keep``).  The forward-keep form runs the projection without the q / k
        epilogue and pads heads to the sizes of the backward kernels (``engine.attn_grad_padded_dim``)."""
        keep = saved is not None
        C_ = self.qkv_proj.in_features
        d = C_ // self.heads
        dp = engine.attn_grad_padded_dim(d) if keep else engine.attn_padded_dim(d, bld.half)
        theta = None
        if self.theta_proj is not None:  # theta = theta_proj(pos) on the host (reference op order), tables on device
            if pos_h is None:
                raise ValueError("this attention layer uses RoPE: pass pos")
            theta = torch.nn.functional.linear(pos_h.to(torch.float32).cpu(), self.theta_proj.weight.detach().float().cpu())
        wq, bq, wy = self.qkv_proj.weight, self.qkv_proj.bias, self.y_proj.weight
        if dp != d:
            if theta is not None:
                theta = engine.pad_head_table(theta, self.heads, d // 2, dp // 2)
            wq, bq = engine.pad_qkv_heads(wq, bq, self.heads, d, dp, "nHC")
            wy = engine.pad_proj_heads(wy, self.heads, d, dp)
        rope = None if theta is None else (bld.const(torch.cos(theta)), bld.const(torch.sin(theta)))
        scale, norm_dim = 1.0 / math.sqrt(d), (d if dp != d else 0)
        if keep:
            qkv = bld.conv(y, bld.pack_conv(wq, bq), 3 * self.heads * dp)
            att, rec = bld.attention_keep(qkv, self.heads, self.qk_norm, scale, rope=rope, mask=mask, norm_dim=norm_dim)
            saved.update(attn=rec, wq=LinearView(wq), wy=LinearView(wy))
        else:
            # with RoPE: q / k RMS norm and the rotation in the projection's epilogue, once per layer (C6-like: attention 0.38 -> 0.49
            # of the MFMA peak).  The RMS norm alone stays in the attention kernel: measured on DiT-B/2 (C3) the kernel gains 7 % but
            # the captured step loses 0.4 % (23.77 vs 23.67 ms, two rounds each) -- a norm of the staged K rows is nearly free there.
            prep = dict(heads=self.heads, head_dim=d, rmsnorm=self.qk_norm, eps=1e-5, rope=rope) if rope and dp == d else None
            qkv = bld.conv(y, bld.pack_conv(wq, bq), 3 * self.heads * dp, qk_prep=prep)
            att = bld.attention(qkv, self.heads, "nHC", self.qk_norm, scale, rope=rope, mask=mask, norm_dim=norm_dim)
            bld.free(qkv)
        out = bld.conv(att, bld.pack_conv(wy, None), C_, res=res)
        if not keep:
            bld.free(att)
        return out

    # -- input gradient (vector-Jacobian product) -------------------------------------------------------------------
    def _emit_bwd(self, bld: Builder, g: Act, saved: dict, cache: dict, res: Act | None = None) -> Act:
        r"""Cotangent of the layer's output -> cotangent of its input (+ ``res`` in the epilogue of the qkv data-gradient GEMM)."""
        g_att = bld.conv_dgrad(g, saved["wy"], cache=cache)
        dqkv = bld.attention_bwd(g_att, saved["attn"])
        bld.free(g_att)
        gy = bld.conv_dgrad(dqkv, saved["wq"], res=res, cache=cache)
        bld.free(dqkv)
        return gy

    @torch.no_grad()
    @_lib.on_device
    def vjp(self, x: Tensor, pos: Tensor | None = None, mask: Tensor | None = None):
        r"""``(out, pullback)``: ``out = self(x, pos, mask)`` and ``pullback(v) = (d out / d x)^T v`` (like ``x``) on the HIP
        tapes of a gradient plan.  The pullback may be called any number of times until the next ``vjp`` of this module with
        the same signature.  fp32 parameters and tensors, head sizes up to 128; anything else raises ``NotImplementedError``."""
        _vjp_scope(self, x, "MultiheadSelfAttention")

        def build(plan, xin, pos_h):
            bld = plan.bld
            saved: dict = {}
            out = self._emit(bld, xin, pos_h, mask, saved=saved)
            plan.set_output(out)
            plan.end_forward([])
            g = plan.cotangent(out.C)
            plan.set_dx(self._emit_bwd(bld, g, saved, {}))

        return _token_grad_plan(self, x, pos, mask, 0, None, build).run(x, None)

    @torch.no_grad()
    @_lib.on_device
    def forward(self, x: Tensor, pos: Tensor | None = None, mask: Tensor | None = None) -> Tensor:
        r"""x: (*, L, H C) tokens; pos: (L, P) positions (RoPE only); mask: boolean (L, L) or broadcastable to
        (B, H, L, L), True = attend -> (*, L, H C)   (reference ``azula/nn/attention.py:72-110``)."""
        from .utils import backbone_io_dtype

        out_dtype = backbone_io_dtype(self, x, "azula_amd.nn.MultiheadSelfAttention")
        plan = _token_plan(self, x, pos, mask, 0, lambda bld, xin, pos_h, plan: self._emit(bld, xin, pos_h, mask))
        return plan.run(x, out_dtype=out_dtype)


def _half_act_ok(module: nn.Module) -> bool:
    r"""A token module cast to half precision can keep its activations in HBM in its own type (engine.HALF_ACT) when every
    kernel on its tape has the typed form: token widths that are multiples of 8 and at most 4096 (az_rownorm_mod_h16, 16-byte
    vectors of 8 values), SwiGLU only through the GEMM's epilogue."""
    for m in module.modules():
        if isinstance(m, MultiheadSelfAttention):
            c = m.qkv_proj.in_features
            if c % 8 or c > 4096 or (c // m.heads) % 4:
                return False
        if isinstance(m, DiTBlock):
            if m.channels % 8 or m.channels > 4096 or m.ffn[3].in_features % 8:
                return False
            if m.ffn_activation == "swiglu" and m.ffn[0].out_features % 16:
                return False
    return True


class _TokenPlan(ForwardPlan):
    r"""One-module plan on a (B, L, C) token tensor: input Act, optional modulation front, output Act."""

    def __init__(self, module: nn.Module, B: int, L: int, Cin: int, pos_h, mod_rows: int, D: int, emit, device) -> None:
        super().__init__(device, half=next(module.parameters()).dtype, half_act=_half_act_ok(module) and Cin % 8 == 0,
                         mod_rows=mod_rows, D=D)
        self.out_tokens = emit(self.bld, self.token_input(B, L, Cin), pos_h, self)
        self.end()


def _host_pos(pos: Tensor | None, L: int) -> Tensor | None:
    r"""Positions as the emitters read them: (L, P) fp32 on the host."""
    return None if pos is None else pos.detach().to("cpu", torch.float32).reshape(L, -1)


def _cached_token_plan(module, x: Tensor, pos, mask, D: int, mod: Tensor | None, make, vjp: bool = False):
    r"""The plan of a standalone token module for shapes, modulation rows and the CONTENT of positions and mask, both baked into
    it (RoPE tables, mask bytes); gradient plans under a ``"vjp"`` key beside the forward ones.  ``make(B, L, Cin, rows, pos_h)``
    builds a missing or stale plan."""
    assert x.ndim >= 2, "expected (*, L, C) tokens"
    L, Cin = x.shape[-2], x.shape[-1]
    B = x.numel() // (L * Cin)
    rows = mod_rows(mod, B, D, "block", tokens=True)
    key = (*(("vjp",) if vjp else ()), B, L, Cin, rows, str(x.device), content_key(module, pos, mask))
    return module._plans.get(key, lambda: make(B, L, Cin, rows, _host_pos(pos, L)), module)


def _token_plan(module, x: Tensor, pos, mask, D: int, emit, mod: Tensor | None = None) -> _TokenPlan:
    return _cached_token_plan(module, x, pos, mask, D, mod,
                              lambda B, L, Cin, rows, pos_h: _TokenPlan(module, B, L, Cin, pos_h, rows, D, emit, x.device))


def _vjp_scope(module: nn.Module, x: Tensor, name: str) -> None:
    r"""``gradplan.vjp_scope``, and head sizes the backward kernels reach."""
    vjp_scope(module, x, name)
    for m in module.modules():
        if isinstance(m, MultiheadSelfAttention):
            engine.attn_grad_padded_dim(m.qkv_proj.in_features // m.heads)  # (raises NotImplementedError above 128)


def _token_grad_plan(module, x: Tensor, pos, mask, D: int, mod: Tensor | None, build) -> _TokenGradTapes:
    r"""The gradient plan of a standalone token module from the same cache; ``build(plan, x_in, pos_h)`` emits both tapes."""
    def make(B, L, Cin, rows, pos_h):
        plan = _TokenGradTapes(x.device, B, L, Cin, rows, D)
        build(plan, plan.token_input(Cin), pos_h)
        return plan

    return _cached_token_plan(module, x, pos, mask, D, mod, make, vjp=True)


class DiTBlock(nn.Module):
    r"""Parameter holder of a modulated DiT block (reference ``azula/nn/dit.py:24-93``)."""

    def __init__(
        self,
        channels: int,
        mod_features: int = 0,
        ffn_factor: int = 4,
        ffn_activation: str = "silu",
        dropout: float | None = None,
        checkpointing: bool = False,
        **kwargs,
    ) -> None:
        super().__init__()
        if ffn_activation not in ("relu", "relu2", "silu", "swiglu"):
            raise NotImplementedError(f"Unknown activation '{ffn_activation}'.")
        self.channels, self.mod_features, self.ffn_activation = channels, mod_features, ffn_activation
        if mod_features > 0:
            self.ada_zero = nn.Sequential(
                nn.Linear(mod_features, mod_features), nn.SiLU(), nn.Linear(mod_features, 3 * channels), nn.Identity()
            )
            self.ada_zero[-2].weight.data.mul_(1e-2)
        else:
            self.ada_zero = nn.Parameter(torch.randn(3, channels))
            self.ada_zero.data.mul_(1e-2)
        self.msa = MultiheadSelfAttention(channels, **kwargs)
        self.ffn = nn.Sequential(
            nn.Linear(channels, ffn_factor * channels),
            nn.Identity(),  # activation (parameter-free; applied in the GEMM epilogue / az_swiglu_f32)
            nn.Identity() if dropout is None else nn.Dropout(dropout),
            nn.Linear(ffn_factor * channels // (2 if ffn_activation == "swiglu" else 1), channels),
        )
        self._plans = PlanCache()

    _ACT_KIND = {"silu": 1, "relu": 2, "relu2": 3}

    def _emit(self, bld: Builder, x: Act, pos_h, mask, D: int, mod_rows: int, mod_jobs: list, keep_input: bool = False,
              saved: dict | None = None) -> Act:
        r"""y = (a + 1) RMSNorm(x) + b;  y = y + MSA(y);  y = FFN(y);  out = x + c y   (reference ``dit.py:95-112``).

        ``saved``: a dict that receives what :meth:`_emit_bwd` reads, kept alive -- the block input ``x``, the attention layer's
        record and the FFN PRE-activation ``h`` (``ffn[0]`` then runs without its activation epilogue; the activation is a pass of
        its own behind it).  The modulated norm output and ``y2`` are only read by weight gradients, which an input gradient
        does not need: they go back to the pool either way."""
        keep = saved is not None
        C_, cs = self.channels, pad4(self.channels)
        abc, bstride = ada_zero_triple(bld, self.ada_zero, C_, D, mod_rows, mod_jobs)
        y = bld.row_norm(x, 1, scale=abc, shift=abc, scale_off=0, shift_off=cs, bstride=bstride)
        msa = {} if keep else None
        y2 = self.msa._emit(bld, y, pos_h, mask, res=y, saved=msa)
        bld.free(y)
        f0, f3 = self.ffn[0], self.ffn[3]
        glu = self.ffn_activation == "swiglu"  # x1 * silu(x2) over interleaved pairs (layers.py:107-110)
        if keep or glu:  # the activation behind the GEMM, or SwiGLU in its epilogue (act = 4) where the width allows
            code = 4 if glu and not keep and f0.out_features % 8 == 0 else 0
        else:
            code = self._ACT_KIND[self.ffn_activation]
        h = bld.conv(y2, bld.pack_conv(f0.weight, f0.bias), f0.out_features, act=code)
        bld.free(y2)
        a1 = h
        if code == 0:
            a1 = bld.swiglu(h) if glu else bld.act(h, self._ACT_KIND[self.ffn_activation])
            if not keep:
                bld.free(h)
        out = bld.conv(a1, bld.pack_conv(f3.weight, f3.bias), C_, gate=abc, gate_off=2 * cs, gate_bstride=bstride, res=x)
        bld.free(a1)
        if keep:
            saved.update(x=x, abc=abc, bstride=bstride, msa=msa, h=h, f0=LinearView(f0.weight), f3=LinearView(f3.weight))
        elif not keep_input:
            bld.free(x)
        return out

    # -- input gradient (vector-Jacobian product) -------------------------------------------------------------------
    def _emit_bwd(self, bld: Builder, g: Act, saved: dict, cache: dict) -> Act:
        r"""Cotangent of the block's output -> cotangent of its input: g_f = c g; g_y2 = ffn^T g_f; g_y = g_y2 + msa^T g_y2 (the
        add in the qkv data-gradient GEMM's epilogue); dx = g + norm^T g_y (``az_rownorm_bwd_f32`` with ``res = g``)."""
        cs = pad4(self.channels)
        abc, bstride = saved["abc"], saved["bstride"]
        g2 = bld.channel_scale(g, abc, 2 * cs, bstride)
        g3 = bld.conv_dgrad(g2, saved["f3"], cache=cache)
        bld.free(g2)
        if self.ffn_activation == "swiglu":
            g4 = bld.swiglu_bwd(g3, saved["h"])
            bld.free(g3)
        else:
            g4 = bld.act_bwd(g3, saved["h"], self._ACT_KIND[self.ffn_activation])
        g5 = bld.conv_dgrad(g4, saved["f0"], cache=cache)
        bld.free(g4)
        gy = self.msa._emit_bwd(bld, g5, saved["msa"], cache, res=g5)
        bld.free(g5)
        dx = bld.row_norm_bwd(saved["x"], gy, 1, scale=abc, scale_off=0, bstride=bstride, res=g)
        bld.free(gy)
        bld.free(g)
        return dx

    @torch.no_grad()
    @_lib.on_device
    def vjp(self, x: Tensor, mod: Tensor | None = None, pos: Tensor | None = None, mask: Tensor | None = None):
        r"""``(out, pullback)``: ``out = self(x, mod, pos, mask)`` and ``pullback(v) = (d out / d x)^T v`` (like ``x``; ``mod`` is
        a constant of the pullback), both on the HIP tapes of a gradient plan.  Callable any number of times until the next
        ``vjp`` of this module with the same signature.  fp32 parameters and tensors, head sizes up to 128."""
        _vjp_scope(self, x, "DiTBlock")
        D = self.mod_features

        def build(plan, xin, pos_h):
            bld = plan.bld
            jobs: list = []
            saved: dict = {}
            out = self._emit(bld, xin, pos_h, mask, D, plan.mod_rows, jobs, saved=saved)
            plan.set_output(out)
            plan.end_forward(jobs)
            g = plan.cotangent(out.C)
            plan.set_dx(self._emit_bwd(bld, g, saved, {}))

        return _token_grad_plan(self, x, pos, mask, D, mod, build).run(x, mod)

    @torch.no_grad()
    @_lib.on_device
    def forward(self, x: Tensor, mod: Tensor | None = None, pos: Tensor | None = None, mask: Tensor | None = None) -> Tensor:
        r"""x: (*, L, C); mod: (D) or (*, D); pos: (L, P); mask: boolean, broadcastable to (B, H, L, L) -> (*, L, C)
        (reference ``azula/nn/dit.py:114-133``)."""
        from .utils import backbone_io_dtype

        out_dtype = backbone_io_dtype(self, x, "azula_amd.nn.DiTBlock")
        D = self.mod_features

        def emit(bld, xin, pos_h, plan):
            return self._emit(bld, xin, pos_h, mask, D, plan.mod_rows, plan.mod_jobs, keep_input=True)

        return _token_plan(self, x, pos, mask, D, emit, mod).run(x, mod, out_dtype=out_dtype)


def host_sine_encoding(x: Tensor, features: int, omega: float) -> Tensor:
    r"""sin block || cos block, computed on the host in the reference's op order
    (``azula/nn/layers.py:286-299``)."""
    x = x.unsqueeze(dim=-1)
    freqs = torch.linspace(0, 1, features // 2, dtype=x.dtype)
    freqs = torch.exp(math.log(1 / omega) * freqs)
    return torch.cat((torch.sin(x * freqs), torch.cos(x * freqs)), dim=-1)


def _pos_table(net: "DiT", bld: Builder, pos: Tensor, L: int) -> Act:
    r"""The batch-shared positional embedding table (L, C) in fp32: host sine encoding -> one GEMM, run here at build time on a
    builder of its own, which the plan's tape keeps alive with the table."""
    C_ = net.hid_channels
    enc = host_sine_encoding(pos.to(torch.float32).cpu(), C_, omega=1e2).flatten(-2)  # (L, P*C)
    pb = Builder(bld.device)
    enc_act = Act(enc.to(bld.device).contiguous().reshape(-1), 1, L, 1, enc.shape[1], enc.shape[1], True)
    ptab = pb.conv(enc_act, pb.pack_conv(net.pos_embedding[2].weight, None), C_)
    pb.finish()
    pb.tape.run()
    ptab.pinned = True
    bld.tape.keep.extend([pb, enc_act, ptab])
    return ptab


class DiTPlan(ForwardPlan):
    r"""Compiled forward for (batch, tokens[, patch geometry], modulation rows)."""

    def __init__(self, net: "DiT", B: int, L: int, pos: Tensor, mod_rows: int, device, patch=None) -> None:
        D, C_ = net.mod_features, net.hid_channels
        super().__init__(device, half=next(net.parameters()).dtype, half_act=_half_act_ok(net) and C_ % 8 == 0, mod_rows=mod_rows, D=D)
        bld, mod_jobs = self.bld, self.mod_jobs
        cin = net.in_proj.in_features
        cout = net.out_proj.out_features
        if patch is not None:
            Z, H, W, p, pu = patch
            x_nchw = self.nchw_input(B, Z, H, W)
            tokens = self.tokens = bld.new_act(B, L, 1, cin, pinned=True, f32=True)  # (the plan's input stays fp32: the first GEMM rounds it per tile)
            bld.tape.add("az_patchify_f32", tokens.ptr, x_nchw.data_ptr(), None, B, Z, H, W, p, tokens.cs)
            bld.wrote(tokens, bounded=False)
        else:
            tokens = self.token_input(B, L, cin, f32=True)

        ptab = _pos_table(net, bld, pos, L)
        if bld.half_act:  # the residual operand of the first GEMM has the destination's element type
            pt = torch.zeros(L, bld.pad(C_), dtype=bld.half, device=device)
            pt[:, :C_] = ptab.buf.view(L, ptab.cs)[:, :C_]
            ptab = Act(pt.reshape(-1), 1, L, 1, C_, bld.pad(C_), True)
        self.pos_table = ptab

        x = bld.conv(tokens, bld.pack_conv(net.in_proj.weight, net.in_proj.bias), C_, res=SharedResidual(ptab))
        for blk in net.blocks:  # (all blocks' modulation MLPs read only `mod`: one GEMV + one grouped GEMV at the front)
            x = blk._emit(bld, x, pos, None, D, mod_rows, mod_jobs)
        o = bld.conv(x, bld.pack_conv(net.out_proj.weight, net.out_proj.bias), cout, out_f32=True)  # (the plan's output: fp32)
        bld.free(x)
        if patch is not None:  # '... A B (Z a b) -> ... Z (A a) (B b)' with the UNPATCH size (reference vit.py:63-74,104-106)
            Z, H, W, p, pu = patch
            Zo, Ho, Wo = cout // (pu * pu), H // p * pu, W // p * pu
            self.out = torch.empty(B, Zo, Ho, Wo, dtype=torch.float32, device=device)
            bld.tape.add("az_unpatchify_f32", self.out.data_ptr(), o.ptr, B, Zo, Ho, Wo, pu, o.cs)
        else:
            self.out_tokens = o
        self.end()


class DiTGradPlan(_TokenGradTapes):
    r"""Gradient plan of a :class:`DiT` for one (batch, tokens, positions, modulation rows) signature, alongside
    ``UNetGradPlan``: the forward-keep tape (the order of :class:`DiTPlan`, nothing the pullback reads released) and the
    backward tape (``out_proj`` data gradient, the blocks in reverse, ``in_proj`` data gradient; the positional table is a
    constant).  Plain ``Tape.run``, no graph capture; ``saved_bytes`` reports the pool."""

    def __init__(self, net: "DiT", B: int, L: int, pos: Tensor, mod_rows: int, device) -> None:
        D, C_ = net.mod_features, net.hid_channels
        cin, cout = net.in_proj.in_features, net.out_proj.out_features
        super().__init__(device, B, L, cin, mod_rows, D)
        bld = self.bld
        tokens = self.token_input(cin)
        x = bld.conv(tokens, bld.pack_conv(net.in_proj.weight, net.in_proj.bias), C_, res=SharedResidual(_pos_table(net, bld, pos, L)))
        mod_jobs: list[tuple] = []
        recs = []
        for blk in net.blocks:
            rec: dict = {}
            x = blk._emit(bld, x, pos, None, D, mod_rows, mod_jobs, saved=rec)
            recs.append((blk, rec))
        self.set_output(bld.conv(x, bld.pack_conv(net.out_proj.weight, net.out_proj.bias), cout))
        bld.free(x)  # (the last block's output: no pullback reads it)
        self.end_forward(mod_jobs)

        cache: dict = {}
        wo, wi = LinearView(net.out_proj.weight), LinearView(net.in_proj.weight)
        bld.tape.keep.extend([wo, wi])
        g = bld.conv_dgrad(self.cotangent(cout), wo, cache=cache)
        for blk, rec in reversed(recs):
            g = blk._emit_bwd(bld, g, rec, cache)
        dx = bld.conv_dgrad(g, wi, cache=cache)
        bld.free(g)
        self.set_dx(dx)


class DiT(nn.Module):
    r"""Modulated DiT-like module on token tensors (reference ``azula/nn/dit.py:135-218``)."""

    def __init__(
        self,
        in_channels: int,
        out_channels: int,
        cond_channels: int = 0,
        mod_features: int = 0,
        pos_channels: int = 1,
        hid_channels: int = 1024,
        hid_blocks: int = 3,
        **kwargs,
    ) -> None:
        super().__init__()
        self.mod_features, self.hid_channels, self.pos_channels = mod_features, hid_channels, pos_channels
        self.cond_channels = cond_channels
        self.in_proj = nn.Linear(in_channels + cond_channels, hid_channels)
        self.out_proj = nn.Linear(hid_channels, out_channels)
        self.pos_embedding = nn.Sequential(
            nn.Identity(), nn.Identity(), nn.Linear(pos_channels * hid_channels, hid_channels, bias=False)
        )
        self.pos_embedding[-1].weight.data.mul_(1e-2)
        self.blocks = nn.ModuleList([
            DiTBlock(channels=hid_channels, pos_channels=pos_channels, mod_features=mod_features, **kwargs)
            for _ in range(hid_blocks)
        ])
        self._plans = PlanCache()

    def _check_device(self, x: Tensor) -> torch.dtype:
        from .utils import backbone_io_dtype

        return backbone_io_dtype(self, x, f"azula_amd.nn.{type(self).__name__}")

    def _mod_rows(self, mod, B: int) -> int:
        return mod_rows(mod, B, self.mod_features, "network")

    def _pos(self, pos: Tensor | None, L: int) -> tuple:
        r"""(key element, host loader) of the positions a plan bakes in: ``None`` stands for the sequence indices."""
        if pos is None:
            return None, lambda: torch.arange(L, dtype=torch.float32)[:, None]
        return content_key(self, pos), lambda: _host_pos(pos, L)

    @torch.no_grad()
    @_lib.on_device
    def forward(self, x: Tensor, mod: Tensor | None = None, pos: Tensor | None = None, cond: Tensor | None = None):
        r"""x: (B, L, C_i) tokens -> (B, L, C_o).  ``pos``: (L, P) or None (sequence indices)."""
        out_dtype = self._check_device(x)
        assert x.ndim == 3, "DiT.forward expects (B, L, C) tokens"
        B, L, _ = x.shape
        rows = self._mod_rows(mod, B)
        pkey, pos_h = self._pos(pos, L)
        plan = self._plans.get((B, L, rows, pkey, str(x.device)), lambda: DiTPlan(self, B, L, pos_h(), rows, x.device), self)
        return plan.run(x, mod, cond=cond, out_dtype=out_dtype)

    # -- input gradient --------------------------------------------------------------------------------------------
    @torch.no_grad()
    @_lib.on_device
    def vjp(self, x: Tensor, mod: Tensor | None = None, pos: Tensor | None = None, cond: Tensor | None = None):
        r"""``(out, pullback)``: ``out = self(x, mod, pos)`` and ``pullback(v) = (d out / d x)^T v`` (like ``x``): the input
        gradient that ``azula.guidance`` takes from ``torch.autograd``, on HIP tapes (:class:`DiTGradPlan`).  ``mod`` and the
        positions are constants of the pullback; it may be called any number of times until the next ``vjp`` with the same
        signature.  Scope: fp32 parameters and tensors, no ``cond_channels`` / ``cond``, head sizes up to 128; anything else
        raises ``NotImplementedError`` (the forward is not affected)."""
        if self.cond_channels or cond is not None:
            raise NotImplementedError("DiT.vjp: cond_channels / cond are not supported")
        _vjp_scope(self, x, "DiT")
        assert x.ndim == 3, "DiT.vjp expects (B, L, C) tokens"
        B, L, _ = x.shape
        rows = self._mod_rows(mod, B)
        pkey, pos_h = self._pos(pos, L)
        plan = self._plans.get(("vjp", B, L, rows, pkey, str(x.device)), lambda: DiTGradPlan(self, B, L, pos_h(), rows, x.device), self)
        return plan.run(x, mod)


def _patchify_nd(x: Tensor, patch: Sequence[int]) -> Tensor:
    r"""'B Z (A a) (B b) ... -> B A B ... (Z a b ...)'."""
    B, Z, *dims = x.shape
    n = len(patch)
    assert len(dims) == n and all(d % p == 0 for d, p in zip(dims, patch)), (x.shape, patch)
    x = x.reshape(B, Z, *[v for d, p in zip(dims, patch) for v in (d // p, p)])
    grid_axes = [2 + 2 * i for i in range(n)]
    patch_axes = [3 + 2 * i for i in range(n)]
    x = x.permute(0, *grid_axes, 1, *patch_axes)
    return x.reshape(B, *[d // p for d, p in zip(dims, patch)], Z * math.prod(patch))


def _unpatchify_nd(y: Tensor, patch: Sequence[int]) -> Tensor:
    r"""'B A B ... (Z a b ...) -> B Z (A a) (B b) ...'."""
    B, *grid, F = y.shape
    n = len(patch)
    Z = F // math.prod(patch)
    y = y.reshape(B, *grid, Z, *patch)
    order = [0, 1 + n] + [v for i in range(n) for v in (1 + i, 2 + n + i)]
    return y.permute(*order).reshape(B, Z, *[g * p for g, p in zip(grid, patch)])


class ViT(DiT):
    r"""Modulated ViT-like module on images (reference ``azula/nn/vit.py:22-108``)."""

    def __init__(
        self,
        in_channels: int,
        out_channels: int,
        cond_channels: int = 0,
        mod_features: int = 0,
        hid_channels: int = 1024,
        hid_blocks: int = 3,
        spatial: int = 2,
        patch_size: int | Sequence[int] = 1,
        unpatch_size: int | Sequence[int] | None = None,
        **kwargs,
    ) -> None:
        if isinstance(patch_size, int):
            patch_size = [patch_size] * spatial
        if unpatch_size is None:
            unpatch_size = patch_size
        elif isinstance(unpatch_size, int):
            unpatch_size = [unpatch_size] * spatial
        assert len(patch_size) == len(unpatch_size) == spatial
        super().__init__(
            in_channels=math.prod(patch_size) * in_channels, out_channels=math.prod(unpatch_size) * out_channels,
            cond_channels=math.prod(patch_size) * cond_channels, mod_features=mod_features, pos_channels=spatial,
            hid_channels=hid_channels, hid_blocks=hid_blocks, **kwargs,
        )
        self.patch_shape, self.unpatch_shape = tuple(patch_size), tuple(unpatch_size)
        # images with square patches take the fused patchify / unpatchify kernels (and the captured sampling graph);
        # any other geometry (1-D, 3-D, anisotropic patches) rearranges with torch index ops around the token network
        self.native = spatial == 2 and len(set(patch_size)) == 1 and len(set(unpatch_size)) == 1
        self.patch_size, self.unpatch_size = patch_size[0], unpatch_size[0]
        self.image_in, self.image_out, self.image_cond = in_channels, out_channels, cond_channels
        self.spatial = spatial

    # The token network's pullback is DiT.vjp; a ViT also needs the patchify / unpatchify pullbacks around it.  That follow-up
    # flips tests/test_guidance_vjp_host.py::test_backbone_error_names_the_backbone and
    # tests/test_gpu_tds.py::test_vit_backbone_is_an_error; until then a ViT has no input-gradient path.
    vjp = None

    def _vit_plan(self, B: int, H: int, W: int, rows: int, device) -> DiTPlan:
        p = self.patch_size
        Hp, Wp = H // p, W // p
        pos = torch.cartesian_prod(torch.arange(Hp, dtype=torch.float32), torch.arange(Wp, dtype=torch.float32))
        pos = pos.reshape(-1, 2)
        return self._plans.get(
            ("vit", B, H, W, rows, str(device)),
            lambda: DiTPlan(self, B, Hp * Wp, pos, rows, device, patch=(self.image_in + self.image_cond, H, W, p, self.unpatch_size)),
            self,
        )

    @torch.no_grad()
    @_lib.on_device
    def forward(self, x: Tensor, mod: Tensor | None = None, cond: Tensor | None = None) -> Tensor:
        r"""x: (B, C_i, H, W); mod: (D) or (B, D) -> (B, C_o, H, W)."""
        out_dtype = self._check_device(x)
        assert (cond is not None) == (self.image_cond > 0), "pass cond iff the network was built with cond_channels"
        if not self.native:
            return self._forward_rearranged(x, mod, cond)
        B, Z, H, W = x.shape
        assert Z == self.image_in and H % self.patch_size == 0 and W % self.patch_size == 0
        rows = self._mod_rows(mod, B)
        # patchify(x) || patchify(cond) along the token features == patchify of the channel concatenation: the
        # feature index is (channel, a, b) with the channel slowest (reference vit.py:92-96, layers.py:198-222)
        return self._vit_plan(B, H, W, rows, x.device).run(x, mod, cond=cond, out_dtype=out_dtype)

    def _forward_rearranged(self, x: Tensor, mod, cond) -> Tensor:
        r"""Any number of spatial dimensions / anisotropic patches: ``Patchify`` and ``Unpatchify`` (reference
        ``azula/nn/layers.py:198-247``, channel_last) as torch reshapes around the compiled token network."""
        assert x.ndim == 2 + self.spatial and x.shape[1] == self.image_in
        t = _patchify_nd(x, self.patch_shape)
        grid = t.shape[1:-1]
        pos = torch.cartesian_prod(*(torch.arange(n, dtype=torch.float32) for n in grid)).reshape(-1, len(grid))
        t = t.flatten(1, -2)
        c = None if cond is None else _patchify_nd(cond, self.patch_shape).flatten(1, -2)
        y = DiT.forward(self, t, mod, pos=pos, cond=c)
        return _unpatchify_nd(y.unflatten(1, grid), self.unpatch_shape)

    # -- fused sampling ---------------------------------------------------------------------------
    def _az_compile_modulated(self, x: Tensor, mod_rows: int = 1):
        if not self.native:
            return None
        if self.mod_features == 0 or x.ndim != 4 or self.image_cond or self.unpatch_size != self.patch_size:
            return None  # cond / a different output geometry: the generic step loop (eager forward per step)
        self._check_device(x)
        B, _, H, W = x.shape
        plan = self._vit_plan(B, H, W, mod_rows, x.device)
        return plan.program(self.image_out), plan.mod
