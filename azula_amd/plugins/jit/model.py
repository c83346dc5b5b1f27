r"""JiT ("Just image Transformer") backbone executed by gfx950 kernels.

Parameter holder with the ``state_dict`` keys of the reference's vendored model
(``azula/plugins/jit/_src/model.py:218-381``, from LTH14/JiT) plus a compiled forward built from the
same kernels as ``azula_amd.nn.vit``:

* bottleneck patch embedding = patchify remap + two MFMA GEMMs, the fixed sin-cos positional table
  added in the second GEMM's epilogue;
* conditioning c = MLP(sinusoid(t)) + label embedding: ``az_timestep_embedding_f32``, the small-M
  linear kernel, ``az_gather_rows_f32``; the 6-way adaLN projections of ALL blocks (and the final layer's) are
  one MFMA GEMM on SiLU(c), issued once per forward;
* block: weighted RMSNorm + modulate is one row pass (``az_rownorm_mod_f32``); the q/k RMSNorm gains,
  the 2-D rotary embedding and the 1/sqrt(d) scale are folded into the attention kernel's operand loads
  ('(3 H C)' fused-QKV layout read in place); ``x + gate * proj(.)`` and ``x + gate * w3(.)`` are GEMM
  epilogues; SwiGLU reads w12's output once (w12's rows are interleaved at build time so the kernel's
  pair layout applies);
* the in-context class tokens are prepended by two token-window kernels at ``in_context_start`` and dropped
  before the final layer; the final linear's rows are permuted at build time from the model's (p, q, c)
  feature order to the unpatchify kernel's (c, p, q).

``JiT.vjp`` is the input gradient on a plan of its own (:class:`JiTGradPlan`); ``JiTPlan`` does not change.
"""

from __future__ import annotations

import math
import weakref

import torch
import torch.nn as nn
from torch import Tensor

from ... import _lib, engine
from ...engine import Act, LinearView, PlanCache, SharedResidual, param_versions
from ...gradplan import _GradTapes, vjp_scope
from ...plan import ForwardPlan

__all__ = ["JiT", "JiTGradPlan", "JiT_models"]


class _Gain(nn.Module):
    r"""RMSNorm gain holder (``_src/util.py:149-157``): key ``weight``."""

    def __init__(self, n: int) -> None:
        super().__init__()
        self.weight = nn.Parameter(torch.ones(n))


class _Attention(nn.Module):
    def __init__(self, dim: int, heads: int) -> None:
        super().__init__()
        self.q_norm, self.k_norm = _Gain(dim // heads), _Gain(dim // heads)
        self.qkv = nn.Linear(dim, 3 * dim)
        self.proj = nn.Linear(dim, dim)


class _SwiGLU(nn.Module):
    def __init__(self, dim: int, hidden: int) -> None:
        super().__init__()
        hidden = int(hidden * 2 / 3)  # _src/model.py:153
        self.w12 = nn.Linear(dim, 2 * hidden)
        self.w3 = nn.Linear(hidden, dim)


def _ada(dim: int, ways: int) -> nn.Sequential:
    seq = nn.Sequential(nn.SiLU(), nn.Linear(dim, ways * dim))
    nn.init.zeros_(seq[1].weight)
    nn.init.zeros_(seq[1].bias)
    return seq


class _Block(nn.Module):
    def __init__(self, dim: int, heads: int, mlp_ratio: float) -> None:
        super().__init__()
        self.norm1 = _Gain(dim)
        self.attn = _Attention(dim, heads)
        self.norm2 = _Gain(dim)
        self.mlp = _SwiGLU(dim, int(dim * mlp_ratio))
        self.adaLN_modulation = _ada(dim, 6)


class _Final(nn.Module):
    def __init__(self, dim: int, patch: int, channels: int) -> None:
        super().__init__()
        self.norm_final = _Gain(dim)
        self.linear = nn.Linear(dim, patch * patch * channels)
        self.adaLN_modulation = _ada(dim, 2)
        nn.init.zeros_(self.linear.weight)
        nn.init.zeros_(self.linear.bias)


def sincos_table(dim: int, grid: int) -> Tensor:
    r"""Fixed 2-D sin-cos positional table (grid^2, dim): the column index drives the first half of the
    features, the row index the second; each half is [sin | cos] over dim/4 log-spaced frequencies
    (fp64, reference ``_src/util.py:166-212``)."""
    omega = 1.0 / 10000 ** (torch.arange(dim // 4, dtype=torch.float64) / (dim / 4.0))
    idx = torch.arange(grid, dtype=torch.float64)
    ang = idx[:, None] * omega[None]
    enc = torch.cat((ang.sin(), ang.cos()), dim=1)  # (grid, dim / 2)
    cols = enc[None, :, :].expand(grid, grid, -1)
    rows = enc[:, None, :].expand(grid, grid, -1)
    return torch.cat((cols, rows), dim=-1).reshape(grid * grid, dim).float()


def rotary_tables(head_dim: int, heads: int, grid: int, ctx: int) -> tuple[Tensor, Tensor]:
    r"""cos / sin of the rotation angle per (token, head, channel pair), laid out as ``az_attention_f32``
    reads them: (ctx + grid^2, heads, head_dim / 2).  Pairs [0, d/4) turn with the patch row, [d/4, d/2)
    with the patch column, frequencies 10000^(-2j / (d/2)); context tokens are not rotated
    (reference ``_src/util.py:100-143`` with dim = head_dim / 2)."""
    quarter = head_dim // 4
    freqs = 1.0 / (10000.0 ** (torch.arange(0, head_dim // 2, 2)[:quarter].float() / (head_dim // 2)))
    pos = torch.arange(grid) / grid * grid
    ang = pos[:, None] * freqs[None]  # (grid, d/4)
    full = torch.cat((ang[:, None, :].expand(grid, grid, quarter), ang[None, :, :].expand(grid, grid, quarter)), dim=-1)
    full = full.reshape(grid * grid, 2 * quarter)
    cos, sin = full.cos(), full.sin()
    if ctx:
        cos = torch.cat((torch.ones(ctx, 2 * quarter), cos))
        sin = torch.cat((torch.zeros(ctx, 2 * quarter), sin))
    expand = lambda t: t[:, None, :].expand(-1, heads, -1).contiguous()  # noqa: E731
    return expand(cos), expand(sin)


def _emit_forward(plan, net: "JiT", B: int, t_shared: bool, x_nchw: Tensor, out_nchw: Tensor, keep: bool = False) -> dict:
    r"""The network on ``plan.bld``'s tape, from the planar ``x_nchw`` to the planar ``out_nchw``: the conditioning front and its
    one modulation GEMM, the patch embedding, the blocks with the class tokens joining and leaving, the final layer.  Sets the
    plan's ``t`` and ``labels`` inputs.

    ``keep``: the forward-keep tape of :class:`JiTGradPlan` (fp32).  Kept per block: the block input (``norm1``'s pullback), the
    attention record -- raw qkv, q^ | k^ from ``az_qk_prep_w_f32`` (``Builder.attention_keep`` with the gains; the qkv projection
    runs without its q / k epilogue, heads padded to the backward kernels' sizes), the attention output --, ``x2`` (``norm2``) and
    the w12 pre-activation (SwiGLU is a pass of its own behind it).  Returns what the backward tape reads."""
    bld, device = plan.bld, plan.bld.device
    tape = bld.tape
    Hd, heads, p, Z = net.hidden_size, net.num_heads, net.patch_size, net.in_channels
    S = net.input_size
    grid = S // p
    L, Lc = grid * grid, net.in_context_len
    hd = Hd // heads
    depth, start = len(net.blocks), net.in_context_start
    joins = bool(Lc) and start < depth  # (the class tokens enter the sequence at block `start`)
    plan.t = torch.zeros(1 if t_shared else B, dtype=torch.float32, device=device)
    plan.labels = torch.zeros(B, dtype=torch.int64, device=device)

    # ---- conditioning: c = t_embedder(t) + y_embedder(y)     (_src/model.py:353-355); constants of a pullback
    F_ = net.t_embedder.frequency_embedding_size
    m0, m2 = net.t_embedder.mlp[0], net.t_embedder.mlp[2]
    table = net.y_embedder.embedding_table.weight
    freq, hid, t_emb, y_emb, c = (bld.empty(B, n) for n in (F_, Hd, Hd, Hd, Hd))
    ones = bld.const(torch.ones(1))
    tape.add("az_timestep_embedding_f32", freq.data_ptr(), F_, plan.t.data_ptr(), 0 if t_shared else 1, B, F_ // 2, 10000.0)
    bld.linear_small(hid, Hd, freq, F_, bld.const(m0.weight), bld.const(m0.bias), B, Hd, F_, 0, 1)
    bld.linear_small(t_emb, Hd, hid, Hd, bld.const(m2.weight), bld.const(m2.bias), B, Hd, Hd, 0, 0)
    tape.add("az_gather_rows_f32", y_emb.data_ptr(), bld.const(table).data_ptr(), plan.labels.data_ptr(), B, Hd, table.shape[0])
    tape.add("az_axpby_f32", c.data_ptr(), ones.data_ptr(), t_emb.data_ptr(), ones.data_ptr(), y_emb.data_ptr(), 1, B * Hd, 0)
    # every adaLN projection reads only SiLU(c): the 6-way projections of all blocks and the final layer's
    # 2-way one are ONE GEMM (B x Hd) @ (Hd x (6 depth + 2) Hd) on the MFMA kernel, issued once per forward
    heads_ = [blk.adaLN_modulation[1] for blk in net.blocks] + [net.final_layer.adaLN_modulation[1]]
    w_all = torch.cat([m.weight.detach() for m in heads_]).to(device)
    b_all = torch.cat([m.bias.detach() for m in heads_]).to(device)
    c_act = Act(bld.empty(B * Hd), 1, B, 1, Hd, Hd, True)
    tape.add("az_silu_f32", c_act.ptr, c.data_ptr(), B * Hd)
    bld.wrote(c_act, bounded=False)
    mods = bld.conv(c_act, bld.pack_conv(w_all, b_all), w_all.shape[0], out_f32=True)  # (the modulation table stays fp32)
    mods.pinned = True
    mod, MS = mods.buf, mods.cs  # row stride of the modulation table

    # ---- bottleneck patch embedding + fixed positional table  (_src/model.py:16-43,358-359)
    e = net.x_embedder
    tokens = bld.new_act(B, L, 1, Z * p * p, pinned=True, f32=True)  # (the plan's input stays fp32)
    tape.add("az_patchify_f32", tokens.ptr, x_nchw.data_ptr(), None, B, Z, S, S, p, tokens.cs)
    bld.wrote(tokens, bounded=False)
    low = bld.conv(tokens, bld.pack_conv(e.proj1.weight.detach().reshape(e.proj1.out_channels, -1), None), e.proj1.out_channels)
    pos_t = bld.const(net.pos_embed.detach().reshape(-1))
    if bld.half_act:  # (the residual operand has the destination's element type)
        pos_t = pos_t.to(bld.half)
        tape.keep.append(pos_t)
    x = bld.conv(low, bld.pack_conv(e.proj2.weight.detach().reshape(Hd, -1), e.proj2.bias), Hd,
                 res=SharedResidual(Act(pos_t, 1, L, 1, Hd, Hd, True)))
    bld.free(low)

    # a head size the kernels are not instantiated for: zero-padded heads (engine.ATTN_HEAD_DIMS)
    hdp = engine.attn_grad_padded_dim(hd) if keep else engine.attn_padded_dim(hd, bld.half)

    def rope_tables(ctx: int) -> tuple:
        cos, sin = rotary_tables(hd, heads, grid, ctx)  # (tokens, heads, hd / 2)
        if hdp != hd:  # padded pairs do not turn
            cos = torch.cat([cos, cos.new_ones(*cos.shape[:-1], (hdp - hd) // 2)], dim=-1).contiguous()
            sin = torch.cat([sin, sin.new_zeros(*sin.shape[:-1], (hdp - hd) // 2)], dim=-1).contiguous()
        return bld.const(cos), bld.const(sin)

    rope_img = rope_tables(0)
    rope_ctx = rope_tables(Lc) if Lc else rope_img
    recs = []
    for i, blk in enumerate(net.blocks):
        if joins and i == start:  # prepend the class tokens (_src/model.py:364-367); no pullback reads the narrow copy
            wide = bld.new_act(B, L + Lc, 1, Hd)
            ctx_pos = bld.const(net.in_context_posemb.detach().reshape(-1))
            if wide.half:  # 2-byte tokens: typed fill; the copy moves Hd / 2 floats per token
                tape.add("az_token_fill_h16", wide.ptr, L + Lc, 0, Lc, y_emb.data_ptr(), Hd, ctx_pos.data_ptr(), B, Hd, 2 if bld.half == torch.float16 else 1)
                tape.add("az_token_copy_f32", wide.ptr, L + Lc, Lc, x.ptr, L, 0, L, B, Hd // 2)
            else:
                tape.add("az_token_fill_f32", wide.ptr, L + Lc, 0, Lc, y_emb.data_ptr(), Hd, ctx_pos.data_ptr(), B, Hd)
                tape.add("az_token_copy_f32", wide.ptr, L + Lc, Lc, x.ptr, L, 0, L, B, Hd)
            bld.wrote(wide, bounded=False)
            bld.free(x)
            x = wide
        m0_ = 6 * Hd * i  # this block's columns: shift_a | scale_a | gate_a | shift_m | scale_m | gate_m
        at = blk.attn
        norm1, norm2 = bld.const(blk.norm1.weight), bld.const(blk.norm2.weight)
        n1 = bld.row_norm(x, 1, weight=norm1, scale=mod, shift=mod, scale_off=m0_ + Hd, shift_off=m0_, bstride=MS, eps=1e-6)
        rope_i = rope_img if i < start else rope_ctx
        wq, bq, wp = at.qkv.weight.detach(), at.qkv.bias, at.proj.weight.detach()
        if hdp != hd:  # gain 1 on the pad lanes
            pad1 = torch.ones(hdp - hd)
            gains = tuple(bld.const(torch.cat([w_.detach().float().cpu(), pad1])) for w_ in (at.q_norm.weight, at.k_norm.weight))
            wq, bq = engine.pad_qkv_heads(wq, bq, heads, hd, hdp, "3HC")
            wp = engine.pad_proj_heads(wp, heads, hd, hdp)
        else:
            gains = (bld.const(at.q_norm.weight), bld.const(at.k_norm.weight))
        scale, norm_dim = 1.0 / math.sqrt(hd), (hd if hdp != hd else 0)
        if keep:
            qkv = bld.conv(n1, bld.pack_conv(wq, bq), 3 * heads * hdp)
            bld.free(n1)
            att, arec = bld.attention_keep(qkv, heads, True, scale, eps=1e-6, rope=rope_i, norm_dim=norm_dim, order="3HC", qk_weight=gains)
        else:
            # q / k RMS norm, gains and RoPE in the projection's epilogue, once per layer (padded heads -- head_dim 80 of JiT-H --: in
            # the attention kernel)
            prep = dict(heads=heads, head_dim=hd, rmsnorm=True, eps=1e-6, rope=rope_i, weight=gains) if hdp == hd else None
            qkv = bld.conv(n1, bld.pack_conv(wq, bq), 3 * heads * hdp, qk_prep=prep)
            bld.free(n1)
            att = bld.attention(qkv, heads, "3HC", True, scale, eps=1e-6, rope=rope_i, qk_weight=gains, norm_dim=norm_dim)
            bld.free(qkv)
        x2 = bld.conv(att, bld.pack_conv(wp, at.proj.bias), Hd, gate=mod, gate_off=m0_ + 2 * Hd, gate_bstride=MS, res=x)
        if not keep:
            bld.free(att)
            bld.free(x)
        n2 = bld.row_norm(x2, 1, weight=norm2, scale=mod, shift=mod, scale_off=m0_ + 4 * Hd, shift_off=m0_ + 3 * Hd, bstride=MS, eps=1e-6)
        # silu(x1) * x2 over halves (_src/model.py:159-162) -> interleave rows: pair (x2_c, x1_c)
        w12, b12 = blk.mlp.w12.weight.detach(), blk.mlp.w12.bias.detach()
        half = w12.shape[0] // 2
        w12i = torch.stack((w12[half:], w12[:half]), dim=1).reshape(2 * half, -1).contiguous()
        b12i = torch.stack((b12[half:], b12[:half]), dim=1).reshape(-1).contiguous()
        # SwiGLU in the GEMM's epilogue (AzConvArgs.act = 4): no separate pass over the 4096-wide tensor
        fused = not keep and half % 4 == 0
        h = bld.conv(n2, bld.pack_conv(w12i, b12i), 2 * half, act=4 if fused else 0)
        bld.free(n2)
        glu = h
        if not fused:
            glu = bld.swiglu(h)
            if not keep:
                bld.free(h)
        out = bld.conv(glu, bld.pack_conv(blk.mlp.w3.weight, blk.mlp.w3.bias), Hd, gate=mod, gate_off=m0_ + 5 * Hd, gate_bstride=MS,
                       res=x2)
        bld.free(glu)
        if keep:
            recs.append(dict(x=x, attn=arec, x2=x2, h=h, m0=m0_, norm1=norm1, norm2=norm2, wqkv=LinearView(wq), wproj=LinearView(wp),
                             w12=LinearView(w12i), w3=LinearView(blk.mlp.w3.weight)))
        else:
            bld.free(x2)
        x = out
    if joins:  # x[:, in_context_len:]
        body = bld.new_act(B, L, 1, Hd)
        tape.add("az_token_copy_f32", body.ptr, L, 0, x.ptr, L + Lc, Lc, L, B, Hd // 2 if body.half else Hd)
        bld.wrote(body, bounded=False)
        bld.free(x)
        x = body

    # ---- final layer + unpatchify 'nhwpqc->nchpwq'          (_src/model.py:166-184,331-344)
    fl = net.final_layer
    mf = 6 * Hd * depth  # final layer's columns: shift | scale
    norm_f = bld.const(fl.norm_final.weight)
    n = bld.row_norm(x, 1, weight=norm_f, scale=mod, shift=mod, scale_off=mf + Hd, shift_off=mf, bstride=MS, eps=1e-6)
    if not keep:  # (kept: norm_final's pullback reads it)
        bld.free(x)
    wl = fl.linear.weight.detach().reshape(p * p, Z, Hd).transpose(0, 1).reshape(Z * p * p, Hd).contiguous()
    bl = fl.linear.bias.detach().reshape(p * p, Z).t().reshape(-1).contiguous()
    o = bld.conv(n, bld.pack_conv(wl, bl), Z * p * p, out_f32=True)  # (the plan's output: fp32 tokens for the unpatchify pass)
    bld.free(n)
    tape.add("az_unpatchify_f32", out_nchw.data_ptr(), o.ptr, B, Z, S, S, p, o.cs)
    bld.free(o)
    return dict(recs=recs, x_last=x, norm_f=norm_f, wl=wl, w1=LinearView(e.proj1.weight), w2=LinearView(e.proj2.weight), mods=mods, mf=mf,
                joins=joins)


class JiTPlan(ForwardPlan):
    r"""Compiled forward for one (batch, shared/per-sample time) signature."""

    def __init__(self, net: "JiT", B: int, t_shared: bool, device) -> None:
        # a network cast to half precision keeps its activations in HBM in its own type (engine.HALF_ACT): widths in multiples of 8,
        # SwiGLU through the GEMM's epilogue
        half_act = net.hidden_size % 8 == 0 and all((blk.mlp.w12.weight.shape[0] // 2) % 8 == 0 for blk in net.blocks) and net.hidden_size <= 4096
        super().__init__(device, half=net.pos_embed.dtype, half_act=half_act)
        Z, S = net.in_channels, net.input_size
        self.out = torch.empty(B, Z, S, S, dtype=torch.float32, device=device)
        _emit_forward(self, net, B, t_shared, self.nchw_input(B, Z, S, S), self.out)
        self.end()


class JiTGradPlan(_GradTapes):
    r"""Gradient plan of a :class:`JiT` for one (batch, shared/per-sample time) signature, alongside ``DiTGradPlan``: the
    forward-keep tape (:class:`JiTPlan`'s walk in its keep form, :func:`_emit_forward`) and the backward tape, on planar
    (B, C, S, S) buffers.  ``t`` and ``y`` are constants of the pullback, so the modulation table is one.

    The backward tape reads a block right to left: gate, w3 and w12 data gradients around ``az_swiglu_bwd_f32``,
    ``az_rownorm_bwd_w_f32`` with ``res = g``; gate, proj data gradient, ``az_attention_bwd_f32`` + ``az_qk_prep_bwd_w_f32``, qkv data
    gradient, ``az_rownorm_bwd_w_f32`` with the residual path's cotangent as ``res``.  The class tokens do not depend on x: where
    they join, the cotangent drops their rows; where they leave, it is copied behind zeroed rows.  Unpatchify and patchify are each
    other's adjoints.  Plain ``Tape.run``, no graph capture; ``saved_bytes`` reports the pool."""

    def __init__(self, net: "JiT", B: int, t_shared: bool, device) -> None:
        Hd, p, Z = net.hidden_size, net.patch_size, net.in_channels
        S = net.input_size
        super().__init__(device, B, Z, Z, S, S, 0, 0)
        self._net = weakref.ref(net)
        bld = self.bld
        L, Lc = (S // p) ** 2, net.in_context_len
        depth, start = len(net.blocks), net.in_context_start
        kept = _emit_forward(self, net, B, t_shared, self.x_in, self.out, keep=True)
        recs, x_last, norm_f, wl, w1, w2, mods, mf, joins = (kept[k] for k in ("recs", "x_last", "norm_f", "wl", "w1", "w2", "mods", "mf", "joins"))
        mod, MS = mods.buf, mods.cs
        self.end_forward([])

        # ---- backward
        tape = bld.tape
        cache: dict = {}
        wlv = LinearView(wl)
        tape.keep.extend([wlv, w1, w2, mods] + [r[k] for r in recs for k in ("wqkv", "wproj", "w12", "w3")])
        g = bld.new_act(B, L, 1, Z * p * p)
        tape.add("az_patchify_f32", g.ptr, self.v_in.data_ptr(), None, B, Z, S, S, p, g.cs)  # (the unpatchify's adjoint)
        bld.wrote(g, bounded=False)
        gn = bld.conv_dgrad(g, wlv, cache=cache)
        bld.free(g)
        g = bld.row_norm_bwd(x_last, gn, 1, scale=mod, scale_off=mf + Hd, bstride=MS, eps=1e-6, weight=norm_f)
        bld.free(gn)
        if joins:  # the slice's adjoint: zero rows for the class tokens (a launch of its own: the pool reuses the buffer)
            gw = bld.new_act(B, L + Lc, 1, Hd)
            zrow, zpos = bld.const(torch.zeros(Hd)), bld.const(torch.zeros(Lc * Hd))
            tape.add("az_token_fill_f32", gw.ptr, L + Lc, 0, Lc, zrow.data_ptr(), 0, zpos.data_ptr(), B, Hd, keep=[zrow, zpos])
            tape.add("az_token_copy_f32", gw.ptr, L + Lc, Lc, g.ptr, L, 0, L, B, Hd)
            bld.wrote(gw, bounded=False)
            bld.free(g)
            g = gw
        for i in range(depth - 1, -1, -1):
            r = recs[i]
            m0_ = r["m0"]
            g2 = bld.channel_scale(g, mod, m0_ + 5 * Hd, MS)
            g3 = bld.conv_dgrad(g2, r["w3"], cache=cache)
            bld.free(g2)
            g4 = bld.swiglu_bwd(g3, r["h"])
            bld.free(g3)
            g5 = bld.conv_dgrad(g4, r["w12"], cache=cache)
            bld.free(g4)
            gx2 = bld.row_norm_bwd(r["x2"], g5, 1, scale=mod, scale_off=m0_ + 4 * Hd, bstride=MS, res=g, eps=1e-6, weight=r["norm2"])
            bld.free(g5)
            bld.free(g)
            g6 = bld.channel_scale(gx2, mod, m0_ + 2 * Hd, MS)
            g7 = bld.conv_dgrad(g6, r["wproj"], cache=cache)
            bld.free(g6)
            g8 = bld.attention_bwd(g7, r["attn"])
            bld.free(g7)
            g9 = bld.conv_dgrad(g8, r["wqkv"], cache=cache)
            bld.free(g8)
            g = bld.row_norm_bwd(r["x"], g9, 1, scale=mod, scale_off=m0_ + Hd, bstride=MS, res=gx2, eps=1e-6, weight=r["norm1"])
            bld.free(g9)
            bld.free(gx2)
            if joins and i == start:  # the class tokens do not depend on x: their rows of the cotangent are dropped
                gb = bld.new_act(B, L, 1, Hd)
                tape.add("az_token_copy_f32", gb.ptr, L, 0, g.ptr, L + Lc, Lc, L, B, Hd)
                bld.wrote(gb, bounded=False)
                bld.free(g)
                g = gb
        glow = bld.conv_dgrad(g, w2, cache=cache)
        bld.free(g)
        gt = bld.conv_dgrad(glow, w1, cache=cache)
        bld.free(glow)
        tape.add("az_unpatchify_f32", self.dx.data_ptr(), gt.ptr, B, Z, S, S, p, gt.cs)  # (the patchify's adjoint)
        bld.free(gt)
        self.end_backward()

    def run_jit(self, x: Tensor, t: Tensor, y: Tensor):
        self.t.copy_(t.to(device=x.device, dtype=torch.float32))
        self.labels.copy_(y.to(device=x.device, dtype=torch.int64).expand(self.labels.shape[0]))
        out, pull = self.run(x, None)
        net = self._net
        versions = param_versions(net())

        def pullback(v: Tensor) -> Tensor:
            # the tapes read the norm gains, biases and tables where the module keeps them, the GEMM weights from packed copies:
            # after an in-place parameter change the saved tensors no longer belong to what the backward tape would read
            m = net()
            if m is None or param_versions(m) != versions:
                raise RuntimeError("this pullback belongs to an earlier vjp call: the module's parameters have changed since, "
                                   "and its saved tensors belong to the old ones")
            return pull(v)

        return out, pullback


class _TimestepEmbedder(nn.Module):
    def __init__(self, hidden: int, frequency_embedding_size: int = 256) -> None:
        super().__init__()
        self.mlp = nn.Sequential(nn.Linear(frequency_embedding_size, hidden), nn.SiLU(), nn.Linear(hidden, hidden))
        self.frequency_embedding_size = frequency_embedding_size
        nn.init.normal_(self.mlp[0].weight, std=0.02)
        nn.init.normal_(self.mlp[2].weight, std=0.02)


class _LabelEmbedder(nn.Module):
    def __init__(self, num_classes: int, hidden: int) -> None:
        super().__init__()
        self.embedding_table = nn.Embedding(num_classes + 1, hidden)  # + the "null" class of CFG
        nn.init.normal_(self.embedding_table.weight, std=0.02)


class _PatchEmbed(nn.Module):
    def __init__(self, patch: int, channels: int, bottleneck: int, hidden: int) -> None:
        super().__init__()
        self.proj1 = nn.Conv2d(channels, bottleneck, kernel_size=patch, stride=patch, bias=False)
        self.proj2 = nn.Conv2d(bottleneck, hidden, kernel_size=1)
        nn.init.xavier_uniform_(self.proj1.weight.data.view(bottleneck, -1))
        nn.init.xavier_uniform_(self.proj2.weight.data.view(hidden, -1))
        nn.init.zeros_(self.proj2.bias)


class JiT(nn.Module):
    r"""Just image Transformer (reference ``_src/model.py:218-381``): class- and time-conditional pixel-space
    DiT with a bottleneck patch embedding, 6-way adaLN-zero blocks, SwiGLU FFN, q/k RMSNorm, 2-D rotary
    attention and ``in_context_len`` class tokens joining the sequence at block ``in_context_start``.

    ``forward(x, t, y)``: x (B, C, S, S), t (B,) or (1,), y (B,) int64 -> (B, C, S, S)."""

    def __init__(
        self,
        input_size: int = 256,
        patch_size: int = 16,
        in_channels: int = 3,
        hidden_size: int = 1024,
        depth: int = 24,
        num_heads: int = 16,
        mlp_ratio: float = 4.0,
        attn_drop: float = 0.0,
        proj_drop: float = 0.0,
        num_classes: int = 1000,
        bottleneck_dim: int = 128,
        in_context_len: int = 32,
        in_context_start: int = 8,
    ) -> None:
        super().__init__()
        if hidden_size % num_heads or hidden_size // num_heads > 128 or (hidden_size // num_heads) % 4:
            raise NotImplementedError(  # (the rotary layout splits a head into quarters: reference _src/util.py:100-143)
                f"head_dim {hidden_size / num_heads:g}: the gfx950 attention kernels take heads of up to 128 channels "
                "(16/32/64/80/128 natively, other multiples of 4 zero-padded to the next of those)"
            )
        if input_size % patch_size or hidden_size % 8:
            raise ValueError("input_size must be a multiple of patch_size and hidden_size of 8")
        self.in_channels = self.out_channels = in_channels
        self.patch_size, self.num_heads, self.hidden_size, self.input_size = patch_size, num_heads, hidden_size, input_size
        self.in_context_len, self.in_context_start, self.num_classes = in_context_len, in_context_start, num_classes
        self.t_embedder = _TimestepEmbedder(hidden_size)
        self.y_embedder = _LabelEmbedder(num_classes, hidden_size)
        self.x_embedder = _PatchEmbed(patch_size, in_channels, bottleneck_dim, hidden_size)
        grid = input_size // patch_size
        self.pos_embed = nn.Parameter(sincos_table(hidden_size, grid)[None], requires_grad=False)
        if in_context_len > 0:
            self.in_context_posemb = nn.Parameter(0.02 * torch.randn(1, in_context_len, hidden_size))
        self.blocks = nn.ModuleList([_Block(hidden_size, num_heads, mlp_ratio) for _ in range(depth)])
        self.final_layer = _Final(hidden_size, patch_size, in_channels)
        for blk in self.blocks:  # Xavier weights / zero biases; adaLN and the output layer start at zero
            for lin in (blk.attn.qkv, blk.attn.proj, blk.mlp.w12, blk.mlp.w3):
                nn.init.xavier_uniform_(lin.weight)
                nn.init.zeros_(lin.bias)
        self._plans = PlanCache()

    def plan(self, B: int, t_shared: bool, device) -> JiTPlan:
        return self._plans.get((B, t_shared, str(device)), lambda: JiTPlan(self, B, t_shared, device), self)

    # -- input gradient --------------------------------------------------------------------------------------------
    def grad_plan(self, B: int, t_shared: bool, device) -> JiTGradPlan:
        return self._plans.get(("vjp", B, t_shared, str(device)), lambda: JiTGradPlan(self, B, t_shared, device), self)

    @torch.no_grad()
    @_lib.on_device
    def vjp(self, x: Tensor, t: Tensor, y: Tensor):
        r"""``(out, pullback)``: ``out = self(x, t, y)`` and ``pullback(v) = (d out / d x)^T v`` (like ``x``): the input gradient
        that ``azula.guidance`` takes from ``torch.autograd``, on HIP tapes (:class:`JiTGradPlan`).  ``t`` and ``y`` are constants
        of the pullback; it may be called any number of times until the next ``vjp`` with the same signature.  Scope: fp32
        parameters and fp32 device tensors; anything else raises ``NotImplementedError`` (the forward is not affected)."""
        vjp_scope(self, x, "JiT", "azula_amd.plugins.jit.JiT")
        self._check(x)
        t = t.reshape(-1)
        return self.grad_plan(x.shape[0], t.numel() == 1, x.device).run_jit(x.contiguous(), t, y)

    def _check(self, x: Tensor) -> torch.dtype:
        from ...nn.utils import backbone_io_dtype

        out_dtype = backbone_io_dtype(self, x, "azula_amd.plugins.jit.JiT")
        if tuple(x.shape[1:]) != (self.in_channels, self.input_size, self.input_size):
            raise ValueError(f"expected (B, {self.in_channels}, {self.input_size}, {self.input_size}), got {tuple(x.shape)}")
        return out_dtype

    @torch.no_grad()
    @_lib.on_device
    def forward(self, x: Tensor, t: Tensor, y: Tensor) -> Tensor:
        out_dtype = self._check(x)
        B = x.shape[0]
        t = t.reshape(-1)
        plan = self.plan(B, t.numel() == 1, x.device)
        plan.t.copy_(t.to(device=x.device, dtype=torch.float32))
        plan.labels.copy_(y.to(device=x.device, dtype=torch.int64).expand(B))
        return plan.run(x, out_dtype=out_dtype)


_ARCH = {  # name: (depth, hidden, heads, bottleneck, context start, patch)   (_src/model.py:384-457)
    "JiT-B/16": (12, 768, 12, 128, 4, 16), "JiT-B/32": (12, 768, 12, 128, 4, 32),
    "JiT-L/16": (24, 1024, 16, 128, 8, 16), "JiT-L/32": (24, 1024, 16, 128, 8, 32),
    "JiT-H/16": (32, 1280, 16, 256, 10, 16), "JiT-H/32": (32, 1280, 16, 256, 10, 32),
}


def _factory(name: str):
    depth, hidden, heads, bottleneck, start, patch = _ARCH[name]

    def make(**kwargs) -> JiT:
        return JiT(depth=depth, hidden_size=hidden, num_heads=heads, bottleneck_dim=bottleneck, in_context_len=32,
                   in_context_start=start, patch_size=patch, **kwargs)

    return make


JiT_models = {name: _factory(name) for name in _ARCH}
