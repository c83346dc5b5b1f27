r"""The v-diffusion backbones (Katherine Crowson's v-diffusion-pytorch; reference ``azula/plugins/vdm/_src/*.py``) and their
compiled forward, :class:`VDMPlan`.

One parametrised module, :class:`VDMModel`, and one table, :data:`ARCHITECTURES`, that spells the six published networks
out.  Every network is a residual U-Net of depth ``len(widths) - 1``:

    level l:   blocks x ResConvBlock(-> widths[l])          [each followed by SelfAttention2d if l >= attention_from]
               SkipBlock(AvgPool2d(2), level l + 1, Upsample(x2))        (concatenates its input with the inner result)
               blocks x ResConvBlock, the first reading 2 widths[l] channels, the last writing widths[l - 1]
    innermost: 2 blocks x ResConvBlock, the first reading widths[l - 1], the last writing widths[l - 1]

with ``3 + 16`` input channels (image | Fourier planes of the time) and 3 output channels at level 0.  The module tree
(``timestep_embed``, ``net.<i>.main.<j>...``, ``skip``, ``qkv_proj``, ``out_proj``, ``norm``) reproduces the reference's
``state_dict`` keys, shapes and order, so a published checkpoint loads with ``strict=True``.

The four 128 / 256 px networks have NO normalisation: 3x3 conv -> ReLU -> 3x3 conv -> ReLU -> + skip.  On the engine that is
conv(act = 2), conv(act = 2, res = block input or its bias-free 1x1 projection); every activation is unbounded
(``engine.Act.bounded``), so every f16x2 launch of the plan takes a measured scale or runs bf16x3 (``engine.choose_conv``).
"""

from __future__ import annotations

import math

import torch
import torch.nn as nn
from torch import Tensor

from ... import _lib, engine
from ...engine import Act, PlanCache
from ...plan import ForwardPlan

__all__ = ["ARCHITECTURES", "VDMModel", "VDMPlan", "ResConvBlock", "SelfAttention2d", "SkipBlock", "FourierFeatures"]

# name -> base width c, widths per level in units of c / 2, ResConvBlocks per side of a level, first level with attention (None: no
# attention), channels per attention head, GroupNorm(1, c) in front of the qkv projection, concatenation order of a SkipBlock,
# up-sampling mode, what the Fourier features see ("log_snr": log(cos^2(t pi / 2) / sin^2(t pi / 2)), "t": t), their initial std,
# ReLU behind the last convolution, nominal image size
ARCHITECTURES: dict[str, dict] = {
    "danbooru_128": dict(c=256, widths=(2, 4, 4, 8, 8, 16), blocks=2, attention_from=3, head_dim=128, attn_norm=False,
                         cat="skip_main", up="nearest", embed="log_snr", std=0.2, relu_last=True, size=128),
    "imagenet_128": dict(c=128, widths=(2, 4, 4, 8, 8, 16), blocks=4, attention_from=3, head_dim=128, attn_norm=False,
                         cat="skip_main", up="nearest", embed="log_snr", std=0.2, relu_last=False, size=128),
    "wikiart_128": dict(c=128, widths=(2, 4, 4, 8, 8, 16), blocks=4, attention_from=None, head_dim=128, attn_norm=False,
                        cat="skip_main", up="nearest", embed="log_snr", std=0.2, relu_last=True, size=128),
    "wikiart_256": dict(c=128, widths=(1, 2, 4, 4, 8, 8, 16), blocks=4, attention_from=4, head_dim=128, attn_norm=False,
                        cat="skip_main", up="nearest", embed="log_snr", std=0.2, relu_last=False, size=256),
    "yfcc_1": dict(c=128, widths=(2, 2, 4, 4, 8, 8, 16, 16), blocks=4, attention_from=5, head_dim=64, attn_norm=True,
                   cat="main_skip", up="bilinear", embed="t", std=1.0, relu_last=False, size=512),
    "yfcc_2": dict(c=256, widths=(1, 2, 4, 4, 8, 8, 16, 16), blocks=2, attention_from=5, head_dim=64, attn_norm=True,
                   cat="main_skip", up="bilinear", embed="t", std=1.0, relu_last=False, size=512),
}


class ResConvBlock(nn.Module):
    r"""``main(x) + skip(x)``: conv3x3 - ReLU - conv3x3 - (ReLU | Identity), skip = Identity or a bias-free 1x1 convolution.
    ``skip_first``: the registration order of the two children (the 128 / 256 px files register ``skip`` first)."""

    def __init__(self, c_in: int, c_mid: int, c_out: int, relu_last: bool = True, skip_first: bool = True) -> None:
        super().__init__()
        skip = nn.Identity() if c_in == c_out else nn.Conv2d(c_in, c_out, 1, bias=False)
        main = nn.Sequential(nn.Conv2d(c_in, c_mid, 3, padding=1), nn.ReLU(inplace=True), nn.Conv2d(c_mid, c_out, 3, padding=1),
                             nn.ReLU(inplace=True) if relu_last else nn.Identity())
        for name, m in ((("skip", skip), ("main", main)) if skip_first else (("main", main), ("skip", skip))):
            self.add_module(name, m)
        self.relu_last = relu_last


class SelfAttention2d(nn.Module):
    r"""x + out_proj(softmax(q k^T / sqrt(d)) v) over the pixels, q | k | v = qkv_proj([norm](x)) in '(3 head d)' channel order."""

    def __init__(self, c_in: int, n_head: int = 1, norm: bool = False) -> None:
        super().__init__()
        assert c_in % n_head == 0
        if norm:
            self.norm = nn.GroupNorm(1, c_in)
        self.n_head = n_head
        self.qkv_proj = nn.Conv2d(c_in, c_in * 3, 1)
        self.out_proj = nn.Conv2d(c_in, c_in, 1)


class SkipBlock(nn.Module):
    r"""cat[x, main(x)] (``order = "skip_main"``) or cat[main(x), x] (``"main_skip"``) along the channels."""

    def __init__(self, main: list, order: str = "skip_main") -> None:
        super().__init__()
        assert order in ("skip_main", "main_skip")
        self.main = nn.Sequential(*main)
        self.skip = nn.Identity()
        self.order = order


class FourierFeatures(nn.Module):
    r"""Holds the ``out_features / 2`` random frequencies (one row per frequency) of the time embedding; the plan evaluates
    cos | sin of ``2 pi u w`` on the device (``az_fourier_planes_f32``)."""

    def __init__(self, in_features: int, out_features: int, std: float = 1.0) -> None:
        super().__init__()
        if out_features % 2:
            raise ValueError(f"FourierFeatures: an even number of features (cos | sin halves), got {out_features}")
        self.weight = nn.Parameter(std * torch.randn(out_features // 2, in_features))


def _level_modules(a: dict, c: int) -> nn.Sequential:
    w = [c * u // 2 for u in a["widths"]]
    n, last = a["blocks"], len(w) - 1
    sf = a["cat"] == "skip_main"  # (the files that concatenate skip first also register ResidualBlock.skip first)

    def attn(level: int, width: int) -> list:
        if a["attention_from"] is None or level < a["attention_from"]:
            return []
        heads = max(1, width // a["head_dim"])  # (narrow test networks: one head where the width is below the head size)
        if width % heads or width // heads not in engine.ATTN_HEAD_DIMS:
            raise ValueError(f"vdm: attention width {width} does not split into heads of {a['head_dim']} channels (base_channels = {c})")
        return [SelfAttention2d(width, heads, norm=a["attn_norm"])]

    def level(l: int) -> list:
        cin = 3 + 16 if l == 0 else w[l - 1]
        cout = 3 if l == 0 else w[l - 1]
        mods: list = []
        if l == last:
            for i in range(2 * n):
                co = w[l] if i < 2 * n - 1 else cout
                mods += [ResConvBlock(cin if i == 0 else w[l], w[l], co, skip_first=sf), *attn(l, co)]
            return mods
        for i in range(n):
            mods += [ResConvBlock(cin if i == 0 else w[l], w[l], w[l], skip_first=sf), *attn(l, w[l])]
        up = nn.Upsample(scale_factor=2, mode="nearest") if a["up"] == "nearest" else nn.Upsample(scale_factor=2, mode="bilinear", align_corners=False)
        mods.append(SkipBlock([nn.AvgPool2d(2), *level(l + 1), up], order=a["cat"]))
        for i in range(n):
            is_out = l == 0 and i == n - 1
            co = w[l] if i < n - 1 else cout
            mods += [ResConvBlock(2 * w[l] if i == 0 else w[l], w[l], co, relu_last=a["relu_last"] or not is_out, skip_first=sf)]
            if not is_out:
                mods += attn(l, co)
        return mods

    return nn.Sequential(*level(0))


# Kernel tests only: {kernel size: a ``Builder.conv(winograd=...)`` override} applied to every convolution of a plan whose source
# strides are multiples of 16 channels (the f16x2 kernels' K step) -- {3: "wh2d", 1: "h2d"} pushes a whole network through the
# measured-scale f16x2 kernels at shapes where ``engine.choose_conv`` would not pick them.  None: the engine's policy.
CONV_OVERRIDE: dict | None = None


class VDMPlan(ForwardPlan):
    r"""Compiled forward of a ``nn.Sequential`` of ResConvBlock / SelfAttention2d / SkipBlock / AvgPool2d / Upsample modules for
    one (batch, H, W).  ``embed = (weight, mode)``: the input carries 3 image channels and the Fourier planes of the time in
    channels 3 .. 3 + 2 len(weight), written each run by ``az_fourier_planes_f32`` from ``t_ptr`` (stride ``t_stride``)."""

    def __init__(self, seq: nn.Sequential, B: int, H: int, W: int, cin: int, device, *, embed: tuple | None = None,
                 coef_ptr: int | None = None) -> None:
        super().__init__(device)
        bld = self.bld
        cs = self.nhwc_input(B, H, W, cin).cs
        self.t = torch.zeros(B, dtype=torch.float32, device=device)
        if embed is not None:
            weight, mode = embed
            wdev = bld.const(weight.detach().reshape(-1))
            nh = wdev.numel()
            assert cin == 3 + 2 * nh
            t_ptr, t_stride = (self.t.data_ptr(), 1) if coef_ptr is None else (coef_ptr + 4 * _lib.COEF_FIELDS.index("c_time"), 0)
            # (constant planes are NOT a bias of the stem: with zero padding the border taps see zeros where the planes end)
            bld.tape.add("az_fourier_planes_f32", self.x_in.ptr, B, H * W, cs, 3, wdev.data_ptr(), nh, t_ptr, t_stride, mode, keep=[self.t])
        bld.wrote(self.x_in, bounded=False)

        def pack(conv: nn.Conv2d, cin0: int | None = None):
            return bld.pack_conv(conv.weight, conv.bias, cin0=cin0)

        def how(conv: nn.Conv2d, *srcs: Act | None, up0: int = 0) -> dict:
            w = (CONV_OVERRIDE or {}).get(conv.kernel_size[0])
            if w is None or any(s_ is not None and s_.cs % 16 for s_ in srcs):
                return {}
            if conv.kernel_size[0] == 3 and min(srcs[0].H << up0, srcs[0].W << up0) < 4:
                return {}  # (maps below two Winograd tiles per axis stay with the engine's choice, the direct kernel)
            return {"winograd": w}

        def resblock(rb: ResConvBlock, x0: Act, x1: Act | None, up0: int, up1: int) -> Act:
            c1, c2 = rb.main[0], rb.main[2]
            cin0 = x0.C if x1 is not None else None
            h = bld.conv(x0, pack(c1, cin0), c1.out_channels, src1=x1, up0=up0, up1=up1, act=2, **how(c1, x0, x1, up0=up0))
            if isinstance(rb.skip, nn.Identity):
                assert x1 is None and up0 == 0
                res = x0
            else:
                res = bld.conv(x0, pack(rb.skip, cin0), c2.out_channels, src1=x1, up0=up0, up1=up1, **how(rb.skip, x0, x1))
            out = bld.conv(h, pack(c2), c2.out_channels, act=2 if rb.relu_last else 0, res=res, **how(c2, h))
            bld.free(h)
            if res is not x0:
                bld.free(res)
            return out

        def attention(ab: SelfAttention2d, x: Act) -> Act:
            Cc, heads = x.C, ab.n_head
            d = Cc // heads
            assert x.cs == Cc and d in engine.ATTN_HEAD_DIMS, "vdm attention: head sizes 64 / 128 on unpadded channels"
            src = x
            if hasattr(ab, "norm"):  # (the one bounded tensor of a VDM plan: its consumer may take the fixed f16x2 scale)
                src = bld.group_norm(x, 1, weight=bld.const(ab.norm.weight), bias=bld.const(ab.norm.bias), eps=ab.norm.eps)
            tok = src.view(x.B, x.H * x.W, 1, Cc)
            qkv = bld.conv(tok, pack(ab.qkv_proj), 3 * Cc, **({} if src is not x else how(ab.qkv_proj, tok)))
            if src is not x:
                bld.free(src)
            # the reference scales q and k by d^-1/4 each; un-normalised q / k: choose_attention never takes the f16x2 kernel
            att = bld.attention(qkv, heads, "3HC", False, 1.0 / math.sqrt(d))
            bld.free(qkv)
            o = bld.conv(att, pack(ab.out_proj), Cc, res=x.view(x.B, x.H * x.W, 1, Cc), **how(ab.out_proj, att))
            bld.free(att)
            return o.view(x.B, x.H, x.W, pinned=False)

        def run(mods, h: Act, owned: bool) -> tuple[Act, str | None]:
            r"""-> (result, pending up-sampling).  ``owned``: ``h`` may be released once consumed."""
            pend: tuple | None = None  # a SkipBlock's concatenation waiting for its consumer: (src0, src1, up0, up1, to free)
            up: str | None = None
            for m in mods:
                assert up is None, "vdm: an Upsample must end a SkipBlock's main branch"
                if isinstance(m, ResConvBlock):
                    if pend is not None:
                        nh = resblock(m, *pend[:4])
                        for a in pend[4]:
                            bld.free(a)
                        pend = None
                    else:
                        nh = resblock(m, h, None, 0, 0)
                        if owned:
                            bld.free(h)
                elif pend is not None:
                    raise NotImplementedError("vdm: a SkipBlock must be followed by a ResConvBlock (its concatenation is read in place)")
                elif isinstance(m, SelfAttention2d):
                    nh = attention(m, h)
                    if owned:
                        bld.free(h)
                elif isinstance(m, nn.AvgPool2d):
                    nh = bld.avgpool(h, 1)
                    if owned:
                        bld.free(h)
                elif isinstance(m, nn.Upsample):
                    up, nh = m.mode, h
                elif isinstance(m, SkipBlock):
                    inner, iup = run(m.main, h, False)
                    lift = 0
                    if iup == "bilinear":  # materialised; nearest x2 is read through the consumer's gather (up = 1)
                        wide = bld.new_act(inner.B, 2 * inner.H, 2 * inner.W, inner.C)
                        bld.tape.add("az_upsample_bilinear2x_f32", wide.ptr, inner.ptr, inner.B, inner.H, inner.W, inner.cs)
                        bld.wrote(wide, bounded=False)
                        bld.free(inner)
                        inner = wide
                    elif iup == "nearest":
                        lift = 1
                    assert (inner.H << lift, inner.W << lift) == (h.H, h.W), "vdm: a SkipBlock's branch must return to its input size"
                    free = [inner] + ([h] if owned else [])
                    pend = (h, inner, 0, lift, free) if m.order == "skip_main" else (inner, h, lift, 0, free)
                    nh = h
                else:
                    raise NotImplementedError(f"vdm: no kernel plan for {type(m).__name__}")
                h, owned = nh, True
            if pend is not None:
                raise NotImplementedError("vdm: a SkipBlock must be followed by a ResConvBlock (its concatenation is read in place)")
            return h, up

        y, up = run(seq, self.x_in, False)
        assert up is None
        self.out = torch.empty(B, y.C, y.H, y.W, dtype=torch.float32, device=device)
        bld.tape.add("az_nhwc_to_nchw_f32", self.out.data_ptr(), y.ptr, B, y.C, y.H * y.W, y.cs, keep=[y.buf])
        self.end()

    def __call__(self, x: Tensor, t: Tensor | None = None) -> Tensor:
        if t is not None:
            self.t.copy_(t.to(torch.float32).reshape(-1).expand(x.shape[0]))
        return self.run(x)


class VDMModel(nn.Module):
    r"""One of the six v-diffusion backbones (``model``: a key of :data:`ARCHITECTURES`).  ``base_channels`` (default: the
    model's own 128 / 256) is this project's one extension, for narrow test networks.  ``forward(x, t)``: x (B, 3, H, W) with
    H = W a multiple of ``2 ** depth``, t (B,) or a scalar in [0, 1]."""

    def __init__(self, model: str = "imagenet_128", base_channels: int | None = None) -> None:
        super().__init__()
        if model not in ARCHITECTURES:
            hint = " (cc12m_1 needs CLIP embeddings and is out of this plugin's scope)" if model.startswith("cc12m") else ""
            raise KeyError(f"vdm: unknown model {model!r}{hint}; one of {sorted(ARCHITECTURES)}")
        a = self.arch = ARCHITECTURES[model]
        c = a["c"] if base_channels is None else int(base_channels)
        if c < 2 or c % 2:
            raise ValueError(f"vdm: base_channels must be even, got {c}")
        self.model, self.base_channels = model, c
        self.shape = (3, a["size"], a["size"])
        self.depth = len(a["widths"]) - 1
        self.out_channels = 3
        self.timestep_embed = FourierFeatures(1, 16, std=a["std"])
        self.net = _level_modules(a, c)
        self._plans = PlanCache()

    # -- half precision: out of scope ---------------------------------------------------------------------------------
    def half(self):
        raise NotImplementedError("azula_amd.plugins.vdm: half-precision VDM backbones are not implemented (fp32 parameters only)")

    def bfloat16(self):
        raise NotImplementedError("azula_amd.plugins.vdm: half-precision VDM backbones are not implemented (fp32 parameters only)")

    def plan(self, B: int, H: int, W: int, device, coef_ptr: int | None = None) -> VDMPlan:
        if H % (1 << self.depth) or W % (1 << self.depth):
            raise ValueError(f"vdm {self.model}: H and W must be multiples of {1 << self.depth} ({self.depth} poolings), got {H} x {W}")
        if next(self.parameters()).dtype != torch.float32:
            raise NotImplementedError("azula_amd.plugins.vdm: half-precision VDM backbones are not implemented (fp32 parameters only)")
        mode = 1 if self.arch["embed"] == "log_snr" else 0
        return self._plans.get(
            (B, H, W, str(device), coef_ptr),
            lambda: VDMPlan(self.net, B, H, W, 3 + 16, device, embed=(self.timestep_embed.weight, mode), coef_ptr=coef_ptr),
            self, extra=tuple(sorted(CONV_OVERRIDE.items())) if CONV_OVERRIDE else (),
        )

    @torch.no_grad()
    @_lib.on_device
    def forward(self, x: Tensor, t: Tensor) -> Tensor:
        from ...nn.utils import backbone_io_dtype

        backbone_io_dtype(self, x, "azula_amd VDM backbone")
        if x.ndim != 4 or x.shape[1] != 3:
            raise ValueError(f"vdm {self.model}: expected a (B, 3, H, W) input, got {tuple(x.shape)}")
        B, _, H, W = x.shape
        t = torch.as_tensor(t, device=x.device).reshape(-1)
        assert t.numel() in (1, B), "t: a scalar or one time per sample"
        return self.plan(B, H, W, x.device)(x, t)
