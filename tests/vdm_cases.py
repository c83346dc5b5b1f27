r"""Shapes and synthetic weights of the VDM tests (tests/test_vdm_host.py, tests/test_gpu_vdm.py, tools/make_golden_vdm.py).

Weights are SYNTHESISED, never committed (imagenet_128 has 290 M parameters): element ``i`` of the tensor named ``key`` is a
counter-based integer hash of (crc32(key), i) -- exact uint64 arithmetic in numpy, the top 24 bits mapped to a uniform float in
[-1, 1) -- times a per-layer gain.  Every machine gets identical bits.

Gains.  Torch's default initialisation makes the main branch of a deep residual block nearly invisible next to its skip, which
would hide wiring errors; here the first 3x3 convolution of a block has std 0.8 sqrt(2 / fan_in) and the second
0.3 sqrt(2 / fan_in) (He scaling keeps the second moment through conv + ReLU, so the main branch comes out at about 0.3 x the
rms of the block input; tests/test_vdm_host.py asserts 0.1 .. 1), 1x1 skip projections 1 / sqrt(fan_in), the q and k rows of an
attention projection 0.25 / sqrt(c) (logits stay O(1) while the residual stream grows), v rows and out_proj 1 / sqrt(c) and
0.5 / sqrt(c), biases 0.1, GroupNorm gains 1 +- 0.1.
"""

from __future__ import annotations

import math
import zlib

import numpy as np
import torch

MODELS = ("danbooru_128", "imagenet_128", "wikiart_128", "wikiart_256", "yfcc_1", "yfcc_2")
POOLINGS = {"danbooru_128": 5, "imagenet_128": 5, "wikiart_128": 5, "wikiart_256": 6, "yfcc_1": 7, "yfcc_2": 7}
EMBED_STD = {m: (1.0 if m.startswith("yfcc") else 0.2) for m in MODELS}
SQRT3 = math.sqrt(3.0)  # a uniform on [-1, 1) has std 1 / sqrt(3)


def smallest_size(model: str) -> int:
    return 1 << POOLINGS[model]


def uniform(key: str, n: int, salt: int = 0) -> np.ndarray:
    r"""n floats in [-1, 1): splitmix64's finaliser of (crc32(key) + salt) * 2^32 + i, top 24 bits."""
    seed = np.uint64(((zlib.crc32(key.encode()) + salt) & 0xFFFFFFFF) << 32)
    z = np.arange(n, dtype=np.uint64) + seed
    with np.errstate(over="ignore"):
        z = (z + np.uint64(0x9E3779B97F4A7C15))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return ((z >> np.uint64(40)).astype(np.float64) / 8388608.0 - 1.0).astype(np.float32)


def tensor(key: str, shape, gain: float = 1.0, offset: float = 0.0, salt: int = 0) -> torch.Tensor:
    n = int(np.prod(shape)) if len(shape) else 1
    return torch.from_numpy(uniform(key, n, salt) * np.float32(gain) + np.float32(offset)).reshape(tuple(shape))


def gain_of(key: str, shape, embed_std: float = 0.2, depth: int | None = None) -> tuple[float, float]:
    r"""(gain, offset) of the uniform draw for the parameter ``key`` of a VDM backbone / block.  ``depth``: the poolings of the
    network the key belongs to; a 3x3 convolution at level l (the ``.main.`` segments in front of the block) then runs on a map
    of H = 2^(depth - l) pixels at the smallest legal input, where zero padding leaves only ((3H - 2) / H)^2 of its 9 H^2 taps on
    data (1 of 9 at H = 1): its gain is raised by the square root of that fraction's inverse, so that the innermost blocks are
    as visible as the outer ones at the size the tests run."""
    leaf = key.split(".")
    name, kind = leaf[-2] if len(leaf) > 1 else "", leaf[-1]
    if key.endswith("timestep_embed.weight"):
        return embed_std * SQRT3, 0.0
    if name == "norm":
        return (0.1, 1.0) if kind == "weight" else (0.1, 0.0)
    if kind == "bias":
        return 0.1, 0.0
    fan_in = int(np.prod(shape[1:]))
    pad = 1.0
    if depth is not None and name in ("0", "2"):
        H = 1 << max(0, depth - (key.count(".main.") - 1))
        pad = 3.0 * H / (3.0 * H - 2.0)
    if name == "skip":
        return SQRT3 / math.sqrt(fan_in), 0.0
    if name == "qkv_proj":
        return SQRT3 / math.sqrt(fan_in), 0.0  # (the q | k rows are scaled down below)
    if name == "out_proj":
        return 0.5 * SQRT3 / math.sqrt(fan_in), 0.0
    if name == "0":  # first 3x3 of a ResConvBlock
        return pad * 0.8 * SQRT3 * math.sqrt(2.0 / fan_in), 0.0
    if name == "2":
        return pad * 0.3 * SQRT3 * math.sqrt(2.0 / fan_in), 0.0
    raise KeyError(key)


def synthesise(spec, embed_std: float = 0.2, salt: int = 0, depth: int | None = None, qk: float = 0.25) -> dict[str, torch.Tensor]:
    r"""``spec``: (key, shape) pairs (a state_dict's) -> {key: fp32 tensor}.  ``qk``: the factor on the q and k rows of an
    attention projection."""
    out = {}
    for key, shape in spec:
        g, off = gain_of(key, shape, embed_std, depth)
        w = tensor(key, shape, g, off, salt)
        if key.endswith("qkv_proj.weight"):
            w[: 2 * shape[0] // 3] *= qk
        out[key] = w
    return out


def spec_of(module: torch.nn.Module) -> list:
    return [(k, tuple(v.shape)) for k, v in module.state_dict().items()]


def load_synthetic(module: torch.nn.Module, embed_std: float = 0.2, salt: int = 0) -> torch.nn.Module:
    module.load_state_dict(synthesise(spec_of(module), embed_std, salt), strict=True)
    return module


OUT_SCALE = 0.02


def synthesise_model(model: str, spec, salt: int = 0) -> dict[str, torch.Tensor]:
    r"""The weights of one of the six backbones (any base width): its embedding std, its depth.  Two more choices keep the
    network a well-conditioned function, so that an error ratio between two fp32 evaluations means something: the q and k rows
    carry 0.05 / sqrt(c) instead of 0.25 / sqrt(c) (the residual stream of these norm-free networks grows to an rms of some
    tens in the inner levels; with 0.25 the logits reach the hundreds, the softmax saturates, and near-ties between two keys
    turn one rounding into an O(1) change of the output -- measured: fp32 against fp64 1300 ulp of the output on wikiart_256),
    and the last block (second convolution, its bias and its 1x1 skip) is scaled by OUT_SCALE, so that the output is O(1) for
    an O(1) input as a trained denoiser's is, and a sampler's feedback loop does not overflow."""
    state = synthesise(spec, EMBED_STD[model], salt, POOLINGS[model], qk=0.05)
    last = max(int(k.split(".")[1]) for k, _ in spec if k.startswith("net."))
    for k in (f"net.{last}.main.2.weight", f"net.{last}.main.2.bias", f"net.{last}.skip.weight"):
        state[k] = state[k] * OUT_SCALE
    return state


def block_scales(spec, seed: int, lo: float = 1e-3, hi: float = 1e3) -> dict[str, float]:
    r"""Per ResConvBlock a factor g, log-uniform in [lo, hi]: its first convolution x g, its second x 1 / g (weights and biases
    alike, so the block computes the same function: ReLU is positively homogeneous)."""
    blocks = sorted({k[: -len(".main.0.weight")] for k, _ in spec if k.endswith(".main.0.weight") and len(_) == 4})
    out = {}
    for b in blocks:
        u = float(uniform(b, 1, salt=seed)[0])  # [-1, 1)
        g = math.exp(0.5 * (u + 1.0) * (math.log(hi) - math.log(lo)) + math.log(lo))
        out[b] = g
    return out


def rescale_blocks(state: dict, scales: dict[str, float]) -> dict:
    state = dict(state)
    for b, g in scales.items():
        state[b + ".main.0.weight"] = state[b + ".main.0.weight"] * g
        state[b + ".main.0.bias"] = state[b + ".main.0.bias"] * g
        state[b + ".main.2.weight"] = state[b + ".main.2.weight"] / g
    return state


def image(key: str, shape) -> torch.Tensor:
    r"""A test input with unit-scale entries (sum of three uniforms, std 1)."""
    return sum(tensor(f"{key}/{i}", shape) for i in range(3))


# (name, constructor arguments of azula_amd.plugins.vdm.model blocks, input shape) of the block-level goldens
BLOCK_CASES = {
    "res_19_128_5x7": ("res", dict(c_in=19, c_mid=128, c_out=128), (2, 19, 5, 7)),
    "res_19_128_6x10": ("res", dict(c_in=19, c_mid=128, c_out=128), (2, 19, 6, 10)),
    "res_128_256_skip": ("res", dict(c_in=128, c_mid=128, c_out=256), (2, 128, 6, 10)),
    "res_128_3_last": ("res", dict(c_in=128, c_mid=128, c_out=3, relu_last=False), (2, 128, 6, 10)),
    "attn_256_4x4": ("attn", dict(c_in=256, n_head=2, norm=False), (2, 256, 4, 4)),
    "attn_256_8x8": ("attn", dict(c_in=256, n_head=2, norm=False), (2, 256, 8, 8)),
    "attn_norm_128_4x4": ("attn", dict(c_in=128, n_head=2, norm=True), (2, 128, 4, 4)),
    "skip_nearest_skip_main": ("skip", dict(order="skip_main", up="nearest"), (2, 32, 8, 12)),
    "skip_bilinear_skip_main": ("skip", dict(order="skip_main", up="bilinear"), (2, 32, 8, 12)),
    "skip_nearest_main_skip": ("skip", dict(order="main_skip", up="nearest"), (2, 32, 8, 12)),
    "skip_bilinear_main_skip": ("skip", dict(order="main_skip", up="bilinear"), (2, 32, 8, 12)),
}
FULL_WIDTH = ("imagenet_128", "wikiart_256", "yfcc_1")
T_NET = 0.3


# -- helpers shared by the host and the GPU test files -------------------------------------------------------------------
def _vm():
    from azula_amd.plugins.vdm import model

    return model


def _engine():
    from azula_amd import engine

    return engine


def block_module(kind: str, args: dict) -> torch.nn.Sequential:
    r"""The plugin's module of a block case (the GPU tests run these; here they only name the parameters)."""
    if kind == "res":
        return torch.nn.Sequential(_vm().ResConvBlock(**args))
    if kind == "attn":
        return torch.nn.Sequential(_vm().SelfAttention2d(**args))
    o, sf = args["order"], args["order"] == "skip_main"

    def up():
        return torch.nn.Upsample(scale_factor=2, mode="nearest") if args["up"] == "nearest" else torch.nn.Upsample(scale_factor=2, mode="bilinear", align_corners=False)

    vm = _vm()
    R = lambda a, b, c: vm.ResConvBlock(a, b, c, skip_first=sf)  # noqa: E731
    return torch.nn.Sequential(
        R(32, 32, 32),
        _vm().SkipBlock([torch.nn.AvgPool2d(2), R(32, 64, 64), _vm().SkipBlock([torch.nn.AvgPool2d(2), R(64, 64, 64), up()], order=o), R(128, 64, 32), up()], order=o),
        R(64, 32, 32),
    )



def run_sequential(seq: torch.nn.Sequential, x: torch.Tensor) -> torch.Tensor:
    r"""A ``nn.Sequential`` of the plugin's blocks on the (B, C, H, W) device tensor ``x`` through a fresh ``VDMPlan`` (built in the
    arithmetic mode and under the kernel override in force at the call)."""
    x = x.to(torch.float32).contiguous()
    with torch.no_grad(), torch.cuda.device(x.device):
        return _vm().VDMPlan(seq, x.shape[0], x.shape[2], x.shape[3], x.shape[1], x.device)(x)


def vdm_conv_layers(model: str, base_channels: int, B: int, size: int):
    r"""The (ConvLayer, bounded source) of every convolution a VDM plan emits, derived from the module tree as VDMPlan walks
    it: no source is bounded except the output of yfcc's GroupNorm."""
    with torch.device("meta"):
        net = _vm().VDMModel(model, base_channels=base_channels)
    layers = []

    def src(C, H, W, bounded=False):
        return _engine().ConvSource(C, B * H * W * _engine().pad4(C), bounded, False, False, False)

    def conv(ks, H, W, c0, c1, cout, up0=0, bounded=False):
        layers.append(_engine().ConvLayer(ks, 1, False, B, H, W, _engine().pad4(c0), _engine().pad4(c1) if c1 else 0, cout, _engine().pad4(cout), up0, False,
                                       None, None, src(c0, H, W, bounded), src(c1, H, W) if c1 else None, True))

    def walk(mods, C, H, W):
        pend = 0
        for m in mods:
            if isinstance(m, _vm().ResConvBlock):
                c1, c2 = m.main[0], m.main[2]
                conv(3, H, W, C, pend, c1.out_channels)
                if not isinstance(m.skip, torch.nn.Identity):
                    conv(1, H, W, C, pend, c2.out_channels)
                conv(3, H, W, c1.out_channels, 0, c2.out_channels)
                C, pend = c2.out_channels, 0
            elif isinstance(m, _vm().SelfAttention2d):
                conv(1, H * W, 1, C, 0, 3 * C, bounded=hasattr(m, "norm"))
                conv(1, H * W, 1, C, 0, C)
            elif isinstance(m, _vm().SkipBlock):
                pend = walk(list(m.main)[1:-1], C, H // 2, W // 2)
        return C

    walk(net.net, 19, size, size)
    return layers



U = 2.0**-24
TIMES = (0.0064, 0.1, 0.5, 0.9, 0.9936)  # the default schedule's c_time range


def fourier_reference(t: torch.Tensor, w: torch.Tensor, mode: int):
    r"""(values, arguments f) of the reference formula in ``t``'s dtype: (B,), (nh,) -> (B, 2 nh)."""
    u = t
    if mode == 1:
        alpha, sigma = torch.cos(t * math.pi / 2), torch.sin(t * math.pi / 2)
        u = torch.log(alpha**2 / sigma**2)
    f = 2 * math.pi * u[:, None] @ w[None, :]
    return torch.cat([f.cos(), f.sin()], dim=-1), torch.cat([f, f], dim=-1)


def fourier_case(std: float, mode: int, t_stride: int, pair: int):
    w = tensor(f"fourier/w/{std}", (8,), std * SQRT3)
    t = torch.tensor([TIMES[pair], TIMES[(pair + 2) % len(TIMES)]]) if t_stride else torch.tensor([TIMES[pair]])
    return w, t


def torch_fp32_slack(t: torch.Tensor, w: torch.Tensor, mode: int) -> torch.Tensor:
    r"""What torch's fp32 evaluation needs beyond ``16 * 2^-24 * (1 + |f|)`` in mode 1: the angle ``a = t pi / 2`` carries up to two
    fp32 roundings, which move ``u = log(cos^2 a / sin^2 a)`` by ``2 a (tan a + 1 / tan a) * 2 * 2^-24`` -- 3e-5 at t = 0.9936, where
    cos a = 0.01 -- and the argument ``f`` by ``2 pi |w|`` times that.  (The kernel evaluates u in fp64 and needs none.)"""
    if mode == 0:
        return torch.zeros(t.numel(), 2 * w.numel(), dtype=torch.float64)
    a = t.double() * math.pi / 2
    du = 2 * a * (torch.tan(a) + 1 / torch.tan(a)) * 2 * U
    return (2 * math.pi * du[:, None] * w.double().abs()[None, :]).repeat(1, 2)


def check_torch_fp32(std, mode):
    r"""The premise of the kernel's bound, on the CPU: torch's own fp32 evaluation of the reference formula stays inside
    ``16 * 2^-24 * (1 + |f|)`` -- measured: at most 0.11 x the bound in mode 0 and in mode 1 up to t = 0.9, but 1.95 x at
    (mode 1, t = 0.9936), where the formula is ill conditioned; there the conditioning term of ``torch_fp32_slack`` is added."""
    for pair in range(len(TIMES)):
        w, t = fourier_case(std, mode, 1, pair)
        exact, f = fourier_reference(t.double(), w.double(), mode)
        got, _ = fourier_reference(t, w, mode)
        err = (got.double() - exact).abs()
        bound = 16 * U * (1 + f.abs())
        well = (t < 0.95)[:, None].expand_as(err) if mode == 1 else torch.ones_like(err, dtype=torch.bool)
        assert (err[well] <= bound[well]).all()  # (the bound as stated, everywhere but at the one ill-conditioned point)
        assert (err <= bound + torch_fp32_slack(t, w, mode)).all()
