r"""CPU oracle of the VDM plugin: the six v-diffusion backbones and ``VelocityDenoiser`` as torch functional ops on a flat
``{key: tensor}`` state (fp32 or fp64: the arithmetic follows the tensors).  Written for this project's tests; it shares no code
with ``azula_amd.plugins.vdm`` -- the architectures are spelt out a second time below, as programs of

    ("res", prefix, relu_last) | ("attn", prefix, heads) | ("skip", prefix, program, order, up_mode)

over the state's key prefixes.  tools/make_golden_vdm.py asserts that it equals the reference implementation bit for bit in fp32.
"""

from __future__ import annotations

import math

import torch
import torch.nn.functional as F

# model -> (base width, widths per level as multiples of c / 2, blocks per side, first attention level, head size, norm in attention,
#           concatenation order, up-sampling, Fourier input, ReLU behind the last convolution)
TABLE = {
    "danbooru_128": (256, (2, 4, 4, 8, 8, 16), 2, 3, 128, False, "skip_main", "nearest", "log_snr", True),
    "imagenet_128": (128, (2, 4, 4, 8, 8, 16), 4, 3, 128, False, "skip_main", "nearest", "log_snr", False),
    "wikiart_128": (128, (2, 4, 4, 8, 8, 16), 4, None, 128, False, "skip_main", "nearest", "log_snr", True),
    "wikiart_256": (128, (1, 2, 4, 4, 8, 8, 16), 4, 4, 128, False, "skip_main", "nearest", "log_snr", False),
    "yfcc_1": (128, (2, 2, 4, 4, 8, 8, 16, 16), 4, 5, 64, True, "main_skip", "bilinear", "t", False),
    "yfcc_2": (256, (1, 2, 4, 4, 8, 8, 16, 16), 2, 5, 64, True, "main_skip", "bilinear", "t", False),
}


def program(model: str, base_channels: int | None = None) -> tuple[list, str]:
    r"""(program over the keys ``net.<i>...``, Fourier input) of one backbone."""
    c0, units, n, afrom, hd, _norm, order, up, embed, relu_last = TABLE[model]
    c = c0 if base_channels is None else base_channels
    w = [c * u // 2 for u in units]
    last = len(w) - 1

    def level(l: int, prefix: str, start: int) -> list:
        ops: list = []
        attn = afrom is not None and l >= afrom

        def push(kind, *rest):
            ops.append((kind, f"{prefix}{start + len(ops)}", *rest))

        def block(cout: int, relu: bool = True, with_attn: bool = True):
            push("res", relu)
            if attn and with_attn:
                push("attn", max(1, cout // hd))

        cout = 3 if l == 0 else w[l - 1]
        if l == last:
            for i in range(2 * n):
                block(w[l] if i < 2 * n - 1 else cout)
            return ops
        for _ in range(n):
            block(w[l])
        sp = f"{prefix}{start + len(ops)}"
        # (the branch: main.0 = pooling, main.1 ... = the next level, the last entry = the up-sampling)
        ops.append(("skip", sp, level(l + 1, sp + ".main.", 1), order, up))
        for i in range(n):
            out = l == 0 and i == n - 1
            block(w[l] if i < n - 1 else cout, relu=relu_last or not out, with_attn=not out)
        return ops

    return level(0, "net.", 0), embed


def res_block(s: dict, p: str, x, relu_last: bool = True):
    h = F.relu(F.conv2d(x, s[p + ".main.0.weight"], s[p + ".main.0.bias"], padding=1))
    h = F.conv2d(h, s[p + ".main.2.weight"], s[p + ".main.2.bias"], padding=1)
    if relu_last:
        h = F.relu(h)
    skip = F.conv2d(x, s[p + ".skip.weight"]) if (p + ".skip.weight") in s else x
    return h + skip


def attention(s: dict, p: str, x, heads: int):
    r"""Self-attention over the pixels: channels of the projection are (q | k | v, head, d); q and k each carry d^-1/4."""
    B, C, H, W = x.shape
    d, L = C // heads, H * W
    inp = F.group_norm(x, 1, s[p + ".norm.weight"], s[p + ".norm.bias"], 1e-5) if (p + ".norm.weight") in s else x
    proj = F.conv2d(inp, s[p + ".qkv_proj.weight"], s[p + ".qkv_proj.bias"])
    tokens = proj.reshape(B, 3 * heads, d, L).permute(0, 1, 3, 2)  # (B, 3 heads, L, d)
    q, k, v = tokens[:, :heads], tokens[:, heads : 2 * heads], tokens[:, 2 * heads :]
    quarter = d ** -0.25
    weights = torch.softmax(torch.matmul(q * quarter, k.permute(0, 1, 3, 2) * quarter), dim=-1)
    mixed = torch.matmul(weights, v).permute(0, 1, 3, 2).reshape(B, C, H, W)
    return x + F.conv2d(mixed, s[p + ".out_proj.weight"], s[p + ".out_proj.bias"])


def run(ops: list, s: dict, x):
    for op in ops:
        if op[0] == "res":
            x = res_block(s, op[1], x, op[2])
        elif op[0] == "attn":
            x = attention(s, op[1], x, op[2])
        else:
            _, _p, inner, order, up = op
            y = run(inner, s, F.avg_pool2d(x, 2))
            y = F.interpolate(y, scale_factor=2, mode="nearest") if up == "nearest" else F.interpolate(y, scale_factor=2, mode="bilinear", align_corners=False)
            x = torch.cat([x, y], dim=1) if order == "skip_main" else torch.cat([y, x], dim=1)
    return x


def fourier_input(t, embed: str):
    if embed == "t":
        return t
    alpha, sigma = torch.cos(t * math.pi / 2), torch.sin(t * math.pi / 2)
    return torch.log(alpha**2 / sigma**2)


def backbone(model: str, s: dict, x, t, base_channels: int | None = None):
    ops, embed = program(model, base_channels)
    u = fourier_input(t, embed)
    f = 2 * math.pi * u[:, None] @ s["timestep_embed.weight"].T
    planes = torch.cat([f.cos(), f.sin()], dim=-1)[..., None, None].repeat([1, 1, x.shape[2], x.shape[3]])
    return run(ops, s, torch.cat([x, planes], dim=1))


# -- the block-level cases of tests/vdm_cases.BLOCK_CASES ---------------------------------------------------------------
def skip_net_program(order: str, up: str) -> list:
    r"""res(32) | skip[pool, res(32 -> 64), skip[pool, res(64), up], res(128 -> 64 -> 32), up] | res(64 -> 32): two levels."""
    inner2 = [("res", "1.main.2.main.1", True)]
    inner1 = [("res", "1.main.1", True), ("skip", "1.main.2", inner2, order, up), ("res", "1.main.3", True)]
    return [("res", "0", True), ("skip", "1", inner1, order, up), ("res", "2", True)]


def skip_net_spec() -> list:
    def res(p, ci, cm, co):
        out = [] if ci == co else [(p + ".skip.weight", (co, ci, 1, 1))]
        return out + [(p + ".main.0.weight", (cm, ci, 3, 3)), (p + ".main.0.bias", (cm,)), (p + ".main.2.weight", (co, cm, 3, 3)), (p + ".main.2.bias", (co,))]

    return res("0", 32, 32, 32) + res("1.main.1", 32, 64, 64) + res("1.main.2.main.1", 64, 64, 64) + res("1.main.3", 128, 64, 32) + res("2", 64, 32, 32)


def block_case(kind: str, args: dict, s: dict, x):
    if kind == "res":
        return res_block(s, "0", x, args.get("relu_last", True))
    if kind == "attn":
        return attention(s, "0", x, args["n_head"])
    return run(skip_net_program(args["order"], args["up"]), s, x)


# -- the denoiser -----------------------------------------------------------------------------------------------------------
def vp_schedule(t, alpha_min: float = 1e-2, sigma_min: float = 1e-2):
    r"""azula.noise.VPSchedule: alpha = exp(log(alpha_min) t^2), sigma = sqrt(1 - alpha^2 + sigma_min^2)."""
    alpha = torch.exp(math.log(alpha_min) * t**2)
    sigma = torch.sqrt(1 - alpha**2 + sigma_min**2)
    return alpha, sigma


def coefficients(alpha, sigma):
    c_in = torch.rsqrt(alpha**2 + sigma**2)
    c_out = -sigma * torch.rsqrt(alpha**2 + sigma**2)
    c_skip = alpha * torch.rsqrt(alpha**2 + sigma**2)
    c_time = torch.atan2(sigma, alpha).flatten() / math.pi * 2
    return c_in, c_out, c_skip, c_time


def denoise(model: str, s: dict, x_t, t, base_channels: int | None = None):
    alpha, sigma = vp_schedule(t)
    while alpha.ndim < x_t.ndim:
        alpha, sigma = alpha[..., None], sigma[..., None]
    c_in, c_out, c_skip, c_time = coefficients(alpha, sigma)
    out = backbone(model, s, c_in * x_t, c_time.expand(x_t.shape[0]) if c_time.numel() == 1 else c_time, base_channels)
    return c_skip * x_t + c_out * out
