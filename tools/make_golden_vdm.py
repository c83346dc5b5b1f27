r"""Writes the VDM fixtures ``tests/golden/g26_vdm_*`` from the REFERENCE implementation (``azula.plugins.vdm``).

    python tools/make_golden_vdm.py /path/to/reference [--only keys|blocks|nets|denoiser]

Runs on a machine that has the reference checkout; the tests never need it.  The reference's ``hub.py`` imports ``gdown`` and the
plugin's ``utils.py`` imports ``torchvision`` (and ``requests``); neither is used on this path, so empty stand-in modules are
registered first.  Weights are synthesised (tests/vdm_cases.py) and loaded into the reference modules; for every case the script
asserts that tests/vdm_oracle.py equals the reference BIT FOR BIT in fp32, then stores the inputs, the reference's fp32 output and
the output of the same modules run in fp64.  No weights are stored.
"""

from __future__ import annotations

import importlib
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF = next((a for a in sys.argv[1:] if not a.startswith("--")), None)
if REF is None:
    raise SystemExit(__doc__)
sys.path.insert(0, REF)
for name in ("gdown", "requests", "torchvision", "torchvision.transforms", "torchvision.transforms.functional"):
    try:
        importlib.import_module(name)
    except ImportError:
        sys.modules[name] = types.ModuleType(name)
sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
sys.modules["torchvision.transforms"].functional = sys.modules["torchvision.transforms.functional"]

import vdm_cases as vc  # noqa: E402
import vdm_oracle as vo  # noqa: E402
from azula.nn.utils import skip_init  # noqa: E402  (the reference)
from azula.plugins import vdm as ref_vdm  # noqa: E402
from azula.plugins.vdm._src import get_model, imagenet_128 as ref_in, yfcc_1 as ref_yf  # noqa: E402
from azula.sample import DDIMSampler, DDPMSampler  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
ONLY = next((sys.argv[i + 1] for i, a in enumerate(sys.argv[:-1]) if a == "--only"), None)
torch.set_grad_enabled(False)
torch.set_num_threads(8)


def same(a: torch.Tensor, b: torch.Tensor, what: str) -> None:
    assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), f"{what}: vdm_oracle differs from the reference"


def save(name: str, **arrays) -> None:
    path = os.path.join(GOLD, f"g26_vdm_{name}.npz")
    np.savez(path, **{k: (v.numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in arrays.items()})
    print(f"{path}: {os.path.getsize(path) / 1024:.0f} KiB", flush=True)


def double(state: dict) -> dict:
    return {k: v.double() for k, v in state.items()}


def ref_model(model: str) -> torch.nn.Module:
    with skip_init():
        return get_model(model)().eval()


def keys() -> None:
    out = {}
    for m in vc.MODELS:
        net = ref_model(m)  # (uninitialised storage: the constructors call .item(), which a meta device refuses)
        out[m] = [[k, list(v.shape)] for k, v in net.state_dict().items()]
        del net
    with open(os.path.join(GOLD, "g26_vdm_keys.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))


def ref_block(kind: str, args: dict) -> torch.nn.Module:
    if kind == "res":
        return torch.nn.Sequential(ref_in.ResConvBlock(args["c_in"], args["c_mid"], args["c_out"], is_last=not args.get("relu_last", True)))
    if kind == "attn":
        mod = ref_yf if args["norm"] else ref_in
        return torch.nn.Sequential(mod.SelfAttention2d(args["c_in"], args["n_head"]))
    mod = ref_in if args["order"] == "skip_main" else ref_yf
    R, S = mod.ResConvBlock, mod.SkipBlock

    def up():
        return torch.nn.Upsample(scale_factor=2, mode="nearest") if args["up"] == "nearest" else torch.nn.Upsample(scale_factor=2, mode="bilinear", align_corners=False)

    return torch.nn.Sequential(
        R(32, 32, 32),
        S([torch.nn.AvgPool2d(2), R(32, 64, 64), S([torch.nn.AvgPool2d(2), R(64, 64, 64), up()]), R(128, 64, 32), up()]),
        R(64, 32, 32),
    )


def blocks() -> None:
    arrays = {}
    for name, (kind, args, shape) in vc.BLOCK_CASES.items():
        net = ref_block(kind, args).eval()
        state = vc.synthesise(vc.spec_of(net), salt=1)
        net.load_state_dict(state, strict=True)
        x = vc.image("block/" + name, shape)
        out32 = net(x)
        same(vo.block_case(kind, args, state, x), out32, name)
        out64 = net.double()(x.double())
        same(vo.block_case(kind, args, double(state), x.double()), out64, name + " (fp64)")
        arrays[name + "/x"], arrays[name + "/out32"], arrays[name + "/out64"] = x, out32, out64
        print(name, "fp32 vs fp64", float((out32.double() - out64).abs().max()), "max |out|", float(out64.abs().max()), flush=True)
    for kind in ("res", "attn", "skip"):  # (one file per kind: each stays well under the size limit of a committed file)
        save("blocks_" + kind, **{k: v for k, v in arrays.items() if vc.BLOCK_CASES[k.split("/")[0]][0] == kind})


def nets() -> None:
    for m in ("imagenet_128", "wikiart_256", "yfcc_1", "danbooru_128", "wikiart_128"):
        net = ref_model(m)
        state = vc.synthesise_model(m, vc.spec_of(net))
        net.load_state_dict(state, strict=True)
        n = vc.smallest_size(m)
        x, t = vc.image("net/" + m, (1, 3, n, n)), torch.tensor([vc.T_NET])
        out32 = net(x, t)
        same(vo.backbone(m, state, x, t), out32, m)
        print(m, "oracle == reference at full width", flush=True)
        if m in vc.FULL_WIDTH:
            out64 = net.double()(x.double(), t.double())
            print(m, "fp32 vs fp64", float((out32.double() - out64).abs().max()), "max |out|", float(out64.abs().max()), flush=True)
            save("net_" + m, x=x, t=t, out32=out32, out64=out64)
        del net, state


def per_sample(sampler, x1: torch.Tensor, noises: list) -> torch.Tensor:
    r"""The reference sampler on each sample of the batch on its own, the step's ``randn_like`` answered from ``noises``.  (The
    reference hands the backbone ONE time for the whole batch, and its ``expand_to_planes`` then builds planes of batch 1: its
    samplers run these models at batch 1 only.)"""
    real, out = torch.randn_like, []
    for b in range(x1.shape[0]):
        it = iter(noises)
        torch.randn_like = lambda like, **kw: next(it)[b : b + 1].to(like)
        try:
            out.append(sampler(x1[b : b + 1]))
        finally:
            torch.randn_like = real
    return torch.cat(out)


def denoiser() -> None:
    net = ref_model("imagenet_128")
    state = vc.synthesise_model("imagenet_128", vc.spec_of(net))
    net.load_state_dict(state, strict=True)
    den = ref_vdm.VelocityDenoiser(net).eval()
    arrays = {}
    # the coefficients at 9 times across [0, 1], both ends included
    ts = torch.linspace(0, 1, 9)
    alpha, sigma = den.schedule(ts)
    c_in, c_out, c_skip = torch.rsqrt(alpha**2 + sigma**2), -sigma * torch.rsqrt(alpha**2 + sigma**2), alpha * torch.rsqrt(alpha**2 + sigma**2)
    c_time = torch.atan2(sigma, alpha).flatten() / torch.pi * 2
    for k, v, o in zip(("c_in", "c_out", "c_skip", "c_time"), (c_in, c_out, c_skip, c_time), vo.coefficients(*vo.vp_schedule(ts))):
        same(o, v, k)
        arrays["coef/" + k] = v
    arrays["coef/t"] = ts
    # forward with one time per sample
    x_t, t = vc.image("denoiser/x_t", (2, 3, 32, 32)), torch.tensor([0.2, 0.7])
    mean32 = den(x_t, t).mean
    same(vo.denoise("imagenet_128", state, x_t, t), mean32, "VelocityDenoiser.forward")
    # the samplers: a stored start, stored noises (one randn_like per step, drawn even where it is not read)
    x1 = vc.image("sampler/x1", (2, 3, 32, 32))
    noises = [vc.image(f"sampler/eps{i}", (2, 3, 32, 32)) for i in range(4)]
    for key, make in (("ddim4", lambda d: DDIMSampler(d, steps=4, silent=True)), ("ddpm4", lambda d: DDPMSampler(d, steps=4, silent=True))):
        arrays["sampler/" + key] = per_sample(make(den), x1, noises)
    net64 = net.double()
    den64 = ref_vdm.VelocityDenoiser(net64).eval()
    arrays["forward/x_t"], arrays["forward/t"], arrays["sampler/x1"], arrays["sampler/eps"] = x_t, t, x1, torch.stack(noises)
    arrays["forward/mean32"], arrays["forward/mean64"] = mean32, den64(x_t.double(), t.double()).mean
    for key, make in (("ddim4", lambda d: DDIMSampler(d, steps=4, silent=True, dtype=torch.float64)), ("ddpm4", lambda d: DDPMSampler(d, steps=4, silent=True, dtype=torch.float64))):
        arrays["sampler/" + key + "_64"] = per_sample(make(den64), x1.double(), noises)
    save("denoiser", **arrays)


if __name__ == "__main__":
    for fn in (keys, blocks, nets, denoiser):
        if ONLY in (None, fn.__name__):
            fn()
