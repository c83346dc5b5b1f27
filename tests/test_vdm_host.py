r"""Host-side tests of the VDM plugin (no GPU): the module trees against the reference's ``state_dict`` keys, the CPU oracle
against the reference-written goldens, the coefficients, the cards, the weight synthesiser's gains and -- on the kernel-choice
function, which is pure -- the arithmetic policy of a VDM plan."""

import itertools
import json
import os

import numpy as np
import pytest
import torch

import vdm_cases as vc
import vdm_oracle as vo
from conftest import GOLDEN
from azula_amd import engine
from azula_amd.nn.utils import skip_init
from azula_amd.plugins import vdm
from azula_amd.plugins.vdm import model as vm

torch.set_grad_enabled(False)


def npz(name: str) -> dict:
    z = np.load(os.path.join(GOLDEN, f"g26_vdm_{name}.npz"))
    return {k: torch.from_numpy(z[k]) for k in z.files}


@pytest.mark.parametrize("model", vc.MODELS)
def test_state_dict_equals_the_reference(model):
    with open(os.path.join(GOLDEN, "g26_vdm_keys.json")) as f:
        want = json.load(f)[model]
    with torch.device("meta"):
        net = vm.VDMModel(model)
    got = [[k, list(v.shape)] for k, v in net.state_dict().items()]
    assert got == want  # keys, shapes and order: a reference checkpoint loads with strict=True


@pytest.mark.parametrize("model", vc.MODELS)
def test_oracle_program_covers_the_state_dict(model):
    r"""The oracle's second statement of the architecture names exactly the reference's parameters."""
    with open(os.path.join(GOLDEN, "g26_vdm_keys.json")) as f:
        want = {k for k, _ in json.load(f)[model]}
    ops, _ = vo.program(model)
    seen = {"timestep_embed.weight"}

    def walk(ops):
        for op in ops:
            if op[0] == "res":
                seen.update(op[1] + s for s in (".main.0.weight", ".main.0.bias", ".main.2.weight", ".main.2.bias"))
            elif op[0] == "attn":
                seen.update(op[1] + s for s in (".qkv_proj.weight", ".qkv_proj.bias", ".out_proj.weight", ".out_proj.bias"))
            else:
                walk(op[2])

    walk(ops)
    optional = {k for k in want if k.endswith(".skip.weight") or ".norm." in k}
    assert seen == want - optional


@pytest.mark.parametrize("kind", ["res", "attn", "skip"])
def test_oracle_equals_the_block_goldens(kind):
    g = npz("blocks_" + kind)
    for name, (k, args, shape) in vc.BLOCK_CASES.items():
        if k != kind:
            continue
        spec = vo.skip_net_spec() if kind == "skip" else vc.spec_of(vc.block_module(kind, args))
        state = vc.synthesise(spec, salt=1)
        x = vc.image("block/" + name, shape)
        assert torch.equal(vo.block_case(kind, args, state, x), g[name + "/out32"]), name
        state64 = {k_: v.double() for k_, v in state.items()}
        # (fp64: to rounding -- the summation order of an fp64 convolution follows the thread count)
        assert float((vo.block_case(kind, args, state64, x.double()) - g[name + "/out64"]).abs().max()) < 1e-12, name


def test_skip_net_spec_names_the_plugin_modules():
    for order in ("skip_main", "main_skip"):
        got = {k: s for k, s in vc.spec_of(vc.block_module("skip", dict(order=order, up="nearest")))}
        assert got == dict(vo.skip_net_spec())


def test_coefficients_equal_the_golden():
    g = npz("denoiser")
    ts = g["coef/t"]
    assert ts.numel() == 9 and float(ts[0]) == 0.0 and float(ts[-1]) == 1.0
    den = vdm.VelocityDenoiser(torch.nn.Identity())
    assert (den.schedule.alpha_min, den.schedule.sigma_min) == (1e-2, 1e-2)
    got = vdm.velocity_coefficients(*den.schedule(ts))
    for k, v in zip(("c_in", "c_out", "c_skip", "c_time"), got):
        assert torch.equal(v, g["coef/" + k]), k
    # ... and as the fused loop forms them: one 0-d host tensor per step
    for i in range(9):
        row = den.host_coefficients(*den.schedule(ts[i]))
        for k in ("c_in", "c_out", "c_skip", "c_time"):
            assert torch.equal(row[k].reshape(()), g["coef/" + k][i]), (k, i)


def test_cards_parse_and_configure_every_model():
    cards = vdm.load_cards(vdm)
    assert sorted(cards) == ["danbooru_128x128", "imagenet_128x128", "wikiart_128x128", "wikiart_256x256", "yfcc_512x512", "yfcc_512x512_large"]
    for name, card in cards.items():
        assert card.url.startswith("https://") and card.url.endswith(card.config["model"] + ".pth") and card.hash.startswith("sha256:")
        with torch.device("meta"), skip_init():
            den = vdm.make_model(**card.config)
        assert isinstance(den, vdm.VelocityDenoiser) and den.backbone.model == card.config["model"]
    with pytest.raises(KeyError, match="cc12m"):
        vm.VDMModel("cc12m_1")


def test_half_precision_is_refused_by_name():
    net = vm.VDMModel("wikiart_128", base_channels=2)
    for cast in (net.half, net.bfloat16):
        with pytest.raises(NotImplementedError, match="plugins.vdm"):
            cast()


def test_no_vjp():
    assert not hasattr(vdm.VelocityDenoiser(torch.nn.Identity()), "_az_vjp")


@pytest.mark.parametrize("model", ["imagenet_128", "yfcc_1"])
def test_main_branch_is_visible_next_to_its_skip(model):
    r"""The synthesiser's gains: every ResConvBlock's main branch has an rms between 0.1 and 1 x that of the block's input
    (base_channels = 32, smallest legal size)."""
    net = vm.VDMModel(model, base_channels=32)
    state = vc.synthesise_model(model, vc.spec_of(net))
    n = vc.smallest_size(model)
    x, t = vc.image("net/" + model, (1, 3, n, n)), torch.tensor([vc.T_NET])
    ratios = []
    real = vo.res_block
    last = "net.%d" % max(int(k.split(".")[1]) for k in state if k.startswith("net."))

    def spy(s, p, x_, relu_last=True):
        out = real(s, p, x_, relu_last)
        skip = torch.nn.functional.conv2d(x_, s[p + ".skip.weight"]) if (p + ".skip.weight") in s else x_
        out_scale = vc.OUT_SCALE if p == last else 1.0  # (the last block is scaled as a whole: main and skip alike)
        ratios.append((p, float((out - skip).square().mean().sqrt() / x_.square().mean().sqrt()) / out_scale))
        return out

    vo.res_block = spy
    try:
        out = vo.backbone(model, state, x, t, base_channels=32)
    finally:
        vo.res_block = real
    assert torch.isfinite(out).all()
    lo, hi = min(ratios, key=lambda r: r[1]), max(ratios, key=lambda r: r[1])
    print(model, "main / input rms: min", lo, "max", hi)
    assert 0.1 <= lo[1] and hi[1] <= 1.0


@pytest.mark.parametrize("std,mode", itertools.product((0.2, 1.0), (0, 1)))
def test_fourier_bound_holds_for_torch_fp32(std, mode):
    vc.check_torch_fp32(std, mode)


@pytest.mark.parametrize("model,width,B,size", [("imagenet_128", 32, 2, 32), ("yfcc_1", 32, 2, 128), ("imagenet_128", None, 64, 128), ("yfcc_1", None, 16, 256)])
def test_no_fixed_scale_f16x2_on_an_unnormalised_tensor(model, width, B, size, monkeypatch):
    r"""Kernel choice of every convolution of a VDM plan in f16x2 mode (``engine.choose_conv`` is pure, so this needs no device):
    an f16x2 launch either measures its scale (``dyn``: ``in_absmax0`` is set) or reads the direct output of a GroupNorm; every
    other launch is a bf16x3 / fp32 entry.  The GPU suite checks the same on the tape's launch arguments."""
    monkeypatch.setattr(engine, "FP32_MFMA", "f16x2")
    layers = vc.vdm_conv_layers(model, width, B, size)
    assert len(layers) > 100
    n_h2 = 0
    for l in layers:
        ch = engine.choose_conv(l)
        if ch.h2:
            n_h2 += 1
            assert ch.dyn or l.src0.bounded, l
            assert l.src0.bounded == (model == "yfcc_1" and l.ks == 1 and l.cout == 3 * l.src0.C) or ch.dyn
    print(model, width, len(layers), "convolutions,", n_h2, "on f16x2")
    # (full width at a large batch: the measured-scale form is chosen where its absmax pass costs less than it saves -- wide layers;
    #  narrow or small layers run bf16x3)
    assert n_h2 > 0 or width is not None
