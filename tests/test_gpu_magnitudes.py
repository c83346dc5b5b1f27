r"""Networks whose hidden activations are not O(1), against the fp64 oracle, in every AZ_FP32_MFMA mode.

The synthetic weights of the other network tests keep every hidden tensor near 1, where the f16x2 kernels' fixed activation scale
(|x| < ~1e6, include/azula_amd.h) and the f16x2 attention kernel's key limit (|k| < 4094) are never in reach.  Here the same
networks run with rescaled state dicts: "wide" spreads the hidden tensors of every block over six decades (a gain g in the first
layer of a block's FFN, 1 / g in the second, so that outputs stay O(1)), the "hot" cases put one hidden tensor at ~1e6 or the keys
of an attention layer past 4094 while the scores stay what they were.  The oracle (oracle/nets.py) runs on the CPU in float64 on
the same state dict."""

import pytest
import torch

from oracle import nets, sampling, synth

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

MODES = ("native", "bf16x3", "f16x2")


def err_of(y, ref) -> float:
    return (y.double().cpu() - ref).abs().max().item()


def tape_names(module) -> list[str]:
    return [n for plan in module._plans.values() for _, _, n in plan.tape.ops]


def wide(sd: dict, firsts: list[str], seconds: list[str], seed: int) -> dict:
    r"""Per block i, a seeded log-uniform gain g in [1e-3, 1e3]: ``firsts[i]`` (weight and bias) x g, ``seconds[i]`` x 1 / g."""
    g = torch.Generator().manual_seed(seed)
    sd = dict(sd)
    for a, b in zip(firsts, seconds):
        gain = 10.0 ** (6.0 * torch.rand((), generator=g).item() - 3.0)
        sd[a + ".weight"], sd[a + ".bias"] = sd[a + ".weight"] * gain, sd[a + ".bias"] * gain
        sd[b + ".weight"] = sd[b + ".weight"] / gain
    return sd


def scaled_rows(sd: dict, key: str, rows, factor: float) -> dict:
    r"""Rows ``rows`` (a boolean mask over the output rows) of ``key``.weight / .bias multiplied by ``factor``."""
    sd = dict(sd)
    f = torch.where(rows, factor, 1.0).to(sd[key + ".weight"].dtype)
    sd[key + ".weight"] = sd[key + ".weight"] * f.reshape(-1, *[1] * (sd[key + ".weight"].ndim - 1))
    if key + ".bias" in sd:
        sd[key + ".bias"] = sd[key + ".bias"] * f
    return sd


# ---------------------------------------------------------------------------------------------------------------- models
UNET = dict(in_channels=3, out_channels=3, hid_channels=(8, 16, 32), hid_blocks=(2, 2, 2), norm="group", groups=4, mod_features=16)
VIT = dict(in_channels=4, out_channels=4, hid_channels=128, hid_blocks=2, attention_heads=2, patch_size=2, mod_features=32)
ADM = dict(image_size=32, num_channels=32, channel_mult=[1, 2, 2], num_res_blocks=1, attention_resolutions=[16, 8], num_head_channels=16,
           resblock_updown=True, use_scale_shift_norm=True, num_classes=None, discrete_schedule="linear", discrete_steps=1000)


def make_unet():
    from azula_amd.nn import UNet

    c = UNET
    return UNet(c["in_channels"], c["out_channels"], hid_channels=c["hid_channels"], hid_blocks=c["hid_blocks"], norm=c["norm"],
                groups=c["groups"], mod_features=c["mod_features"])


def make_vit(qk_norm: bool):
    from azula_amd.nn import ViT

    c = VIT
    return ViT(c["in_channels"], c["out_channels"], hid_channels=c["hid_channels"], hid_blocks=c["hid_blocks"],
               attention_heads=c["attention_heads"], patch_size=c["patch_size"], mod_features=c["mod_features"], qk_norm=qk_norm)


def make_adm():
    from azula_amd.plugins import adm

    return adm.make_model(**ADM).backbone


def qkv_rows(sd: dict, key: str, heads: int, which: str, order: str) -> torch.Tensor:
    r"""Mask of the q / k / v rows of a fused projection: order "nHC" = rows (n, head, c), "H3C" = rows (head, n, c)."""
    n = sd[key + ".weight"].shape[0]
    d = n // (3 * heads)
    idx = torch.arange(n)
    part = idx // (heads * d) if order == "nHC" else (idx // d) % 3
    return part == "qkv".index(which)


def case_state(model: str, case: str, sd: dict) -> dict:
    keys = list(sd)
    if model == "unet":
        blocks = sorted({k[: -len(".ffn.0.weight")] for k in keys if k.endswith(".ffn.0.weight")})
        if case == "wide":
            return wide(sd, [b + ".ffn.0" for b in blocks], [b + ".ffn.3" for b in blocks], seed=1)
        if case == "hot_ffn":  # one block's conv input ~1e6 (SiLU(1e6 z))
            b = blocks[len(blocks) // 2]
            return wide(sd, [b + ".ffn.0"], [b + ".ffn.3"], seed=0) | {b + ".ffn.0.weight": sd[b + ".ffn.0.weight"] * 1e6,
                                                                      b + ".ffn.0.bias": sd[b + ".ffn.0.bias"] * 1e6,
                                                                      b + ".ffn.3.weight": sd[b + ".ffn.3.weight"] * 1e-6}
    if model.startswith("vit"):
        blocks = sorted({k[: -len(".ffn.0.weight")] for k in keys if k.endswith(".ffn.0.weight")})
        if case == "wide":
            return wide(sd, [b + ".ffn.0" for b in blocks], [b + ".ffn.3" for b in blocks], seed=2)
        if case == "hot_ffn":
            b = blocks[0]
            return sd | {b + ".ffn.0.weight": sd[b + ".ffn.0.weight"] * 1e6, b + ".ffn.0.bias": sd[b + ".ffn.0.bias"] * 1e6,
                         b + ".ffn.3.weight": sd[b + ".ffn.3.weight"] * 1e-6}
        if case == "hot_k":  # keys x 3e3, queries x 1 / 3e3: the scores do not change, |k| > 4094
            for b in blocks:
                key = b + ".msa.qkv_proj"
                sd = scaled_rows(sd, key, qkv_rows(sd, key, VIT["attention_heads"], "k", "nHC"), 3e3)
                sd = scaled_rows(sd, key, qkv_rows(sd, key, VIT["attention_heads"], "q", "nHC"), 1 / 3e3)
            return sd
    if model == "adm":
        atts = sorted({k[: -len(".qkv.weight")] for k in keys if k.endswith(".qkv.weight")})
        heads = lambda a: sd[a + ".qkv.weight"].shape[0] // 3 // ADM["num_head_channels"]  # noqa: E731
        if case == "wide":
            blocks = sorted({k[: -len(".in_layers.2.weight")] for k in keys if k.endswith(".in_layers.2.weight")})
            return wide(sd, [b + ".in_layers.2" for b in blocks], [b + ".out_layers.3" for b in blocks], seed=3)
        if case == "hot_k":
            for a in atts:
                sd = scaled_rows(sd, a + ".qkv", qkv_rows(sd, a + ".qkv", heads(a), "k", "H3C"), 3e3)
                sd = scaled_rows(sd, a + ".qkv", qkv_rows(sd, a + ".qkv", heads(a), "q", "H3C"), 1 / 3e3)
            return sd
        if case == "hot_v":  # attention output ~1e6 into proj_out
            for a in atts:
                sd = scaled_rows(sd, a + ".qkv", qkv_rows(sd, a + ".qkv", heads(a), "v", "H3C"), 3e5)
                sd = sd | {a + ".proj_out.weight": sd[a + ".proj_out.weight"] / 3e5}
            return sd
    raise ValueError((model, case))


CASES = [("unet", "wide"), ("unet", "hot_ffn"), ("vit_qknorm", "wide"), ("vit_qknorm", "hot_ffn"), ("vit_plain", "hot_k"),
         ("adm", "wide"), ("adm", "hot_k"), ("adm", "hot_v")]


def run_case(model: str, case: str, monkeypatch):
    r"""{mode: (output, names on the tape)} and the fp64 oracle's output."""
    from azula_amd import engine

    monkeypatch.setattr(engine, "X3_MIN_CHANNELS", 4)  # (narrow nets: the f16x2 direct / Winograd kernels really run)
    monkeypatch.setattr(engine, "WINOGRAD", "2")
    g = torch.Generator().manual_seed(7)
    make = {"unet": make_unet, "vit_qknorm": lambda: make_vit(True), "vit_plain": lambda: make_vit(False), "adm": make_adm}[model]
    sd0 = synth.synth_state_dict(synth.shapes_of(make().state_dict()), 5)
    if model == "adm":
        nets.rerandomise_zero_tensors(sd0)
    sd = case_state(model, case, sd0)
    if model == "unet":
        x, mod = torch.randn(2, 3, 16, 16, generator=g), torch.randn(2, UNET["mod_features"], generator=g)
        fwd = lambda net: net(x.cuda(), mod.cuda())  # noqa: E731
        ref = nets.unet_forward({k: v.double() for k, v in sd.items()}, UNET, x.double(), mod.double())
    elif model.startswith("vit"):
        x, mod = torch.randn(2, 4, 8, 8, generator=g), torch.randn(2, VIT["mod_features"], generator=g)
        fwd = lambda net: net(x.cuda(), mod.cuda())  # noqa: E731
        ref = nets.vit_forward({k: v.double() for k, v in sd.items()}, dict(VIT, qk_norm=model == "vit_qknorm"), x.double(), mod.double())
    else:
        x, t = torch.randn(2, 3, 32, 32, generator=g), torch.tensor([17, 640])
        fwd = lambda net: net(x.cuda(), t.cuda())  # noqa: E731
        emb = nets.adm_timestep_embedding  # (fp32 in the reference, as on the device: the same values, carried on in fp64)
        monkeypatch.setattr(nets, "adm_timestep_embedding", lambda *a, **k: emb(*a, **k).double())
        ref = nets.adm_unet_forward({k: v.double() for k, v in sd.items()}, ADM, x.double(), t)
    outs = {}
    for mode in MODES:
        monkeypatch.setattr(engine, "FP32_MFMA", mode)
        net = make()
        net.load_state_dict(sd)
        net = net.cuda().eval()
        outs[mode] = (fwd(net).cpu(), tape_names(net))
        del net
    return outs, ref


@pytest.mark.parametrize("model, case", CASES, ids=[f"{m}-{c}" for m, c in CASES])
def test_hidden_magnitudes_match_the_fp64_oracle(model, case, monkeypatch):
    """Every mode finite and within 1e-4 max(1, scale) of the fp64 oracle; f16x2 and bf16x3 no worse than twice the native fp32
    MFMA's error (+ 1e-7 scale): where a fixed-scale split would overflow, the plan must have chosen a form that does not."""
    outs, ref = run_case(model, case, monkeypatch)
    sc = ref.abs().max().item()
    errs = {}
    for mode, (y, names) in outs.items():
        assert torch.isfinite(y).all(), (mode, "non-finite output")
        errs[mode] = err_of(y, ref)
        print(model, case, mode, "max|d| vs fp64 oracle", errs[mode], "scale", sc)
    names = outs["f16x2"][1]
    if (model, case) == ("vit_plain", "hot_k"):  # (its qkv projection's rows span 1e7: ConvWeights.h2_range keeps it on bf16x3)
        assert "az_attention_x3_f32" in names and "az_attention_f16x2_f32" not in names, names
    else:  # the f16x2 convolutions really ran
        assert any(n in ("az_conv2d_winograd_f16x2_f32", "az_conv2d_f16x2_f32") for n in names), names
    for mode in MODES:
        assert errs[mode] <= 1e-4 * max(1.0, sc), (mode, errs)
    for mode in ("f16x2", "bf16x3"):
        assert errs[mode] <= 2 * errs["native"] + 1e-7 * sc, (mode, errs)


def test_wide_unet_ddim8_fused_loop(monkeypatch):
    """DDIM-8 through the fused captured loop on the "wide" UNet (hidden tensors over six decades), every mode against the fp64
    oracle sampler on the same state dict."""
    from azula_amd import engine
    from azula_amd.denoise import KarrasDenoiser
    from azula_amd.nn import TimeModulated, UNet
    from azula_amd.noise import VPSchedule
    from azula_amd.sample import DDIMSampler

    monkeypatch.setattr(engine, "X3_MIN_CHANNELS", 4)
    monkeypatch.setattr(engine, "WINOGRAD", "2")

    def make():
        return TimeModulated(UNet(3, 3, hid_channels=UNET["hid_channels"], hid_blocks=UNET["hid_blocks"], norm="group", groups=4,
                                  mod_features=16), 16, name="unet")

    sd = synth.synth_state_dict(synth.shapes_of(make().state_dict()), 42)
    blocks = sorted({k[: -len(".ffn.0.weight")] for k in sd if k.endswith(".ffn.0.weight")})
    sd = wide(sd, [b + ".ffn.0" for b in blocks], [b + ".ffn.3" for b in blocks], seed=4)
    g = torch.Generator().manual_seed(3)
    x1 = torch.randn(2, 3, 16, 16, generator=g)
    sdd = {k: v.double() for k, v in sd.items()}
    omean = lambda a, c: sampling.karras_mean(lambda u, s: nets.time_wrapped_unet(sdd, UNET, u, s), a, c,  # noqa: E731
                                              backbone_dtype=torch.float64)
    ref = sampling.sample(omean, x1.double(), steps=8, eta=0.0)
    sc = ref.abs().max().item()
    errs = {}
    for mode in MODES:
        monkeypatch.setattr(engine, "FP32_MFMA", mode)
        net = make()
        net.load_state_dict(sd)
        den = KarrasDenoiser(net, VPSchedule()).cuda().eval()
        x0 = DDIMSampler(den, steps=8, silent=True)(x1.cuda())
        assert torch.isfinite(x0).all(), mode
        errs[mode] = err_of(x0, ref)
        print("ddim8 wide", mode, errs[mode], "scale", sc)
        assert errs[mode] <= 1e-4 * max(1.0, sc), errs
    for mode in ("f16x2", "bf16x3"):
        assert errs[mode] <= 2 * errs["native"] + 1e-7 * sc, errs


# ---------------------------------------------------------------------------------------------------------------- tape audit
def audit(tape) -> tuple[int, int]:
    r"""Every f16x2 convolution with the FIXED activation scale (in_absmax0 == 0) reads a normalisation's output (the apply pass, a
    row norm, or its own in-gather affine), and every f16x2 attention launch normalises q / k itself or reads a projection whose
    epilogue did.  Returns (fixed-scale convolutions, f16x2 attention launches) seen."""
    norm_ops = ("az_affine_act_f32", "az_affine_act_h16", "az_rownorm_mod_f32", "az_rownorm_mod_h16")
    writer: dict[int, str] = {}
    n_conv = n_att = 0
    for _, args, name in tape.ops:
        if name in norm_ops:
            writer[int(args[0])] = "norm"
        elif name.startswith("az_conv2d"):
            a = args[0]._obj
            if name in ("az_conv2d_f16x2_f32", "az_conv2d_winograd_f16x2_f32") and not a.in_absmax0:
                n_conv += 1
                srcs = [s for s in (a.src0, a.src1) if s]
                assert a.in_affine or all(writer.get(int(s)) == "norm" for s in srcs), (name, [writer.get(int(s)) for s in srcs])
            if a.dst:
                writer[int(a.dst)] = "qk" if (a.act == 5 and a.qk_rmsnorm) else "conv"
        elif name.startswith("az_attention"):
            a = args[0]._obj
            if name == "az_attention_f16x2_f32":
                n_att += 1
                assert a.qk_rmsnorm or writer.get(int(a.q)) == "qk", name
            writer[int(a.out)] = "attention"
    return n_conv, n_att


@pytest.mark.parametrize("which", ["c2", "c3", "c3_plain", "adm"])
def test_f16x2_fixed_scale_reads_only_normalisations(which, monkeypatch):
    """The default-mode plans of the C2 UNet and C3 DiT-B/2 (their bench.py widths at a reduced batch and resolution), a
    qk_norm=False DiT and an ADM UNet, audited launch by launch (see audit)."""
    from azula_amd import engine
    from azula_amd.nn import UNet, ViT

    monkeypatch.setattr(engine, "FP32_MFMA", "f16x2")
    g = torch.Generator().manual_seed(0)
    if which == "c2":
        net = UNet(3, 3, hid_channels=(256, 256, 512, 512, 1024, 1024), hid_blocks=(2, 2, 2, 2, 2, 2), norm="group", groups=32,
                   mod_features=1024).cuda().eval()
        net(torch.randn(1, 3, 64, 64, generator=g).cuda(), torch.randn(1, 1024, generator=g).cuda())
    elif which in ("c3", "c3_plain"):
        net = ViT(4, 4, hid_channels=768, hid_blocks=12, attention_heads=12, patch_size=2, mod_features=768,
                  qk_norm=which == "c3").cuda().eval()
        net(torch.randn(2, 4, 32, 32, generator=g).cuda(), torch.randn(2, 768, generator=g).cuda())
    else:
        net = make_adm().cuda().eval()
        net(torch.randn(2, 3, 32, 32, generator=g).cuda(), torch.tensor([3, 500]).cuda())
    for plan in net._plans.values():
        n_conv, n_att = audit(plan.tape)
        print(which, "fixed-scale f16x2 convolutions", n_conv, "f16x2 attention launches", n_att)
        assert n_conv > 0
        if which in ("c3_plain", "adm"):
            assert n_att == 0
