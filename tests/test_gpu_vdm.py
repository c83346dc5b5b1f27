r"""The VDM plugin on the GPU: blocks, whole backbones, the denoiser and the fused samplers.

Error rule, used throughout: with ``e_gpu = max |gpu - out_f64|`` and ``e_ref = max |out_f32 - out_f64|`` (the fp32 CPU
evaluation against the same modules in fp64, both written by the reference into the goldens or, for the narrow networks,
computed by tests/vdm_oracle.py), require ``e_gpu <= 4 e_ref``: the margin covers a different accumulation order and the
Winograd transform (tests/test_gpu_kernels.py measures that form within ~1.5 x of the direct fp32 kernel against fp64; two such
layers per block compound).  Every figure is printed before it is asserted.

The network tests run in the three ``AZ_FP32_MFMA`` modes (``engine.FP32_MFMA`` is read per plan, so it is switched per test).
"""

import os

import numpy as np
import pytest
import torch

import vdm_cases as vc
import vdm_oracle as vo
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
MODES = ("f16x2", "bf16x3", "native")
MARGIN = 4.0


def npz(name: str) -> dict:
    z = np.load(os.path.join(GOLDEN, f"g26_vdm_{name}.npz"))
    return {k: torch.from_numpy(z[k]) for k in z.files}


def check(what: str, got: torch.Tensor, out32: torch.Tensor, out64: torch.Tensor) -> None:
    got = got.detach().cpu().double()
    assert got.shape == out64.shape and torch.isfinite(got).all(), what
    e_gpu, e_ref = float((got - out64).abs().max()), float((out32.double() - out64).abs().max())
    print(f"{what}: e_gpu {e_gpu:.3e} e_ref {e_ref:.3e} ratio {e_gpu / e_ref:.2f} max |out| {float(out64.abs().max()):.3g}")
    assert e_gpu <= MARGIN * e_ref, what


def set_mode(monkeypatch, mode: str) -> None:
    from azula_amd import engine

    monkeypatch.setattr(engine, "FP32_MFMA", mode)


# ------------------------------------------------------------------------------------------------------------ blocks
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(vc.BLOCK_CASES))
def test_block(name, mode, monkeypatch):
    set_mode(monkeypatch, mode)
    kind, args, shape = vc.BLOCK_CASES[name]
    g = npz("blocks_" + kind)
    assert torch.equal(g[name + "/x"], vc.image("block/" + name, shape))  # (the stored input is the synthesiser's)
    seq = vc.load_synthetic(vc.block_module(kind, args), salt=1).cuda()
    got = vc.run_sequential(seq, g[name + "/x"].cuda())
    check(f"{name} [{mode}]", got, g[name + "/out32"], g[name + "/out64"])


# ------------------------------------------------------------------------------------------------ whole backbones
@pytest.fixture(scope="module")
def full_width():
    r"""The full-width backbones with their synthesised weights, made once per module (synthesis and packing dominate)."""
    cache = {}

    def get(model: str):
        from azula_amd.nn.utils import skip_init
        from azula_amd.plugins.vdm.model import VDMModel

        if model not in cache:
            cache.clear()  # (one at a time: imagenet_128 alone packs 290 M parameters)
            with skip_init():
                net = VDMModel(model)
            net.load_state_dict(vc.synthesise_model(model, vc.spec_of(net)), strict=True)
            cache[model] = net.cuda().eval()
        return cache[model]

    yield get
    cache.clear()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("model", vc.FULL_WIDTH)
def test_backbone_full_width(model, mode, full_width, monkeypatch):
    set_mode(monkeypatch, mode)
    g = npz("net_" + model)
    n = vc.smallest_size(model)
    net = full_width(model)
    assert tuple(g["x"].shape) == (1, 3, n, n) and float(g["t"]) == pytest.approx(vc.T_NET)
    got = net(g["x"].cuda(), g["t"].cuda())
    check(f"{model} {n}x{n} [{mode}]", got, g["out32"], g["out64"])
    net._plans.clear()


def narrow(model: str, state: dict | None = None):
    from azula_amd.plugins.vdm.model import VDMModel

    net = VDMModel(model, base_channels=32)
    state = vc.synthesise_model(model, vc.spec_of(net)) if state is None else state
    net.load_state_dict(state, strict=True)
    return net.cuda().eval(), state


@pytest.fixture(scope="module")
def narrow_reference():
    r"""(state, x, t, fp32 oracle output, fp64 oracle output) of the six narrow networks, computed once."""
    cache = {}

    def get(model: str):
        if model not in cache:
            from azula_amd.plugins.vdm.model import VDMModel

            with torch.device("meta"):
                spec = vc.spec_of(VDMModel(model, base_channels=32))
            state = vc.synthesise_model(model, spec)
            n = vc.smallest_size(model)
            x, t = vc.image("net/" + model, (2, 3, n, n)), torch.tensor([vc.T_NET, 0.8])
            out32 = vo.backbone(model, state, x, t, 32)
            out64 = vo.backbone(model, {k: v.double() for k, v in state.items()}, x.double(), t.double(), 32)
            cache[model] = (state, x, t, out32, out64)
        return cache[model]

    return get


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("model", vc.MODELS)
def test_backbone_narrow(model, mode, narrow_reference, monkeypatch):
    set_mode(monkeypatch, mode)
    state, x, t, out32, out64 = narrow_reference(model)
    net, _ = narrow(model, state)
    check(f"{model} c = 32 [{mode}]", net(x.cuda(), t.cuda()), out32, out64)


@pytest.mark.parametrize("mode", MODES)
def test_hidden_activations_away_from_one(mode, narrow_reference, monkeypatch):
    r"""imagenet_128 at c = 32 with the first convolution of every block x g and the second x 1 / g, g log-uniform in
    [1e-3, 1e3] per block: the same function (ReLU is positively homogeneous) through hidden tensors of 1e-3 .. 1e3."""
    set_mode(monkeypatch, mode)
    state, x, t, _, _ = narrow_reference("imagenet_128")
    scales = vc.block_scales([(k, tuple(v.shape)) for k, v in state.items()], seed=7)
    assert min(scales.values()) < 1e-2 and max(scales.values()) > 1e2
    state = vc.rescale_blocks(state, scales)
    out32 = vo.backbone("imagenet_128", state, x, t, 32)
    out64 = vo.backbone("imagenet_128", {k: v.double() for k, v in state.items()}, x.double(), t.double(), 32)
    net, _ = narrow("imagenet_128", state)
    check(f"imagenet_128 c = 32 rescaled [{mode}]", net(x.cuda(), t.cuda()), out32, out64)


def read_tape(plan):
    r"""(launch names, f16x2 convolution descriptors with the flag "its source 0 is the GroupNorm apply pass right before it")."""
    from azula_amd.engine import H2_NAMES

    names, h2, last_norm_dst = [op[2] for op in plan.tape.ops], [], None
    for _fn, args, name in plan.tape.ops:
        if name == "az_affine_act_f32":
            last_norm_dst = args[0]
        if name in H2_NAMES:
            a = args[0]._obj  # (the AzConvArgs behind the recorded byref)
            h2.append((a, a.src0 == last_norm_dst))
    return names, h2


@pytest.mark.parametrize("model", ["imagenet_128", "yfcc_1"])
def test_tape_has_no_fixed_scale_f16x2_on_an_unnormalised_tensor(model, monkeypatch):
    r"""The launch arguments of the recorded tape in f16x2 mode, under the engine's own policy: every f16x2 convolution carries
    ``in_absmax0`` (a measured scale) unless its source is the output of the GroupNorm apply pass right before it; no f16x2
    attention entry at all.  At this width the policy gives the norm-free network no f16x2 launch (the absmax pass would cost more
    than it saves): the measured-scale launches are exercised by the ``measured_scale`` tests below.  The convolution entries of
    the tape are also those that tests/vdm_cases.vdm_conv_layers predicts, which ties the host policy test to the real plan."""
    from azula_amd import engine

    set_mode(monkeypatch, "f16x2")
    net, _ = narrow(model)
    n = vc.smallest_size(model)
    plan = net.plan(2, n, n, torch.device("cuda", torch.cuda.current_device()))
    names, h2 = read_tape(plan)
    assert "az_attention_f16x2_f32" not in names and "az_fourier_planes_f32" == names[0]
    fixed = [a for a, after_norm in h2 if not a.in_absmax0]
    for a, after_norm in h2:
        assert a.in_absmax0 or (model == "yfcc_1" and after_norm), "a fixed-scale f16x2 launch on an un-normalised tensor"
    print(model, len(names), "launches,", len(h2), "f16x2 convolutions,", len(fixed), "on the fixed scale")
    assert (len(fixed) > 0) == (model == "yfcc_1")
    predicted = [engine.choose_conv(l).name for l in vc.vdm_conv_layers(model, 32, 2, n)]
    assert [nm for nm in names if nm.startswith("az_conv2d")] == predicted


# ---------------------------------------------------------------------------- the measured-scale f16x2 kernels on whole networks
# At the test shapes engine.choose_conv never finds the absmax pass worth its cost (it does from the 256-channel levels on at
# batch 64), so these tests route every convolution whose sources have 16-channel strides through the measured-scale f16x2
# kernels (model.CONV_OVERRIDE: Winograd form for 3 x 3, direct form for 1 x 1) and hold the result to the same 4 x e_ref rule.
H2D = {3: "wh2d", 1: "h2d"}


def measured_scale(monkeypatch) -> None:
    from azula_amd.plugins.vdm import model as vm

    set_mode(monkeypatch, "f16x2")
    monkeypatch.setattr(vm, "CONV_OVERRIDE", H2D)


def assert_measured(plan, min_launches: int) -> None:
    r"""Every f16x2 launch of the tape measures its scale -- ``in_absmax0`` set, and ``in_absmax1`` exactly where there is a second
    source -- except behind yfcc's GroupNorm, and there are at least ``min_launches`` of them, some with two sources and some
    reading a source through nearest up-sampling."""
    names, h2 = read_tape(plan)
    dyn = [a for a, _ in h2 if a.in_absmax0]
    for a, after_norm in h2:
        assert a.in_absmax0 or after_norm
        assert bool(a.in_absmax1) == bool(a.src1) or not a.in_absmax0
    print(len(names), "launches,", len(h2), "f16x2 convolutions,", len(dyn), "with a measured scale,",
          sum(1 for a in dyn if a.src1), "on a concatenation,", sum(1 for a in dyn if a.up0 or a.up1), "through up = 1,",
          names.count("az_absmax_f32"), "absmax passes")
    assert len(dyn) >= min_launches and "az_absmax_f32" in names
    return dyn


@pytest.mark.parametrize("model", ["imagenet_128", "yfcc_1"])
def test_measured_scale_backbone(model, narrow_reference, monkeypatch):
    measured_scale(monkeypatch)
    state, x, t, out32, out64 = narrow_reference(model)
    net, _ = narrow(model, state)
    got = net(x.cuda(), t.cuda())
    dyn = assert_measured(next(iter(net._plans.values())), 100)
    assert any(a.src1 for a in dyn)
    if model == "imagenet_128":  # (nearest x2 read through the gather of a measured-scale launch, on either source)
        assert any(a.up1 for a in dyn if a.src1)
    check(f"{model} c = 32 [measured-scale f16x2]", got, out32, out64)


def test_measured_scale_hidden_activations_away_from_one(narrow_reference, monkeypatch):
    r"""The rescaled network (hidden tensors of 1e-3 .. 1e3 per block) where every such tensor meets a measured scale."""
    measured_scale(monkeypatch)
    state, x, t, _, _ = narrow_reference("imagenet_128")
    state = vc.rescale_blocks(state, vc.block_scales([(k, tuple(v.shape)) for k, v in state.items()], seed=7))
    out32 = vo.backbone("imagenet_128", state, x, t, 32)
    out64 = vo.backbone("imagenet_128", {k: v.double() for k, v in state.items()}, x.double(), t.double(), 32)
    net, _ = narrow("imagenet_128", state)
    got = net(x.cuda(), t.cuda())
    assert_measured(next(iter(net._plans.values())), 100)
    check("imagenet_128 c = 32 rescaled [measured-scale f16x2]", got, out32, out64)


@pytest.mark.parametrize("name", [n for n, c in vc.BLOCK_CASES.items() if c[0] == "skip"] + ["res_128_256_skip", "attn_256_8x8"])
def test_measured_scale_block(name, monkeypatch):
    r"""The SkipBlock cases (both concatenation orders, nearest through ``up = 1`` and bilinear), a projected residual block and an
    attention block, against the reference-written goldens."""
    from azula_amd.plugins.vdm.model import VDMPlan

    measured_scale(monkeypatch)
    kind, args, shape = vc.BLOCK_CASES[name]
    g = npz("blocks_" + kind)
    seq = vc.load_synthetic(vc.block_module(kind, args), salt=1).cuda()
    x = g[name + "/x"].cuda()
    plan = VDMPlan(seq, x.shape[0], x.shape[2], x.shape[3], x.shape[1], x.device)
    dyn = assert_measured(plan, 2)
    if kind == "skip":
        assert sum(1 for a in dyn if a.src1) >= 2
        assert (args["up"] == "nearest") == any(a.up0 or a.up1 for a in dyn)
    check(f"{name} [measured-scale f16x2]", plan(x), g[name + "/out32"], g[name + "/out64"])


# ------------------------------------------------------------------------------------------- denoiser and samplers
@pytest.fixture(scope="module")
def denoiser(full_width):
    from azula_amd.plugins.vdm import VelocityDenoiser

    return VelocityDenoiser(full_width("imagenet_128")).eval()


def test_denoiser_forward_per_sample_times(denoiser):
    g = npz("denoiser")
    x_t, t = g["forward/x_t"], g["forward/t"]
    assert t.shape == (2,)
    q = denoiser(x_t.cuda(), t.cuda())
    from azula_amd.denoise import DiracPosterior

    assert isinstance(q, DiracPosterior)
    check("VelocityDenoiser.forward", q.mean, g["forward/mean32"], g["forward/mean64"])


def stored_noise(sampler, noises):
    r"""Answers the sampler's per-step ``randn_like`` from the golden's stored noises."""
    it = iter(noises)

    def draw(like, out=None):
        eps = next(it).to(like)
        return eps if out is None else out.copy_(eps)

    sampler._draw_noise = draw
    return sampler


@pytest.mark.parametrize("kind", ["ddim4", "ddpm4"])
def test_fused_sampler_equals_the_reference_sampler(kind, denoiser):
    from azula_amd import sample as S

    g = npz("denoiser")
    x1, noises = g["sampler/x1"], list(g["sampler/eps"])
    assert x1.shape == (2, 3, 32, 32) and len(noises) == 4
    smp = (S.DDIMSampler if kind == "ddim4" else S.DDPMSampler)(denoiser, steps=4, silent=True)
    x0 = stored_noise(smp, noises)(x1.cuda())
    assert len(smp._fused_cache) == 1, "the sampler did not take the captured loop"
    check(f"{kind} fused", x0, g["sampler/" + kind], g["sampler/" + kind + "_64"])


@pytest.mark.parametrize("kind", ["heun", "zeab"])
def test_fused_sampler_agrees_with_the_unfused_loop(kind, narrow_reference):
    r"""Heun / zEAB through the captured loop against the same sampler's generic loop (one ``denoiser.forward`` per evaluation):
    both evaluate the same fp32 statements on the same kernels, up to the preconditioning being fused into the transition, so
    they agree to the generic loop's own rounding -- 1e-5 of the result's scale."""
    from azula_amd import sample as S
    from azula_amd.plugins.vdm import VelocityDenoiser

    net, _ = narrow("imagenet_128", narrow_reference("imagenet_128")[0])
    den = VelocityDenoiser(net).eval()
    x1 = vc.image("sampler/x1", (2, 3, 32, 32)).cuda()
    make = (lambda: S.HeunSampler(den, steps=4, silent=True)) if kind == "heun" else (lambda: S.zEABSampler(den, steps=4, silent=True))
    fused = make()
    x0 = fused(x1)
    assert len(fused._fused_cache) == 1
    loop = make()
    loop._call_fused = lambda x, kwargs: None
    ref = loop(x1)
    err, scale = float((x0 - ref).abs().max()), float(ref.abs().max())
    print(f"{kind}: fused vs generic {err:.3e} scale {scale:.3g}")
    assert torch.isfinite(x0).all() and err <= 1e-5 * max(1.0, scale)


def test_sampler_float64_runs(narrow_reference):
    from azula_amd import sample as S
    from azula_amd.plugins.vdm import VelocityDenoiser

    net, _ = narrow("imagenet_128", narrow_reference("imagenet_128")[0])
    den = VelocityDenoiser(net).eval()
    x1 = vc.image("sampler/x1", (2, 3, 32, 32)).cuda()
    x0 = S.DDIMSampler(den, steps=4, silent=True, dtype=torch.float64)(x1)
    x0_32 = S.DDIMSampler(den, steps=4, silent=True)(x1)
    assert x0.dtype == torch.float64 and torch.isfinite(x0).all()
    err = float((x0 - x0_32.double()).abs().max())
    print(f"fp64 clock vs fp32 clock: {err:.3e}")
    assert err <= 1e-4 * max(1.0, float(x0.abs().max()))


def test_gradient_guidance_fails_clearly(narrow_reference):
    from azula_amd.guidance._vjp import mean_and_pullback
    from azula_amd.plugins.vdm import VelocityDenoiser

    net, _ = narrow("imagenet_128", narrow_reference("imagenet_128")[0])
    den = VelocityDenoiser(net).eval()
    x = vc.image("sampler/x1", (1, 3, 32, 32)).cuda()
    with pytest.raises(NotImplementedError, match="VelocityDenoiser has no input-gradient path"):
        mean_and_pullback(den, x, torch.tensor(0.5).cuda(), {})


def test_plan_sees_reloaded_weights(narrow_reference):
    from azula_amd import sample as S
    from azula_amd.plugins.vdm import VelocityDenoiser

    state = narrow_reference("imagenet_128")[0]
    net, _ = narrow("imagenet_128", state)
    den = VelocityDenoiser(net).eval()
    x1 = vc.image("sampler/x1", (2, 3, 32, 32)).cuda()
    smp = S.DDIMSampler(den, steps=4, silent=True)
    a = smp(x1)
    with torch.device("meta"):
        spec = vc.spec_of(type(net)("imagenet_128", base_channels=32))
    other = vc.synthesise_model("imagenet_128", spec, salt=3)
    net.load_state_dict(other)
    b = smp(x1)
    fresh_net, _ = narrow("imagenet_128", other)
    fresh = S.DDIMSampler(VelocityDenoiser(fresh_net).eval(), steps=4, silent=True)(x1)
    assert not torch.equal(a, b) and torch.equal(b, fresh), "the cached plan replayed stale packed weights"
    y_a = net(x1, torch.tensor([0.3]).cuda())
    net.load_state_dict(state)
    assert not torch.equal(net(x1, torch.tensor([0.3]).cuda()), y_a)
