r"""``UNetModel.vjp`` (``ADMGradPlan``: HIP forward-keep + backward tapes), ``AblatedDenoiser._az_vjp`` and one DPS / MMPS step on
ADM, against fp64 autograd through the oracle (``oracle.nets.adm_unet_forward``, ``oracle.sampling.adm_posterior``).

The oracle runs in fp64 once ``nets.adm_timestep_embedding`` (always fp32) is cast to the weights' dtype (``emb_cast`` below); its
attention softmax stays fp32 by the reference's own cast, which the 1e-4 floor covers.

Bounds.  (a) the forward of the gradient plan: ``tests/test_gpu_adm.py``'s forward bounds on the same fixtures.  Every pullback:
``max(4 e_ref, 1e-4)`` relative to the largest magnitude of the fp64 result, ``e_ref`` = what the ORACLE's own fp32 autograd loses
against fp64 on the same quantity, measured here on the CPU (the rule of ``tests/test_gpu_unet_vjp.py``).
"""

import contextlib

import pytest
import torch

import guidance_vjp_oracle as go
from conftest import max_err
from oracle import nets, sampling, synth

pytestmark = pytest.mark.gpu

# fixture -> the forward bound tests/test_gpu_adm.py applies to it (relative to max(1, |out|max))
FIXTURES = {
    "g5_adm_uncond": 7e-6, "g5_adm_cond_neworder": 7e-6,
    "g14_adm_plain_conv": 5e-6, "g14_adm_plain_pool": 5e-6, "g14_adm_film_noupdown": 5e-6,
    "g24_adm_hd24_legacy": 5e-6, "g24_adm_hd48_hd96_neworder": 5e-6,
    "g22_adm_1d_film_updown": 7e-6, "g22_adm_1d_plain_conv": 7e-6, "g22_adm_1d_plain_pool": 7e-6,
}


@contextlib.contextmanager
def emb_cast(dtype):
    orig = nets.adm_timestep_embedding
    nets.adm_timestep_embedding = lambda *a, **k: orig(*a, **k).to(dtype)
    try:
        yield
    finally:
        nets.adm_timestep_embedding = orig


def build(g):
    from azula_amd.plugins import adm

    cfg = g.meta["cfg"]
    den = adm.make_model(**cfg)
    shapes = {k: tuple(v) for k, v in g.meta["shapes"].items()}
    sd = synth.synth_state_dict(shapes, g.meta["weight_seed"])
    den.backbone.load_state_dict(sd)
    return den.cuda().eval(), sd, cfg


def backbone_fn(sd, cfg, dtype):
    sdd = {k: v.to(dtype) for k, v in sd.items()}

    def fn(x, idx, y=None):
        with emb_cast(dtype):
            return nets.adm_unet_forward(sdd, cfg, x, idx, y)

    return fn


def oracle_vjp(fn, x, v, dtype):
    xx = x.detach().to(dtype).clone().requires_grad_()
    with torch.enable_grad():  # (other test modules switch gradients off for the whole session)
        y = fn(xx)
        return y.detach().double(), torch.autograd.grad(y, xx, v.to(dtype))[0].double()


def rel(a, ref):
    return float((a.double().cpu() - ref).abs().max() / ref.abs().max())


def bound(e_ref):
    return max(4 * e_ref, 1e-4)


@pytest.mark.parametrize("name", list(FIXTURES))
def test_adm_unet_vjp(golden, name):
    g = golden(name)
    den, sd, cfg = build(g)
    net = den.backbone
    x, idx = g["x"], g["idx"]
    y = g["y"] if "y" in g else None
    gen = torch.Generator().manual_seed(7)
    v = torch.randn(g["out"].shape, generator=gen)
    u = torch.randn(x.shape, generator=gen)
    xd, yd = x.cuda(), None if y is None else y.cuda()
    f64 = lambda xx: backbone_fn(sd, cfg, torch.float64)(xx, idx, y)  # noqa: E731
    f32 = lambda xx: backbone_fn(sd, cfg, torch.float32)(xx, idx, y)  # noqa: E731

    out, pull = net.vjp(xd, idx.cuda(), yd)
    # (a) the forward-keep tape computes what the sampling plan computes, and the golden output
    scale = max(1.0, g["out"].abs().max().item())
    err_plan, err_gold = max_err(out, net(xd, idx.cuda(), y=yd)), max_err(out, g["out"])
    print(name, "(a) forward-keep vs sampling plan:", err_plan, "vs golden:", err_gold, "scale", scale)
    assert out.shape == g["out"].shape
    assert err_plan < FIXTURES[name] * scale and err_gold < FIXTURES[name] * scale

    # (b) pullback of a random cotangent
    _, ref = oracle_vjp(f64, x, v, torch.float64)
    _, ref32 = oracle_vjp(f32, x, v, torch.float32)
    e_ref = rel(ref32, ref)
    dx = pull(v.cuda())
    err_b = rel(dx, ref)
    print(name, f"(b) pullback err {err_b:.3e} e_ref {e_ref:.3e}")
    assert dx.shape == x.shape and torch.isfinite(dx).all()
    assert err_b < bound(e_ref)

    # (e) a second pullback after the same forward: same bits
    assert torch.equal(pull(v.cuda()), dx)

    # (c) adjoint identity <J u, v> = <u, J^T v>, J u from the fp64 oracle
    with torch.enable_grad():
        _, ju = torch.func.jvp(f64, (x.double(),), (u.double(),))
    lhs = float((ju * v.double()).sum())
    rhs = float((u.double() * dx.double().cpu()).sum())
    norm = float(ju.norm() * v.double().norm())
    print(name, f"(c) adjoint identity: {lhs:.9e} vs {rhs:.9e} (|Ju||v| = {norm:.3e})")
    assert abs(lhs - rhs) < bound(e_ref) * norm

    # (d) linearity over the range a cotangent takes
    for s in (1e-6, 1e4):
        dxs = pull((v * s).cuda())
        err_d = rel(dxs, ref * s)
        print(name, f"(d) pullback({s:g} v) err {err_d:.3e}")
        assert torch.isfinite(dxs).all()
        assert err_d < bound(e_ref)

    # a pullback of an earlier forward is refused once the plan has run again
    net.vjp(xd, idx.cuda(), yd)
    with pytest.raises(RuntimeError, match="earlier vjp"):
        pull(v.cuda())


@pytest.mark.parametrize("name", ["g5_adm_uncond", "g14_adm_plain_conv", "g24_adm_hd24_legacy"])
def test_tape_shape(golden, name):
    r"""No SiLU pass on either tape (the norm pullback recomputes silu' from its input: nothing but x and the statistics is
    kept); every f16x2 convolution on the backward tape takes its activation scale from a measured maximum."""
    from azula_amd import engine

    g = golden(name)
    den, _, _ = build(g)
    net = den.backbone
    x = g["x"].cuda()
    net.vjp(x, g["idx"].cuda(), g["y"].cuda() if "y" in g else None)
    rows = x.shape[0] if (g["idx"].numel() > 1 or net.num_classes is not None) else 1
    plan = net.grad_plan(x.shape[0], x.shape[-2], x.shape[-1], rows, x.device)
    fwd, bwd = [op for _, _, op in plan.fwd.ops], [op for _, _, op in plan.bwd.ops]
    assert "az_silu_f32" not in fwd and "az_act_f32" not in fwd
    assert "az_silu_bwd_f32" not in bwd and "az_act_bwd_f32" not in bwd
    assert "az_groupnorm_bwd_apply_f32" not in bwd
    norms = sum(op == "az_affine_act_f32" for op in fwd)
    assert sum(op == "az_norm_affine_bwd_apply_f32" for op in bwd) > 0
    assert sum(op == "az_norm_affine_bwd_stats_f32" for op in bwd) == sum(op == "az_norm_affine_bwd_apply_f32" for op in bwd) <= norms
    convs = 0
    for fn, args, op in plan.bwd.ops:
        if op.startswith("az_conv2d"):
            convs += 1
            a = args[0]._obj
            assert not a.in_affine
            if op in engine.H2_NAMES:
                assert a.in_absmax0, f"{op}: fixed-scale f16x2 launch on a cotangent"
    assert convs >= 4
    assert plan.saved_bytes > 0


def test_card_shaped_case():
    r"""The imagenet cards' wiring (FiLM, resblock_updown, 64-channel heads, attention at 16 x 16) at 128 channels, 1 x 3 x 64 x 64."""
    from azula_amd.plugins import adm

    cfg = dict(image_size=64, num_channels=128, channel_mult=[1, 2, 2], num_res_blocks=2, attention_resolutions=[16],
               num_head_channels=64, resblock_updown=True, use_scale_shift_norm=True)
    den = adm.make_model(**cfg)
    sd = synth.synth_state_dict({k: tuple(v.shape) for k, v in den.backbone.state_dict().items()}, 31)
    den.backbone.load_state_dict(sd)
    net = den.backbone.cuda().eval()
    gen = torch.Generator().manual_seed(32)
    x = torch.randn(1, 3, 64, 64, generator=gen)
    v = torch.randn(1, 6, 64, 64, generator=gen)
    idx = torch.tensor([417])
    torch.set_num_threads(min(16, torch.get_num_threads()))
    _, ref = oracle_vjp(lambda xx: backbone_fn(sd, cfg, torch.float64)(xx, idx), x, v, torch.float64)
    _, ref32 = oracle_vjp(lambda xx: backbone_fn(sd, cfg, torch.float32)(xx, idx), x, v, torch.float32)
    e_ref = rel(ref32, ref)
    out, pull = net.vjp(x.cuda(), idx.cuda())
    dx = pull(v.cuda())
    err = rel(dx, ref)
    print(f"card-shaped pullback err {err:.3e} e_ref {e_ref:.3e}")
    assert torch.isfinite(out).all() and torch.isfinite(dx).all()
    assert err < bound(e_ref)
    assert max_err(out, net(x.cuda(), idx.cuda())) < 7e-6 * max(1.0, out.abs().max().item())


def posterior_fn(sd, cfg, dtype, label=None, clip=True):
    sig = sampling.adm_sigmas(cfg["discrete_schedule"], cfg["discrete_steps"]).to(dtype)
    bb = backbone_fn(sd, cfg, dtype)
    return lambda x, t: sampling.adm_posterior(bb, x, t, sig, label=label, clip_mean=clip)[0]


@pytest.mark.parametrize("name", ["g5_adm_uncond", "g5_adm_cond_neworder"])
@pytest.mark.parametrize("mode", ["scalar_t", "per_sample_t", "train", "no_clip"])
def test_denoiser_pullback(golden, name, mode):
    g = golden(name)
    den, sd, cfg = build(g)
    label = g["y"] if "y" in g else None
    x_t = 0.5 * g["x"]
    B = x_t.shape[0]
    t = torch.tensor([0.3, 0.6][:B] + [0.3] * max(0, B - 2)) if mode == "per_sample_t" else torch.tensor(0.3)
    clip = mode in ("scalar_t", "per_sample_t")
    if mode == "train":
        den.train()
    elif mode == "no_clip":
        den.clip_mean = False
    v = torch.randn(x_t.shape, generator=torch.Generator().manual_seed(9))

    def run(dtype):
        mean = posterior_fn(sd, cfg, dtype, label, clip)
        x = x_t.to(dtype).requires_grad_()
        with torch.enable_grad():
            m = mean(x, t.to(dtype))
            return m.detach().double(), torch.autograd.grad(m, x, v.to(dtype))[0].double()

    m64, ref = run(torch.float64)
    _, ref32 = run(torch.float32)
    e_ref = rel(ref32, ref)
    kw = {"label": label.cuda()} if label is not None else {}
    mean, pull = den._az_vjp(x_t.cuda(), t.cuda(), **kw)
    mask64 = m64.abs() < 1.0 if clip else torch.ones_like(m64, dtype=torch.bool)
    mask = mean.abs().cpu() < 1.0 if clip else torch.ones_like(mask64)
    print(name, mode, f"clipped share {1 - mask64.double().mean().item():.3f}, mask flips {(mask != mask64).sum().item()}")
    assert torch.equal(mask, mask64), "the GPU mean clips other elements than the fp64 oracle"
    assert max_err(mean, m64) < 5e-5  # (the posterior bound of tests/test_gpu_adm.py)
    dx = pull(v.cuda())
    err = rel(dx, ref)
    print(name, mode, f"_az_vjp pullback err {err:.3e} e_ref {e_ref:.3e}")
    assert torch.isfinite(dx).all() and err < bound(e_ref)
    assert torch.equal(pull(v.cuda()), dx)


@pytest.fixture(scope="module")
def guided(golden):
    g = golden("g5_adm_uncond")
    den, sd, cfg = build(g)
    x_t = 0.5 * g["x"]
    gen = torch.Generator().manual_seed(78)
    mask = (torch.rand(1, *x_t.shape[1:], generator=gen) < 0.5).float()
    A = lambda x: (x * mask.to(x)).flatten(1)  # noqa: E731
    y = A(torch.randn(x_t.shape, generator=gen))
    sched = lambda t: sampling.vp_schedule(t, 1e-2, 1e-2)  # noqa: E731
    return dict(den=den, mean=lambda dt: posterior_fn(sd, cfg, dt), x_t=x_t, y=y, A=A, t=torch.tensor(0.3), s=torch.tensor(0.25), sched=sched)


def both(fn, s):
    r64 = fn(s["mean"](torch.float64), lambda v: v.double())
    r32 = fn(s["mean"](torch.float32), lambda v: v.float())
    return r64.double(), rel(r32, r64.double())


def test_dps_step(guided):
    from azula_amd.guidance import DPSSampler

    s = guided
    A = s["A"]
    smp = DPSSampler(s["den"], s["y"].cuda(), lambda x: A(x), steps=8, silent=True)
    torch.manual_seed(5)
    eps = torch.randn_like(s["x_t"].cuda()).cpu()
    torch.manual_seed(5)
    out = smp.step(s["x_t"].cuda(), s["t"].cuda(), s["s"].cuda())
    ref, e_ref = both(lambda mean, cast: go.dps_step(mean, cast(s["x_t"]), cast(s["t"]), cast(s["s"]), cast(eps), cast(s["y"]), A,
                                                     schedule=s["sched"]), s)
    err = rel(out, ref)
    print(f"DPS step on ADM: err {err:.3e} e_ref {e_ref:.3e}")
    assert out.shape == ref.shape and torch.isfinite(out).all()
    assert err < bound(e_ref)


def test_mmps_denoiser(guided):
    from azula_amd.guidance import MMPSDenoiser
    from azula_amd.linalg.covariance import IsotropicCovariance

    s = guided
    A = s["A"]
    var_y = 0.01
    cov = IsotropicCovariance(torch.tensor(var_y, device="cuda"))
    out = MMPSDenoiser(s["den"], s["y"].cuda(), lambda x: A(x), cov, solver="gmres", iterations=2)(s["x_t"].cuda(), s["t"].cuda()).mean
    ref, e_ref = both(lambda mean, cast: go.mmps_mean(mean, cast(s["x_t"]), cast(s["t"]), cast(s["y"]), A, lambda v: var_y * v, "gmres", 2,
                                                      schedule=s["sched"]), s)
    err = rel(out, ref)
    print(f"MMPS (gmres, 2 iterations) on ADM: err {err:.3e} e_ref {e_ref:.3e}")
    assert out.shape == ref.shape and torch.isfinite(out).all()
    assert err < bound(e_ref)
