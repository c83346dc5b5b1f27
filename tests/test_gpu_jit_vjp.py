r"""``JiT.vjp`` (``JiTGradPlan``: HIP forward-keep + backward tapes), ``JITDenoiser._az_vjp``, ``CFGDenoiser._az_vjp`` (the guided
mean as ONE pullback of the stacked 2B batch, around JiT and around the class-conditional ADM) and one DPS / MMPS step on the
guided JiT prior, against fp64 autograd through the oracle (``oracle.nets.jit_forward``, ``oracle.sampling.jit_mean`` /
``adm_posterior``).

The oracle's ``nets.jit_rms_norm`` takes its statistics in fp32 whatever the input type, so an fp64 run through it is not fp64
(it deviates 1.2e-7 from one on ``g10_jit_ctx``): every test here runs the oracle with a dtype-preserving version.

Bounds, as in ``test_gpu_dit_vjp.py``.  The forward of a gradient plan: ``1e-4 * max(1, |y|max)`` against the sampling plan and
against the oracle.  A pullback: ``max(4 e_ref, 1e-4)`` relative to the largest magnitude of the fp64 result, ``e_ref`` being what
the ORACLE's own fp32 autograd loses against fp64 on the same quantity (measured here on the CPU, never from the code under test;
3.7e-7 .. 7.1e-7 on these fixtures, so the bound is the 1e-4 floor).
"""

import pytest
import torch

import guidance_vjp_oracle as go
from conftest import max_err
from oracle import nets, sampling, synth
from test_gpu_adm_vjp import build as build_adm
from test_gpu_adm_vjp import posterior_fn
from test_gpu_dit_vjp import FWD_TOL, bound, check_vjp, oracle_vjp, rel

pytestmark = pytest.mark.gpu

FIXTURES = ["g10_jit_ctx", "g10_jit_noctx_hd32", "g10_jit_hd80", "g24_jit_hd48"]  # heads of 16, 32, 80 -> 128 and 48 -> 64 channels
T3 = torch.linspace(0.3, 0.8, 3)


@pytest.fixture(autouse=True)
def fp64_rms_norm(monkeypatch):
    monkeypatch.setattr(nets, "jit_rms_norm", lambda x, weight, eps=1e-6: weight * x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps))


def build(g):
    from azula_amd.plugins import jit

    cfg = g.meta["cfg"]
    sd = synth.synth_state_dict({k: tuple(v) for k, v in g.meta["shapes"].items()}, g.meta["weight_seed"])
    net = jit.JiT(**cfg)
    net.load_state_dict(sd)
    return jit.JITDenoiser(net, num_classes=cfg["num_classes"]).cuda().eval(), sd, cfg


def backbone_fn(sd, cfg, dtype):
    sdd = {k: v.to(dtype) if v.is_floating_point() else v for k, v in sd.items()}
    return lambda x, t, y: nets.jit_forward(sdd, cfg, x, t.to(dtype), y)


def jit_fn(sd, cfg, t, y):
    return lambda dtype: (lambda xx: backbone_fn(sd, cfg, dtype)(xx, t, y))


def pair(run):
    r"""``run(dtype) -> (mean, grad)`` in fp64 and fp32: the fp64 results and the oracle's own fp32 loss on the gradient."""
    m64, ref = run(torch.float64)
    _, ref32 = run(torch.float32)
    return m64, ref, rel(ref32, ref)


def mean_grad(mean_fn, x_t, t, v):
    def run(dtype):
        x = x_t.to(dtype).requires_grad_()
        with torch.enable_grad():
            m = mean_fn(dtype)(x, t.to(dtype))
            return m.detach().double(), torch.autograd.grad(m, x, v.to(dtype))[0].double()

    return pair(run)


# ------------------------------------------------------------------------------------------------ JiT.vjp
@pytest.mark.parametrize("shared", [False, True], ids=["per_sample_t", "shared_t"])
@pytest.mark.parametrize("name", FIXTURES)
def test_jit_vjp(golden, name, shared):
    g = golden(name)
    den, sd, cfg = build(g)
    net = den.backbone
    x, y = g["x"], g["y"].long()
    t = T3[1:2] if shared else T3
    xd, td, yd = x.cuda(), t.cuda(), y.cuda()
    check_vjp(f"{name} shared_t={shared}", lambda: net.vjp(xd, td, yd), lambda: net(xd, td, yd), jit_fn(sd, cfg, t.expand(3), y), x, 71)
    # measured (MI355X): forward-keep <= 1.2e-6 vs the plan, <= 2.4e-6 vs the oracle; pullback <= 8.7e-7 (e_ref 3.7e-7 .. 7.1e-7),
    # <= 9.7e-7 under scaling; adjoint identity within 5e-9 |Ju||v|
    plan = next(p for k, p in net._plans.items() if k[0] == "vjp")
    assert plan.saved_bytes > 0
    bwd = [op for _, _, op in plan.bwd.ops]
    depth = cfg["depth"]
    assert bwd.count("az_rownorm_bwd_w_f32") == 2 * depth + 1 and bwd.count("az_qk_prep_bwd_w_f32") == depth
    assert bwd.count("az_attention_bwd_f32") == depth and bwd.count("az_swiglu_bwd_f32") == depth
    assert [op for _, _, op in plan.fwd.ops].count("az_qk_prep_w_f32") == depth


def test_jit_vjp_plans(golden):
    r"""The gradient plan leaves the sampling plan alone (its forward gives the same bits before and after a ``vjp``) and is
    rebuilt after an in-place parameter change."""
    g = golden("g10_jit_ctx")
    den, sd, cfg = build(g)
    net = den.backbone
    x, y = g["x"], g["y"].long()
    xd, td, yd = x.cuda(), T3.cuda(), y.cuda()
    before = net(xd, td, yd)
    out, pull = net.vjp(xd, td, yd)
    v = torch.randn(out.shape, generator=torch.Generator().manual_seed(72))
    dx = pull(v.cuda())
    assert torch.equal(net(xd, td, yd), before)
    assert torch.equal(pull(v.cuda()), dx)  # (the sampling plan's run did not touch the saved tensors)
    plan = next(p for k, p in net._plans.items() if k[0] == "vjp")
    key = "blocks.1.norm2.weight"
    with torch.no_grad():
        net.get_parameter(key).mul_(1.5)
    with pytest.raises(RuntimeError, match="earlier vjp"):  # (also before the next vjp call builds a new plan)
        pull(v.cuda())
    sd2 = dict(sd)
    sd2[key] = sd[key] * 1.5
    out2, pull2 = net.vjp(xd, td, yd)
    assert next(p for k, p in net._plans.items() if k[0] == "vjp") is not plan
    with pytest.raises(RuntimeError, match="earlier vjp"):  # (the old tapes read some parameters in place: refused, not mixed)
        pull(v.cuda())
    y64, ref, e_ref = pair(lambda dtype: oracle_vjp(jit_fn(sd2, cfg, T3, y)(dtype), x, v, dtype))
    err = rel(pull2(v.cuda()), ref)
    print(f"after an in-place change of {key}: forward err {max_err(out2, y64):.3e}, pullback err {err:.3e} e_ref {e_ref:.3e}")
    assert max_err(out2, y64) < FWD_TOL * max(1.0, y64.abs().max().item()) and err < bound(e_ref)
    assert rel(dx, ref) > 1e-3  # (the change is visible in the gradient: the new plan is not the old one)


# ------------------------------------------------------------------------------------------------ JITDenoiser._az_vjp
def jit_mean_fn(sd, cfg, label):
    return lambda dtype: (lambda x, t: sampling.jit_mean(backbone_fn(sd, cfg, dtype), x, t, label=label, num_classes=cfg["num_classes"]))


@pytest.mark.parametrize("t,labelled", [(0.4, True), (0.7, False)], ids=["t04_labels", "t07_null_class"])
def test_denoiser_pullback(golden, t, labelled):
    g = golden("g10_jit_ctx")
    den, sd, cfg = build(g)
    x_t, t = g["x"], torch.tensor(t)
    label = g["y"].long() if labelled else None
    v = torch.randn(x_t.shape, generator=torch.Generator().manual_seed(73))
    m64, ref, e_ref = mean_grad(jit_mean_fn(sd, cfg, label), x_t, t, v)
    mean, pull = den._az_vjp(x_t.cuda(), t.cuda(), **({"label": label.cuda()} if labelled else {}))
    dx = pull(v.cuda())
    err_m, err = max_err(mean, m64), rel(dx, ref)
    print(f"JITDenoiser._az_vjp t={t:g} labelled={labelled}: mean err {err_m:.3e}, pullback err {err:.3e} e_ref {e_ref:.3e}")
    assert err_m < FWD_TOL * max(1.0, m64.abs().max().item())
    assert torch.isfinite(dx).all() and err < bound(e_ref)  # measured <= 7.9e-7, mean <= 1.8e-6 (MI355X)
    assert torch.equal(pull(v.cuda()), dx)
    assert max_err(mean, den(x_t.cuda(), t.cuda(), label=None if label is None else label.cuda()).mean) < FWD_TOL * max(1.0, m64.abs().max().item())


# ------------------------------------------------------------------------------------------------ CFGDenoiser._az_vjp
def guided_fn(pos_fn, neg_fn, guidance):
    def fn(dtype):
        mp, mn = pos_fn(dtype), neg_fn(dtype)

        def mean(x, t):
            a, b = mp(x, t), mn(x, t)
            return a + guidance * (a - b)

        return mean

    return fn


def test_cfg_pullback_jit(golden):
    from azula_amd.guidance import CFGDenoiser

    g = golden("g10_jit_ctx")
    den, sd, cfg = build(g)
    x_t, t, y, guidance = g["x"], torch.tensor(0.4), g["y"].long(), 2.5
    v = torch.randn(x_t.shape, generator=torch.Generator().manual_seed(74))
    m64, ref, e_ref = mean_grad(guided_fn(jit_mean_fn(sd, cfg, y), jit_mean_fn(sd, cfg, None), guidance), x_t, t, v)
    cfgden = CFGDenoiser(den)
    mean, pull = cfgden._az_vjp(x_t.cuda(), t.cuda(), positive={"label": y.cuda()}, negative={}, guidance=guidance)
    dx = pull(v.cuda())
    err_m, err = max_err(mean, m64), rel(dx, ref)
    print(f"CFG(JiT) guidance {guidance}: mean err {err_m:.3e}, pullback err {err:.3e} e_ref {e_ref:.3e}")
    # measured (MI355X): mean 5.6e-6 / 7.7e-6 (per-sample t), pullback 7.1e-7 / 6.8e-7 (e_ref 6.6e-7 / 8.6e-7)
    assert mean.shape == x_t.shape and dx.shape == x_t.shape
    assert err_m < FWD_TOL * max(1.0, m64.abs().max().item())
    assert torch.isfinite(dx).all() and err < bound(e_ref)
    assert torch.equal(pull(v.cuda()), dx)
    # the guided mean of the gradient path is the guided mean of the sampling path
    fwd = cfgden(x_t.cuda(), t.cuda(), positive={"label": y.cuda()}, guidance=guidance).mean
    assert max_err(mean, fwd) < FWD_TOL * max(1.0, m64.abs().max().item())
    # per-sample times repeat over the two halves
    m64, ref, e_ref = mean_grad(guided_fn(jit_mean_fn(sd, cfg, y), jit_mean_fn(sd, cfg, None), guidance), x_t, T3, v)
    mean, pull = cfgden._az_vjp(x_t.cuda(), T3.cuda(), positive={"label": y.cuda()}, guidance=guidance)
    err_m, err = max_err(mean, m64), rel(pull(v.cuda()), ref)
    print(f"CFG(JiT) per-sample t: mean err {err_m:.3e}, pullback err {err:.3e} e_ref {e_ref:.3e}")
    assert err_m < FWD_TOL * max(1.0, m64.abs().max().item()) and err < bound(e_ref)


def test_cfg_pullback_adm(golden):
    from azula_amd.guidance import CFGDenoiser

    g = golden("g5_adm_cond_neworder")
    den, sd, cfg = build_adm(g)
    x_t, t, guidance = 0.5 * g["x"], torch.tensor(0.3), 1.5
    y, neg = g["y"], g["neg_label"]
    B = x_t.shape[0]
    v = torch.randn(x_t.shape, generator=torch.Generator().manual_seed(75))
    pos_fn = lambda dtype: posterior_fn(sd, cfg, dtype, y)  # noqa: E731
    neg_fn = lambda dtype: posterior_fn(sd, cfg, dtype, neg)  # noqa: E731
    m64, ref, e_ref = mean_grad(guided_fn(pos_fn, neg_fn, guidance), x_t, t, v)
    # the clip masks of the stacked batch (what AblatedDenoiser._az_vjp computes per row) are the fp64 oracle's, branch by branch
    with torch.no_grad():
        branch64 = torch.cat([f(torch.float64)(x_t.double(), t.double()) for f in (pos_fn, neg_fn)])
    mean2, _ = den._az_vjp(torch.cat((x_t, x_t)).cuda(), t.cuda(), label=torch.cat((y, neg)).cuda())
    mask, mask64 = mean2.abs().cpu() < 1.0, branch64.abs() < 1.0
    print(f"CFG(ADM): clipped share {1 - mask64.double().mean().item():.3f}, mask flips {(mask != mask64).sum().item()}")
    assert torch.equal(mask, mask64), "the GPU means clip other elements than the fp64 oracle"
    mean, pull = CFGDenoiser(den)._az_vjp(x_t.cuda(), t.cuda(), positive={"label": y.cuda()}, negative={"label": neg.cuda()}, guidance=guidance)
    assert torch.equal(mean, mean2[:B] + guidance * (mean2[:B] - mean2[B:]))  # az_cfg_combine_f32 over the two halves
    dx = pull(v.cuda())
    err_m, err = max_err(mean, m64), rel(dx, ref)
    print(f"CFG(ADM) guidance {guidance}: mean err {err_m:.3e}, pullback err {err:.3e} e_ref {e_ref:.3e}")
    # measured (MI355X): mean 6.3e-6, pullback 2.1e-6 (e_ref 2.8e-6), clipped share 0.337, no mask flip
    assert err_m < FWD_TOL * max(1.0, m64.abs().max().item())
    assert torch.isfinite(dx).all() and err < bound(e_ref)
    assert torch.equal(pull(v.cuda()), dx)
    with pytest.raises(NotImplementedError, match="CFG"):
        CFGDenoiser(den)._az_vjp(x_t.cuda(), t.cuda(), positive={"label": y.cuda()})  # ADM has no null class


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def guided(golden):
    from azula_amd.guidance import CFGDenoiser

    g = golden("g10_jit_ctx")
    den, sd, cfg = build(g)
    x_t, y_lab, guidance = g["x"], g["y"].long(), 2.5
    A = lambda x: x[..., ::2, ::2].flatten(1)  # noqa: E731  (a linear subsampling)
    y = A(torch.randn(x_t.shape, generator=torch.Generator().manual_seed(76)))
    mean = guided_fn(jit_mean_fn(sd, cfg, y_lab), jit_mean_fn(sd, cfg, None), guidance)
    kw = dict(positive={"label": y_lab.cuda()}, guidance=guidance)
    return dict(den=CFGDenoiser(den), mean=mean, x_t=x_t, y=y, A=A, t=torch.tensor(0.4), s=torch.tensor(0.35), kw=kw)


def both(fn, s):
    # (the module-scoped fixture outlives the per-test monkeypatch: the oracle calls run inside the tests, under it)
    r64 = fn(s["mean"](torch.float64), lambda v: v.double()).double()
    r32 = fn(s["mean"](torch.float32), lambda v: v.float())
    return r64, rel(r32, r64)


def test_dps_step(guided):
    from azula_amd.guidance import DPSSampler

    s = guided
    A = s["A"]
    smp = DPSSampler(s["den"], s["y"].cuda(), lambda x: A(x), steps=8, silent=True)
    torch.manual_seed(5)
    eps = torch.randn_like(s["x_t"].cuda()).cpu()
    torch.manual_seed(5)
    out = smp.step(s["x_t"].cuda(), s["t"].cuda(), s["s"].cuda(), **s["kw"])
    ref, e_ref = both(lambda mean, cast: go.dps_step(mean, cast(s["x_t"]), cast(s["t"]), cast(s["s"]), cast(eps), cast(s["y"]), A,
                                                     schedule=sampling.rectified_schedule), s)
    err = rel(out, ref)
    print(f"DPS step on CFG(JiT): err {err:.3e} e_ref {e_ref:.3e}")
    assert out.shape == ref.shape and torch.isfinite(out).all()
    assert err < bound(e_ref)  # measured 5.1e-7 (e_ref 5.8e-7, MI355X)


def test_mmps_denoiser(guided):
    from azula_amd.guidance import MMPSDenoiser
    from azula_amd.linalg.covariance import IsotropicCovariance

    s = guided
    A = s["A"]
    var_y = 0.01
    cov = IsotropicCovariance(torch.tensor(var_y, device="cuda"))
    out = MMPSDenoiser(s["den"], s["y"].cuda(), lambda x: A(x), cov, solver="gmres", iterations=2)(s["x_t"].cuda(), s["t"].cuda(), **s["kw"]).mean
    ref, e_ref = both(lambda mean, cast: go.mmps_mean(mean, cast(s["x_t"]), cast(s["t"]), cast(s["y"]), A, lambda v: var_y * v, "gmres", 2,
                                                      schedule=sampling.rectified_schedule), s)
    err = rel(out, ref)
    print(f"MMPS (gmres, 2 iterations) on CFG(JiT): err {err:.3e} e_ref {e_ref:.3e}")
    assert out.shape == ref.shape and torch.isfinite(out).all()
    assert err < bound(e_ref)  # measured 5.5e-7 (e_ref 5.2e-7, MI355X)
