r"""``UNetBlock.vjp`` and ``UNet.vjp`` (HIP forward-keep + backward tapes) against fp64 autograd through the oracle
(``oracle.nets.unet_forward`` / ``unet_block``) on the G5 UNet fixtures.

Bounds.  (a) the forward of the gradient plan: the fixture's existing forward bound, ``1e-4 * max(1, |y|max)``
(``tests/test_gpu_unet.py``).  (b) - (d) a pullback: ``max(4 e_ref, 1e-4)`` relative to the largest magnitude of the fp64
result, where ``e_ref`` is what the ORACLE's own fp32 autograd loses against fp64 on the same quantity (measured here on the
CPU, never from the code under test); the factor 4 covers a different summation order in two chained passes; 1e-4 is the
relative tolerance the forward test applies to the same fixture.
"""

import pytest
import torch

from conftest import max_err
from oracle import nets, synth

pytestmark = pytest.mark.gpu

NAMES = ["unet_group", "unet_layer_odd", "unet_rms_nomod"]
FWD_TOL = 1e-4


def build_unet(cfg, **kw):
    from azula_amd.nn import UNet

    return UNet(cfg["in_channels"], cfg["out_channels"], hid_channels=cfg["hid_channels"], hid_blocks=cfg["hid_blocks"],
                norm=cfg["norm"], groups=cfg["groups"], mod_features=cfg["mod_features"], **kw)


def load(golden, name):
    g = golden("g5_" + name)
    cfg = g.meta["cfg"]
    sd = synth.synth_state_dict({k: tuple(v) for k, v in g.meta["shapes"].items()}, g.meta["weight_seed"])
    net = build_unet(cfg)
    net.load_state_dict(sd)
    return g, cfg, sd, net.cuda().eval()


def oracle_vjp(fn, x, v, dtype):
    xx = x.detach().to(dtype).clone().requires_grad_()
    with torch.enable_grad():  # (other test modules switch gradients off for the whole session)
        y = fn(xx)
        return y.detach().double(), torch.autograd.grad(y, xx, v.to(dtype))[0].double()


def rel(a, ref):
    return float((a.double().cpu() - ref).abs().max() / ref.abs().max())


def bound(e_ref):
    return max(4 * e_ref, FWD_TOL)


def net_fn(sd, cfg, mod, dtype):
    sdd = {k: v.to(dtype) for k, v in sd.items()}
    m = None if mod is None else mod.to(dtype)
    return lambda x: nets.unet_forward(sdd, cfg, x, m)


@pytest.mark.parametrize("name", NAMES)
def test_unet_vjp(golden, name):
    g, cfg, sd, net = load(golden, name)
    x = g["x"]
    mod = g["modB"] if "modB" in g else None
    gen = torch.Generator().manual_seed(7)
    v = torch.randn(g["y_modB"].shape, generator=gen)
    u = torch.randn(x.shape, generator=gen)
    xd, md = x.cuda(), None if mod is None else mod.cuda()

    out, pull = net.vjp(xd, md)
    # (a) the forward-keep tape computes what the sampling plan computes
    y_plan = net(xd, md)
    err_a = max_err(out, y_plan)
    scale = max(1.0, g["y_modB"].abs().max().item())
    print(name, "(a) forward-keep vs sampling plan:", err_a, "vs golden:", max_err(out, g["y_modB"]))
    assert err_a < FWD_TOL * scale  # measured <= 2.6e-6 (MI355X)
    assert max_err(out, g["y_modB"]) < FWD_TOL * scale

    # (b) pullback of a random cotangent
    y64, ref = oracle_vjp(net_fn(sd, cfg, mod, torch.float64), x, v, torch.float64)
    _, ref32 = oracle_vjp(net_fn(sd, cfg, mod, torch.float32), x, v, torch.float32)
    e_ref = rel(ref32, ref)
    dx = pull(v.cuda())
    err_b = rel(dx, ref)
    print(name, f"(b) pullback err {err_b:.3e} e_ref {e_ref:.3e}")
    assert dx.shape == x.shape and torch.isfinite(dx).all()
    assert err_b < bound(e_ref)  # measured 5.5e-7 / 7.4e-7 / 3.7e-7 (MI355X)

    # (e) a second pullback after the same forward: same bits
    assert torch.equal(pull(v.cuda()), dx)

    # (c) adjoint identity <J u, v> = <u, J^T v>, J u from the fp64 oracle
    with torch.enable_grad():
        _, ju = torch.func.jvp(net_fn(sd, cfg, mod, torch.float64), (x.double(),), (u.double(),))
    lhs = float((ju * v.double()).sum())
    rhs = float((u.double() * dx.double().cpu()).sum())
    norm = float(ju.norm() * v.double().norm())
    print(name, f"(c) adjoint identity: {lhs:.9e} vs {rhs:.9e} (|Ju||v| = {norm:.3e})")
    assert abs(lhs - rhs) < bound(e_ref) * norm  # measured <= 4e-9 |Ju||v| (MI355X)

    # (d) linearity over the range a cotangent takes: a fixed-scale half-precision launch would lose 1e-6 v and overflow on 1e4 v
    for s in (1e-6, 1e4):
        dxs = pull((v * s).cuda())
        err_d = rel(dxs, ref * s)
        print(name, f"(d) pullback({s:g} v) err {err_d:.3e}")
        assert torch.isfinite(dxs).all()
        assert err_d < bound(e_ref)  # measured <= 6.4e-7 (MI355X)

    # a pullback of an earlier forward is refused once the plan has run again
    net.vjp(xd, md)
    with pytest.raises(RuntimeError, match="earlier vjp"):
        pull(v.cuda())


@pytest.mark.parametrize("name", NAMES)
def test_backward_tape_has_no_fixed_scale_f16x2_launch(golden, name):
    r"""(f) a cotangent has no range: every f16x2 launch on the backward tape takes its activation scale from a measured
    maximum (``AzConvArgs.in_absmax0``), and every tensor it wrote is unbounded."""
    from azula_amd import engine

    g, cfg, sd, net = load(golden, name)
    x = g["x"].cuda()
    rows = 0 if "modB" not in g else g["modB"].shape[0]
    net.vjp(x, g["modB"].cuda() if rows else None)
    plan = net.grad_plan(x.shape[0], x.shape[2], x.shape[3], rows, x.device)
    convs = 0
    for fn, args, op in plan.bwd.ops:
        if op.startswith("az_conv2d"):
            convs += 1
            a = args[0]._obj
            assert not a.in_affine
            if op in engine.H2_NAMES:
                assert a.in_absmax0, f"{op}: fixed-scale f16x2 launch on a cotangent"
    assert convs >= 2 * sum(cfg["hid_blocks"]) * 2
    assert any(op == "az_silu_bwd_f32" for _, _, op in plan.bwd.ops)


@pytest.mark.parametrize("name", NAMES)
def test_unet_block_vjp(golden, name):
    from azula_amd.nn import UNetBlock

    g = golden("g5_" + name)
    cfg = g.meta["cfg"]
    C, D = cfg["hid_channels"][1], cfg["mod_features"]
    torch.manual_seed(11)
    blk = UNetBlock(C, mod_features=D, norm=cfg["norm"], groups=cfg["groups"])
    if D > 0:
        blk.ada_zero[-2].weight.data.mul_(30.0)  # (a, b, c of order 0.3 instead of 0.01: the block is not a near-identity)
    else:
        blk.ada_zero.data.mul_(30.0)
    sd = {k: v.detach().clone() for k, v in blk.state_dict().items()}
    blk = blk.cuda().eval()
    B, H, W = 2, 9, 7
    gen = torch.Generator().manual_seed(12)
    x = torch.randn(B, C, H, W, generator=gen) * 3 + 10.0 * (torch.arange(C) % 3 - 1).float().reshape(1, C, 1, 1)
    mod = torch.randn(B, D, generator=gen) if D > 0 else None
    v = torch.randn(B, C, H, W, generator=gen)

    def fn(dtype):
        sdd = {"b." + k: t.to(dtype) for k, t in sd.items()}
        m = None if mod is None else mod.to(dtype)
        return lambda xx: nets.unet_block(sdd, "b", xx, m, cfg["norm"], cfg["groups"])

    y64, ref = oracle_vjp(fn(torch.float64), x, v, torch.float64)
    _, ref32 = oracle_vjp(fn(torch.float32), x, v, torch.float32)
    e_ref = rel(ref32, ref)
    out, pull = blk.vjp(x.cuda(), None if mod is None else mod.cuda())
    assert max_err(out, y64) < FWD_TOL * max(1.0, y64.abs().max().item())
    assert max_err(out, blk(x.cuda(), None if mod is None else mod.cuda())) < FWD_TOL * max(1.0, y64.abs().max().item())
    dx = pull(v.cuda())
    err = rel(dx, ref)
    print(name, f"block pullback err {err:.3e} e_ref {e_ref:.3e}")
    assert err < bound(e_ref)  # measured <= 3.8e-8 (MI355X)
    assert torch.equal(pull(v.cuda()), dx)
    for s in (1e-6, 1e4):
        assert rel(pull((v * s).cuda()), ref * s) < bound(e_ref)


def test_unet_vjp_full_width():
    r"""The headline channel plan (64, 128, 256 channels, 3 blocks per level, GroupNorm) at 2 x 3 x 64 x 64: finite, and the
    pullback at the same bound against fp64 autograd through the oracle."""
    from azula_amd.nn import UNet

    torch.manual_seed(21)
    cfg = {"hid_channels": [64, 128, 256], "hid_blocks": [3, 3, 3], "norm": "group", "groups": 16}
    net = UNet(3, 3, hid_channels=cfg["hid_channels"], hid_blocks=cfg["hid_blocks"], norm="group", groups=16, mod_features=64)
    for m in net.modules():
        if hasattr(m, "ada_zero") and not isinstance(m.ada_zero, torch.nn.Parameter):
            m.ada_zero[-2].weight.data.mul_(10.0)
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    net = net.cuda().eval()
    gen = torch.Generator().manual_seed(22)
    x = torch.randn(2, 3, 64, 64, generator=gen)
    mod = torch.randn(2, 64, generator=gen)
    v = torch.randn(2, 3, 64, 64, generator=gen)
    _, ref = oracle_vjp(net_fn(sd, cfg, mod, torch.float64), x, v, torch.float64)
    _, ref32 = oracle_vjp(net_fn(sd, cfg, mod, torch.float32), x, v, torch.float32)
    e_ref = rel(ref32, ref)
    out, pull = net.vjp(x.cuda(), mod.cuda())
    dx = pull(v.cuda())
    assert torch.isfinite(out).all() and torch.isfinite(dx).all()
    err = rel(dx, ref)
    print(f"full-width pullback err {err:.3e} e_ref {e_ref:.3e}")
    assert err < bound(e_ref)  # measured 4.9e-7 (MI355X)
    assert max_err(out, net(x.cuda(), mod.cuda())) < FWD_TOL * max(1.0, out.abs().max().item())


def test_vjp_scope_errors():
    from azula_amd.nn import UNet

    x = torch.zeros(1, 2, 8, 8, device="cuda")
    with pytest.raises(NotImplementedError):
        UNet(2, 2, hid_channels=(8,), hid_blocks=(1,), periodic=True).cuda().vjp(x)
    with pytest.raises(NotImplementedError):
        UNet(1, 2, cond_channels=1, hid_channels=(8,), hid_blocks=(1,)).cuda().vjp(x[:, :1])
    with pytest.raises(NotImplementedError):
        UNet(2, 2, hid_channels=(8,), hid_blocks=(1,), spatial=3).cuda().vjp(x[:, :, None])
