r"""``MultiheadSelfAttention.vjp``, ``DiTBlock.vjp`` and ``DiT.vjp`` (HIP forward-keep + backward tapes on the attention backward
kernels) against fp64 autograd through the oracle (``oracle.nets.msa_forward`` / ``dit_block`` / ``dit_forward``).

Bounds, as in ``test_gpu_unet_vjp.py``.  The forward of a gradient plan: ``1e-4 * max(1, |y|max)`` against the sampling plan and
against the oracle.  A pullback: ``max(4 e_ref, 1e-4)`` relative to the largest magnitude of the fp64 result, ``e_ref`` being what
the ORACLE's own fp32 autograd loses against fp64 on the same quantity (measured here on the CPU, never from the code under test).
"""

import pytest
import torch
from torch.nn.attention import SDPBackend, sdpa_kernel

from conftest import max_err
from oracle import nets, synth

pytestmark = pytest.mark.gpu

FWD_TOL = 1e-4


def oracle_vjp(fn, x, v, dtype):
    xx = x.detach().to(dtype).clone().requires_grad_()
    with torch.enable_grad():  # (other test modules switch gradients off for the whole session)
        y = fn(xx)
        return y.detach().double(), torch.autograd.grad(y, xx, v.to(dtype))[0].double()


def rel(a, ref):
    return float((a.double().cpu() - ref).abs().max() / ref.abs().max())


def bound(e_ref):
    return max(4 * e_ref, FWD_TOL)


def check_vjp(label, vjp, forward, fn, x, seed, stale=True):
    r"""(a) - (e) of ``test_gpu_unet_vjp.py`` for one module.  ``vjp()`` / ``forward()`` run the module on the device,
    ``fn(dtype)`` is the oracle as a function of x."""
    out, pull = vjp()
    gen = torch.Generator().manual_seed(seed)
    v = torch.randn(out.shape, generator=gen)
    u = torch.randn(x.shape, generator=gen)
    y64, ref = oracle_vjp(fn(torch.float64), x, v, torch.float64)
    _, ref32 = oracle_vjp(fn(torch.float32), x, v, torch.float32)
    e_ref = rel(ref32, ref)
    # (a) the forward-keep tape computes what the sampling plan and the oracle compute
    scale = max(1.0, y64.abs().max().item())
    err_plan, err_orc = max_err(out, forward()), max_err(out, y64)
    print(label, f"(a) forward-keep vs sampling plan {err_plan:.3e}, vs oracle {err_orc:.3e} (|y|max {scale:.3g})")
    # measured (MI355X): <= 2.9e-6 against the plan, <= 1.5e-5 against the oracle (at |y|max 25)
    assert err_plan < FWD_TOL * scale and err_orc < FWD_TOL * scale
    # (b) pullback of a random cotangent
    dx = pull(v.cuda())
    err_b = rel(dx, ref)
    print(label, f"(b) pullback err {err_b:.3e} e_ref {e_ref:.3e}")
    assert dx.shape == x.shape and torch.isfinite(dx).all()
    assert err_b < bound(e_ref)  # measured (MI355X): msa <= 5.9e-7, block <= 3.9e-8, DiT <= 9.3e-7 (e_ref 9.5e-7)
    # (e) a second pullback after the same forward: the same bits
    assert torch.equal(pull(v.cuda()), dx)
    # (c) adjoint identity <J u, v> = <u, J^T v>, J u from the fp64 oracle
    # (the CPU's fused attention has no forward-mode derivative: the oracle's attention runs as its plain matmul / softmax form here)
    with torch.enable_grad(), sdpa_kernel(SDPBackend.MATH):
        _, ju = torch.func.jvp(fn(torch.float64), (x.double(),), (u.double(),))
    lhs, rhs = float((ju * v.double()).sum()), float((u.double() * dx.double().cpu()).sum())
    norm = float(ju.norm() * v.double().norm())
    print(label, f"(c) adjoint identity: {lhs:.9e} vs {rhs:.9e} (|Ju||v| = {norm:.3e})")
    assert abs(lhs - rhs) < bound(e_ref) * norm  # measured <= 1.3e-7 |Ju||v| (MI355X)
    # (d) linearity over the range a cotangent takes
    for s in (1e-6, 1e4):
        dxs = pull((v * s).cuda())
        err_d = rel(dxs, ref * s)
        print(label, f"(d) pullback({s:g} v) err {err_d:.3e}")
        assert torch.isfinite(dxs).all() and err_d < bound(e_ref)  # measured <= 8.9e-7 (MI355X)
    # a pullback of an earlier forward is refused once the plan has run again
    if stale:
        vjp()
        with pytest.raises(RuntimeError, match="earlier vjp"):
            pull(v.cuda())


GRID = torch.cartesian_prod(torch.arange(3.0), torch.arange(3.0))  # (9, 2) positions


@pytest.mark.parametrize("qk_norm,rope,causal", [(True, False, False), (False, False, False), (True, True, False), (False, True, False),
                                                 (True, False, True), (True, True, True)])
def test_msa_vjp(qk_norm, rope, causal):
    from azula_amd.nn import MultiheadSelfAttention

    torch.manual_seed(31)
    msa = MultiheadSelfAttention(64, pos_channels=2, attention_heads=4, qk_norm=qk_norm, rope=rope)
    sd = {"m." + k: v.detach().clone() for k, v in msa.state_dict().items()}
    msa = msa.cuda().eval()
    B, L = 2, 9
    x = torch.randn(B, L, 64, generator=torch.Generator().manual_seed(32)) * 2
    pos = GRID if rope else None
    mask = torch.ones(L, L, dtype=torch.bool).tril() if causal else None
    xd = x.cuda()
    pd, md = (None if pos is None else pos.cuda()), (None if mask is None else mask.cuda())

    def fn(dtype):
        sdd = {k: t.to(dtype) for k, t in sd.items()}
        p = None if pos is None else pos.to(dtype)
        return lambda xx: nets.msa_forward(sdd, "m", xx, 4, qk_norm=qk_norm, pos=p, mask=mask)

    check_vjp(f"msa qk_norm={qk_norm} rope={rope} causal={causal}", lambda: msa.vjp(xd, pd, md), lambda: msa(xd, pd, md), fn, x, 33)


@pytest.mark.parametrize("act", ["silu", "relu", "relu2", "swiglu"])
@pytest.mark.parametrize("D", [32, 0])
def test_dit_block_vjp(act, D):
    from azula_amd.nn import DiTBlock

    torch.manual_seed(41)
    blk = DiTBlock(64, mod_features=D, ffn_activation=act, attention_heads=4)
    if D > 0:
        blk.ada_zero[-2].weight.data.mul_(30.0)  # (a, b, c of order 0.3 instead of 0.01: the block is not a near-identity)
    else:
        blk.ada_zero.data.mul_(30.0)
    sd = {"b." + k: v.detach().clone() for k, v in blk.state_dict().items()}
    blk = blk.cuda().eval()
    B, L = 2, 9
    gen = torch.Generator().manual_seed(42)
    x = torch.randn(B, L, 64, generator=gen) * 3 + (torch.arange(64) % 3 - 1).float()
    mod = torch.randn(B, D, generator=gen) if D > 0 else None
    xd, md = x.cuda(), None if mod is None else mod.cuda()

    def fn(dtype):
        sdd = {k: t.to(dtype) for k, t in sd.items()}
        m = None if mod is None else mod.to(dtype)
        return lambda xx: nets.dit_block(sdd, "b", xx, m, 4, act=act)

    check_vjp(f"block {act} D={D}", lambda: blk.vjp(xd, md), lambda: blk(xd, md), fn, x, 43)


DIT_FIXTURES = ["g5_vit", "g5_vit_rope_swiglu", "g5_vit_relu2_noqknorm", "g24_vit_hd24"]
POS44 = torch.cartesian_prod(torch.arange(4.0), torch.arange(4.0))  # the 4 x 4 patch grid of the fixtures


def load_dit(golden, name):
    from azula_amd.nn import DiT

    g = golden(name)
    cfg = g.meta["cfg"]
    extra = {k: cfg[k] for k in ("rope", "ffn_activation", "qk_norm") if k in cfg}
    net = DiT(16, 16, pos_channels=2, mod_features=cfg["mod_features"], hid_channels=cfg["hid_channels"], hid_blocks=cfg["hid_blocks"],
              attention_heads=cfg["attention_heads"], **extra)
    shapes = {k: tuple(v) for k, v in g.meta["shapes"].items()}
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == shapes
    sd = synth.synth_state_dict(shapes, g.meta["weight_seed"])
    net.load_state_dict(sd)
    return g, cfg, sd, net.cuda().eval()


def dit_fn(sd, cfg, mod, pos):
    def fn(dtype):
        sdd = {k: t.to(dtype) for k, t in sd.items()}
        return lambda xx: nets.dit_forward(sdd, cfg, xx, mod.to(dtype), pos=pos.to(dtype))

    return fn


@pytest.mark.parametrize("name", DIT_FIXTURES)
def test_dit_vjp(golden, name):
    g, cfg, sd, net = load_dit(golden, name)
    gen = torch.Generator().manual_seed(51)
    x = torch.randn(2, 16, 16, generator=gen)
    mod = g["modB"]
    xd, md, pd = x.cuda(), mod.cuda(), POS44.cuda()
    check_vjp(name, lambda: net.vjp(xd, md, pd), lambda: net(xd, md, pd), dit_fn(sd, cfg, mod, POS44), x, 52)
    plan = next(p for k, p in net._plans.items() if k[0] == "vjp")
    assert plan.saved_bytes > 0


def test_backward_tape_has_no_fixed_scale_f16x2_launch(golden):
    r"""A cotangent has no range: every f16x2 GEMM of the backward tape takes its activation scale from a measured maximum
    (``AzConvArgs.in_absmax0``), and the attention gradient is the fp32 kernel."""
    from azula_amd import engine

    g, cfg, sd, net = load_dit(golden, "g5_vit")
    net.vjp(torch.zeros(2, 16, 16, device="cuda"), g["modB"].cuda(), POS44.cuda())
    plan = next(p for k, p in net._plans.items() if k[0] == "vjp")
    ops = [op for _, _, op in plan.bwd.ops]
    convs = 0
    for fn, args, op in plan.bwd.ops:
        if op.startswith("az_conv2d"):
            convs += 1
            a = args[0]._obj
            assert not a.in_affine
            if op in engine.H2_NAMES:
                assert a.in_absmax0, f"{op}: fixed-scale f16x2 launch on a cotangent"
    assert convs == 2 + 4 * cfg["hid_blocks"]
    assert ops.count("az_attention_bwd_f32") == cfg["hid_blocks"] and ops.count("az_qk_prep_bwd_f32") == cfg["hid_blocks"]
    assert ops.count("az_rownorm_bwd_f32") == cfg["hid_blocks"] and "az_act_bwd_f32" in ops
    assert not any(op.startswith("az_attention") and op != "az_attention_bwd_f32" for op in ops)


def test_dit_vjp_dit_b_width():
    r"""A DiT-B-shaped width (768 channels, 12 heads of 64, 2 blocks) at B = 2, L = 256: finite, and the pullback at the same
    bound against fp64 autograd through the oracle."""
    from azula_amd.nn import DiT

    torch.manual_seed(61)
    cfg = {"hid_channels": 768, "hid_blocks": 2, "attention_heads": 12}
    net = DiT(16, 16, mod_features=64, hid_channels=768, hid_blocks=2, attention_heads=12)
    for blk in net.blocks:
        blk.ada_zero[-2].weight.data.mul_(10.0)
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    net = net.cuda().eval()
    gen = torch.Generator().manual_seed(62)
    x = torch.randn(2, 256, 16, generator=gen)
    mod = torch.randn(2, 64, generator=gen)
    v = torch.randn(2, 256, 16, generator=gen)

    def fn(dtype):
        sdd = {k: t.to(dtype) for k, t in sd.items()}
        return lambda xx: nets.dit_forward(sdd, cfg, xx, mod.to(dtype))

    _, ref = oracle_vjp(fn(torch.float64), x, v, torch.float64)
    _, ref32 = oracle_vjp(fn(torch.float32), x, v, torch.float32)
    e_ref = rel(ref32, ref)
    out, pull = net.vjp(x.cuda(), mod.cuda())
    dx = pull(v.cuda())
    assert torch.isfinite(out).all() and torch.isfinite(dx).all()
    err = rel(dx, ref)
    print(f"DiT-B width pullback err {err:.3e} e_ref {e_ref:.3e}")
    assert err < bound(e_ref)  # measured 4.1e-7, e_ref 2.6e-7 (MI355X)
    assert max_err(out, net(x.cuda(), mod.cuda())) < FWD_TOL * max(1.0, out.abs().max().item())


def test_vjp_scope_errors():
    from azula_amd.nn import DiT, ViT

    x = torch.zeros(1, 4, 8, device="cuda")
    kw = dict(hid_channels=32, hid_blocks=1, attention_heads=2)
    with pytest.raises(NotImplementedError):
        DiT(8, 8, **kw).cuda().bfloat16().vjp(x)
    with pytest.raises(NotImplementedError):
        DiT(8, 8, **kw).cuda().vjp(x.half())
    with pytest.raises(NotImplementedError):
        DiT(4, 8, cond_channels=4, **kw).cuda().vjp(x[..., :4], cond=x[..., 4:])
    with pytest.raises(NotImplementedError):
        DiT(8, 8, hid_channels=256, hid_blocks=1, attention_heads=1).cuda().vjp(x)  # head size 256
    assert ViT(4, 4, hid_channels=32, hid_blocks=1, attention_heads=2, patch_size=2).vjp is None
    net = DiT(8, 8, **kw).cuda()
    y = net(x)  # the forward is unaffected
    out, _ = net.vjp(x)
    assert max_err(out, y) < FWD_TOL
