r"""``azula_amd.plan.ForwardPlan``: what every backbone's forward plan shares -- the input in its four layouts (planar latent,
channel-padded NHWC, pinned tokens, the NCHW buffer of a patchify launch), the modulation buffer and front, ``run`` and
``program``.  The smallest networks that reach each form: a 3-channel U-Net at 16 x 16 (planar; NHWC with the planar stem
switched off, 3 channels in a stride of 4), a 6-channel U-Net block (NHWC in a pool activation, stride 8), a DiT block on 60
channels (tokens; 60 is a multiple of the fp32 stride unit of 4, so this input has no pad lanes), a DiT on 6-channel tokens (stride 8:
the pad lanes of the token form) and a patch-4 ViT (NCHW).  Every comparison is of bits: a plan that runs twice launches the same
kernels on the same arguments as a fresh plan of the same weights."""

import gc
import weakref

import pytest
import torch

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

B, D = 2, 16


def _unet(mod_features=D):
    from azula_amd.nn import UNet

    return UNet(3, 3, hid_channels=(8, 16), hid_blocks=(1, 1), norm="group", groups=4, mod_features=mod_features)


def _block():
    from azula_amd.nn import UNetBlock

    return UNetBlock(6, mod_features=D, norm="layer")


def _dit_block():
    from azula_amd.nn import DiTBlock

    return DiTBlock(60, mod_features=32, ffn_factor=3, ffn_activation="swiglu", attention_heads=3)


def _dit():
    from azula_amd.nn import DiT

    return DiT(6, 6, mod_features=D, hid_channels=64, hid_blocks=1, attention_heads=4)


def _vit():
    from azula_amd.nn import ViT

    return ViT(3, 3, hid_channels=64, hid_blocks=1, attention_heads=4, patch_size=4, mod_features=D)


# form -> (constructor, input shape, modulation features, the plan's input form)
FORMS = {
    "planar": (_unet, (B, 3, 16, 16), D, "planar"),
    "nhwc": (_unet, (B, 3, 16, 16), D, "nhwc"),
    "nhwc_pool": (_block, (B, 6, 12, 12), D, "nhwc"),
    "tokens": (_dit_block, (B, 9, 60), 32, "tokens"),
    "tokens_padded": (_dit, (B, 9, 6), D, "tokens"),
    "nchw": (_vit, (B, 3, 16, 16), D, "nchw"),
}


@pytest.fixture(params=list(FORMS))
def form(request, monkeypatch):
    r"""(make: a network with the same weights each call, inputs: n -> (x, mod)) for one input form."""
    from azula_amd import engine

    name = request.param
    ctor, shape, feats, kind = FORMS[name]
    if name == "nhwc":
        monkeypatch.setattr(engine, "STEM_PLANAR", False)

    def make():
        torch.manual_seed(5)
        return ctor().cuda().eval()

    def inputs(n: int):
        g = torch.Generator().manual_seed(100 + n)
        return torch.randn(shape, generator=g).cuda(), torch.randn(B, feats, generator=g).cuda()

    return name, kind, make, inputs


def _plan(net):
    (plan,) = net._plans.values()
    return plan


def test_second_run_equals_a_fresh_plan(form):
    r"""No state survives a run: pad lanes, modulation rows and activations of the first input leave no trace in the second."""
    name, kind, make, inputs = form
    (x1, m1), (x2, m2) = inputs(1), inputs(2)
    net = make()
    y1 = net(x1, m1)
    plan = _plan(net)
    assert plan._form == kind and plan.planar == (name == "planar")
    if kind in ("nhwc", "tokens"):  # (padded inputs: 3 -> 4, 6 -> 8; 60 channels fill their stride)
        assert (plan.x_in.C, plan.x_in.cs) == {"nhwc": (3, 4), "nhwc_pool": (6, 8), "tokens": (60, 60), "tokens_padded": (6, 8)}[name]
    y2 = net(x2, m2)
    assert _plan(net) is plan, "the second call built another plan"
    fresh = make()(x2, m2)
    assert torch.isfinite(y2).all() and not torch.equal(y1, y2)
    assert torch.equal(y2, fresh)


def test_result_is_the_callers_own(form):
    _, _, make, inputs = form
    x, m = inputs(3)
    net = make()
    y1 = net(x, m)
    want = y1.clone()
    y1.fill_(float("nan"))
    y2 = net(x, m)
    assert y2.data_ptr() != y1.data_ptr() and torch.equal(y2, want)


def test_modulation_rows_and_front():
    r"""``mod`` (D) -> one row, (B, D) -> B rows, the same function of each row; the front is two launches ahead of the walk, and
    a network without modulation has none."""
    x = torch.randn(B, 3, 16, 16, generator=torch.Generator().manual_seed(7)).cuda()
    mod = torch.randn(D, generator=torch.Generator().manual_seed(8)).cuda()
    torch.manual_seed(5)
    net = _unet().cuda().eval()
    y_shared = net(x, mod)
    y_rows = net(x, mod.expand(B, D).contiguous())
    one, per = net._plans.values()
    assert (one.mod_rows, tuple(one.mod.shape)) == (1, (1, D)) and (per.mod_rows, tuple(per.mod.shape)) == (B, (B, D))
    # the same arithmetic per row in another launch shape: fp32 rounding of sums of a few hundred O(1) terms, far below 1e-4
    assert (y_shared - y_rows).abs().max().item() <= 1e-4 * max(1.0, y_shared.abs().max().item())
    for plan in (one, per):
        assert [n for _, _, n in plan.tape.ops[:2]] == ["az_linear_small_f32", "az_linear_small_grouped_f32"]
        assert len(plan.mod_jobs) == 4 and len(plan.tape) == len(plan.bld.tape) + 2
    torch.manual_seed(5)
    bare = _unet(mod_features=0).cuda().eval()
    bare(x)
    plan = _plan(bare)
    assert plan.mod_rows == 0 and plan.mod_jobs == [] and plan.tape is plan.bld.tape  # (nothing prepended)
    assert not any(n.startswith("az_linear_small") for _, _, n in plan.tape.ops)
    assert len(plan.tape) == len(one.tape) - 2  # (the same walk without its front)


@pytest.mark.parametrize("name", ["planar", "nhwc", "nchw"])
def test_program_leaves_the_plan_alone(name, monkeypatch):
    from azula_amd import engine

    if name == "nhwc":
        monkeypatch.setattr(engine, "STEM_PLANAR", False)
    device = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(5)
    if name == "nchw":
        net = _vit().cuda().eval()
        plan = net._vit_plan(B, 16, 16, 1, device)
        x_in = plan.x_nchw
    else:
        net = _unet().cuda().eval()
        plan = net.plan(B, 16, 16, 1, device)
        x_in = plan.x_in.buf
    n = len(plan.tape)
    prog = plan.program(3)
    assert prog.tape is not plan.tape and len(prog.tape) == n
    prog.tape.extend(plan.tape)
    assert len(prog.tape) == 2 * n and len(plan.tape) == n
    assert prog.x_in is x_in and prog.out is plan.out and prog.f_channels == 3 and not prog.f_nhwc
    assert prog.x_in_cs == (plan.x_in.cs if name == "nhwc" else 0) and (name != "nhwc" or plan.x_in.cs == 4)
    alive = weakref.ref(plan)
    net._plans.clear()
    del plan
    gc.collect()
    assert alive() is not None, "the program does not keep its plan alive"
    del prog
    gc.collect()
    assert alive() is None
