r"""The normalisation kernels (csrc/norm.hip) and the GroupNorm moments the convolutions leave, against a float64 reference on
inputs chosen for what their algorithm finds hard: mean / std up to 1e5, variance exactly 0 or far below eps, chunk means far
apart, a spike on the statistics threads' pivots, up to 512 pixel chunks per group (every part of the finalize kernel), every
form of the row norm on both sides of its limits.  Families, references, the bound and the case lists live in
tests/norm_cases.py; test_norm_cases_host.py asserts on the CPU that each case reaches the branch it is for and that the bound
can fail.

Nothing is compared with a kernel's own output.  Every case asserts, per element,

    |out - ref| <= M 2^-24 cond  (+ half an ulp of a 2-byte output),   M = 4 M_REF = norm_cases.M_DEVICE

(norm_cases has the derivation), finite outputs, pad channels exactly 0 and a second run of the tape bit-equal to the first.
Each case prints entry point, family, shape, ``err``, the worst ratio err / (2^-24 cond) and M; DESIGN.md (section 4) holds the
largest ratio per entry point."""

import math

import pytest
import torch

import norm_cases as nc

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


def nhwc(x, H, W, cs, dtype=torch.float32):
    r"""(B, C, HW) -> flat (B, H, W, cs) on the device, pad channels 0."""
    B, C, _ = x.shape
    y = torch.zeros(B, H, W, cs, dtype=dtype)
    y[..., :C] = x.reshape(B, C, H, W).permute(0, 2, 3, 1).to(dtype)
    return y.reshape(-1).cuda()


def read(act, C):
    r"""An Act -> (B, C, HW) float64 on the CPU, after checking its pad channels."""
    t = act.buf[: act.B * act.H * act.W * act.cs].reshape(act.B, act.H * act.W, act.cs)
    assert bool((t[..., C:] == 0).all()), "pad channels"
    return t[..., :C].permute(0, 2, 1).double().cpu()


def check(tag, entry, got, ref, unit, out_dtype=None):
    assert got.shape == ref.shape and bool(torch.isfinite(got).all()), (tag, entry, "not finite")
    ratio, err = nc.worst_ratio(got, ref, unit, out_dtype)
    print(f"NORM {entry} {tag}: err {err:.3e} ratio {ratio:.2f} M {nc.M_DEVICE:.0f}")
    assert ratio <= nc.M_DEVICE, (tag, entry, err, ratio)
    return ratio


def run_twice(bld, out, C):
    bld.tape.run()
    torch.cuda.synchronize()
    got = read(out, C)
    raw = out.buf.clone()
    bld.tape.run()
    torch.cuda.synchronize()
    assert torch.equal(out.buf, raw), "a second run of the tape differs"
    return got


def modulation(scale, shift, cs, off=0):
    r"""[scale | shift] rows as the networks hold them: one (B, 2 cs + 4) tensor, the rows ``off`` floats past a 16-byte boundary."""
    if scale is None:
        return dict()
    B, C = scale.shape
    ab = torch.zeros(B, 2 * cs + 4, device="cuda")
    ab[:, off : off + C], ab[:, cs + off : cs + off + C] = scale.cuda(), shift.cuda()
    return dict(scale=ab, shift=ab, scale_off=off, shift_off=cs + off, bstride=2 * cs + 4)


# ------------------------------------------------------------------------------------------------ GroupNorm, separate statistics
@pytest.mark.parametrize("case", nc.GN_CASES, ids=nc.case_id)
def test_groupnorm_separate_pass(case):
    """az_groupnorm_stats_f32 / _h16 (vector and generic form, one and two sources, 1 to 512 chunks, ragged and empty chunks),
    az_groupnorm_finalize_f32 on its own partials (every part of its item loop, groups of up to 256 channels) and the four apply
    kernels, fp32 and 2-byte."""
    from azula_amd.engine import Act, Builder

    c = case
    inp = nc.gn_inputs(c)
    ref, unit = nc.groupnorm_ref(inp["x"], **nc.gn_kwargs(c, inp))
    c0 = c.C - c.c1
    if c.half is None and c.cs != nc.pad4(c.C):
        # an fp32 tensor on a stride of 8: what a half-activation plan holds at its fp32 ends (Builder.new_act(f32=True)); the
        # builder must own the stride, because group_norm gives the output the plan's stride for C
        bld = Builder(torch.device("cuda"), half=torch.bfloat16, half_act=True)
        xa = bld.new_act(c.B, c.H, c.W, c.C, pinned=True, f32=True)
        assert xa.cs == c.cs and not xa.half and not c.c1
        xa.buf.copy_(nhwc(inp["x"], c.H, c.W, c.cs))
        xb = None
    elif c.half is None:
        bld = Builder(torch.device("cuda"))
        cs0 = c.cs - c.c1
        xa = Act(nhwc(inp["x"][:, :c0], c.H, c.W, cs0), c.B, c.H, c.W, c0, cs0, True)
        xb = Act(nhwc(inp["x"][:, c0:], c.H, c.W, c.c1), c.B, c.H, c.W, c.c1, c.c1, True) if c.c1 else None
    else:
        bld = Builder(torch.device("cuda"), half=c.half, half_act=True)
        xa = bld.new_act(c.B, c.H, c.W, c0, pinned=True)
        xa.buf.copy_(nhwc(inp["x"][:, :c0], c.H, c.W, xa.cs, c.half))
        xb = None
        if c.c1:
            xb = bld.new_act(c.B, c.H, c.W, c.c1, pinned=True)
            xb.buf.copy_(nhwc(inp["x"][:, c0:], c.H, c.W, xb.cs, c.half))
    dev = lambda t: None if t is None else t.cuda()  # noqa: E731
    y = bld.group_norm(xa, c.groups, weight=dev(inp["weight"]), bias=dev(inp["bias"]), act=c.act, pool=c.pool, x1=xb,
                       **modulation(inp["scale"], inp["shift"], c.cs))
    sfx = "_f32" if c.half is None else "_h16"
    names = [n for _, _, n in bld.tape.ops]
    assert names == ["az_groupnorm_stats" + sfx, "az_groupnorm_finalize_f32", "az_affine_act" + sfx], names
    assert y.cs == c.cs and y.buf.numel() >= y.B * y.H * y.W * y.cs
    got = run_twice(bld, y, c.C)
    check(nc.case_id(c), names[0] + "+" + names[2], got, ref, unit, c.half)


# ------------------------------------------------------------------------------------------------ moments from the producers
PRODUCERS = {  # producer -> (B, Cin, Cout, H, W, ks, Builder.conv(winograd=...), split-K expected)
    "stem": (2, 3, 128, 24, 40, 3, None, False),
    "wino": (2, 16, 128, 32, 16, 3, True, False),
    "wx3": (2, 16, 128, 32, 16, 3, "wx3", False),
    "wh2": (2, 16, 128, 32, 16, 3, "wh2", False),
    "splitk_direct": (2, 256, 128, 8, 8, 3, False, True),
    "splitk_wino": (4, 256, 256, 16, 16, 3, True, True),
    "wino_128items": (1, 16, 256, 64, 64, 3, "wx3", False),   # 16 tile blocks x 8 quads per group
    "wino_512items": (1, 16, 256, 128, 128, 3, True, False),  # 64 tile blocks x 8 quads: the finalize loop from item 256 on
    "wh2_512items": (1, 16, 256, 128, 128, 3, "wh2", False),
}
ENTRY_OF = {None: "az_conv2d_stem_f32", True: "az_conv2d_winograd_f32", "wx3": "az_conv2d_winograd_x3_f32",
            "wh2": "az_conv2d_winograd_f16x2_f32", False: "az_conv2d_f32"}
STEERS = ("bias30", "bias1e3", "res50", "zero_group", "silu_neg30")
PRODUCER_CASES = [(p, s) for p in PRODUCERS for s in STEERS
                  if not (p == "stem" and s in ("res50", "silu_neg30")) and not (p.endswith("items") and s not in ("bias30", "zero_group"))]


@pytest.mark.parametrize("producer,steer", PRODUCER_CASES)
def test_groupnorm_on_producer_moments(producer, steer):
    """az_groupnorm_finalize_f32 on the (n, mean, M2) records of every kernel that writes AzConvArgs.gn_quads -- the stem's
    direct-tap epilogue, the F(2x2) epilogue, the piece forms' epilogue (wino_x3.hip), the split-K combine behind the direct and
    behind the Winograd kernel -- with the output distribution steered through bias, residual and weights: mean / std 30 to 1e3, a
    group of zero weights and a constant bias (variance exactly 0: the producers do not clamp s2 - s1^2 / n), a group at -30 under
    SiLU (values ~1e-12, far below sqrt(eps)), 2 to 512 records per group.  The reference is the float64 GroupNorm of the
    convolution output the device stored, so the convolution's own rounding is not charged to the norm."""
    from azula_amd.engine import Act, Builder

    B, Cin, Cout, H, W, ks, mode, splitk = PRODUCERS[producer]
    groups = 8
    Cg = Cout // groups
    g = torch.Generator().manual_seed(len(producer) * 7 + len(steer))
    x = torch.randn(B, Cin, H * W, generator=g)
    w = torch.randn(Cout, Cin, ks, ks, generator=g) / math.sqrt(ks * ks * Cin)
    b = torch.randn(Cout, generator=g)
    gate = res = None
    act = 0
    if steer == "bias30":
        b += 30.0
    elif steer == "bias1e3":
        b += 1e3
    elif steer == "res50":
        b += 30.0
        gate = torch.randn(B, Cout, generator=g)
        res = torch.randn(B, Cout, H * W, generator=g) * 0.5 + 50.0
    elif steer == "zero_group":
        w[:Cg] = 0.0
        b[:Cg] = 7.5
    elif steer == "silu_neg30":
        act = 1
        b[Cg : 2 * Cg] -= 30.0
    gw, gb = 1.0 + 0.5 * torch.randn(Cout, generator=g), torch.randn(Cout, generator=g)

    bld = Builder(torch.device("cuda"))
    packed = bld.pack_conv(w.cuda(), b.cuda())
    if producer == "stem":
        y = bld.conv_stem(x.reshape(B, Cin, H, W).cuda().contiguous(), B, Cin, H, W, packed, Cout, gn_stats=True)
    else:
        xa = Act(nhwc(x, H, W, Cin), B, H, W, Cin, Cin, True)
        kw = {}
        if res is not None:
            kw = dict(gate=gate.cuda(), gate_bstride=Cout, res=Act(nhwc(res, H, W, Cout), B, H, W, Cout, Cout, True))
        y = bld.conv(xa, packed, Cout, act=act, winograd=mode, gn_stats=True, **kw)
    assert y.gn_quads is not None, "the producer left no moments"
    n = bld.group_norm(y, groups, weight=gw.cuda(), bias=gb.cuda(), act=1)
    bld.finish()
    names = [nm for _, _, nm in bld.tape.ops]
    conv = [a[0]._obj for _, a, nm in bld.tape.ops if nm.startswith("az_conv2d")][0]
    assert names[0] == ENTRY_OF[mode] and "az_groupnorm_stats_f32" not in names, names
    assert (conv.splitk > 1) == splitk, conv.splitk
    kind = "stem" if producer == "stem" else ("combine" if splitk else "wino")
    assert y.gn_quads[1] == nc.fused_chunks(kind, H, W, Cout)
    items = nc.finalize_items(y.gn_quads[1], Cg // 4)
    if producer.endswith("items"):
        assert nc.finalize_branch(items) == ("gt256" if "512" in producer else "le256"), items
    got = run_twice(bld, n, Cout)
    stored = read(y, Cout).float()
    if steer == "zero_group":
        assert bool((stored[:, :Cg] == 7.5).all())
    if steer == "silu_neg30":
        assert stored[:, Cg : 2 * Cg].abs().max().item() < 1e-9
    ref, unit = nc.groupnorm_ref(stored, groups, H, W, weight=gw, bias=gb, act=1)
    check(f"{producer} {steer} items {items}", names[0] + ("+combine" if splitk else "") + "+az_groupnorm_finalize_f32", got, ref, unit)


# ------------------------------------------------------------------------------------------------ row norms
@pytest.mark.parametrize("case", nc.ROW_CASES, ids=nc.case_id)
def test_rownorm(case):
    """az_rownorm_mod_f32 (register form up to 2048, looping vector form beyond it and under misaligned modulation rows, scalar
    form with pad channels, the grid-stride loop over 18000 rows of three samples) and az_rownorm_mod_h16, LayerNorm and RMSNorm,
    with and without ``weight`` and modulation."""
    from azula_amd.engine import Act, Builder

    c = case
    inp = nc.row_inputs(c)
    ref, unit = nc.rownorm_ref(inp["x"], c.kind, weight=inp["weight"], scale=inp["scale"], shift=inp["shift"], rows_per_batch=c.rpb)
    rows = c.B * c.rpb
    x3 = inp["x"].reshape(c.B, c.rpb, c.C).permute(0, 2, 1)  # (B, C, HW)
    if c.half is None:
        bld = Builder(torch.device("cuda"))
        xa = Act(nhwc(x3, c.rpb, 1, c.cs), c.B, c.rpb, 1, c.C, c.cs, True)
    else:
        bld = Builder(torch.device("cuda"), half=c.half, half_act=True)
        xa = bld.new_act(c.B, c.rpb, 1, c.C, pinned=True)
        assert xa.cs == c.cs
        xa.buf.copy_(nhwc(x3, c.rpb, 1, c.cs, c.half))
    y = bld.row_norm(xa, c.kind, weight=None if inp["weight"] is None else inp["weight"].cuda(),
                     **modulation(inp["scale"], inp["shift"], c.cs, off=1 if c.mod == 2 else 0))
    entry = "az_rownorm_mod_f32" if c.half is None else "az_rownorm_mod_h16"
    assert [n for _, _, n in bld.tape.ops] == [entry] and y.cs == c.cs
    got = run_twice(bld, y, c.C).permute(0, 2, 1).reshape(rows, c.C)
    if c.family == "zero_row":  # the output is exactly the shift
        want = torch.zeros(rows, c.C, dtype=torch.float64) if inp["shift"] is None else nc.round_to(inp["shift"], c.half).double()[
            torch.arange(rows) // c.rpb]
        assert torch.equal(got, want)
    check(nc.case_id(c), entry, got, ref, unit, c.half)
