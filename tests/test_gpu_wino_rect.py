r"""Rectangular tile blocks of the x3 / f16x2 Winograd kernel (csrc/wino_x3.hip: RECT) against the run form of the same kernel.

Only the staging geometry differs between the two forms: every output accumulates the same products in the same order, so the
outputs must be BIT-EQUAL; a GroupNorm record covers a rectangle instead of a run, so the normalised outputs agree at the bound of
the moments tests (tests/test_gpu_kernels.py::test_groupnorm_statistics_from_the_conv_epilogue).  The form is forced per launch
with AZ_X3_BLOCK="w,h" (honoured under AZ_DEBUG_AB; "64,1" = the run form); one layer is also held against fp64 at the bound of
test_conv2d_x3_accuracy, so that both forms being wrong together is not a pass."""

import math

import pytest
import torch
import torch.nn.functional as F

from conftest import max_err

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

NAME = {"wx3": "az_conv2d_winograd_x3_f32", "wh2": "az_conv2d_winograd_f16x2_f32"}
RECTS = ["32,2", "16,4", "8,8", "4,16"]


@pytest.fixture(scope="module")
def az():
    from azula_amd import _lib

    _lib.lib()
    return _lib


def dev(t):
    return t.to("cuda").contiguous()


def to_nhwc(x, cs=None):
    B, Cc, H, W = x.shape
    cs = cs or (Cc + 3) // 4 * 4
    y = torch.zeros(B, H, W, cs, dtype=x.dtype, device=x.device)
    y[..., :Cc] = x.permute(0, 2, 3, 1)
    return y.contiguous()


def from_nhwc(y, Cc):
    return y[..., :Cc].permute(0, 3, 1, 2).contiguous()


def run_forms(monkeypatch, bld, outs, forms):
    r"""Runs the finished tape once per block form; the outputs are poisoned in between so that a launch that writes nothing shows."""
    monkeypatch.setenv("AZ_DEBUG_AB", "1")  # (A/B overrides are honoured only under the debug switch)
    res = {}
    for form in forms:
        monkeypatch.setenv("AZ_X3_BLOCK", form)
        for o in outs:
            o.buf.fill_(float("nan"))
        bld.tape.run()
        torch.cuda.synchronize()
        res[form] = [o.buf.clone() for o in outs]
    return res


def assert_bit_equal(res, what=""):
    ref = res["64,1"]
    for form, got in res.items():
        for r, g in zip(ref, got):
            assert torch.isfinite(r).all(), (what, "run form left non-finite values")
            assert torch.equal(r, g), (what, form, (r - g).abs().max().item())


def layer(B, H, W, C0, Cout, *, C1=0, up1=0, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + 7 * C0 + Cout + H)
    x0 = torch.randn(B, C0, H, W, generator=g)
    x1 = torch.randn(B, C1, (H + (1 << up1) - 1) >> up1, (W + (1 << up1) - 1) >> up1, generator=g) if C1 else None
    w = torch.randn(Cout, C0 + C1, 3, 3, generator=g) / math.sqrt(9 * (C0 + C1))
    b = torch.randn(Cout, generator=g)
    return g, x0, x1, w, b


def act_of(x):
    from azula_amd.engine import Act

    B, Cc, H, W = x.shape
    return Act(to_nhwc(dev(x)).reshape(-1), B, H, W, Cc, (Cc + 3) // 4 * 4, True)


def the_conv(bld, mode):
    convs = [(args[0]._obj, nm) for _, args, nm in bld.tape.ops if nm.startswith("az_conv2d")]
    assert [nm for _, nm in convs] == [NAME[mode]], convs
    return convs[0][0]


def test_the_block_switch_is_live(az, monkeypatch):
    r"""A shape outside the candidate set is refused: the comparisons below really run two different forms."""
    from azula_amd.engine import Builder

    _, x0, _, w, b = layer(1, 16, 16, 16, 64)
    bld = Builder(torch.device("cuda"))
    a0 = act_of(x0)  # (the descriptor holds raw addresses: the sources stay alive here)
    bld.conv(a0, bld.pack_conv(dev(w), dev(b)), 64, winograd="wx3")
    bld.finish()
    monkeypatch.setenv("AZ_DEBUG_AB", "1")
    monkeypatch.setenv("AZ_X3_BLOCK", "8,4")
    with pytest.raises(az.AzulaAmdError):
        bld.tape.run()
    monkeypatch.setenv("AZ_X3_BLOCK", "8,8")
    bld.tape.run()
    torch.cuda.synchronize()


@pytest.mark.parametrize("mode", ["wx3", "wh2"])
@pytest.mark.parametrize(
    "B,H,W,Cin,Cout",
    [
        (1, 16, 16, 16, 64),    # one full 8 x 8 block
        (3, 20, 12, 32, 64),    # 10 x 6 tiles: ragged both ways, an image's tiles never share a block with the next image's
        (2, 6, 6, 16, 64),      # 3 x 3 tiles: narrower than any rectangle
        (2, 34, 18, 24, 128),   # 17 x 9 tiles, Cin 24: the last K step is a channel tail (TAIL); two cout blocks
    ],
)
def test_plain_layers_every_shape(az, monkeypatch, B, H, W, Cin, Cout, mode):
    from azula_amd.engine import Builder

    _, x0, _, w, b = layer(B, H, W, Cin, Cout)
    bld = Builder(torch.device("cuda"))
    a0 = act_of(x0)
    y = bld.conv(a0, bld.pack_conv(dev(w), dev(b)), Cout, winograd=mode)
    bld.finish()
    the_conv(bld, mode)
    res = run_forms(monkeypatch, bld, [y], ["64,1"] + RECTS)
    assert_bit_equal(res, (B, H, W, Cin, Cout))
    ref = F.conv2d(x0, w, b, padding=1)
    out = from_nhwc(res["8,8"][0].reshape(B, H, W, -1), Cout)
    tol = 3 * (3e-6 * math.sqrt(Cin * 9) + 1e-5)  # (tests/test_gpu_kernels.py: conv_tol of the Winograd piece forms)
    assert max_err(out, ref) < tol * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("mode", ["wx3", "wh2"])
@pytest.mark.parametrize("rect", ["8,8", "16,4"])
def test_two_sources_upsampled_with_the_switch_inside_the_k_range(az, monkeypatch, rect, mode):
    r"""32 + 16 channels: K steps 0, 1 gather from source 0, step 2 from source 1 (nearest x 2 upsampled): the offsets parked for
    the second source are the rectangle's too."""
    from azula_amd.engine import Builder

    B, H, W, C0, C1, Cout = 2, 20, 12, 32, 16, 64
    _, x0, x1, w, b = layer(B, H, W, C0, Cout, C1=C1, up1=1)
    bld = Builder(torch.device("cuda"))
    a0, a1 = act_of(x0), act_of(x1)
    y = bld.conv(a0, bld.pack_conv(dev(w), dev(b), cin0=C0), Cout, src1=a1, up1=1, hin=H, win=W, winograd=mode)
    bld.finish()
    res = run_forms(monkeypatch, bld, [y], ["64,1", rect])
    assert_bit_equal(res)
    up = F.interpolate(x1, scale_factor=(2.0, 2.0), mode="nearest")[:, :, :H, :W]
    ref = F.conv2d(torch.cat((x0, up), 1), w, b, padding=1)
    tol = 3 * (3e-6 * math.sqrt((C0 + C1) * 9) + 1e-5)
    assert max_err(from_nhwc(res[rect][0].reshape(B, H, W, -1), Cout), ref) < tol * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("mode", ["wx3", "wh2"])
@pytest.mark.parametrize("rect", ["8,8", "4,16", "32,2"])
def test_circular_padding(az, monkeypatch, rect, mode):
    r"""Odd sizes: the window of a block past the edge wraps on both sides."""
    from azula_amd.engine import Builder

    B, H, W, Cin, Cout = 2, 18, 13, 16, 64
    _, x0, _, w, b = layer(B, H, W, Cin, Cout)
    bld = Builder(torch.device("cuda"))
    a0 = act_of(x0)
    y = bld.conv(a0, bld.pack_conv(dev(w), dev(b)), Cout, winograd=mode, periodic=True)
    bld.finish()
    assert the_conv(bld, mode).pad_mode == 1
    res = run_forms(monkeypatch, bld, [y], ["64,1", rect])
    assert_bit_equal(res)
    ref = F.conv2d(F.pad(x0, (1, 1, 1, 1), mode="circular"), w, b)
    tol = 3 * (3e-6 * math.sqrt(Cin * 9) + 1e-5)
    assert max_err(from_nhwc(res[rect][0].reshape(B, H, W, -1), Cout), ref) < tol * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("mode", ["wx3", "wh2"])
@pytest.mark.parametrize("in_act", [0, 1])
def test_affine_in_the_gather(az, monkeypatch, in_act, mode):
    r"""AzConvArgs.in_affine (AFF = 1 plain, 2 with SiLU): the validity mask that keeps padding at zero comes from the rectangle's
    tile coordinates; ragged 9 x 7 tiles, so masked tiles and edge patches are both there."""
    from azula_amd.engine import Builder

    B, H, W, Cin, Cout = 2, 18, 14, 16, 64
    g, x0, _, w, b = layer(B, H, W, Cin, Cout)
    sc, sh = torch.randn(B, Cin, generator=g), torch.randn(B, Cin, generator=g)
    bld = Builder(torch.device("cuda"))
    xa = act_of(x0)
    xa.affine = (dev(torch.cat((sc.reshape(-1), sh.reshape(-1)))), in_act)
    y = bld.conv(xa, bld.pack_conv(dev(w), dev(b)), Cout, winograd=mode)
    bld.finish()
    assert the_conv(bld, mode).in_affine, "the affine was materialised instead of folded into the gather"
    res = run_forms(monkeypatch, bld, [y], ["64,1", "8,8", "16,4"])
    assert_bit_equal(res)
    xin = x0 * sc[:, :, None, None] + sh[:, :, None, None]
    ref = F.conv2d(F.silu(xin) if in_act else xin, w, b, padding=1)
    tol = 3 * (3e-6 * math.sqrt(Cin * 9) + 1e-5)
    assert max_err(from_nhwc(res["8,8"][0].reshape(B, H, W, -1), Cout), ref) < tol * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("mode", ["wx3", "wh2"])
def test_residual_gate_and_silu_epilogue(az, monkeypatch, mode):
    from azula_amd.engine import Builder

    B, H, W, Cin, Cout = 3, 20, 12, 32, 64
    g, x0, _, w, b = layer(B, H, W, Cin, Cout)
    gate, r = torch.randn(B, Cout, generator=g), torch.randn(B, Cout, H, W, generator=g)
    bld = Builder(torch.device("cuda"))
    a0, ra = act_of(x0), act_of(r)
    y = bld.conv(a0, bld.pack_conv(dev(w), dev(b)), Cout, act=1, gate=dev(gate), gate_bstride=Cout, res=ra, winograd=mode)
    bld.finish()
    res = run_forms(monkeypatch, bld, [y], ["64,1", "8,8", "4,16"])
    assert_bit_equal(res)
    ref = r + gate[:, :, None, None] * F.silu(F.conv2d(x0, w, b, padding=1))
    tol = 3 * (3e-6 * math.sqrt(Cin * 9) + 1e-5)
    assert max_err(from_nhwc(res["8,8"][0].reshape(B, H, W, -1), Cout), ref) < tol * max(1.0, ref.abs().max().item())


def gn_reference(x0, w, b, groups, gw, gb):
    return F.silu(F.group_norm(F.conv2d(x0, w, b, padding=1), groups, gw, gb, eps=1e-5))


@pytest.mark.parametrize("mode", ["wx3", "wh2"])
@pytest.mark.parametrize("B,H,W,Cin,Cout,rects", [(1, 16, 16, 16, 64, ["8,8"]), (2, 32, 16, 16, 128, ["8,8", "4,16"])])
def test_groupnorm_moments_of_whole_rectangles(az, monkeypatch, B, H, W, Cin, Cout, rects, mode):
    r"""gn_quads with splitk 1: a record covers a rectangle (1024 values) instead of a run.  Outputs bit-equal; the normalised
    outputs at the bound of the moments tests (2.5e-5 between two groupings of the same output, 6e-5 against torch; mean >> std)."""
    from azula_amd.engine import Builder

    g, x0, _, w, b = layer(B, H, W, Cin, Cout)
    b = b + 30.0
    gw, gb = torch.randn(Cout, generator=g), torch.randn(Cout, generator=g)
    bld = Builder(torch.device("cuda"))
    a0 = act_of(x0)
    y = bld.conv(a0, bld.pack_conv(dev(w), dev(b)), Cout, winograd=mode, gn_stats=True)
    n = bld.group_norm(y, 8, weight=dev(gw), bias=dev(gb), act=1)
    bld.finish()
    conv = the_conv(bld, mode)
    assert conv.splitk == 1 and y.gn_quads is not None
    assert "az_groupnorm_stats_f32" not in [nm for _, _, nm in bld.tape.ops]
    res = run_forms(monkeypatch, bld, [y, n], ["64,1"] + rects)
    ref = gn_reference(x0, w, b, 8, gw, gb)
    for form in rects:
        assert torch.equal(res["64,1"][0], res[form][0]), form
        e_ab = max_err(res["64,1"][1], res[form][1])
        e_ref = max_err(from_nhwc(res[form][1].reshape(B, H, W, -1), Cout), ref)
        print(f"{mode} {form}: rectangle vs run records {e_ab:.2e}, vs torch {e_ref:.2e}")
        assert e_ab < 2.5e-5 and e_ref < 6e-5
    # a shape that does not divide the tile grid cannot carry the moments: refused, not silently wrong
    monkeypatch.setenv("AZ_X3_BLOCK", "32,2")
    with pytest.raises(az.AzulaAmdError):
        bld.tape.run()


@pytest.mark.parametrize("mode", ["wx3", "wh2"])
def test_split_k_with_the_stats_combining_reduce(az, monkeypatch, mode):
    r"""Two K slices write slabs, the combine kernel sums them and produces the GroupNorm moments: the slabs are bit-equal, so
    everything behind them is."""
    from azula_amd.engine import Builder

    B, H, W, Cin, Cout = 2, 16, 16, 128, 128
    g, x0, _, w, b = layer(B, H, W, Cin, Cout)
    gw, gb = torch.randn(Cout, generator=g), torch.randn(Cout, generator=g)
    bld = Builder(torch.device("cuda"))
    a0 = act_of(x0)
    y = bld.conv(a0, bld.pack_conv(dev(w), dev(b)), Cout, winograd=mode, gn_stats=True)
    n = bld.group_norm(y, 8, weight=dev(gw), bias=dev(gb), act=1)
    bld.finish()
    assert the_conv(bld, mode).splitk == 2 and y.gn_quads is not None
    res = run_forms(monkeypatch, bld, [y, n], ["64,1", "8,8", "16,4"])
    assert_bit_equal(res)
    ref = gn_reference(x0, w, b, 8, gw, gb)
    assert max_err(from_nhwc(res["8,8"][1].reshape(B, H, W, -1), Cout), ref) < 6e-5


def test_rectangular_form_against_fp64(az, monkeypatch):
    r"""The layer and the bound of test_conv2d_x3_accuracy (Cin = 256, K = 2304, mixed channel scales): the piece forms with square
    blocks stay at the error level of the fp32 Winograd stream -- rms <= 1.25 x, max <= 1.5 x."""
    from azula_amd.engine import Act, Builder

    g = torch.Generator().manual_seed(5)
    B, Cin, Cout, H, W = 1, 256, 128, 32, 32
    x = torch.randn(B, Cin, H, W, generator=g) * torch.exp(torch.randn(B, Cin, 1, 1, generator=g))  # mixed channel scales
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin)
    b = torch.randn(Cout, generator=g)
    ref = F.conv2d(x.double(), w.double(), b.double(), padding=1)
    monkeypatch.setenv("AZ_DEBUG_AB", "1")
    monkeypatch.setenv("AZ_X3_BLOCK", "8,8")
    errs = {}
    for mode in (True, "wx3", "wh2"):
        bld = Builder(torch.device("cuda"))
        xa = Act(to_nhwc(dev(x)).reshape(-1), B, H, W, Cin, Cin, True)
        y = bld.conv(xa, bld.pack_conv(dev(w), dev(b)), Cout, winograd=mode)
        bld.finish()
        bld.tape.run()
        e = (from_nhwc(y.buf.reshape(B, H, W, Cout), Cout).double().cpu() - ref).abs()
        errs[mode] = (e.max().item(), e.pow(2).mean().sqrt().item())
    print("conv error vs fp64 (max, rms):", errs)
    for mode in ("wx3", "wh2"):
        assert errs[mode][1] <= 1.25 * errs[True][1] and errs[mode][0] <= 1.5 * errs[True][0], errs
