r"""The pending normalisation of the x3 / f16x2 Winograd kernel's input (AzConvArgs.in_affine; csrc/wino_x3.hip: AFF) in the
rectangle form, where act(x * scale + shift) is applied ONCE per staged pixel on its way into LDS instead of on every thread's
4 x 4 patch.  The run form ("64,1") still transforms the patch, under its validity mask: it is the reference.

Every case asserts
  (a) the rectangle forms are BIT-EQUAL to the run form of the same tape (AZ_DEBUG_AB=1 / AZ_X3_BLOCK, as in
      tests/test_gpu_wino_rect.py): the same fused multiply-add on the same bits, zeros where the patch mask put zeros;
  (b) the error against F.conv2d in float64 on the explicitly normalised input stays below that file's bound,
      3 (3e-6 sqrt(9 Cin) + 1e-5) max(1, max|ref|), so that both forms being wrong together is not a pass.
The shapes are the smallest at which each mechanism exists."""

import math

import pytest
import torch
import torch.nn.functional as F

from conftest import max_err

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

NAME = {"wx3": "az_conv2d_winograd_x3_f32", "wh2": "az_conv2d_winograd_f16x2_f32"}
MODES = ["wx3", "wh2"]


@pytest.fixture(scope="module")
def az():
    from azula_amd import _lib

    _lib.lib()
    return _lib


def dev(t):
    return t.to("cuda").contiguous()


def to_nhwc(x):
    B, Cc, H, W = x.shape
    cs = (Cc + 3) // 4 * 4
    y = torch.zeros(B, H, W, cs, dtype=x.dtype, device=x.device)
    y[..., :Cc] = x.permute(0, 2, 3, 1)
    return y.contiguous()


def from_nhwc(y, Cc):
    return y[..., :Cc].permute(0, 3, 1, 2).contiguous()


def act_of(x, affine=None):
    r"""The source tensor as an Act; affine = (scale (B, C), shift (B, C), in_act): its normalisation is still pending."""
    from azula_amd.engine import Act

    B, Cc, H, W = x.shape
    a = Act(to_nhwc(dev(x)).reshape(-1), B, H, W, Cc, (Cc + 3) // 4 * 4, True)
    if affine is not None:
        sc, sh, in_act = affine
        a.affine = (dev(torch.cat((sc.reshape(-1), sh.reshape(-1)))), in_act)
    return a


def layer(B, H, W, Cin, Cout, *, seed=0, zero_scale=False):
    g = torch.Generator().manual_seed(1000 * seed + 7 * Cin + Cout + H)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin)
    b = torch.randn(Cout, generator=g)
    sc, sh = torch.randn(B, Cin, generator=g), torch.randn(B, Cin, generator=g)
    if zero_scale:
        sc = torch.zeros_like(sc)
    return x, w, b, sc, sh


def normalised(x, sc, sh, in_act):
    xin = x.double() * sc.double()[:, :, None, None] + sh.double()[:, :, None, None]
    return F.silu(xin) if in_act else xin


def conv_ops(bld):
    return [(args[0]._obj, nm) for _, args, nm in bld.tape.ops if nm.startswith("az_conv2d")]


def the_conv(bld, mode):
    convs = conv_ops(bld)
    assert [nm for _, nm in convs] == [NAME[mode]], convs
    assert convs[0][0].in_affine, "the affine was materialised instead of folded into the gather"
    return convs[0][0]


def run_forms(monkeypatch, bld, bufs, forms):
    r"""Runs the finished tape once per block form; the outputs are poisoned in between so that a launch that writes nothing shows."""
    monkeypatch.setenv("AZ_DEBUG_AB", "1")  # (A/B overrides are honoured only under the debug switch)
    res = {}
    for form in forms:
        monkeypatch.setenv("AZ_X3_BLOCK", form)
        for t in bufs:
            t.fill_(float("nan"))
        bld.tape.run()
        torch.cuda.synchronize()
        res[form] = [t.clone() for t in bufs]
    return res


def assert_bit_equal(res, what=""):
    ref = res["64,1"]
    for form, got in res.items():
        for r, g in zip(ref, got):
            assert torch.isfinite(r).all(), (what, "run form left non-finite values")
            assert torch.equal(r, g), (what, form, (r - g).abs().max().item())


def assert_close_to_fp64(out_nhwc, shape, Cin, Cout, ref, what=""):
    B, H, W = shape
    tol = 3 * (3e-6 * math.sqrt(Cin * 9) + 1e-5)  # (tests/test_gpu_wino_rect.py)
    err = max_err(from_nhwc(out_nhwc.reshape(B, H, W, -1), Cout), ref)
    bound = tol * max(1.0, ref.abs().max().item())
    print(f"{what}: max error against fp64 {err:.3e} (bound {bound:.3e})")
    assert err < bound, (what, err, bound)


def affine_layer(monkeypatch, mode, B, H, W, Cin, Cout, in_act, rects, *, zero_scale=False, periodic=False):
    from azula_amd.engine import Builder

    x, w, b, sc, sh = layer(B, H, W, Cin, Cout, zero_scale=zero_scale)
    bld = Builder(torch.device("cuda"))
    xa = act_of(x, (sc, sh, in_act))  # (the descriptor holds raw addresses: the sources stay alive here)
    y = bld.conv(xa, bld.pack_conv(dev(w), dev(b)), Cout, winograd=mode, periodic=periodic)
    bld.finish()
    conv = the_conv(bld, mode)
    assert conv.in_act == in_act and conv.pad_mode == int(periodic)
    res = run_forms(monkeypatch, bld, [y.buf], ["64,1"] + rects)
    what = (mode, B, H, W, Cin, Cout, in_act)
    assert_bit_equal(res, what)
    xin = normalised(x, sc, sh, in_act)
    if periodic:
        ref = F.conv2d(F.pad(xin, (1, 1, 1, 1), mode="circular"), w.double(), b.double())
    else:
        ref = F.conv2d(xin, w.double(), b.double(), padding=1)
    for form in rects:
        assert_close_to_fp64(res[form][0], (B, H, W), Cin, Cout, ref, f"{what} {form}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("in_act", [0, 1])
def test_shift_stays_out_of_the_padding(az, monkeypatch, in_act, mode):
    r"""One full 8 x 8 block; scale exactly 0, shift O(1): the input is act(shift) inside the map and ZERO in the padding, so a
    padding slot that received the shift shows in (b) at the border pixels (an error of O(shift), five orders above the bound)."""
    affine_layer(monkeypatch, mode, 1, 16, 16, 16, 64, in_act, ["8,8"], zero_scale=True)


@pytest.mark.parametrize("mode", MODES)
def test_scale_and_shift_of_the_blocks_own_image(az, monkeypatch, mode):
    r"""10 x 6 tiles: the rectangles are ragged both ways and no block shares images; scales and shifts differ by image."""
    affine_layer(monkeypatch, mode, 3, 20, 12, 32, 64, 0, ["8,8", "16,4", "4,16"])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("in_act", [0, 1])
def test_channel_tail(az, monkeypatch, in_act, mode):
    r"""Cin = 24: the last K step holds 8 channels (TAIL), the quads past the source's end get scale = shift = 0; two cout blocks."""
    affine_layer(monkeypatch, mode, 2, 34, 18, 24, 128, in_act, ["8,8", "16,4"])


@pytest.mark.parametrize("mode", MODES)
def test_circular_padding(az, monkeypatch, mode):
    r"""Odd sizes, the window wraps on both sides: no slot is out of bounds, every staged pixel is transformed."""
    affine_layer(monkeypatch, mode, 2, 18, 13, 16, 64, 0, ["8,8", "4,16", "32,2"], periodic=True)


@pytest.mark.parametrize("mode", MODES)
def test_upsampled_single_source(az, monkeypatch, mode):
    r"""up0 = 1, source 9 x 7 read as 18 x 14: the slot geometry (and with it the padding) lives in output coordinates."""
    from azula_amd.engine import Builder

    B, H, W, Cin, Cout = 2, 18, 14, 16, 64
    x, w, b, sc, sh = layer(B, H // 2, W // 2, Cin, Cout)
    bld = Builder(torch.device("cuda"))
    xa = act_of(x, (sc, sh, 0))
    y = bld.conv(xa, bld.pack_conv(dev(w), dev(b)), Cout, up0=1, hin=H, win=W, winograd=mode)
    bld.finish()
    assert the_conv(bld, mode).up0 == 1
    res = run_forms(monkeypatch, bld, [y.buf], ["64,1", "8,8", "16,4"])
    assert_bit_equal(res)
    up = F.interpolate(normalised(x, sc, sh, 0), scale_factor=(2.0, 2.0), mode="nearest")
    ref = F.conv2d(up, w.double(), b.double(), padding=1)
    for form in ("8,8", "16,4"):
        assert_close_to_fp64(res[form][0], (B, H, W), Cin, Cout, ref, f"{mode} up0 {form}")


@pytest.mark.parametrize("mode", MODES)
def test_split_k_slice_inside_the_k_range(az, monkeypatch, mode):
    r"""Four K steps in two slices: the second workgroup row starts at step 2, whose scale / shift its first staging loads."""
    from azula_amd.engine import Builder

    B, H, W, Cin, Cout = 2, 16, 16, 64, 64
    x, w, b, sc, sh = layer(B, H, W, Cin, Cout)
    bld = Builder(torch.device("cuda"))
    xa = act_of(x, (sc, sh, 0))
    y = bld.conv(xa, bld.pack_conv(dev(w), dev(b)), Cout, winograd=mode)
    conv = the_conv(bld, mode)
    if conv.splitk != 2:  # (forced: the launcher's rule may leave so small a layer whole)
        if conv.splitk == 1:
            bld._ws_users.append(conv)
        conv.splitk = 2
        bld._ws_need = max(bld._ws_need, 2 * B * H * W * conv.cout_s)
    bld.finish()
    assert the_conv(bld, mode).splitk == 2
    res = run_forms(monkeypatch, bld, [y.buf], ["64,1", "8,8", "16,4"])
    assert_bit_equal(res)
    ref = F.conv2d(normalised(x, sc, sh, 0), w.double(), b.double(), padding=1)
    for form in ("8,8", "16,4"):
        assert_close_to_fp64(res[form][0], (B, H, W), Cin, Cout, ref, f"{mode} split-K {form}")


@pytest.mark.parametrize("mode", MODES)
def test_groupnorm_moments_of_the_output(az, monkeypatch, mode):
    r"""gn_quads with an affine input.  The outputs of all forms are bit-equal.  A record covers the tiles of its block, so records
    of different block shapes hold different partial sums: they are compared bit for bit where the blocks hold the same tiles in
    the same order (8 x 8 rectangles on a map 8 tiles wide are the runs), and for EVERY form with the records of the same form
    on the materialised tensor (az_affine_act_f32 evaluates the same fused multiply-add, so that tape's gather stages the same bits
    through the plain kernel)."""
    from azula_amd.engine import Builder

    B, H, W, Cin, Cout = 2, 32, 16, 16, 128
    x, w, b, sc, sh = layer(B, H, W, Cin, Cout)
    forms = ["64,1", "8,8", "4,16"]
    res = {}
    for lazy in (True, False):
        bld = Builder(torch.device("cuda"))
        xa = act_of(x, (sc, sh, 0))
        src = xa if lazy else bld.materialize(xa)
        y = bld.conv(src, bld.pack_conv(dev(w), dev(b)), Cout, winograd=mode, gn_stats=True)
        bld.finish()
        (conv, name), = conv_ops(bld)
        assert name == NAME[mode] and bool(conv.in_affine) == lazy and conv.splitk == 1 and y.gn_quads is not None
        res[lazy] = run_forms(monkeypatch, bld, [y.buf, y.gn_quads[0]], forms)
    for form in forms:
        assert torch.isfinite(res[True][form][1]).all(), form
        assert torch.equal(res[True]["64,1"][0], res[True][form][0]), (form, "outputs against the run form")
        assert torch.equal(res[True][form][0], res[False][form][0]), (form, "outputs against the materialised input")
        assert torch.equal(res[True][form][1], res[False][form][1]), (form, "records against the materialised input")
    assert torch.equal(res[True]["64,1"][1], res[True]["8,8"][1]), "records of 8 x 8 rectangles against the runs"
    ref = F.conv2d(normalised(x, sc, sh, 0), w.double(), b.double(), padding=1)
    for form in ("8,8", "4,16"):
        assert_close_to_fp64(res[True][form][0], (B, H, W), Cin, Cout, ref, f"{mode} moments {form}")
