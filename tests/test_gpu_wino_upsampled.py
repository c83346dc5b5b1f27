r"""Structured (nearest-upsampled) sources of the x3 / f16x2 Winograd kernel (csrc/wino_x3.hip: UPS) against the same kernel
without the skip.

On a source read through nearest upsampling of an even-sized map, frequency index 2 of B^T d B is exactly +0 in both
directions (csrc/conv_shared.h: x3_structured_mask); the UPS kernels leave those 7 of 16 frequencies out on that source's K
steps.  They add +0 to accumulators that start at +0, so the outputs must be BIT-EQUAL with the switch on and off
(AZ_X3_UPS=0, honoured under AZ_DEBUG_AB, empties the mask: the kernels without UPS run).  One case per group is also held
against F.conv2d on the explicitly upsampled and concatenated input at the bound of tests/test_gpu_wino_rect.py, so that both
forms being wrong together is not a pass."""

import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import max_err

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

NAME = {"wx3": "az_conv2d_winograd_x3_f32", "wh2": "az_conv2d_winograd_f16x2_f32", "wh2d": "az_conv2d_winograd_f16x2_f32"}
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
    y = torch.zeros(B, H, W, (Cc + 3) // 4 * 4, dtype=x.dtype, device=x.device)
    y[..., :Cc] = x.permute(0, 2, 3, 1)
    return y.contiguous()


def from_nhwc(y, Cc):
    return y[..., :Cc].permute(0, 3, 1, 2).contiguous()


def act_of(x):
    from azula_amd.engine import Act

    B, Cc, H, W = x.shape
    return Act(to_nhwc(dev(x)).reshape(-1), B, H, W, Cc, (Cc + 3) // 4 * 4, True)


def low(n, up):
    return (n + (1 << up) - 1) >> up


def tensors(B, H, W, C0, C1, Cout, up0=0, up1=0, seed=0):
    r"""x0 (read through up0), x1 (through up1; None without a second source), weight, bias; (H, W) is the map the conv sees."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * C0 + 3 * C1 + Cout + H)
    x0 = torch.randn(B, C0, low(H, up0), low(W, up0), generator=g)
    x1 = torch.randn(B, C1, low(H, up1), low(W, up1), generator=g) if C1 else None
    w = torch.randn(Cout, C0 + C1, 3, 3, generator=g) / math.sqrt(9 * (C0 + C1))
    b = torch.randn(Cout, generator=g)
    return g, x0, x1, w, b


def upsampled(x, up, H, W):
    if x is None:
        return None
    return x.repeat_interleave(1 << up, 2).repeat_interleave(1 << up, 3)[:, :, :H, :W] if up else x


def reference(x0, x1, w, b, H, W, up0=0, up1=0, periodic=False):
    x = upsampled(x0, up0, H, W)
    if x1 is not None:
        x = torch.cat((x, upsampled(x1, up1, H, W)), 1)
    if periodic:
        return F.conv2d(F.pad(x, (1, 1, 1, 1), mode="circular"), w, b)
    return F.conv2d(x, w, b, padding=1)


def tol_of(cin):
    return 3 * (3e-6 * math.sqrt(cin * 9) + 1e-5)  # (tests/test_gpu_wino_rect.py, tests/test_gpu_kernels.py: conv_tol of the piece forms)


def the_conv(bld, mode):
    convs = [(args[0]._obj, nm) for _, args, nm in bld.tape.ops if nm.startswith("az_conv2d")]
    assert [nm for _, nm in convs] == [NAME[mode]], convs
    return convs[0][0]


def masks(az, a):
    r"""(the rule's mask, the mask a launch made now hands the kernel) of descriptor ``a`` -- host arithmetic only."""
    m, lm = C.c_int32(-1), C.c_int32(-1)
    assert az.lib().az_winograd_x3_structured_mask(C.byref(a), C.addressof(m), C.addressof(lm)) == 0
    return m.value, lm.value


def run_switch(monkeypatch, az, bld, outs, a, expect_mask, block=None):
    r"""Runs the finished tape with the skip on and off (outputs poisoned in between); checks what the host entry reports in
    either state, that everything written is finite, and bit-equality.  Returns the outputs of the run with the skip on."""
    monkeypatch.setenv("AZ_DEBUG_AB", "1")  # (A/B overrides are honoured only under the debug switch)
    if block is not None:
        monkeypatch.setenv("AZ_X3_BLOCK", block)
    res = {}
    for ups in ("1", "0"):
        monkeypatch.setenv("AZ_X3_UPS", ups)
        if a is not None:
            assert masks(az, a) == (expect_mask, expect_mask if ups == "1" else 0), (ups, masks(az, a))
        for o in outs:
            o.fill_(float("nan"))
        bld.tape.run()
        torch.cuda.synchronize()
        res[ups] = [o.clone() for o in outs]
    for on, off in zip(res["1"], res["0"]):
        assert torch.isfinite(off).all(), "the launch without the skip left non-finite values"
        assert torch.equal(on, off), (on - off).abs().max().item()
    return res["1"]


def merge_layer(bld, mode, x0, x1, w, b, Cout, H, W, up1=1, **kw):
    a0, a1 = act_of(x0), act_of(x1)  # (the descriptor holds raw addresses: the caller keeps these alive)
    y = bld.conv(a0, bld.pack_conv(dev(w), dev(b), cin0=x0.shape[1]), Cout, src1=a1, up1=up1, hin=H, win=W, winograd=mode, **kw)
    return y, (a0, a1)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize(
    "B,H,W,C0,C1,Cout",
    [
        (1, 16, 16, 16, 16, 64),    # one block, one plain step and one structured step
        (2, 20, 12, 32, 48, 128),   # several structured steps, ragged tiles, two cout blocks
        (2, 20, 12, 16, 24, 64),    # the channel TAIL lies inside the structured source
    ],
)
def test_merge_form(az, monkeypatch, B, H, W, C0, C1, Cout, mode):
    from azula_amd.engine import Builder

    _, x0, x1, w, b = tensors(B, H, W, C0, C1, Cout, up1=1)
    bld = Builder(torch.device("cuda"))
    y, keep = merge_layer(bld, mode, x0, x1, w, b, Cout, H, W)
    bld.finish()
    (out,) = run_switch(monkeypatch, az, bld, [y.buf], the_conv(bld, mode), 2)
    ref = reference(x0, x1, w, b, H, W, up1=1)
    assert max_err(from_nhwc(out.reshape(B, H, W, -1), Cout), ref) < tol_of(C0 + C1) * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("block", ["64,1", "8,8"])
def test_block_forms(az, monkeypatch, block, mode):
    r"""The run form and the rectangular form of the block (AZ_X3_BLOCK) each have their own UPS instantiation."""
    from azula_amd.engine import Builder

    B, H, W, C0, C1, Cout = 2, 20, 12, 32, 48, 64
    _, x0, x1, w, b = tensors(B, H, W, C0, C1, Cout, up1=1, seed=1)
    bld = Builder(torch.device("cuda"))
    y, keep = merge_layer(bld, mode, x0, x1, w, b, Cout, H, W)
    bld.finish()
    (out,) = run_switch(monkeypatch, az, bld, [y.buf], the_conv(bld, mode), 2, block=block)
    ref = reference(x0, x1, w, b, H, W, up1=1)
    assert max_err(from_nhwc(out.reshape(B, H, W, -1), Cout), ref) < tol_of(C0 + C1) * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("mode", MODES)
def test_split_k_with_a_slice_that_begins_inside_the_second_source(az, monkeypatch, mode):
    r"""96 + 160 channels = 6 + 10 steps cut into K slices: one slice crosses the source switch, a later one begins inside the
    structured source."""
    from azula_amd.engine import Builder

    B, H, W, C0, C1, Cout = 2, 16, 16, 96, 160, 64
    _, x0, x1, w, b = tensors(B, H, W, C0, C1, Cout, up1=1)
    bld = Builder(torch.device("cuda"))
    y, keep = merge_layer(bld, mode, x0, x1, w, b, Cout, H, W)
    bld.finish()
    a = the_conv(bld, mode)
    nkc0, nk = C0 // 16, (C0 + C1) // 16
    kps = (nk + a.splitk - 1) // a.splitk
    starts = list(range(0, nk, kps))
    assert a.splitk > 1 and any(s > nkc0 for s in starts) and any(s < nkc0 < s + kps for s in starts), (a.splitk, starts)
    (out,) = run_switch(monkeypatch, az, bld, [y.buf], a, 2)
    ref = reference(x0, x1, w, b, H, W, up1=1)
    assert max_err(from_nhwc(out.reshape(B, H, W, -1), Cout), ref) < tol_of(C0 + C1) * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("mode", MODES)
def test_circular_padding(az, monkeypatch, mode):
    from azula_amd.engine import Builder

    B, H, W, C0, C1, Cout = 2, 20, 12, 16, 32, 64
    _, x0, x1, w, b = tensors(B, H, W, C0, C1, Cout, up1=1, seed=2)
    bld = Builder(torch.device("cuda"))
    y, keep = merge_layer(bld, mode, x0, x1, w, b, Cout, H, W, periodic=True)
    bld.finish()
    a = the_conv(bld, mode)
    assert a.pad_mode == 1
    (out,) = run_switch(monkeypatch, az, bld, [y.buf], a, 2)
    ref = reference(x0, x1, w, b, H, W, up1=1, periodic=True)
    assert max_err(from_nhwc(out.reshape(B, H, W, -1), Cout), ref) < tol_of(C0 + C1) * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("mode", MODES)
def test_groupnorm_moments_record(az, monkeypatch, mode):
    r"""gn_stats: the moments record of the epilogue is computed from the same outputs, so it is bit-equal too."""
    from azula_amd.engine import Builder

    B, H, W, C0, C1, Cout = 1, 16, 16, 16, 16, 64
    _, x0, x1, w, b = tensors(B, H, W, C0, C1, Cout, up1=1, seed=3)
    bld = Builder(torch.device("cuda"))
    y, keep = merge_layer(bld, mode, x0, x1, w, b, Cout, H, W, gn_stats=True)
    bld.finish()
    a = the_conv(bld, mode)
    assert a.splitk == 1 and y.gn_quads is not None and a.gn_quads
    out, rec = run_switch(monkeypatch, az, bld, [y.buf, y.gn_quads[0]], a, 2)
    ref = reference(x0, x1, w, b, H, W, up1=1)
    assert max_err(from_nhwc(out.reshape(B, H, W, -1), Cout), ref) < tol_of(C0 + C1) * max(1.0, ref.abs().max().item())
    # the record: (count, mean, M2, 0) per channel quad of the one 64-tile block -- the mean against the outputs themselves
    quads = rec.reshape(Cout // 4, 4)
    assert torch.equal(quads[:, 0], torch.full_like(quads[:, 0], 1024.0))
    mean = out.reshape(H * W, Cout // 4, 4).mean((0, 2))
    assert max_err(quads[:, 1], mean) < 1e-5 * max(1.0, mean.abs().max().item())


def test_f16x2_with_the_measured_scale(az, monkeypatch):
    r"""in_absmax on both sources: the kernel picks the activation scale from the sources' maxima."""
    from azula_amd.engine import Builder

    B, H, W, C0, C1, Cout = 2, 20, 12, 32, 48, 64
    _, x0, x1, w, b = tensors(B, H, W, C0, C1, Cout, up1=1, seed=4)
    x0, x1 = 37.0 * x0, 0.02 * x1  # (away from the fixed scale's O(1))
    bld = Builder(torch.device("cuda"))
    y, keep = merge_layer(bld, "wh2d", x0, x1, w, b, Cout, H, W)
    bld.finish()
    convs = [args[0]._obj for _, args, nm in bld.tape.ops if nm == NAME["wh2d"]]
    assert len(convs) == 1 and convs[0].in_absmax0 and convs[0].in_absmax1
    (out,) = run_switch(monkeypatch, az, bld, [y.buf], convs[0], 2)
    ref = reference(x0, x1, w, b, H, W, up1=1)
    assert max_err(from_nhwc(out.reshape(B, H, W, -1), Cout), ref) < tol_of(C0 + C1) * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("up", [1, 2])
def test_whole_launch_form(az, monkeypatch, up, mode):
    r"""up0 on a single source (ADM's up-ResBlocks and Upsample layers): every K step of the launch is structured.  up = 2: rows
    2 th and 2 th + 1 differ in bit 0 only, so any shift >= 1 qualifies."""
    from azula_amd.engine import Builder

    B, H, W, C0, Cout = 1, 16, 16, 32, 64
    _, x0, _, w, b = tensors(B, H, W, C0, 0, Cout, up0=up)
    bld = Builder(torch.device("cuda"))
    a0 = act_of(x0)
    y = bld.conv(a0, bld.pack_conv(dev(w), dev(b)), Cout, up0=up, winograd=mode)
    bld.finish()
    (out,) = run_switch(monkeypatch, az, bld, [y.buf], the_conv(bld, mode), 1)
    ref = reference(x0, None, w, b, H, W, up0=up)
    assert max_err(from_nhwc(out.reshape(B, H, W, -1), Cout), ref) < tol_of(C0) * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("mode", MODES)
def test_an_odd_narrowed_map_is_not_structured(az, monkeypatch, mode):
    r"""15 x 13 over an 8 x 7 source: the last tile row has patch row 1 inside the map and row 2 outside (d2 = 0 != d1).  The rule
    says no, the switch changes nothing, and the result is right."""
    from azula_amd.engine import Builder

    B, H, W, C0, C1, Cout = 2, 15, 13, 16, 16, 64
    _, x0, x1, w, b = tensors(B, H, W, C0, C1, Cout, up1=1, seed=5)
    bld = Builder(torch.device("cuda"))
    y, keep = merge_layer(bld, mode, x0, x1, w, b, Cout, H, W)
    bld.finish()
    (out,) = run_switch(monkeypatch, az, bld, [y.buf], the_conv(bld, mode), 0)
    ref = reference(x0, x1, w, b, H, W, up1=1)
    assert max_err(from_nhwc(out.reshape(B, H, W, -1), Cout), ref) < tol_of(C0 + C1) * max(1.0, ref.abs().max().item())


def test_an_anisotropic_shift_is_not_structured(az, monkeypatch):
    r"""Upsampling along one axis only takes the anisotropic descriptor, which the Winograd kernels do not run: whatever kernel
    the engine picks, the rule says no and the switch changes nothing."""
    from azula_amd.engine import Builder

    B, H, W, C0, C1, Cout = 2, 16, 12, 16, 16, 64
    g = torch.Generator().manual_seed(11)
    x0 = torch.randn(B, C0, H, W, generator=g)
    x1 = torch.randn(B, C1, H // 2, W, generator=g)
    w = torch.randn(Cout, C0 + C1, 3, 3, generator=g) / math.sqrt(9 * (C0 + C1))
    b = torch.randn(Cout, generator=g)
    bld = Builder(torch.device("cuda"))
    a0, a1 = act_of(x0), act_of(x1)
    y = bld.conv(a0, bld.pack_conv(dev(w), dev(b), cin0=C0), Cout, src1=a1, up1=(1, 0), hin=H, win=W)
    bld.finish()
    convs = [args[0]._obj for _, args, nm in bld.tape.ops if nm.startswith("az_conv2d")]
    assert len(convs) == 1 and convs[0].aniso == 1
    (out,) = run_switch(monkeypatch, az, bld, [y.buf], convs[0], 0)
    ref = F.conv2d(torch.cat((x0, x1.repeat_interleave(2, 2)), 1), w, b, padding=1)
    assert max_err(from_nhwc(out.reshape(B, H, W, -1), Cout), ref) < tol_of(C0 + C1) * max(1.0, ref.abs().max().item())


def test_a_structured_first_source_in_front_of_a_plain_second_is_plain(az, monkeypatch):
    r"""The kernel walks plain steps first and structured steps behind them; the opposite order is reported (and run) as plain."""
    from azula_amd.engine import Builder

    B, H, W, C0, C1, Cout = 1, 16, 16, 16, 16, 64
    _, x0, x1, w, b = tensors(B, H, W, C0, C1, Cout, up0=1, seed=6)
    bld = Builder(torch.device("cuda"))
    a0, a1 = act_of(x0), act_of(x1)
    y = bld.conv(a0, bld.pack_conv(dev(w), dev(b), cin0=C0), Cout, src1=a1, up0=1, winograd="wx3")
    bld.finish()
    (out,) = run_switch(monkeypatch, az, bld, [y.buf], the_conv(bld, "wx3"), 0)
    ref = reference(x0, x1, w, b, H, W, up0=1)
    assert max_err(from_nhwc(out.reshape(B, H, W, -1), Cout), ref) < tol_of(C0 + C1) * max(1.0, ref.abs().max().item())


def test_the_switch_is_live(az, monkeypatch):
    r"""On an eligible layer the host entry reports the mask the kernel is given -- the rule's with the skip on, none with
    AZ_X3_UPS=0 -- and the switch is ignored without AZ_DEBUG_AB, like every A/B override."""
    from azula_amd.engine import Builder

    B, H, W, C0, C1, Cout = 1, 16, 16, 16, 16, 64
    _, x0, x1, w, b = tensors(B, H, W, C0, C1, Cout, up1=1)
    bld = Builder(torch.device("cuda"))
    y, keep = merge_layer(bld, "wh2", x0, x1, w, b, Cout, H, W)
    bld.finish()
    a = the_conv(bld, "wh2")
    monkeypatch.delenv("AZ_DEBUG_AB", raising=False)
    monkeypatch.setenv("AZ_X3_UPS", "0")
    assert masks(az, a) == (2, 2)
    monkeypatch.setenv("AZ_DEBUG_AB", "1")
    assert masks(az, a) == (2, 0)
    monkeypatch.setenv("AZ_X3_UPS", "1")
    assert masks(az, a) == (2, 2)
