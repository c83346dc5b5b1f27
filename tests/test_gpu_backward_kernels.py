r"""The input-gradient kernels of ``csrc/backward.hip`` against torch fp64 autograd of the same operation on the CPU.

Inputs are not O(1) randn: per-channel offsets of 10 with unit spread, overall scales 1e-3 and 1e3, one constant group; odd
H and W; channel counts 3 / 20 / 64 (the pad lanes of the channel-padded layout must read back as exactly zero); strides 2 and
3; a narrowed upsampling.  Every kernel runs twice and must give the same bits.

Bounds (relative to the largest magnitude of the fp64 result).  ``e_ref`` is what torch's own fp32 autograd loses on the same
inputs against fp64, measured here on the CPU.
* normalisation pullbacks: ``max(4 e_ref, 1e-5)``.  The floor is reasoned, not measured: with a channel offset of 10 and unit
  spread, ``x - mean`` loses log2(10) = 3.3 of its 24 bits (5e-7 per element of xh); the pullback subtracts two group means of
  such terms from q, so a few 1e-6 is the format's floor and 1e-5 leaves a factor of about four over it.
* SiLU pullback: 2e-6.  v_exp_f32 and v_rcp_f32 are within 1 ulp each, the fp32 rounding of p log2(e) adds |p| 6e-8 to the
  exponent (common.h, az_silu): about 16 ulp of the largest value for |p| of a few units.
* channel scale: one rounding, 2^-23.  Zero stuffing: exact.  Upsampling pullback: at most sh sw - 1 additions, (sh sw) 2^-24.
"""

import pytest
import torch
import torch.nn.functional as F

from azula_amd import _lib

pytestmark = pytest.mark.gpu


def pad4(c):
    return (c + 3) // 4 * 4


def to_nhwc(t, cs=None):
    B, C, H, W = t.shape
    cs = pad4(C) if cs is None else cs
    out = torch.zeros(B, H, W, cs, dtype=torch.float32)
    out[..., :C] = t.permute(0, 2, 3, 1)
    return out.cuda().contiguous()


def from_nhwc(t, C):
    return t.cpu()[..., :C].permute(0, 3, 1, 2).double()


def pads_zero(t, C):
    return bool((t.cpu()[..., C:] == 0).all())


def hard(shape, scale, seed, const_channels=()):
    r"""(B, C, H, W): per-channel offsets of +-10, unit spread, times ``scale``; ``const_channels`` hold one constant."""
    gen = torch.Generator().manual_seed(seed)
    B, C, H, W = shape
    off = 10.0 * (torch.arange(C) % 3 - 1).double().reshape(1, C, 1, 1)
    x = torch.randn(shape, generator=gen, dtype=torch.float64) + off
    for c in const_channels:
        x[:, c] = 10.0
    return (x * scale).float()


def rel(a, ref):
    return float((a - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def twice(fn):
    a = fn()
    b = fn()
    assert torch.equal(a, b), "two runs differ"
    return a


def ref_pair(fn, x, g, *extra):
    r"""(fp64 gradient, e_ref): autograd of ``fn`` at x with cotangent g in fp64, and the error of torch's fp32 against it."""
    outs = []
    with torch.enable_grad():  # (other test modules switch gradients off for the whole session)
        for dt in (torch.float64, torch.float32):
            xx = x.to(dt).requires_grad_()
            y = fn(xx, *[e.to(dt) for e in extra])
            outs.append(torch.autograd.grad(y, xx, g.to(dt))[0].double())
    return outs[0], rel(outs[1], outs[0])


S = lambda: _lib.stream_ptr()  # noqa: E731


@pytest.mark.parametrize("scale", [1.0, 1e-3, 1e3])
@pytest.mark.parametrize("C,groups,const", [(3, 3, ()), (20, 4, ()), (20, 5, (4, 5, 6, 7)), (64, 4, tuple(range(16, 32)))])
def test_groupnorm_bwd(C, groups, const, scale):
    B, H, W = 2, 7, 5
    cs = pad4(C)
    x = hard((B, C, H, W), scale, 1, const)
    gen = torch.Generator().manual_seed(2)
    g = torch.randn(B, C, H, W, generator=gen) * 1e-3
    res = torch.randn(B, C, H, W, generator=gen) * 1e-3
    a = torch.randn(B, C, generator=gen) * 0.3
    eps = 1e-5

    def fn(xx, aa):
        return (1 + aa[:, :, None, None]) * F.group_norm(xx, groups, eps=eps)

    ref, e_ref = ref_pair(fn, x, g, a)
    ref = ref + res.double()
    xd, gd, rd = to_nhwc(x), to_nhwc(g), to_nhwc(res)
    ad = torch.zeros(B, cs)
    ad[:, :C] = a
    ad = ad.cuda()
    fch, bch = 3, 2
    fpart = torch.empty(B * fch * groups * 4, device="cuda")
    _lib.call("az_groupnorm_stats_f32", fpart.data_ptr(), xd.data_ptr(), None, 0, B, H * W, C, cs, groups, fch, S())

    def run():
        bpart = torch.empty(B * bch * groups * 4, device="cuda")
        dx = torch.full((B, H, W, cs), float("nan"), device="cuda")
        _lib.call("az_groupnorm_bwd_stats_f32", bpart.data_ptr(), xd.data_ptr(), gd.data_ptr(), ad.data_ptr(), cs, fpart.data_ptr(), fch,
                  B, H * W, C, cs, groups, bch, eps, S())
        _lib.call("az_groupnorm_bwd_apply_f32", dx.data_ptr(), xd.data_ptr(), gd.data_ptr(), rd.data_ptr(), ad.data_ptr(), cs,
                  fpart.data_ptr(), fch, bpart.data_ptr(), bch, B, H * W, C, cs, groups, eps, S())
        return dx

    dx = twice(run)
    assert pads_zero(dx, C)
    err = rel(from_nhwc(dx, C), ref)
    print(f"groupnorm_bwd C={C} groups={groups} scale={scale}: err {err:.3e} e_ref {e_ref:.3e}")
    assert err < max(4 * e_ref, 1e-5)  # measured <= 1.2e-7 (MI355X)


@pytest.mark.parametrize("scale", [1.0, 1e-3, 1e3])
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("C", [3, 20, 64])
def test_rownorm_bwd(C, kind, scale):
    B, H, W = 2, 7, 5
    cs = pad4(C)
    x = hard((B, C, H, W), scale, 3)
    gen = torch.Generator().manual_seed(4)
    g = torch.randn(B, C, H, W, generator=gen) * 1e3
    res = torch.randn(B, C, H, W, generator=gen) * 1e3
    a = torch.randn(B, C, generator=gen) * 0.3
    eps = 1e-5

    def fn(xx, aa):
        if kind == 0:
            var, mean = torch.var_mean(xx, dim=1, keepdim=True)  # unbiased
            n = (xx - mean) / torch.sqrt(var + eps)
        else:
            n = xx * torch.rsqrt(xx.square().mean(dim=1, keepdim=True) + eps)
        return (1 + aa[:, :, None, None]) * n

    ref, e_ref = ref_pair(fn, x, g, a)
    ref = ref + res.double()
    xd, gd, rd = to_nhwc(x), to_nhwc(g), to_nhwc(res)
    ad = torch.zeros(B, cs)
    ad[:, :C] = a
    ad = ad.cuda()

    def run():
        dx = torch.full((B, H, W, cs), float("nan"), device="cuda")
        _lib.call("az_rownorm_bwd_f32", dx.data_ptr(), xd.data_ptr(), gd.data_ptr(), rd.data_ptr(), ad.data_ptr(), cs, B * H * W, H * W,
                  C, cs, kind, eps, S())
        return dx

    dx = twice(run)
    assert pads_zero(dx, C)
    err = rel(from_nhwc(dx, C), ref)
    print(f"rownorm_bwd C={C} kind={kind} scale={scale}: err {err:.3e} e_ref {e_ref:.3e}")
    assert err < max(4 * e_ref, 1e-5)  # measured <= 2.2e-7 (MI355X)


@pytest.mark.parametrize("gscale", [1e-8, 1.0, 1e4])
@pytest.mark.parametrize("C", [3, 20, 64])
def test_silu_bwd(C, gscale):
    B, H, W = 2, 7, 5
    p = hard((B, C, H, W), 1.0, 5)
    p[0, 0, 0, :3] = torch.tensor([-90.0, 0.0, 90.0])
    g = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(6)) * gscale
    ref, _ = ref_pair(lambda pp: F.silu(pp), p, g)
    pd, gd = to_nhwc(p), to_nhwc(g)

    def run():
        y = torch.full_like(pd, float("nan"))
        _lib.call("az_silu_bwd_f32", y.data_ptr(), gd.data_ptr(), pd.data_ptr(), pd.numel(), S())
        return y

    y = twice(run)
    assert pads_zero(y, C)
    err = rel(from_nhwc(y, C), ref)
    print(f"silu_bwd C={C} gscale={gscale}: err {err:.3e}")
    assert err < 2e-6  # measured <= 5.4e-7 (MI355X)


@pytest.mark.parametrize("C", [3, 20, 64])
def test_channel_scale(C):
    B, H, W = 2, 7, 5
    cs = pad4(C)
    x = hard((B, C, H, W), 1e3, 7)
    s = torch.randn(B, 3 * cs, generator=torch.Generator().manual_seed(8))
    ref = x.double() * s[:, 2 * cs : 2 * cs + C].double()[:, :, None, None]
    xd, sd = to_nhwc(x), s.cuda()

    def run():
        y = torch.full_like(xd, float("nan"))
        _lib.call("az_channel_scale_f32", y.data_ptr(), xd.data_ptr(), sd.data_ptr() + 4 * 2 * cs, 3 * cs, B, H * W, C, cs, S())
        return y

    y = twice(run)
    assert pads_zero(y, C)
    assert rel(from_nhwc(y, C), ref) < 2.0 ** -23  # measured: below the bound (MI355X)


@pytest.mark.parametrize("stride", [(2, 2), (3, 3), (2, 3)])
@pytest.mark.parametrize("C", [3, 20, 64])
def test_zero_stuff_is_the_strided_conv_pullback(C, stride):
    r"""Zero stuffing alone is exact; with a stride-1 convolution of the transposed, flipped weight (torch, fp64) behind it, it is
    the data gradient of the strided convolution."""
    B, H, W = 2, 7, 9
    sh, sw = stride
    h, w = (H - 1) // sh + 1, (W - 1) // sw + 1
    g = hard((B, C, h, w), 1e3, 9)
    gd = to_nhwc(g)

    def run():
        G = torch.full((B, H, W, pad4(C)), float("nan"), device="cuda")
        _lib.call("az_zero_stuff_f32", G.data_ptr(), gd.data_ptr(), B, h, w, pad4(C), sh, sw, H, W, S())
        return G

    G = twice(run)
    assert pads_zero(G, C)
    ref = torch.zeros(B, C, H, W, dtype=torch.float64)
    ref[:, :, ::sh, ::sw] = g.double()
    assert torch.equal(from_nhwc(G, C), ref)
    wt = torch.randn(C, 4, 3, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(10))  # (cout = C, cin = 4)
    with torch.enable_grad():
        xin = torch.randn(B, 4, H, W, dtype=torch.float64).requires_grad_()
        want = torch.autograd.grad(F.conv2d(xin, wt, stride=stride, padding=1), xin, g.double())[0]
    got = F.conv2d(from_nhwc(G, C), wt.transpose(0, 1).flip(2, 3), padding=1)
    assert rel(got, want) < 1e-12


@pytest.mark.parametrize("stride,narrow", [((2, 2), (7, 5)), ((3, 3), (7, 8)), ((2, 3), (8, 9)), ((3, 2), (4, 3))])
@pytest.mark.parametrize("C", [3, 20, 64])
def test_upsample_nearest_bwd(C, stride, narrow):
    B, h, w = 2, 4, 3
    sh, sw = stride
    hn, wn = narrow
    assert hn <= h * sh and wn <= w * sw
    g = hard((B, C, hn, wn), 1e-3, 11)

    def fn(xx):
        return F.interpolate(xx, scale_factor=(float(sh), float(sw)), mode="nearest")[:, :, :hn, :wn]

    ref, _ = ref_pair(fn, torch.zeros(B, C, h, w), g)
    gd = to_nhwc(g)

    def run():
        dx = torch.full((B, h, w, pad4(C)), float("nan"), device="cuda")
        _lib.call("az_upsample_nearest_bwd_f32", dx.data_ptr(), gd.data_ptr(), B, h, w, pad4(C), sh, sw, hn, wn, S())
        return dx

    dx = twice(run)
    assert pads_zero(dx, C)
    err = rel(from_nhwc(dx, C), ref)
    print(f"upsample_nearest_bwd C={C} stride={stride} narrow={narrow}: err {err:.3e}")
    assert err < sh * sw * 2.0 ** -24  # measured <= 1.4e-7 (MI355X)
