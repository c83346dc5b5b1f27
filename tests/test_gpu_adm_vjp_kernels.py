r"""The input-gradient kernels of ``csrc/backward_adm.hip`` against torch fp64 autograd of the same operation on the CPU.

* norm-affine pullback (``az_norm_affine_bwd_{stats,apply}_f32``): the pooled, activated, FiLM-modulated ``F.group_norm`` over one
  source or a channel concatenation read in place.  Inputs are ``3 randn + 10 ((c % 3) - 1)`` per channel (a one-pass variance
  fails on them), ``scale`` of order 0.3; cotangents v, 1e-6 v and 1e4 v (linearity over the range a cotangent takes); a second
  launch gives the same bits.
* ``az_avgpool_bwd_f32`` and the ADM preconditioning pullback (``az_adm_precond_bwd_{out,in}_f32``) on the same grids, F = 2 C:
  the log-variance channels come out exactly 0.

Bound: ``max(4 e_ref, 1e-4)`` relative to the largest magnitude of the fp64 result, ``e_ref`` = what torch's own fp32 autograd loses
against fp64 on the same inputs, measured here on the CPU (the rule of ``tests/test_gpu_unet_vjp.py``).
"""

import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from azula_amd import _lib

pytestmark = pytest.mark.gpu

S = lambda: _lib.stream_ptr()  # noqa: E731
EPS = 1e-5


def rel(a, ref):
    return float((a - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def bound(e_ref):
    return max(4 * e_ref, 1e-4)


def nhwc(t, cs=None):
    B, Cc, H, W = t.shape
    out = torch.zeros(B, H, W, Cc if cs is None else cs, dtype=torch.float32)
    out[..., :Cc] = t.permute(0, 2, 3, 1)
    return out.cuda().contiguous()


def nchw(t, Cc):
    return t.cpu()[..., :Cc].permute(0, 3, 1, 2).double()


def padded(t, cs):
    out = torch.zeros(*t.shape[:-1], cs)
    out[..., : t.shape[-1]] = t
    return out.cuda().contiguous()


def pool_fn(y, pool):
    if pool == 1:
        return F.avg_pool2d(y, 2)
    if pool == 2:
        return F.avg_pool2d(y, (1, 2))
    return y


# (name, channels of the sources, (H, W), groups, act, pool, res, channel stride of a one-source tensor)
CASES = [
    ("i_float4_chunks", (128,), (24, 24), 32, 1, 0, True, 128),
    ("ii_pool_cg3_straddle", (32, 64), (6, 10), 32, 1, 1, False, None),
    ("iii_two_sources", (32, 32), (7, 5), 4, 0, 0, True, None),
    ("iii_two_sources_float4_straddle", (32, 32), (7, 5), 1, 1, 0, True, None),
    ("iv_pool_1x2", (64,), (1, 12), 32, 1, 2, False, 64),
    ("iv_pool_1x2_float4", (64,), (1, 12), 8, 0, 2, True, 64),
    ("v_padded_lanes", (40,), (5, 3), 8, 0, 0, False, 44),
    ("v_padded_lanes_float4", (40,), (6, 4), 2, 1, 1, True, 44),
]


@pytest.mark.parametrize("name,chans,hw,groups,act,pool,with_res,cs1", CASES, ids=[c[0] for c in CASES])
def test_norm_affine_bwd(name, chans, hw, groups, act, pool, with_res, cs1):
    B, (H, W) = 2, hw
    Ct = sum(chans)
    cs = Ct if len(chans) == 2 else cs1
    gen = torch.Generator().manual_seed(3)
    x = 3 * torch.randn(B, Ct, H, W, generator=gen) + 10.0 * (torch.arange(Ct) % 3 - 1).float().reshape(1, Ct, 1, 1)
    gamma = 1 + 0.3 * torch.randn(Ct, generator=gen)
    beta = torch.randn(Ct, generator=gen)
    scale = 0.3 * torch.randn(B, Ct, generator=gen)
    shift = torch.randn(B, Ct, generator=gen)
    Ho, Wo = (H // 2 if pool == 1 else H), (W // 2 if pool else W)
    v = torch.randn(B, Ct, Ho, Wo, generator=gen)
    res = torch.randn(B, Ct, H, W, generator=gen) if with_res else None

    def fn(xx, dt):
        y = F.group_norm(xx, groups, gamma.to(dt), beta.to(dt), EPS)
        y = y * (1 + scale.to(dt)[:, :, None, None]) + shift.to(dt)[:, :, None, None]
        return pool_fn(F.silu(y) if act else y, pool)

    grads = []
    with torch.enable_grad():
        for dt in (torch.float64, torch.float32):
            xx = x.to(dt).requires_grad_()
            grads.append(torch.autograd.grad(fn(xx, dt), xx, v.to(dt))[0].double())
    ref, e_ref = grads[0], rel(grads[1], grads[0])

    # device tensors: the sources in place, the tables of the forward (statistics pass + finalize)
    if len(chans) == 2:
        c0 = chans[0]
        x0d, x1d = nhwc(x[:, :c0]), nhwc(x[:, c0:])
        x1p, c0s = x1d.data_ptr(), c0
    else:
        x0d, x1d = nhwc(x, cs), None
        x1p, c0s = None, 0
    gd, bd = gamma.cuda(), beta.cuda()
    scd, shd = padded(scale, cs), padded(shift, cs)
    fch, bch = 3, (3 if H * W >= 3 else 1)
    fpart = torch.empty(B * fch * groups * 4, device="cuda")
    _lib.call("az_groupnorm_stats_f32", fpart.data_ptr(), x0d.data_ptr(), x1p, c0s, B, H * W, Ct, cs, groups, fch, S())
    ST = torch.empty(2, B, cs, device="cuda")
    f = _lib.AzNormFinalizeArgs()
    f.S, f.T, f.partials = ST[0].data_ptr(), ST[1].data_ptr(), fpart.data_ptr()
    f.weight, f.bias, f.scale, f.shift, f.scale_bstride = gd.data_ptr(), bd.data_ptr(), scd.data_ptr(), shd.data_ptr(), cs
    f.B, f.C, f.cs, f.groups, f.nchunks, f.eps = B, Ct, cs, groups, fch, EPS
    _lib.call("az_groupnorm_finalize_f32", C.byref(f), S())

    def ptr(t):
        return None if t is None else t.data_ptr()

    def run(s):  # the cotangent and the residual (the cotangent of a second consumer) scaled alike
        vd = nhwc(v * s, cs)
        r0d = r1d = None
        if with_res and x1d is not None:
            r0d, r1d = nhwc(res[:, : chans[0]] * s), nhwc(res[:, chans[0] :] * s)
        elif with_res:
            r0d = nhwc(res * s, cs)
        bpart = torch.empty(B * bch * groups * 4, device="cuda")
        dx0 = torch.full_like(x0d, float("nan"))
        dx1 = torch.full_like(x1d, float("nan")) if x1d is not None else None
        _lib.call("az_norm_affine_bwd_stats_f32", bpart.data_ptr(), x0d.data_ptr(), x1p, c0s, vd.data_ptr(), ST[0].data_ptr(),
                  ST[1].data_ptr(), gd.data_ptr(), scd.data_ptr(), cs, fpart.data_ptr(), fch, B, H, W, Ct, cs, groups, bch, act, pool, EPS, S())
        _lib.call("az_norm_affine_bwd_apply_f32", dx0.data_ptr(), ptr(dx1), ptr(r0d), ptr(r1d), x0d.data_ptr(), x1p, c0s, vd.data_ptr(),
                  ST[0].data_ptr(), ST[1].data_ptr(), gd.data_ptr(), scd.data_ptr(), cs, fpart.data_ptr(), fch, bpart.data_ptr(), bch,
                  B, H, W, Ct, cs, groups, act, pool, EPS, S())
        torch.cuda.synchronize()
        return dx0, dx1

    def gather(d0, d1):
        if d1 is None:
            assert bool((d0.cpu()[..., Ct:] == 0).all()), "pad lanes are written as zero"
            return nchw(d0, Ct)
        return torch.cat([nchw(d0, chans[0]), nchw(d1, chans[1])], dim=1)

    if with_res:
        ref = ref + res.double()
    d0, d1 = run(1.0)
    e0, e1 = run(1.0)
    assert torch.equal(d0, e0) and (d1 is None or torch.equal(d1, e1)), "two launches differ"
    for s in (1.0, 1e-6, 1e4):
        got = gather(*run(s))
        err = rel(got, ref * s)
        print(f"norm_affine_bwd {name} cotangent x{s:g}: err {err:.3e} e_ref {e_ref:.3e}")
        assert torch.isfinite(got).all()
        assert err < bound(e_ref)


GRIDS = [(24, 24, 1), (6, 10, 1), (1, 12, 2), (4, 6, 2)]


@pytest.mark.parametrize("H,W,pool", GRIDS)
@pytest.mark.parametrize("with_res", [False, True])
def test_avgpool_bwd(H, W, pool, with_res):
    B, Cc, cs = 2, 6, 8
    gen = torch.Generator().manual_seed(4)
    Ho, Wo = (H // 2 if pool == 1 else H), W // 2
    g = torch.randn(B, Cc, Ho, Wo, generator=gen) * 1e3
    res = torch.randn(B, Cc, H, W, generator=gen) * 1e3 if with_res else None
    with torch.enable_grad():
        xx = torch.zeros(B, Cc, H, W, dtype=torch.float64, requires_grad=True)
        ref = torch.autograd.grad(pool_fn(xx, pool), xx, g.double())[0]
    if with_res:
        ref = ref + res.double()
    gd, rd = nhwc(g, cs), (nhwc(res, cs) if with_res else None)
    outs = []
    for _ in range(2):
        dx = torch.full((B, H, W, cs), float("nan"), device="cuda")
        _lib.call("az_avgpool_bwd_f32", dx.data_ptr(), gd.data_ptr(), None if rd is None else rd.data_ptr(), B, H, W, cs, pool, S())
        outs.append(dx)
    assert torch.equal(outs[0], outs[1])
    assert bool((outs[0].cpu()[..., Cc:] == 0).all())
    err = rel(nchw(outs[0], Cc), ref)
    print(f"avgpool_bwd {H}x{W} pool {pool}: err {err:.3e}")
    assert err < 2.0 ** -22  # one product by a power of two (exact) and at most one addition


@pytest.mark.parametrize("H,W", [(24, 24), (6, 10), (1, 12)])
@pytest.mark.parametrize("per_sample", [False, True])
@pytest.mark.parametrize("clip", [True, False])
def test_adm_precond_bwd(H, W, per_sample, clip):
    B, Cc = 2, 3
    Fc = 2 * Cc
    gen = torch.Generator().manual_seed(5)
    x_t = torch.randn(B, Cc, H, W, generator=gen)
    eps_hat = torch.randn(B, Cc, H, W, generator=gen)
    v = torch.randn(B, Cc, H, W, generator=gen)
    gback = torch.randn(B, Cc, H, W, generator=gen)  # (stands for the backbone's pullback)
    n = B if per_sample else 1
    c_in, c_out, c_skip = (torch.rand(n, generator=gen) + 0.5 for _ in range(3))
    c_out = -c_out
    ex = lambda c: c.reshape(-1, 1, 1, 1).double()  # noqa: E731
    lo, hi = (-1.0, 1.0) if clip else (-float("inf"), float("inf"))
    raw = ex(c_skip) * x_t.double() + ex(c_out) * eps_hat.double()
    mean = raw.clamp(lo, hi).float()
    mask = ((raw > lo) & (raw < hi)).double()
    assert not clip or 0.1 < 1 - mask.mean() < 0.9
    ref_out = torch.zeros(B, Fc, H, W, dtype=torch.float64)
    ref_out[:, :Cc] = ex(c_out) * mask * v.double()
    ref_in = ex(c_in) * gback.double() + ex(c_skip) * mask * v.double()
    md, vd, gd = mean.cuda(), v.cuda(), gback.cuda()
    gF = torch.full((B, Fc, H, W), float("nan"), device="cuda")
    dx = torch.full((B, Cc, H, W), float("nan"), device="cuda")
    ci, co, ck = c_in.cuda(), c_out.cuda(), c_skip.cuda()
    _lib.call("az_adm_precond_bwd_out_f32", gF.data_ptr(), vd.data_ptr(), md.data_ptr(), co.data_ptr(), int(per_sample), B, Cc, Fc, H * W, lo, hi, S())
    _lib.call("az_adm_precond_bwd_in_f32", dx.data_ptr(), gd.data_ptr(), vd.data_ptr(), md.data_ptr(), ci.data_ptr(), ck.data_ptr(), int(per_sample),
              B, Cc * H * W, lo, hi, S())
    assert bool((gF[:, Cc:] == 0).all()), "the log-variance channels take no cotangent"
    e_out, e_in = rel(gF.cpu().double(), ref_out), rel(dx.cpu().double(), ref_in)
    print(f"adm_precond_bwd {H}x{W} per_sample={per_sample} clip={clip}: out {e_out:.3e} in {e_in:.3e}")
    assert e_out < 2.0 ** -22 and e_in < 2.0 ** -21  # one / two roundings (a product, a fused multiply-add behind a product)
