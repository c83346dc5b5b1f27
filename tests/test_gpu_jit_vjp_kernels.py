r"""The C entries ``JiT.vjp`` and ``CFGDenoiser._az_vjp`` add (``az_rownorm_bwd_w_f32``, ``az_qk_prep_w_f32`` /
``az_qk_prep_bwd_w_f32``, ``az_cfg_split_f32``), through ctypes, against fp64 autograd of the torch formula.

Bounds, as in ``test_gpu_dit_vjp.py``: a pullback ``max(4 e_ref, 1e-4)`` relative to the largest magnitude of the fp64 result,
``e_ref`` being what the same torch formula loses under fp32 autograd (measured here on the CPU, never from the code under test);
the forward of the q / k preparation ``1e-5`` relative to the largest magnitude.  With NULL gains the new entries give the bits
of the entries they extend; the split is bit-equal to torch's fp32 products.
"""

import pytest
import torch

from test_gpu_dit_vjp import bound, oracle_vjp, rel

pytestmark = pytest.mark.gpu

B, ROWS = 2, 9


@pytest.fixture(scope="module")
def az():
    from azula_amd import _lib

    _lib.lib()
    return _lib


def ptr(t):
    return None if t is None else t.data_ptr()


# ------------------------------------------------------------------------------------------------ az_rownorm_bwd_w_f32
def rownorm_fn(kind, weight, scale, eps):
    def fn(x):  # (B, ROWS, C)
        w = weight.to(x.dtype)
        if kind == 0:
            var, mean = torch.var_mean(x, dim=-1, keepdim=True)  # unbiased
            n = (x - mean) / torch.sqrt(var + eps)
        else:
            n = x * torch.rsqrt(x.square().mean(dim=-1, keepdim=True) + eps)
        y = w * n
        return y if scale is None else (1 + scale.to(x.dtype)[:, None, :]) * y

    return fn


@pytest.mark.parametrize("has_res", [True, False])
@pytest.mark.parametrize("has_scale", [True, False])
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("C,cs", [(22, 24), (64, 64), (160, 160), (1280, 1280)])
def test_rownorm_bwd_with_gain(az, C, cs, kind, has_scale, has_res):
    gen = torch.Generator().manual_seed(1000 + C + 2 * kind + has_scale)
    x = 3 * torch.randn(B, ROWS, C, generator=gen) + (torch.arange(C) % 3 - 1).float()
    g = torch.randn(B, ROWS, C, generator=gen)
    weight = torch.randn(C, generator=gen)  # mixed signs, not near 1
    scale = 0.3 * torch.randn(B, C, generator=gen) if has_scale else None
    res = torch.randn(B, ROWS, C, generator=gen) if has_res else None
    eps = 1e-6
    _, ref = oracle_vjp(rownorm_fn(kind, weight, scale, eps), x, g, torch.float64)
    _, ref32 = oracle_vjp(rownorm_fn(kind, weight, scale, eps), x, g, torch.float32)
    e_ref = rel(ref32, ref)
    if has_res:
        ref = ref + res.double()

    def padded(t):  # (..., C) -> (..., cs) on the device, pad lanes holding what must not leak
        p = torch.full((*t.shape[:-1], cs), 7.0)
        p[..., :C] = t
        return p.cuda().contiguous()

    xd, gd = padded(x), padded(g)
    rd = padded(res) if has_res else None
    sd = padded(scale) if has_scale else None
    wd = weight.cuda()

    def run(entry, *w):
        dx = torch.full((B, ROWS, cs), float("nan"), device="cuda")
        az.call(entry, ptr(dx), ptr(xd), ptr(gd), ptr(rd), ptr(sd), cs, *w, B * ROWS, ROWS, C, cs, kind, eps, az.stream_ptr())
        return dx

    dx = run("az_rownorm_bwd_w_f32", ptr(wd))
    assert torch.equal(run("az_rownorm_bwd_w_f32", ptr(wd)), dx)  # deterministic
    assert (dx[..., C:] == 0).all()  # pad lanes written as zero
    err = rel(dx[..., :C], ref)
    print(f"rownorm_bwd_w C={C} kind={kind} scale={has_scale} res={has_res}: err {err:.3e} e_ref {e_ref:.3e}")
    assert torch.isfinite(dx).all() and err < bound(e_ref)  # measured <= 1.7e-7 (MI355X)
    # weight = NULL: the bits of az_rownorm_bwd_f32
    assert torch.equal(run("az_rownorm_bwd_w_f32", None), run("az_rownorm_bwd_f32"))


# ------------------------------------------------------------------------------------------------ az_qk_prep_w_f32 and its pullback
L, CTX, H = 9, 2, 2


def rotate(t, cos, sin):
    pairs = t.unflatten(-1, (-1, 2))
    rot = torch.stack((-pairs[..., 1], pairs[..., 0]), dim=-1).flatten(-2)
    return t * cos.repeat_interleave(2, dim=-1) + rot * sin.repeat_interleave(2, dim=-1)


def qk_fn(w, theta, d, eps):
    def fn(x):  # (B, L, H, d) real channels -> rope(w rms_norm(x))
        n = x * torch.rsqrt(x.square().mean(dim=-1, keepdim=True) + eps)
        th = theta[..., : d // 2].to(x.dtype)
        return rotate(w[:d].to(x.dtype) * n, torch.cos(th), torch.sin(th))

    return fn


@pytest.mark.parametrize("D,d", [(16, 16), (32, 32), (64, 64), (128, 128), (32, 24), (128, 80)])
def test_qk_prep_with_gains(az, D, d):
    gen = torch.Generator().manual_seed(2000 + D + d)
    HD = H * D
    eps = 1e-6
    qkv = torch.randn(B, L, 3, H, D, generator=gen) * 2
    qkv[:, :, :2, :, d:] = 0  # zero-padded heads: the projection packs zero rows there
    theta = torch.randn(L, H, D // 2, generator=gen) * 2
    theta[:CTX] = 0  # unrotated context tokens: cos 1, sin 0
    theta[..., d // 2:] = 0  # padded pairs do not turn
    gains = [1 + 0.5 * torch.randn(D, generator=gen) for _ in range(2)]
    for w in gains:
        w[d:] = 1  # unit gains on the pad lanes
    cot = torch.randn(B, L, 2, H, D, generator=gen)

    qkv_d = qkv.reshape(B, L, 3 * HD).cuda().contiguous()
    cot_d = cot.reshape(B, L, 2 * HD).cuda().contiguous()
    cs_d, sn_d = torch.cos(theta).cuda().contiguous(), torch.sin(theta).cuda().contiguous()
    w_d = [w.cuda() for w in gains]
    nd = d if d != D else 0

    def run(suffix, *w):
        hat = torch.full((B, L, 2 * HD), float("nan"), device="cuda")
        dqkv = torch.full((B, L, 3 * HD), float("nan"), device="cuda")
        s = az.stream_ptr()
        # q, k read in place from the fused (3 H C) token tensor through the strides
        az.call("az_qk_prep" + suffix, ptr(hat), ptr(hat) + 4 * HD, ptr(qkv_d), ptr(qkv_d) + 4 * HD, B, L, H, D, L * 3 * HD, 3 * HD, D,
                L * 2 * HD, 2 * HD, D, 1, nd, eps, ptr(cs_d), ptr(sn_d), *w, s)
        az.call("az_qk_prep_bwd" + suffix, ptr(dqkv), ptr(dqkv) + 4 * HD, ptr(cot_d), ptr(cot_d) + 4 * HD, ptr(qkv_d), ptr(qkv_d) + 4 * HD,
                B, L, H, D, L * 2 * HD, 2 * HD, D, L * 3 * HD, 3 * HD, D, L * 3 * HD, 3 * HD, D, 1, nd, eps, ptr(cs_d), ptr(sn_d), *w, s)
        torch.cuda.synchronize()
        return hat, dqkv

    hat, dqkv = run("_w_f32", ptr(w_d[0]), ptr(w_d[1]))
    assert torch.isnan(dqkv[..., 2 * HD:]).all(), "the v third belongs to az_attention_bwd_f32"
    hat, dq = hat.reshape(B, L, 2, H, D), dqkv[..., : 2 * HD].reshape(B, L, 2, H, D)
    assert (hat[..., d:] == 0).all()  # padded channels of q^ / k^ stay zero
    for n, tag in enumerate("qk"):
        x = qkv[:, :, n, :, :d]
        v = cot[:, :, n, :, :d]
        y64, ref = oracle_vjp(qk_fn(gains[n], theta, d, eps), x, v, torch.float64)
        _, ref32 = oracle_vjp(qk_fn(gains[n], theta, d, eps), x, v, torch.float32)
        e_ref = rel(ref32, ref)
        err_f, err_b = rel(hat[:, :, n, :, :d], y64), rel(dq[:, :, n, :, :d], ref)
        print(f"qk_prep_w D={D} d={d} {tag}: forward err {err_f:.3e}, pullback err {err_b:.3e} e_ref {e_ref:.3e}")
        assert err_f < 1e-5 and err_b < bound(e_ref)  # measured: forward <= 1.3e-7, pullback <= 1.4e-7 (MI355X)
    # NULL gains: the bits of the existing pair
    a, b = run("_w_f32", None, None), run("_f32")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1][..., : 2 * HD], b[1][..., : 2 * HD])


# ------------------------------------------------------------------------------------------------ az_cfg_split_f32
@pytest.mark.parametrize("g", [0.0, 2.5, -0.5])
@pytest.mark.parametrize("n", [4, 150, 4099])
def test_cfg_split(az, n, g):
    v = torch.randn(n, generator=torch.Generator().manual_seed(n)).cuda()
    gd = torch.tensor([g], dtype=torch.float32, device="cuda")
    v2 = torch.full((2 * n + 4,), float("nan"), device="cuda")
    az.call("az_cfg_split_f32", ptr(v2), ptr(v), ptr(gd), n, az.stream_ptr())
    assert torch.equal(v2[:n], (1.0 + gd) * v) and torch.equal(v2[n: 2 * n], -gd * v)
    assert torch.isnan(v2[2 * n:]).all()  # nothing past 2 n is written
