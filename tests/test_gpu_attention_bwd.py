r"""The attention backward kernels (``csrc/attention_bwd.hip``) and the FFN activation pullbacks against fp64 autograd.

Bound, as in ``test_gpu_unet_vjp.py``: the error is relative to the fp64 result's largest magnitude and must stay below
``max(4 e_ref, 1e-4)``, ``e_ref`` being what the reference's own fp32 autograd loses against fp64 on the same quantity (measured on
the CPU, ``attention_bwd_cases.reference``; below 2.5e-5 for every case, ``test_attention_bwd_cases_host.py``).
"""

import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

import attention_bwd_cases as cases
from oracle import nets

pytestmark = pytest.mark.gpu

TOL = 1e-4


def bound(e_ref):
    return max(4 * e_ref, TOL)


def rel(a, ref):
    return float((a.double().cpu() - ref).abs().max() / ref.abs().max())


def tokens_of(t):  # (B, H, L, D) -> (B, L, H D)
    b, h, l, d = t.shape
    return t.permute(0, 2, 1, 3).reshape(b, l, h * d)


def heads_of(t, h):  # (B, L, H D) -> (B, H, L, D)
    b, l, hd = t.shape
    return t.reshape(b, l, h, hd // h).permute(0, 2, 1, 3)


def run_bwd(q, k, v, out, dout, mask, scale):
    r"""``az_attention_bwd_f32`` on the fused layouts of the gradient plan: q^ | k^ in a (B, L, 2 H D) buffer, v in the last third
    of a (B, L, 3 H D) one; dq^ | dk^ into a (B, L, 2 H D) buffer, dv into the last third of a (B, L, 3 H D) one whose other
    thirds must stay untouched."""
    from azula_amd import _lib

    B, H, L, D = q.shape
    HD = H * D
    dev = "cuda"
    qk = torch.cat((tokens_of(q), tokens_of(k)), dim=-1).float().to(dev).contiguous()
    qkv = torch.zeros(B, L, 3 * HD, device=dev)
    qkv[..., 2 * HD:] = tokens_of(v).float().to(dev)
    o = tokens_of(out).float().to(dev).contiguous()
    do = tokens_of(dout).float().to(dev).contiguous()
    dqk = torch.full((B, L, 2 * HD), float("nan"), device=dev)
    dqkv = torch.full((B, L, 3 * HD), float("nan"), device=dev)
    ws = torch.empty(2 * B * H * L, device=dev)
    a = _lib.AzAttnBwdArgs()
    a.q, a.k, a.v, a.out, a.dout = qk.data_ptr(), qk.data_ptr() + 4 * HD, qkv.data_ptr() + 8 * HD, o.data_ptr(), do.data_ptr()
    a.dq, a.dk, a.dv, a.workspace = dqk.data_ptr(), dqk.data_ptr() + 4 * HD, dqkv.data_ptr() + 8 * HD, ws.data_ptr()
    a.batch, a.heads, a.tokens, a.head_dim, a.scale = B, H, L, D, scale
    for n, w in (("q", 2), ("k", 2), ("v", 3), ("o", 1), ("do", 1), ("dq", 2), ("dk", 2), ("dv", 3)):
        setattr(a, n + "_bstride", L * w * HD)
        setattr(a, n + "_tstride", w * HD)
        setattr(a, n + "_hstride", D)
    m8 = None
    if mask is not None:
        m = mask[None, None] if mask.ndim == 2 else mask
        m8 = m.to(device=dev, dtype=torch.uint8).contiguous()
        a.mask = m8.data_ptr()
        a.mask_bstride = m8.stride(0) if m.shape[0] > 1 else 0
        a.mask_hstride = m8.stride(1) if m.shape[1] > 1 else 0
    _lib.call("az_attention_bwd_f32", ctypes.byref(a), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert torch.isnan(dqkv[..., : 2 * HD]).all(), "the q / k thirds of the dqkv tensor belong to az_qk_prep_bwd_f32"
    return heads_of(dqk[..., :HD], H), heads_of(dqk[..., HD:], H), heads_of(dqkv[..., 2 * HD:], H)


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_attention_bwd_matches_fp64(name):
    c = cases.make_case(name)
    (out, dq, dk, dv), e_ref = cases.reference(name)
    got = run_bwd(c["q"], c["k"], c["v"], out, c["dout"], c["mask"], c["scale"])
    for tag, g, ref, e in zip(("dq", "dk", "dv"), got, (dq, dk, dv), e_ref):
        err = rel(g, ref)
        print(name, tag, f"err {err:.3e} e_ref {e:.3e}")
        assert torch.isfinite(g).all()
        assert err < bound(e)  # measured <= 8.9e-7; the +-30-logit case 2.9e-6 (e_ref 1.2e-6) (MI355X)
    # two calls on the same inputs: the same bits
    again = run_bwd(c["q"], c["k"], c["v"], out, c["dout"], c["mask"], c["scale"])
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    # a cotangent has no range: 1e-6 dout and 1e4 dout scale the result within the same bound
    for s in (1e-6, 1e4):
        gs = run_bwd(c["q"], c["k"], c["v"], out, c["dout"] * s, c["mask"], c["scale"])
        for tag, g, ref, e in zip(("dq", "dk", "dv"), gs, (dq, dk, dv), e_ref):
            err = rel(g, ref * s)
            print(name, tag, f"dout * {s:g}: err {err:.3e}")
            assert torch.isfinite(g).all() and err < bound(e)  # measured: as above (<= 2.9e-6) (MI355X)


def test_masked_pairs_leave_no_trace():
    r"""Keys masked for every query get exactly zero gradients, and changing their k / v changes no bit of any output."""
    c = cases.make_case("d64_l130")
    L = c["L"]
    dead = torch.zeros(L, dtype=torch.bool)
    dead[5] = True
    dead[64:101] = True  # (the 32 keys [64, 96) of one wave of the dK / dV pass -- a key tile dead for every query -- and five more)
    mask = (~dead)[None, :].expand(L, L).contiguous()
    out = cases.sdpa_grads(c["q"], c["k"], c["v"], c["dout"], mask, c["scale"], torch.float64)[0]
    base = run_bwd(c["q"], c["k"], c["v"], out, c["dout"], mask, c["scale"])
    k2, v2 = c["k"].clone(), c["v"].clone()
    k2[:, :, dead] = k2[:, :, dead] * 3.0 + 1.0
    v2[:, :, dead] = v2[:, :, dead] - 7.0
    pert = run_bwd(c["q"], k2, v2, out, c["dout"], mask, c["scale"])
    for a, b in zip(base, pert):
        assert torch.equal(a, b)
    assert (base[1][:, :, dead] == 0).all() and (base[2][:, :, dead] == 0).all()
    ref = cases.sdpa_grads(c["q"], c["k"], c["v"], c["dout"], mask, c["scale"], torch.float64)[1:]
    for g, r in zip(base, ref):
        assert rel(g, r) < TOL


# ------------------------------------------------------------------------------------------------ q / k preparation
def qk_prep_reference(q, k, theta, norm, d, dtype, gq=None, gk=None):
    r"""rope(rms_norm(q | k)) on the REAL ``d`` channels of every head and, with cotangents, its pullback (fp64 results)."""
    qq, kk = (t[..., :d].detach().to(dtype).clone().requires_grad_() for t in (q, k))
    with torch.enable_grad():
        a, b = qq, kk
        if norm:
            a, b = F.rms_norm(a, (d,), eps=1e-5), F.rms_norm(b, (d,), eps=1e-5)
        if theta is not None:
            a, b = nets.apply_rope(a, b, theta[..., : d // 2].to(dtype))
        if gq is None:
            return a.detach().double(), b.detach().double()
        grads = torch.autograd.grad((a, b), (qq, kk), (gq[..., :d].to(dtype), gk[..., :d].to(dtype)))
    return a.detach().double(), b.detach().double(), grads[0].double(), grads[1].double()


@pytest.mark.parametrize("norm,rope,D,d", [(1, 1, 32, 32), (1, 0, 64, 64), (0, 1, 16, 16), (0, 0, 32, 32), (1, 1, 32, 24), (1, 1, 128, 128)])
def test_qk_prep_and_its_pullback(norm, rope, D, d):
    from azula_amd import _lib

    B, L, H = 2, 37, 3
    gen = torch.Generator().manual_seed(100 + D + d + 2 * norm + rope)
    # token rows of magnitude 1e-3, 1 and 1e3
    mag = torch.tensor([1e-3, 1.0, 1e3])[torch.arange(L) % 3].reshape(1, L, 1, 1)
    q = torch.randn(B, L, H, D, generator=gen) * mag
    k = torch.randn(B, L, H, D, generator=gen) * mag
    q[..., d:] = 0  # (zero-padded heads: the projection packs zero rows there)
    k[..., d:] = 0
    theta = None
    if rope:
        theta = torch.randn(L, H, D // 2, generator=gen) * 2
        theta[..., d // 2:] = 0  # (padded pairs do not turn)
    gq = torch.randn(B, L, H, D, generator=gen)
    gk = torch.randn(B, L, H, D, generator=gen)
    r64 = qk_prep_reference(q, k, theta, norm, d, torch.float64, gq, gk)
    r32 = qk_prep_reference(q, k, theta, norm, d, torch.float32, gq, gk)

    HD = H * D
    qkv = torch.zeros(B, L, 3 * HD)
    qkv[..., :HD], qkv[..., HD: 2 * HD] = q.reshape(B, L, HD), k.reshape(B, L, HD)
    qkv = qkv.cuda()
    hat = torch.full((B, L, 2 * HD), float("nan"), device="cuda")
    cs = sn = None
    if rope:
        cs, sn = torch.cos(theta).cuda().contiguous(), torch.sin(theta).cuda().contiguous()
    tabs = (cs.data_ptr(), sn.data_ptr()) if rope else (None, None)
    s = _lib.stream_ptr()
    _lib.call("az_qk_prep_f32", hat.data_ptr(), hat.data_ptr() + 4 * HD, qkv.data_ptr(), qkv.data_ptr() + 4 * HD, B, L, H, D,
              L * 3 * HD, 3 * HD, D, L * 2 * HD, 2 * HD, D, norm, d if d != D else 0, 1e-5, *tabs, s)
    g = torch.cat((gq.reshape(B, L, HD), gk.reshape(B, L, HD)), dim=-1).cuda().contiguous()
    dqkv = torch.full((B, L, 3 * HD), float("nan"), device="cuda")
    _lib.call("az_qk_prep_bwd_f32", dqkv.data_ptr(), dqkv.data_ptr() + 4 * HD, g.data_ptr(), g.data_ptr() + 4 * HD, qkv.data_ptr(),
              qkv.data_ptr() + 4 * HD, B, L, H, D, L * 2 * HD, 2 * HD, D, L * 3 * HD, 3 * HD, D, L * 3 * HD, 3 * HD, D, norm,
              d if d != D else 0, 1e-5, *tabs, s)
    torch.cuda.synchronize()
    assert torch.isnan(dqkv[..., 2 * HD:]).all(), "the v third belongs to az_attention_bwd_f32"
    got = (hat[..., :HD].reshape(B, L, H, D), hat[..., HD:].reshape(B, L, H, D),
           dqkv[..., :HD].reshape(B, L, H, D), dqkv[..., HD: 2 * HD].reshape(B, L, H, D))
    assert (got[0][..., d:] == 0).all() and (got[1][..., d:] == 0).all()  # padded channels of q^ / k^ stay zero
    for tag, gg, a64, a32 in zip(("q^", "k^", "dq", "dk"), got, r64, r32):
        assert torch.isfinite(gg).all()
        for cls in range(3):  # each magnitude class against its own largest value
            rows = torch.arange(L) % 3 == cls
            e_ref = rel(a32[:, rows], a64[:, rows])
            err = rel(gg[:, rows][..., :d], a64[:, rows])
            print(f"norm={norm} rope={rope} D={D} d={d} {tag} rows x{[1e-3, 1, 1e3][cls]:g}: err {err:.3e} e_ref {e_ref:.3e}")
            assert err < bound(e_ref)  # measured <= 1.6e-7 (MI355X)


# ------------------------------------------------------------------------------------------------ FFN activations
def act_ref(kind, p):
    return {1: F.silu, 2: F.relu, 3: lambda t: F.relu(t).square()}[kind](p)


@pytest.mark.parametrize("kind", [1, 2, 3])
def test_act_and_its_pullback(kind):
    from azula_amd import _lib

    gen = torch.Generator().manual_seed(40 + kind)
    n = 4 * 1031
    p = torch.randn(n, generator=gen) * 3
    p[:8] = torch.tensor([0.0, -0.0, 1e-30, -1e-30, 1e-6, -1e-6, 30.0, -30.0])  # the inputs straddle 0
    g = torch.randn(n, generator=gen)

    def ref(dtype):
        pp = p.to(dtype).clone().requires_grad_()
        with torch.enable_grad():
            y = act_ref(kind, pp)
            return y.detach().double(), torch.autograd.grad(y, pp, g.to(dtype))[0].double()

    (y64, d64), (y32, d32) = ref(torch.float64), ref(torch.float32)
    pd, gd = p.cuda(), g.cuda()
    y, d = torch.empty_like(pd), torch.empty_like(pd)
    _lib.call("az_act_f32", y.data_ptr(), pd.data_ptr(), n, kind, _lib.stream_ptr())
    _lib.call("az_act_bwd_f32", d.data_ptr(), gd.data_ptr(), pd.data_ptr(), n, kind, _lib.stream_ptr())
    print(f"kind {kind}: act err {rel(y, y64):.3e} (e_ref {rel(y32, y64):.3e}) bwd err {rel(d, d64):.3e} (e_ref {rel(d32, d64):.3e})")
    assert rel(y, y64) < bound(rel(y32, y64)) and rel(d, d64) < bound(rel(d32, d64))  # measured: bwd 3.1e-7 / 0 / 3.4e-8 (MI355X)
    if kind in (2, 3):
        assert (d[p.cuda() <= 0] == 0).all()
    for s in (1e-6, 1e4):
        _lib.call("az_act_bwd_f32", d.data_ptr(), (gd * s).data_ptr(), pd.data_ptr(), n, kind, _lib.stream_ptr())
        assert rel(d, d64 * s) < bound(rel(d32, d64))


@pytest.mark.parametrize("cout,xs", [(10, 20), (9, 20), (64, 128)])
def test_swiglu_pullback(cout, xs):
    from azula_amd import _lib

    gen = torch.Generator().manual_seed(50 + cout)
    rows, gs = 23, (cout + 3) // 4 * 4
    x = torch.randn(rows, xs, generator=gen) * 3
    g = torch.randn(rows, gs, generator=gen)

    def ref(dtype):
        xx = x[:, : 2 * cout].to(dtype).clone().requires_grad_()
        with torch.enable_grad():
            u = xx.unflatten(-1, (-1, 2))
            y = u[..., 0] * F.silu(u[..., 1])
            return torch.autograd.grad(y, xx, g[:, :cout].to(dtype))[0].double()

    d64, d32 = ref(torch.float64), ref(torch.float32)
    xd, gd = x.cuda(), g.cuda()
    dx = torch.full_like(xd, float("nan"))
    _lib.call("az_swiglu_bwd_f32", dx.data_ptr(), gd.data_ptr(), xd.data_ptr(), rows, cout, xs, gs, _lib.stream_ptr())
    err, e_ref = rel(dx[:, : 2 * cout], d64), rel(d32, d64)
    print(f"swiglu bwd cout {cout}: err {err:.3e} e_ref {e_ref:.3e}")
    assert err < bound(e_ref)  # measured <= 1.0e-7 (MI355X)
    assert (dx[:, 2 * cout:] == 0).all()  # the pad lanes are written as zero


# ------------------------------------------------------------------------------------------------ argument validation
def test_new_entries_validate_their_arguments():
    r"""Every new entry returns its error code before it launches anything (the addresses are never dereferenced)."""
    from azula_amd import _lib

    lib = _lib.lib()
    P, Q = 0x10000, 0x10004  # aligned / misaligned

    def args(**kw):
        d = dict(q=P, k=P, v=P, out=P, dout=P, dq=P, dk=P, dv=P, workspace=P, batch=1, heads=2, tokens=9, head_dim=32, scale=0.1)
        for n in ("q", "k", "v", "o", "do", "dq", "dk", "dv"):
            d.update({n + "_bstride": 9 * 64, n + "_tstride": 64, n + "_hstride": 32})
        d.update(kw)
        return ctypes.byref(_lib.AzAttnBwdArgs(**d))

    bw = lambda **kw: lib.az_attention_bwd_f32(args(**kw), None)  # noqa: E731
    assert lib.az_attention_bwd_f32(None, None) == -1
    for n in ("q", "k", "v", "out", "dout", "dq", "dk", "dv", "workspace"):
        assert bw(**{n: None}) == -1, n
        assert bw(**{n: Q}) == -3, n
    assert bw(head_dim=24) == -4 and bw(head_dim=80) == -4 and bw(head_dim=256) == -4
    assert bw(tokens=0) == -2 and bw(batch=0) == -2 and bw(heads=0) == -2
    for n in ("q_tstride", "k_hstride", "v_bstride", "o_tstride", "do_tstride", "dq_hstride", "dk_tstride", "dv_bstride"):
        assert bw(**{n: 66}) == -3, n

    fw = (P, P, P, P, 2, 9, 2, 32, 9 * 192, 192, 32, 9 * 128, 128, 32, 1, 0, 1e-5, None, None)
    prep = lambda a: lib.az_qk_prep_f32(*a, None)  # noqa: E731
    sub = lambda a, i, v: a[:i] + (v,) + a[i + 1:]  # noqa: E731
    assert prep(sub(fw, 0, None)) == -1 and prep(sub(fw, 3, None)) == -1 and prep(sub(fw, 17, P)) == -1  # (one table without the other)
    assert prep(sub(fw, 7, 24)) == -4
    assert prep(sub(fw, 1, Q)) == -3 and prep(sub(fw, 9, 190)) == -3 and prep(sub(fw, 13, 30)) == -3
    assert prep(sub(fw, 5, 0)) == -2 and prep(sub(fw, 15, 33)) == -2  # no tokens; norm_dim > head_dim
    bk = (P, P, P, P, P, P, 2, 9, 2, 32, 9 * 128, 128, 32, 9 * 192, 192, 32, 9 * 192, 192, 32, 1, 0, 1e-5, None, None)
    prepb = lambda a: lib.az_qk_prep_bwd_f32(*a, None)  # noqa: E731
    assert prepb(sub(bk, 0, None)) == -1 and prepb(sub(bk, 2, None)) == -1 and prepb(sub(bk, 5, None)) == -1
    assert prepb(sub(bk, 9, 24)) == -4
    assert prepb(sub(bk, 3, Q)) == -3 and prepb(sub(bk, 11, 130)) == -3 and prepb(sub(bk, 17, 190)) == -3
    assert prepb(sub(bk, 7, 0)) == -2

    assert lib.az_act_f32(P, None, 16, 1, None) == -1 and lib.az_act_f32(P, P, 18, 1, None) == -2
    assert lib.az_act_f32(P, P, 16, 4, None) == -2 and lib.az_act_f32(Q, P, 16, 1, None) == -3
    assert lib.az_act_bwd_f32(P, P, None, 16, 1, None) == -1 and lib.az_act_bwd_f32(P, P, P, 18, 1, None) == -2
    assert lib.az_act_bwd_f32(P, P, P, 16, 0, None) == -2 and lib.az_act_bwd_f32(P, Q, P, 16, 1, None) == -3
    assert lib.az_swiglu_bwd_f32(P, None, P, 4, 8, 16, 8, None) == -1 and lib.az_swiglu_bwd_f32(P, P, P, 4, 8, 18, 8, None) == -2
    assert lib.az_swiglu_bwd_f32(P, P, P, 4, 9, 16, 12, None) == -2 and lib.az_swiglu_bwd_f32(P, P, Q, 4, 8, 16, 8, None) == -3
