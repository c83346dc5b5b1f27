r"""``az_op_fft2_f32``, ``FourierOperator`` and ``MRIOperator`` on the GPU against the dense fp64 DFT matrices of
``tests/fft_oracle.py``.

* exact: H, W <= 4 on integers, every form and both directions, EQUAL to the oracle (twiddles at quarter turns are 0 / +-1);
* the accuracy rule, per plane: ``||got - ref64||_2 <= max(4 e_ref, 2 * 2^-24) * S`` with ``S`` the 2-norm of the full complex
  fp64 result and ``e_ref`` what torch's own fp32 CPU transform loses on the same plane by the same measure (the margin of 4: a
  radix-2 kernel has twice pocketfft's rounding stages; ``test_operators_fft_host.py`` asserts that ``e_ref`` is far below the
  worst-case bound, so the rule cannot pass vacuously).  Measured ``err / (e_ref S)`` on an MI355X: DESIGN.md section 9d;
* planes and strides, determinism, the operators and their autograd Function, the dtype and size paths, and one DPS step and one
  MMPS mean of 4x accelerated MRI on the ``g28_guidance_vjp`` fixture's UNet.
"""

import ctypes as C
import math

import pytest
import torch

import fft_cases as fc
import fft_oracle as fo
import guidance_vjp_cases as gc
import guidance_vjp_oracle as go

pytestmark = pytest.mark.gpu
F64 = torch.float64


@pytest.fixture(autouse=True)
def _grad_mode_on():
    r"""Some modules of the suite switch grad mode off for the whole process; these tests differentiate."""
    with torch.enable_grad():
        yield


def _ops():
    from azula_amd.guidance import operators

    return operators


def _spy(monkeypatch):
    ops = _ops()
    names, launch = [], ops._launch
    monkeypatch.setattr(ops, "_launch", lambda name, *a: (names.append(name), launch(name, *a))[1])
    return names


def fft2(re, im, inverse, scale=1.0, want_im=True):
    r"""``az_op_fft2_f32`` on contiguous (B, C, H, W) device tensors: (dst_re, dst_im or None)."""
    from azula_amd import _lib

    B, Cc, H, W = re.shape
    dre, dim = torch.empty_like(re), torch.empty_like(re) if want_im else None
    floats = C.c_int64(-1)
    _lib.call("az_op_fft2_work", B, Cc, H, W, C.byref(floats))
    work = torch.empty(max(floats.value, 4), device=re.device) if not want_im else None
    n = Cc * H * W
    _lib.call("az_op_fft2_f32", dre.data_ptr(), None if dim is None else dim.data_ptr(), n, re.data_ptr(),
              None if im is None else im.data_ptr(), n, None if work is None else work.data_ptr(), B, Cc, H, W, int(inverse),
              scale, _lib.stream_ptr())
    return dre, dim


# ------------------------------------------------------------------------------------------------------------------ exact
@pytest.mark.parametrize("size", fc.EXACT_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_small_sizes_equal_the_fp64_oracle_on_integers(size):
    H, W = size
    for B, Cc in fc.EXACT_BC:
        re, im = fc.exact_planes(B, Cc, H, W, 1), fc.exact_planes(B, Cc, H, W, 2)
        for inverse in (False, True):
            for real_in in (True, False):
                ref = fo.dft2(re, None if real_in else im, inverse)
                for want_im in (True, False):
                    got_re, got_im = fft2(re.cuda(), None if real_in else im.cuda(), inverse, 1.0, want_im)
                    assert torch.equal(got_re.double().cpu(), ref.real), (B, Cc, inverse, real_in, want_im)
                    assert got_im is None or torch.equal(got_im.double().cpu(), ref.imag), (B, Cc, inverse, real_in)


# ------------------------------------------------------------------------------------------------------ the accuracy rule
@pytest.mark.parametrize("size", fc.ACCURACY_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_accuracy_rule(size):
    r"""The four data kinds are the four channels of one launch per form.  Two references per size: the forward transform of the
    real input (real -> real, measured in the inverse direction, has its conjugate) and the inverse transform of the complex
    input."""
    H, W = size
    re = torch.stack([fc.planes(kind, H, W)[0] for kind in fc.DATA])[None]
    im = torch.stack([fc.planes(kind, H, W)[1] for kind in fc.DATA])[None]
    ref_r, ref_c = fo.dft2(re, None, False), fo.dft2(re, im, True)
    refs = {"r2c": ref_r, "r2r": ref_r.conj(), "c2c": ref_c, "c2r": ref_c}
    worst = 0.0
    for form, (real_in, real_out, inverse) in fc.FORMS.items():
        ref = refs[form]
        S, e_ref, bound = fo.rule(ref, re, None if real_in else im, inverse)
        got_re, got_im = fft2(re.cuda(), None if real_in else im.cuda(), inverse, 1.0, not real_out)
        err2 = (got_re.double().cpu() - ref.real) ** 2
        if got_im is not None:
            err2 = err2 + (got_im.double().cpu() - ref.imag) ** 2
        err = err2.sum((-2, -1)).sqrt()
        for k, kind in enumerate(fc.DATA):
            e, b, s, r = (float(v[0, k]) for v in (err, bound, S, e_ref))
            print(f"fft {H}x{W} {form} {kind}: err/S {e / s:.3e} e_ref {r:.3e} ratio {e / s / r if r else math.inf:.2f} "
                  f"bound/S {b / s:.3e}")
            worst = max(worst, e / b)
        assert (err <= bound).all(), (form, (err / bound).tolist())
    print(f"fft {H}x{W}: worst err / bound {worst:.3f}")


# ---------------------------------------------------------------------------------------------------- planes and strides
def test_more_planes_than_workgroups():
    x = fc.exact_planes(7000, 10, 4, 4, 3)
    ref = fo.dft2(x)
    got_re, got_im = fft2(x.cuda(), None, False)
    assert torch.equal(got_re.double().cpu(), ref.real) and torch.equal(got_im.double().cpu(), ref.imag)


def test_strided_destination_guards_and_determinism():
    r"""(B, C) = (3, 5) at 32 x 16 into the two halves of a (3, 10, 32, 16) destination whose samples lie 64 guard words apart,
    with 64 more in front and behind; a plane alone gives the bits it has in the batch; two runs give the same bits."""
    from azula_amd import _lib

    B, Cc, H, W, G = 3, 5, 32, 16, 64
    x = torch.randn(B, Cc, H, W, generator=torch.Generator().manual_seed(5)).cuda()
    n, stride = Cc * H * W, 2 * Cc * H * W + G
    runs = []
    for _ in range(2):
        buf = torch.full((G + B * stride,), 7.5, device="cuda")
        base = buf.data_ptr() + 4 * G
        _lib.call("az_op_fft2_f32", base, base + 4 * n, stride, x.data_ptr(), None, n, None, B, Cc, H, W, 0, 1.0, _lib.stream_ptr())
        runs.append(buf.cpu())
    assert torch.equal(runs[0], runs[1])
    buf = runs[0]
    assert (buf[:G] == 7.5).all()
    body = buf[G:].reshape(B, stride)
    assert (body[:, 2 * n:] == 7.5).all()
    y = body[:, :2 * n].reshape(B, 2 * Cc, H, W)
    ref = fo.dft2(x.cpu())
    S, e_ref, bound = fo.rule(ref, x.cpu(), None, False)
    err = ((y[:, :Cc].double() - ref.real) ** 2 + (y[:, Cc:].double() - ref.imag) ** 2).sum((-2, -1)).sqrt()
    assert (err <= bound).all()
    for b, c in ((0, 0), (1, 3), (2, 4)):
        one_re, one_im = fft2(x[b:b + 1, c:c + 1].contiguous(), None, False)
        assert torch.equal(one_re.cpu()[0, 0], y[b, c]) and torch.equal(one_im.cpu()[0, 0], y[b, Cc + c])
    # the two-pass form: a plane alone against the same plane in a batch, and the real-output form through `work`
    big = torch.randn(2, 2, 128, 128, generator=torch.Generator().manual_seed(6)).cuda()
    all_re, all_im = fft2(big, None, False)
    one_re, one_im = fft2(big[1:, 1:].contiguous(), None, False)
    assert torch.equal(one_re[0, 0], all_re[1, 1]) and torch.equal(one_im[0, 0], all_im[1, 1])
    back, _ = fft2(all_re, all_im, True, 1.0, want_im=False)
    both, _ = fft2(all_re, all_im, True, 1.0, want_im=True)
    assert torch.equal(back, both) and torch.equal(back, fft2(all_re, all_im, True, 1.0, want_im=False)[0])


# ------------------------------------------------------------------------------------------------ operators on the device
def _rel_rule(x, inverse=False, im=None):
    r"""The rule's relative bound max(4 e_ref, 2 * 2^-24), the worst over the planes of ``x`` (host tensors)."""
    ref = fo.dft2(x, im, inverse)
    _, e_ref, _ = fo.rule(ref, x, im, inverse)
    return max(4 * float(e_ref.max()), 2 * fo.EPS)


@pytest.mark.parametrize("size", [(16, 16), (64, 32), (128, 256)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_operators_adjoint_inverse_and_flatten(size):
    from azula_amd.guidance import FourierOperator, MRIOperator, cartesian_mask

    H, W = size
    gen = torch.Generator().manual_seed(H + W)
    x, w = torch.randn(2, 3, H, W, generator=gen), torch.randn(2, 6, H, W, generator=gen)
    rel = max(_rel_rule(x), _rel_rule(w[:, :3], True, w[:, 3:]))
    norm2 = lambda v: float(v.double().pow(2).sum().sqrt())  # noqa: E731
    for norm in fc.NORMS:
        A = FourierOperator(norm)
        op_norm = math.sqrt(H * W) * fo.scale_of(norm, H * W)  # ||A||: sqrt(H W) times the scale
        y, g = A(x.cuda()), A.adjoint(w.cuda())
        assert y.shape == w.shape and g.shape == x.shape and y.dtype == torch.float32
        lhs, rhs = float((y.double().cpu() * w.double()).sum()), float((x.double() * g.double().cpu()).sum())
        print(f"adjointness {H}x{W} {norm}: |lhs - rhs| {abs(lhs - rhs):.3e} bound {rel * op_norm * norm2(x) * norm2(w):.3e}")
        assert abs(lhs - rhs) <= rel * op_norm * norm2(x) * norm2(w)
        # each plane of the result within the rule of the fp64 operator
        assert norm2(y.cpu() - fo.apply(x, norm)) <= rel * op_norm * norm2(x)
        back = A.pinv(y)
        err = (back.double().cpu() - x.double()).pow(2).sum((-2, -1)).sqrt()
        assert (err <= 2 * rel * x.double().pow(2).sum((-2, -1)).sqrt()).all(), norm  # A^+ A x = x: two transforms, twice the rule
        if norm == "ortho":
            assert torch.equal(back, A.adjoint(y))  # A^T A = I
        F = FourierOperator(norm, flatten=True)
        yf = F(x.cuda())
        assert yf.shape == (2, 6 * H * W) and torch.equal(yf, y.flatten(1))
        assert torch.equal(F.adjoint(yf), A.adjoint(y)) and torch.equal(F.adjoint(y), A.adjoint(y))
        assert torch.equal(F.pinv(yf), back)
    # the pseudo-inverse identities of 4x accelerated MRI: k transforms in an expression, k times the rule
    m = cartesian_mask(H, W, 4)
    A = MRIOperator(m)
    xd, zd = x.cuda(), w.cuda()
    y = A(xd)
    assert torch.equal(y, A.fourier(xd) * m.cuda())
    assert norm2(A(A.pinv(y)) - y) <= 3 * rel * norm2(x)  # A A^+ A = A
    p = A.pinv(zd)
    assert norm2(A.pinv(A(p)) - p) <= 3 * rel * norm2(w)  # A^+ A A^+ = A^+
    u = torch.randn(w.shape, generator=gen).cuda()
    lhs, rhs = float((A(A.pinv(zd)).double() * u.double()).sum()), float((zd.double() * A(A.pinv(u)).double()).sum())
    assert abs(lhs - rhs) <= 2 * rel * norm2(w) * norm2(u)  # (A A^+)^T = A A^+
    v = torch.randn(x.shape, generator=gen).cuda()
    lhs, rhs = float((A.pinv(A(xd)).double() * v.double()).sum()), float((xd.double() * A.pinv(A(v)).double()).sum())
    assert abs(lhs - rhs) <= 2 * rel * norm2(x) * norm2(v)  # (A^+ A)^T = A^+ A
    Af = MRIOperator(m, flatten=True)
    assert torch.equal(Af(xd), y.flatten(1)) and torch.equal(Af.adjoint(y.flatten(1)), A.adjoint(y))
    assert torch.equal(Af.pinv(y.flatten(1)), A.pinv(y))


def test_transforms_issue_the_same_launches(monkeypatch):
    from azula_amd.guidance import FourierOperator, MRIOperator, cartesian_mask

    gen = torch.Generator().manual_seed(9)
    x, w = torch.randn(2, 3, 32, 64, generator=gen).cuda(), torch.randn(2, 6, 32, 64, generator=gen).cuda()
    names = _spy(monkeypatch)
    for A, entries in ((FourierOperator("backward"), {"az_op_fft2_f32"}),
                       (MRIOperator(cartesian_mask(32, 64, 4)), {"az_op_fft2_f32", "az_op_mul_f32"})):
        y, want_t = A(x), A.adjoint(w)
        for fn in (lambda: torch.func.jvp(A, (x,), (x,))[1], lambda: A(x)):
            names.clear()
            assert torch.equal(fn(), y) and set(names) == entries
        xr = x.clone().requires_grad_()
        for fn in (lambda: torch.autograd.grad(A(xr), xr, w)[0], lambda: torch.func.vjp(A, x)[1](w)[0], lambda: A.T(w)):
            names.clear()
            assert torch.equal(fn(), want_t) and set(names) == entries
        names.clear()
        p = A.pinv(w)
        assert torch.equal(torch.func.jvp(A.pinv, (w,), (w,))[1], p) and set(names) == entries
        wr = w.clone().requires_grad_()
        assert torch.equal(torch.func.vjp(A.pinv, w)[1](x)[0], torch.autograd.grad(A.pinv(wr), wr, x)[0])


# --------------------------------------------------------------------------------------------------- dtype and size paths
def test_dtype_and_size_paths(monkeypatch):
    from azula_amd.guidance import FourierOperator

    A = FourierOperator()
    with pytest.raises(NotImplementedError, match="96 x 96"):
        A(torch.zeros(1, 1, 96, 96, device="cuda"))
    with pytest.raises(NotImplementedError, match="2048"):
        A.adjoint(torch.zeros(1, 2, 2, 2048, device="cuda"))
    names = _spy(monkeypatch)
    x = torch.randn(1, 2, 96, 96, dtype=F64, generator=torch.Generator().manual_seed(2))
    y = A(x.cuda())
    assert not names and y.dtype == F64 and float((y.cpu() - fo.apply(x)).abs().max()) < 1e-12
    with pytest.raises(NotImplementedError):
        A(torch.zeros(1, 1, 8, 8, device="cuda", dtype=torch.bfloat16))
    base = torch.randn(2, 3, 16, 32, generator=torch.Generator().manual_seed(3)).cuda()
    view = base.transpose(2, 3)  # (2, 3, 32, 16), not contiguous
    assert not view.is_contiguous()
    assert torch.equal(A(view), A(view.contiguous())) and names == ["az_op_fft2_f32"] * 2
    names.clear()
    tiny = torch.randn(1, 3, 1, 2, generator=torch.Generator().manual_seed(4)).cuda()  # C H W % 4 != 0: separate halves
    yt = A(tiny)
    assert names == ["az_op_fft2_f32"] and float((yt.double().cpu() - fo.apply(tiny.cpu())).abs().max()) < 1e-6
    assert float((A.adjoint(yt).double().cpu() - tiny.double().cpu()).abs().max()) < 1e-6


# ---------------------------------------------------------------------------------------------------------------- guidance
def _mri_setup(golden):
    from test_gpu_guidance_vjp import device_denoiser

    from azula_amd.guidance import MRIOperator, cartesian_mask

    g = golden("g28_guidance_vjp")
    mean64, _, arr64, sd, cfg = gc.setup(g, torch.float64)
    mean32, _, arr32, _, _ = gc.setup(g)
    H, W = g["x_t"].shape[2:]
    m = cartesian_mask(H, W, 4)

    def A_oracle(z):  # a torch.fft lambda, as a user would have written it
        f = torch.fft.fft2(z, norm="ortho")
        return (torch.cat([f.real, f.imag], dim=1) * m.to(z.dtype)).flatten(1)

    gen = torch.Generator().manual_seed(13)
    clean = A_oracle(torch.rand(g["x_t"].shape, generator=gen) - 0.5)
    y = clean + g.meta["var_y"] ** 0.5 * torch.randn(clean.shape, generator=gen)
    return g, device_denoiser(sd, cfg), MRIOperator(m, flatten=True), A_oracle, y, (mean64, arr64), (mean32, arr32)


def _check(tag, out, ref, ref32):
    assert out.shape == ref.shape and torch.isfinite(out).all()
    scale = float(ref.abs().max())
    err, e_ref = float((out.double().cpu() - ref).abs().max()) / scale, float((ref32.double() - ref).abs().max()) / scale
    print(f"{tag}: err {err:.3e} e_ref {e_ref:.3e} bound {max(4 * e_ref, 1e-4):.3e}")
    assert err < max(4 * e_ref, 1e-4)


def test_dps_mri_step(golden, monkeypatch):
    r"""One DPS step with ``MRIOperator(cartesian_mask(H, W, 4), flatten=True)`` on the fixture's denoiser, set up as
    ``test_dps_colourisation_step``: against the fp64 restatement with a ``torch.fft`` lambda as A, at max(4 e_ref, 1e-4)."""
    from test_gpu_guidance_vjp import SEED

    from azula_amd.guidance import DPSSampler

    g, den, A, A_oracle, y, (mean64, arr64), (mean32, arr32) = _mri_setup(golden)
    x_t, t, s = g["x_t"].cuda(), g["t"].cuda(), g["s"].cuda()
    torch.manual_seed(SEED)
    eps = torch.randn_like(x_t).cpu()
    torch.manual_seed(SEED)
    names = _spy(monkeypatch)
    out = DPSSampler(den, y.cuda(), A, steps=g.meta["steps"], silent=True).step(x_t, t, s)
    assert set(names) == {"az_op_fft2_f32", "az_op_mul_f32"}
    ref = go.dps_step(mean64, arr64["x_t"], arr64["t"], arr64["s"], eps.double(), y=y.double(), A=A_oracle)
    ref32 = go.dps_step(mean32, arr32["x_t"], arr32["t"], arr32["s"], eps, y=y, A=A_oracle)
    _check("dps mri", out, ref, ref32)


def test_mmps_mri_mean(golden, monkeypatch):
    r"""``MMPSDenoiser`` (cg, 2 iterations) with the same operator: ``autograd.grad`` on a retained graph and ``func.jvp``."""
    from azula_amd.guidance import MMPSDenoiser
    from azula_amd.linalg.covariance import IsotropicCovariance

    g, den, A, A_oracle, y, (mean64, arr64), (mean32, arr32) = _mri_setup(golden)
    var_y = g.meta["var_y"]
    names = _spy(monkeypatch)
    cov = IsotropicCovariance(torch.tensor(var_y, device="cuda"))
    out = MMPSDenoiser(den, y.cuda(), A, cov, solver="cg", iterations=2)(g["x_t"].cuda(), g["t"].cuda()).mean
    assert set(names) == {"az_op_fft2_f32", "az_op_mul_f32"}
    ref = go.mmps_mean(mean64, arr64["x_t"], arr64["t"], y.double(), A_oracle, lambda v: var_y * v, "cg", 2)
    ref32 = go.mmps_mean(mean32, arr32["x_t"], arr32["t"], y, A_oracle, lambda v: var_y * v, "cg", 2)
    _check("mmps mri", out, ref, ref32)
