r"""``az_op_coil_expand_f32``, ``az_op_coil_combine_f32`` and ``MultiCoilMRIOperator`` on the GPU against the fp64 oracle of
``tests/coil_oracle.py``.

* entries, exact: integers of magnitude at most 8 for image, coil data and maps, so every product and sum is exact in fp32 and the
  results EQUAL the oracle; real-image expand is bit-equal to torch's fp32 products on randn data;
* entries, float data: the standard bounds of an fma chain, per element, with ``u = 2^-24`` and ``gamma = 2 K u / (1 - 2 K u)``;
* entries, layout: guard words, a sample alone and in a batch, two runs, more items than one sweep of the grid, argument codes;
* the operator, per output plane: ``||got - ref64||_2 <= max(4 e_ref, 2 * 2^-24) S`` -- the rule and the margin of
  ``test_gpu_operators_fft.py`` -- with ``e_ref`` the loss of the torch fp32 host path on the same plane
  (``test_operators_coil_host.py`` asserts that it stays below 4e-7).  Measured ``err / (e_ref S)`` on an MI355X: DESIGN.md 9f;
* one DPS step, one MMPS mean and one PGDM step of 4-coil, 4x accelerated MRI of a colour image's two mixed channels on the
  ``g28_guidance_vjp`` fixture's UNet.
"""

import math

import pytest
import torch

import coil_cases as cc
import coil_oracle as co
import guidance_vjp_cases as gc
import guidance_vjp_oracle as go

pytestmark = pytest.mark.gpu
F64 = torch.float64
U = 2.0**-24


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


def _ptr(t):
    return None if t is None else t.data_ptr()


def expand(x_re, x_im, s_re, s_im):
    r"""``az_op_coil_expand_f32`` on contiguous device tensors: x (B, HW), maps (K, HW) or (B, K, HW) -> (B, K, HW) re, im."""
    from azula_amd import _lib

    (B, HW), K = x_re.shape, s_re.shape[-2]
    d_re, d_im = torch.empty(B, K, HW, device="cuda"), torch.empty(B, K, HW, device="cuda")
    _lib.call("az_op_coil_expand_f32", d_re.data_ptr(), d_im.data_ptr(), K * HW, x_re.data_ptr(), _ptr(x_im), HW, s_re.data_ptr(),
              s_im.data_ptr(), K * HW if s_re.ndim == 3 else 0, B, K, HW, _lib.stream_ptr())
    return d_re, d_im


def combine(z_re, z_im, s_re, s_im, want_im=True, normalize=False):
    r"""``az_op_coil_combine_f32`` on contiguous device tensors: z (B, K, HW) -> (B, HW) re and im (or None)."""
    from azula_amd import _lib

    B, K, HW = z_re.shape
    d_re, d_im = torch.empty(B, HW, device="cuda"), torch.empty(B, HW, device="cuda") if want_im else None
    _lib.call("az_op_coil_combine_f32", d_re.data_ptr(), _ptr(d_im), HW, z_re.data_ptr(), z_im.data_ptr(), K * HW, s_re.data_ptr(),
              s_im.data_ptr(), K * HW if s_re.ndim == 3 else 0, B, K, HW, int(normalize), _lib.stream_ptr())
    return d_re, d_im


def _dev(*ts):
    return tuple(None if t is None else t.cuda() for t in ts)


# ------------------------------------------------------------------------------------------------------- entries, exact
@pytest.mark.parametrize("K", cc.ENTRY_K)
def test_entries_equal_the_fp64_oracle_on_integers(K):
    for B in cc.ENTRY_B:
        for HW in cc.ENTRY_HW:
            for per_sample in (False, True):
                lead = (B, K) if per_sample else (K,)
                s_re, s_im = cc.ints(*lead, HW, seed=1), cc.ints(*lead, HW, seed=2)
                x_re, x_im = cc.ints(B, HW, seed=3), cc.ints(B, HW, seed=4)
                z_re, z_im = cc.ints(B, K, HW, seed=5), cc.ints(B, K, HW, seed=6)
                tag = (B, K, HW, per_sample)
                for im in (x_im, None):  # complex and real image
                    got_re, got_im = expand(*_dev(x_re, im, s_re, s_im))
                    ref_re, ref_im = co.expand(x_re, im, s_re, s_im)
                    assert torch.equal(got_re.double().cpu(), ref_re) and torch.equal(got_im.double().cpu(), ref_im), tag
                ref_re, ref_im = co.combine(z_re, z_im, s_re, s_im)
                for want_im in (True, False):  # dst_im = NULL: the real part only
                    got_re, got_im = combine(*_dev(z_re, z_im, s_re, s_im), want_im)
                    assert torch.equal(got_re.double().cpu(), ref_re), tag
                    assert got_im is None or torch.equal(got_im.double().cpu(), ref_im), tag
                # normalised: maps whose sum |S|^2 is 0 or a power of two keep the quotient exact
                if K in (1, 8):
                    e_re, e_im = (t.flatten(-2) for t in cc.exact_maps(K, 1, HW, seed=HW, batch=B if per_sample else None))
                    ref_re, ref_im = co.combine(z_re, z_im, e_re, e_im, normalize=True)
                    got_re, got_im = combine(*_dev(z_re, z_im, e_re, e_im), True, True)
                    assert torch.equal(got_re.double().cpu(), ref_re) and torch.equal(got_im.double().cpu(), ref_im), tag


def test_real_image_expand_is_bit_equal_to_torch_products():
    for K, HW in ((4, 16 * 16), (3, 7)):
        x = cc.randn(2, HW, seed=1).cuda()
        s_re, s_im = cc.randn(K, HW, seed=2).cuda(), cc.randn(K, HW, seed=3).cuda()
        got_re, got_im = expand(x, None, s_re, s_im)
        assert torch.equal(got_re, x[:, None] * s_re) and torch.equal(got_im, x[:, None] * s_im)


# -------------------------------------------------------------------------------------------------- entries, float data
@pytest.mark.parametrize("K", cc.FLOAT_K)
def test_entries_meet_the_fma_chain_bounds(K):
    r"""randn data and birdcage maps at 16 x 16 (and 5 x 3: the scalar form), B = 2.  The references are fp64 sums of the fp32
    inputs.  plain combine: ``|got - ref| <= gamma T`` with T the sum of the absolute values of the 2 K products of a component;
    normalised: ``gamma T / D + (gamma + 2 u)(|ref| + gamma T / D)`` (the chain of D's 2 K fmas, then one division);
    expand: ``2 u (|a c| + |b d|)`` (a rounded product inside one fma)."""
    from azula_amd.guidance import birdcage_maps

    gamma = 2 * K * U / (1 - 2 * K * U)
    for H, W in ((16, 16), (5, 3)):
        maps = birdcage_maps(K, H, W).to(torch.complex64).flatten(-2)
        s_re, s_im = maps.real.contiguous(), maps.imag.contiguous()
        z_re, z_im = cc.randn(2, K, H * W, seed=K), cc.randn(2, K, H * W, seed=K + 1)
        T_re, T_im, D = co.combine_bound(z_re, z_im, s_re, s_im)
        for normalize in (False, True):
            ref_re, ref_im = co.combine(z_re, z_im, s_re, s_im, normalize)
            got_re, got_im = combine(*_dev(z_re, z_im, s_re, s_im), True, normalize)
            for got, ref, T, part in ((got_re, ref_re, T_re, "re"), (got_im, ref_im, T_im, "im")):
                bound = gamma * T / D + (gamma + 2 * U) * (ref.abs() + gamma * T / D) if normalize else gamma * T
                ratio = float(((got.double().cpu() - ref).abs() / bound).max())
                print(f"combine K {K} {H}x{W} normalize {int(normalize)} {part}: worst err / bound {ratio:.3f}")
                assert ratio <= 1.0
        x_re, x_im = cc.randn(2, H * W, seed=K + 2), cc.randn(2, H * W, seed=K + 3)
        for im in (x_im, None):
            got_re, got_im = expand(*_dev(x_re, im, s_re, s_im))
            (ref_re, ref_im), (P_re, P_im) = co.expand(x_re, im, s_re, s_im), co.expand_bound(x_re, im, s_re, s_im)
            for got, ref, P in ((got_re, ref_re, P_re), (got_im, ref_im, P_im)):
                assert ((got.double().cpu() - ref).abs() <= 2 * U * P).all()


# ------------------------------------------------------------------------------------------------------ entries, layout
def test_strided_destination_guards_batches_and_determinism():
    r"""(B, K) = (3, 5) at 16 x 8 into the two halves of a (3, 10, 16, 8) destination whose samples lie 64 guard words apart, with
    64 more in front and behind; the combined (3, 2, 16, 8) image likewise; a sample alone gives the bits it has in the batch; two
    runs give the same bits."""
    from azula_amd import _lib

    B, K, HW, G = 3, 5, 16 * 8, 64
    n = K * HW
    x = cc.randn(B, 2, HW, seed=1).cuda()
    s = cc.randn(2, B, K, HW, seed=2).cuda()  # per-sample maps: (re | im)
    z = cc.randn(B, 2, K, HW, seed=3).cuda()
    for entry, planes in (("expand", n), ("combine", HW)):
        stride, runs = 2 * planes + G, []
        for _ in range(2):
            buf = torch.full((G + B * stride,), 7.5, device="cuda")
            base = buf.data_ptr() + 4 * G
            if entry == "expand":
                _lib.call("az_op_coil_expand_f32", base, base + 4 * n, stride, x.data_ptr(), x.data_ptr() + 4 * HW, 2 * HW,
                          s[0].data_ptr(), s[1].data_ptr(), n, B, K, HW, _lib.stream_ptr())
            else:
                _lib.call("az_op_coil_combine_f32", base, base + 4 * HW, stride, z.data_ptr(), z.data_ptr() + 4 * n, 2 * n,
                          s[0].data_ptr(), s[1].data_ptr(), n, B, K, HW, 1, _lib.stream_ptr())
            runs.append(buf.cpu())
        assert torch.equal(runs[0], runs[1])
        buf = runs[0]
        assert (buf[:G] == 7.5).all()
        body = buf[G:].reshape(B, stride)
        assert (body[:, 2 * planes:] == 7.5).all()
        got = body[:, :2 * planes].reshape(B, 2, planes).cuda()
        for b in range(B):  # the sample alone, from contiguous tensors
            if entry == "expand":
                one_re, one_im = expand(x[b:b + 1, 0].contiguous(), x[b:b + 1, 1].contiguous(), s[0, b:b + 1].contiguous(),
                                        s[1, b:b + 1].contiguous())
            else:
                one_re, one_im = combine(z[b:b + 1, 0].contiguous(), z[b:b + 1, 1].contiguous(), s[0, b:b + 1].contiguous(),
                                         s[1, b:b + 1].contiguous(), True, True)
            assert torch.equal(one_re.flatten(), got[b, 0]) and torch.equal(one_im.flatten(), got[b, 1]), (entry, b)
        ref = co.expand(x[:, 0].cpu(), x[:, 1].cpu(), s[0].cpu(), s[1].cpu()) if entry == "expand" else \
            co.combine(z[:, 0].cpu(), z[:, 1].cpu(), s[0].cpu(), s[1].cpu(), True)
        for part in (0, 1):
            assert float((got[:, part].double().cpu() - ref[part].reshape(B, planes)).abs().max()) <= 1e-5 * float(ref[part].abs().max())


def test_more_items_than_one_sweep_of_the_grid():
    B, K, HW = cc.SWEEP
    s_re, s_im = cc.ints(K, HW, seed=1), cc.ints(K, HW, seed=2)
    x_re, x_im = cc.ints(B, HW, seed=3), cc.ints(B, HW, seed=4)
    got_re, got_im = expand(*_dev(x_re, x_im, s_re, s_im))
    ref_re, ref_im = co.expand(x_re, x_im, s_re, s_im)
    assert torch.equal(got_re.cpu(), ref_re.float()) and torch.equal(got_im.cpu(), ref_im.float())
    back_re, back_im = combine(got_re, got_im, s_re.cuda(), s_im.cuda())  # |values| <= 128, products <= 1024, 4 of them: exact
    ref_re, ref_im = co.combine(ref_re, ref_im, s_re, s_im)
    assert torch.equal(back_re.cpu(), ref_re.float()) and torch.equal(back_im.cpu(), ref_im.float())


def test_argument_errors_return_codes_without_a_launch():
    from azula_amd import _lib

    cc.argument_errors(_lib.lib())
    torch.cuda.synchronize()  # (nothing was launched: nothing can have faulted)


# ------------------------------------------------------------------------------------------------------------ operator
@pytest.mark.parametrize("per_sample", [False, True], ids=["shared", "per-sample"])
@pytest.mark.parametrize("complex_image", [True, False], ids=["complex", "real"])
@pytest.mark.parametrize("size", cc.OPERATOR_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_operator_meets_the_accuracy_rule(size, complex_image, per_sample):
    from azula_amd.guidance import MultiCoilMRIOperator

    H, W = size
    x, w, maps, m = cc.operator_case(H, W, per_sample, complex_image)
    s_re, s_im = maps.real, maps.imag
    norm2 = lambda v: float(v.double().pow(2).sum().sqrt())  # noqa: E731
    for norm in cc.NORMS:
        A = MultiCoilMRIOperator(m, maps, norm, complex_image)
        y, g, r = A(x.cuda()), A.adjoint(w.cuda()), A.zero_filled(w.cuda())
        assert y.shape == w.shape and g.shape == x.shape == r.shape and y.dtype == torch.float32
        rel = 0.0
        for what, got, got32, ref in (("apply", y, A(x), co.apply(x, m, s_re, s_im, norm)),
                                      ("adjoint", g, A.adjoint(w), co.adjoint(w, m, s_re, s_im, norm, complex_image)),
                                      ("zero_filled", r, A.zero_filled(w), co.adjoint(w, m, s_re, s_im, norm, complex_image, True))):
            S, e_ref, bound = co.rule(ref, got32)
            err, _ = co.plane_loss(got.cpu(), ref)
            print(f"multi-coil {H}x{W} {norm} {what}: worst err/S {float((err / S).max()):.3e} e_ref {float(e_ref.max()):.3e} "
                  f"ratio err/(e_ref S) {float((err / (e_ref * S)).max()):.2f} err/bound {float((err / bound).max()):.3f}")
            assert (err <= bound).all(), (norm, what, (err / bound).tolist())
            if what != "zero_filled":
                assert float(e_ref.max()) <= cc.E_REF_MAX
                rel = max(rel, 4 * float(e_ref.max()), 2 * U)
        # adjointness in fp64 dot products of the device results.  Each side is within the rule of its fp64 value, plane by plane,
        # so ||y - A x|| <= rel ||A|| ||x|| and ||g - A^T w|| <= rel ||A|| ||w||; ||A|| <= max |M| sqrt(H W) s sqrt(max sum |S|^2).
        op_norm = float(m.max()) * math.sqrt(H * W) * A.fourier._scale(H * W, "apply") * math.sqrt(float(co.density(s_re, s_im).max()))
        lhs, rhs = float((y.double().cpu() * w.double()).sum()), float((x.double() * g.double().cpu()).sum())
        print(f"adjointness {H}x{W} {norm}: |lhs - rhs| {abs(lhs - rhs):.3e} bound {2 * rel * op_norm * norm2(x) * norm2(w):.3e}")
        assert abs(lhs - rhs) <= 2 * rel * op_norm * norm2(x) * norm2(w)
        F = MultiCoilMRIOperator(m, maps, norm, complex_image, flatten=True)  # the flatten round trip
        yf = F(x.cuda())
        assert yf.shape == (x.shape[0], w[0].numel()) and torch.equal(yf, y.flatten(1))
        assert torch.equal(F.adjoint(yf), A.adjoint(y)) and torch.equal(F.adjoint(y), A.adjoint(y))
        assert torch.equal(F.zero_filled(yf), A.zero_filled(y))


def test_transforms_issue_the_same_launches(monkeypatch):
    from azula_amd.guidance import MultiCoilMRIOperator

    fwd = ["az_op_coil_expand_f32", "az_op_fft2_f32", "az_op_mul_f32"]
    back = ["az_op_mul_f32", "az_op_fft2_f32", "az_op_coil_combine_f32"]
    names = _spy(monkeypatch)
    for complex_image in (True, False):
        x, w, maps, m = cc.operator_case(32, 64, True, complex_image)
        x, w = x.cuda(), w.cuda()
        A = MultiCoilMRIOperator(m, maps, "backward", complex_image)
        y, want_t, want_z = A(x), A.adjoint(w), A.zero_filled(w)
        for fn in (lambda: torch.func.jvp(A, (x,), (x,))[1], lambda: A(x)):
            names.clear()
            assert torch.equal(fn(), y) and set(names) == set(fwd) and names[-3:] == fwd
        xr = x.clone().requires_grad_()
        for fn, entries in ((lambda: torch.autograd.grad(A(xr), xr, w)[0], fwd + back), (lambda: torch.func.vjp(A, x)[1](w)[0], fwd + back),
                            (lambda: A.T(w), back)):
            names.clear()
            assert torch.equal(fn(), want_t) and set(names) == set(entries) and names[-3:] == back
        names.clear()
        assert torch.equal(torch.func.jvp(A.zero_filled, (w,), (w,))[1], want_z) and set(names) == set(back)
        wr = w.clone().requires_grad_()
        assert torch.equal(torch.func.vjp(A.zero_filled, w)[1](x)[0], torch.autograd.grad(A.zero_filled(wr), wr, x)[0])
        assert names[-3:] == fwd
        assert torch.equal(A(x), y) and torch.equal(A.adjoint(w), want_t)  # two runs give the same bits


def test_dtype_and_size_paths(monkeypatch):
    from azula_amd.guidance import MultiCoilMRIOperator, birdcage_maps

    K = 3
    A = MultiCoilMRIOperator(torch.ones(96, 96), birdcage_maps(K, 96, 96))
    with pytest.raises(NotImplementedError, match="96 x 96"):
        A(torch.zeros(1, 2, 96, 96, device="cuda"))
    with pytest.raises(NotImplementedError, match="96 x 96"):
        A.zero_filled(torch.zeros(1, 2 * K, 96, 96, device="cuda"))
    names = _spy(monkeypatch)
    x = cc.randn(1, 2, 96, 96, seed=2, dtype=F64)
    s = birdcage_maps(K, 96, 96)
    y = A(x.cuda())  # fp64 on the device: the torch path, at any size
    ref = co.apply(x, torch.ones(96, 96), s.real, s.imag)
    assert not names and y.dtype == F64 and float((y.cpu() - ref).abs().max()) < 1e-12 * float(ref.abs().max())
    with pytest.raises(NotImplementedError):
        A(torch.zeros(1, 2, 96, 96, device="cuda", dtype=torch.bfloat16))
    m = torch.ones(16, 32)
    B = MultiCoilMRIOperator(m, birdcage_maps(K, 16, 32))
    base = cc.randn(2, 2, 32, 16, seed=3).cuda()
    view = base.transpose(2, 3)  # (2, 2, 16, 32), not contiguous
    assert not view.is_contiguous()
    assert torch.equal(B(view), B(view.contiguous())) and names == ["az_op_coil_expand_f32", "az_op_fft2_f32", "az_op_mul_f32"] * 2
    names.clear()
    t = birdcage_maps(K, 1, 2)  # K H W % 4 != 0: separate halves, and the entries' scalar form
    T = MultiCoilMRIOperator(torch.ones(1, 2), t)
    tiny = cc.randn(2, 2, 1, 2, seed=4)
    yt = T(tiny.cuda())
    ref = co.apply(tiny, torch.ones(1, 2), t.real, t.imag)
    assert names == ["az_op_coil_expand_f32", "az_op_fft2_f32", "az_op_mul_f32"]
    assert float((yt.double().cpu() - ref).abs().max()) < 1e-6
    assert float((T.zero_filled(yt).double().cpu() - tiny.double()).abs().max()) < 1e-6  # full sampling: the inverse
    assert T(torch.zeros(0, 2, 1, 2, device="cuda")).shape == (0, 2 * K, 1, 2)  # empty: nothing is launched
    assert T.adjoint(torch.zeros(0, 2 * K, 1, 2, device="cuda")).shape == (0, 2, 1, 2) and len(names) == 6


# ---------------------------------------------------------------------------------------------------------------- guidance
MIX = [[0.5, 0.25, -0.25], [-0.125, 0.5, 0.375]]  # the fixed 2 x 3 channel mix: 3 colour channels -> re | im of one complex image


def _sense_setup(golden):
    r"""As ``_mri_setup`` of ``test_gpu_operators_fft.py``, with A = (4-coil SENSE, 4x accelerated) @ (the 2 x 3 channel mix)."""
    from test_gpu_guidance_vjp import device_denoiser

    from azula_amd.guidance import ChannelMixOperator, MultiCoilMRIOperator, birdcage_maps, cartesian_mask

    g = golden("g28_guidance_vjp")
    mean64, _, arr64, sd, cfg = gc.setup(g, torch.float64)
    mean32, _, arr32, _, _ = gc.setup(g)
    H, W = g["x_t"].shape[2:]
    m, maps, M = cartesian_mask(H, W, 4), birdcage_maps(4, H, W), torch.tensor(MIX, dtype=F64)
    A_mc, mix = MultiCoilMRIOperator(m, maps, flatten=True, in_shape=(2, H, W)), ChannelMixOperator(M)
    M_pinv = torch.linalg.pinv(M)
    D = (maps.real**2 + maps.imag**2).sum(0)

    def A_oracle(z):  # a torch lambda, as a user would have written it: channel mix, complex multiply, torch.fft, mask
        c = torch.einsum("oc,bchw->bohw", M.to(z.dtype), z)
        s = maps.to(torch.complex64 if z.dtype == torch.float32 else torch.complex128)
        f = torch.fft.fft2(s * torch.complex(c[:, 0], c[:, 1])[:, None], norm="ortho")
        return (torch.cat([f.real, f.imag], dim=1) * m.to(z.dtype)).flatten(1)

    def A_inv_oracle(v):  # the coil-combined zero-filled reconstruction, then the mix's pseudo-inverse
        v = v.unflatten(1, (8, H, W)) * m.to(v.dtype)
        s = maps.to(torch.complex64 if v.dtype == torch.float32 else torch.complex128)
        img = (s.conj() * torch.fft.ifft2(torch.complex(v[:, :4], v[:, 4:]), norm="ortho")).sum(1) / D.to(v.dtype)
        return torch.einsum("co,bohw->bchw", M_pinv.to(v.dtype), torch.stack([img.real, img.imag], dim=1))

    gen = torch.Generator().manual_seed(13)
    clean = A_oracle(torch.rand(g["x_t"].shape, generator=gen) - 0.5)
    y = clean + g.meta["var_y"] ** 0.5 * torch.randn(clean.shape, generator=gen)
    A_inv = lambda v: mix.pinv(A_mc.zero_filled(v))  # noqa: E731
    return g, device_denoiser(sd, cfg), A_mc @ mix, A_inv, A_oracle, A_inv_oracle, y, (mean64, arr64), (mean32, arr32)


def _check(tag, out, ref, ref32):
    assert out.shape == ref.shape and torch.isfinite(out).all()
    scale = float(ref.abs().max())
    err, e_ref = float((out.double().cpu() - ref).abs().max()) / scale, float((ref32.double() - ref).abs().max()) / scale
    print(f"{tag}: err {err:.3e} e_ref {e_ref:.3e} bound {max(4 * e_ref, 1e-4):.3e}")
    assert err < max(4 * e_ref, 1e-4)


FWD = {"az_op_chanmix_f32", "az_op_coil_expand_f32", "az_op_fft2_f32", "az_op_mul_f32"}


def test_dps_sense_step(golden, monkeypatch):
    r"""One DPS step, set up and bounded as ``test_dps_mri_step``: against the fp64 restatement with a torch lambda as A, at
    max(4 e_ref, 1e-4) of the fp64 maximum, ``e_ref`` the restatement's own fp32 loss."""
    from test_gpu_guidance_vjp import SEED

    from azula_amd.guidance import DPSSampler

    g, den, A, _, A_oracle, _, y, (mean64, arr64), (mean32, arr32) = _sense_setup(golden)
    x_t, t, s = g["x_t"].cuda(), g["t"].cuda(), g["s"].cuda()
    torch.manual_seed(SEED)
    eps = torch.randn_like(x_t).cpu()
    torch.manual_seed(SEED)
    names = _spy(monkeypatch)
    out = DPSSampler(den, y.cuda(), A, steps=g.meta["steps"], silent=True).step(x_t, t, s)
    assert set(names) == FWD | {"az_op_coil_combine_f32"}
    ref = go.dps_step(mean64, arr64["x_t"], arr64["t"], arr64["s"], eps.double(), y=y.double(), A=A_oracle)
    ref32 = go.dps_step(mean32, arr32["x_t"], arr32["t"], arr32["s"], eps, y=y, A=A_oracle)
    _check("dps sense", out, ref, ref32)


def test_mmps_sense_mean(golden, monkeypatch):
    r"""``MMPSDenoiser`` (cg, 2 iterations) with the same operator: ``autograd.grad`` on a retained graph and ``func.jvp``."""
    from azula_amd.guidance import MMPSDenoiser
    from azula_amd.linalg.covariance import IsotropicCovariance

    g, den, A, _, A_oracle, _, y, (mean64, arr64), (mean32, arr32) = _sense_setup(golden)
    var_y = g.meta["var_y"]
    names = _spy(monkeypatch)
    cov = IsotropicCovariance(torch.tensor(var_y, device="cuda"))
    out = MMPSDenoiser(den, y.cuda(), A, cov, solver="cg", iterations=2)(g["x_t"].cuda(), g["t"].cuda()).mean
    assert set(names) == FWD | {"az_op_coil_combine_f32"}
    ref = go.mmps_mean(mean64, arr64["x_t"], arr64["t"], y.double(), A_oracle, lambda v: var_y * v, "cg", 2)
    ref32 = go.mmps_mean(mean32, arr32["x_t"], arr32["t"], y, A_oracle, lambda v: var_y * v, "cg", 2)
    _check("mmps sense", out, ref, ref32)


def test_pgdm_sense_step(golden, monkeypatch):
    r"""One ``PGDMSampler`` step with ``A_inv = lambda y: M_pinv(A_mc.zero_filled(y))``."""
    from test_gpu_guidance_vjp import SEED

    from azula_amd.guidance import PGDMSampler

    g, den, A, A_inv, A_oracle, A_inv_oracle, y, (mean64, arr64), (mean32, arr32) = _sense_setup(golden)
    x_t, t, s = g["x_t"].cuda(), g["t"].cuda(), g["s"].cuda()
    torch.manual_seed(SEED)
    eps = torch.randn_like(x_t).cpu()
    torch.manual_seed(SEED)
    names = _spy(monkeypatch)
    out = PGDMSampler(den, y.cuda(), A, A_inv, steps=g.meta["steps"], silent=True).step(x_t, t, s)
    assert set(names) == FWD | {"az_op_coil_combine_f32"}
    ref = go.pgdm_step(mean64, arr64["x_t"], arr64["t"], arr64["s"], eps.double(), y=y.double(), A=A_oracle, A_inv=A_inv_oracle)
    ref32 = go.pgdm_step(mean32, arr32["x_t"], arr32["t"], arr32["s"], eps, y=y, A=A_oracle, A_inv=A_inv_oracle)
    _check("pgdm sense", out, ref, ref32)
