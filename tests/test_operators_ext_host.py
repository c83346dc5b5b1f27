r"""``PSFOperator``, ``DecimateOperator`` and ``ChannelMixOperator`` without a GPU: the torch path EQUAL to the oracle on the exact
data and adjoint in fp64, pseudo-inverses, the helpers ``motion_psf`` and ``bicubic_taps``, the shape conventions and their
errors, the autograd Function under every transform the guidance classes use (on a stand-in launcher that reads raw pointers,
as the real one does), and the argument codes of the new C entries."""

import ctypes as C

import numpy as np
import pytest
import torch

import operator_cases as oc
import operator_ext_cases as xc
import operator_ext_oracle as xo
import operator_oracle as oo
from azula_amd.guidance import (BlurOperator, ChannelMixOperator, DecimateOperator, DownsampleOperator, MaskOperator, PSFOperator,
                                bicubic_taps, motion_psf)
from azula_amd.guidance import operators as ops

F64 = torch.float64


@pytest.fixture(autouse=True)
def _grad_mode_on():
    r"""Some modules of the suite switch grad mode off for the whole process; these tests differentiate."""
    with torch.enable_grad():
        yield


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def _psf_reference(psfs, x, B, Cc, form, circ):
    r"""The oracle's result for a (B, C) input under ``form``: PSF number ``psf_number`` on every plane."""
    k = torch.stack([torch.stack([psfs[xc.psf_number(form, b, c, Cc)] for c in range(Cc)]) for b in range(B)])
    return lambda z: xo.psf(z, k, circ)


# ------------------------------------------------------------------------------------------------------- the torch path
@pytest.mark.parametrize("padding", oc.PADDINGS)
def test_psf_torch_path_equals_the_fp64_oracle_on_exact_data(padding):
    circ = padding == "circular"
    for rh, rw in ((0, 0), (1, 0), (0, 2), (1, 2), (3, 1)):
        kh, kw = 2 * rh + 1, 2 * rw + 1
        psfs = xc.exact_psfs(kh, kw)
        for B, Cc in xc.PSF_BC:
            x, w = oc.exact_image(B, Cc, 5, 4, seed=B), oc.exact_image(B, Cc, 5, 4, seed=Cc + 10)
            for form in xc.PSF_FORMS:
                A = PSFOperator(xc.psf_argument(psfs, form, B, Cc), padding=padding)
                ref = _psf_reference(psfs, x, B, Cc, form, circ)
                want, want_t = ref(x.double()), oo.adjoint(ref, x.shape, w.double())
                for dtype in (F64, torch.float32):
                    y, g = A(x.to(dtype)), A.adjoint(w.to(dtype))
                    assert y.dtype == dtype and g.dtype == dtype
                    assert torch.equal(y.double(), want) and torch.equal(g.double(), want_t), (rh, rw, B, Cc, form)
                    assert torch.equal(A.T(w.to(dtype)).double(), want_t) and A.T.T is A


def test_decimate_torch_path_equals_the_oracle():
    for fh, fw in xc.DEC_FACTORS:
        for oh, ow in xc.offsets(fh, fw):
            A = DecimateOperator((fh, fw), (oh, ow))
            for Ho, Wo in xc.DEC_OUTPUTS[:4]:
                x, w = oc.random_image(2, 3, Ho * fh, Wo * fw, seed=Ho).double(), oc.random_image(2, 3, Ho, Wo, seed=Wo).double()
                ref = lambda z: xo.decimate(z, fh, fw, oh, ow)  # noqa: E731, B023
                assert torch.equal(A(x), ref(x)) and A(x).shape == (2, 3, Ho, Wo)
                assert torch.equal(A.adjoint(w), oo.adjoint(ref, x.shape, w))
                assert torch.equal(A.adjoint(w), xo.zero_stuff(w, fh, fw, oh, ow)) and torch.equal(A.pinv(w), A.adjoint(w))
                assert torch.equal(A(A.pinv(A(x))), A(x)) and torch.equal(A(A.adjoint(w)), w)  # A A^T = I


def test_mix_torch_path_equals_the_fp64_oracle_on_exact_data():
    for k, (Cin, Cout) in enumerate(xc.MIX_CHANNELS):
        M = xc.exact_matrix(Cout, Cin, k)
        A = ChannelMixOperator(M)
        x, w = oc.exact_image(2, Cin, 3, 5, seed=k), oc.exact_image(2, Cout, 3, 5, seed=k + 20)
        ref = lambda z: xo.mix(z, M)  # noqa: E731, B023
        for dtype in (F64, torch.float32):
            assert torch.equal(A(x.to(dtype)).double(), ref(x.double())), (Cin, Cout)
            assert torch.equal(A.adjoint(w.to(dtype)).double(), oo.adjoint(ref, x.shape, w.double())), (Cin, Cout)


def test_dyadic_pseudo_inverses_are_exact():
    r"""The matrices the GPU test applies ``pinv`` with: their pseudo-inverse, as the operator forms it, is dyadic and exact in
    fp32, and on exact data ``pinv`` EQUALS the oracle with the hand-written pseudo-inverse."""
    for k, (M, P) in enumerate(zip(xc.MIX_PINV, xc.MIX_PINV_BY_HAND)):
        M, P = torch.tensor(M, dtype=F64), torch.tensor(P, dtype=F64)
        assert torch.allclose(torch.linalg.pinv(M), P, atol=1e-14, rtol=0)
        A = ChannelMixOperator(M)
        y = oc.exact_image(2, M.shape[0], 3, 4, seed=k)
        assert torch.equal(A._matrix(y, "pinv").double(), P) and torch.equal(A._matrix(y, "pinv_t").double(), P.T)
        assert torch.equal(A.pinv(y).double(), xo.mix(y.double(), P))
        if torch.linalg.matrix_rank(M) == M.shape[0]:  # full row rank: A A^+ = I
            x = oc.exact_image(2, M.shape[1], 3, 4, seed=k + 5)
            assert torch.equal(A(A.pinv(A(x))), A(x))
    A = ChannelMixOperator([[1, 0, 0], [0, 1, 1]])
    x = oc.exact_image(2, 3, 4, 4, seed=9)
    assert torch.equal(A(A.pinv(A(x))), A(x))
    with pytest.raises(NotImplementedError):
        PSFOperator(torch.ones(3, 3)).pinv(x)


def _operators(C_, H, W, flatten=False, exact=False):
    r"""(name, operator, oracle map) for a (2, C, H, W) input: the new operators and compositions with the existing ones."""
    k1 = xc.exact_psf(3, 5) if exact else xc.random_psf(3, 5, seed=1)
    kb = xc.exact_psfs(5, 3)[:2].reshape(2, 1, 5, 3) if exact else xc.random_psf(2, 1, 5, 3, seed=2)
    M = (xc.exact_matrix(2, C_, 1) if exact else xc.random_matrix(2, C_, 1)).double()
    taps = oc.exact_taps(5) if exact else bicubic_taps(2)
    m = (torch.rand((1, C_, H, W), generator=torch.Generator().manual_seed(7)) < 0.6).float()
    out = [("decimate", DecimateOperator((2, 3), (1, 2), flatten=flatten), lambda x: xo.decimate(x, 2, 3, 1, 2)),
           ("mix", ChannelMixOperator(M, flatten=flatten), lambda x: xo.mix(x, M))]
    for pad in oc.PADDINGS:
        out.append((f"psf_{pad}", PSFOperator(k1, padding=pad, flatten=flatten), lambda x, pad=pad: xo.psf(x, k1, pad == "circular")))
    out.append(("psf_per_sample", PSFOperator(kb, flatten=flatten), lambda x: xo.psf(x, kb, False)))
    out.append(("bicubic", DecimateOperator(2, 1, flatten=flatten) @ BlurOperator(taps),
                lambda x: xo.decimate(oo.blur(x, taps, taps, False), 2, 2, 1, 1)))
    out.append(("mix_of_psf", ChannelMixOperator(M, flatten=flatten) @ PSFOperator(k1), lambda x: xo.mix(xo.psf(x, k1, False), M)))
    out.append(("pool_of_psf", DownsampleOperator(2, flatten=flatten) @ PSFOperator(k1), lambda x: oo.pool(xo.psf(x, k1, False), 2, 2)))
    out.append(("psf_of_mask", PSFOperator(k1, flatten=flatten) @ MaskOperator(m), lambda x: xo.psf(oo.mask(x, m), k1, False)))
    return out


@pytest.mark.parametrize("flatten", [False, True])
def test_adjoints_flatten_and_composition_in_fp64(flatten):
    B, C_, H, W = 2, 3, 8, 6
    x = oc.random_image(B, C_, H, W, seed=1).double()
    for name, A, ref in _operators(C_, H, W, flatten):
        want = ref(x)
        w = oc.random_image(*want.shape, seed=2).double()
        y = A(x)
        assert y.dtype == F64 and y.shape == ((B, want[0].numel()) if flatten else want.shape), name
        assert _rel(y.reshape(want.shape), want) < 1e-14, name
        want_t = oo.adjoint(ref, x.shape, w)
        for v in (w, w.flatten(1)) if flatten else (w,):  # the flat and the image shape
            assert _rel(A.adjoint(v), want_t) < 1e-14 and _rel(A.T(v), want_t) < 1e-14, name
        lhs, rhs = float((y.reshape(want.shape) * w).sum()), float((x * A.adjoint(w)).sum())
        assert abs(lhs - rhs) <= 1e-12 * float(y.abs().sum() * w.abs().max()), name  # <A x, w> == <x, A^T w>
        xr = x.clone().requires_grad_()  # torch differentiates the torch path itself
        assert _rel(torch.autograd.grad(A(xr), xr, w.reshape(A(xr).shape))[0], want_t) < 1e-14, name


def test_flat_observations_need_the_image_shape():
    x = torch.zeros(2, 3, 8, 6)
    for A, n in ((DecimateOperator(2, 1, flatten=True), 3 * 4 * 3), (ChannelMixOperator.grayscale(flatten=True), 48),
                 (PSFOperator(torch.ones(3, 3), flatten=True), 144)):
        v = torch.zeros(2, n)
        with pytest.raises(ValueError, match="in_shape"):
            A.adjoint(v)
        assert A(x).shape == v.shape and A.adjoint(v).shape == x.shape and A.T(v).shape == x.shape
        with pytest.raises(ValueError, match="flattened"):
            A.adjoint(v[:, :-1])
    D = DecimateOperator(2, flatten=True, in_shape=(3, 8, 6))
    assert D.adjoint(torch.zeros(2, 36)).shape == x.shape and D.pinv(torch.zeros(2, 36)).shape == x.shape
    G = ChannelMixOperator.grayscale(flatten=True, in_shape=(3, 8, 6))
    assert G.pinv(torch.zeros(2, 48)).shape == x.shape


def test_constructor_and_shape_errors():
    x = torch.zeros(2, 3, 8, 6)
    for A in (PSFOperator(torch.ones(3, 3)), DecimateOperator(2), ChannelMixOperator.grayscale()):
        for bad in (x[0], x.flatten(1), x[None]):
            with pytest.raises(ValueError, match="B, C, H, W"):
                A(bad)
    for bad in (torch.ones(2, 3), torch.ones(3, 4), torch.ones(67, 3), torch.ones(3, 67), torch.ones(3), torch.ones(1, 1, 1, 3, 3)):
        with pytest.raises(ValueError, match="odd"):
            PSFOperator(bad)
    with pytest.raises(ValueError, match="padding"):
        PSFOperator(torch.ones(3, 3), padding="reflect")
    with pytest.raises(ValueError, match="circular"):
        PSFOperator(torch.ones(3, 13), padding="circular")(x)  # radius 6 >= W = 6
    assert PSFOperator(torch.ones(3, 11), padding="circular")(x).shape == x.shape
    with pytest.raises(ValueError, match="channels"):
        PSFOperator(torch.ones(2, 3, 3))(x)
    with pytest.raises(ValueError, match="batch"):
        PSFOperator(torch.ones(3, 1, 3, 3))(x)
    with pytest.raises(ValueError, match="batch"):
        PSFOperator(torch.ones(3, 3, 3, 3)).adjoint(x)
    assert PSFOperator(torch.ones(2, 3, 3, 3))(x).shape == x.shape and PSFOperator(torch.ones(2, 1, 3, 3))(x).shape == x.shape
    for factor, offset in ((17, 0), (0, 0), ((2, 17), 0), (2, 2), (2, -1), ((2, 3), (1, 3)), (2.0, 0)):
        with pytest.raises(ValueError):
            DecimateOperator(factor, offset)
    with pytest.raises(ValueError, match="multiples"):
        DecimateOperator(4)(x)
    with pytest.raises(ValueError, match="multiples"):
        DecimateOperator((2, 4))(x)
    for bad in (torch.ones(3), torch.ones(17, 3), torch.ones(3, 17), torch.ones(1, 2, 3)):
        with pytest.raises(ValueError, match="Cout, Cin"):
            ChannelMixOperator(bad)
    with pytest.raises(ValueError, match="channels"):
        ChannelMixOperator(torch.ones(2, 4))(x)
    with pytest.raises(ValueError, match="channels"):
        ChannelMixOperator(torch.ones(2, 3)).adjoint(x)
    with pytest.raises(ValueError, match="channels"):
        ChannelMixOperator(torch.ones(2, 3)).pinv(x)
    G = ChannelMixOperator.grayscale()
    assert G(x).shape == (2, 1, 8, 6) and G.adjoint(G(x)).shape == x.shape and G.pinv(G(x)).shape == x.shape
    assert torch.equal(G.matrix, torch.full((1, 3), 1 / 3, dtype=F64))
    assert torch.equal(ChannelMixOperator.grayscale((0.299, 0.587, 0.114)).matrix, torch.tensor([[0.299, 0.587, 0.114]], dtype=F64))


def test_half_and_host_fp32_run_the_torch_path(monkeypatch):
    monkeypatch.setattr(ops, "_launch", lambda *a: pytest.fail("a host tensor reached the kernels"))
    x = oc.exact_image(1, 3, 4, 4)
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        for A in (PSFOperator(xc.exact_psf(3, 3)), DecimateOperator(2, 1), ChannelMixOperator([[1, 0, 0], [0, 1, 1]])):
            y = A(x.to(dtype))
            assert y.dtype == dtype and A.adjoint(y).dtype == dtype
    xt = oc.exact_image(1, 3, 4, 4).transpose(2, 3)  # non-contiguous
    assert torch.equal(PSFOperator(xc.exact_psf(3, 3))(xt), xo.psf(xt, xc.exact_psf(3, 3), False))


# --------------------------------------------------------------------------------------------------------------- helpers
def test_bicubic_taps():
    for f in (1, 2, 3, 4, 8, 16):
        t = bicubic_taps(f)
        assert t.dtype == torch.float32 and t.shape == (4 * f + 1,)
        assert abs(float(t.double().sum()) - 1) <= (4 * f + 1) * 2.0**-25  # each rounding moves the sum by at most 2^-25
        assert torch.equal(t, t.flip(0)) and t.argmax() == 2 * f and t[0] == 0 and t[-1] == 0
    assert torch.equal(bicubic_taps(1), torch.tensor([0.0, 0, 1, 0, 0]))
    # Keys, a = -0.5, at |t| = 1/2 and 3/2: 9/16 and -1/16; the five taps at factor 2 sum to 2 before normalisation
    assert torch.equal(bicubic_taps(2), torch.tensor([0, -1 / 32, 0, 9 / 32, 0.5, 9 / 32, 0, -1 / 32, 0]))
    for bad in (0, 17, 2.0):
        with pytest.raises(ValueError):
            bicubic_taps(bad)
    # bicubic super-resolution as the docstring states it: a constant image stays constant away from the border
    A = DecimateOperator(2, 1) @ BlurOperator(bicubic_taps(2))
    y = A(torch.ones(1, 1, 16, 16, dtype=F64))
    assert y.shape == (1, 1, 8, 8) and torch.allclose(y[:, :, 2:-2, 2:-2], torch.ones(1, 1, 4, 4, dtype=F64), atol=1e-6)


def test_motion_psf():
    for length, size in ((1, 1), (9, 9), (5, 9), (31.5, 61), (61, 61)):
        k = motion_psf(length, 0.0, size)
        assert k.dtype == torch.float32 and k.shape == (size, size)
        assert abs(float(k.double().sum()) - 1) <= size * 2.0**-25
        rows = k.abs().sum(1).nonzero().flatten()
        assert rows.tolist() == [size // 2], (length, size)  # angle 0: one row
        assert torch.equal(k, k.flip(1)) and (k >= 0).all()
        lit = (k[size // 2] > 0).nonzero().flatten()  # the pixels the segment of `length` pixels touches, and no others
        assert int(lit[-1] - lit[0]) + 1 == 2 * int(np.ceil((length - 1) / 2)) + 1, (length, size)
    assert torch.equal(motion_psf(9, 90.0, 9).abs().sum(0).nonzero().flatten(), torch.tensor([4]))  # vertical: one column
    k = motion_psf(9, 30.0, 9)
    assert torch.equal(k, motion_psf(9, 30.0, 9)) and (k >= 0).all()  # deterministic
    assert torch.equal(k, k.flip(0, 1))  # a centred segment: point symmetric
    assert k[0, 8] > 0 or k[1, 8] > 0 or k[2, 8] > 0 or k[2, 7] > 0  # counter-clockwise: the right end points up
    assert float(k[5:, 6:].sum()) == 0 and not torch.equal(k, motion_psf(9, -30.0, 9))
    assert torch.equal(motion_psf(1, 77.0, 5), torch.zeros(5, 5).index_put((torch.tensor(2), torch.tensor(2)), torch.tensor(1.0)))
    for length, size in ((0.5, 5), (7, 5), (3, 4), (3, 0)):
        with pytest.raises(ValueError):
            motion_psf(length, 0.0, size)


# ----------------------------------------------------------------------------------------------- the autograd Function
def _f32(ptr, n):
    return np.ctypeslib.as_array((C.c_float * n).from_address(ptr))


def _raw_launch(name, *a):
    r"""What the kernels compute, from raw pointers alone -- a functorch wrapper has none to give."""
    if name == "az_op_psf_f32":
        y, x, psf, kh, kw, bs, cs, B, Cc, H, W, circular = a
        src = _f32(x, B * Cc * H * W).reshape(B, Cc, H, W)
        k = _f32(psf, ((B - 1) * bs + (Cc - 1) * cs + 1) * kh * kw).reshape(-1, kh, kw)
        pad = ((0, 0), (0, 0), (kh // 2, kh // 2), (kw // 2, kw // 2))
        src = np.pad(src, pad, mode="wrap") if circular else np.pad(src, pad)
        out = np.zeros((B, Cc, H, W), np.float32)
        for b in range(B):
            for c in range(Cc):
                for i in range(kh):
                    for j in range(kw):
                        out[b, c] += k[b * bs + c * cs, i, j] * src[b, c, i:i + H, j:j + W]
        _f32(y, B * Cc * H * W)[:] = out.ravel()
    elif name == "az_op_decimate_f32":
        y, x, planes, H, W, fh, fw, oh, ow = a
        _f32(y, planes * (H // fh) * (W // fw))[:] = _f32(x, planes * H * W).reshape(planes, H, W)[:, oh::fh, ow::fw].ravel()
    elif name == "az_op_decimate_adj_f32":
        dx, g, planes, H, W, fh, fw, oh, ow = a
        out = np.zeros((planes, H, W), np.float32)
        out[:, oh::fh, ow::fw] = _f32(g, planes * (H // fh) * (W // fw)).reshape(planes, H // fh, W // fw)
        _f32(dx, planes * H * W)[:] = out.ravel()
    elif name == "az_op_chanmix_f32":
        y, x, M, B, Cin, Cout, HW = a
        m = _f32(M, Cout * Cin).reshape(Cout, Cin)
        _f32(y, B * Cout * HW)[:] = np.einsum("oc,bcp->bop", m, _f32(x, B * Cin * HW).reshape(B, Cin, HW)).ravel()
    else:
        from test_operators_host import _raw_launch as earlier

        earlier(name, *a)


@pytest.mark.parametrize("flatten", [False, True])
def test_transforms_never_hand_the_launcher_a_wrapped_tensor(monkeypatch, flatten):
    r"""The method of ``test_operators_host.py`` for the new classes: the kernel path forced onto host tensors with a launcher
    that consumes ``data_ptr()``.  Under ``torch.func.jvp`` / ``vjp`` the tensors that ``backward`` and ``jvp`` of the Function
    receive are wrappers without storage; as applications of the Function they reach ``forward`` unwrapped.  Exact data, so
    every result EQUALS the oracle's."""
    calls = []
    monkeypatch.setattr(ops, "_use_kernels", lambda x: x.dtype == torch.float32)
    monkeypatch.setattr(ops, "_launch", lambda name, *a: (calls.append(name), _raw_launch(name, *a))[1])
    B, C_, H, W = 2, 3, 8, 6
    x, v = oc.exact_image(B, C_, H, W, seed=1), oc.exact_image(B, C_, H, W, seed=2)
    new = {"az_op_psf_f32", "az_op_decimate_f32", "az_op_decimate_adj_f32", "az_op_chanmix_f32"}
    for name, A, ref in _operators(C_, H, W, flatten, exact=True):
        shape = A(x).shape
        want, want_v = ref(x).reshape(shape), ref(v).reshape(shape)
        w = oc.exact_image(*shape, seed=3)
        want_t = oo.adjoint(lambda z: ref(z).reshape(shape), x.shape, w)
        calls.clear()
        assert torch.equal(A(x), want) and torch.equal(A.adjoint(w), want_t) and new & set(calls), name
        y, jv = torch.func.jvp(A, (x,), (v,))
        assert torch.equal(y, want) and torch.equal(jv, want_v), name
        y, pull = torch.func.vjp(A, x)
        assert torch.equal(y, want) and torch.equal(pull(w)[0], want_t), name
        assert torch.equal(torch.func.jvp(lambda u: torch.func.vjp(A, x)[1](u)[0], (w,), (w,))[1], want_t), name
        assert torch.equal(torch.func.vjp(lambda u: torch.func.jvp(A, (x,), (u,))[1], v)[1](w)[0], want_t), name
        with torch.no_grad():
            with torch.enable_grad():
                x_hat = x.clone().requires_grad_()
                y_hat = A(x_hat)
            for _ in range(2):
                assert torch.equal(torch.autograd.grad(y_hat, x_hat, w, retain_graph=True)[0], want_t), name
            assert torch.equal(torch.func.jvp(A, (x_hat.detach(),), (v,))[1], want_v), name
        xr, wr = x.clone().requires_grad_(), w.clone().requires_grad_()
        g = torch.autograd.grad(A(xr), xr, wr, create_graph=True)[0]
        assert torch.equal(g, want_t) and torch.equal(torch.autograd.grad(g, wr, v)[0], want_v), name


def test_pinv_goes_through_the_function_too(monkeypatch):
    monkeypatch.setattr(ops, "_use_kernels", lambda x: x.dtype == torch.float32)
    monkeypatch.setattr(ops, "_launch", _raw_launch)
    x = oc.exact_image(2, 3, 8, 8, seed=4)
    P = torch.tensor([[1, 0], [0, 0.5], [0, 0.5]])
    for A, inv in ((DecimateOperator((2, 4), (1, 3)), lambda y: xo.zero_stuff(y, 2, 4, 1, 3)),
                   (ChannelMixOperator([[1, 0, 0], [0, 1, 1]]), lambda y: xo.mix(y, P))):
        y = A(x)
        assert torch.equal(A.pinv(y), inv(y))
        assert torch.equal(torch.func.jvp(A.pinv, (y,), (y,))[1], inv(y))
        assert torch.equal(torch.func.vjp(A.pinv, y)[1](x)[0], oo.adjoint(inv, y.shape, x))


# ----------------------------------------------------------------------------------------------------- argument codes
def test_new_entries_validate_their_arguments():
    from azula_amd import _lib
    from azula_amd.csrc import build

    build.build()
    lib = _lib.lib()
    P, P2, Q, T, TQ = 0x100000, 0x900000, 0x500004, 0x1000, 0x1002  # aligned tensors, a misaligned one, a PSF (never dereferenced)
    NULL, SHAPE, ALIGN = -1, -2, -3
    psf = lambda *a: lib.az_op_psf_f32(*a, None)  # noqa: E731
    ok = (3, 3, 0, 0, 1, 1, 8, 8, 0)
    assert psf(None, P, T, *ok) == NULL and psf(P2, None, T, *ok) == NULL and psf(P2, P, None, *ok) == NULL
    assert psf(P2, P, T, 4, 3, 0, 0, 1, 1, 8, 8, 0) == SHAPE and psf(P2, P, T, 3, 2, 0, 0, 1, 1, 8, 8, 0) == SHAPE  # even sizes
    assert psf(P2, P, T, 67, 3, 0, 0, 1, 1, 80, 80, 0) == SHAPE and psf(P2, P, T, 3, 67, 0, 0, 1, 1, 80, 80, 0) == SHAPE  # above 65
    assert psf(P2, P, T, 0, 3, 0, 0, 1, 1, 8, 8, 0) == SHAPE and psf(P2, P, T, 3, 3, 0, 0, 1, 1, 8, 8, 2) == SHAPE
    assert psf(P2, P, T, 3, 3, -1, 0, 1, 1, 8, 8, 0) == SHAPE and psf(P2, P, T, 3, 3, 0, -1, 1, 1, 8, 8, 0) == SHAPE
    assert psf(P2, P, T, 3, 3, 0, 0, 0, 1, 8, 8, 0) == SHAPE and psf(P2, P, T, 3, 3, 0, 0, 1, 0, 8, 8, 0) == SHAPE
    assert psf(P2, P, T, 17, 3, 0, 0, 1, 1, 8, 8, 1) == SHAPE and psf(P2, P, T, 3, 17, 0, 0, 1, 1, 8, 8, 1) == SHAPE  # circular, r >= size
    assert psf(P, P, T, *ok) == SHAPE and psf(P + 64, P, T, *ok) == SHAPE  # y == x / overlapping
    assert psf(Q, P, T, *ok) == ALIGN and psf(P2, Q, T, *ok) == ALIGN and psf(P2, P, TQ, *ok) == ALIGN
    th, tw = C.c_int32(), C.c_int32()
    assert lib.az_op_psf_tile(3, 3, None, C.byref(tw)) == NULL and lib.az_op_psf_tile(3, 3, C.byref(th), None) == NULL
    assert lib.az_op_psf_tile(4, 3, C.byref(th), C.byref(tw)) == SHAPE and lib.az_op_psf_tile(3, 67, C.byref(th), C.byref(tw)) == SHAPE
    for kh, kw in ((1, 1), (3, 5), (9, 9), (17, 17), (21, 21), (65, 1), (1, 65), (61, 61), (65, 65)):
        assert lib.az_op_psf_tile(kh, kw, C.byref(th), C.byref(tw)) == 0
        # the tile and its halo fit the static LDS of the instantiation the launch takes: 16 KiB where they fit that, else 40 KiB
        staged = (th.value + kh - 1) * (tw.value + kw - 1) * 4
        assert tw.value == 64 and th.value >= 4 and staged <= 40960 and (th.value, tw.value) == xc.PSF_TILE
        assert ops.psf_tile(kh, kw) == (th.value, tw.value)
    for name in ("az_op_decimate_f32", "az_op_decimate_adj_f32"):
        fn = lambda *a: getattr(lib, name)(*a, None)  # noqa: E731, B023
        assert fn(None, P, 1, 8, 8, 2, 2, 0, 0) == NULL and fn(P2, None, 1, 8, 8, 2, 2, 0, 0) == NULL
        assert fn(P2, P, 1, 9, 8, 2, 2, 0, 0) == SHAPE and fn(P2, P, 1, 8, 8, 2, 3, 0, 0) == SHAPE  # H % fh, W % fw
        assert fn(P2, P, 1, 34, 8, 17, 2, 0, 0) == SHAPE and fn(P2, P, 1, 8, 8, 0, 2, 0, 0) == SHAPE and fn(P2, P, 0, 8, 8, 2, 2, 0, 0) == SHAPE
        assert fn(P2, P, 1, 8, 8, 2, 2, 2, 0) == SHAPE and fn(P2, P, 1, 8, 8, 2, 2, 0, 2) == SHAPE  # offsets
        assert fn(P2, P, 1, 8, 8, 2, 2, -1, 0) == SHAPE and fn(P2, P, 1, 8, 8, 2, 2, 0, -1) == SHAPE
        assert fn(P, P, 1, 8, 8, 2, 2, 0, 0) == SHAPE and fn(P + 32, P, 1, 8, 8, 2, 2, 0, 0) == SHAPE  # overlapping
        assert fn(Q, P, 1, 8, 8, 2, 2, 1, 1) == ALIGN and fn(P2, Q, 1, 8, 8, 2, 2, 1, 1) == ALIGN
    mix = lambda *a: lib.az_op_chanmix_f32(*a, None)  # noqa: E731
    assert mix(None, P, T, 1, 3, 1, 16) == NULL and mix(P2, None, T, 1, 3, 1, 16) == NULL and mix(P2, P, None, 1, 3, 1, 16) == NULL
    assert mix(P2, P, T, 1, 17, 1, 16) == SHAPE and mix(P2, P, T, 1, 3, 17, 16) == SHAPE  # more than 16 channels
    assert mix(P2, P, T, 1, 0, 1, 16) == SHAPE and mix(P2, P, T, 1, 3, 0, 16) == SHAPE
    assert mix(P2, P, T, 0, 3, 1, 16) == SHAPE and mix(P2, P, T, 1, 3, 1, 0) == SHAPE
    assert mix(P, P, T, 1, 3, 1, 16) == SHAPE and mix(P + 64, P, T, 1, 3, 3, 16) == SHAPE  # overlapping
    assert mix(Q, P, T, 1, 3, 1, 16) == ALIGN and mix(P2, Q, T, 1, 3, 1, 16) == ALIGN and mix(P2, P, TQ, 1, 3, 1, 16) == ALIGN
