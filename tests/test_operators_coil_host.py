r"""``MultiCoilMRIOperator`` and ``birdcage_maps`` without a GPU: the torch path against the fp64 oracle of ``coil_oracle.py``,
adjointness, ``zero_filled`` against ``torch.linalg.pinv`` of the dense matrix, the validation errors, the premise of the GPU
tests' accuracy rule, the autograd Function under every transform the guidance classes use (on a stand-in launcher that reads
raw pointers, as the real one does), and the argument codes of the two C entries."""

import ctypes as C

import numpy as np
import pytest
import torch

import coil_cases as cc
import coil_oracle as co
import fft_cases as fc
from azula_amd.guidance import MaskOperator, MultiCoilMRIOperator, birdcage_maps, cartesian_mask
from azula_amd.guidance import operators as ops

F64 = torch.float64


@pytest.fixture(autouse=True)
def _grad_mode_on():
    r"""Some modules of the suite switch grad mode off for the whole process; these tests differentiate."""
    with torch.enable_grad():
        yield


def _close(got, ref, tol=1e-12):
    return got.shape == ref.shape and float((got - ref).abs().max()) <= tol * float(ref.abs().max())


def _maps64(K, H, W, per_sample, B=2):
    r"""complex128 maps and their split planes: birdcage maps with a per-coil complex weight, so that ``sum |S|^2`` varies."""
    s = birdcage_maps(K, H, W) * torch.complex(cc.randn(K, 1, 1, seed=1, dtype=F64), cc.randn(K, 1, 1, seed=2, dtype=F64))
    if per_sample:
        s = torch.stack([s * (b + 1) for b in range(B)])
    return s, s.real, s.imag


def _weighted_mask(H, W, seed=0):
    r"""A sampling mask with zeros and weights, (H, W) fp64."""
    return torch.tensor([0.0, 0.0, 0.5, 1.0, 2.0], dtype=F64)[torch.randint(0, 5, (H, W), generator=torch.Generator().manual_seed(seed))]


# ------------------------------------------------------------------------------------------------------- the torch path
@pytest.mark.parametrize("per_sample", [False, True], ids=["shared", "per-sample"])
@pytest.mark.parametrize("complex_image", [True, False], ids=["complex", "real"])
@pytest.mark.parametrize("norm", cc.NORMS)
def test_torch_path_equals_the_oracle(norm, complex_image, per_sample):
    B, K = 2, 3
    for H, W in ((6, 10), (4, 8), (1, 2)):  # (6 x 10: not a power of two)
        s, s_re, s_im = _maps64(K, H, W, per_sample)
        m = _weighted_mask(H, W, seed=H)
        x, w = cc.randn(B, 2 if complex_image else 1, H, W, seed=3, dtype=F64), cc.randn(B, 2 * K, H, W, seed=4, dtype=F64)
        A = MultiCoilMRIOperator(m, s, norm, complex_image)
        y = A(x)
        assert y.dtype == F64 and y.shape == (B, 2 * K, H, W) and A.coils == K and A.mask is m
        assert _close(y, co.apply(x, m, s_re, s_im, norm))
        ref_t, ref_z = co.adjoint(w, m, s_re, s_im, norm, complex_image), co.adjoint(w, m, s_re, s_im, norm, complex_image, True)
        assert _close(A.adjoint(w), ref_t) and _close(A.T(w), ref_t) and _close(A.zero_filled(w), ref_z)
        xr = x.clone().requires_grad_()  # torch differentiates the torch path itself
        assert _close(torch.autograd.grad(A(xr), xr, w)[0], ref_t)
        assert _close(torch.func.jvp(A, (x,), (x,))[1], co.apply(x, m, s_re, s_im, norm))
        wr = w.clone().requires_grad_()
        assert _close(torch.autograd.grad(A.zero_filled(wr), wr, x)[0], co.apply(x, m, s_re, s_im, norm, True))
        F = MultiCoilMRIOperator(m, s, norm, complex_image, flatten=True)
        yf = F(x)
        assert yf.shape == (B, 2 * K * H * W) and torch.equal(yf, y.flatten(1))
        for v in (w, w.flatten(1)):  # the flat and the image shape
            assert torch.equal(F.adjoint(v), A.adjoint(w)) and torch.equal(F.zero_filled(v), A.zero_filled(w))
        G = MultiCoilMRIOperator(m, s, norm, complex_image, flatten=True, in_shape=x.shape[1:])
        assert torch.equal(G.adjoint(w.flatten(1)), A.adjoint(w))
        comp = MaskOperator(m, flatten=True) @ MultiCoilMRIOperator(torch.ones(H, W, dtype=F64), s, norm, complex_image)
        assert _close(comp(x).reshape(y.shape), co.apply(x, m, s_re, s_im, norm))  # A2 @ A1 applies unchanged
        assert _close(comp.adjoint(w.flatten(1)), ref_t)
        y32 = MultiCoilMRIOperator(m, s.to(torch.complex64), norm, complex_image)(x.float())  # complex64 maps, fp32 input
        assert y32.dtype == torch.float32 and _close(y32.double(), y, 1e-5)


@pytest.mark.parametrize("complex_image", [True, False], ids=["complex", "real"])
@pytest.mark.parametrize("norm", cc.NORMS)
def test_adjointness_in_fp64(norm, complex_image):
    B, K, H, W = 2, 5, 6, 10
    for per_sample in (False, True):
        s, _, _ = _maps64(K, H, W, per_sample)
        A = MultiCoilMRIOperator(_weighted_mask(H, W, 1), s, norm, complex_image)
        x, w = cc.randn(B, 2 if complex_image else 1, H, W, seed=5, dtype=F64), cc.randn(B, 2 * K, H, W, seed=6, dtype=F64)
        lhs, rhs = float((A(x) * w).sum()), float((x * A.adjoint(w)).sum())
        assert abs(lhs - rhs) <= 1e-12 * abs(lhs)  # <A x, w> == <x, A^T w>
        lhs, rhs = float((A.zero_filled(w) * x).sum()), float((w * co.apply(x, A.mask, s.real, s.imag, norm, True)).sum())
        assert abs(lhs - rhs) <= 1e-12 * abs(lhs)  # and zero_filled against its transpose


@pytest.mark.parametrize("complex_image", [True, False], ids=["complex", "real"])
@pytest.mark.parametrize("norm", cc.NORMS)
def test_zero_filled_is_the_pseudo_inverse_under_full_sampling(norm, complex_image):
    r"""4 x 4, K = 2, full mask: ``zero_filled`` against ``torch.linalg.pinv`` of the dense real matrix of A, and A^+ A = I."""
    K, H, W = 2, 4, 4
    c = 2 if complex_image else 1
    s, _, _ = _maps64(K, H, W, False)
    A = MultiCoilMRIOperator(torch.ones(H, W, dtype=F64), s, norm, complex_image)
    n_in, n_out = c * H * W, 2 * K * H * W
    dense = A(torch.eye(n_in, dtype=F64).reshape(n_in, c, H, W)).reshape(n_in, n_out).T  # (n_out, n_in): column j is A e_j
    inv = A.zero_filled(torch.eye(n_out, dtype=F64).reshape(n_out, 2 * K, H, W)).reshape(n_out, n_in).T  # (n_in, n_out)
    want = torch.linalg.pinv(dense)
    assert float((inv - want).abs().max()) <= 1e-10 * float(want.abs().max())
    x = cc.randn(3, c, H, W, seed=7, dtype=F64)
    assert _close(A.zero_filled(A(x)), x, 1e-12)
    big = MultiCoilMRIOperator(torch.ones(6, 10, dtype=F64), _maps64(3, 6, 10, True, B=3)[0], norm, complex_image, flatten=True)
    xb = cc.randn(3, c, 6, 10, seed=8, dtype=F64)
    assert _close(big.zero_filled(big(xb)), xb, 1e-12)


def test_birdcage_maps():
    for K, H, W, radius in ((1, 4, 4, 1.5), (4, 16, 16, 1.5), (8, 6, 10, 2.0), (15, 32, 8, 1.5)):
        s = birdcage_maps(K, H, W, radius)
        assert s.shape == (K, H, W) and s.dtype == torch.complex128 and s.device.type == "cpu"
        assert float(((s.real**2 + s.imag**2).sum(0) - 1).abs().max()) <= 1e-12
        assert torch.isfinite(s.abs()).all() and (s.abs() > 0).all()
        assert torch.equal(s, birdcage_maps(K, H, W, radius))  # no random numbers
    s = birdcage_maps(2, 8, 8)  # coil 0 sits on the +x axis: stronger, and in phase, on that side
    assert float(s[0].abs()[:, -1].min()) > float(s[0].abs()[:, 0].max()) and float(s[1].abs()[:, 0].min()) > float(s[1].abs()[:, -1].max())
    assert (s[0].real > 0).all() and (s[1].real < 0).all()
    for bad in ((0, 4, 4, 1.5), (2, 0, 4, 1.5), (2, 4, 0, 1.5), (2, 4, 4, 1.0), (2.0, 4, 4, 1.5)):
        with pytest.raises(ValueError):
            birdcage_maps(*bad)


def test_errors():
    H, W, K = 6, 8, 3
    m = fc.symmetric_mask(H, W, seed=4)
    s = birdcage_maps(K, H, W)
    for bad in (s.real, s.real.float(), s.real.long(), [[1j]]):
        with pytest.raises(ValueError, match="complex64 or complex128"):
            MultiCoilMRIOperator(m, bad)
    for value in (float("nan"), float("inf")):
        broken = s.clone()
        broken[1, 2, 3] = complex(0.0, value)
        with pytest.raises(ValueError, match="non-finite"):
            MultiCoilMRIOperator(m, broken)
    for shape in ((0, H, W), (H, W), (2, 0, H, W), (1, 1, K, H, W)):
        with pytest.raises(ValueError, match="K >= 1"):
            MultiCoilMRIOperator(m, torch.ones(shape, dtype=torch.complex64))
    with pytest.raises(ValueError, match="norm"):
        MultiCoilMRIOperator(m, s, "unitary")
    with pytest.raises(ValueError, match="real and the imaginary"):  # the mask rules of MRIOperator
        MultiCoilMRIOperator(torch.cat([m.expand(K, H, W), 1 - m.expand(K, H, W)]), s)
    with pytest.raises(ValueError):
        MultiCoilMRIOperator(torch.ones(W), s)
    A, R = MultiCoilMRIOperator(m, s), MultiCoilMRIOperator(m, s, complex_image=False)
    assert A(torch.zeros(1, 2, H, W)).shape == (1, 2 * K, H, W) and R(torch.zeros(1, 1, H, W)).shape == (1, 2 * K, H, W)
    assert A.adjoint(torch.zeros(1, 2 * K, H, W)).shape == (1, 2, H, W) and R.zero_filled(torch.zeros(1, 2 * K, H, W)).shape == (1, 1, H, W)
    for op, channels in ((A, (1, 3, 4)), (R, (2, 3))):
        for c in channels:
            with pytest.raises(ValueError, match="channel"):
                op(torch.zeros(1, c, H, W))
    with pytest.raises(ValueError, match="maps are"):
        A(torch.zeros(1, 2, H, W + 2))
    with pytest.raises(ValueError, match="B, C, H, W"):
        A(torch.zeros(2, H, W))
    for fn in (A.adjoint, A.zero_filled):
        with pytest.raises(ValueError, match="channels"):
            fn(torch.zeros(1, 2 * K + 2, H, W))
    with pytest.raises(ValueError, match="broadcast"):
        MultiCoilMRIOperator(m.expand(4, H, W), s)(torch.zeros(1, 2, H, W))  # 4 mask channels against 2 K = 6
    assert torch.equal(MultiCoilMRIOperator(m.expand(2 * K, H, W), s)(torch.ones(1, 2, H, W)), A(torch.ones(1, 2, H, W)))
    per = MultiCoilMRIOperator(m, torch.stack([s, s]))
    with pytest.raises(ValueError, match="batch of 2"):
        per(torch.zeros(3, 2, H, W))
    with pytest.raises(NotImplementedError, match="zero_filled.*linalg.cg"):
        A.pinv(torch.zeros(1, 2 * K, H, W))
    flat = MultiCoilMRIOperator(m, s, flatten=True)
    with pytest.raises(ValueError, match="in_shape"):
        flat.zero_filled(torch.zeros(1, 2 * K * H * W))  # a flat input without the image shape
    flat(torch.zeros(1, 2, H, W))
    assert flat.zero_filled(torch.zeros(1, 2 * K * H * W)).shape == (1, 2, H, W)
    with pytest.raises(ValueError, match="flattened"):
        flat.adjoint(torch.zeros(1, 2 * K * H * W - 1))
    for dtype in (torch.float16, torch.bfloat16):
        with pytest.raises(NotImplementedError, match="fp32 and fp64"):
            A(torch.zeros(1, 2, H, W, dtype=dtype))


def test_host_tensors_never_reach_the_kernel(monkeypatch):
    monkeypatch.setattr(ops, "_launch", lambda *a: pytest.fail("a host tensor reached the kernels"))
    A = MultiCoilMRIOperator(fc.symmetric_mask(6, 10), birdcage_maps(3, 6, 10))
    x = cc.randn(1, 2, 6, 10)
    assert A(x).dtype == torch.float32 and A.zero_filled(A(x)).shape == x.shape and A.adjoint(A(x)).shape == x.shape


# ------------------------------------------------------------------------------------------ the accuracy rule's premise
@pytest.mark.parametrize("size", cc.OPERATOR_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_reference_error_of_the_accuracy_rule_is_small(size):
    r"""The GPU tests bound the operator per output plane by ``max(4 e_ref, 2 * 2^-24) S`` with ``e_ref`` the relative 2-norm loss
    of the torch fp32 host path against the fp64 oracle.  The rule would pass anything if ``e_ref`` were large: on the GPU
    tests' own shapes and data it stays below 4e-7 (a host measurement up to 256 x 256 and K = 15 gave at most 1.6e-7)."""
    H, W = size
    worst = 0.0
    for complex_image in (True, False):
        for per_sample in (False, True):
            x, w, maps, m = cc.operator_case(H, W, per_sample, complex_image)
            s_re, s_im = maps.real, maps.imag
            for norm in cc.NORMS:
                A = MultiCoilMRIOperator(m, maps, norm, complex_image)
                for got, ref in ((A(x), co.apply(x, m, s_re, s_im, norm)),
                                 (A.adjoint(w), co.adjoint(w, m, s_re, s_im, norm, complex_image))):
                    _, e_ref, _ = co.rule(ref, got)
                    worst = max(worst, float(e_ref.max()))
                    assert float(e_ref.max()) <= cc.E_REF_MAX, (norm, complex_image, per_sample, e_ref.tolist())
    print(f"multi-coil {H}x{W}: worst e_ref {worst:.3e}")


# ----------------------------------------------------------------------------------------------- the autograd Function
def _f32(ptr, n):
    return np.ctypeslib.as_array((C.c_float * n).from_address(ptr))


def _read(ptr, bstride, B, n):
    r"""(B, n) fp64 copies of the samples that lie ``bstride`` floats apart from the raw pointer (0: one shared by all)."""
    flat = _f32(ptr, (B - 1) * bstride + n)
    return np.stack([flat[b * bstride:b * bstride + n] for b in range(B)]).astype(np.float64)


def _write(ptr, bstride, B, n, values):
    flat = _f32(ptr, (B - 1) * bstride + n)
    for b in range(B):
        flat[b * bstride:b * bstride + n] = values[b].astype(np.float32).ravel()


def _raw_launch(name, *a):
    r"""What the two coil entries compute, from raw pointers alone -- a functorch wrapper has none to give."""
    if name == "az_op_coil_expand_f32":
        dre, dim, dbs, xre, xim, xbs, sre, sim, sbs, B, K, HW = a
        x = _read(xre, xbs, B, HW) + (0 if xim is None else 1j * _read(xim, xbs, B, HW))
        s = (_read(sre, sbs, B, K * HW) + 1j * _read(sim, sbs, B, K * HW)).reshape(B, K, HW)
        out = s * x[:, None]
        _write(dre, dbs, B, K * HW, out.real)
        _write(dim, dbs, B, K * HW, out.imag)
    elif name == "az_op_coil_combine_f32":
        dre, dim, dbs, zre, zim, zbs, sre, sim, sbs, B, K, HW, normalize = a
        z = (_read(zre, zbs, B, K * HW) + 1j * _read(zim, zbs, B, K * HW)).reshape(B, K, HW)
        s = (_read(sre, sbs, B, K * HW) + 1j * _read(sim, sbs, B, K * HW)).reshape(B, K, HW)
        out = (s.conj() * z).sum(1)
        if normalize:
            D = (s.real**2 + s.imag**2).sum(1)
            out = np.where(D != 0, out / np.where(D != 0, D, 1.0), 0.0)
        _write(dre, dbs, B, HW, out.real)
        if dim is not None:
            _write(dim, dbs, B, HW, out.imag)
    else:
        from test_operators_fft_host import _raw_launch as earlier  # (az_op_fft2_f32, az_op_mul_f32)

        earlier(name, *a)


def _force_kernels(monkeypatch, calls):
    r"""The method of ``test_operators_fft_host.py``: the kernel path forced onto fp32 host tensors."""
    monkeypatch.setattr(ops, "_use_kernels", lambda x: x.dtype == torch.float32)
    monkeypatch.setattr(ops, "_lib", type("lib", (), {"call": staticmethod(lambda name, *a: None)}))
    monkeypatch.setattr(ops, "_launch", lambda name, *a: (calls.append(name), _raw_launch(name, *a))[1])


@pytest.mark.parametrize("per_sample", [False, True], ids=["shared", "per-sample"])
@pytest.mark.parametrize("complex_image", [True, False], ids=["complex", "real"])
@pytest.mark.parametrize("case", [(4, 4, 4, False), (2, 2, 4, True), (3, 1, 2, False), (1, 4, 1, True)],
                         ids=lambda c: f"K{c[0]}-{c[1]}x{c[2]}{'-flat' if c[3] else ''}")
def test_transforms_never_hand_the_launcher_a_wrapped_tensor(monkeypatch, case, complex_image, per_sample):
    r"""Under ``torch.func.jvp`` / ``vjp`` the tensors that ``backward`` and ``jvp`` of the Function receive are wrappers without
    storage; as applications of the Function they reach ``forward`` unwrapped.  Integers of magnitude at most 8, Gaussian-integer
    maps whose ``sum |S|^2`` is 0 or a power of two, ``norm="backward"``, H, W <= 4 and a 0/1 mask: every product, sum, scale and
    quotient is exact in fp32, so every result EQUALS the fp64 oracle's.  K = 3 at 1 x 2: K H W % 4 != 0, separate halves."""
    K, H, W, flatten = case
    B, c = 2, 2 if complex_image else 1
    calls = []
    _force_kernels(monkeypatch, calls)
    s_re, s_im = cc.exact_maps(K, H, W, seed=K + H, batch=B if per_sample else None)
    m = fc.symmetric_mask(H, W, seed=2)
    A = MultiCoilMRIOperator(m, torch.complex(s_re, s_im), "backward", complex_image, flatten=flatten)
    x, v = cc.ints(B, c, H, W, seed=1), cc.ints(B, c, H, W, seed=2)
    shape = A(x).shape
    assert shape == ((B, 2 * K * H * W) if flatten else (B, 2 * K, H, W))
    fwd = lambda t: co.apply(t, m, s_re, s_im, "backward").reshape(shape).float()  # noqa: E731
    want, want_v = fwd(x), fwd(v)
    w = cc.ints(B, 2 * K, H, W, seed=3).reshape(shape)
    w4 = w.reshape(B, 2 * K, H, W)
    want_t = co.adjoint(w4, m, s_re, s_im, "backward", complex_image).float()
    calls.clear()
    assert torch.equal(A(x), want) and calls == ["az_op_coil_expand_f32", "az_op_fft2_f32", "az_op_mul_f32"]
    calls.clear()
    assert torch.equal(A.adjoint(w), want_t) and calls == ["az_op_mul_f32", "az_op_fft2_f32", "az_op_coil_combine_f32"]
    y, jv = torch.func.jvp(A, (x,), (v,))
    assert torch.equal(y, want) and torch.equal(jv, want_v)
    y, pull = torch.func.vjp(A, x)
    assert torch.equal(y, want) and torch.equal(pull(w)[0], want_t)
    assert torch.equal(torch.func.jvp(lambda u: torch.func.vjp(A, x)[1](u)[0], (w,), (w,))[1], want_t)
    assert torch.equal(torch.func.vjp(lambda u: torch.func.jvp(A, (x,), (u,))[1], v)[1](w)[0], want_t)
    with torch.no_grad():
        with torch.enable_grad():
            x_hat = x.clone().requires_grad_()
            y_hat = A(x_hat)
        for _ in range(2):
            assert torch.equal(torch.autograd.grad(y_hat, x_hat, w, retain_graph=True)[0], want_t)
        assert torch.equal(torch.func.jvp(A, (x_hat.detach(),), (v,))[1], want_v)
    xr, wr = x.clone().requires_grad_(), w.clone().requires_grad_()
    g = torch.autograd.grad(A(xr), xr, wr, create_graph=True)[0]
    assert torch.equal(g, want_t) and torch.equal(torch.autograd.grad(g, wr, v)[0], want_v)
    # zero_filled and its transpose: M^+ = M for a 0/1 mask, the pinv's scale 1 / (H W) and sum |S|^2 are powers of two
    want_z = co.adjoint(w4, m, s_re, s_im, "backward", complex_image, zero_filled=True).float()
    want_zt = co.apply(x, m, s_re, s_im, "backward", transpose_of_zero_filled=True).float()
    calls.clear()
    assert torch.equal(A.zero_filled(w), want_z) and calls == ["az_op_mul_f32", "az_op_fft2_f32", "az_op_coil_combine_f32"]
    assert torch.equal(torch.func.jvp(A.zero_filled, (w,), (w,))[1], want_z)
    calls.clear()
    assert torch.equal(torch.func.vjp(A.zero_filled, w4)[1](x)[0], want_zt)
    assert calls[-3:] == ["az_op_coil_expand_f32", "az_op_fft2_f32", "az_op_mul_f32"]
    wr = w4.clone().requires_grad_()
    assert torch.equal(torch.autograd.grad(A.zero_filled(wr), wr, x)[0], want_zt)
    assert torch.equal(torch.func.vjp(lambda u: torch.func.vjp(A.zero_filled, w4)[1](u)[0], x)[1](w4)[0], want_z)  # and back


# ----------------------------------------------------------------------------------------------------- argument codes
def test_coil_entries_validate_their_arguments():
    from azula_amd import _lib
    from azula_amd.csrc import build

    build.build()
    cc.argument_errors(_lib.lib())
