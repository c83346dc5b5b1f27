r"""``FourierOperator``, ``MRIOperator`` and ``cartesian_mask`` without a GPU: the torch path against the dense-matrix oracle in
fp64, adjoints, pseudo-inverses and the Moore-Penrose identities, the shape conventions and their errors, the premise of the GPU
tests' accuracy rule, the autograd Function under every transform the guidance classes use (on a stand-in launcher that reads raw
pointers, as the real one does), and the argument codes of the two C entries."""

import ctypes as C

import numpy as np
import pytest
import torch

import fft_cases as fc
import fft_oracle as fo
from azula_amd.guidance import FourierOperator, MaskOperator, MRIOperator, cartesian_mask
from azula_amd.guidance import operators as ops

F64 = torch.float64
SIZES = [(6, 10), (1, 8), (8, 8), (4, 2), (16, 1)]


@pytest.fixture(autouse=True)
def _grad_mode_on():
    r"""Some modules of the suite switch grad mode off for the whole process; these tests differentiate."""
    with torch.enable_grad():
        yield


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def _randn(*shape, seed=0, dtype=F64):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=dtype)


# ------------------------------------------------------------------------------------------------------- the torch path
@pytest.mark.parametrize("norm", fc.NORMS)
def test_torch_path_equals_the_dft_matrix_oracle(norm):
    for H, W in SIZES:
        x, z = _randn(2, 3, H, W, seed=H), _randn(2, 6, H, W, seed=W)
        A = FourierOperator(norm)
        y = A(x)
        assert y.shape == (2, 6, H, W) and y.dtype == F64
        assert _rel(y, fo.apply(x, norm)) < 1e-12
        f = fo.dft2(x, scale=fo.scale_of(norm, H * W))
        assert _rel(y[:, :3], f.real) < 1e-12 and float((y[:, 3:] - f.imag).abs().max()) < 1e-12 * float(f.abs().max())  # the layout
        assert _rel(A.adjoint(z), fo.adjoint(z, norm)) < 1e-12 and _rel(A.T(z), fo.adjoint(z, norm)) < 1e-12
        assert _rel(A.pinv(z), fo.adjoint(z, norm, pinv=True)) < 1e-12
        y32 = A(x.float())
        assert y32.dtype == torch.float32 and _rel(y32.double(), fo.apply(x.float(), norm)) < 1e-5


@pytest.mark.parametrize("norm", fc.NORMS)
def test_adjoint_inverse_flatten_and_composition_in_fp64(norm):
    B, Cc, H, W = 2, 3, 6, 10
    x, w = _randn(B, Cc, H, W, seed=1), _randn(B, 2 * Cc, H, W, seed=2)
    A = FourierOperator(norm)
    y = A(x)
    lhs, rhs = float((y * w).sum()), float((x * A.adjoint(w)).sum())
    assert abs(lhs - rhs) <= 1e-12 * float(y.abs().sum() * w.abs().max())  # <A x, w> == <x, A^T w>
    assert _rel(A.pinv(y), x) < 1e-12
    if norm == "ortho":
        assert _rel(A.adjoint(y), x) < 1e-12  # A^T A = I
    xr = x.clone().requires_grad_()  # torch differentiates the torch path itself
    assert _rel(torch.autograd.grad(A(xr), xr, w)[0], fo.adjoint(w, norm)) < 1e-12
    F = FourierOperator(norm, flatten=True)
    yf = F(x)
    assert yf.shape == (B, 2 * Cc * H * W) and torch.equal(yf, y.flatten(1))
    for v in (w, w.flatten(1)):  # the flat and the image shape
        assert torch.equal(F.adjoint(v), A.adjoint(w)) and torch.equal(F.pinv(v), A.pinv(w)) and torch.equal(F.T(v), A.adjoint(w))
    assert _rel(F.pinv(yf), x) < 1e-12
    m = fc.symmetric_mask(H, W, seed=3).double()
    for comp in (MaskOperator(m) @ A, MaskOperator(m, flatten=True) @ A):
        assert _rel(comp(x).reshape(y.shape), fo.mri(x, m, norm)) < 1e-12
        assert _rel(comp.adjoint(w), fo.mri_adjoint(w, m, norm)) < 1e-12 and _rel(comp.T(w), fo.mri_adjoint(w, m, norm)) < 1e-12
    assert _rel((A.T @ MaskOperator(m))(w), fo.mri_adjoint(w, m, norm)) < 1e-12


# ---------------------------------------------------------------------------------------------------------- cartesian_mask
def test_cartesian_mask():
    for H, W, acc, cf in ((8, 16, 4, 0.08), (16, 64, 4, 0.08), (4, 256, 8, 0.04), (4, 320, 4, 0.08), (2, 33, 3, 0.1), (2, 8, 1, 0.08),
                          (2, 16, 4, 1.0), (3, 1, 4, 0.08), (2, 64, 100, 0.0)):
        m = cartesian_mask(H, W, acc, cf)
        assert m.shape == (H, W) and m.dtype == torch.float32 and ((m == 0) | (m == 1)).all()
        assert torch.equal(m, m.flip(0, 1).roll((1, 1), (0, 1))), (H, W)  # symmetric under k -> -k
        assert torch.equal(m, cartesian_mask(H, W, acc, cf)) and (m == m[:1]).all()  # the same every time; whole columns
        c = int(np.floor(cf * W + 0.5)) // 2
        freq = torch.minimum(torch.arange(W), W - torch.arange(W))
        assert (m[0][freq <= c] == 1).all() and int((freq <= c).sum()) == min(W, 2 * c + 1) >= min(W, int(np.floor(cf * W + 0.5)))
        n, pairs = int(np.floor(W / acc + 0.5)), max(0, (W - 1) // 2 - c)
        kept = min(W, 2 * c + 1) + 2 * min(pairs, max(0, (n - (2 * c + 1)) // 2))
        assert int(m[0].sum()) == kept == ops.cartesian_columns(W, acc, cf), (H, W, acc, cf)
    assert int(cartesian_mask(1, 256, 4)[0].sum()) == 63 and int(cartesian_mask(1, 64, 1)[0].sum()) == 63  # (never the Nyquist column)
    assert not torch.equal(cartesian_mask(4, 256, 4, seed=0), cartesian_mask(4, 256, 4, seed=1))
    assert MRIOperator(cartesian_mask(16, 64, 4)).symmetric
    for bad in ((0, 4, 0.08), (8, 0.5, 0.08), (8, 4, 1.5), (8, 4, -0.1)):
        with pytest.raises(ValueError):
            cartesian_mask(4, *bad)


# ------------------------------------------------------------------------------------------------------------------- MRI
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("norm", fc.NORMS)
def test_mri_moore_penrose_identities(norm, weighted):
    B, Cc, H, W = 2, 2, 6, 8
    m = fc.symmetric_mask(H, W, seed=4, weighted=weighted).double()
    A = MRIOperator(m, norm)
    assert A.symmetric and A.mask is m
    x, z, u, v = _randn(B, Cc, H, W, seed=1), _randn(B, 2 * Cc, H, W, seed=2), _randn(B, 2 * Cc, H, W, seed=3), _randn(B, Cc, H, W, seed=4)
    y = A(x)
    assert _rel(y, fo.mri(x, m, norm)) < 1e-12 and _rel(A.adjoint(z), fo.mri_adjoint(z, m, norm)) < 1e-12
    P = A.pinv
    assert _rel(A(P(y)), y) < 1e-12  # A A^+ A = A
    assert _rel(P(A(P(z))), P(z)) < 1e-12  # A^+ A A^+ = A^+
    assert abs(float((A(P(z)) * u).sum() - (z * A(P(u))).sum())) < 1e-12 * float(z.norm() * u.norm())  # (A A^+)^T = A A^+
    assert abs(float((P(A(x)) * v).sum() - (x * P(A(v))).sum())) < 1e-12 * float(x.norm() * v.norm())  # (A^+ A)^T = A^+ A
    for shape in ((1, H, W), (1, 1, H, W), (2 * Cc, H, W)):  # everything that broadcasts identically over a re / im pair
        assert torch.equal(MRIOperator(m.expand(shape), norm)(x), y)
    Af = MRIOperator(m, norm, flatten=True)
    assert torch.equal(Af(x), y.flatten(1)) and torch.equal(Af.pinv(y.flatten(1)), P(y)) and torch.equal(Af.adjoint(z.flatten(1)), A.adjoint(z))


def test_mri_errors():
    H, W = 6, 8
    m = fc.symmetric_mask(H, W, seed=4)
    unsym = m.clone()
    unsym[1, 2], unsym[H - 1, W - 2] = 1.0, 0.0
    A = MRIOperator(unsym)
    assert not A.symmetric and A(torch.zeros(1, 2, H, W)).shape == (1, 4, H, W) and A.adjoint(torch.zeros(1, 4, H, W)).shape == (1, 2, H, W)
    with pytest.raises(NotImplementedError, match="symmetric"):
        A.pinv(torch.zeros(1, 4, H, W))
    with pytest.raises(ValueError, match="broadcast"):
        MRIOperator(m)(torch.zeros(1, 2, H, W + 2))  # the mask does not broadcast
    with pytest.raises(ValueError, match="broadcast"):
        MRIOperator(m.expand(6, H, W))(torch.zeros(1, 2, H, W))  # 6 channels against 2 C = 4
    halves = torch.stack([m, m, m, 1 - m])
    with pytest.raises(ValueError, match="real and the imaginary"):
        MRIOperator(halves)
    with pytest.raises(ValueError, match="real and the imaginary"):
        MRIOperator(torch.stack([m, m, m]))
    with pytest.raises(ValueError):
        MRIOperator(torch.ones(W))
    for op in (MRIOperator(m), FourierOperator()):
        with pytest.raises(ValueError, match="even"):
            op.adjoint(torch.zeros(1, 3, H, W))  # odd channels on the way back
        with pytest.raises(ValueError, match="even"):
            op.pinv(torch.zeros(1, 3, H, W))
        with pytest.raises(ValueError, match="B, C, H, W"):
            op(torch.zeros(2, H, W))
    for op in (MRIOperator(m, flatten=True), FourierOperator(flatten=True)):
        with pytest.raises(ValueError, match="in_shape"):
            op.adjoint(torch.zeros(1, 4 * H * W))  # a flat input without the image shape
        op(torch.zeros(1, 2, H, W))
        assert op.adjoint(torch.zeros(1, 4 * H * W)).shape == (1, 2, H, W)
        with pytest.raises(ValueError, match="flattened"):
            op.adjoint(torch.zeros(1, 4 * H * W - 1))
    assert MRIOperator(m, flatten=True, in_shape=(2, H, W)).pinv(torch.zeros(1, 4 * H * W)).shape == (1, 2, H, W)
    with pytest.raises(ValueError, match="norm"):
        FourierOperator("unitary")
    for dtype in (torch.float16, torch.bfloat16):
        with pytest.raises(NotImplementedError, match="fp32 and fp64"):
            FourierOperator()(torch.zeros(1, 1, 4, 4, dtype=dtype))


def test_host_tensors_never_reach_the_kernel(monkeypatch):
    monkeypatch.setattr(ops, "_launch", lambda *a: pytest.fail("a host tensor reached the kernels"))
    x = _randn(1, 2, 6, 10, dtype=torch.float32)
    A = MRIOperator(fc.symmetric_mask(6, 10))
    assert A(x).dtype == torch.float32 and A.pinv(A(x)).shape == x.shape
    assert _rel(FourierOperator()(x.transpose(2, 3)).double(), fo.apply(x.transpose(2, 3))) < 1e-5


# ------------------------------------------------------------------------------------------ the accuracy rule's premise
def test_the_reference_error_of_the_accuracy_rule_is_small():
    r"""The GPU tests bound the kernel by ``max(4 e_ref, 2 * 2^-24)`` with ``e_ref`` the relative loss of torch's fp32 CPU
    transform against fp64.  The rule would pass anything if ``e_ref`` were large: it is at most the worst-case relative error
    of a radix-2 transform, ``8 * 2^-24 * (log2 H + log2 W + 1)`` (measured: at most 0.06 of it)."""
    for H, W in ((2, 2), (8, 8), (1, 1024), (256, 8), (64, 64), (128, 128), (512, 512)):
        re = torch.stack([fc.planes(kind, H, W)[0] for kind in fc.DATA])
        im = torch.stack([fc.planes(kind, H, W)[1] for kind in fc.DATA])
        for i, inverse in ((None, False), (im, True)):
            _, e_ref, bound = fo.rule(fo.dft2(re, i, inverse), re, i, inverse)
            assert float(e_ref.max()) <= fo.worst_case(H, W), (H, W, e_ref.tolist())
            assert float(e_ref.max()) <= 2e-7  # (and the bound the rule gives is a few 1e-7 of S)


# ----------------------------------------------------------------------------------------------- the autograd Function
def _f32(ptr, n):
    return np.ctypeslib.as_array((C.c_float * n).from_address(ptr))


def _planes(ptr, stride, B, Cc, H, W):
    r"""(B, C, H, W) from the raw pointer of a tensor whose samples lie ``stride`` floats apart."""
    flat = _f32(ptr, (B - 1) * stride + Cc * H * W)
    return np.stack([flat[b * stride:b * stride + Cc * H * W].reshape(Cc, H, W) for b in range(B)])


def _raw_launch(name, *a):
    r"""What the kernels compute, from raw pointers alone -- a functorch wrapper has none to give."""
    if name == "az_op_fft2_f32":
        dre, dim, dbs, sre, sim, sbs, work, B, Cc, H, W, inverse, scale = a
        z = _planes(sre, sbs, B, Cc, H, W).astype(np.complex128)
        if sim is not None:
            z = z + 1j * _planes(sim, sbs, B, Cc, H, W)
        out = np.asarray(fo.dft2(torch.from_numpy(z.real.copy()), torch.from_numpy(z.imag.copy()), bool(inverse))) * np.float32(scale)
        for ptr, part in ((dre, out.real), (dim, out.imag)):
            if ptr is not None:
                flat = _f32(ptr, (B - 1) * dbs + Cc * H * W)
                for b in range(B):
                    flat[b * dbs:b * dbs + Cc * H * W] = part[b].astype(np.float32).ravel()
    else:
        from test_operators_host import _raw_launch as earlier

        earlier(name, *a)


def _force_kernels(monkeypatch, calls=None):
    monkeypatch.setattr(ops, "_use_kernels", lambda x: x.dtype == torch.float32)
    monkeypatch.setattr(ops, "_lib", type("lib", (), {"call": staticmethod(lambda name, *a: None)}))  # (az_op_fft2_work: none)
    launch = _raw_launch if calls is None else lambda name, *a: (calls.append(name), _raw_launch(name, *a))[1]
    monkeypatch.setattr(ops, "_launch", launch)


@pytest.mark.parametrize("flatten", [False, True])
@pytest.mark.parametrize("size", [(4, 4), (2, 4), (1, 2)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_transforms_never_hand_the_launcher_a_wrapped_tensor(monkeypatch, flatten, size):
    r"""The method of ``test_operators_host.py``: the kernel path forced onto host tensors with a launcher that consumes
    ``data_ptr()``.  Under ``torch.func.jvp`` / ``vjp`` the tensors that ``backward`` and ``jvp`` of the Function receive are
    wrappers without storage; as applications of the Function they reach ``forward`` unwrapped.  H, W <= 4, integers and
    ``norm="backward"`` (and a 0/1 mask): every result EQUALS the oracle's."""
    calls = []
    _force_kernels(monkeypatch, calls)
    H, W = size
    B, Cc = 2, 3  # (1 x 2: C H W % 4 != 0, the operator's separate halves)
    x, v = fc.exact_planes(B, Cc, H, W, 1), fc.exact_planes(B, Cc, H, W, 2)
    m = fc.symmetric_mask(H, W, seed=2)
    cases = [(FourierOperator("backward", flatten=flatten), lambda t: fo.apply(t, "backward"), lambda t: fo.adjoint(t, "backward")),
             (MRIOperator(m, "backward", flatten=flatten), lambda t: fo.mri(t, m, "backward"), lambda t: fo.mri_adjoint(t, m, "backward")),
             (MaskOperator(m, flatten=flatten) @ FourierOperator("backward"), lambda t: fo.mri(t, m, "backward"),
              lambda t: fo.mri_adjoint(t, m, "backward"))]
    for A, ref, ref_t in cases:
        shape = A(x).shape
        want, want_v = ref(x.double()).reshape(shape).float(), ref(v.double()).reshape(shape).float()
        w = fc.exact_planes(B, 2 * Cc, H, W, 3).reshape(shape)
        want_t = ref_t(w.double().reshape(B, 2 * Cc, H, W)).float()
        calls.clear()
        assert torch.equal(A(x), want) and torch.equal(A.adjoint(w), want_t) and "az_op_fft2_f32" in calls
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


def test_pinv_goes_through_the_function_too(monkeypatch):
    r"""``pinv`` and its transpose (the apply map at the pinv's scale) under ``jvp`` / ``vjp``: with ``norm="forward"`` the
    pseudo-inverse has scale 1, so on integers it EQUALS the oracle."""
    _force_kernels(monkeypatch)
    H, W = 4, 2
    m = fc.symmetric_mask(H, W, seed=2)
    z, x = fc.exact_planes(2, 4, H, W, 5), fc.exact_planes(2, 2, H, W, 6)
    for A, inv, inv_t in ((FourierOperator("forward"), lambda t: fo.adjoint(t, "forward", pinv=True), lambda t: fo.apply(t, "forward", True)),
                          (MRIOperator(m, "forward"), lambda t: fo.adjoint(t * m, "forward", pinv=True),
                           lambda t: fo.apply(t, "forward", True) * m)):
        want, want_t = inv(z.double()).float(), inv_t(x.double()).float()
        assert torch.equal(A.pinv(z), want)
        assert torch.equal(torch.func.jvp(A.pinv, (z,), (z,))[1], want)
        assert torch.equal(torch.func.vjp(A.pinv, z)[1](x)[0], want_t)
        zr = z.clone().requires_grad_()
        assert torch.equal(torch.autograd.grad(A.pinv(zr), zr, x)[0], want_t)


# ----------------------------------------------------------------------------------------------------- argument codes
def test_fft_entries_validate_their_arguments():
    from azula_amd import _lib
    from azula_amd.csrc import build

    build.build()
    lib = _lib.lib()
    P, P2, P3, P4, Wk, Q = 0x100000, 0x900000, 0x1100000, 0x1900000, 0x2100000, 0x500004  # aligned bases (never dereferenced), a misaligned one
    NULL, SHAPE, ALIGN = -1, -2, -3
    fft = lambda *a: lib.az_op_fft2_f32(*a, None)  # noqa: E731

    def call(dre=P, dim=P2, dbs=192, sre=P3, sim=P4, sbs=192, work=None, B=1, Cc=3, H=8, W=8, inverse=0, scale=1.0):
        return fft(dre, dim, dbs, sre, sim, sbs, work, B, Cc, H, W, inverse, scale)

    # (nothing here may launch: every call below fails its validation)
    assert call(dre=None) == NULL and call(sre=None) == NULL
    assert call(dim=None, H=128, W=128, dbs=3 << 14, sbs=3 << 14) == NULL  # two passes, no imaginary output: `work` is required
    for bad in (0, 3, 6, 12, 96, 2048, -8):
        assert call(H=bad) == SHAPE and call(W=bad) == SHAPE, bad  # zero, not a power of two, above the maximum
    assert ops.MAX_FFT == 1024 and call(H=2048, W=1) == SHAPE
    assert call(B=0) == SHAPE and call(Cc=0) == SHAPE and call(inverse=2) == SHAPE and call(inverse=-1) == SHAPE
    assert call(B=2, dbs=191) == SHAPE and call(B=2, sbs=100) == SHAPE and call(B=2, dbs=-192) == SHAPE  # a tensor's own planes overlap
    for name in ("dre", "dim", "sre", "sim"):
        assert call(**{name: Q}) == ALIGN, name
    assert call(dim=None, H=128, W=128, dbs=3 << 14, sbs=3 << 14, work=Q) == ALIGN
    assert call(dre=P3) == SHAPE and call(dre=P3 + 64) == SHAPE and call(dim=P4) == SHAPE and call(dim=P) == SHAPE  # overlap
    assert call(dre=P4 + 16) == SHAPE and call(sim=P3) == SHAPE and call(dim=P + 16 * 3) == SHAPE
    assert call(dim=None, sim=None, dre=P3) == SHAPE
    assert call(dim=None, H=128, W=128, dbs=3 << 14, sbs=3 << 14, work=P) == SHAPE  # `work` over dst_re
    assert call(dim=None, H=128, W=128, dbs=3 << 14, sbs=3 << 14, work=P3 + 64) == SHAPE  # `work` over src_re
    # the halves of one (B, 2 C, H, W) tensor interleave and are not an overlap; their misplacement is one
    assert call(B=2, dim=P + 4 * 192, dbs=384, sre=P, sim=P + 4 * 192, sbs=384) == SHAPE  # (dst == src)
    assert call(B=2, dim=P + 4 * 100, dbs=384) == SHAPE
    floats = C.c_int64(-1)
    assert lib.az_op_fft2_work(1, 3, 8, 8, None) == NULL
    for bad in ((0, 3, 8, 8), (1, 0, 8, 8), (1, 3, 12, 8), (1, 3, 8, 2048), (1, 3, 0, 8)):
        assert lib.az_op_fft2_work(*bad, C.byref(floats)) == SHAPE
    for H, W in fc.ACCURACY_SIZES + fc.EXACT_SIZES:
        assert lib.az_op_fft2_work(2, 3, H, W, C.byref(floats)) == 0
        assert floats.value == (0 if H * W <= fc.WHOLE_PLANE_POINTS else 6 * H * W), (H, W)
    assert lib.az_op_fft2_work(1, 1, 1024, 1024, C.byref(floats)) == 0 and floats.value == 1 << 20
