r"""``RadonOperator`` and ``radon_angles`` without a GPU: the sparse-matrix path against the oracle of ``radon_oracle.py``, the
shape conventions and their errors, the properties of the fp32 weights that the definition promises, filtered back-projection of
the fp64 model on a phantom, the autograd Functions under every transform the guidance classes use (the kernel path on a
stand-in launcher that reads raw pointers, as the real one does), and the argument codes of the four C entries."""

import ctypes as C
import math

import numpy as np
import pytest
import torch

import radon_cases as rc
import radon_oracle as ro
from azula_amd.guidance import MaskOperator, RadonOperator, radon_angles
from azula_amd.guidance import operators as ops

F64 = torch.float64
SMALL = [(5, 3, None, 1.0), (16, 16, None, 1.5), (9, 12, 3, 2.0), (7, 7, 40, 8.0), (1, 1, None, 1.0)]


@pytest.fixture(autouse=True)
def _grad_mode_on():
    r"""Some modules of the suite switch grad mode off for the whole process; these tests differentiate."""
    with torch.enable_grad():
        yield


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def _randn(*shape, seed=0, dtype=F64):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=dtype)


# ------------------------------------------------------------------------------------------------- the weights' definition
def test_the_scatter_form_of_the_oracle_is_the_dense_definition():
    r"""``Geometry`` keeps the bins floor(p) and floor(p) + 1 only; ``dense`` evaluates every bin of every pixel."""
    for H, W, D, d in SMALL + [(33, 47, None, 1.0)]:
        g = ro.geometry(rc.ANGLES, H, W, D, d)
        assert np.array_equal(ro.dense(rc.ANGLES, H, W, g.D, d), g.dense().numpy()), (H, W, D, d)


def test_operator_and_oracle_hold_the_same_fp32_numbers():
    for H, W, D, d in SMALL:
        A, g = RadonOperator(rc.ANGLES, (H, W), D, d), ro.geometry(rc.ANGLES, H, W, D, d)
        assert A.det_count == g.D and A.angles == g.A == len(rc.ANGLES)
        assert np.array_equal(A.table.numpy(), ro.table(rc.ANGLES)) and A.table.dtype == torch.float32
        assert torch.equal(A.taps, g.taps) and A.taps.dtype == torch.float32 and A.fbp_scale == g.fbp_scale
        M, Mt, T = A._matrices(torch.zeros(1, dtype=F64))
        assert torch.equal(M.to_dense(), g.dense()) and torch.equal(Mt.to_dense(), g.dense().T)
        assert torch.equal(T, ro.toeplitz(g.taps))
    for n, odd in ((8, False), (9, True)):  # the default detector count: odd, and it covers the diagonal
        D = RadonOperator([0.0], (n, n)).det_count
        assert D == ro.default_det_count(n, n) and D % 2 == 1 and D >= math.hypot(n, n)


def test_angle_properties():
    for t in (0.0, 90.0, 180.0, 270.0, 360.0, -90.0, 450.0, 1e-300 - 90.0):
        c, s = ro.cos_sin(t)
        assert {abs(float(c)), abs(float(s))} == {0.0, 1.0}, t
    assert ro.cos_sin(0.0) == (1, 0) and ro.cos_sin(90.0) == (0, 1) and ro.cos_sin(180.0) == (-1, 0) and ro.cos_sin(270.0) == (0, -1)
    for t, sc, ss in ((45.0, 1, 1), (135.0, -1, 1), (225.0, -1, -1), (315.0, 1, -1), (405.0, 1, 1), (-45.0, 1, -1)):
        c, s = ro.cos_sin(t)
        assert c * sc == s * ss == np.float32(math.sqrt(0.5)), t  # c == s bitwise, up to the quadrant's signs
    assert ro.cos_sin(720.5) == ro.cos_sin(0.5) and ro.cos_sin(-30.0) == ro.cos_sin(330.0)
    for H, W in ((4, 4), (5, 3), (8, 7)):
        M = ro.geometry(rc.RIGHT_ANGLES, H, W).dense()
        assert set(M.unique().tolist()) <= {0.0, 0.5, 1.0}, (H, W)  # multiples of 90 degrees: weights 0, 1/2, 1
    for H, W, d in ((16, 16, 1.0), (33, 47, 1.0), (9, 12, 2.0), (7, 7, 8.0), (12, 5, 1.5)):
        g = ro.geometry(rc.ANGLES, H, W, None, d)
        per_angle = g.dense().reshape(g.A, g.D, H * W).sum(1)  # every pixel's weights of one angle
        if d == 1.0:
            assert torch.equal(per_angle, torch.ones_like(per_angle)), (H, W)  # exactly 1 once D covers the image
        else:
            assert float((per_angle - 1).abs().max()) <= 4 * ro.EPS, (H, W, d)  # p is a rounded product: 1 to two roundings
    assert torch.equal(radon_angles(4), torch.tensor([0.0, 45.0, 90.0, 135.0], dtype=F64))
    assert torch.equal(radon_angles(3, 90.0), torch.tensor([0.0, 30.0, 60.0], dtype=F64))
    with pytest.raises(ValueError):
        radon_angles(0)


# ------------------------------------------------------------------------------------------------------- the torch path
def test_torch_path_equals_the_oracle():
    for H, W, D, d in SMALL:
        A, g = RadonOperator(rc.ANGLES, (H, W), D, d), ro.geometry(rc.ANGLES, H, W, D, d)
        x, v = _randn(2, 3, H, W, seed=H), _randn(2, 3, g.A, g.D, seed=W)
        y = A(x)
        assert y.shape == (2, 3, g.A, g.D) and y.dtype == F64
        assert _rel(y, g.apply(x)) < 1e-13 and _rel(A.adjoint(v), g.adjoint(v)) < 1e-13 and _rel(A.T(v), g.adjoint(v)) < 1e-13
        assert _rel(A.fbp(v), g.fbp(v)) < 1e-13
        y32 = A(x.float())
        assert y32.dtype == torch.float32 and (y32.double() - g.apply(x.float())).abs().le(g.bound_apply(x.float()) * 2).all()
        lhs, rhs = float((y * v).sum()), float((x * A.adjoint(v)).sum())
        assert abs(lhs - rhs) <= 1e-13 * float(y.norm() * v.norm())  # <A x, w> == <x, A^T w>
    h = RadonOperator(rc.EVEN, (8, 8))(torch.ones(1, 1, 8, 8, dtype=torch.bfloat16))  # half precision: the fp32 product, rounded
    g = ro.geometry(rc.EVEN, 8, 8)
    ref = g.apply(torch.ones(1, 1, 8, 8))  # (the rule at bf16's 2^-9: it covers a product made in bf16 throughout as well)
    assert h.dtype == torch.bfloat16 and ((h.double() - ref).abs() <= (g.nnz_rows + 3) * 2.0 ** -9 * ref).all()


def test_shapes_flatten_transpose_and_composition():
    B, Cc, H, W = 2, 3, 9, 12
    A, g = RadonOperator(rc.EVEN, (H, W)), ro.geometry(rc.EVEN, H, W)
    x, v = _randn(B, Cc, H, W, seed=1), _randn(B, Cc, g.A, g.D, seed=2)
    y = A(x)
    assert A.in_shape == (Cc, H, W) and A.size == (H, W)
    xr = x.clone().requires_grad_()
    assert _rel(torch.autograd.grad(A(xr), xr, v)[0], g.adjoint(v)) < 1e-13
    F = RadonOperator(rc.EVEN, (H, W), flatten=True)
    for vv in (v, v.flatten(1)):  # the flat and the image shape; no forward call was needed: A D is known
        assert torch.equal(F.adjoint(vv), A.adjoint(v)) and torch.equal(F.fbp(vv), A.fbp(v)) and torch.equal(F.T(vv), A.adjoint(v))
    yf = F(x)
    assert yf.shape == (B, Cc * g.A * g.D) and torch.equal(yf, y.flatten(1)) and F.in_shape == (Cc, H, W)
    assert torch.equal(A.T.T(x), y) and torch.equal(A.T.adjoint(x), y)
    m = (torch.rand(H, W, generator=torch.Generator().manual_seed(3)) < 0.5).double()
    for comp in (A @ MaskOperator(m), F @ MaskOperator(m)):
        assert _rel(comp(x).reshape(y.shape), g.apply(x * m)) < 1e-13
        assert _rel(comp.adjoint(v), g.adjoint(v) * m) < 1e-13 and _rel(comp.T(v), g.adjoint(v) * m) < 1e-13
    assert _rel((A.T @ A)(x), g.adjoint(g.apply(x))) < 1e-13
    one = RadonOperator(torch.tensor([30.0]), (H, W), det_count=5, det_spacing=2)  # a tensor of angles, an int spacing
    assert one(x).shape == (B, Cc, 1, 5)


def test_errors():
    H, W = 6, 8
    A = RadonOperator(rc.EVEN, (H, W))
    with pytest.raises(ValueError, match="6 x 8"):
        A(torch.zeros(1, 1, H, W + 1))  # a wrong size
    with pytest.raises(ValueError, match="6 x 8"):
        A(torch.zeros(1, 1, W, H))
    with pytest.raises(ValueError, match="B, C, H, W"):
        A(torch.zeros(H, W))
    with pytest.raises(ValueError, match="angles x bins"):
        A.adjoint(torch.zeros(1, 1, len(rc.EVEN), A.det_count + 1))
    with pytest.raises(ValueError, match="angles x bins"):
        A.fbp(torch.zeros(1, 1, len(rc.EVEN) - 1, A.det_count))
    with pytest.raises(ValueError, match="flattened"):
        A.adjoint(torch.zeros(1, len(rc.EVEN) * A.det_count + 1))
    for d in (0.5, 0.999, 8.5, float("nan")):  # d < 1 leaves combs between the bins; d > 8 is past the kernels' window
        with pytest.raises(ValueError, match="det_spacing"):
            RadonOperator(rc.EVEN, (H, W), det_spacing=d)
    assert ops.MAX_RADON_SIZE == 1024 and ops.MAX_RADON_DET == 2048 and ops.MAX_RADON_ANGLES == 4096
    for size in ((1025, 8), (8, 1025), (0, 8), (8,), (8, 8, 8), (8.0, 8), 8):
        with pytest.raises(ValueError, match="size"):
            RadonOperator(rc.EVEN, size)
    for D in (0, 2049, -3, 2.5):
        with pytest.raises(ValueError, match="det_count"):
            RadonOperator(rc.EVEN, (H, W), det_count=D)
    assert RadonOperator(rc.EVEN, (1024, 1024)).det_count == 1451  # (the largest image's default count is within the limit)


def test_errors_of_theta_and_pinv():
    with pytest.raises(ValueError, match="theta"):
        RadonOperator([], (4, 4))
    with pytest.raises(ValueError, match="theta"):
        RadonOperator(torch.zeros(4097), (4, 4))
    with pytest.raises(ValueError, match="theta"):
        RadonOperator([0.0, float("inf")], (4, 4))
    assert RadonOperator(torch.zeros(4096), (4, 4)).angles == 4096
    A = RadonOperator(rc.EVEN, (4, 4))
    with pytest.raises(NotImplementedError, match="fbp"):
        A.pinv(torch.zeros(1, 1, len(rc.EVEN), A.det_count))


def test_host_tensors_never_reach_the_kernels(monkeypatch):
    monkeypatch.setattr(ops, "_launch", lambda *a: pytest.fail("a host tensor reached the kernels"))
    A = RadonOperator(rc.EVEN, (6, 10))
    x = _randn(1, 2, 6, 10, dtype=torch.float32)
    y = A(x)
    assert y.dtype == torch.float32 and A.adjoint(y).shape == x.shape and A.fbp(y).shape == x.shape
    At = RadonOperator(rc.EVEN, (10, 6))
    assert _rel(At(x.transpose(2, 3)).double(), ro.geometry(rc.EVEN, 10, 6).apply(x.transpose(2, 3))) < 1e-5


# ------------------------------------------------------------------------------------------------ FBP of the fp64 model
@pytest.mark.parametrize("d,limit", [(1.0, 0.05), (2.0, 0.07)])
def test_fbp_of_the_fp64_model_reconstructs_a_phantom(d, limit):
    r"""A condition on the DEFINITION (weights, taps, the pi / A factor), not on the kernels: 48 angles over 180 degrees of a
    32 x 32 phantom, relative L2 error inside r < N / 2 - 2.  Measured: 0.0405 (d = 1), 0.0568 (d = 2)."""
    N = 32
    g = ro.geometry(tuple(radon_angles(48).tolist()), N, N, None, d)
    x = rc.phantom(N)
    rec = g.fbp(g.apply(x))
    keep = rc.inner(N)
    err = float((rec - x)[keep].norm() / x[keep].norm())
    print(f"fbp of the fp64 model, d = {d}: relative L2 error {err:.4f}")
    assert err <= limit
    A = RadonOperator(radon_angles(48), (N, N), det_spacing=d)  # and the operator's torch path is that model
    assert _rel(A.fbp(A(x[None, None]))[0, 0], rec) < 1e-12


# ----------------------------------------------------------------------------------------------- the autograd Functions
def test_autograd_of_the_torch_path():
    r"""``torch.sparse.mm`` has no forward-mode rule; the Function around it serves ``func.jvp`` as MMPS calls it."""
    H, W = 7, 5
    A, g = RadonOperator(rc.ANGLES, (H, W), det_spacing=1.5), ro.geometry(rc.ANGLES, H, W, None, 1.5)
    x, w = _randn(2, 2, H, W, seed=1), _randn(2, 2, g.A, g.D, seed=3)
    for fn, M, Mt, a, b in ((A, g.apply, g.adjoint, x, w), (A.fbp, g.fbp, g.fbp_t, w, x), (A.adjoint, g.adjoint, g.apply, w, x)):
        ar = a.clone().requires_grad_()
        assert _rel(torch.autograd.grad(fn(ar), ar, b)[0], Mt(b)) < 1e-13
        y, jv = torch.func.jvp(fn, (a,), (2 * a,))
        assert _rel(y, M(a)) < 1e-13 and _rel(jv, 2 * M(a)) < 1e-13
        y, pull = torch.func.vjp(fn, a)
        assert _rel(pull(b)[0], Mt(b)) < 1e-13
        br = b.clone().requires_grad_()
        gg = torch.autograd.grad(fn(ar), ar, br, create_graph=True)[0]
        assert _rel(torch.autograd.grad(gg, br, a)[0], M(a)) < 1e-13  # double differentiation


def _f32(ptr, n):
    return np.ctypeslib.as_array((C.c_float * n).from_address(ptr))


def _raw_launch(name, *a):
    r"""What the kernels compute, from raw pointers alone -- a functorch wrapper has none to give.  The geometry is rebuilt from
    the angle table the operator uploads: the oracle takes (cos, sin) rows as they are."""
    if name in ("az_op_radon_f32", "az_op_radon_adj_f32"):
        if name == "az_op_radon_f32":
            dst, src, table, work, planes, H, W, A, D, inv = a
            scale = 1.0
        else:
            dst, src, table, planes, H, W, A, D, inv, scale = a
        tab = _f32(table, 2 * A).reshape(A, 2)
        g = _RIGHT[(H, W, D)]
        assert inv == 1.0 and np.array_equal(tab, ro.table(rc.RIGHT_ANGLES))
        if name == "az_op_radon_f32":
            assert work is not None and work % 16 == 0
            out = g.apply(torch.from_numpy(_f32(src, planes * H * W).reshape(planes, H, W).copy()))
            _f32(dst, planes * A * D)[:] = out.numpy().astype(np.float32).ravel()
        else:
            out = g.adjoint(torch.from_numpy(_f32(src, planes * A * D).reshape(planes, A, D).copy())) * np.float32(scale)
            _f32(dst, planes * H * W)[:] = out.numpy().astype(np.float32).ravel()
    elif name == "az_op_radon_filter_f32":
        dst, src, taps, rows, D, scale = a
        t = ro.toeplitz(torch.from_numpy(_f32(taps, D).copy()))
        out = (torch.from_numpy(_f32(src, rows * D).reshape(rows, D).copy()).double() @ t) * np.float32(scale)
        _f32(dst, rows * D)[:] = out.numpy().astype(np.float32).ravel()
    else:
        from test_operators_host import _raw_launch as earlier

        earlier(name, *a)


_RIGHT = {(H, W, D): ro.geometry(rc.RIGHT_ANGLES, H, W, D) for H, W, D in rc.EXACT_HWD}


def _fake_lib_call(name, *a):
    assert name == "az_op_radon_work"
    planes, H, W, floats = a
    floats._obj.value = planes * H * W


def _force_kernels(monkeypatch, calls):
    monkeypatch.setattr(ops, "_use_kernels", lambda x: x.dtype == torch.float32)
    monkeypatch.setattr(ops, "_lib", type("lib", (), {"call": staticmethod(_fake_lib_call)}))
    monkeypatch.setattr(ops, "_launch", lambda name, *a: (calls.append(name), _raw_launch(name, *a))[1])


@pytest.mark.parametrize("flatten", [False, True])
@pytest.mark.parametrize("hwd", [(4, 4, 5), (5, 3, 7), (8, 8, 5)], ids=lambda s: "x".join(map(str, s)))
def test_dispatch_and_transforms_on_the_kernel_path(monkeypatch, flatten, hwd):
    r"""The method of ``test_operators_fft_host.py``: the kernel path forced onto host tensors with a launcher that consumes
    ``data_ptr()``.  fp32 tensors reach exactly the expected entries, and under ``torch.func.jvp`` / ``vjp`` ``backward`` and
    ``jvp`` of the Function never launch on a wrapper.  Right angles and integers: apply and adjoint EQUAL the oracle's."""
    calls = []
    _force_kernels(monkeypatch, calls)
    H, W, D = hwd
    B, Cc = 2, 3
    g = _RIGHT[hwd]
    A = RadonOperator(rc.RIGHT_ANGLES, (H, W), D, flatten=flatten)
    x, v = rc.exact_planes(B, Cc, H, W, 1), rc.exact_planes(B, Cc, H, W, 2)
    shape = A(x).shape
    w = rc.exact_planes(B, Cc, 4, D, 3).reshape(shape)
    want, want_v = g.apply(x).float().reshape(shape), g.apply(v).float().reshape(shape)
    want_t = g.adjoint(w.reshape(B, Cc, 4, D)).float()
    for fn, entries in ((lambda: A(x), ["az_op_radon_f32"]), (lambda: A.adjoint(w), ["az_op_radon_adj_f32"]),
                        (lambda: A.T(w), ["az_op_radon_adj_f32"]), (lambda: A.fbp(w), ["az_op_radon_filter_f32", "az_op_radon_adj_f32"]),
                        (lambda: torch.func.vjp(A.fbp, w)[1](x)[0], ["az_op_radon_filter_f32", "az_op_radon_adj_f32", "az_op_radon_f32",
                                                                      "az_op_radon_filter_f32"])):
        calls.clear()
        fn()
        assert calls == entries
    assert torch.equal(A(x), want) and torch.equal(A.adjoint(w), want_t)
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
    xr, wr = x.clone().requires_grad_(), w.clone().requires_grad_()
    gg = torch.autograd.grad(A(xr), xr, wr, create_graph=True)[0]
    assert torch.equal(gg, want_t) and torch.equal(torch.autograd.grad(gg, wr, v)[0], want_v)
    # fbp and its transpose, (pi / A) h * (A g): within fp32 rounding of the oracle (the taps are no dyadic numbers)
    rec, rec_t = g.fbp(w.reshape(B, Cc, 4, D).double()), g.fbp_t(x.double()).reshape(shape)
    wr = w.clone().requires_grad_()
    for got, ref in ((A.fbp(w), rec), (torch.func.jvp(A.fbp, (w,), (w,))[1], rec), (torch.func.vjp(A.fbp, w)[1](x)[0], rec_t),
                     (torch.autograd.grad(A.fbp(wr), wr, x)[0], rec_t)):
        assert got.shape == ref.shape and _rel(got.double(), ref) < 1e-6
    comp = A @ MaskOperator(torch.ones(H, W))  # a composition reaches both operators' entries
    calls.clear()
    assert torch.equal(comp(x), want) and calls == ["az_op_mul_f32", "az_op_radon_f32"]


# ----------------------------------------------------------------------------------------------------- argument codes
def test_radon_entries_validate_their_arguments():
    from azula_amd import _lib
    from azula_amd.csrc import build

    build.build()
    lib = _lib.lib()
    # aligned bases 32 MiB apart (never dereferenced: every call below fails its validation), and misaligned ones
    P, P2, P3, P4 = 0x10000000, 0x12000000, 0x14000000, 0x16000000
    Q16, Q4 = P + 4, P4 + 2
    NULL, SHAPE, ALIGN = -1, -2, -3

    def fwd(dst=P, src=P2, table=P4, work=P3, planes=2, H=8, W=8, A=4, D=13, inv=1.0):
        return lib.az_op_radon_f32(dst, src, table, work, planes, H, W, A, D, inv, None)

    def adj(dst=P, src=P2, table=P4, planes=2, H=8, W=8, A=4, D=13, inv=1.0, scale=1.0):
        return lib.az_op_radon_adj_f32(dst, src, table, planes, H, W, A, D, inv, scale, None)

    def flt(dst=P, src=P2, taps=P4, rows=8, D=13, scale=1.0):
        return lib.az_op_radon_filter_f32(dst, src, taps, rows, D, scale, None)

    for name in ("dst", "src", "table", "work"):
        assert fwd(**{name: None}) == NULL, name
    for name in ("dst", "src", "table"):
        assert adj(**{name: None}) == NULL, name
    for name in ("dst", "src", "taps"):
        assert flt(**{name: None}) == NULL, name
    for call in (fwd, adj):
        for bad in (dict(planes=0), dict(planes=-1), dict(planes=(1 << 31) + 1), dict(H=0), dict(W=0), dict(H=1025), dict(W=1025),
                    dict(A=0), dict(A=4097), dict(D=0), dict(D=2049), dict(inv=0.1249), dict(inv=1.0001), dict(inv=0.0), dict(inv=-1.0),
                    dict(inv=float("nan"))):
            assert call(**bad) == SHAPE, (call.__name__, bad)
        assert call(dst=Q16) == ALIGN and call(src=Q16 + 0x2000000) == ALIGN and call(table=Q4) == ALIGN
        assert call(dst=P2) == SHAPE and call(src=P + 16) == SHAPE and call(table=P) == SHAPE  # overlap with the destination
    assert fwd(work=P3 + 4) == ALIGN
    assert fwd(work=P) == SHAPE and fwd(work=P2) == SHAPE and fwd(work=P + 4 * 2 * 4 * 13 - 16) == SHAPE  # `work` over dst, src
    assert fwd(work=P4 - 16) == SHAPE  # `work` runs into the table
    for bad in (dict(rows=0), dict(rows=-2), dict(D=0), dict(D=2049)):
        assert flt(**bad) == SHAPE, bad
    assert flt(dst=Q16) == ALIGN and flt(src=P2 + 8) == ALIGN and flt(taps=Q4) == ALIGN
    assert flt(dst=P2) == SHAPE and flt(src=P + 4 * 8 * 13 - 16) == SHAPE and flt(taps=P + 16) == SHAPE
    floats = C.c_int64(-1)
    assert lib.az_op_radon_work(2, 8, 8, None) == NULL
    for bad in ((0, 8, 8), (2, 0, 8), (2, 8, 1025), (2, 1025, 8), (-1, 8, 8)):
        assert lib.az_op_radon_work(*bad, C.byref(floats)) == SHAPE and floats.value == -1
    assert lib.az_op_radon_work(6, 33, 47, C.byref(floats)) == 0 and floats.value == 6 * 33 * 47
    assert lib.az_op_radon_work(1, 1024, 1024, C.byref(floats)) == 0 and floats.value == 1 << 20
