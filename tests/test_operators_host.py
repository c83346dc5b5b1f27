r"""``azula_amd.guidance.operators`` without a GPU: the torch path against the oracle in fp64, the shape conventions and their
errors, the autograd Function under every transform the guidance classes use (on a stand-in launcher that reads raw pointers,
as the real one does), and the argument codes of the new C entries."""

import ctypes as C

import numpy as np
import pytest
import torch

import operator_cases as oc
import operator_oracle as oo
from azula_amd.guidance import BlurOperator, DownsampleOperator, LinearOperator, MaskOperator, gaussian_taps
from azula_amd.guidance import operators as ops

F64 = torch.float64


@pytest.fixture(autouse=True)
def _grad_mode_on():
    r"""Some modules of the suite switch grad mode off for the whole process; these tests differentiate."""
    with torch.enable_grad():
        yield


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def _mask(shape, seed=0):
    gen = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=gen) < 0.6).float() * torch.randint(1, 4, shape, generator=gen)


def _operators(C_, H, W, flatten=False):
    r"""(name, operator, oracle map, observation image shape) for a (C, H, W) input."""
    m = _mask((1, C_, H, W))
    th, tw = oc.random_taps(5, 1), oc.random_taps(3, 2)
    out = [
        ("mask", MaskOperator(m, flatten=flatten), lambda x: oo.mask(x, m), (C_, H, W)),
        ("pool", DownsampleOperator((2, 3), flatten=flatten), lambda x: oo.pool(x, 2, 3), (C_, H // 2, W // 3)),
    ]
    for pad in oc.PADDINGS:
        out.append((f"blur_{pad}", BlurOperator(th, tw, padding=pad, flatten=flatten),
                    lambda x, pad=pad: oo.blur(x, th, tw, pad == "circular"), (C_, H, W)))
    out.append(("pool_of_blur", DownsampleOperator(2, flatten=flatten) @ BlurOperator(th, tw),
                lambda x: oo.pool(oo.blur(x, th, tw, False), 2, 2), (C_, H // 2, W // 2)))
    return out


@pytest.mark.parametrize("flatten", [False, True])
def test_torch_path_matches_the_oracle_in_fp64(flatten):
    B, C_, H, W = 2, 3, 8, 6
    x = oc.random_image(B, C_, H, W, seed=1).double()
    for name, A, ref, oshape in _operators(C_, H, W, flatten):
        want = ref(x)
        w = oc.random_image(*want.shape, seed=2).double()
        y = A(x)
        assert y.dtype == F64 and y.shape == ((B, want[0].numel()) if flatten else want.shape), name
        assert _rel(y.reshape(want.shape), want) < 1e-14, name
        want_t = oo.adjoint(ref, x.shape, w)
        for v in (w, w.flatten(1)) if flatten else (w,):
            assert _rel(A.adjoint(v), want_t) < 1e-14, name
            assert _rel(A.T(v), want_t) < 1e-14, name
        assert A.T.T is A and _rel(A.T.adjoint(x).reshape(want.shape), want) < 1e-14, name
        # torch differentiates the torch path itself
        xr = x.clone().requires_grad_()
        g = torch.autograd.grad(A(xr), xr, w.reshape(A(xr).shape))[0]
        assert _rel(g, want_t) < 1e-14, name


def test_pinv():
    B, C_, H, W = 2, 3, 8, 6
    x = oc.random_image(B, C_, H, W, seed=3).double()
    for flatten in (False, True):
        m = _mask((1, C_, H, W))
        for A, inv in ((MaskOperator(m, flatten=flatten), lambda y: torch.where(m != 0, y / m, 0 * y)),
                       (DownsampleOperator((2, 3), flatten=flatten), lambda y: oo.unpool(y, 2, 3))):
            y = A(x)
            assert _rel(A(A.pinv(y)), y) < 1e-14
            img = y.reshape(B, *A._out_shape((C_, H, W)))
            assert _rel(A.pinv(y), inv(img)) < 1e-14 and _rel(A.pinv(img), inv(img)) < 1e-14
    D = DownsampleOperator(2)
    y = D(x)
    assert torch.equal(D.pinv(y), 4 * D.adjoint(y))
    for A in (BlurOperator([0.25, 0.5, 0.25]), D @ D, D.T, LinearOperator()):
        with pytest.raises(NotImplementedError):
            A.pinv(x)


def test_shape_conventions_and_errors():
    x = torch.zeros(2, 3, 8, 6)
    for A in (MaskOperator(torch.ones(8, 6)), DownsampleOperator(2), BlurOperator([1.0])):
        for bad in (x[0], x.flatten(1), x[None]):
            with pytest.raises(ValueError, match="B, C, H, W"):
                A(bad)
    with pytest.raises(ValueError, match="multiples"):
        DownsampleOperator(4)(x)
    with pytest.raises(ValueError, match="multiples"):
        DownsampleOperator((2, 4))(x)
    with pytest.raises(ValueError):
        DownsampleOperator(17)
    with pytest.raises(ValueError):
        DownsampleOperator(0)
    with pytest.raises(ValueError, match="odd"):
        BlurOperator([0.5, 0.5])
    with pytest.raises(ValueError, match="odd"):
        BlurOperator(torch.ones(67))
    with pytest.raises(ValueError, match="padding"):
        BlurOperator([1.0], padding="reflect")
    with pytest.raises(ValueError, match="circular"):
        BlurOperator(torch.ones(13), padding="circular")(x)  # radius 6 >= W = 6
    assert BlurOperator(torch.ones(11), padding="circular")(x).shape == x.shape
    with pytest.raises(ValueError, match="broadcast"):
        MaskOperator(torch.ones(5, 6))(x)
    # a flat observation needs the image shape: from in_shape= or from the last forward call
    A = DownsampleOperator(2, flatten=True)
    v = torch.zeros(2, 3 * 4 * 3)
    for fn in (A.adjoint, A.pinv, A.T):
        with pytest.raises(ValueError, match="in_shape"):
            fn(v)
    assert DownsampleOperator(2, flatten=True, in_shape=(3, 8, 6)).adjoint(v).shape == x.shape
    assert A(x).shape == v.shape and A.adjoint(v).shape == x.shape and A.pinv(v).shape == x.shape
    with pytest.raises(ValueError, match="flattened"):
        A.adjoint(v[:, :-1])
    with pytest.raises(ValueError):
        A.adjoint(torch.zeros(3))
    M = MaskOperator(torch.ones(1, 3, 8, 6), flatten=True, in_shape=(3, 8, 6))
    assert M.pinv(torch.ones(2, 144)).shape == x.shape


def test_half_and_host_fp32_run_the_torch_path(monkeypatch):
    monkeypatch.setattr(ops, "_launch", lambda *a: pytest.fail("a host tensor reached the kernels"))
    x = oc.exact_image(1, 2, 4, 4)
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        for A in (MaskOperator(torch.ones(4, 4, dtype=torch.bool)), DownsampleOperator(2), BlurOperator([0.25, 0.5, 0.25])):
            y = A(x.to(dtype))
            assert y.dtype == dtype and A.adjoint(y).dtype == dtype


def test_gaussian_taps():
    for sigma, size in ((1.0, 5), (3.0, 61), (0.5, 1), (10.0, 65)):
        t = gaussian_taps(sigma, size)
        assert t.dtype == torch.float32 and t.shape == (size,)
        assert abs(float(t.double().sum()) - 1) <= size * 2.0**-25  # each of `size` roundings moves the sum by at most 2^-25
        assert torch.equal(t, t.flip(0)) and t.argmax() == size // 2
    t = gaussian_taps(1.0, 5).double()
    assert abs(float(t[1] / t[2]) - float(np.exp(-0.5))) < 1e-7
    B = BlurOperator.gaussian(2.0, 9, padding="circular")
    assert torch.equal(B.taps_h, gaussian_taps(2.0, 9)) and torch.equal(B.taps_w, B.taps_h) and B.padding == "circular"


# ----------------------------------------------------------------------------------------------- the autograd Function
def _f32(ptr, n):
    return np.ctypeslib.as_array((C.c_float * n).from_address(ptr))


def _raw_launch(name, *a):
    r"""What the kernels compute, from raw pointers alone -- a functorch wrapper has none to give."""
    if name == "az_op_mul_f32":
        y, x, m, n, m_n = a
        _f32(y, n)[:] = _f32(x, n) * np.tile(_f32(m, m_n), n // m_n)
    elif name == "az_op_avgpool_f32":
        y, x, planes, H, W, fh, fw = a
        src = _f32(x, planes * H * W).reshape(planes, H // fh, fh, W // fw, fw)
        _f32(y, planes * (H // fh) * (W // fw))[:] = (src.sum(axis=(2, 4)) * np.float32(1.0 / (fh * fw))).ravel()
    elif name == "az_op_avgpool_adj_f32":
        dx, g, planes, H, W, fh, fw, scale = a
        src = _f32(g, planes * (H // fh) * (W // fw)).reshape(planes, H // fh, W // fw)
        _f32(dx, planes * H * W)[:] = (np.float32(scale) * src.repeat(fh, axis=1).repeat(fw, axis=2)).ravel()
    elif name == "az_op_blur_f32":
        y, x, th, nh, tw, nw, planes, H, W, circular = a
        src = _f32(x, planes * H * W).reshape(planes, H, W)
        pad = ((0, 0), (nh // 2, nh // 2), (nw // 2, nw // 2))
        src = np.pad(src, pad, mode="wrap") if circular else np.pad(src, pad)
        out = np.zeros((planes, H, W), np.float32)
        for i, ta in enumerate(_f32(th, nh)):
            for j, tb in enumerate(_f32(tw, nw)):
                out += ta * tb * src[:, i:i + H, j:j + W]
        _f32(y, planes * H * W)[:] = out.ravel()
    else:
        raise AssertionError(name)


def _exact_operators(C_, H, W, flatten):
    m = _mask((1, C_, H, W), seed=5)
    th, tw = oc.exact_taps(5), oc.exact_taps(3)
    out = [(MaskOperator(m, flatten=flatten), lambda x: oo.mask(x, m)),
           (MaskOperator(m[:, :1].expand(2, 1, H, W), flatten=flatten), lambda x: oo.mask(x, m[:, :1])),
           (DownsampleOperator((2, 4), flatten=flatten), lambda x: oo.pool(x, 2, 4))]
    for pad in oc.PADDINGS:
        out.append((BlurOperator(th, tw, padding=pad, flatten=flatten), lambda x, pad=pad: oo.blur(x, th, tw, pad == "circular")))
    out.append((DownsampleOperator(2, flatten=flatten) @ BlurOperator(th, tw), lambda x: oo.pool(oo.blur(x, th, tw, False), 2, 2)))
    return out


@pytest.mark.parametrize("flatten", [False, True])
def test_transforms_never_hand_the_launcher_a_wrapped_tensor(monkeypatch, flatten):
    r"""The kernel path forced onto host tensors with a launcher that, like the real one, consumes ``data_ptr()``.  Under
    ``torch.func.jvp`` / ``vjp`` the tensors that ``backward`` and ``jvp`` of the Function receive are wrappers without storage:
    a direct launch on them dies with "Cannot access data pointer"; as applications of the Function they reach ``forward``
    unwrapped.  Exact data, so every result EQUALS the oracle's."""
    calls = []
    monkeypatch.setattr(ops, "_use_kernels", lambda x: x.dtype == torch.float32)
    monkeypatch.setattr(ops, "_launch", lambda name, *a: (calls.append(name), _raw_launch(name, *a))[1])
    B, C_, H, W = 2, 3, 8, 8
    x, v = oc.exact_image(B, C_, H, W, seed=1), oc.exact_image(B, C_, H, W, seed=2)
    for A, ref in _exact_operators(C_, H, W, flatten):
        shape = A(x).shape
        want, want_v = ref(x).reshape(shape), ref(v).reshape(shape)
        w = oc.exact_image(*shape, seed=3)
        want_t = oo.adjoint(lambda z: ref(z).reshape(shape), x.shape, w)
        calls.clear()
        assert torch.equal(A(x), want) and torch.equal(A.adjoint(w), want_t) and calls
        # torch.func.jvp / vjp, as MMPS and JFPS call them
        y, jv = torch.func.jvp(A, (x,), (v,))
        assert torch.equal(y, want) and torch.equal(jv, want_v)
        y, pull = torch.func.vjp(A, x)
        assert torch.equal(y, want) and torch.equal(pull(w)[0], want_t)
        # jvp of the pullback and pullback of the jvp: two levels of wrappers
        assert torch.equal(torch.func.jvp(lambda u: torch.func.vjp(A, x)[1](u)[0], (w,), (w,))[1], want_t)
        assert torch.equal(torch.func.vjp(lambda u: torch.func.jvp(A, (x,), (u,))[1], v)[1](w)[0], want_t)
        # autograd.grad under no_grad with an inner enable_grad, graph retained, as mmps.py / diffpir.py do it
        with torch.no_grad():
            with torch.enable_grad():
                x_hat = x.clone().requires_grad_()
                y_hat = A(x_hat)
            for _ in range(2):
                assert torch.equal(torch.autograd.grad(y_hat, x_hat, w, retain_graph=True)[0], want_t)
            assert torch.equal(torch.func.jvp(A, (x_hat.detach(),), (v,))[1], want_v)
        # second order: d/dw <A^T w, u> = A u
        xr, wr = x.clone().requires_grad_(), w.clone().requires_grad_()
        g = torch.autograd.grad(A(xr), xr, wr, create_graph=True)[0]
        assert torch.equal(g, want_t)
        assert torch.equal(torch.autograd.grad(g, wr, v)[0], want_v)


def test_pinv_goes_through_the_function_too(monkeypatch):
    monkeypatch.setattr(ops, "_use_kernels", lambda x: x.dtype == torch.float32)
    monkeypatch.setattr(ops, "_launch", _raw_launch)
    x = oc.exact_image(2, 3, 8, 8, seed=4)
    m = (_mask((1, 3, 8, 8), seed=6) != 0).float() * 2
    for A, inv in ((MaskOperator(m), lambda y: y * (m / 4)), (DownsampleOperator((2, 4)), lambda y: oo.unpool(y, 2, 4))):
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
    P, P2, Q, T, TQ = 0x100000, 0x900000, 0x500004, 0x1000, 0x1002  # aligned tensors, a misaligned one, taps (never dereferenced)
    NULL, SHAPE, ALIGN = -1, -2, -3
    mul = lambda *a: lib.az_op_mul_f32(*a, None)  # noqa: E731
    assert mul(None, P, P, 16, 16) == NULL and mul(P, None, P, 16, 16) == NULL and mul(P, P, None, 16, 16) == NULL
    assert mul(P, P, P2, 16, 5) == SHAPE and mul(P, P, P2, 0, 1) == SHAPE and mul(P, P, P2, 16, 32) == SHAPE
    assert mul(Q, P, P2, 16, 4) == ALIGN and mul(P, Q, P2, 16, 4) == ALIGN and mul(P, P, Q, 16, 4) == ALIGN
    for name, extra in (("az_op_avgpool_f32", ()), ("az_op_avgpool_adj_f32", (0.25,))):
        fn = lambda *a: getattr(lib, name)(*a, *extra, None)  # noqa: E731, B023
        assert fn(None, P, 1, 8, 8, 2, 2) == NULL and fn(P, None, 1, 8, 8, 2, 2) == NULL
        assert fn(P2, P, 1, 9, 8, 2, 2) == SHAPE and fn(P2, P, 1, 8, 8, 2, 3) == SHAPE  # H % fh, W % fw
        assert fn(P2, P, 1, 34, 8, 17, 2) == SHAPE and fn(P2, P, 1, 8, 8, 0, 2) == SHAPE and fn(P2, P, 0, 8, 8, 2, 2) == SHAPE
        assert fn(Q, P, 1, 8, 8, 2, 2) == ALIGN and fn(P2, Q, 1, 8, 8, 2, 2) == ALIGN
    blur = lambda *a: lib.az_op_blur_f32(*a, None)  # noqa: E731
    assert blur(None, P, T, 3, T, 3, 1, 8, 8, 0) == NULL and blur(P2, P, None, 3, T, 3, 1, 8, 8, 0) == NULL
    assert blur(P2, None, T, 3, T, 3, 1, 8, 8, 0) == NULL and blur(P2, P, T, 3, None, 3, 1, 8, 8, 0) == NULL
    assert blur(P2, P, T, 4, T, 3, 1, 8, 8, 0) == SHAPE and blur(P2, P, T, 3, T, 2, 1, 8, 8, 0) == SHAPE  # even tap counts
    assert blur(P2, P, T, 67, T, 3, 1, 80, 80, 0) == SHAPE and blur(P2, P, T, 3, T, 67, 1, 80, 80, 0) == SHAPE  # more than 65
    assert blur(P2, P, T, 0, T, 3, 1, 8, 8, 0) == SHAPE and blur(P2, P, T, 3, T, 3, 1, 8, 8, 2) == SHAPE
    assert blur(P2, P, T, 17, T, 3, 1, 8, 8, 1) == SHAPE and blur(P2, P, T, 3, T, 17, 1, 8, 8, 1) == SHAPE  # circular, r >= size
    assert blur(P, P, T, 3, T, 3, 1, 8, 8, 0) == SHAPE and blur(P + 64, P, T, 3, T, 3, 1, 8, 8, 0) == SHAPE  # y == x / overlapping
    assert blur(Q, P, T, 3, T, 3, 1, 8, 8, 0) == ALIGN and blur(P2, Q, T, 3, T, 3, 1, 8, 8, 0) == ALIGN
    assert blur(P2, P, TQ, 3, T, 3, 1, 8, 8, 0) == ALIGN and blur(P2, P, T, 3, TQ, 3, 1, 8, 8, 0) == ALIGN
    th, tw = C.c_int32(), C.c_int32()
    assert lib.az_op_blur_tile(3, 3, None, C.byref(tw)) == NULL and lib.az_op_blur_tile(4, 3, C.byref(th), C.byref(tw)) == SHAPE
    for nh, nw in ((1, 1), (3, 5), (65, 1), (1, 65), (65, 65)):
        assert lib.az_op_blur_tile(nh, nw, C.byref(th), C.byref(tw)) == 0
        # tile and halo, staged and row-passed, fit 64 KiB of LDS: two workgroups per CU
        assert tw.value == 64 and 4 <= th.value <= 32 and (th.value + nh - 1) * (2 * tw.value + nw - 1) * 4 <= 65536
        assert ops.blur_tile(nh, nw) == (th.value, tw.value)
