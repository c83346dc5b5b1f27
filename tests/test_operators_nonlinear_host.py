r"""The nonlinear operators (``NonlinearOperator``, ``MagnitudeOperator``, ``PhaseRetrievalOperator``, ``ClipOperator``,
``QuantizeOperator``) and ``PadOperator`` without a GPU: the torch path in fp64 against independent lambdas, the Jacobians'
transposition, the conventions at the singular points, the rules of the kernel path's Function (run on host tensors through
``NonlinearOperator._function``), the conditions of ``nonlinear_cases`` that the GPU file relies on, and the new entries'
argument checks on the built library."""

import math

import pytest
import torch
import torch.nn.functional as F

import nonlinear_cases as nc
from azula_amd.guidance import (ClipOperator, DownsampleOperator, FourierOperator, LinearOperator, MagnitudeOperator,
                                NonlinearOperator, PadOperator, PhaseRetrievalOperator, QuantizeOperator)

F64 = torch.float64


@pytest.fixture(autouse=True)
def _grad_mode_on():
    r"""Some modules of the suite switch grad mode off for the whole process; these tests differentiate."""
    with torch.enable_grad():
        yield


def _randn(*shape, seed=0):
    return torch.randn(*shape, dtype=F64, generator=torch.Generator().manual_seed(seed))


def _away_from_kinks(x, gain, lo, hi, margin=1e-2):
    r"""``x`` with every element at least ``margin`` from the points where ``gain x`` is a bound (moved outwards)."""
    for bound in (lo / gain, hi / gain):
        near = (x - bound).abs() < margin
        x = torch.where(near, bound + margin * torch.where(x >= bound, 2.0, -2.0), x)
    return x


def _instances():
    r"""(name, operator, input shape (C, H, W), an independent lambda or None)."""
    return [
        ("magnitude", MagnitudeOperator(), (4, 5, 6), lambda z: torch.complex(z[:, :2], z[:, 2:]).abs()),
        ("intensity", MagnitudeOperator(squared=True), (4, 5, 6), lambda z: z[:, :2] ** 2 + z[:, 2:] ** 2),
        ("clip", ClipOperator(gain=2.0), (3, 5, 6), lambda z: torch.clamp(2.0 * z, -1.0, 1.0)),
        ("clip-bounds", ClipOperator(-0.25, 0.75, -1.5), (3, 5, 6), lambda z: torch.clamp(-1.5 * z, -0.25, 0.75)),
        ("quantize", QuantizeOperator(4), (3, 5, 6), None),
        ("chain", MagnitudeOperator() @ FourierOperator() @ PadOperator((1, 2, 0, 1)), (2, 5, 7),
         lambda z: torch.fft.fft2(F.pad(z, (0, 1, 1, 2)), norm="ortho").abs()),
        ("phase-retrieval", PhaseRetrievalOperator(4, norm="backward", squared=True), (3, 8, 8),
         lambda z: torch.fft.fft2(F.pad(z, (4, 4, 4, 4))).abs() ** 2),
        ("linear-on-nonlinear", DownsampleOperator(2) @ ClipOperator(gain=2.0), (3, 4, 6),
         lambda z: F.avg_pool2d(torch.clamp(2.0 * z, -1.0, 1.0), 2)),
        ("nonlinear-on-nonlinear", QuantizeOperator(4) @ ClipOperator(gain=2.0), (3, 4, 6), None),
    ]


INSTANCES = _instances()
IDS = [i[0] for i in INSTANCES]


# ----------------------------------------------------------------------------------------------------------- derivatives
@pytest.mark.parametrize("name, N, in_shape, _", INSTANCES, ids=IDS)
def test_jacobian_and_its_adjoint_are_transposes_in_fp64(name, N, in_shape, _):
    x = _randn(2, *in_shape, seed=1)
    J = N.jacobian(x)
    assert isinstance(J, LinearOperator)
    t, w = _randn(2, *in_shape, seed=2), _randn(*N(x).shape, seed=3)
    y, g = J(t), J.adjoint(w)
    assert y.dtype == F64 and y.shape == w.shape and g.shape == x.shape
    lhs, rhs = float((y * w).sum()), float((t * g).sum())
    bound = 1e-12 * float(y.abs().sum() * w.abs().max())
    print(f"{name}: |<J t, w> - <t, J^T w>| = {abs(lhs - rhs):.3e}, bound {bound:.3e}")
    assert abs(lhs - rhs) <= bound
    assert torch.equal(J.T(w), g) and torch.equal(J.T.T(t), y)
    assert torch.equal((J @ PadOperator(0))(t), y)  # the usual @ of a LinearOperator


@pytest.mark.parametrize("name, N, in_shape, fn", [i for i in INSTANCES if i[3] is not None],
                         ids=[i[0] for i in INSTANCES if i[3] is not None])
def test_gradients_agree_with_an_independent_lambda(name, N, in_shape, fn):
    x, t = _randn(2, *in_shape, seed=4), _randn(2, *in_shape, seed=5)
    close = lambda a, b: float((a - b).abs().max()) <= 1e-12 * float(b.abs().max())  # noqa: E731
    assert close(N(x), fn(x))
    w = _randn(*fn(x).shape, seed=6)
    xr, xl = x.clone().requires_grad_(), x.clone().requires_grad_()
    g, g_ref = torch.autograd.grad(N(xr), xr, w)[0], torch.autograd.grad(fn(xl), xl, w)[0]
    assert close(g, g_ref) and close(N.jacobian(x).adjoint(w), g_ref)
    assert close(torch.func.vjp(N, x)[1](w)[0], g_ref)
    y, ty = torch.func.jvp(N, (x,), (t,))
    y_ref, ty_ref = torch.func.jvp(fn, (x,), (t,))
    assert close(y, y_ref) and close(ty, ty_ref) and close(N.jacobian(x)(t), ty_ref)


def test_gradcheck_of_the_smooth_cases():
    z = _randn(2, 4, 3, 3, seed=7).requires_grad_()
    assert torch.autograd.gradcheck(MagnitudeOperator(squared=True), (z,))
    assert torch.autograd.gradcheck(PhaseRetrievalOperator(1, squared=True), (_randn(1, 2, 2, 2, seed=8).requires_grad_(),))
    x = _away_from_kinks(_randn(2, 3, 4, 4, seed=9), 2.0, -1.0, 1.0).requires_grad_()
    assert float(((2.0 * x.detach()).abs() - 1.0).abs().min()) >= 1e-2
    assert torch.autograd.gradcheck(ClipOperator(gain=2.0), (x,))
    # and through the Function of the kernel path
    assert torch.autograd.gradcheck(MagnitudeOperator(squared=True)._function, (z,))
    assert torch.autograd.gradcheck(ClipOperator(gain=2.0)._function, (x,))


@pytest.mark.parametrize("name, N, in_shape, _", INSTANCES[:5], ids=IDS[:5])
def test_the_function_of_the_kernel_path_on_host_tensors(name, N, in_shape, _):
    r"""``_function`` runs host tensors through the Functions the kernels sit in: ``backward`` is ``jacobian(x).adjoint``, ``jvp``
    is ``jacobian(x)``, under ``autograd.grad`` and under ``torch.func``; the Jacobian's own derivative with respect to what it
    is applied to is the transposed / same map; a second derivative through ``x`` raises in every transform."""
    x, t = _randn(2, *in_shape, seed=10), _randn(2, *in_shape, seed=11)
    w = _randn(*N(x).shape, seed=12)
    J = N.jacobian(x)
    xr = x.clone().requires_grad_()
    assert torch.equal(N._function(x), N(x))
    assert torch.equal(torch.autograd.grad(N._function(xr), xr, w)[0], J.adjoint(w))
    assert torch.equal(torch.func.vjp(N._function, x)[1](w)[0], J.adjoint(w))
    assert torch.equal(torch.func.jvp(N._function, (x,), (t,))[1], J(t))
    # linear in its argument: differentiating J(x)^T w with respect to w gives J(x)
    wr = w.clone().requires_grad_()
    g1 = torch.autograd.grad(N._function(xr), xr, wr, create_graph=True)[0]
    assert torch.equal(torch.autograd.grad(g1, wr, t)[0], J(t))
    # second derivatives through the operating point
    g1 = torch.autograd.grad(N._function(xr), xr, w, create_graph=True)[0]  # (first order: does not raise)
    with pytest.raises(NotImplementedError, match="second derivative"):
        torch.autograd.grad(g1.sum(), xr)
    g1 = torch.autograd.grad(N._function(xr), xr, w, create_graph=True)[0]
    with pytest.raises(NotImplementedError, match="second derivative"):
        g1.sum().backward()
    with pytest.raises(NotImplementedError, match="second derivative"):
        torch.func.grad(lambda z: torch.func.vjp(N._function, z)[1](w)[0].sum())(x)
    with pytest.raises(NotImplementedError, match="second derivative"):
        torch.func.jvp(lambda z: torch.func.jvp(N._function, (z,), (t,))[1], (x,), (t,))


# ----------------------------------------------------------------------------------------------------------- conventions
def test_exact_conventions():
    nan = math.nan
    for squared in (False, True):
        M = MagnitudeOperator(squared)
        z = torch.tensor([[0.0, 3.0, nan], [0.0, 4.0, 1.0]], dtype=F64).reshape(1, 2, 1, 3).requires_grad_()
        y = M(z)
        assert y[0, 0, 0, 0] == 0 and y[0, 0, 0, 1] == (25.0 if squared else 5.0) and torch.isnan(y[0, 0, 0, 2])
        w = torch.full((1, 1, 1, 3), 2.0, dtype=F64)
        for g in (torch.autograd.grad(y, z, w)[0], M.jacobian(z.detach()).adjoint(w)):
            assert g[0, 0, 0, 0] == 0 and g[0, 1, 0, 0] == 0  # z = 0: a zero row
            assert torch.allclose(g[0, :, 0, 1], torch.tensor([12.0, 16.0] if squared else [1.2, 1.6], dtype=F64), rtol=1e-15)
        t = torch.ones(1, 2, 1, 3, dtype=F64)
        assert M.jacobian(z.detach())(t)[0, 0, 0, 0] == 0
    A = ClipOperator(-1.0, 1.0, gain=2.0)
    x = torch.tensor([0.5, -0.5, 0.5 + 2**-50, -0.5 - 2**-50, 0.0, nan], dtype=F64).reshape(1, 1, 1, 6).requires_grad_()
    y = A(x)
    assert torch.equal(y[0, 0, 0, :5], torch.tensor([1.0, -1.0, 1.0, -1.0, 0.0], dtype=F64)) and torch.isnan(y[0, 0, 0, 5])
    w = torch.full((1, 1, 1, 6), 3.0, dtype=F64)
    want = torch.tensor([6.0, 6.0, 0.0, 0.0, 6.0, 0.0], dtype=F64)  # on a bound: passes; beyond: not; NaN: a zero cotangent
    assert torch.equal(torch.autograd.grad(y, x, w)[0].reshape(-1), want)
    assert torch.equal(A.jacobian(x.detach()).adjoint(w).reshape(-1), want) and torch.equal(A.jacobian(x.detach())(w).reshape(-1), want)
    xr = x.detach().clone().requires_grad_()
    assert torch.equal(torch.autograd.grad(A._function(xr), xr, w)[0].reshape(-1), want)


def test_quantize_is_the_written_out_sequence():
    for levels in nc.LEVELS:
        for lo, hi in ((-1.0, 1.0), (0.0, 1.0)):
            Q = QuantizeOperator(levels, lo, hi)
            assert Q.step == nc.step_of(levels, lo, hi)
            for dtype in (torch.float32, F64):
                x = nc.quantize_data(4096, levels, lo, hi).to(dtype).reshape(1, 1, 64, 64)
                q = Q(x)
                ref = nc.quantize_ref(x, levels, lo, hi)
                assert q.dtype == dtype and torch.equal(q.nan_to_num(7.0), ref.nan_to_num(7.0))
                assert torch.isnan(q).sum() == 1 and q[~torch.isnan(q)].unique().numel() <= levels
                assert float(q[~torch.isnan(q)].min()) == lo and abs(float(q[~torch.isnan(q)].max()) - hi) <= 2e-7 * levels
    # the straight-through Jacobian: the clamp's
    Q = QuantizeOperator(4)
    x = torch.tensor([-1.5, -1.0, 0.1, 1.0, 1.5, math.nan], dtype=F64).reshape(1, 1, 1, 6).requires_grad_()
    g = torch.autograd.grad(Q(x), x, torch.full((1, 1, 1, 6), 3.0, dtype=F64))[0]
    assert torch.equal(g.reshape(-1), torch.tensor([0.0, 3.0, 3.0, 3.0, 0.0, 0.0], dtype=F64))


def test_phase_retrieval_is_the_chain():
    x = _randn(2, 3, 8, 8, seed=13)
    for pad, norm, squared in ((4, "ortho", False), ((1, 3, 0, 4), "backward", True)):
        A = PhaseRetrievalOperator(pad, norm, squared)
        chain = MagnitudeOperator(squared) @ FourierOperator(norm) @ PadOperator(pad)
        assert isinstance(A, NonlinearOperator) and isinstance(chain, NonlinearOperator)
        assert torch.equal(A(x), chain(x)) and torch.equal(A(x.float()), chain(x.float()))
        w = _randn(*A(x).shape, seed=14)
        assert torch.equal(A.jacobian(x).adjoint(w), chain.jacobian(x).adjoint(w))
        assert torch.equal(A.jacobian(x)(x), chain.jacobian(x)(x))


def test_pad_operator():
    for (H, W), pad in nc.PAD_CASES:
        P = PadOperator(pad)
        t, b, l, r = (pad,) * 4 if isinstance(pad, int) else pad
        x = _randn(*nc.PAD_PLANES, H, W, seed=15)
        y = P(x)
        assert torch.equal(y, F.pad(x, (l, r, t, b))) and torch.equal(P.pinv(y), x) and torch.equal(P.adjoint(y), x)
        w = _randn(*y.shape, seed=16)
        assert torch.equal(P.adjoint(w), w[:, :, t:t + H, l:l + W]) and torch.equal(P.T(w), P.adjoint(w))
        for m, tm in P._TRANSPOSE.items():  # the modes' transposition check
            a, c = (x, w) if m in ("apply", "pinv_t") else (w, x)
            lhs, rhs = float((P._torch(a, m) * c).sum()), float((a * P._torch(c, tm)).sum())
            assert abs(lhs - rhs) <= 1e-12 * float(P._torch(a, m).abs().sum() * c.abs().max())
        Pf = PadOperator(pad, flatten=True)
        assert torch.equal(Pf(x), y.flatten(1)) and torch.equal(Pf.pinv(y.flatten(1)), x)
    for bad in (-1, (1, 2, 3), (1, 2, 3, -4), 1.5):
        with pytest.raises(ValueError):
            PadOperator(bad)
    with pytest.raises(ValueError):
        PadOperator(4).adjoint(torch.zeros(1, 1, 7, 9))


# ------------------------------------------------------------------------------------------------------ shapes and errors
def test_shapes_flatten_and_errors():
    x = _randn(2, 4, 6, 6, seed=17)
    M, Mf = MagnitudeOperator(), MagnitudeOperator(flatten=True)
    assert Mf(x).shape == (2, 2 * 36) and torch.equal(Mf(x), M(x).flatten(1)) and Mf.in_shape == (4, 6, 6)
    w = _randn(2, 2, 6, 6, seed=18)
    J = Mf.jacobian(x)
    assert torch.equal(J.adjoint(w.flatten(1)), M.jacobian(x).adjoint(w)) and torch.equal(J.adjoint(w), J.adjoint(w.flatten(1)))
    assert J(x).shape == (2, 72)
    A = PhaseRetrievalOperator(3, flatten=True, in_shape=(2, 6, 6))
    assert A.in_shape == (2, 6, 6) and A.flatten and A(x[:, :2]).shape == (2, 2 * 12 * 12)
    assert A.jacobian(x[:, :2]).adjoint(_randn(2, 2 * 144, seed=19)).shape == (2, 2, 6, 6)
    assert ClipOperator(flatten=True)(x).shape == (2, 144) and QuantizeOperator(8, flatten=True)(x).shape == (2, 144)
    with pytest.raises(ValueError, match="even channel count"):
        MagnitudeOperator()(x[:, :3])
    with pytest.raises(ValueError, match="even channel count"):
        MagnitudeOperator().jacobian(x[:, :3])
    for bad in (lambda: ClipOperator(1.0, 1.0), lambda: ClipOperator(2.0, 1.0), lambda: ClipOperator(high=math.inf),
                lambda: ClipOperator(low=math.nan), lambda: ClipOperator(gain=math.inf), lambda: QuantizeOperator(1),
                lambda: QuantizeOperator(2.5), lambda: QuantizeOperator(4, 1.0, 1.0), lambda: MagnitudeOperator(in_shape=(2, 3)),
                lambda: MagnitudeOperator(flatten=True) @ FourierOperator(flatten=True)):
        with pytest.raises(ValueError):
            bad()
    for N in (MagnitudeOperator(), ClipOperator(), QuantizeOperator(4), PhaseRetrievalOperator(2), PadOperator(1)):
        with pytest.raises(ValueError, match=r"\(B, C, H, W\)"):
            N(torch.zeros(4, 6, 6))
    with pytest.raises(ValueError, match="Jacobian"):
        M.jacobian(x)(x[:1])
    with pytest.raises(TypeError):
        MagnitudeOperator() @ (lambda z: z)
    with pytest.raises(NotImplementedError):
        MagnitudeOperator()(x.to(torch.bfloat16))


def test_a_jacobian_takes_only_the_shapes_of_its_operating_point():
    r"""The kernels take every count from ``x``, so a tensor of another shape must never reach them: whatever the operator's own
    shape rules would accept, ``jacobian(x)`` takes ``x``'s shape and pulls back ``N(x)``'s, 4-D or flat, and a refused call
    leaves the recorded shape alone."""
    x = _randn(2, 4, 6, 6, seed=20)
    for N in (MagnitudeOperator(), MagnitudeOperator(flatten=True), ClipOperator(gain=2.0), QuantizeOperator(4, flatten=True),
              PhaseRetrievalOperator(1)):
        J = N.jacobian(x)
        out = tuple(N(x).shape[1:]) if not N.flatten else tuple(N._out_shape((4, 6, 6)))
        for bad in (x[:, :2], x[:, :, :4], x[:, :, :, :5], x[:1], torch.cat([x, x], dim=2), x.flatten(1), x[0]):
            with pytest.raises(ValueError):
                J(bad)
        w = _randn(2, *out, seed=21)
        for bad in (w[:, :1], w[:, :, :3], w[:1], torch.cat([w, w], dim=3), w.flatten(1)[:, :-1], w[0]):
            with pytest.raises(ValueError):
                J.adjoint(bad)
        assert J.in_shape in ((4, 6, 6), None)  # (None: the chain's composition, whose parts hold the shapes)
        assert J(x).shape == N(x).shape and J.adjoint(w).shape == x.shape and J.adjoint(w.flatten(1)).shape == x.shape


def test_a_chain_with_a_flattening_linear_part_outermost():
    r"""``jacobian(x)`` does not call the outermost part; a linear one that flattens and was never applied still un-flattens a
    flat cotangent: the chain records the shape it would have seen."""
    x, t = _randn(2, 3, 4, 6, seed=23), _randn(2, 3, 4, 6, seed=24)
    A = DownsampleOperator(2, flatten=True) @ ClipOperator(gain=2.0)
    J = A.jacobian(x)
    w = _randn(2, 3 * 2 * 3, seed=25)
    g = J.adjoint(w)
    assert g.shape == x.shape and J(t).shape == (2, 18)
    ref = (DownsampleOperator(2) @ ClipOperator(gain=2.0)).jacobian(x)
    assert torch.equal(g, ref.adjoint(w.unflatten(1, (3, 2, 3)))) and torch.equal(J(t), ref(t).flatten(1))
    xr = x.clone().requires_grad_()
    assert torch.equal(torch.autograd.grad(A(xr), xr, w)[0], g)


# ---------------------------------------------------------------------------------------- the conditions of the GPU file
def test_the_emulated_arithmetic_is_exact_on_the_exact_data():
    pairs = nc.pythagorean_pairs()
    assert pairs.shape[0] == 4530 and int(pairs[:, 2].max()) < 4096
    assert torch.equal(pairs[:, 0] ** 2 + pairs[:, 1] ** 2, pairs[:, 2] ** 2) and (pairs[:, 0] < pairs[:, 1]).all()
    re, im, hyp = nc.exact_data()
    assert re.numel() == len(nc.SCALES) * (2 * pairs.shape[0] + 14)
    assert torch.equal(re.double() ** 2 + im.double() ** 2, hyp.double() ** 2)  # (fp64 holds the squares exactly)
    assert torch.equal(nc.emulate_cmag(re, im), hyp)
    assert ((re == 0) & (im == 0)).sum() >= 2 * len(nc.SCALES) and (re < 0).any() and (im < 0).any()
    unit = re.numel() // len(nc.SCALES)
    sq = re[unit:2 * unit].double() ** 2 + im[unit:2 * unit].double() ** 2  # k = 0: |z|^2 < 2^24 is an fp32 integer
    assert torch.equal(sq.float().double(), sq)


def test_the_accuracy_data_and_the_emulation():
    for squared in (False, True):
        re, im, g, t_re, t_im = nc.accuracy_data(1 << 16, squared)
        ratio = (im.abs() / re.abs()).log2()
        assert torch.isfinite(ratio).all() and float(re.abs().log2().max() - re.abs().log2().min()) > 100 / (2 if squared else 1)
        ref = nc.ref_cmag(re, im, squared)
        assert float(ref.max()) < 2.0**120 and float(ref.min()) > 2.0**-120  # normal fp32 numbers throughout
    re, im = nc.accuracy_data(1 << 18, False)[:2]
    ref = nc.ref_cmag(re, im, False)
    worst = float(((nc.emulate_cmag(re, im).double() - ref).abs() / ref).max()) / nc.U
    print(f"emulated cmag: worst error {worst:.3f} * 2^-24")
    assert worst <= 2.0  # the bound the GPU file asserts: 2^-23 |ref|


def test_clip_and_quantize_data_hit_their_edges():
    gain, lo, hi = nc.CLIP
    x = nc.clip_data(64, gain, lo, hi)
    u = gain * x
    assert (u == lo).any() and (u == hi).any() and (u > hi).any() and (u < lo).any() and torch.isnan(x).sum() == 1
    assert torch.equal(torch.signbit(x[6:8]), torch.tensor([False, True])) and (x[6:8] == 0).all()
    for levels in nc.LEVELS:
        x = nc.quantize_data(256, levels, -1.0, 1.0)
        assert (x < -1).any() and (x > 1).any() and torch.isnan(x).sum() == 1
    assert nc.beyond_one_trip() > nc.trip_floats() >= 4 * 256 and nc.beyond_one_trip() % 4 != 0


# ------------------------------------------------------------------------------------------------------------------ C ABI
def test_new_entries_return_argument_errors():
    r"""Every new entry validates its arguments BEFORE touching the device and reports through its int status: checkable without
    a GPU, as ``test_cabi.py::test_argument_errors_are_returned_not_raised``."""
    from azula_amd import _lib
    from azula_amd.csrc import build

    build.build()
    lib = _lib.lib()
    NULL, SHAPE, ALIGN = -1, -2, -3
    a, b, c, d = 0x10000, 0x20000, 0x30000, 0x40000  # (never dereferenced: every call below fails its checks or is empty)
    # cmag: y, y_bs, z_re, z_im, z_bs, B, n, squared
    assert lib.az_op_cmag_f32(None, 16, b, c, 16, 1, 16, 0, None) == NULL
    assert lib.az_op_cmag_f32(a, 16, b, None, 16, 1, 16, 0, None) == NULL
    assert lib.az_op_cmag_f32(a, 16, b, c, 16, 1, -1, 0, None) == SHAPE
    assert lib.az_op_cmag_f32(a, 16, b, c, 16, -1, 16, 0, None) == SHAPE
    assert lib.az_op_cmag_f32(a, 16, b, c, -16, 1, 16, 0, None) == SHAPE
    assert lib.az_op_cmag_f32(a, 8, b, c, 16, 2, 16, 0, None) == SHAPE  # a tensor's own samples overlap
    assert lib.az_op_cmag_f32(a, 16, b, c, 16, 1, 16, 2, None) == SHAPE
    assert lib.az_op_cmag_f32(a + 2, 16, b, c, 16, 1, 16, 0, None) == ALIGN
    assert lib.az_op_cmag_f32(a, 16, a + 32, c, 16, 1, 16, 0, None) == SHAPE  # y overlaps z_re
    assert lib.az_op_cmag_f32(a, 16, b, a, 16, 1, 16, 0, None) == SHAPE  # y is z_im
    assert lib.az_op_cmag_f32(None, 0, None, None, 0, 0, 16, 0, None) == 0 and lib.az_op_cmag_f32(None, 0, None, None, 0, 3, 0, 1, None) == 0
    # cmag_vjp: d_re, d_im, d_bs, g, g_bs, z_re, z_im, z_bs, B, n, squared
    assert lib.az_op_cmag_vjp_f32(a, None, 32, b, 16, c, d, 32, 1, 16, 0, None) == NULL
    assert lib.az_op_cmag_vjp_f32(a, a + 64, 32, None, 16, c, d, 32, 1, 16, 0, None) == NULL
    assert lib.az_op_cmag_vjp_f32(a, a + 64, 32, b, 16, c, d, 32, 1, -4, 0, None) == SHAPE
    assert lib.az_op_cmag_vjp_f32(a, a + 32, 32, b, 16, c, d, 32, 1, 16, 0, None) == SHAPE  # d_re overlaps d_im
    assert lib.az_op_cmag_vjp_f32(a, a + 64, 32, b, 16, a + 64, d, 32, 2, 16, 0, None) == SHAPE  # d_im is z_re
    assert lib.az_op_cmag_vjp_f32(a, a + 64, 32, a + 4, 16, c, d, 32, 1, 16, 0, None) == SHAPE  # d_re overlaps g
    assert lib.az_op_cmag_vjp_f32(a, a + 64, 32, b + 1, 16, c, d, 32, 1, 16, 0, None) == ALIGN
    assert lib.az_op_cmag_vjp_f32(None, None, 0, None, 0, None, None, 0, 0, 0, 0, None) == 0
    # cmag_jvp: t_y, y_bs, t_re, t_im, t_bs, z_re, z_im, z_bs, B, n, squared
    assert lib.az_op_cmag_jvp_f32(a, 16, b, None, 32, c, d, 32, 1, 16, 0, None) == NULL
    assert lib.az_op_cmag_jvp_f32(a, 16, b, b + 64, 32, c, None, 32, 1, 16, 0, None) == NULL
    assert lib.az_op_cmag_jvp_f32(a, 16, b, b + 64, 32, c, c + 64, 8, 2, 16, 0, None) == SHAPE
    assert lib.az_op_cmag_jvp_f32(a, 16, a + 60, b, 32, c, d, 32, 1, 16, 0, None) == SHAPE  # t_y overlaps t_re
    assert lib.az_op_cmag_jvp_f32(a, 16, b, b + 64, 32, c, d + 3, 32, 1, 16, 0, None) == ALIGN
    # clip: y, x, n, gain, lo, hi;  clip_jac: d, g, x, n, gain, lo, hi;  quantize: q, x, n, lo, hi, step
    assert lib.az_op_clip_f32(None, b, 16, 2.0, -1.0, 1.0, None) == NULL and lib.az_op_clip_f32(a, None, 16, 2.0, -1.0, 1.0, None) == NULL
    assert lib.az_op_clip_f32(a, b, -1, 2.0, -1.0, 1.0, None) == SHAPE and lib.az_op_clip_f32(a, b, 16, 2.0, 1.0, 1.0, None) == SHAPE
    assert lib.az_op_clip_f32(a, b, 16, math.inf, -1.0, 1.0, None) == SHAPE and lib.az_op_clip_f32(a, b, 16, 2.0, math.nan, 1.0, None) == SHAPE
    assert lib.az_op_clip_f32(a, a, 16, 2.0, -1.0, 1.0, None) == SHAPE and lib.az_op_clip_f32(a, a + 60, 16, 2.0, -1.0, 1.0, None) == SHAPE
    assert lib.az_op_clip_f32(a + 1, b, 16, 2.0, -1.0, 1.0, None) == ALIGN and lib.az_op_clip_f32(None, None, 0, 2.0, -1.0, 1.0, None) == 0
    assert lib.az_op_clip_jac_f32(a, None, c, 16, 2.0, -1.0, 1.0, None) == NULL and lib.az_op_clip_jac_f32(a, b, None, 16, 2.0, -1.0, 1.0, None) == NULL
    assert lib.az_op_clip_jac_f32(a, b, c, -16, 2.0, -1.0, 1.0, None) == SHAPE and lib.az_op_clip_jac_f32(a, b, c, 16, 2.0, 1.0, -1.0, None) == SHAPE
    assert lib.az_op_clip_jac_f32(a, a + 32, c, 16, 2.0, -1.0, 1.0, None) == SHAPE and lib.az_op_clip_jac_f32(a, b, a, 16, 2.0, -1.0, 1.0, None) == SHAPE
    assert lib.az_op_clip_jac_f32(a, b + 2, c, 16, 2.0, -1.0, 1.0, None) == ALIGN and lib.az_op_clip_jac_f32(None, None, None, 0, 2.0, -1.0, 1.0, None) == 0
    assert lib.az_op_quantize_f32(None, b, 16, -1.0, 1.0, 0.5, None) == NULL and lib.az_op_quantize_f32(a, b, -1, -1.0, 1.0, 0.5, None) == SHAPE
    assert lib.az_op_quantize_f32(a, b, 16, -1.0, 1.0, 0.0, None) == SHAPE and lib.az_op_quantize_f32(a, b, 16, 1.0, -1.0, 0.5, None) == SHAPE
    assert lib.az_op_quantize_f32(a, a + 4, 16, -1.0, 1.0, 0.5, None) == SHAPE and lib.az_op_quantize_f32(a, b + 3, 16, -1.0, 1.0, 0.5, None) == ALIGN
    assert lib.az_op_quantize_f32(None, None, 0, -1.0, 1.0, 0.5, None) == 0
    # pad: dst, src, planes, H, W, top, bottom, left, right, adjoint
    assert lib.az_op_pad_f32(None, b, 1, 4, 4, 1, 1, 1, 1, 0, None) == NULL and lib.az_op_pad_f32(a, None, 1, 4, 4, 1, 1, 1, 1, 1, None) == NULL
    assert lib.az_op_pad_f32(a, b, -1, 4, 4, 1, 1, 1, 1, 0, None) == SHAPE and lib.az_op_pad_f32(a, b, 1, 4, 4, -1, 1, 1, 1, 0, None) == SHAPE
    assert lib.az_op_pad_f32(a, b, 1, 4, -4, 1, 1, 1, 1, 0, None) == SHAPE and lib.az_op_pad_f32(a, b, 1, 4, 4, 1, 1, 1, 1, 2, None) == SHAPE
    assert lib.az_op_pad_f32(a, a + 64, 1, 4, 4, 1, 1, 1, 1, 0, None) == SHAPE  # the 6 x 6 destination covers the source
    assert lib.az_op_pad_f32(a + 64, a, 1, 4, 4, 1, 1, 1, 1, 1, None) == SHAPE  # the crop's source covers its destination
    assert lib.az_op_pad_f32(a, b + 2, 1, 4, 4, 1, 1, 1, 1, 0, None) == ALIGN
    assert lib.az_op_pad_f32(None, None, 0, 4, 4, 1, 1, 1, 1, 0, None) == 0 and lib.az_op_pad_f32(None, None, 3, 0, 4, 1, 1, 1, 1, 1, None) == 0
    assert lib.az_op_nonlinear_trip(None) == NULL
