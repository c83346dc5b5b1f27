r"""The entries of ``csrc/nonlinear.hip`` and the operators on them (``PadOperator``, ``MagnitudeOperator``,
``PhaseRetrievalOperator``, ``ClipOperator``, ``QuantizeOperator``) on the GPU.

* exact: ``az_op_cmag_f32`` on every Pythagorean pair at three scales EQUALS the hypotenuse; ``az_op_clip_f32``,
  ``az_op_clip_jac_f32`` and ``az_op_quantize_f32`` are bit-equal to torch's fp32 CPU results, the bounds, +-0 and NaN included;
  ``az_op_pad_f32`` equals ``F.pad`` and the slice;
* accuracy against fp64, elementwise, with bounds that count roundings (``u = 2^-24``): ``cmag`` (both forms) ``2 u |ref|`` --
  ``b b``, the fma and the square root round once each and the root halves what precedes it; ``cmag_vjp`` ``8 u |ref|`` -- at
  most five roundings, the rest leaves the order of the division and the product free; ``cmag_jvp``
  ``8 u (|re t_re| + |im t_im|) / |z|`` -- the sum may cancel, so the bound is on the terms.  Measured worst ratios: DESIGN.md
  section 9g;
* launch forms: every element count, stride form and base offset against one contiguous aligned launch, guard words, a sample
  alone, two runs, one more grid-stride trip than the capped grid covers;
* the operators: accuracy of phase retrieval by section 9d's rule plus the magnitude's own rounding, the transforms' launches,
  and one DPS step (phase retrieval, HDR) and one PGDM step on the ``g28_guidance_vjp`` fixture's UNet.
"""

import math

import pytest
import torch
import torch.nn.functional as F

import fft_oracle as fo
import guidance_vjp_cases as gc
import guidance_vjp_oracle as go
import nonlinear_cases as nc

pytestmark = pytest.mark.gpu
F64 = torch.float64
SENTINEL = 7.5

# entry -> (destination planes, planes of every source group in argument order); the host data of the groups comes as
# {"z": (re, im), "g": (g,), "t": (t_re, t_im)}
CMAG = {"az_op_cmag_f32": (1, ("z",)), "az_op_cmag_vjp_f32": (2, ("g", "z")), "az_op_cmag_jvp_f32": (1, ("t", "z"))}
# the flat entries: sources in argument order
FLAT = {"az_op_clip_f32": ("x",), "az_op_clip_jac_f32": ("g", "x"), "az_op_quantize_f32": ("x",)}


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


def _call(name, *args):
    from azula_amd import _lib

    _lib.call(name, *args, _lib.stream_ptr())


class Planes:
    r"""``k`` planes of (B, n) floats in ONE device buffer full of a sentinel: plane j of sample b starts ``lead + b stride + j n``
    floats in, ``stride = k n + gap``.  ``lead = 1`` offsets every base by one float (the scalar form), ``gap`` and ``lead`` are
    the guard words of a strided destination."""

    def __init__(self, k, B, n, data=None, lead=0, gap=0):
        self.k, self.B, self.n, self.lead, self.stride = k, B, n, lead, k * n + gap
        self.buf = torch.full((lead + B * self.stride + nc.GUARD,), SENTINEL, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        if data is not None:
            body = self.buf[lead:lead + B * self.stride].view(B, self.stride)
            for j, plane in enumerate(data):
                body[:, j * n:(j + 1) * n] = plane.reshape(B, n).cuda()

    def args(self):
        base = self.buf.data_ptr() + 4 * self.lead
        return [base + 4 * j * self.n for j in range(self.k)] + [self.stride]

    def planes(self):
        r"""The k planes as host (B, n) tensors, after asserting that every float outside them still holds the sentinel."""
        buf = self.buf.cpu()
        body = buf[self.lead:self.lead + self.B * self.stride].view(self.B, self.stride)
        assert (buf[:self.lead] == SENTINEL).all() and (buf[self.lead + self.B * self.stride:] == SENTINEL).all()
        assert (body[:, self.k * self.n:] == SENTINEL).all()
        return [body[:, j * self.n:(j + 1) * self.n].clone() for j in range(self.k)]


def run_cmag(name, data, B, n, squared, form="aligned"):
    r"""One launch of a cmag entry on host (B * n,) vectors ``data`` in the stride form ``form``: the destination planes as host
    (B, n) tensors."""
    kd, groups = CMAG[name]
    lead, gap = {"aligned": (0, 0), "offset": (0, 0), "guarded": (nc.GUARD, nc.GUARD), "separate": (0, 0)}[form]
    dst = Planes(kd, B, n, None, lead, gap)
    args = dst.args()
    keep = []
    for i, gname in enumerate(groups):
        planes = data[gname]
        if form == "separate" and len(planes) == 2:  # two tensors instead of the halves of one
            a, b = Planes(1, B, n, planes[:1]), Planes(1, B, n, planes[1:])
            keep += [a, b]
            args += [a.args()[0], b.args()[0], n]
        else:
            src = Planes(len(planes), B, n, planes, lead=1 if form == "offset" and i == 0 else 0)
            keep.append(src)
            args += src.args()
    _call(name, *args, B, n, int(squared))
    return dst.planes()


def run_flat(name, data, n, params, lead_dst=0, lead_src=0):
    dst = Planes(1, 1, n, None, lead_dst)
    srcs = [Planes(1, 1, n, (data[s],), lead_src if i == 0 else 0) for i, s in enumerate(FLAT[name])]
    _call(name, dst.args()[0], *[s.args()[0] for s in srcs], n, *params)
    return dst.planes()[0].reshape(-1)


def _same_bits(a, b):
    r"""Equal as bit patterns, every NaN counting as one value."""
    nan = torch.isnan(a)
    return torch.equal(nan, torch.isnan(b)) and torch.equal(a[~nan].view(torch.int32), b[~nan].view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------ exact
def test_cmag_is_exact_on_pythagorean_pairs():
    re, im, hyp = nc.exact_data()
    n = re.numel()
    (y,) = run_cmag("az_op_cmag_f32", {"z": (re, im)}, 1, n, False)
    assert torch.equal(y.reshape(-1), hyp)
    unit = n // len(nc.SCALES)
    k0 = slice(nc.SCALES.index(0) * unit, (nc.SCALES.index(0) + 1) * unit)
    (y2,) = run_cmag("az_op_cmag_f32", {"z": (re[k0], im[k0])}, 1, unit, True)
    assert torch.equal(y2.reshape(-1).double(), hyp[k0].double() ** 2)
    # the conventions of the linearisations at z = 0 and at a NaN part
    z = (torch.tensor([0.0, -0.0, 3.0, math.nan, 1.0]), torch.tensor([0.0, 0.0, -4.0, 1.0, math.nan]))
    g = torch.tensor([2.0, math.inf, 5.0, 1.0, 1.0])
    for squared in (False, True):
        (y,) = run_cmag("az_op_cmag_f32", {"z": z}, 1, 5, squared)
        assert torch.equal(y[0, :3], torch.tensor([0.0, 0.0, 25.0 if squared else 5.0])) and torch.isnan(y[0, 3:]).all()
        dr, di = run_cmag("az_op_cmag_vjp_f32", {"g": (g,), "z": z}, 1, 5, squared)
        (ty,) = run_cmag("az_op_cmag_jvp_f32", {"t": (g, g), "z": z}, 1, 5, squared)
        assert torch.isnan(dr[0, 3]) and torch.isnan(di[0, 4]) and torch.isnan(ty[0, 3:]).all()  # (a NaN part, where it enters)
        if squared:
            assert torch.equal(dr[0, 2:3], torch.tensor([30.0])) and torch.equal(di[0, 2:3], torch.tensor([-40.0]))
            assert dr[0, 0] == 0 and di[0, 0] == 0 and ty[0, 0] == 0 and ty[0, 2] == -10.0
        else:  # the unit vector is NaN as a whole; exactly 0 at z = 0, whatever g is
            assert torch.isnan(dr[0, 3:]).all() and torch.isnan(di[0, 3:]).all()
            assert _same_bits(dr[0, :2], torch.zeros(2)) and _same_bits(di[0, :2], torch.zeros(2)) and _same_bits(ty[0, :2], torch.zeros(2))
            assert abs(float(dr[0, 2]) - 3.0) <= 4e-7 and abs(float(di[0, 2]) + 4.0) <= 4e-7 and abs(float(ty[0, 2]) + 1.0) <= 4e-7


def test_clip_and_its_jacobian_equal_torch_on_the_cpu():
    n = 4099
    for gain, lo, hi in (nc.CLIP, (-0.5, -0.25, 0.75), (1.0, 0.5, 2.0)):
        x = nc.clip_data(n, gain, lo, hi)
        g = torch.randn(n, generator=torch.Generator().manual_seed(3))
        xr = x.clone().requires_grad_()
        want = torch.clamp(gain * xr, lo, hi)
        (want_d,) = torch.autograd.grad(want, xr, g)
        got = run_flat("az_op_clip_f32", {"x": x}, n, (gain, lo, hi))
        got_d = run_flat("az_op_clip_jac_f32", {"g": g, "x": x}, n, (gain, lo, hi))
        assert _same_bits(got, want.detach()), (gain, lo, hi)
        assert _same_bits(got_d, want_d), (gain, lo, hi)
        assert torch.isnan(got).sum() == 1 and not torch.isnan(got_d).any()


@pytest.mark.parametrize("levels", nc.LEVELS)
def test_quantize_equals_the_torch_sequence_on_the_cpu(levels):
    n = 8197
    for lo, hi in ((-1.0, 1.0), (0.0, 1.0)):
        x = nc.quantize_data(n, levels, lo, hi)
        want = nc.quantize_ref(x, levels, lo, hi)
        got = run_flat("az_op_quantize_f32", {"x": x}, n, (lo, hi, nc.step_of(levels, lo, hi)))
        assert _same_bits(got, want), (levels, lo, hi)
        assert got[~torch.isnan(got)].unique().numel() <= levels


def test_pad_equals_f_pad_and_the_slice():
    B, Cc = nc.PAD_PLANES
    for (H, W), pad in nc.PAD_CASES:
        t, b, l, r = (pad,) * 4 if isinstance(pad, int) else pad
        Hp, Wp = H + t + b, W + l + r
        x = torch.randn(B, Cc, H, W, generator=torch.Generator().manual_seed(H + W))
        w = torch.randn(B, Cc, Hp, Wp, generator=torch.Generator().manual_seed(Hp + Wp))
        for lead in (0, 1):  # (1: the scalar form whatever the widths)
            src, dst = Planes(1, 1, x.numel(), (x.reshape(-1),), lead), Planes(1, 1, w.numel(), None, nc.GUARD)
            _call("az_op_pad_f32", dst.args()[0], src.args()[0], B * Cc, H, W, t, b, l, r, 0)
            assert torch.equal(dst.planes()[0].reshape(B, Cc, Hp, Wp), F.pad(x, (l, r, t, b))), ((H, W), pad, lead)
            src, dst = Planes(1, 1, w.numel(), (w.reshape(-1),), lead), Planes(1, 1, x.numel(), None, nc.GUARD)
            _call("az_op_pad_f32", dst.args()[0], src.args()[0], B * Cc, H, W, t, b, l, r, 1)
            assert torch.equal(dst.planes()[0].reshape(B, Cc, H, W), w[:, :, t:t + H, l:l + W]), ((H, W), pad, lead)


# --------------------------------------------------------------------------------------------------------------- accuracy
@pytest.mark.parametrize("squared", [False, True], ids=["magnitude", "squared"])
def test_accuracy_against_fp64(squared):
    n = 1 << 20
    re, im, g, t_re, t_im = nc.accuracy_data(n, squared)
    (y,) = run_cmag("az_op_cmag_f32", {"z": (re, im)}, 1, n, squared)
    ref = nc.ref_cmag(re, im, squared)
    ratio = float(((y.reshape(-1).double() - ref).abs() / ref).max()) / nc.U
    print(f"cmag squared={squared}: worst |got - ref| / |ref| = {ratio:.3f} * 2^-24 (bound 2)")
    assert ratio <= 2.0
    dr, di = run_cmag("az_op_cmag_vjp_f32", {"g": (g,), "z": (re, im)}, 1, n, squared)
    ref_r, ref_i = nc.ref_vjp(re, im, g, squared)
    ratio = max(float(((d.reshape(-1).double() - r).abs() / r.abs()).max()) for d, r in ((dr, ref_r), (di, ref_i))) / nc.U
    print(f"cmag_vjp squared={squared}: worst |got - ref| / |ref| = {ratio:.3f} * 2^-24 (bound 8)")
    assert ratio <= 8.0
    (ty,) = run_cmag("az_op_cmag_jvp_f32", {"t": (t_re, t_im), "z": (re, im)}, 1, n, squared)
    ref_t, terms = nc.ref_jvp(re, im, t_re, t_im, squared)
    ratio = float(((ty.reshape(-1).double() - ref_t).abs() / terms).max()) / nc.U
    print(f"cmag_jvp squared={squared}: worst |got - ref| / (|re t_re| + |im t_im|) / |z| = {ratio:.3f} * 2^-24 (bound 8)")
    assert ratio <= 8.0


# ----------------------------------------------------------------------------------------------------------- launch forms
def _cmag_data(count, squared):
    re, im, g, t_re, t_im = nc.accuracy_data(count, squared, seed=count)
    re[::7], im[::7] = 0.0, 0.0  # (the z = 0 branch in every form)
    return {"z": (re, im), "g": (g,), "t": (t_re, t_im)}


@pytest.mark.parametrize("name", list(CMAG))
def test_cmag_launch_forms(name):
    r"""Every element count and batch as the halves of one tensor, as separate tensors, with a base offset by one float and into
    a guarded strided destination: the bits of ONE contiguous aligned launch over the same data.  A sample alone and a second
    run: the same bits."""
    for squared in (False, True):
        for B in nc.BATCHES:
            for n in nc.COUNTS:
                data = _cmag_data(B * n, squared)
                want = [p.reshape(B, n) for p in run_cmag(name, data, 1, B * n, squared, "separate")]
                for form in ("aligned", "separate", "offset", "guarded"):
                    got = run_cmag(name, data, B, n, squared, form)
                    assert all(_same_bits(a, b) for a, b in zip(got, want)), (squared, B, n, form)
                if B > 1:
                    one = {k: tuple(p.reshape(B, n)[1] for p in v) for k, v in data.items()}
                    alone = run_cmag(name, one, 1, n, squared, "aligned")
                    assert all(_same_bits(a[0], b[1]) for a, b in zip(alone, want)), (squared, n)
                again = run_cmag(name, data, B, n, squared, "guarded")
                assert all(_same_bits(a, b) for a, b in zip(again, want))


def test_flat_launch_forms():
    gain, lo, hi = nc.CLIP
    for n in nc.COUNTS:
        x, g = nc.clip_data(max(n, 16), gain, lo, hi)[:n], torch.randn(n, generator=torch.Generator().manual_seed(n))
        for name, params in (("az_op_clip_f32", nc.CLIP), ("az_op_clip_jac_f32", nc.CLIP),
                             ("az_op_quantize_f32", (lo, hi, nc.step_of(4, lo, hi)))):
            data = {"x": x, "g": g}
            want = run_flat(name, data, n, params)
            for lead_dst, lead_src in ((1, 0), (0, 1), (nc.GUARD, 0)):
                assert _same_bits(run_flat(name, data, n, params, lead_dst, lead_src), want), (name, n, lead_dst, lead_src)


def test_one_more_trip_than_the_capped_grid():
    r"""More items than one trip of the capped grid covers: the tail runs in the grid-stride loop's second trip.  Against the same
    data in two launches that each stay inside one trip."""
    n, cut = nc.beyond_one_trip(), nc.trip_floats() // 2
    assert n - cut <= nc.trip_floats()
    data = _cmag_data(n, False)
    part = lambda lo, hi: {k: tuple(p[lo:hi] for p in v) for k, v in data.items()}  # noqa: E731
    for name in CMAG:
        got = run_cmag(name, data, 1, n, False)
        head, tail = run_cmag(name, part(0, cut), 1, cut, False), run_cmag(name, part(cut, n), 1, n - cut, False)
        assert all(_same_bits(a, torch.cat([b, c], dim=1)) for a, b, c in zip(got, head, tail)), name
    flat = {"x": data["g"][0], "g": data["t"][0]}
    for name, params in (("az_op_clip_f32", nc.CLIP), ("az_op_clip_jac_f32", nc.CLIP), ("az_op_quantize_f32", (-1.0, 1.0, nc.step_of(256, -1.0, 1.0)))):
        got = run_flat(name, flat, n, params)
        head = run_flat(name, {k: v[:cut] for k, v in flat.items()}, cut, params)
        tail = run_flat(name, {k: v[cut:] for k, v in flat.items()}, n - cut, params)
        assert _same_bits(got, torch.cat([head, tail])), name
    # padding: 5 planes of 512 x 512 to 516 x 520 and back
    x = torch.randn(5, 1, 512, 512, generator=torch.Generator().manual_seed(1)).cuda()
    assert 5 * 516 * 520 > nc.trip_floats() and x.numel() > nc.trip_floats()
    y = torch.empty(5, 1, 516, 520, device="cuda")
    _call("az_op_pad_f32", y.data_ptr(), x.data_ptr(), 5, 512, 512, 1, 3, 4, 4, 0)
    assert torch.equal(y, F.pad(x, (4, 4, 1, 3)))
    back = torch.empty_like(x)
    _call("az_op_pad_f32", back.data_ptr(), y.data_ptr(), 5, 512, 512, 1, 3, 4, 4, 1)
    assert torch.equal(back, x)


# ------------------------------------------------------------------------------------------------ operators on the device
@pytest.mark.parametrize("H", [16, 64, 128], ids=lambda h: f"{h}to{2 * h}")
def test_phase_retrieval_accuracy(H):
    r"""Per plane ``||got - ref||_2 <= bound + 2^-23 S``: the magnitude is 1-Lipschitz, so the transform's rule (section 9d) on the
    padded plane carries over, plus the magnitude's own rounding.  128 -> 256 is the FFT's two-pass form."""
    from azula_amd.guidance import PhaseRetrievalOperator

    x = torch.randn(2, 3, H, H, generator=torch.Generator().manual_seed(H))
    A = PhaseRetrievalOperator(H // 2)
    got = A(x.cuda())
    assert got.shape == (2, 3, 2 * H, 2 * H) and got.dtype == torch.float32
    padded = F.pad(x, (H // 2,) * 4)
    ref = torch.fft.fft2(padded.double())  # unscaled: the rule's convention
    S, e_ref, bound = fo.rule(ref, padded, None, False)
    scale = 1.0 / (2 * H)  # "ortho"
    err = fo.plane_norm(got.double().cpu() - ref.abs() * scale)
    limit = (bound + 2.0**-23 * S) * scale
    print(f"phase retrieval {H}->{2 * H}: worst err / (S s) {float((err / (S * scale)).max()):.3e}, e_ref {float(e_ref.max()):.3e}, "
          f"worst err / limit {float((err / limit).max()):.3f}")
    assert (err <= limit).all()
    Af = PhaseRetrievalOperator(H // 2, flatten=True)
    assert torch.equal(Af(x.cuda()), got.flatten(1))


def test_transforms_issue_the_same_launches(monkeypatch):
    from azula_amd.guidance import ClipOperator, PhaseRetrievalOperator, QuantizeOperator

    gen = torch.Generator().manual_seed(9)
    x, t = torch.randn(2, 3, 16, 32, generator=gen).cuda(), torch.randn(2, 3, 16, 32, generator=gen).cuda()
    names = _spy(monkeypatch)
    pr, inner = {"az_op_pad_f32", "az_op_fft2_f32", "az_op_cmag_f32"}, {"az_op_pad_f32", "az_op_fft2_f32"}
    # operator, the forward's entries, those of the parts inside the outermost one (jacobian(x) runs them again to find its
    # operating point), the pullback's own entry, the tangent map's own entry
    for A, fwd, inner, vjp, jvp in (
            (PhaseRetrievalOperator((8, 8, 16, 16)), pr, inner, "az_op_cmag_vjp_f32", "az_op_cmag_jvp_f32"),
            (PhaseRetrievalOperator((8, 8, 16, 16), "backward", True, flatten=True), pr, inner, "az_op_cmag_vjp_f32", "az_op_cmag_jvp_f32"),
            (ClipOperator(gain=2.0), {"az_op_clip_f32"}, set(), "az_op_clip_jac_f32", "az_op_clip_jac_f32"),
            (QuantizeOperator(16, flatten=True), {"az_op_quantize_f32"}, set(), "az_op_clip_jac_f32", "az_op_clip_jac_f32")):
        names.clear()
        y = A(x)
        assert set(names) == fwd
        w = torch.randn(y.shape, generator=gen).cuda()
        J = A.jacobian(x)
        want_t, want_j = J.adjoint(w), J(t)
        xr = x.clone().requires_grad_()
        for fn, entries in ((lambda: torch.autograd.grad(A(xr), xr, w)[0], fwd | {vjp}), (lambda: torch.func.vjp(A, x)[1](w)[0], fwd | {vjp}),
                            (lambda: A.jacobian(x).T(w), inner | {vjp})):
            names.clear()
            assert torch.equal(fn(), want_t) and set(names) == entries
        for fn, entries in ((lambda: torch.func.jvp(A, (x,), (t,))[1], fwd | {jvp}), (lambda: A.jacobian(x)(t), inner | {jvp})):
            names.clear()
            assert torch.equal(fn(), want_j) and set(names) == entries
        assert torch.equal(torch.func.jvp(A, (x,), (t,))[0], y)
        # The Jacobian against the fp64 torch path at the same point, in the 2-norm, where it is well conditioned (everything but
        # the plain magnitude, whose unit vector divides by |z|: its arithmetic is test_accuracy_against_fp64's and its end-to-end
        # use test_dps_phase_retrieval_step's).  At most two transforms, each within fft_oracle.worst_case of its result's norm,
        # elementwise products at 2^-24 each, and a crop that keeps no less than an eighth of a random tensor's norm: 16 times the
        # transform's worst case.
        if getattr(A.parts[0] if hasattr(A, "parts") else A, "squared", True):
            J64, rel = A.jacobian(x.double().cpu()), 16 * fo.worst_case(32, 64)
            for got, ref in ((want_t, J64.adjoint(w.double().cpu())), (want_j, J64(t.double().cpu()))):
                assert float((got.double().cpu() - ref).norm()) <= rel * float(ref.norm())
        # no launch for fp64 or host tensors
        names.clear()
        y64, yh = A(x.double()), A(x.cpu())
        A.jacobian(x.double()).adjoint(w.double())
        assert not names and y64.dtype == F64 and y64.is_cuda and yh.device.type == "cpu" and yh.dtype == torch.float32
        # a non-contiguous device view gives the result of its contiguous copy
        view = torch.randn(2, 3, 32, 16, generator=gen).cuda().transpose(2, 3)
        assert not view.is_contiguous()
        assert torch.equal(A(view), A(view.contiguous()))
        # a second derivative through the operating point raises
        g1 = torch.autograd.grad(A(xr), xr, w, create_graph=True)[0]
        with pytest.raises(NotImplementedError, match="second derivative"):
            torch.autograd.grad(g1.sum(), xr)


def test_a_jacobian_refuses_other_shapes_before_a_launch(monkeypatch):
    r"""The linearisation entries take every count from the operating point: a tensor of another shape raises and launches
    nothing."""
    from azula_amd.guidance import ClipOperator, MagnitudeOperator, QuantizeOperator

    x = torch.randn(2, 4, 8, 8, generator=torch.Generator().manual_seed(31)).cuda()
    names = _spy(monkeypatch)
    for N in (MagnitudeOperator(), MagnitudeOperator(True, flatten=True), ClipOperator(gain=2.0), QuantizeOperator(4)):
        J = N.jacobian(x)
        w = torch.randn(2, *N._out_shape((4, 8, 8))).cuda()
        for bad in (x[:, :2], x[:, :, :4], x[:1], torch.cat([x, x], dim=3), x[0]):
            with pytest.raises(ValueError):
                J(bad.contiguous())
        for bad in (w[:, :1], w[:, :, :, :4], w[:1], torch.cat([w, w], dim=2), w.flatten(1)[:, :-4]):
            with pytest.raises(ValueError):
                J.adjoint(bad.contiguous())
        assert not names
        assert J(x).flatten(1).shape == w.flatten(1).shape and J.adjoint(w.flatten(1)).shape == x.shape and len(names) == 2
        names.clear()


def test_phase_retrieval_size_rule():
    from azula_amd.guidance import PhaseRetrievalOperator

    with pytest.raises(NotImplementedError, match="96 x 96"):
        PhaseRetrievalOperator(24)(torch.zeros(1, 1, 48, 48, device="cuda"))
    y = PhaseRetrievalOperator(24)(torch.ones(1, 1, 48, 48, device="cuda", dtype=F64))
    assert y.shape == (1, 1, 96, 96) and abs(float(y[0, 0, 0, 0]) - 48 * 48 / 96) < 1e-9


# ---------------------------------------------------------------------------------------------------------------- guidance
def _setup(golden, make_oracle):
    from test_gpu_guidance_vjp import device_denoiser

    g = golden("g28_guidance_vjp")
    mean64, _, arr64, sd, cfg = gc.setup(g, torch.float64)
    mean32, _, arr32, _, _ = gc.setup(g)
    A_oracle = make_oracle()
    gen = torch.Generator().manual_seed(13)
    clean = A_oracle(torch.rand(g["x_t"].shape, generator=gen) - 0.5)
    y = clean + g.meta["var_y"] ** 0.5 * torch.randn(clean.shape, generator=gen)
    return g, device_denoiser(sd, cfg), A_oracle, y, (mean64, arr64), (mean32, arr32)


def _check(tag, out, ref, ref32):
    assert out.shape == ref.shape and torch.isfinite(out).all()
    scale = float(ref.abs().max())
    err, e_ref = float((out.double().cpu() - ref).abs().max()) / scale, float((ref32.double() - ref).abs().max()) / scale
    print(f"{tag}: err {err:.3e} e_ref {e_ref:.3e} bound {max(4 * e_ref, 1e-4):.3e}")
    assert err < max(4 * e_ref, 1e-4)


def _dps(golden, monkeypatch, A, A_oracle_maker, entries, tag, condition=None):
    from test_gpu_guidance_vjp import SEED

    from azula_amd.guidance import DPSSampler

    g, den, A_oracle, y, (mean64, arr64), (mean32, arr32) = _setup(golden, A_oracle_maker)
    if condition is not None:
        condition(mean64(arr64["x_t"], arr64["t"]), mean32(arr32["x_t"], arr32["t"]))
    x_t, t, s = g["x_t"].cuda(), g["t"].cuda(), g["s"].cuda()
    torch.manual_seed(SEED)
    eps = torch.randn_like(x_t).cpu()
    torch.manual_seed(SEED)
    names = _spy(monkeypatch)
    out = DPSSampler(den, y.cuda(), A, steps=g.meta["steps"], silent=True).step(x_t, t, s)
    assert set(names) == entries
    ref = go.dps_step(mean64, arr64["x_t"], arr64["t"], arr64["s"], eps.double(), y=y.double(), A=A_oracle)
    ref32 = go.dps_step(mean32, arr32["x_t"], arr32["t"], arr32["s"], eps, y=y, A=A_oracle)
    _check(tag, out, ref, ref32)


def test_dps_phase_retrieval_step(golden, monkeypatch):
    r"""One DPS step with ``PhaseRetrievalOperator(8, flatten=True)`` (16 -> 32) on the fixture's denoiser, set up as
    ``test_dps_mri_step``: against the fp64 restatement with a ``torch.fft`` lambda as A, at max(4 e_ref, 1e-4).  Checked on the
    CPU: ``e_ref = 2.9e-7``, and the smallest ``|z|`` of the padded spectrum of the fixture's ``x_hat`` is 4e-3 against a median
    of 0.48 -- no bin sits at the singular point."""
    from azula_amd.guidance import PhaseRetrievalOperator

    def condition(x_hat64, _):
        mag = torch.fft.fft2(F.pad(x_hat64, (8, 8, 8, 8)), norm="ortho").abs()
        print(f"dps phase retrieval: smallest |z| {float(mag.min()):.3e}, median {float(mag.median()):.3e}")
        assert float(mag.min()) > 1e-3

    oracle = lambda: (lambda z: torch.fft.fft2(F.pad(z, (8, 8, 8, 8)), norm="ortho").abs().flatten(1))  # noqa: E731
    _dps(golden, monkeypatch, PhaseRetrievalOperator(8, flatten=True), oracle,
         {"az_op_pad_f32", "az_op_fft2_f32", "az_op_cmag_f32", "az_op_cmag_vjp_f32"}, "dps phase retrieval", condition)


def _clip_oracle():
    return lambda z: torch.clamp(2.0 * z, -1.0, 1.0).flatten(1)


def test_dps_hdr_step(golden, monkeypatch):
    r"""One DPS step with ``ClipOperator(gain=2.0, flatten=True)``, the same rule (``e_ref = 2.6e-7`` on the CPU).  Condition, on
    the fp64 oracle's ``x_hat``: the saturated share lies in [0.1, 0.9] and no element of ``2 x_hat`` is within 1e-4 of a bound,
    which keeps fp32 and fp64 on the same side of every kink (measured for this fixture: share 0.81, smallest distance 1.06e-3,
    no side flips between the fp32 and the fp64 restatement)."""
    from azula_amd.guidance import ClipOperator

    def condition(x_hat64, x_hat32):
        u = 2.0 * x_hat64
        share, dist = float((u.abs() > 1).double().mean()), float((u.abs() - 1).abs().min())
        print(f"dps hdr: saturated share {share:.3f}, smallest distance to a bound {dist:.3e}")
        assert 0.1 <= share <= 0.9 and dist >= 1e-4
        assert torch.equal((2.0 * x_hat32).abs() > 1, u.abs() > 1)

    _dps(golden, monkeypatch, ClipOperator(gain=2.0, flatten=True), _clip_oracle, {"az_op_clip_f32", "az_op_clip_jac_f32"},
         "dps hdr", condition)


def test_pgdm_hdr_step(golden, monkeypatch):
    r"""One ``PGDMSampler`` step with the same operator and ``A_inv = y / 2``: a non-differentiable use, so the operator launches
    ``az_op_clip_f32`` and no Jacobian."""
    from test_gpu_guidance_vjp import SEED

    from azula_amd.guidance import ClipOperator, PGDMSampler

    g, den, A_oracle, y, (mean64, arr64), (mean32, arr32) = _setup(golden, _clip_oracle)
    A_inv = lambda v: (v / 2).unflatten(1, (3, 16, 16))  # noqa: E731
    x_t, t, s = g["x_t"].cuda(), g["t"].cuda(), g["s"].cuda()
    torch.manual_seed(SEED)
    eps = torch.randn_like(x_t).cpu()
    torch.manual_seed(SEED)
    names = _spy(monkeypatch)
    out = PGDMSampler(den, y.cuda(), ClipOperator(gain=2.0, flatten=True), A_inv, steps=g.meta["steps"], silent=True).step(x_t, t, s)
    assert set(names) == {"az_op_clip_f32"}
    ref = go.pgdm_step(mean64, arr64["x_t"], arr64["t"], arr64["s"], eps.double(), y=y.double(), A=A_oracle, A_inv=A_inv)
    ref32 = go.pgdm_step(mean32, arr32["x_t"], arr32["t"], arr32["s"], eps, y=y, A=A_oracle, A_inv=A_inv)
    _check("pgdm hdr", out, ref, ref32)
