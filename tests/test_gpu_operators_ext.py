r"""``PSFOperator``, ``DecimateOperator`` and ``ChannelMixOperator`` on the GPU: the kernels ``az_op_psf_f32``,
``az_op_decimate_f32`` / ``az_op_decimate_adj_f32`` and ``az_op_chanmix_f32`` against the torch-op restatement of
``tests/operator_ext_oracle.py`` run on the host in fp64.

* exact data (``tests/operator_ext_cases.py``: small integers, dyadic PSFs that differ per PSF number, dyadic matrices):
  ``torch.equal`` with the fp64 oracle -- PSF forward and adjoint at 9 radius pairs x both paddings x 4 (B, C) x every PSF shape
  form x 8 sizes around the tile, more tiles than the launch has workgroups, 70 000 planes; decimation (a copy: random data too)
  at every offset of 5 factors x 5 output sizes; channel mix, its adjoint and its pseudo-inverse at 5 channel pairs x 5 pixel counts;
* random data: within bounds derived from the number of fp32 operations per output,
      PSF  (kh kw + 2) * 2^-24 * sum|k| * max|x|                  (one rounding per FMA of the chain at the inputs' scale, two for
      mix  (Cin + 2) * 2^-24 * max_o sum_c|M[o, c]| * max|x|       the conversion of the operands -- as the blur's bound is formed)
* adjointness on the exact data with fp64 dot products, the autograd Function (bit for bit: the same launches), and the
  guidance classes end to end: DiffPIR motion deblurring and bicubic super-resolution, one DPS step of colourisation.
"""

import pytest
import torch

import diffpir_oracle as do
import guidance_vjp_cases as gc
import guidance_vjp_oracle as go
import operator_cases as oc
import operator_ext_cases as xc
import operator_ext_oracle as xo
import operator_oracle as oo

pytestmark = pytest.mark.gpu
U = 2.0**-24
NEW = {"psf": {"az_op_psf_f32"}, "decimate": {"az_op_decimate_f32", "az_op_decimate_adj_f32"}, "mix": {"az_op_chanmix_f32"},
       "blur": {"az_op_blur_f32"}}


def _ops():
    from azula_amd.guidance import operators

    return operators


def _spy(monkeypatch):
    ops = _ops()
    names, launch = [], ops._launch
    monkeypatch.setattr(ops, "_launch", lambda name, *a: (names.append(name), launch(name, *a))[1])
    return names


# ------------------------------------------------------------------------------------------------------------- exact: PSF
@pytest.mark.parametrize("radii, padding, size", xc.psf_exact_cases(),
                         ids=lambda v: v if isinstance(v, str) else f"{v[0]}x{v[1]}")
def test_psf_equals_the_fp64_oracle_on_exact_data(radii, padding, size, monkeypatch):
    r"""Forward and adjoint for every (B, C) and every PSF shape form.  The reference is computed once, for every (PSF number,
    image) pair that some form meets on some (B, C)."""
    from azula_amd.guidance import PSFOperator

    (rh, rw), (H, W) = radii, size
    kh, kw = 2 * rh + 1, 2 * rw + 1
    assert _ops().psf_tile(kh, kw) == xc.PSF_TILE
    circ = padding == "circular"
    psfs = xc.exact_psfs(kh, kw)
    pairs = xc.psf_pairs()
    at = {pq: n for n, pq in enumerate(pairs)}
    kr = psfs[[p for p, _ in pairs]].reshape(len(pairs), 1, kh, kw)
    ref_fn = lambda z: xo.psf(z, kr, circ)  # noqa: E731
    x6, w6 = oc.exact_image(xc.PSF_COUNT, 1, H, W, seed=H), oc.exact_image(xc.PSF_COUNT, 1, H, W, seed=W + 100)
    q = [q for _, q in pairs]
    ref = ref_fn(x6[q].double())
    ref_t = oo.adjoint(ref_fn, x6[q].shape, w6[q].double())
    names = _spy(monkeypatch)
    for B, C in xc.PSF_BC:
        x, w = x6[:B * C].reshape(B, C, H, W).cuda(), w6[:B * C].reshape(B, C, H, W).cuda()
        for f in xc.PSF_FORMS:
            A = PSFOperator(xc.psf_argument(psfs, f, B, C), padding=padding)
            rows = [at[(xc.psf_number(f, b, c, C), b * C + c)] for b in range(B) for c in range(C)]
            y, g = A(x), A.adjoint(w)
            assert y.dtype == torch.float32 and y.shape == x.shape and g.shape == x.shape
            assert torch.equal(y.cpu().double(), ref[rows].reshape(B, C, H, W)), (B, C, f)
            assert torch.equal(g.cpu().double(), ref_t[rows].reshape(B, C, H, W)), (B, C, f)
    assert torch.equal(A(x), y)  # two runs, the same bits
    assert names == ["az_op_psf_f32"] * (2 * len(xc.PSF_BC) * len(xc.PSF_FORMS) + 1)


@pytest.mark.parametrize("planes", [xc.PSF_GRID_PLANES, xc.PSF_MANY_PLANES], ids=["grid_stride", "planes70000"])
def test_psf_walks_more_tiles_than_its_grid_and_many_planes(planes):
    r"""2^16 + 3 planes of 1 x 1 pixels -- more tiles than the launch's 2^16 workgroups -- and 70 000 planes of 2 x 2, far more than
    grid.y holds, each with its own 3 x 3 PSF (number: plane mod 6), as samples and as channels."""
    from azula_amd.guidance import PSFOperator

    size = 1 if planes == xc.PSF_GRID_PLANES else 2
    k = xc.exact_psfs(3, 3).repeat(planes // xc.PSF_COUNT + 1, 1, 1)[:planes]
    x = oc.exact_image(planes, 1, size, size)
    want = xo.psf(x.double(), k[:, None], False)
    assert torch.equal(PSFOperator(k[:, None])(x.cuda()).cpu().double(), want)
    assert torch.equal(PSFOperator(k)(x.reshape(1, planes, size, size).cuda()).cpu().double(), want.reshape(1, planes, size, size))
    assert torch.equal(PSFOperator(k[0])(x.cuda()).cpu().double(), xo.psf(x.double(), k[0], False))


# ------------------------------------------------------------------------------------------------------ exact: decimation
@pytest.mark.parametrize("factor", xc.DEC_FACTORS, ids=lambda f: f"f{f[0]}x{f[1]}")
def test_decimation_is_the_strided_slice(factor, monkeypatch):
    from azula_amd.guidance import DecimateOperator

    fh, fw = factor
    names = _spy(monkeypatch)
    ran = 0
    for oh, ow in xc.offsets(fh, fw):
        A = DecimateOperator(factor, (oh, ow))
        for Ho, Wo in xc.DEC_OUTPUTS:
            for image in (oc.exact_image, oc.random_image):
                x, w = image(2, 3, Ho * fh, Wo * fw, seed=Ho), image(2, 3, Ho, Wo, seed=Wo + 50)
                y, g, up = A(x.cuda()), A.adjoint(w.cuda()), A.pinv(w.cuda())
                assert y.shape == (2, 3, Ho, Wo) and g.shape == x.shape
                assert torch.equal(y.cpu(), xo.decimate(x, fh, fw, oh, ow)), (oh, ow, Ho, Wo)
                assert torch.equal(g.cpu(), xo.zero_stuff(w, fh, fw, oh, ow)) and torch.equal(up, g), (oh, ow, Ho, Wo)
                ran += 1
        assert torch.equal(g.cpu().double(), oo.adjoint(lambda z: xo.decimate(z, fh, fw, oh, ow), x.shape, w.double()))  # noqa: B023
    assert names == ["az_op_decimate_f32", "az_op_decimate_adj_f32", "az_op_decimate_adj_f32"] * ran


def test_decimation_of_many_planes_and_many_pixels():
    from azula_amd.guidance import DecimateOperator

    A = DecimateOperator(2, (1, 0))
    for shape in ((70_000, 1, 2, 2), (1, 3, 1024, 1024)):  # no plane count on grid.y / grid.z; more outputs than one pass of the grid
        x = oc.exact_image(*shape)
        w = oc.exact_image(shape[0], shape[1], shape[2] // 2, shape[3] // 2, seed=1)
        assert torch.equal(A(x.cuda()).cpu(), xo.decimate(x, 2, 2, 1, 0))
        assert torch.equal(A.adjoint(w.cuda()).cpu(), xo.zero_stuff(w, 2, 2, 1, 0))


# ----------------------------------------------------------------------------------------------------- exact: channel mix
@pytest.mark.parametrize("channels", xc.MIX_CHANNELS, ids=lambda c: f"c{c[0]}to{c[1]}")
def test_channel_mix_equals_the_fp64_oracle_on_exact_data(channels, monkeypatch):
    from azula_amd.guidance import ChannelMixOperator

    Cin, Cout = channels
    M = xc.exact_matrix(Cout, Cin, Cin)
    A = ChannelMixOperator(M)
    ref_fn = lambda z: xo.mix(z, M)  # noqa: E731
    names = _spy(monkeypatch)
    for H, W in xc.MIX_HW:
        x, w = oc.exact_image(3, Cin, H, W, seed=W), oc.exact_image(3, Cout, H, W, seed=W + 7)
        y, g = A(x.cuda()), A.adjoint(w.cuda())
        assert y.shape == (3, Cout, H, W) and g.shape == x.shape
        assert torch.equal(y.cpu().double(), ref_fn(x.double())), (H, W)
        assert torch.equal(g.cpu().double(), oo.adjoint(ref_fn, x.shape, w.double())), (H, W)
        assert torch.equal(A(x.cuda()), y)
    assert names == ["az_op_chanmix_f32"] * (3 * len(xc.MIX_HW))


@pytest.mark.parametrize("k", range(len(xc.MIX_PINV)))
def test_channel_mix_pseudo_inverse_on_exact_data(k, monkeypatch):
    r"""Matrices whose pseudo-inverse is dyadic (``test_operators_ext_host.py`` checks that on the CPU)."""
    from azula_amd.guidance import ChannelMixOperator

    M, P = torch.tensor(xc.MIX_PINV[k], dtype=torch.float64), torch.tensor(xc.MIX_PINV_BY_HAND[k], dtype=torch.float64)
    A = ChannelMixOperator(M)
    names = _spy(monkeypatch)
    for H, W in xc.MIX_HW:
        y = oc.exact_image(2, M.shape[0], H, W, seed=W)
        z = A.pinv(y.cuda())
        assert z.shape == (2, M.shape[1], H, W) and torch.equal(z.cpu().double(), xo.mix(y.double(), P)), (H, W)
        assert torch.equal(A(A.pinv(A(z))), A(z))  # A A^+ A = A
    assert set(names) == {"az_op_chanmix_f32"}


# ------------------------------------------------------------------------------------------------- random data against fp64
@pytest.mark.parametrize("padding", oc.PADDINGS)
def test_psf_on_random_data_is_within_the_derived_bound(padding):
    from azula_amd.guidance import PSFOperator

    worst = 0.0
    for n, (rh, rw) in enumerate(xc.PSF_RADII):
        kh, kw = 2 * rh + 1, 2 * rw + 1
        th, tw = _ops().psf_tile(kh, kw)
        H, W = 2 * th + 3, tw + 5
        k = xc.random_psf(2, 1, kh, kw, seed=n)  # one PSF per sample
        x = oc.random_image(2, 2, H, W, seed=n) * 3
        y = PSFOperator(k, padding=padding)(x.cuda())
        ref = xo.psf(x.double(), k, padding == "circular")
        err = float((y.cpu().double() - ref).abs().max())
        bound = (kh * kw + 2) * U * float(k.abs().sum(dim=(2, 3)).max()) * float(x.abs().max())
        print(f"psf {padding} {kh} x {kw} on {H} x {W}: max|d| {err:.3e} bound {bound:.3e} ratio {err / bound:.3f}")
        worst = max(worst, err / bound)
        assert err <= bound
    print(f"psf {padding}: worst ratio {worst:.3f}")


def test_channel_mix_on_random_data_is_within_the_derived_bound():
    from azula_amd.guidance import ChannelMixOperator

    for n, (Cin, Cout) in enumerate(xc.MIX_CHANNELS):
        M = xc.random_matrix(Cout, Cin, n)
        for H, W in xc.MIX_HW[-2:]:
            x = oc.random_image(2, Cin, H, W, seed=n) * 3
            y = ChannelMixOperator(M)(x.cuda())
            err = float((y.cpu().double() - xo.mix(x.double(), M.double())).abs().max())
            bound = (Cin + 2) * U * float(M.abs().sum(1).max()) * float(x.abs().max())
            print(f"mix {Cin} -> {Cout} on {H} x {W}: max|d| {err:.3e} bound {bound:.3e} ratio {err / bound:.3f}")
            assert err <= bound


# -------------------------------------------------------------------------------------------------------------- adjointness
def _device_operators(C, H, W, flatten=False):
    r"""(name, operator, oracle, launched entries) on exact data for a (2, C, H, W) input."""
    from azula_amd.guidance import BlurOperator, ChannelMixOperator, DecimateOperator, PSFOperator, bicubic_taps

    k1, k6 = xc.exact_psf(7, 3), xc.exact_psfs(3, 5)[:2 * C].reshape(2, C, 3, 5)
    M = xc.exact_matrix(2, C, 4)
    taps = bicubic_taps(2)  # (dyadic: 1 / 32 of 0, -1, 0, 9, 16, 9, 0, -1, 0)
    out = []
    for pad in oc.PADDINGS:
        out.append((f"psf_{pad}", PSFOperator(k1, padding=pad, flatten=flatten), lambda z, pad=pad: xo.psf(z, k1, pad == "circular"),
                    NEW["psf"]))
    out.append(("psf_per_plane", PSFOperator(k6, padding="circular", flatten=flatten), lambda z: xo.psf(z, k6, True), NEW["psf"]))
    out.append(("decimate", DecimateOperator((2, 4), (1, 3), flatten=flatten), lambda z: xo.decimate(z, 2, 4, 1, 3), NEW["decimate"]))
    out.append(("mix", ChannelMixOperator(M, flatten=flatten), lambda z: xo.mix(z, M), NEW["mix"]))
    out.append(("bicubic", DecimateOperator(2, 1, flatten=flatten) @ BlurOperator(taps),
                lambda z: xo.decimate(oo.blur(z, taps, taps, False), 2, 2, 1, 1), NEW["decimate"] | NEW["blur"]))
    out.append(("mix_of_psf", ChannelMixOperator(M, flatten=flatten) @ PSFOperator(k1),
                lambda z: xo.mix(xo.psf(z, k1, False), M), NEW["mix"] | NEW["psf"]))
    return out


def test_adjointness_with_fp64_dot_products():
    r"""<A x, w> == <x, A^T w> exactly: on the exact data both sides are sums of integers (in units of the common denominator)
    far below 2^53."""
    B, C, H, W = 2, 3, 36, 68
    x = oc.exact_image(B, C, H, W, seed=1)
    for name, A, ref, _ in _device_operators(C, H, W):
        Ax = A(x.cuda())
        assert torch.equal(Ax.cpu().double(), ref(x.double())), name
        w = oc.exact_image(*Ax.shape, seed=2)
        Atw = A.adjoint(w.cuda())
        lhs, rhs = (Ax.cpu().double() * w.double()).sum(), (x.double() * Atw.cpu().double()).sum()
        print(f"{name}: <Ax, w> {float(lhs)} <x, A^T w> {float(rhs)}")
        assert Atw.shape == x.shape and float(lhs) == float(rhs) and float(lhs) != 0


# ----------------------------------------------------------------------------------------------------- autograd on the device
@pytest.mark.parametrize("flatten", [False, True])
def test_autograd_and_functorch_reach_the_same_launches(flatten, monkeypatch):
    B, C, H, W = 2, 3, 36, 68
    x, v = oc.random_image(B, C, H, W, seed=1).cuda(), oc.random_image(B, C, H, W, seed=2).cuda()
    names = _spy(monkeypatch)
    for name, A, ref, entries in _device_operators(C, H, W, flatten):
        y = A(x)
        want_shape = ref(x.cpu()).shape
        assert y.shape == ((B, want_shape[1:].numel()) if flatten else want_shape), name
        w = oc.random_image(*y.shape, seed=3).cuda()
        Atw, Av = A.adjoint(w), A(v)
        assert torch.equal(A(x), y) and torch.equal(A.adjoint(w), Atw), name  # two runs, the same bits
        names.clear()
        with torch.no_grad():
            with torch.enable_grad():
                x_hat = x.clone().requires_grad_()
                y_hat = A(x_hat)
            for _ in range(2):
                assert torch.equal(torch.autograd.grad(y_hat, x_hat, w, retain_graph=True)[0], Atw), name
            assert torch.equal(torch.func.jvp(A, (x_hat.detach(),), (v,))[1], Av), name
        out, pull = torch.func.vjp(A, x)
        assert torch.equal(out, y) and torch.equal(pull(w)[0], Atw), name
        assert torch.equal(torch.func.jvp(A, (x,), (v,))[0], y), name
        assert set(names) == entries, (name, set(names))


def test_shape_errors_on_the_device_and_other_dtypes(monkeypatch):
    from azula_amd.guidance import ChannelMixOperator, DecimateOperator, PSFOperator

    x = torch.zeros(2, 3, 6, 6, device="cuda")
    with pytest.raises(ValueError, match="circular"):
        PSFOperator(torch.ones(13, 3), padding="circular")(x)
    with pytest.raises(ValueError, match="batch"):
        PSFOperator(torch.ones(3, 1, 3, 3))(x)
    with pytest.raises(ValueError, match="multiples"):
        DecimateOperator(4)(x)
    with pytest.raises(ValueError, match="channels"):
        ChannelMixOperator(torch.ones(1, 2))(x)
    # fp64 and half device tensors, and a non-contiguous fp32 one: the torch path, in the tensor's dtype (exact in all three)
    names = _spy(monkeypatch)
    k, M = xc.exact_psf(3, 3), torch.tensor([[1.0, 0, 0], [0, 1, 1]])
    xe = oc.exact_image(1, 3, 6, 6).cuda()
    for z in (xe.double(), xe.half(), xe.transpose(2, 3)):
        for A, ref in ((PSFOperator(k), lambda t: xo.psf(t, k, False)), (DecimateOperator(2, 1), lambda t: xo.decimate(t, 2, 2, 1, 1)),
                       (ChannelMixOperator(M), lambda t: xo.mix(t, M))):
            y = A(z)
            assert y.dtype == z.dtype and torch.equal(y.double().cpu(), ref(z.double().cpu()))
    assert not names


# ------------------------------------------------------------------------------------- end to end: DiffPIR on the fixture
def _restoration(task):
    r"""(operator, the oracle's A, launched entries) of an end-to-end case on a (B, 3, 16, 16) input."""
    from azula_amd.guidance import BlurOperator, DecimateOperator, PSFOperator, bicubic_taps, motion_psf

    if task == "motion_deblur":
        k = motion_psf(9, 30.0, 9)
        return PSFOperator(k, flatten=True), (lambda z: xo.psf(z, k, False).flatten(1)), NEW["psf"]
    taps = bicubic_taps(2)
    return (DecimateOperator(2, 1, flatten=True) @ BlurOperator(taps),
            lambda z: xo.decimate(oo.blur(z, taps, taps, False), 2, 2, 1, 1).flatten(1), NEW["decimate"] | NEW["blur"])


@pytest.mark.parametrize("task", ["motion_deblur", "bicubic_sr"])
def test_diffpir_restoration(golden, task, monkeypatch):
    r"""DiffPIR (cg, 3 iterations) on the fixture's UNet, as ``test_diffpir_with_a_blurred_downsampled_observation``: the inner
    mean x^ is the same bits in every run, so the fp64 reference is the restatement on the host from that x^ with the oracle's A.
    e_op: our operators against it; e_lambda: the same call with the oracle's A as fp32 torch ops on the device.  Required:
    e_op <= 4 max(e_lambda, 2^-23 max|ref|) -- 4: the project's margin for another accumulation order; the floor: one ulp of
    the result.

    The solver takes its inner products along the last dimension, here a row of the image.  With the motion PSF, which couples
    rows, the third iteration meets a row with <p, q> < 0 (-7e-3 in the fp64 reference); the step's denominator is floored at
    eps and the result grows to 5.5e13 -- in the reference, with the oracle's A and with the operator alike (measured: e_op
    1.00e8, e_lambda 1.12e8, 1.8e-6 and 2.0e-6 of max|ref|).  The rule is relative to the result and holds there; the same
    rule is also required at 2 iterations, where no step is floored and the result is O(1) (measured: e_op 2.25e-6, e_lambda
    2.77e-6 on max|ref| 6.1)."""
    from test_gpu_guidance_vjp import device_denoiser

    from azula_amd.guidance import DiffPIRDenoiser

    g = golden("g28_guidance_vjp")
    _, _, _, sd, cfg = gc.setup(g)
    den = device_denoiser(sd, cfg)
    x_t, t, var_y = g["x_t"].cuda(), g["t"].cuda(), g.meta["var_y"]
    A, A_oracle, entries = _restoration(task)
    gen = torch.Generator().manual_seed(11)
    clean = A_oracle(torch.rand(x_t.shape, generator=gen) - 0.5)
    y = clean + var_y**0.5 * 0.1 * torch.randn(clean.shape, generator=gen)
    with torch.no_grad():
        x_hat = den(x_t, t).mean
        assert torch.equal(x_hat, den(x_t, t).mean)
    alpha_t, sigma_t = (v.double().cpu() for v in den.schedule(t))
    names = _spy(monkeypatch)
    for iterations in (3, 2):
        ref = do.diffpir_mean(x_hat.double().cpu(), alpha_t, sigma_t, y.double(), A_oracle, var_y, 10.0, "cg", iterations).detach()
        names.clear()
        out_op = DiffPIRDenoiser(den, y.cuda(), A, var_y, solver="cg", iterations=iterations)(x_t, t).mean
        assert set(names) == entries
        out_lambda = DiffPIRDenoiser(den, y.cuda(), A_oracle, var_y, solver="cg", iterations=iterations)(x_t, t).mean
        e_op = float((out_op.double().cpu() - ref).abs().max())
        e_lambda = float((out_lambda.double().cpu() - ref).abs().max())
        floor = 2.0**-23 * float(ref.abs().max())
        print(f"DiffPIR {task}, {iterations} iterations: e_op {e_op:.3e} e_lambda {e_lambda:.3e} floor {floor:.3e} "
              f"max|ref| {float(ref.abs().max()):.3e}")
        assert e_op <= 4 * max(e_lambda, floor)


def test_dps_colourisation_step(golden, monkeypatch):
    r"""One DPS step with ``ChannelMixOperator.grayscale(flatten=True)`` on the fixture's denoiser against the fp64 restatement with
    the device's noise copied over, at ``test_gpu_guidance_vjp``'s bound max(4 e_ref, 1e-4); e_ref: what the restatement itself
    loses in fp32 against fp64 on this case, measured here on the CPU."""
    from test_gpu_guidance_vjp import SEED, device_denoiser

    from azula_amd.guidance import ChannelMixOperator, DPSSampler

    g = golden("g28_guidance_vjp")
    mean64, _, arr64, sd, cfg = gc.setup(g, torch.float64)
    mean32, _, arr32, _, _ = gc.setup(g)
    den = device_denoiser(sd, cfg)
    M = torch.full((1, 3), 1 / 3, dtype=torch.float64)
    A_oracle = lambda z: xo.mix(z, M).flatten(1)  # noqa: E731
    gen = torch.Generator().manual_seed(12)
    clean = A_oracle(torch.rand(g["x_t"].shape, generator=gen) - 0.5)
    y = clean + g.meta["var_y"] ** 0.5 * torch.randn(clean.shape, generator=gen)
    x_t, t, s = g["x_t"].cuda(), g["t"].cuda(), g["s"].cuda()
    torch.manual_seed(SEED)
    eps = torch.randn_like(x_t).cpu()
    torch.manual_seed(SEED)
    names = _spy(monkeypatch)
    out = DPSSampler(den, y.cuda(), ChannelMixOperator.grayscale(flatten=True), steps=g.meta["steps"], silent=True).step(x_t, t, s)
    assert set(names) == NEW["mix"]
    ref = go.dps_step(mean64, arr64["x_t"], arr64["t"], arr64["s"], eps.double(), y=y.double(), A=A_oracle)
    ref32 = go.dps_step(mean32, arr32["x_t"], arr32["t"], arr32["s"], eps, y=y, A=A_oracle)
    assert out.shape == ref.shape and torch.isfinite(out).all()
    scale = float(ref.abs().max())
    err, e_ref = float((out.double().cpu() - ref).abs().max()) / scale, float((ref32.double() - ref).abs().max()) / scale
    print(f"dps colourisation: err {err:.3e} e_ref {e_ref:.3e} bound {max(4 * e_ref, 1e-4):.3e}")
    assert err < max(4 * e_ref, 1e-4)
