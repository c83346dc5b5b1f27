r"""``azula_amd.guidance.operators`` on the GPU: the kernels of ``csrc/operators.hip`` against the torch-op restatement of
``tests/operator_oracle.py`` run on the host in fp64.

* exact data (``tests/operator_cases.py``: small integers, dyadic taps): ``torch.equal`` with the fp64 oracle, at the edges of the
  blur's tile, for odd sizes, several planes, both paddings, more planes than a grid dimension holds and more work items than
  one pass of the grid;
* random data: within bounds derived from the number of fp32 operations per output,
      blur     (nh + nw + 2) * 2^-24 * sum|taps_h| * sum|taps_w| * max|x|     (nh + nw fused multiply-adds and the inputs' scale)
      pooling  (fh * fw + 2) * 2^-24 * max|x|                                  (fh * fw - 1 additions, 1 / (fh fw), the product)
* adjointness on the exact data with fp64 dot products, the autograd Function (bit for bit: the same launches), and the
  guidance classes end to end: every case of the ``g28_guidance_vjp`` fixture with the mask and pooling operators in place of
  the lambdas, and DiffPIR with a blurred, downsampled observation.
"""

import pytest
import torch

import diffpir_oracle as do
import guidance_vjp_cases as gc
import operator_cases as oc
import operator_oracle as oo
from test_guidance_vjp_host import CASES

pytestmark = pytest.mark.gpu
U = 2.0**-24


def _ops():
    from azula_amd.guidance import operators

    return operators


def _spy(monkeypatch):
    ops = _ops()
    names, launch = [], ops._launch
    monkeypatch.setattr(ops, "_launch", lambda name, *a: (names.append(name), launch(name, *a))[1])
    return names


def _planes(t, planes):
    r"""The first ``planes`` planes of a (5, 1, H, W) tensor as a (B, C, H, W) tensor."""
    B, C = oc.split_planes(planes)
    return t[:planes].reshape(B, C, *t.shape[2:])


# ------------------------------------------------------------------------------------------------------------ exact: blur
@pytest.mark.parametrize("padding", oc.PADDINGS)
@pytest.mark.parametrize("radii", oc.BLUR_RADII, ids=lambda r: f"r{r[0]}x{r[1]}")
def test_blur_equals_the_fp64_oracle_on_exact_data(radii, padding, monkeypatch):
    from azula_amd.guidance import BlurOperator

    rh, rw = radii
    nh, nw = 2 * rh + 1, 2 * rw + 1
    taps_h, taps_w = oc.exact_taps(nh), oc.exact_taps(nw, 2)  # (two different vectors also where nh == nw)
    A = BlurOperator(taps_h, taps_w, padding=padding)
    circ = padding == "circular"
    ref_fn = lambda z: oo.blur(z, taps_h, taps_w, circ)  # noqa: E731
    names = _spy(monkeypatch)
    ran = 0
    for H, W in oc.blur_sizes(*_ops().blur_tile(nh, nw)):
        if circ and (rh >= H or rw >= W):
            continue  # (not defined: the operator refuses it, test_shape_errors_on_the_device)
        x5, w5 = oc.exact_image(5, 1, H, W, seed=H), oc.exact_image(5, 1, H, W, seed=W + 100)
        ref = ref_fn(x5.double())  # once for the five planes: planes are independent
        ref_t = oo.adjoint(ref_fn, x5.shape, w5.double())
        for planes in oc.BLUR_PLANES:
            x, w = _planes(x5, planes).cuda(), _planes(w5, planes).cuda()
            y, g = A(x), A.adjoint(w)
            assert y.dtype == torch.float32 and y.shape == x.shape
            assert torch.equal(y.cpu().double(), _planes(ref, planes)), (H, W, planes)
            assert torch.equal(g.cpu().double(), _planes(ref_t, planes)), (H, W, planes)
            ran += 1
    assert ran and names == ["az_op_blur_f32"] * (2 * ran)


def test_blur_walks_more_tiles_than_its_grid():
    r"""2^20 + 3 planes of 1 x 1 pixels: more tiles than the launch's 2^20 workgroups, and far more planes than grid.y holds."""
    from azula_amd.guidance import BlurOperator

    taps_h, taps_w = oc.exact_taps(3), oc.exact_taps(3, 2)
    x = oc.exact_image((1 << 20) + 3, 1, 1, 1)
    y = BlurOperator(taps_h, taps_w)(x.cuda())
    assert torch.equal(y.cpu().double(), oo.blur(x.double(), taps_h, taps_w, False))


# --------------------------------------------------------------------------------------------------------- exact: pooling
@pytest.mark.parametrize("factor", oc.POOL_FACTORS, ids=lambda f: f"f{f[0]}x{f[1]}")
def test_pooling_equals_the_fp64_oracle_on_exact_data(factor, monkeypatch):
    from azula_amd.guidance import DownsampleOperator

    fh, fw = factor
    A = DownsampleOperator(factor)
    ref_fn = lambda z: oo.pool(z, fh, fw)  # noqa: E731
    names = _spy(monkeypatch)
    for Ho, Wo in oc.POOL_OUTPUTS:
        x, w = oc.exact_image(2, 3, Ho * fh, Wo * fw, seed=Ho), oc.exact_image(2, 3, Ho, Wo, seed=Wo + 50)
        y, g, up = A(x.cuda()), A.adjoint(w.cuda()), A.pinv(w.cuda())
        assert y.shape == (2, 3, Ho, Wo) and g.shape == x.shape and up.shape == x.shape
        assert torch.equal(y.cpu().double(), ref_fn(x.double())), (Ho, Wo)
        assert torch.equal(g.cpu().double(), oo.adjoint(ref_fn, x.shape, w.double())), (Ho, Wo)
        assert torch.equal(up.cpu().double(), oo.unpool(w.double(), fh, fw)), (Ho, Wo)
    assert names == ["az_op_avgpool_f32", "az_op_avgpool_adj_f32", "az_op_avgpool_adj_f32"] * len(oc.POOL_OUTPUTS)


@pytest.mark.parametrize("shape", [(oc.POOL_MANY_PLANES, 1, 2, 2), (1, 3, 1024, 1024)], ids=["planes70000", "grid_stride"])
def test_pooling_of_many_planes_and_many_pixels(shape):
    r"""70 000 planes (no plane count on grid.y / grid.z) and more outputs than one pass of the capped grid."""
    from azula_amd.guidance import DownsampleOperator

    A = DownsampleOperator(2)
    x = oc.exact_image(*shape)
    w = oc.exact_image(shape[0], shape[1], shape[2] // 2, shape[3] // 2, seed=1)
    assert torch.equal(A(x.cuda()).cpu().double(), oo.pool(x.double(), 2, 2))
    assert torch.equal(A.pinv(w.cuda()).cpu().double(), oo.unpool(w.double(), 2, 2))
    assert torch.equal(A.adjoint(w.cuda()).cpu().double(), oo.unpool(w.double(), 2, 2) * 0.25)


# ------------------------------------------------------------------------------------------------------------ exact: mask
def _mask_values(shape, seed, boolean):
    gen = torch.Generator().manual_seed(seed)
    keep = torch.rand(shape, generator=gen) < 0.6
    return keep if boolean else keep * torch.randint(1, 6, shape, generator=gen).float()


@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (2, 3, 4, 8), (1, 3, 1024, 1024)], ids=["n210", "n192", "grid_stride"])
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset_view"])
def test_mask_equals_the_device_product(shape, offset, monkeypatch):
    r"""n % 4 != 0 with mask sizes that are no multiple of 4 (gathered factors, scalar tail), n % 4 == 0 (float4 factors), a view
    that starts one float into its buffer, and every broadcast form of the mask, bool and float."""
    from azula_amd.guidance import MaskOperator

    B, C, H, W = shape
    n = B * C * H * W
    buf = torch.randn(n + offset, generator=torch.Generator().manual_seed(n)).cuda()
    x = buf[offset:].view(shape)
    assert x.is_contiguous() and x.data_ptr() % 16 == 4 * offset
    names = _spy(monkeypatch)
    for k, mshape in enumerate([(1, 1, H, W), (1, C, H, W), (B, 1, H, W), shape, (H, W), (W,)]):
        for boolean in (False, True):
            m = _mask_values(mshape, k, boolean)
            A = MaskOperator(m)
            md = m.cuda()
            want = x * md
            assert torch.equal(A(x), want) and torch.equal(A.adjoint(x), want) and torch.equal(A.T(x), want), (mshape, boolean)
            inv = torch.where(md != 0, 1 / md.float(), torch.zeros_like(md, dtype=torch.float32))
            assert torch.equal(A.pinv(x), x * inv), (mshape, boolean)
            if boolean:  # (a projector: m (1 / m) m x == m x bit for bit)
                assert torch.equal(A(A.pinv(A(x))), want)
    assert names and set(names) == {"az_op_mul_f32"}


# ------------------------------------------------------------------------------------------------- random data against fp64
@pytest.mark.parametrize("padding", oc.PADDINGS)
def test_blur_on_random_data_is_within_the_derived_bound(padding):
    from azula_amd.guidance import BlurOperator

    worst = 0.0
    for k, (rh, rw) in enumerate(oc.BLUR_RADII):
        nh, nw = 2 * rh + 1, 2 * rw + 1
        th, tw = _ops().blur_tile(nh, nw)
        H, W = 2 * th + 3, tw + 5
        taps_h, taps_w = oc.random_taps(nh, k), oc.random_taps(nw, k + 10)
        x = oc.random_image(1, 3, H, W, seed=k) * 3
        y = BlurOperator(taps_h, taps_w, padding=padding)(x.cuda())
        ref = oo.blur(x.double(), taps_h, taps_w, padding == "circular")
        err = float((y.cpu().double() - ref).abs().max())
        bound = (nh + nw + 2) * U * float(taps_h.abs().sum()) * float(taps_w.abs().sum()) * float(x.abs().max())
        print(f"blur {padding} taps {nh} x {nw} on {H} x {W}: max|d| {err:.3e} bound {bound:.3e} ratio {err / bound:.3f}")
        worst = max(worst, err / bound)
        assert err <= bound
    print(f"blur {padding}: worst ratio {worst:.3f}")


def test_pooling_on_random_data_is_within_the_derived_bound():
    from azula_amd.guidance import DownsampleOperator

    for k, (fh, fw) in enumerate(oc.POOL_FACTORS_RANDOM):
        for Ho, Wo in oc.POOL_OUTPUTS[-2:]:
            x = oc.random_image(2, 3, Ho * fh, Wo * fw, seed=k) * 3
            y = DownsampleOperator((fh, fw))(x.cuda())
            err = float((y.cpu().double() - oo.pool(x.double(), fh, fw)).abs().max())
            bound = (fh * fw + 2) * U * float(x.abs().max())
            print(f"pool {fh} x {fw} to {Ho} x {Wo}: max|d| {err:.3e} bound {bound:.3e} ratio {err / bound:.3f}")
            assert err <= bound


# -------------------------------------------------------------------------------------------------------------- adjointness
def _device_operators(C, H, W, flatten=False):
    r"""(name, operator, oracle) on exact data for a (C, H, W) input; the composition downsample o blur last."""
    from azula_amd.guidance import BlurOperator, DownsampleOperator, MaskOperator

    m = _mask_values((1, C, H, W), 3, False)
    th, tw = oc.exact_taps(7), oc.exact_taps(3, 2)
    out = [("mask", MaskOperator(m, flatten=flatten), lambda z: oo.mask(z, m)),
           ("pool", DownsampleOperator((2, 4), flatten=flatten), lambda z: oo.pool(z, 2, 4))]
    for pad in oc.PADDINGS:
        out.append((f"blur_{pad}", BlurOperator(th, tw, padding=pad, flatten=flatten),
                    lambda z, pad=pad: oo.blur(z, th, tw, pad == "circular")))
    out.append(("pool_of_blur", DownsampleOperator(2, flatten=flatten) @ BlurOperator(th, tw),
                lambda z: oo.pool(oo.blur(z, th, tw, False), 2, 2)))
    return out


def test_adjointness_with_fp64_dot_products():
    r"""<A x, w> == <x, A^T w> exactly: on the exact data both sides are sums of integers (in units of the common denominator)
    far below 2^53."""
    B, C, H, W = 2, 3, 36, 68
    x = oc.exact_image(B, C, H, W, seed=1)
    for name, A, _ in _device_operators(C, H, W):
        Ax = A(x.cuda())
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
    for name, A, ref in _device_operators(C, H, W, flatten):
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
        assert names and all(n.startswith("az_op_") for n in names), name


def test_shape_errors_on_the_device_and_other_dtypes(monkeypatch):
    from azula_amd.guidance import BlurOperator, DownsampleOperator

    x = torch.zeros(1, 2, 6, 6, device="cuda")
    with pytest.raises(ValueError, match="circular"):
        BlurOperator(torch.ones(13), padding="circular")(x)
    with pytest.raises(ValueError, match="multiples"):
        DownsampleOperator(4)(x)
    # fp64 and half device tensors, and a non-contiguous fp32 one: the torch path, in the tensor's dtype (exact in all three)
    names = _spy(monkeypatch)
    taps = oc.exact_taps(3)
    xe = oc.exact_image(1, 2, 6, 6).cuda()
    for z in (xe.double(), xe.half(), xe.transpose(2, 3)):
        for A, ref in ((BlurOperator(taps), lambda t: oo.blur(t, taps, taps, False)), (DownsampleOperator(2), lambda t: oo.pool(t, 2, 2))):
            y = A(z)
            assert y.dtype == z.dtype and torch.equal(y.double().cpu(), ref(z.double().cpu()))
    assert not names


# --------------------------------------------------------------------------------------- end to end: the committed fixture
@pytest.mark.parametrize("tag", CASES)
def test_guidance_fixture_with_the_operators(golden, tag, monkeypatch):
    r"""``test_gpu_guidance_vjp``'s cases with ``MaskOperator`` / ``DownsampleOperator`` (flattened observations, as the fixture
    has them) in place of the lambdas, against the restatement in fp64; that test's own bound."""
    from test_gpu_guidance_vjp import device_denoiser, run_device

    from azula_amd.guidance import DownsampleOperator, MaskOperator

    g = golden("g28_guidance_vjp")
    mean64, ops64, arr64, sd, cfg = gc.setup(g, torch.float64)
    den = device_denoiser(sd, cfg)
    in_shape = tuple(g["x_t"].shape[1:])
    M, D = MaskOperator(g["mask"], flatten=True, in_shape=in_shape), DownsampleOperator(2, flatten=True, in_shape=in_shape)
    names = _spy(monkeypatch)
    out, eps = run_device(tag, den, {"mask": (M, M.pinv), "pool": (D, D.pinv)}, g)
    assert names and set(names) <= {"az_op_mul_f32", "az_op_avgpool_f32", "az_op_avgpool_adj_f32"}
    ref = gc.run_case(tag, mean64, ops64, arr64, g.meta["steps"], g.meta["var_y"], eps=eps.double())
    assert out.shape == ref.shape and torch.isfinite(out).all()
    err = float((out.double().cpu() - ref).abs().max() / ref.abs().max())
    e_ref = g.meta["e_ref"][tag]
    print(f"{tag}: err {err:.3e} e_ref {e_ref:.3e} bound {max(4 * e_ref, 1e-4):.3e}")
    assert err < max(4 * e_ref, 1e-4)


# -------------------------------------------------------------------------------------------------- end to end: deblurring
def test_diffpir_with_a_blurred_downsampled_observation(golden, monkeypatch):
    r"""DiffPIR (cg, 3 iterations) on the fixture's UNet with A = downsample o Gaussian blur.  The inner mean x^ is the same
    bits in every run, so the fp64 reference is the restatement on the host from that x^ with the oracle's A.  e_op: our
    operators against it; e_lambda: the same call with the oracle's A as fp32 torch ops on the device.  Required:
    e_op <= 4 max(e_lambda, 2^-23 max|ref|) -- 4: the project's margin for another accumulation order (test_gpu_vdm.py); the
    floor: one ulp of the result."""
    from test_gpu_guidance_vjp import device_denoiser

    from azula_amd.guidance import BlurOperator, DiffPIRDenoiser, DownsampleOperator, gaussian_taps

    g = golden("g28_guidance_vjp")
    _, _, _, sd, cfg = gc.setup(g)
    den = device_denoiser(sd, cfg)
    x_t, t, var_y = g["x_t"].cuda(), g["t"].cuda(), g.meta["var_y"]
    taps = gaussian_taps(1.0, 5)
    A_oracle = lambda z: oo.pool(oo.blur(z, taps, taps, False), 2, 2).flatten(1)  # noqa: E731
    gen = torch.Generator().manual_seed(11)
    y = A_oracle(torch.rand(x_t.shape, generator=gen) - 0.5) + var_y**0.5 * 0.1 * torch.randn(x_t.shape[0], 192, generator=gen)
    with torch.no_grad():
        x_hat = den(x_t, t).mean
        assert torch.equal(x_hat, den(x_t, t).mean)
    alpha_t, sigma_t = (v.double().cpu() for v in den.schedule(t))
    ref = do.diffpir_mean(x_hat.double().cpu(), alpha_t, sigma_t, y.double(), A_oracle, var_y, 10.0, "cg", 3).detach()

    A = DownsampleOperator(2, flatten=True) @ BlurOperator.gaussian(1.0, 5)
    names = _spy(monkeypatch)
    out_op = DiffPIRDenoiser(den, y.cuda(), A, var_y, solver="cg", iterations=3)(x_t, t).mean
    assert {"az_op_blur_f32", "az_op_avgpool_f32", "az_op_avgpool_adj_f32"} == set(names)
    out_lambda = DiffPIRDenoiser(den, y.cuda(), A_oracle, var_y, solver="cg", iterations=3)(x_t, t).mean
    e_op = float((out_op.double().cpu() - ref).abs().max())
    e_lambda = float((out_lambda.double().cpu() - ref).abs().max())
    floor = 2.0**-23 * float(ref.abs().max())
    print(f"DiffPIR deblur: e_op {e_op:.3e} e_lambda {e_lambda:.3e} floor {floor:.3e}")
    assert e_op <= 4 * max(e_lambda, floor)
