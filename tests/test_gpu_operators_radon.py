r"""``az_op_radon_f32``, ``az_op_radon_adj_f32``, ``az_op_radon_filter_f32`` and ``RadonOperator`` on the GPU against the oracle of
``tests/radon_oracle.py``: fp64 arithmetic on the fp32 weights ``M32`` of the definition.

* exact: multiples of 90 degrees on integers, apply and adjoint EQUAL to the oracle (weights 0, 1/2, 1), also with more planes
  than the launch has workgroups;
* the accuracy rule, per output and DERIVED, not measured: ``|got - M32 x| <= (nnz + 2) * 2^-24 * (|M32| |x|)`` with ``nnz`` the
  nonzero weights of that output's row (apply) or column (adjoint) -- a chain of ``nnz`` fused multiply-adds rounds ``nnz`` times
  (candidates outside the support add an exact 0), and two roundings are to spare for the ``scale`` factor.  The same rule for the
  ramp filter with ``nnz`` the nonzero taps, and the two bounds composed for ``fbp``.  The rule holds the projector's window: the
  impulse data makes a single missed weight the whole result.  Measured ``err / bound``: DESIGN.md section 9e;
* the transpose identity ``|<A x, w> - <x, A^T w>| <= ||w|| ||b_apply|| + ||x|| ||b_adj||`` (the matrices are transposes exactly,
  so what is left is the two roundings; Cauchy-Schwarz, no new constant);
* determinism, planes, strides, the dtype paths and the autograd Function's launches;
* one DPS step, one MMPS mean and one DiffPIR call of sparse-view CT on the ``g28_guidance_vjp`` fixture's UNet.
"""

import pytest
import torch

import diffpir_oracle as do
import guidance_vjp_cases as gc
import guidance_vjp_oracle as go
import radon_cases as rc
import radon_oracle as ro

pytestmark = pytest.mark.gpu
F64 = torch.float64


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


def _operator(thetas, H, W, D=None, d=1.0, **kw):
    from azula_amd.guidance import RadonOperator

    return RadonOperator(thetas, (H, W), D, d, **kw)


def _ratio(got, ref, bound):
    r"""The worst err / bound; an output whose bound is 0 (no weight at all) must be exactly its reference, 0."""
    err = (got.double().cpu() - ref).abs()
    assert (err[bound == 0] == 0).all()
    return float((err / bound.clamp_min(1e-300)).max()), err


# ------------------------------------------------------------------------------------------------------------------ exact
@pytest.mark.parametrize("hwd", rc.EXACT_HWD, ids=lambda s: "x".join(map(str, s)))
def test_right_angles_equal_the_oracle_on_integers(hwd):
    H, W, D = hwd
    g, A = ro.geometry(rc.RIGHT_ANGLES, H, W, D), _operator(rc.RIGHT_ANGLES, H, W, D)
    for B, Cc in rc.EXACT_BC:
        x, v = rc.exact_planes(B, Cc, H, W, 1), rc.exact_planes(B, Cc, 4, D, 2)
        assert torch.equal(A(x.cuda()).double().cpu(), g.apply(x)), (B, Cc)
        assert torch.equal(A.adjoint(v.cuda()).double().cpu(), g.adjoint(v)), (B, Cc)


def test_more_planes_than_workgroups():
    H, W, D = 4, 4, 5
    g, A = ro.geometry(rc.RIGHT_ANGLES, H, W, D), _operator(rc.RIGHT_ANGLES, H, W, D)
    x, v = rc.exact_planes(rc.MANY_PLANES, 1, H, W, 3), rc.exact_planes(rc.MANY_PLANES, 1, 4, D, 4)
    assert torch.equal(A(x.cuda()).double().cpu(), g.apply(x))
    assert torch.equal(A.adjoint(v.cuda()).double().cpu(), g.adjoint(v))


# ------------------------------------------------------------------------------------------------------ the accuracy rule
def _rule_case(thetas, H, W, kind, d):
    r"""apply, adjoint, filter, fbp and the transpose identity of one operator; the three data kinds are the three channels."""
    D = rc.det_count(kind, H, W, d)
    g, A = ro.geometry(thetas, H, W, D, d), _operator(thetas, H, W, D, d)
    x = torch.stack([rc.planes(k, H, W) for k in rc.DATA])[None]
    v = torch.stack([rc.planes(k, g.A, D, seed=1) for k in rc.DATA])[None]
    xd, vd = x.cuda(), v.cuda()
    y, back, rec = A(xd), A.adjoint(vd), A.fbp(vd)
    filt = A._filter(vd, 1.0)
    b_apply, b_adj = g.bound_apply(x), g.bound_adjoint(v)
    r_apply, _ = _ratio(y, g.apply(x), b_apply)
    r_adj, _ = _ratio(back, g.adjoint(v), b_adj)
    r_filt, _ = _ratio(filt, g.filter(v), g.bound_filter(v))
    r_fbp, _ = _ratio(rec, g.fbp(v), g.bound_fbp(v))
    # <A x, w> = <x, A^T w> in fp64 dot products of the fp32 results
    norm = lambda t: float(t.double().pow(2).sum().sqrt())  # noqa: E731
    gap = abs(float((y.double().cpu() * v.double()).sum()) - float((x.double() * back.double().cpu()).sum()))
    b_gap = norm(v) * norm(b_apply) + norm(x) * norm(b_adj)
    print(f"radon {H}x{W} A {g.A} D {D} ({kind}) d {d}: err/bound apply {r_apply:.3f} adjoint {r_adj:.3f} filter {r_filt:.3f} "
          f"fbp {r_fbp:.3f} transpose {gap / b_gap if b_gap else 0.0:.3f}")
    assert max(r_apply, r_adj, r_filt, r_fbp) <= 1.0 and gap <= b_gap
    return max(r_apply, r_adj, r_filt, r_fbp)


@pytest.mark.parametrize("size", rc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_accuracy_rule(size):
    H, W = size
    worst = max(_rule_case(rc.ANGLES, H, W, kind, d) for kind in rc.DET_COUNTS for d in rc.SPACINGS)
    print(f"radon {H}x{W}: worst err / bound {worst:.3f}")


def test_accuracy_rule_128():
    (H, W), thetas = rc.BIG
    _rule_case(thetas, H, W, "default", 1.0)


# ------------------------------------------------------------------------------------ determinism, planes, strides, paths
def test_determinism_planes_and_strides(monkeypatch):
    H, W = 33, 47
    A = _operator(rc.ANGLES, H, W, None, 1.5)
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(3, 5, H, W, generator=gen).cuda()
    v = torch.randn(3, 5, A.angles, A.det_count, generator=gen).cuda()
    y, back, rec = A(x), A.adjoint(v), A.fbp(v)
    assert torch.equal(y, A(x)) and torch.equal(back, A.adjoint(v)) and torch.equal(rec, A.fbp(v))  # the same bits twice
    for b, c in ((0, 0), (1, 3), (2, 4)):  # a plane alone has the bits it has in the batch
        assert torch.equal(A(x[b:b + 1, c:c + 1].contiguous())[0, 0], y[b, c])
        assert torch.equal(A.adjoint(v[b:b + 1, c:c + 1].contiguous())[0, 0], back[b, c])
        assert torch.equal(A.fbp(v[b:b + 1, c:c + 1].contiguous())[0, 0], rec[b, c])
    names = _spy(monkeypatch)
    At = _operator(rc.ANGLES, W, H, A.det_count, 1.5)
    view = x.transpose(2, 3)  # (3, 5, W, H), not contiguous
    assert not view.is_contiguous() and torch.equal(At(view), At(view.contiguous())) and names == ["az_op_radon_f32"] * 2
    sview = v[:, ::2]
    assert not sview.is_contiguous() and torch.equal(A.adjoint(sview), back[:, ::2])


def test_dtype_paths(monkeypatch):
    H, W = 9, 12
    A, g = _operator(rc.EVEN, H, W), ro.geometry(rc.EVEN, H, W)
    names = _spy(monkeypatch)
    x = torch.randn(1, 2, H, W, dtype=F64, generator=torch.Generator().manual_seed(2))
    v = torch.randn(1, 2, g.A, g.D, dtype=F64, generator=torch.Generator().manual_seed(3))
    y, back, rec = A(x.cuda()), A.adjoint(v.cuda()), A.fbp(v.cuda())
    assert not names and y.dtype == F64 and y.is_cuda
    scale = float(g.apply(x).abs().max())
    assert float((y.cpu() - g.apply(x)).abs().max()) < 1e-12 * scale and float((back.cpu() - g.adjoint(v)).abs().max()) < 1e-12 * scale
    assert float((rec.cpu() - g.fbp(v)).abs().max()) < 1e-12 * scale
    ones = torch.ones(1, 1, H, W)
    h = A(ones.cuda().bfloat16())  # the fp32 product, rounded; the rule at bf16's 2^-9 covers a bf16 product throughout as well
    assert not names and h.dtype == torch.bfloat16
    assert ((h.double().cpu() - g.apply(ones)).abs() <= (g.nnz_rows + 3) * 2.0 ** -9 * g.apply(ones)).all()
    assert A(x.float().cuda()).dtype == torch.float32 and names == ["az_op_radon_f32"]


def test_transforms_issue_the_same_launches(monkeypatch):
    H, W = 16, 24
    A = _operator(rc.ANGLES, H, W)
    gen = torch.Generator().manual_seed(9)
    x, w = torch.randn(2, 3, H, W, generator=gen).cuda(), torch.randn(2, 3, A.angles, A.det_count, generator=gen).cuda()
    names = _spy(monkeypatch)
    y, want_t, rec = A(x), A.adjoint(w), A.fbp(w)
    for fn, launches in ((lambda: torch.func.jvp(A, (x,), (x,))[1], 2), (lambda: A(x), 1)):  # (jvp: the primal and the tangent)
        names.clear()
        assert torch.equal(fn(), y) and names == ["az_op_radon_f32"] * launches
    xr = x.clone().requires_grad_()
    names.clear()
    assert torch.equal(torch.autograd.grad(A(xr), xr, w)[0], want_t) and names == ["az_op_radon_f32", "az_op_radon_adj_f32"]
    names.clear()
    assert torch.equal(torch.func.vjp(A, x)[1](w)[0], want_t) and names == ["az_op_radon_f32", "az_op_radon_adj_f32"]
    names.clear()
    assert torch.equal(A.T(w), want_t) and names == ["az_op_radon_adj_f32"]
    names.clear()
    assert torch.equal(torch.func.jvp(A.fbp, (w,), (w,))[1], rec) and set(names) == {"az_op_radon_filter_f32", "az_op_radon_adj_f32"}
    wr = w.clone().requires_grad_()
    names.clear()
    rec_t = torch.autograd.grad(A.fbp(wr), wr, x)[0]  # the transpose of fbp: (pi / A) h * (A g)
    assert names == ["az_op_radon_filter_f32", "az_op_radon_adj_f32", "az_op_radon_f32", "az_op_radon_filter_f32"]
    assert torch.equal(torch.func.vjp(A.fbp, w)[1](x)[0], rec_t)
    assert torch.equal(rec_t, A._filter(y, A.fbp_scale))


# ---------------------------------------------------------------------------------------------------------------- guidance
def _ct_setup(golden):
    r"""As ``_mri_setup``, with one difference that the operator's size forces.  The ortho-normalised Fourier operator has norm 1,
    and the fixture's ``var_y`` = 1 is a noise level for such an operator.  A sinogram is a line integral: ``||M||_2^2 <=
    ||M||_1 ||M||_inf``, the number of angles (a pixel's weights sum to 1 per angle) times the heaviest bin (about a diagonal's
    length), here about 300.  With ``var_y`` = 1 the term ``A J A^T`` (MMPS) or ``A^T A / var_y`` (DiffPIR) outweighs the identity
    term by that factor, two ``cg`` iterations of the reference's solver -- whose inner products run over the last axis only and
    whose system, with a network Jacobian inside, is not symmetric -- break down, and the fp32 run of the restatement itself is
    NaN (checked on the host).  The noise variance is therefore the fixture's times that norm bound, computed from the oracle's
    matrix: the observation ``A x / sqrt(bound)`` at the fixture's noise level, written as a variance."""
    from test_gpu_guidance_vjp import device_denoiser

    from azula_amd.guidance import RadonOperator, radon_angles

    g = golden("g28_guidance_vjp")
    mean64, _, arr64, sd, cfg = gc.setup(g, torch.float64)
    mean32, _, arr32, _, _ = gc.setup(g)
    H, W = g["x_t"].shape[2:]
    A = RadonOperator(radon_angles(12), (H, W), flatten=True)  # sparse view: 12 projections
    M = ro.geometry(tuple(radon_angles(12).tolist()), H, W).dense()

    def A_oracle(z):  # the dense M32 matmul in the tensor's dtype
        return (z.flatten(2) @ M.to(z.dtype).T).flatten(1)

    var_y = g.meta["var_y"] * float(M.sum(0).max() * M.sum(1).max())
    gen = torch.Generator().manual_seed(17)
    clean = A_oracle(torch.rand(g["x_t"].shape, generator=gen) - 0.5)
    y = clean + var_y ** 0.5 * torch.randn(clean.shape, generator=gen)
    return g, device_denoiser(sd, cfg), A, A_oracle, y, var_y, (mean64, arr64), (mean32, arr32)


def _check(tag, out, ref, ref32):
    assert out.shape == ref.shape and torch.isfinite(out).all()
    scale = float(ref.abs().max())
    err, e_ref = float((out.double().cpu() - ref).abs().max()) / scale, float((ref32.double() - ref).abs().max()) / scale
    print(f"{tag}: err {err:.3e} e_ref {e_ref:.3e} bound {max(4 * e_ref, 1e-4):.3e}")
    assert err < max(4 * e_ref, 1e-4)


def test_dps_ct_step(golden, monkeypatch):
    r"""One DPS step of 12-view CT on the fixture's denoiser, set up as ``test_dps_mri_step``: against the fp64 restatement with
    the dense matrix as A, at max(4 e_ref, 1e-4)."""
    from test_gpu_guidance_vjp import SEED

    from azula_amd.guidance import DPSSampler

    g, den, A, A_oracle, y, var_y, (mean64, arr64), (mean32, arr32) = _ct_setup(golden)
    x_t, t, s = g["x_t"].cuda(), g["t"].cuda(), g["s"].cuda()
    torch.manual_seed(SEED)
    eps = torch.randn_like(x_t).cpu()
    torch.manual_seed(SEED)
    names = _spy(monkeypatch)
    out = DPSSampler(den, y.cuda(), A, steps=g.meta["steps"], silent=True).step(x_t, t, s)
    assert set(names) == {"az_op_radon_f32", "az_op_radon_adj_f32"}
    ref = go.dps_step(mean64, arr64["x_t"], arr64["t"], arr64["s"], eps.double(), y=y.double(), A=A_oracle)
    ref32 = go.dps_step(mean32, arr32["x_t"], arr32["t"], arr32["s"], eps, y=y, A=A_oracle)
    _check("dps ct", out, ref, ref32)


def test_mmps_ct_mean(golden, monkeypatch):
    r"""``MMPSDenoiser`` (cg, 2 iterations) with the same operator: ``autograd.grad`` on a retained graph and ``func.jvp``."""
    from azula_amd.guidance import MMPSDenoiser
    from azula_amd.linalg.covariance import IsotropicCovariance

    g, den, A, A_oracle, y, var_y, (mean64, arr64), (mean32, arr32) = _ct_setup(golden)
    names = _spy(monkeypatch)
    cov = IsotropicCovariance(torch.tensor(var_y, device="cuda"))
    out = MMPSDenoiser(den, y.cuda(), A, cov, solver="cg", iterations=2)(g["x_t"].cuda(), g["t"].cuda()).mean
    assert set(names) == {"az_op_radon_f32", "az_op_radon_adj_f32"}
    ref = go.mmps_mean(mean64, arr64["x_t"], arr64["t"], y.double(), A_oracle, lambda v: var_y * v, "cg", 2)
    ref32 = go.mmps_mean(mean32, arr32["x_t"], arr32["t"], y, A_oracle, lambda v: var_y * v, "cg", 2)
    _check("mmps ct", out, ref, ref32)


def test_diffpir_ct_mean(golden, monkeypatch):
    r"""``DiffPIRDenoiser`` (cg, 2 iterations): the normal equations that need A^T to be the transpose of A."""
    from azula_amd.guidance import DiffPIRDenoiser

    g, den, A, A_oracle, y, var_y, (mean64, arr64), (mean32, arr32) = _ct_setup(golden)
    names = _spy(monkeypatch)
    out = DiffPIRDenoiser(den, y.cuda(), A, var_y, solver="cg", iterations=2)(g["x_t"].cuda(), g["t"].cuda()).mean
    assert set(names) == {"az_op_radon_f32", "az_op_radon_adj_f32"}
    ref = do.diffpir_fn(mean64, y.double(), A_oracle, var_y, solver="cg", iterations=2)(arr64["x_t"], arr64["t"])
    ref32 = do.diffpir_fn(mean32, y, A_oracle, var_y, solver="cg", iterations=2)(arr32["x_t"], arr32["t"])
    _check("diffpir ct", out, ref, ref32)
