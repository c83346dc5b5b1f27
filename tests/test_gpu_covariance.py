r"""``azula_amd.linalg.covariance``, ``GaussianDenoiser`` and ``JFPSDenoiser`` on the GPU: the covariance kernels against
the fp64 host evaluation of the same covariance (every class, fp32 and fp64, small to 3 x 256 x 256, ranks 1 to 200, Full at
N = 3072), the fallbacks, dtype promotion, batch and run invariance, the denoiser against its fp64 host form and in the
captured sampling loop, plan invalidation, and JFPS on a small UNet.

Bounds, relative to the output's largest magnitude: fp64 outputs 1e-11 (only the summation order differs from the host's
einsums: a few ulp times the longest dot product, 3072 or 196608 terms of O(1) factors).  fp32 outputs of ``@`` 3e-5: every
operand is rounded to fp32 once (2^-24 relative each) and the dot products accumulate about sqrt(terms) ulp on top, so
N = 196608 gives ~1e-5.  ``inv`` and ``color`` of the low-rank classes run their r x r ``eigh`` setup in the factors' dtype,
which multiplies that by the conditioning of the capacitance (below 10 for the factors drawn here): 3e-4 in fp32."""

import math

import pytest
import torch

from conftest import max_err

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32


def _spy(monkeypatch):
    from azula_amd import _lib

    names, call = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (names.append(name), call(name, *a))[1])
    return names


def _orth(n, gen):
    Q, _ = torch.linalg.qr(torch.randn(n, n, generator=gen, dtype=F64))
    return Q.contiguous()


def _make(kind, shape, rank=16, seed=0):
    r"""A host fp64 covariance of ``kind`` on ``shape``, well conditioned."""
    from azula_amd.linalg import covariance as cv

    gen = torch.Generator().manual_seed(seed)
    n = math.prod(shape)
    D = 0.5 + torch.rand(shape, generator=gen, dtype=F64)
    if kind == "isotropic":
        return cv.IsotropicCovariance(torch.tensor(1.7, dtype=F64))
    if kind == "diagonal":
        return cv.DiagonalCovariance(D)
    if kind == "full":
        Q = _orth(n, gen).reshape(*shape, n)
        return cv.FullCovariance(Q, 0.5 + torch.rand(n, generator=gen, dtype=F64))
    if kind in ("dplr", "dmlr"):
        if rank == 200:  # the concatenated V of a sum of two DPLRs
            a, b = _make("dplr", shape, 136, seed + 1), _make("dplr", shape, 64, seed + 2)
            return a + b
        V = torch.randn(*shape, rank, generator=gen, dtype=F64) * (0.3 / math.sqrt(rank))
        if kind == "dmlr":  # diag(D) - V V^T positive definite: V^T D^-1 V well under I
            V = V * (2.0 / math.sqrt(n))
            return cv.DMLRCovariance(D + 1.0, V)
        return cv.DPLRCovariance(D, V)
    if kind == "kronecker":
        Qs = [_orth(m, gen) for m in shape]
        return cv.KroneckerCovariance(Qs, cv.DiagonalCovariance(D))
    if kind == "kronecker_dplr":
        Qs = [_orth(m, gen) for m in shape]
        r = min(8, n // 2)
        V = torch.randn(*shape, r, generator=gen, dtype=F64) * (0.3 / math.sqrt(r))
        return cv.KroneckerCovariance(Qs, cv.DPLRCovariance(D, V))
    raise ValueError(kind)


def _check(out, ref, dtype, op):
    sc = max(ref.abs().max().item(), 1e-30)
    bound = 1e-11 if dtype == F64 else (3e-5 if op == "matmul" else 3e-4)
    err = max_err(out.double().cpu(), ref)
    assert out.dtype == dtype and out.is_cuda and out.shape == ref.shape
    assert err <= bound * sc, (op, err / sc)


def _ops(cov):
    return {"matmul": lambda x: cov @ x, "inv": lambda x: cov.inv @ x, "color": lambda x: cov.color(x)}


CASES = (
    [(k, s, r) for k in ("isotropic", "diagonal", "dplr", "dmlr", "kronecker", "kronecker_dplr") for s, r in (((5,), 2), ((3, 5), 4))]
    + [(k, (3, 64, 64), 16) for k in ("isotropic", "diagonal", "dplr", "dmlr", "kronecker", "kronecker_dplr")]
    + [("dplr", (3, 64, 64), r) for r in (1, 64, 200)]
    + [("full", (5,), 0), ("full", (3, 5), 0), ("full", (3, 32, 32), 0)]
)


@pytest.mark.parametrize("kind,shape,rank", CASES)
@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("batch", [(), (4,), (2, 3)])
def test_applies_match_the_host_fp64(kind, shape, rank, dtype, batch, monkeypatch):
    host = _make(kind, shape, rank)
    dev = host.to(device="cuda", dtype=dtype)
    gen = torch.Generator().manual_seed(7)
    x = torch.randn(*batch, *shape, generator=gen, dtype=F64)
    names = _spy(monkeypatch)
    for op, fn in _ops(dev).items():
        names.clear()
        _check(fn(x.to(device="cuda", dtype=dtype)), _ops(host)[op](x), dtype, op)
        assert any(n.startswith("az_cov_") for n in names), op  # each op on the kernels, none a silent fallback


@pytest.mark.parametrize("kind", ["diagonal", "dplr", "dmlr", "kronecker", "kronecker_dplr"])
@pytest.mark.parametrize("dtype", [F32, F64])
def test_full_size_images(kind, dtype):
    shape = (3, 256, 256)
    host = _make(kind, shape, 16)
    dev = host.to(device="cuda", dtype=dtype)
    x = torch.randn(4, *shape, generator=torch.Generator().manual_seed(3), dtype=F64)
    for op, fn in _ops(dev).items():
        _check(fn(x.to(device="cuda", dtype=dtype)), _ops(host)[op](x), dtype, op)


def test_rank_64_and_200_on_full_size_images():
    shape = (3, 256, 256)
    x = torch.randn(2, *shape, generator=torch.Generator().manual_seed(4), dtype=F64)
    for rank in (64, 200):
        host = _make("dplr", shape, rank)
        dev = host.to(device="cuda", dtype=F32)
        _check(dev @ x.cuda().float(), host @ x, F32, "matmul")


def test_full_at_3072_batch_64():
    host = _make("full", (3, 32, 32))
    x = torch.randn(64, 3, 32, 32, generator=torch.Generator().manual_seed(5), dtype=F64)
    for dtype in (F32, F64):
        dev = host.to(device="cuda", dtype=dtype)
        for op, fn in _ops(dev).items():
            _check(fn(x.to(device="cuda", dtype=dtype)), _ops(host)[op](x), dtype, op)


@pytest.mark.parametrize("kind", ["diagonal", "full", "dplr", "kronecker"])
def test_a_row_is_the_same_in_any_batch_and_run(kind):
    shape = (3, 16, 16) if kind != "full" else (3, 8, 8)
    dev = _make(kind, shape, 24).to(device="cuda", dtype=F32)
    x = torch.randn(9, *shape, generator=torch.Generator().manual_seed(6)).cuda()
    for fn in _ops(dev).values():
        full = fn(x)
        assert torch.equal(full, fn(x))
        for r in (0, 4, 8):
            assert torch.equal(fn(x[r].clone()), full[r])
            assert torch.equal(fn(x[r : r + 1].clone()), full[r : r + 1])


def test_promotion_follows_torch():
    from azula_amd.linalg import covariance as cv

    D = (0.5 + torch.rand(3, 5, dtype=F64)).cuda()
    x = torch.randn(4, 3, 5).cuda()
    for cov in (cv.DiagonalCovariance(D), cv.DPLRCovariance(D, 0.1 * torch.randn(3, 5, 2, dtype=F64).cuda())):
        y = cov @ x
        assert y.dtype == F64
        assert max_err(y, cov @ x.double()) <= 1e-15 * y.abs().max().item()
    assert (cv.DiagonalCovariance(D.float()) @ x.double()).dtype == F64
    assert (cv.IsotropicCovariance(torch.tensor(2.0, dtype=F64).cuda()) @ x).dtype == F32  # a 0-d tensor does not promote


@pytest.mark.parametrize("case", ["bf16_x", "strided_factor"])
def test_cases_the_kernels_do_not_take_match_the_torch_sequence(case, monkeypatch):
    from azula_amd.linalg import covariance as cv

    host = _make("dplr", (3, 8, 8), 4)
    D, V = host.D.float().cuda(), host.V.float().cuda()
    x = torch.randn(2, 3, 8, 8).cuda()
    if case == "bf16_x":  # (no color: torch has no bf16 eigh on the device, in the reference's sequence either)
        x = x.bfloat16()
        cov = cv.DPLRCovariance(D.bfloat16(), V.bfloat16())
        ops = [lambda: cov @ x, lambda: cv.DiagonalCovariance(cov.D) @ x]
    else:
        cov = cv.DPLRCovariance((torch.rand(3, 8, 16) + 0.5).cuda()[..., ::2], V)
        assert not cov.D.is_contiguous()
        ops = [lambda: cov @ x, lambda: cov.color(x), lambda: cv.DiagonalCovariance(cov.D) @ x]
    names = _spy(monkeypatch)
    got = [op() for op in ops]
    assert not any(n.startswith("az_cov_") for n in names)
    monkeypatch.setattr(cv, "_kernels_take", lambda *a: False)
    want = [op() for op in ops]
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and torch.equal(g, w)


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs")
def test_applies_on_a_device_that_is_not_current():
    from azula_amd.denoise import GaussianDenoiser
    from azula_amd.noise import VPSchedule

    x = torch.randn(2, 3, 16, 16, generator=torch.Generator().manual_seed(8))
    for kind in ("diagonal", "dplr", "kronecker", "full"):
        host = _make(kind, (3, 16, 16) if kind != "full" else (3, 16, 16), 8)
        on1 = host.to(device="cuda:1", dtype=F32)
        with torch.cuda.device(0):
            for op, fn in _ops(on1).items():
                out = fn(x.to("cuda:1", F32))
                assert out.device == torch.device("cuda:1")
                _check(out, _ops(host)[op](x.double()), F32, op)
    den = GaussianDenoiser(torch.zeros(3, 16, 16), _make("diagonal", (3, 16, 16)), VPSchedule()).to(device="cuda:1",
                                                                                                     dtype=F32)
    with torch.cuda.device(0):
        assert torch.isfinite(den(x.to("cuda:1"), torch.tensor(0.5)).mean).all()


def test_diagonal_rejects_a_partial_row():
    from azula_amd.linalg import covariance as cv

    cov = cv.DiagonalCovariance(torch.ones(3, 5, device="cuda"))
    with pytest.raises(RuntimeError):
        cov @ torch.ones(7, device="cuda")


def test_entries_reject_bad_arguments():
    import ctypes as C

    from azula_amd import _lib

    lib = _lib.lib()
    assert lib.az_cov_scale(None, None) == -1
    x = torch.zeros(8, device="cuda")
    a = _lib.AzCovScaleArgs(x=x.data_ptr(), y=x.data_ptr(), rows=1, n=8, h=9)
    assert lib.az_cov_scale(C.byref(a), None) == -4
    a.h, a.out_dtype = 0, 1  # fp32 x and factors cannot give fp64
    assert lib.az_cov_scale(C.byref(a), None) == -4
    m = _lib.AzCovModeArgs(x=x.data_ptr(), Q=x.data_ptr(), y=x.data_ptr(), outer=1, n=2, inner=4)
    assert lib.az_cov_mode(C.byref(m), None) == -4  # in place


# ------------------------------------------------------------------------------------------------------- GaussianDenoiser
def _gaussian(kind, shape=(3, 8, 8), dtype=F32, rank=4):
    from azula_amd.denoise import GaussianDenoiser
    from azula_amd.noise import VPSchedule

    mean = torch.randn(shape, generator=torch.Generator().manual_seed(11), dtype=F64)
    host = GaussianDenoiser(mean, _make(kind, shape, rank), VPSchedule())
    dev = GaussianDenoiser(mean.clone(), _make(kind, shape, rank), VPSchedule()).to(device="cuda", dtype=dtype)
    return host, dev


SPECTRAL = ["isotropic", "diagonal", "full", "kronecker"]


@pytest.mark.parametrize("kind", SPECTRAL + ["dplr"])
@pytest.mark.parametrize("dtype", [F32, F64])
def test_gaussian_denoiser_matches_the_host_fp64(kind, dtype):
    host, dev = _gaussian(kind, dtype=dtype)
    x = torch.randn(4, 3, 8, 8, generator=torch.Generator().manual_seed(12), dtype=F64)
    for t in (0.05, 0.5, 0.99):
        tt = torch.tensor(t, dtype=F64)
        ref = host(x, tt).mean
        out = dev(x.to(device="cuda", dtype=dtype), tt.to(dtype)).mean
        # the host form cancels like 1/alpha (x ~ 1 at t = 0.99 means z ~ 50): its own fp64 round-off is the floor there
        bound = (1e-10 if dtype == F64 else 1e-4) * max(1.0, ref.abs().max().item())
        assert out.dtype == dtype and max_err(out.double().cpu(), ref) <= bound, (t, max_err(out.double().cpu(), ref))
    if dtype == F32:
        out = dev(x.float().cuda(), torch.tensor(1.0)).mean
        assert torch.isfinite(out).all()


def test_device_gaussian_denoiser_matches_g27(golden):
    from test_covariance_host import rebuild

    from azula_amd.denoise import GaussianDenoiser
    from azula_amd.noise import VPSchedule

    g = golden("g27_covariance")
    tags = [t for t in g.meta["cases"] if t.startswith("gd_")]
    assert len(tags) == 10
    for tag in tags:
        kw = g.meta["cases"][tag]
        dtype = getattr(torch, kw["dtype"])
        den = GaussianDenoiser(g[f"gd_mean_{kw['dtype']}"], rebuild(g, tag + "__f_", kw["factors"]), VPSchedule()).cuda()
        for t in kw["times"]:
            out = den(g[f"gd_x_{kw['dtype']}"].cuda(), torch.tensor(t, dtype=dtype)).mean
            ref = g[f"{tag}_t{t}"]
            # G27 holds the reference's form, which cancels (|z| ~ 1 / alpha): its own round-off, a few ulp of |x_t| / alpha
            # (alpha(0.99) ~ 1e-3), adds to the device's relative bound
            alpha = VPSchedule()(torch.tensor(t, dtype=F64))[0].item()
            eps = torch.finfo(dtype).eps
            bound = (1e-10 if dtype == F64 else 1e-4) * max(1.0, ref.abs().max().item())
            bound += 8 * eps * g[f"gd_x_{kw['dtype']}"].abs().max().item() / alpha
            assert out.dtype == dtype and max_err(out, ref) <= bound, (tag, t, max_err(out, ref))


def _loops(sampler_cls, den, x, monkeypatch):
    r"""(captured loop, generic loop) from the same state of the device generator."""
    from azula_amd import sample

    s = sampler_cls(den, steps=16, silent=True)
    torch.manual_seed(5)
    fused = s(x)
    cached = len(s._fused_cache)
    with monkeypatch.context() as m:
        m.setattr(sample.Sampler, "_fusable", lambda self, x: False)
        torch.manual_seed(5)
        generic = s(x)
    return fused, generic, cached


@pytest.mark.parametrize("kind", SPECTRAL)
@pytest.mark.parametrize("sampler", ["DDIMSampler", "EulerSampler"])
def test_captured_loop_matches_the_generic_loop_and_the_host(kind, sampler, monkeypatch):
    from azula_amd import sample

    host, dev = _gaussian(kind)
    x = torch.randn(4, 3, 8, 8, generator=torch.Generator().manual_seed(13))
    cls = getattr(sample, sampler)
    fused, generic, cached = _loops(cls, dev, x.cuda(), monkeypatch)
    assert cached == 1, "the spectral covariances run in the captured loop"
    sc = max(1.0, generic.abs().max().item())
    assert max_err(fused, generic) <= 2e-4 * sc, max_err(fused, generic)
    if sampler == "EulerSampler":  # deterministic: the fp64 host loop is the reference
        ref = cls(host, steps=16, silent=True)(x.double())
        assert max_err(fused.double().cpu(), ref) <= 2e-4 * sc, max_err(fused.double().cpu(), ref)


def test_dplr_runs_the_generic_loop(monkeypatch):
    from azula_amd import sample

    host, dev = _gaussian("dplr")
    x = torch.randn(4, 3, 8, 8, generator=torch.Generator().manual_seed(14))
    names = _spy(monkeypatch)
    out = sample.EulerSampler(dev, steps=16, silent=True)(x.cuda())
    ref = sample.EulerSampler(host, steps=16, silent=True)(x.double())
    assert "az_cov_project" in names and "az_graph_launch" not in names
    assert max_err(out.double().cpu(), ref) <= 2e-4 * max(1.0, ref.abs().max().item())


def test_reassigned_or_edited_cov_rebuilds_the_plan(monkeypatch):
    from azula_amd import sample
    from azula_amd.linalg import covariance as cv

    _, dev = _gaussian("diagonal")
    x = torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(15)).cuda()
    s = sample.EulerSampler(dev, steps=8, silent=True)

    def generic():
        with monkeypatch.context() as m:
            m.setattr(sample.Sampler, "_fusable", lambda self, x: False)
            return s(x)

    a = s(x)
    plan = next(iter(s._fused_cache.values()))
    dev.cov = cv.DiagonalCovariance(dev.cov.D * 3)
    b = s(x)
    assert next(iter(s._fused_cache.values())) is not plan and not torch.equal(a, b)
    assert max_err(b, generic()) <= 2e-4 * max(1.0, b.abs().max().item())
    plan = next(iter(s._fused_cache.values()))
    dev.cov.D.mul_(0.25)
    c = s(x)
    assert next(iter(s._fused_cache.values())) is not plan
    assert max_err(c, generic()) <= 2e-4 * max(1.0, c.abs().max().item())
    dev.mean.add_(1.0)
    d = s(x)
    assert max_err(d, generic()) <= 2e-4 * max(1.0, d.abs().max().item()) and not torch.equal(c, d)


def test_fp64_sampler_clock_takes_the_generic_loop(monkeypatch):
    from azula_amd import sample

    host, dev = _gaussian("diagonal")
    x = torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(16))
    s = sample.EulerSampler(dev, steps=8, silent=True, dtype=F64)
    built = []
    fused = type(dev)._az_fused
    monkeypatch.setattr(type(dev), "_az_fused", lambda self, *a: (built.append(1), fused(self, *a))[1])
    out = s(x.cuda())
    s(x.cuda())
    assert len(built) == 1, "the fp32-only program is built once, then the rejection is cached"
    assert all(v is sample._NOT_WIDE for v in s._fused_cache.values())
    ref = sample.EulerSampler(host, steps=8, silent=True, dtype=F64)(x)
    assert max_err(out.double().cpu(), ref.double()) <= 2e-4 * max(1.0, ref.abs().max().item())


# ------------------------------------------------------------------------------------------------------------------ JFPS
def _mask_op(seed, shape):
    m = (torch.rand(shape, generator=torch.Generator().manual_seed(seed)) > 0.5).float()
    return m, (lambda x: x * m.to(x))


@pytest.mark.parametrize("kind", ["isotropic", "diagonal", "dplr", "kronecker"])
@pytest.mark.parametrize("solver", ["cg", "gmres"])
def test_jfps_on_the_unet_matches_the_host(golden, kind, solver, monkeypatch):
    from test_gpu_diffpir import _unet

    from azula_amd.guidance import JFPSDenoiser
    from azula_amd.linalg import covariance as cv

    import covariance_oracle as co

    g, den, omean = _unet(golden)
    x_t, t = g["dp_x_t"], g["dp_t"]
    shape = tuple(x_t.shape[1:])
    alpha_t, sigma_t = co.vp(t)
    mask, A = _mask_op(21, shape)
    y = A(omean(x_t, t)) + 0.05 * torch.randn(x_t.shape, generator=torch.Generator().manual_seed(22))
    cov_x = _make(kind, shape, 4)
    cov_y = cv.IsotropicCovariance(0.05)
    names = _spy(monkeypatch)
    jf = JFPSDenoiser(den, y.cuda(), A, cov_y, cov_x.to(device="cuda", dtype=F32), solver=solver, iterations=3)
    out = jf(x_t.cuda(), t.cuda()).mean
    from test_covariance_host import as_dict

    ref = co.jfps_mean(omean(x_t, t), alpha_t, sigma_t, y, A, co.iso(0.05), as_dict(cov_x.to(dtype=F32)), solver, 3)
    err, sc = max_err(out, ref), max(1.0, ref.abs().max().item())
    # (CG on the Kronecker case runs away, to |mean| ~ 1e9, in the host restatement as much as here: the three iterations
    #  amplify the fp32 round-off of the operator by the same growth, so the agreement is relative to that scale)
    bound = 2e-3 if (kind, solver) == ("kronecker", "cg") else 5e-4
    assert out.dtype == F32 and err < bound * sc, err
    assert f"az_{solver}_init" in names and any(n.startswith("az_cov_") for n in names)
    assert jf._az_fused(x_t.cuda(), {}, torch.zeros(16, device="cuda")) is None


def test_jfps_ddim_loop_runs_generic_and_matches(golden, monkeypatch):
    from test_gpu_diffpir import _unet

    from azula_amd import sample
    from azula_amd.guidance import JFPSDenoiser
    from azula_amd.linalg import covariance as cv

    g, den, omean = _unet(golden)
    shape = tuple(g["dp_x_t"].shape[1:])
    mask, A = _mask_op(23, shape)
    y = A(torch.randn(1, *shape, generator=torch.Generator().manual_seed(24)))
    jf = JFPSDenoiser(den, y.cuda(), A, cv.IsotropicCovariance(0.05), _make("diagonal", shape).to(device="cuda", dtype=F32))
    x = torch.randn(1, *shape, generator=torch.Generator().manual_seed(25)).cuda()
    s = sample.DDIMSampler(jf, steps=8, silent=True)
    out = s(x)
    assert not s._fused_cache and torch.isfinite(out).all()


def test_jfps_at_full_size_is_finite():
    import bench

    from azula_amd.guidance import JFPSDenoiser
    from azula_amd.linalg import covariance as cv

    den = bench.build_denoiser(bench.CONFIGS["c2"], torch.device("cuda"))
    shape = (3, 256, 256)
    mask, A = _mask_op(26, shape)
    y = A(torch.randn(4, *shape, generator=torch.Generator().manual_seed(27))).cuda()
    jf = JFPSDenoiser(den, y, A, cv.IsotropicCovariance(0.05), _make("diagonal", shape).to(device="cuda", dtype=F32))
    out = jf(torch.randn(4, *shape).cuda(), torch.tensor(0.5).cuda()).mean
    assert out.shape == (4, *shape) and torch.isfinite(out).all()
