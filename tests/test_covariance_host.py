r"""``azula_amd.linalg.covariance``, ``GaussianDenoiser`` and ``JFPSDenoiser`` without a GPU: the public API against the
reference's recorded signatures; host applies, ``inv``, ``color``, ``logdet``, the algebra and both denoisers against the
restatement of ``tests/covariance_oracle.py`` (independent of ``azula_amd``) bit for bit and against fixture G27 within the
round-off of another CPU; the covariance identities in fp64 for every ``from_data`` variant; the algebra's dispatch rules;
JFPS's public surface; the C ABI of the covariance entries; and the cases of the kernel tests (tests/covariance_cases.py): they reach
every tile constant, the exact family is exact in fp32, five planted faults change its reference, and torch's own evaluation meets
the hard family's derived bound."""

import ctypes
import inspect
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import covariance_cases as cc
import covariance_oracle as co
from conftest import ROOT, max_err
from oracle import nets, sampling, synth

F64 = torch.float64


def _data(shape=(3, 5), samples=64, seed=0):
    g = torch.Generator().manual_seed(seed)
    mix = torch.randn(math.prod(shape), math.prod(shape), generator=g, dtype=F64) / math.prod(shape) ** 0.5
    return (torch.randn(samples, math.prod(shape), generator=g, dtype=F64) @ mix + 0.3 * torch.randn(
        samples, math.prod(shape), generator=g, dtype=F64)).reshape(samples, *shape)


def _variants():
    from azula_amd.linalg import covariance as cv

    torch.manual_seed(0)  # (lobpcg draws its start)
    X = _data()
    return {
        "diagonal": cv.DiagonalCovariance.from_data(X),
        "full": cv.FullCovariance.from_data(X),
        "dplr_pca": cv.DPLRCovariance.from_data(X, rank=2),
        "dplr_em": cv.DPLRCovariance.from_data(X, rank=2, iterations=3),
        "dplr_eigh": cv.DPLRCovariance.from_data(X, rank=5),
        "kronecker": cv.KroneckerCovariance.from_data(X),
        "kronecker_dplr": cv.KroneckerCovariance.from_data(X, rank=2),
        "kronecker_dplr_em": cv.KroneckerCovariance.from_data(X, rank=2, iterations=2),
    }


def _dense(cov, n, shape):
    return torch.stack([cov(e.reshape(shape)).reshape(n) for e in torch.eye(n, dtype=F64)], dim=1)


@pytest.mark.parametrize("name", ["diagonal", "full", "dplr_pca", "dplr_em", "dplr_eigh", "kronecker", "kronecker_dplr",
                                  "kronecker_dplr_em"])
def test_identities_hold_in_fp64(name):
    cov = _variants()[name]
    shape = (3, 5)
    x = torch.randn(4, *shape, generator=torch.Generator().manual_seed(1), dtype=F64)
    sc = x.abs().max().item()
    assert max_err(cov.inv(cov(x)), x) < 1e-10 * sc
    assert max_err(cov(cov.inv(x)), x) < 1e-10 * sc
    assert max_err(cov.inv.inv(x), cov(x)) < 1e-10 * cov(x).abs().max().item()
    C_ = _dense(cov, 15, shape)
    L_ = _dense(cov.color, 15, shape)
    assert max_err(L_ @ L_.T, C_) < 1e-10 * C_.abs().max().item()
    assert abs(cov.logdet().item() + cov.inv.logdet().item()) < 1e-9 * max(1.0, abs(cov.logdet().item()))
    assert abs(cov.logdet().item() - torch.linalg.slogdet(C_).logabsdet.item()) < 1e-9 * max(1.0, abs(cov.logdet().item()))


def test_algebra_follows_the_reference_rules():
    from azula_amd.linalg import covariance as cv

    D = torch.rand(3, 5, dtype=F64) + 0.5
    V = torch.randn(3, 5, 2, dtype=F64)
    iso, diag, dplr = cv.IsotropicCovariance(2.0), cv.DiagonalCovariance(D), cv.DPLRCovariance(D, V)
    assert isinstance(iso + diag, cv.DiagonalCovariance)  # through Diagonal.__radd__
    assert isinstance(diag + dplr, cv.DPLRCovariance) and (diag + dplr).rank == 2
    assert (dplr + dplr).rank == 4 and isinstance(dplr.inv, cv.DMLRCovariance) and isinstance(dplr.inv.inv, cv.DPLRCovariance)
    assert isinstance(cv.IsotropicCovariance(torch.tensor(2.0)) * dplr, cv.DPLRCovariance)
    with pytest.raises(TypeError):
        dplr + dplr.inv
    with pytest.raises(NotImplementedError):
        iso.shape
    with pytest.raises(NotImplementedError):
        iso.logdet()
    assert dplr.shape == (3, 5) and cv.FullCovariance(torch.eye(15, dtype=F64).reshape(3, 5, 15), D.flatten()).shape == (3, 5)
    moved = dplr.to(torch.float32)
    assert moved.D.dtype == torch.float32 and moved.V.dtype == torch.float32 and dplr.D.dtype == F64
    kron = cv.KroneckerCovariance([torch.eye(3, dtype=F64), torch.eye(5, dtype=F64)], diag).to(torch.float32)
    assert all(Q.dtype == torch.float32 for Q in kron.Qs) and kron.L.D.dtype == torch.float32
    assert kron.is_floating_point()


def test_gaussian_denoiser_to_moves_mean_and_cov():
    from azula_amd.denoise import GaussianDenoiser
    from azula_amd.linalg import covariance as cv
    from azula_amd.noise import VPSchedule

    den = GaussianDenoiser(torch.zeros(3, 5), cv.DiagonalCovariance(torch.ones(3, 5)), VPSchedule()).to(F64)
    assert den.mean.dtype == F64 and den.cov.D.dtype == F64
    assert "GaussianDenoiser" in __import__("azula_amd.denoise", fromlist=["__all__"]).__all__


def test_jfps_surface():
    from azula_amd.guidance import JFPSDenoiser
    from azula_amd.denoise import GaussianDenoiser
    from azula_amd.linalg import covariance as cv
    from azula_amd.noise import VPSchedule

    inner = GaussianDenoiser(torch.zeros(3, 5), cv.DiagonalCovariance(torch.ones(3, 5)), VPSchedule())
    with pytest.raises(ValueError):
        JFPSDenoiser(inner, torch.zeros(3, 5), lambda x: x, cv.IsotropicCovariance(0.1), cv.IsotropicCovariance(1.0), solver="lu")
    jf = JFPSDenoiser(inner, torch.zeros(1, 3, 5), lambda x: x, cv.IsotropicCovariance(0.1), cv.IsotropicCovariance(1.0))
    assert jf._az_fused(torch.zeros(1, 3, 5), {}, torch.zeros(16)) is None
    assert jf.schedule is inner.schedule


def test_entries_are_exported_and_reject_bad_arguments():
    from azula_amd import _lib

    lib = _lib.lib()
    for name in ("az_cov_scale", "az_cov_project", "az_cov_expand", "az_cov_mode", "az_cov_segments"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
    assert lib.az_version() == 1
    assert lib.az_cov_segments(0) == 0 and lib.az_cov_segments(512) == 1 and lib.az_cov_segments(513) == 2
    for fn in (lib.az_cov_scale, lib.az_cov_project, lib.az_cov_expand, lib.az_cov_mode):
        assert fn(None, None) == -1
    a = _lib.AzCovLowRankArgs(x=8, W=8, P=8, y=8, rows=0, n=4, r=2)
    assert lib.az_cov_project(ctypes.byref(a), None) == -2
    a.rows, a.x_dtype = 1, 7
    assert lib.az_cov_expand(ctypes.byref(a), None) == -4
    a.x_dtype, a.W = 0, None
    assert lib.az_cov_project(ctypes.byref(a), None) == -1
    s = _lib.AzCovScaleArgs(x=8, y=8, rows=1, n=0)
    assert lib.az_cov_scale(ctypes.byref(s), None) == -2
    s.n, s.e, s.e_len = 4, 8, 3
    assert lib.az_cov_scale(ctypes.byref(s), None) == -2
    m = _lib.AzCovModeArgs(x=8, Q=16, y=24, outer=1, n=0, inner=1)
    assert lib.az_cov_mode(ctypes.byref(m), None) == -2
    m.n, m.out_dtype = 2, 1
    assert lib.az_cov_mode(ctypes.byref(m), None) == -4


# ------------------------------------------------------------------------------------------------------------------ G27
G = "g27_covariance"


def rebuild(g, prefix: str, desc: dict):
    r"""Our covariance from the factors G27 stored under ``prefix``."""
    from azula_amd.linalg import covariance as cv

    cls = desc["cls"]
    if cls == "IsotropicCovariance":
        return cv.IsotropicCovariance(g[prefix + "lmbda"])
    if cls == "KroneckerCovariance":
        return cv.KroneckerCovariance([g[f"{prefix}Q{i}"] for i in range(desc["axes"])], rebuild(g, prefix + "L_", desc["L"]))
    return getattr(cv, cls)(*(g[prefix + k] for k in ("D", "Q", "L", "V") if prefix + k in g))


def as_dict(c) -> dict:
    r"""The restatement's form of one of our covariances (attribute reads only)."""
    n = type(c).__name__
    if n == "IsotropicCovariance":
        return co.iso(c.lmbda)
    if n == "DiagonalCovariance":
        return co.diag(c.D)
    if n == "FullCovariance":
        return co.full(c.Q, c.L)
    if n in ("DPLRCovariance", "DMLRCovariance"):
        return co.lowrank("dplr" if n == "DPLRCovariance" else "dmlr", c.D, c.V)
    return co.kron(c.Qs, as_dict(c.L))


def from_data(variant: str, X):
    from azula_amd.linalg import covariance as cv

    torch.manual_seed(0)
    cls, _, kind = variant.partition("_")
    kw = {"pca": dict(rank=1), "em": dict(rank=1, iterations=3), "eigh": dict(rank=2), "dplr": dict(rank=1, iterations=2)}
    return getattr(cv, cls).from_data(X, **kw.get(kind, {}))


def close(x, ref, rel):
    return x.dtype == ref.dtype and x.shape == ref.shape and max_err(x, ref) <= rel * max(1.0, ref.abs().max().item())


def _ops(c, dtype, shape):
    from azula_amd.linalg import covariance as cv

    ops = {"matmul": lambda x: c @ x, "inv": lambda x: c.inv @ x, "invinv": lambda x: c.inv.inv @ x, "color": c.color}
    alg = {"alg_add_iso": lambda: c + cv.IsotropicCovariance(torch.tensor(0.3, dtype=dtype)),
           "alg_mul_iso": lambda: c * cv.IsotropicCovariance(torch.tensor(2.0, dtype=dtype)),
           "alg_diag_add": lambda: cv.DiagonalCovariance(torch.full(shape, 0.2, dtype=dtype)) + c,
           "alg_self_add": lambda: c + c}
    return ops, alg


def test_api_mirrors_the_reference_signature(golden):
    from azula_amd.denoise import GaussianDenoiser
    from azula_amd.guidance import JFPSDenoiser
    from azula_amd.linalg import covariance as cv

    g = golden(G)
    ours = {f"{n}.__init__": getattr(cv, n).__init__ for n in cv.__all__ if n != "Covariance"}
    ours.update({"GaussianDenoiser.__init__": GaussianDenoiser.__init__, "JFPSDenoiser.__init__": JFPSDenoiser.__init__,
                 "DPLRCovariance.from_data": cv.DPLRCovariance.from_data,
                 "KroneckerCovariance.from_data": cv.KroneckerCovariance.from_data})
    for qual, fn in ours.items():
        names = [(n, k, d) for q, n, k, d in g.meta["signature"] if q == qual]
        assert names, qual
        params = [p for p in inspect.signature(fn).parameters.values() if p.name != "self"]
        got = [(p.name, p.kind.name, None if p.default is inspect.Parameter.empty else repr(p.default)) for p in params]
        assert got == names, qual


def test_host_covariances_equal_the_restatement_and_g27(golden):
    g = golden(G)
    tags = [t for t in g.meta["cases"] if t.startswith("cov_")]
    assert len(tags) == 57
    for tag in tags:
        kw = g.meta["cases"][tag]
        dtype, shape = getattr(torch, kw["dtype"].split(".")[-1]), tuple(kw["shape"])
        st, dn = "x".join(map(str, shape)), kw["dtype"].split(".")[-1]
        if kw["source"] == "fixed":
            c, rel = rebuild(g, tag + "__f_", kw["factors"]), (1e-12 if dtype == F64 else 1e-5)
        else:  # eigenvector signs and lobpcg's path are free across machines: compare by action
            c, rel = from_data(kw["variant"], g[f"X_{st}_{dn}"]), (1e-10 if dtype == F64 else 1e-4)
        cd = as_dict(c)
        ops, alg = _ops(c, dtype, shape)
        mine = {"matmul": lambda x: co.apply(cd, x), "inv": lambda x: co.apply(co.inv(cd), x),
                "invinv": lambda x: co.apply(co.inv(co.inv(cd)), x), "color": lambda x: co.color(cd, x)}
        for out in kw["outputs"]:
            ref = g[f"{tag}__{out}"]
            if out == "logdet":
                got = c.logdet()
                assert torch.equal(got, co.logdet(cd)), (tag, out)
            elif out.startswith("alg_"):
                x = g[f"x_{st}_{dn}_{kw['batches'][0]}"]
                got = alg[out]() @ x
                if kw["source"] == "fixed":
                    assert got.dtype == ref.dtype
            else:
                bt, op = out.split("_", 1)
                x = g[f"x_{st}_{dn}_{bt}"]
                got = ops[op](x)
                assert torch.equal(got, mine[op](x)), (tag, out)
            if kw["source"] == "data" and out.endswith("_color"):
                continue  # (color is unique only up to an orthogonal factor: pinned by colorᵀ color = C below)
            assert close(got, ref, rel), (tag, out, max_err(got, ref))


def test_host_gaussian_denoiser_equals_the_restatement_and_g27(golden):
    from azula_amd.denoise import GaussianDenoiser
    from azula_amd.noise import VPSchedule

    g = golden(G)
    tags = [t for t in g.meta["cases"] if t.startswith("gd_")]
    assert len(tags) == 10
    for tag in tags:
        kw = g.meta["cases"][tag]
        dtype = getattr(torch, kw["dtype"])
        cov = rebuild(g, tag + "__f_", kw["factors"])
        mean, x = g[f"gd_mean_{kw['dtype']}"], g[f"gd_x_{kw['dtype']}"]
        den = GaussianDenoiser(mean, cov, VPSchedule())
        for t in kw["times"]:
            tt = torch.tensor(t, dtype=dtype)
            out = den(x, tt).mean
            a, s = VPSchedule()(tt)
            assert torch.equal(out, co.gaussian_mean(mean, as_dict(cov), x, a, s)), (tag, t)
            # the reference's form divides by alpha after a sum of O(|x_t|) terms: its round-off on another CPU is a few ulp of
            # |x_t| / alpha (alpha(0.99) ~ 1e-3), on top of the usual relative round-off of the result
            ref = g[f"{tag}_t{t}"]
            eps = torch.finfo(dtype).eps
            bound = (1e-12 if dtype == F64 else 1e-5) * max(1.0, ref.abs().max().item()) + 8 * eps * x.abs().max().item() / a.item()
            assert max_err(out, ref) <= bound, (tag, t, max_err(out, ref), bound)


def test_host_ddim_loop_over_the_gaussian_denoiser(golden):
    from azula_amd.denoise import GaussianDenoiser
    from azula_amd.linalg import covariance as cv
    from azula_amd.noise import VPSchedule
    from azula_amd.sample import DDIMSampler

    g = golden(G)
    lp = g.meta["gd_loop"]
    cov, mean = cv.DiagonalCovariance(g["gd_DiagonalCovariance_float32__f_D"]), g["gd_mean_float32"]
    torch.manual_seed(lp["seed"])
    x0 = DDIMSampler(GaussianDenoiser(mean, cov, VPSchedule()), steps=lp["steps"], eta=lp["eta"], silent=True)(g["gd_loop_x1"])
    torch.manual_seed(lp["seed"])
    ref = sampling.sample(co.gaussian_fn(mean, as_dict(cov)), g["gd_loop_x1"], steps=lp["steps"], eta=lp["eta"])
    assert torch.equal(x0, ref)
    assert close(x0, g["gd_loop_x0"], 1e-4)


class MeanDenoiser(torch.nn.Module):
    def __init__(self, mean_fn):
        super().__init__()
        self.mean_fn = mean_fn
        from azula_amd.noise import VPSchedule

        self.schedule = VPSchedule()

    def forward(self, x_t, t, **kwargs):
        from azula_amd.denoise import DiracPosterior

        return DiracPosterior(mean=self.mean_fn(x_t, t, **kwargs))


def unet_mean(g):
    cfg = g.meta["unet_cfg"]
    sd = synth.synth_state_dict({k: tuple(v) for k, v in g.meta["unet_shapes"].items()}, g.meta["unet_weight_seed"])
    return lambda x, t: sampling.karras_mean(lambda a, c: nets.time_wrapped_unet(sd, cfg, a, c), x, t)  # noqa: E731


def test_host_jfps_equals_the_restatement_and_g27(golden):
    from azula_amd.guidance import JFPSDenoiser
    from azula_amd.linalg import covariance as cv

    g = golden(G)
    omean = unet_mean(g)
    x_t, t, y, mask = g["jf_x_t"], g["jf_t"], g["jf_y"], g["jf_mask"]
    A = lambda x: x * mask  # noqa: E731
    mean = omean(x_t, t)
    alpha_t, sigma_t = sampling.vp_schedule(t)
    tags = [c for c in g.meta["cases"] if c.startswith("jf_")]
    assert len(tags) == 8
    for tag in tags:
        kw = g.meta["cases"][tag]
        cls = tag.split("_")[1]
        cov_x = rebuild(g, f"jf_{cls}__f_", kw["factors"])
        jf = JFPSDenoiser(MeanDenoiser(omean), y, A, cv.IsotropicCovariance(0.05), cov_x, solver=kw["solver"],
                          iterations=kw["iterations"])
        out = jf(x_t, t).mean
        ref = co.jfps_mean(mean, alpha_t, sigma_t, y, A, co.iso(0.05), as_dict(cov_x), kw["solver"], kw["iterations"])
        assert torch.equal(out, ref), tag
        assert close(out, g[tag], 1e-4), (tag, max_err(out, g[tag]))


def test_host_ddim_loop_with_jfps(golden):
    from azula_amd.guidance import JFPSDenoiser
    from azula_amd.linalg import covariance as cv
    from azula_amd.sample import DDIMSampler

    g = golden(G)
    lp = g.meta["jf_loop"]
    omean = unet_mean(g)
    mask = g["jf_mask"]
    A = lambda x: x * mask  # noqa: E731
    cov_x = cv.DiagonalCovariance(g["jf_DiagonalCovariance__f_D"])
    jf = JFPSDenoiser(MeanDenoiser(omean), g["jf_y"], A, cv.IsotropicCovariance(0.05), cov_x, solver=lp["solver"],
                      iterations=lp["iterations"])
    torch.manual_seed(lp["seed"])
    x0 = DDIMSampler(jf, steps=lp["steps"], eta=lp["eta"], silent=True)(g["jf_loop_x1"])
    torch.manual_seed(lp["seed"])
    ref = sampling.sample(co.jfps_fn(omean, g["jf_y"], A, co.iso(0.05), as_dict(cov_x), solver=lp["solver"],
                                     iterations=lp["iterations"]), g["jf_loop_x1"], steps=lp["steps"], eta=lp["eta"])
    assert torch.equal(x0, ref)
    assert close(x0, g["jf_loop_x0"], 1e-4)


# ------------------------------------------------------------------------------------ the kernel tests' cases (covariance_cases.py)
ALL_CASES = [c for cases in cc.CASES.values() for c in cases]
DOT_CASES = cc.PROJECT_CASES + cc.EXPAND_CASES + cc.MODE_CASES


def test_case_lists_reach_every_tile_constant():
    r"""Just below, on and just above: 64 features, 64 rank columns, 32 rows, 512 per segment, inner = 64, the grid caps."""
    def values(cases, field):
        return {getattr(c, field) for c in cases}

    assert values(cc.PROJECT_CASES, "n") >= {1, 63, 64, 65, 511, 512, 513, 1100}
    assert values(cc.PROJECT_CASES, "r") >= {1, 63, 64, 65, 130} and values(cc.PROJECT_CASES, "rows") >= {1, 31, 32, 33, 70}
    assert values(cc.PROJECT_CASES, "c") == {0, 1}
    assert any(c.n % cc.SEG % cc.TILE and c.n > cc.SEG for c in cc.PROJECT_CASES)  # a ragged tile inside a later segment
    assert values(cc.EXPAND_CASES, "n") >= {1, 63, 64, 65, 130} and values(cc.EXPAND_CASES, "r") >= {1, 64, 65, 200}
    assert values(cc.EXPAND_CASES, "rows") >= {1, 32, 33, 70} and values(cc.EXPAND_CASES, "x") == {"none", "d", "d0"}
    assert values(cc.EXPAND_CASES, "a") == {0, 1} == values(cc.EXPAND_CASES, "g") and values(cc.EXPAND_CASES, "s") == {1, -1}
    assert values(cc.MODE_CASES, "n") >= {1, 5, 63, 64, 65, 100, 130} and values(cc.MODE_CASES, "inner") >= {1, 7, 63, 64, 70}
    assert values(cc.MODE_CASES, "outer") >= {1, 3, 10} and values(cc.MODE_CASES, "transpose") == {0, 1}
    ragged = [c for c in cc.MODE_CASES if (c.outer * c.inner) % cc.TILE]
    assert any(c.inner >= 64 for c in ragged) and any(c.inner < 64 and c.outer * c.inner > cc.TILE for c in ragged)
    assert any(64 < c.n < 128 for c in cc.MODE_CASES)
    pairs = {("f32", "f32"), ("f64", "f64"), ("f32", "f64"), ("f64", "f32")}
    for cases in (cc.PROJECT_CASES, cc.EXPAND_CASES, cc.MODE_CASES):
        assert {(c.xd, c.fd) for c in cases} == pairs
    s = cc.SCALE_CASES
    assert values(s, "h") == {0, 1, 2, 3} and values(s, "e") == {"n", "1", "none"} and values(s, "n") >= {1, 255, 256, 257}
    assert values(s, "u") == {0, 1} == values(s, "v") == values(s, "alias") and values(s, "k") == {"one", "host", "dev"}
    assert values(s, "rho") == {"host", "dev"} and any(c.sd == "f64" and c.xd == "f32" and c.k == "dev" for c in s)
    assert any(c.rows == 65535 + 2 and c.n == 3 for c in s) and cc.STRIDE_X_N == 256 * 65536 + 5
    assert all(not c.alias or cc.DT[c.xd] == cc.out_dtype(c) for c in s)
    assert len({cc.case_id(c) for c in ALL_CASES}) == len(ALL_CASES)


@pytest.mark.parametrize("case", ALL_CASES, ids=cc.case_id)
def test_exact_family_is_exact_in_fp32(case):
    r"""Every intermediate any evaluation order could form is bounded by the sum of absolute values: below 2^24, so fp32 is
    exact, and torch's fp32 evaluation equals the integer reference."""
    inp = cc.inputs(case, "exact")
    if isinstance(case, cc.Scale):
        ref, B = cc.scale_ref(inp, case, np.float64, want_bound=True)
        assert B.max() < 2.0 ** 24 and np.isfinite(ref).all()
        assert (ref * 4 == np.round(ref * 4)).all()  # quarters at the finest (e / (e + rho) = 3 / 4)
    else:
        ref = cc.reference(case, inp, dt=np.float64)
        assert cc.magnitude(case, inp).max() < 2.0 ** 24
        assert (ref == np.round(ref)).all() and np.abs(ref).max() > 0
        assert np.array_equal(cc.reference(case, inp).astype(np.float64), ref)
    got = cc.torch_eval(case, inp, torch.float32)
    assert got.dtype == torch.float32 and torch.equal(got.double(), torch.from_numpy(ref))
    for name in ("W", "Q"):
        if name in inp:
            F = inp[name]
            assert (F[-1] != 0).all() and (F[:, -1] != 0).all() and F[0, 0] != 0 and F.abs().max() <= 3
            assert F.shape[0] != F.shape[1] or F.shape[0] < 3 or not torch.equal(F, F.T)
            if min(F.shape) >= 8:  # no two rows and no two columns alike
                assert len({tuple(r.tolist()) for r in F}) == F.shape[0] and len({tuple(r.tolist()) for r in F.T}) == F.shape[1]


@pytest.mark.parametrize("case", DOT_CASES, ids=cc.case_id)
def test_planted_faults_change_the_exact_reference(case):
    inp = cc.inputs(case, "exact")
    ref = cc.reference(case, inp, dt=np.float64)
    for fault in cc.FAULTS:
        if cc.fault_applies(case, fault):
            bad = cc.reference(case, inp, fault=fault, dt=np.float64)
            assert bad.shape == ref.shape and not np.array_equal(bad, ref), fault


def test_every_fault_occurs_in_every_entry_it_exists_for():
    for cases in (cc.PROJECT_CASES, cc.EXPAND_CASES, cc.MODE_CASES):
        for fault in cc.FAULTS:
            n = sum(cc.fault_applies(c, fault) for c in cases)
            assert n >= 2 or (fault == "segment_twice" and cases is not cc.PROJECT_CASES), (fault, n)


def test_project_partials_sum_to_the_projection():
    for case in cc.PROJECT_CASES:
        inp = cc.inputs(case, "exact")
        parts = cc.project_partials(inp)
        assert parts.shape == (cc.segments(case.n), case.rows, case.r)
        assert np.array_equal(parts.sum(0), cc.reference(case, inp, dt=np.float64))


@pytest.mark.parametrize("case", ALL_CASES, ids=cc.case_id)
def test_hard_family_bound_holds_for_torch(case):
    r"""torch's own evaluation in the output dtype (fp32 wherever the operands are stored in fp32) is inside the derived bound: a
    bound that the plain evaluation cannot meet would show here."""
    inp = cc.inputs(case, "hard")
    ref, allowed, dtype = cc.reference(case, inp), cc.bound(case, inp), cc.out_dtype(case)
    assert np.isfinite(ref.astype(np.float64)).all() and (allowed >= 0).all()
    ratio, err = cc.worst_ratio(cc.torch_eval(case, inp, dtype), ref, allowed)
    print(f"COV host {cc.case_id(case)}: err {err:.3e} ratio {ratio:.4f}")
    assert ratio <= 1.0, (err, ratio)


def test_hard_family_spans_three_decades_and_the_bound_can_fail():
    case = cc.Project(1100, 130, 70, 1, "f32", "f32")
    inp = cc.inputs(case, "hard")
    W = inp["W"].abs()
    assert W.max() / W.min() > 500 and (inp["W"] < 0).any() and (inp["W"] > 0).any()
    assert inp["x"].double().mean(1).abs().max() > 3  # the rows' offsets
    ref, allowed = cc.reference(case, inp), cc.bound(case, inp)
    half = cc.torch_eval(case, {k: (v.bfloat16().float() if torch.is_tensor(v) else v) for k, v in inp.items()}, torch.float32)
    assert cc.worst_ratio(half, ref, allowed)[0] > 1.0  # operands rounded to 8 bits are outside it
    bad = torch.from_numpy(cc.reference(case, inp, fault="last_feature").astype(np.float64)).float()
    assert cc.worst_ratio(bad, ref, allowed)[0] > 1.0
    assert cc.roundings(case) == (512 + 3, 1) and cc.roundings(cc.Expand(65, 200, 70, "d", 1, 1, -1, "f32", "f32")) == (200, 4)
    assert cc.roundings(cc.Mode(130, 7, 3, 1, "f64", "f32")) == (130, 0)
