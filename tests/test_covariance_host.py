r"""``azula_amd.linalg.covariance``, ``GaussianDenoiser`` and ``JFPSDenoiser`` without a GPU: the public API against the
reference's recorded signatures; host applies, ``inv``, ``color``, ``logdet``, the algebra and both denoisers against the
restatement of ``tests/covariance_oracle.py`` (independent of ``azula_amd``) bit for bit and against fixture G27 within the
round-off of another CPU; the covariance identities in fp64 for every ``from_data`` variant; the algebra's dispatch rules;
JFPS's public surface; and the C ABI of the covariance entries."""

import ctypes
import inspect
import math
import os
import subprocess
import tempfile

import pytest
import torch

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
