r"""Write ``tests/golden/g27_covariance.npz``: the reference's covariances, ``GaussianDenoiser`` and ``JFPSDenoiser`` -- TEST
INFRASTRUCTURE.

    python tools/make_golden_covariance.py

Like ``oracle/make_golden.py`` (whose helpers it imports) it needs the reference checkout, so it runs in the build container
only.  For every case it (1) runs the reference, (2) runs the restatement of ``tests/covariance_oracle.py`` on the same inputs
and asserts that both are bit-identical, (3) stores the inputs and the reference's output.  Network weights are not stored:
they are regenerated from the stored parameter shapes by ``oracle.synth``.

Covariance cases (``cov_<class>_<source>_<shape>_<dtype>``): every class from fixed factors on shapes (5,), (3, 5), (3, 8, 8)
(Full only on the first two) and from ``from_data`` on (5,), (3, 5) (DPLR: PCA, EM and the ``eigh`` branch; Kronecker: Diagonal
and DPLR cores), in fp32 and fp64.  Recorded: ``@``, ``inv @``, ``inv.inv @`` and ``color`` on batches (), (4,), (2, 3)
(the (3, 8, 8) shape: fp64 and (2, 3) only, to keep the file small), ``logdet``, and ``@`` of the algebra results (``+ Isotropic``,
``Diagonal +``, ``* Isotropic``, ``cov + cov`` for the low-rank classes).  ``from_data`` runs under ``torch.manual_seed(0)``
(``lobpcg`` draws its start).  GaussianDenoiser at t in {0.05, 0.5, 0.99} per spectral and low-rank class, and one DDIM-8
loop; JFPS on G26's small UNet with Isotropic, Diagonal, DPLR and Kronecker ``cov_x``, cg and gmres, and one DDIM-8 loop.
"""

from __future__ import annotations

import inspect
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from oracle import make_golden as mg  # noqa: E402  (puts the reference on sys.path)
from oracle import nets, sampling  # noqa: E402

import azula.linalg.covariance as R  # noqa: E402  (the reference)
from azula.denoise import GaussianDenoiser, KarrasDenoiser  # noqa: E402
from azula.guidance.jfps import JFPSDenoiser  # noqa: E402
from azula.noise import VPSchedule  # noqa: E402
from azula.sample import DDIMSampler  # noqa: E402

import covariance_oracle as co  # noqa: E402

torch.set_grad_enabled(False)
CLASSES = ["IsotropicCovariance", "DiagonalCovariance", "FullCovariance", "DPLRCovariance", "DMLRCovariance", "KroneckerCovariance"]


def signature() -> list:
    out = []
    fns = [getattr(R, c).__init__ for c in CLASSES] + [GaussianDenoiser.__init__, JFPSDenoiser.__init__]
    fns += [R.DPLRCovariance.from_data, R.KroneckerCovariance.from_data]
    for fn in fns:
        for p in list(inspect.signature(fn).parameters.values()):
            if p.name == "self":
                continue
            default = None if p.default is inspect.Parameter.empty else repr(p.default)
            out.append([fn.__qualname__, p.name, p.kind.name, default])
    return out


def as_dict(c) -> dict:
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


def factors(c, prefix: str, arrays: dict) -> dict:
    r"""The factor tensors of ``c`` under ``prefix``; returns the description the tests rebuild it from."""
    n = type(c).__name__
    if n == "IsotropicCovariance":
        arrays[prefix + "lmbda"] = c.lmbda
        return {"cls": n}
    if n == "KroneckerCovariance":
        for i, Q in enumerate(c.Qs):
            arrays[f"{prefix}Q{i}"] = Q
        return {"cls": n, "axes": len(c.Qs), "L": factors(c.L, prefix + "L_", arrays)}
    for k in ("D", "Q", "L", "V"):
        if k in c.__dict__:
            arrays[prefix + k] = c.__dict__[k]
    return {"cls": n}


def fixed(cls: str, shape, dtype, g) -> object:
    n = 1
    for s in shape:
        n *= s
    D = (0.5 + torch.rand(shape, generator=g, dtype=torch.float64)).to(dtype)
    orth = lambda m: torch.linalg.qr(torch.randn(m, m, generator=g, dtype=torch.float64))[0].contiguous().to(dtype)  # noqa: E731
    if cls == "IsotropicCovariance":
        return R.IsotropicCovariance(torch.tensor(1.7, dtype=dtype))
    if cls == "DiagonalCovariance":
        return R.DiagonalCovariance(D)
    if cls == "FullCovariance":
        return R.FullCovariance(orth(n).reshape(*shape, n), (0.5 + torch.rand(n, generator=g, dtype=torch.float64)).to(dtype))
    if cls in ("DPLRCovariance", "DMLRCovariance"):
        V = (torch.randn(*shape, 3, generator=g, dtype=torch.float64) * (0.3 / n**0.5)).to(dtype)
        return getattr(R, cls)(D + (1.0 if cls == "DMLRCovariance" else 0.0), V)
    return R.KroneckerCovariance([orth(m) for m in shape], R.DiagonalCovariance(D))


def from_data(variant: str, X):
    torch.manual_seed(0)
    return {
        "IsotropicCovariance": lambda: R.IsotropicCovariance.from_data(X),
        "DiagonalCovariance": lambda: R.DiagonalCovariance.from_data(X),
        "FullCovariance": lambda: R.FullCovariance.from_data(X),
        "DPLRCovariance_pca": lambda: R.DPLRCovariance.from_data(X, rank=1),
        "DPLRCovariance_em": lambda: R.DPLRCovariance.from_data(X, rank=1, iterations=3),
        "DPLRCovariance_eigh": lambda: R.DPLRCovariance.from_data(X, rank=2),
        "KroneckerCovariance": lambda: R.KroneckerCovariance.from_data(X),
        "KroneckerCovariance_dplr": lambda: R.KroneckerCovariance.from_data(X, rank=1, iterations=2),
    }[variant]()


def record(tag: str, c, shape, dtype, xs: dict, arrays: dict, cases: dict, desc: dict, lowrank: bool) -> None:
    cd = as_dict(c)
    outs = {}
    for bt, x in xs.items():
        outs[f"{bt}_matmul"] = (c @ x, co.apply(cd, x))
        outs[f"{bt}_inv"] = (c.inv @ x, co.apply(co.inv(cd), x))
        outs[f"{bt}_invinv"] = (c.inv.inv @ x, co.apply(co.inv(co.inv(cd)), x))
        outs[f"{bt}_color"] = (c.color(x), co.color(cd, x))
    x = next(iter(xs.values()))
    iso3, dg = R.IsotropicCovariance(torch.tensor(0.3, dtype=dtype)), R.DiagonalCovariance(torch.full(shape, 0.2, dtype=dtype))
    outs["alg_add_iso"] = ((c + iso3) @ x, co.apply(co.add(cd, co.iso(iso3.lmbda)), x))
    outs["alg_mul_iso"] = ((c * R.IsotropicCovariance(torch.tensor(2.0, dtype=dtype))) @ x,
                           co.apply(co.mul(cd, co.iso(torch.tensor(2.0, dtype=dtype))), x))
    if type(c).__name__ not in ("FullCovariance", "KroneckerCovariance"):
        outs["alg_diag_add"] = ((dg + c) @ x, co.apply(co.add(co.diag(dg.D), cd), x))
    if lowrank:
        outs["alg_self_add"] = ((c + c) @ x, co.apply(co.add(cd, cd), x))
    if type(c).__name__ != "IsotropicCovariance":
        outs["logdet"] = (c.logdet(), co.logdet(cd))
    for k, (ref, mine) in outs.items():
        mg.same(ref, mine, f"{tag} {k}")
        arrays[f"{tag}__{k}"] = ref
    cases[tag] = dict(desc, shape=list(shape), dtype=str(dtype), batches=list(xs), outputs=sorted(outs))


def covariance_cases(arrays: dict, cases: dict) -> None:
    g = torch.Generator().manual_seed(27)
    for dtype in (torch.float64, torch.float32):
        dn = str(dtype)[6:]
        for shape in ((5,), (3, 5), (3, 8, 8)) if dtype == torch.float64 else ((5,), (3, 5)):
            st = "x".join(map(str, shape))
            batches = {"b0": (), "b4": (4,), "b23": (2, 3)} if len(shape) < 3 else {"b23": (2, 3)}
            xs = {}
            for bt, b in batches.items():
                xs[bt] = torch.randn(*b, *shape, generator=g, dtype=torch.float64).to(dtype)
                arrays[f"x_{st}_{dn}_{bt}"] = xs[bt]
            for cls in CLASSES:
                if cls == "FullCovariance" and len(shape) == 3:
                    continue
                c = fixed(cls, shape, dtype, g)
                tag = f"cov_{cls}_fixed_{st}_{dn}"
                desc = dict(source="fixed", factors=factors(c, tag + "__f_", arrays))
                record(tag, c, shape, dtype, xs, arrays, cases, desc, "LR" in cls)
            if len(shape) == 3:
                continue
            X = (torch.randn(40, *shape, generator=g, dtype=torch.float64) * (1 + torch.rand(shape, generator=g,
                                                                                             dtype=torch.float64))).to(dtype)
            arrays[f"X_{st}_{dn}"] = X
            for variant in ("IsotropicCovariance", "DiagonalCovariance", "FullCovariance", "DPLRCovariance_pca", "DPLRCovariance_em",
                            "DPLRCovariance_eigh", "KroneckerCovariance", "KroneckerCovariance_dplr"):
                if variant.startswith("DPLR") and shape == (5,) and variant.endswith("eigh"):
                    continue
                if variant == "KroneckerCovariance_dplr" and len(shape) < 2:
                    continue
                c = from_data(variant, X)
                tag = f"cov_{variant}_data_{st}_{dn}"
                record(tag, c, shape, dtype, xs, arrays, cases, dict(source="data", variant=variant), "DPLR" in variant)


def gaussian_cases(arrays: dict, cases: dict, meta: dict) -> None:
    g = torch.Generator().manual_seed(127)
    shape = (3, 5)
    for dtype in (torch.float64, torch.float32):
        dn = str(dtype)[6:]
        mean = torch.randn(shape, generator=g, dtype=torch.float64).to(dtype)
        x = torch.randn(4, *shape, generator=g, dtype=torch.float64).to(dtype)
        arrays[f"gd_mean_{dn}"], arrays[f"gd_x_{dn}"] = mean, x
        for cls in ("IsotropicCovariance", "DiagonalCovariance", "FullCovariance", "DPLRCovariance", "KroneckerCovariance"):
            c = fixed(cls, shape, dtype, g)
            ctag = f"gd_{cls}_{dn}"
            desc = factors(c, ctag + "__f_", arrays)
            for t in (0.05, 0.5, 0.99):
                tt = torch.tensor(t, dtype=dtype)
                ref = GaussianDenoiser(mean, c, VPSchedule())(x, tt).mean
                a, s = VPSchedule()(tt)
                mg.same(ref, co.gaussian_mean(mean, as_dict(c), x, a, s), f"{ctag} t={t}")
                arrays[f"{ctag}_t{t}"] = ref
            cases[ctag] = dict(factors=desc, dtype=dn, times=[0.05, 0.5, 0.99])
    # one DDIM-8 loop (eta = 0.5) over the fp32 Diagonal prior
    c = R.DiagonalCovariance(arrays["gd_DiagonalCovariance_float32__f_D"])
    mean = arrays["gd_mean_float32"]
    torch.manual_seed(1)
    x1 = DDIMSampler(GaussianDenoiser(mean, c, VPSchedule()), steps=8, silent=True).init((2, *shape))
    torch.manual_seed(2)
    x0 = DDIMSampler(GaussianDenoiser(mean, c, VPSchedule()), steps=8, eta=0.5, silent=True)(x1)
    torch.manual_seed(2)
    ox0 = sampling.sample(co.gaussian_fn(mean, as_dict(c)), x1, steps=8, eta=0.5)
    mg.same(x0, ox0, "gaussian ddim8")
    arrays.update({"gd_loop_x1": x1, "gd_loop_x0": x0})
    meta["gd_loop"] = dict(steps=8, eta=0.5, seed=2, cls="DiagonalCovariance", dtype="float32")


def jfps_cases(arrays: dict, cases: dict, meta: dict) -> None:
    cfg = mg.UNET_CFGS["unet_group"]
    wrapped = mg.TimeWrapped(mg.make_unet(cfg), "unet", cfg["mod_features"]).eval()
    meta["unet_shapes"] = mg.load_synth(wrapped, seed=6)
    meta["unet_cfg"], meta["unet_weight_seed"] = cfg, 6
    usd = {k: v.clone() for k, v in wrapped.state_dict().items()}
    den = KarrasDenoiser(wrapped, VPSchedule()).eval()
    omean = lambda x, t: sampling.karras_mean(lambda a, c: nets.time_wrapped_unet(usd, cfg, a, c), x, t)  # noqa: E731
    g = torch.Generator().manual_seed(227)
    shape = (3, 8, 8)
    mask = (torch.rand(1, 1, 8, 8, generator=g) < 0.5).float()
    A = lambda x: x * mask  # noqa: E731
    x_t = torch.randn(1, *shape, generator=g)
    t = torch.tensor(0.6)
    y = A(torch.randn(1, *shape, generator=g))
    arrays.update({"jf_mask": mask, "jf_x_t": x_t, "jf_t": t, "jf_y": y})
    cov_y = R.IsotropicCovariance(0.05)
    alpha_t, sigma_t = sampling.vp_schedule(t)
    mean = omean(x_t, t)
    for cls in ("IsotropicCovariance", "DiagonalCovariance", "DPLRCovariance", "KroneckerCovariance"):
        c = fixed(cls, shape, torch.float32, g)
        desc = factors(c, f"jf_{cls}__f_", arrays)
        for solver in ("cg", "gmres"):
            tag = f"jf_{cls}_{solver}"
            ref = JFPSDenoiser(den, y, A, cov_y, c, solver=solver, iterations=3)(x_t, t).mean
            mine = co.jfps_mean(mean, alpha_t, sigma_t, y, A, co.iso(0.05), as_dict(c), solver, 3)
            mg.same(ref, mine, tag)
            arrays[tag] = ref
            cases[tag] = dict(factors=desc, solver=solver, iterations=3)
    c = R.DiagonalCovariance(arrays["jf_DiagonalCovariance__f_D"])
    torch.manual_seed(1)
    x1 = DDIMSampler(den, steps=8, silent=True).init((1, *shape))
    torch.manual_seed(2)
    x0 = DDIMSampler(JFPSDenoiser(den, y, A, cov_y, c, solver="gmres", iterations=2), steps=8, eta=0.5, silent=True)(x1)
    torch.manual_seed(2)
    ox0 = sampling.sample(co.jfps_fn(omean, y, A, co.iso(0.05), as_dict(c), solver="gmres", iterations=2), x1, steps=8, eta=0.5)
    mg.same(x0, ox0, "jfps ddim8")
    arrays.update({"jf_loop_x1": x1, "jf_loop_x0": x0})
    meta["jf_loop"] = dict(steps=8, eta=0.5, seed=2, solver="gmres", iterations=2, cls="DiagonalCovariance")


def main() -> None:
    arrays, cases, meta = {}, {}, {}
    covariance_cases(arrays, cases)
    gaussian_cases(arrays, cases, meta)
    jfps_cases(arrays, cases, meta)
    meta.update({"cases": cases, "signature": signature()})
    mg.save("g27_covariance", meta, **arrays)


if __name__ == "__main__":
    main()
