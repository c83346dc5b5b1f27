r"""Write ``tests/golden/g26_diffpir.npz``: the reference's ``cg`` / ``gmres`` and ``DiffPIRDenoiser`` -- TEST INFRASTRUCTURE.

    python tools/make_golden_diffpir.py

Like ``oracle/make_golden.py`` (whose helpers it imports) it needs the reference checkout, so it runs in the build
container only.  For every case it (1) runs the reference, (2) runs the restatement of ``tests/diffpir_oracle.py`` on the
same inputs and asserts that both are bit-identical, (3) stores the inputs and the reference's output.  Network weights are
not stored: they are regenerated from the stored parameter shapes by ``oracle.synth``.

Solver cases (``solve_<op>_<solver>_b<batch>_<x0>_it<n>_<dtype>``): rows of D = 8; ``spd`` is x -> x S^T with S symmetric
positive semi-definite of rank 3, ``nonsym`` is x -> x N^T with N = U C U^T non-symmetric of rank 3; b lies in their range,
so three iterations solve exactly.  DiffPIR cases (``dp_<op>_<solver>_it<n>_<var>``) on the small UNet of G25 (one image
3 x 8 x 8) at t = 0.6: a pixel mask, a 2x average-pool downsampling and a per-row matrix; and one DDIM-8 loop.
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

from azula.denoise import KarrasDenoiser  # noqa: E402  (the reference)
from azula.guidance.diffpir import DiffPIRDenoiser  # noqa: E402
from azula.linalg.solve import cg, gmres  # noqa: E402
from azula.noise import VPSchedule  # noqa: E402
from azula.sample import DDIMSampler  # noqa: E402

import diffpir_oracle as do  # noqa: E402

torch.set_grad_enabled(False)

D, RANK = 8, 3


def signature() -> list:
    out = []
    for fn in (DiffPIRDenoiser.__init__, cg, gmres):
        params = list(inspect.signature(fn).parameters.values())
        for p in params[1:] if fn is DiffPIRDenoiser.__init__ else params:
            default = None if p.default is inspect.Parameter.empty else repr(p.default)
            out.append([fn.__qualname__, p.name, p.kind.name, default])
    return out


def operators(g: torch.Generator) -> dict:
    U, _ = torch.linalg.qr(torch.randn(D, RANK, generator=g, dtype=torch.float64))
    S = U @ torch.diag(torch.tensor([3.0, 1.5, 0.5], dtype=torch.float64)) @ U.mT
    C = torch.randn(RANK, RANK, generator=g, dtype=torch.float64) + 2 * torch.eye(RANK, dtype=torch.float64)
    N = U @ C @ U.mT
    return {"spd": S.float(), "nonsym": N.float(), "range": U.float()}


def solver_cases(arrays: dict, cases: dict) -> None:
    g = torch.Generator().manual_seed(26)
    ops = operators(g)
    arrays.update({"op_spd": ops["spd"], "op_nonsym": ops["nonsym"]})
    for batch in ((), (64,)):
        coef = torch.randn(*batch, RANK, generator=g)
        b = coef @ ops["range"].mT  # in the range of both operators
        x0 = 0.1 * torch.randn(*batch, D, generator=g)
        tagb = f"b{batch[0] if batch else 0}"
        arrays[f"solve_{tagb}_b"], arrays[f"solve_{tagb}_x0"] = b, x0
        for op, solver in (("spd", "cg"), ("spd", "gmres"), ("nonsym", "gmres")):
            A = do.row_matrix(ops[op])
            ref, mine = {"cg": cg, "gmres": gmres}[solver], do.SOLVERS[solver]
            for with_x0 in (False, True):
                for it in (1, RANK):
                    for dtype in (torch.float64, torch.float32):
                        if batch and dtype == torch.float32 and (with_x0 or it != RANK):
                            continue  # (fp32 state on a batch: one case per operator keeps the fixture small)
                        tag = f"solve_{op}_{solver}_{tagb}_{'x0' if with_x0 else 'nox0'}_it{it}_{str(dtype)[6:]}"
                        kw = dict(x0=x0 if with_x0 else None, iterations=it, dtype=dtype)
                        out = ref(A, b, **kw)
                        mg.same(out, mine(A, b, **kw), tag)
                        arrays[tag] = out
                        cases[tag] = dict(op=op, solver=solver, batch=tagb, x0=with_x0, iterations=it, dtype=str(dtype))


def diffpir_cases(arrays: dict, cases: dict, meta: dict) -> None:
    cfg = mg.UNET_CFGS["unet_group"]
    wrapped = mg.TimeWrapped(mg.make_unet(cfg), "unet", cfg["mod_features"]).eval()
    meta["unet_shapes"] = mg.load_synth(wrapped, seed=6)
    meta["unet_cfg"], meta["unet_weight_seed"] = cfg, 6
    usd = {k: v.clone() for k, v in wrapped.state_dict().items()}
    den = KarrasDenoiser(wrapped, VPSchedule()).eval()
    omean = lambda x, t: sampling.karras_mean(lambda a, c: nets.time_wrapped_unet(usd, cfg, a, c), x, t)  # noqa: E731
    g = torch.Generator().manual_seed(126)
    truth = torch.randn(1, 3, 8, 8, generator=g)
    mask = (torch.rand(1, 1, 8, 8, generator=g) < 0.4).float()
    M = torch.randn(8, 8, generator=g) / 3
    ops = {"mask": do.pixel_mask(mask), "pool": do.avg_pool2, "rows": do.row_matrix(M)}
    arrays.update({"dp_truth": truth, "dp_mask": mask, "dp_rows": M})
    x_t = 0.8 * truth + 0.6 * torch.randn(1, 3, 8, 8, generator=g)
    t = torch.tensor(0.6)
    arrays.update({"dp_x_t": x_t, "dp_t": t})
    var_tensor = torch.tensor(0.05)
    for name, A in ops.items():
        clean = A(truth)
        y = clean + 0.05 * torch.randn(clean.shape, generator=g)
        arrays[f"dp_{name}_y"] = y
        for solver in ("cg", "gmres"):
            for it in (1, 4):
                for var in ("float", "tensor"):
                    if var == "tensor" and it != 1:
                        continue
                    var_y = 0.05 if var == "float" else var_tensor
                    tag = f"dp_{name}_{solver}_it{it}_{var}"
                    ref = DiffPIRDenoiser(den, y, A, var_y, lmbda=10.0, solver=solver, iterations=it)(x_t, t).mean
                    alpha_t, sigma_t = sampling.vp_schedule(t)
                    mine = do.diffpir_mean(omean(x_t, t), alpha_t, sigma_t, y, A, var_y, 10.0, solver, it)
                    mg.same(ref, mine, tag)
                    arrays[tag] = ref
                    cases[tag] = dict(op=name, solver=solver, iterations=it, var_y=var)

    # a DDIM-8 loop with DiffPIR (gmres, 2 iterations, the mask operator) on a batch of two
    y2 = ops["mask"](torch.randn(2, 3, 8, 8, generator=g))
    torch.manual_seed(1)
    x1 = DDIMSampler(den, steps=8, silent=True).init((2, 3, 8, 8))
    dp = DiffPIRDenoiser(den, y2, ops["mask"], 0.05, lmbda=10.0, solver="gmres", iterations=2)
    torch.manual_seed(2)
    x0 = DDIMSampler(dp, steps=8, eta=0.5, silent=True)(x1)
    torch.manual_seed(2)
    ox0 = sampling.sample(do.diffpir_fn(omean, y2, ops["mask"], 0.05, lmbda=10.0, solver="gmres", iterations=2), x1,
                          steps=8, eta=0.5)
    mg.same(x0, ox0, "ddim8 loop")
    arrays.update({"loop_y": y2, "loop_x1": x1, "loop_x0": x0})
    meta["loop"] = dict(steps=8, eta=0.5, solver="gmres", iterations=2, var_y=0.05, lmbda=10.0, op="mask", seed=2)


def main() -> None:
    arrays, cases, meta = {}, {}, {}
    solver_cases(arrays, cases)
    diffpir_cases(arrays, cases, meta)
    meta.update({"cases": cases, "signature": signature(), "D": D, "rank": RANK})
    mg.save("g26_diffpir", meta, **arrays)


if __name__ == "__main__":
    main()
