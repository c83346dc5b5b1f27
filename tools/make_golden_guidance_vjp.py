r"""Write ``tests/golden/g28_guidance_vjp.npz``: the reference's DPS / PGDM / TMPD / MMPS -- TEST INFRASTRUCTURE.

    python tools/make_golden_guidance_vjp.py

Like ``tools/make_golden_diffpir.py`` it needs the reference checkout.  On the small G5 UNet (``unet_group`` config, batch 2,
3 x 16 x 16) behind a ``KarrasDenoiser`` it (1) runs the reference's classes, (2) runs the restatement of
``tests/guidance_vjp_oracle.py`` on the same inputs and asserts that both are bit-identical, (3) stores the inputs, the noise
lists and the reference's outputs, and (4) per quantity ``e_ref``: the reference's fp32 result against the restatement run
in fp64 on the same inputs, relative to the largest magnitude of the fp64 result.  Operators: a pixel mask and a 2x average
pooling, observations flattened to (B, D).  The observation variance is 1: with the synthetic weights the network's Jacobian
is not positive semi-definite, and ``cov_y + A gamma_t J^T A^T`` has to be positive definite for the reference's own ``cg`` to be
defined (``azula/linalg/solve.py:23-24``; at var_y = 0.05 its third iteration overflows to NaN in the reference itself, in
fp32 and in fp64).  Network weights are regenerated from the stored shapes by ``oracle.synth``.
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
from azula.guidance.dps import DPSSampler  # noqa: E402
from azula.guidance.mmps import MMPSDenoiser  # noqa: E402
from azula.guidance.pgdm import PGDMSampler  # noqa: E402
from azula.guidance.tmpd import TMPDenoiser  # noqa: E402
from azula.linalg.covariance import IsotropicCovariance  # noqa: E402
from azula.noise import VPSchedule  # noqa: E402

import guidance_vjp_oracle as go  # noqa: E402

STEPS, VAR_Y = 8, 1.0


def signature() -> list:
    out = []
    for cls in (DPSSampler, PGDMSampler, TMPDenoiser, MMPSDenoiser):
        for p in list(inspect.signature(cls.__init__).parameters.values())[1:]:
            out.append([cls.__name__, p.name, p.kind.name, None if p.default is inspect.Parameter.empty else repr(p.default)])
    return out


def rel(a: torch.Tensor, ref: torch.Tensor) -> float:
    return float((a.double() - ref).abs().max() / ref.abs().max())


def main() -> None:
    cfg = mg.UNET_CFGS["unet_group"]
    wrapped = mg.TimeWrapped(mg.make_unet(cfg), "unet", cfg["mod_features"]).eval()
    meta = {"unet_shapes": mg.load_synth(wrapped, seed=6), "unet_cfg": cfg, "unet_weight_seed": 6, "steps": STEPS, "var_y": VAR_Y}
    usd = {k: v.clone() for k, v in wrapped.state_dict().items()}
    usd64 = {k: v.double() for k, v in usd.items()}
    den = KarrasDenoiser(wrapped, VPSchedule()).eval()
    omean = lambda x, t: sampling.karras_mean(lambda a, c: nets.time_wrapped_unet(usd, cfg, a, c), x, t)  # noqa: E731
    omean64 = lambda x, t: sampling.karras_mean(lambda a, c: nets.time_wrapped_unet(usd64, cfg, a, c), x, t, backbone_dtype=torch.float64)  # noqa: E731

    g = torch.Generator().manual_seed(128)
    B, H, W = 2, 16, 16
    truth = torch.randn(B, 3, H, W, generator=g)
    mask = (torch.rand(1, 1, H, W, generator=g) < 0.4).float()
    ops = {"mask": go.mask_op(mask), "pool": go.pool_op(H, W)}
    t, s = torch.tensor(0.6), torch.tensor(0.5)
    x_t = 0.8 * truth + 0.6 * torch.randn(B, 3, H, W, generator=g)
    x1 = torch.randn(B, 3, H, W, generator=g)
    eps = torch.randn(STEPS, B, 3, H, W, generator=g)
    arrays = {"mask": mask, "x_t": x_t, "t": t, "s": s, "x1": x1, "eps": eps}
    e_ref: dict = {}
    d = lambda v: v.double() if torch.is_tensor(v) and v.is_floating_point() else v  # noqa: E731

    def record(tag: str, ref: torch.Tensor, mine: torch.Tensor, wide: torch.Tensor) -> None:
        mg.same(ref, mine, tag)
        arrays[tag] = ref
        e_ref[tag] = rel(ref, wide)
        print(f"{tag}: e_ref {e_ref[tag]:.3e}")

    class Fed:  # the reference's randn_like, fed from the stored list
        def __init__(self, seq):
            self.seq, self.k = seq, 0

        def __call__(self, like):
            self.k += 1
            return self.seq[self.k - 1].to(like)

    for name, (A, A_inv) in ops.items():
        y = A(truth) + VAR_Y**0.5 * torch.randn(A(truth).shape, generator=g)
        arrays[f"{name}_y"] = y
        for zeta in (1.0, 0.3):
            kw = dict(y=y, A=A, zeta=zeta)
            smp = DPSSampler(den, y, A, zeta=zeta, steps=STEPS, silent=True)
            torch.randn_like, keep = Fed(eps), torch.randn_like
            try:
                one = smp.step(x_t, t, s)
                torch.randn_like = Fed(eps)
                full = smp(x1) if zeta == 1.0 else None
            finally:
                torch.randn_like = keep
            record(f"dps_{name}_zeta{zeta}_step", one, go.dps_step(omean, x_t, t, s, eps[0], **kw),
                   go.dps_step(omean64, d(x_t), d(t), d(s), d(eps[0]), y=d(y), A=A, zeta=zeta))
            if full is not None:
                record(f"dps_{name}_loop", full, go.loop(lambda **a: go.dps_step(omean, **a, **kw), x1, list(eps), STEPS),
                       go.loop(lambda **a: go.dps_step(omean64, **a, y=d(y), A=A, zeta=zeta), d(x1), list(d(eps)), STEPS))
        for eta in (0.0, 0.5):
            kw = dict(y=y, A=A, A_inv=A_inv, eta=eta)
            smp = PGDMSampler(den, y, A, A_inv, eta=eta, steps=STEPS, silent=True)
            torch.randn_like, keep = Fed(eps), torch.randn_like
            try:
                one = smp.step(x_t, t, s)
                torch.randn_like = Fed(eps)
                full = smp(x1) if eta == 0.0 else None
            finally:
                torch.randn_like = keep
            record(f"pgdm_{name}_eta{eta}_step", one, go.pgdm_step(omean, x_t, t, s, eps[0], **kw),
                   go.pgdm_step(omean64, d(x_t), d(t), d(s), d(eps[0]), y=d(y), A=A, A_inv=A_inv, eta=eta))
            if full is not None:
                record(f"pgdm_{name}_loop", full, go.loop(lambda **a: go.pgdm_step(omean, **a, **kw), x1, list(eps), STEPS),
                       go.loop(lambda **a: go.pgdm_step(omean64, **a, y=d(y), A=A, A_inv=A_inv, eta=eta), d(x1), list(d(eps)), STEPS))
        record(f"tmpd_{name}", TMPDenoiser(den, y, A, VAR_Y)(x_t, t).mean, go.tmpd_mean(omean, x_t, t, y, A, VAR_Y),
               go.tmpd_mean(omean64, d(x_t), d(t), d(y), A, VAR_Y))
        cov = IsotropicCovariance(torch.tensor(VAR_Y))
        for solver in ("cg", "gmres"):
            for it in (1, 3):
                record(f"mmps_{name}_{solver}_it{it}", MMPSDenoiser(den, y, A, cov, solver=solver, iterations=it)(x_t, t).mean,
                       go.mmps_mean(omean, x_t, t, y, A, lambda v: VAR_Y * v, solver, it),
                       go.mmps_mean(omean64, d(x_t), d(t), d(y), A, lambda v: VAR_Y * v, solver, it))
    meta.update({"e_ref": e_ref, "signature": signature()})
    mg.save("g28_guidance_vjp", meta, **arrays)


if __name__ == "__main__":
    main()
