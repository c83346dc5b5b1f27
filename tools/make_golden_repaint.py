r"""Write ``tests/golden/g25_repaint.npz``: the reference's ``RePaintSampler`` on small denoisers -- TEST INFRASTRUCTURE.

    python tools/make_golden_repaint.py

Like ``oracle/make_golden.py`` (whose helpers it imports) it needs the reference checkout, so it runs in the build
container only.  For every case it (1) runs the reference sampler, (2) runs the restatement of ``tests/repaint_oracle.py`` on
the same inputs and seed and asserts that both the output and the generator state afterwards are bit-identical, (3) stores
inputs, output, the per-step 0-d scalars and one ``torch.randn(4)`` drawn after sampling (the generator state).  Network
weights are not stored: they are regenerated from the stored parameter shapes by ``oracle.synth``.
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
from azula.guidance.repaint import RePaintSampler  # noqa: E402
from azula.noise import VPSchedule  # noqa: E402
from azula.sample import DDIMSampler  # noqa: E402

import repaint_oracle  # noqa: E402

torch.set_grad_enabled(False)


def signature() -> list:
    r"""(name, kind, default) of the reference's constructor and of the DDIM / Sampler constructors its kwargs reach."""
    out = []
    for cls in (RePaintSampler, DDIMSampler, DDIMSampler.__mro__[1]):
        for p in list(inspect.signature(cls.__init__).parameters.values())[1:]:
            default = None if p.default is inspect.Parameter.empty else repr(p.default)
            out.append([cls.__name__, p.name, p.kind.name, default])
    return out


def run_case(tag: str, den, omean, x1: torch.Tensor, y: torch.Tensor, mask: torch.Tensor, arrays: dict, **kw) -> dict:
    dtype = kw.get("dtype")
    torch.manual_seed(2)
    x0 = RePaintSampler(den, y, mask, silent=True, **kw)(x1)
    after = torch.randn(4)
    torch.manual_seed(2)
    ox0 = repaint_oracle.sample_repaint(omean, x1, y, mask, steps=kw["steps"], iterations=kw.get("iterations", 3),
                                        eta=kw.get("eta", 0.0), dtype=dtype)
    mg.same(x0, ox0, tag)
    mg.same(after, torch.randn(4), tag + " generator state")
    sched = den.schedule
    ts = torch.linspace(1.0, 0.0, kw["steps"] + 1, dtype=dtype)
    ref_scalars = []
    for t, s in ts.unfold(0, 2, 1).unbind():  # the reference's 0-d values, its op order (repaint.py:48-49,55,59-61)
        alpha_s, sigma_s = sched(s)
        alpha_t, sigma_t = sched(t)
        ref_scalars.append(torch.stack([alpha_s, sigma_s, alpha_t / alpha_s,
                                        alpha_t * torch.sqrt((sigma_t / alpha_t) ** 2 - (sigma_s / alpha_s) ** 2)]))
    scalars = torch.stack(ref_scalars)
    mg.same(scalars, repaint_oracle.scalar_table(sched, steps=kw["steps"], dtype=dtype), tag + " scalars")
    arrays.update({f"{tag}_x1": x1, f"{tag}_y": y, f"{tag}_mask": mask, f"{tag}_x0": x0, f"{tag}_randn_after": after,
                   f"{tag}_scalars": scalars})
    return {k: (str(v) if isinstance(v, torch.dtype) else v) for k, v in kw.items()}


def main() -> None:
    arrays, cases = {}, {}

    # ToyMLP (the reference tests' backbone), batch 64 x 5 features
    net = mg.ToyMLP(5)
    toy_shapes = mg.load_synth(net, seed=4)
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    den = KarrasDenoiser(net, VPSchedule()).eval()
    omean = lambda x, t: sampling.karras_mean(mg.toy_oracle(sd), x, t)  # noqa: E731
    g = torch.Generator().manual_seed(25)
    truth = torch.randn(64, 5, generator=g)
    full = torch.rand(64, 5, generator=g) < 0.5
    bcast = torch.tensor([[True, False, True, True, False]])
    torch.manual_seed(1)
    x1 = DDIMSampler(den, steps=16, silent=True).init((64, 5))
    cases["toy_eta0_it3"] = run_case("toy_eta0_it3", den, omean, x1, truth * full, full, arrays, steps=16, iterations=3, eta=0.0)
    cases["toy_eta06_it2_bcast"] = run_case("toy_eta06_it2_bcast", den, omean, x1, truth * bcast, bcast, arrays, steps=16,
                                            iterations=2, eta=0.6)
    cases["toy_f64"] = run_case("toy_f64", den, omean, x1, truth * full, full, arrays, steps=16, iterations=2, eta=0.3,
                                dtype=torch.float64)
    assert arrays["toy_f64_x0"].dtype == torch.float64

    # the small UNet of G6 (2 x 3 x 16 x 16), a box of observed pixels shared by every image and channel
    cfg = mg.UNET_CFGS["unet_group"]
    wrapped = mg.TimeWrapped(mg.make_unet(cfg), "unet", cfg["mod_features"]).eval()
    unet_shapes = mg.load_synth(wrapped, seed=6)
    usd = {k: v.clone() for k, v in wrapped.state_dict().items()}
    uden = KarrasDenoiser(wrapped, VPSchedule()).eval()
    umean = lambda x, t: sampling.karras_mean(lambda a, c: nets.time_wrapped_unet(usd, cfg, a, c), x, t)  # noqa: E731
    box = torch.zeros(1, 1, 16, 16, dtype=torch.bool)
    box[..., 4:12, 3:10] = True
    utruth = torch.randn(2, 3, 16, 16, generator=g)
    torch.manual_seed(1)
    ux1 = DDIMSampler(uden, steps=8, silent=True).init((2, 3, 16, 16))
    cases["unet_it3"] = run_case("unet_it3", uden, umean, ux1, utruth * box, box, arrays, steps=8, iterations=3, eta=0.0)

    meta = {"cases": cases, "signature": signature(), "loop_seed": 2, "toy_shapes": toy_shapes, "toy_weight_seed": 4,
            "unet_cfg": cfg, "unet_shapes": unet_shapes, "unet_weight_seed": 6}
    mg.save("g25_repaint", meta, **arrays)


if __name__ == "__main__":
    main()
