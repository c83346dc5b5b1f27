r"""Write ``tests/golden/g29_tds.npz``: the reference's ``TDSSampler`` -- TEST INFRASTRUCTURE.

    python tools/make_golden_tds.py

Like ``tools/make_golden_guidance_vjp.py`` it needs the reference checkout.  On the small G5 UNet (``unet_group`` config) behind
a ``KarrasDenoiser`` with K = 4 particles of 3 x 16 x 16, a Gaussian twist over a pixel mask and over a 2x average pooling, it
(1) runs the reference's class on the CPU under a seed, one step and the 8-step loop, recording the ancestors that
``torch.multinomial`` returned and the standard normals behind every ``Normal.sample``; (2) runs the restatement of
``tests/tds_oracle.py`` under the same seed and asserts that it is bit-identical, and once more with the recorded ancestors and
normals fed in; (3) stores the inputs, the per-step ancestors, summed twists and ``log_w`` and the outputs; (4) per case
``e_ref``: the reference's fp32 results against the restatement in fp64 with the same ancestors and normals, the largest over the
steps -- ``x`` relative to the largest magnitude, ``log_w`` as an absolute error over ``max(1, max |log_w|)``.

The observation variance and the seed are searched for (first hit in a fixed order) so that over every loop at least one
step selects two or more distinct ancestors and at least one step repeats one: a fixture whose weights collapse onto one
particle at every step would test no gather.  The script asserts it.
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
from azula.guidance.tds import TDSSampler  # noqa: E402
from azula.noise import VPSchedule  # noqa: E402

import tds_cases as tc  # noqa: E402

STEPS, K, H, W = 8, 4, 16, 16
SEARCH = [(var_y, seed) for var_y in (1.0, 4.0, 0.25, 16.0) for seed in range(129, 139)]


def signature() -> list:
    return [["TDSSampler", p.name, p.kind.name, None if p.default is inspect.Parameter.empty else repr(p.default)]
            for p in list(inspect.signature(TDSSampler.__init__).parameters.values())[1:]]


class Recorder:
    r"""Wraps ``torch.multinomial`` and ``torch.normal`` for one run of the reference: the draws stay the generator's own; what is
    kept is the ancestors and, re-drawn from the generator state in front of each ``normal``, the standard normals behind it."""

    def __enter__(self):
        self.ancestors, self.eps = [], []
        self.keep = (torch.multinomial, torch.normal)

        def multinomial(*a, **k):
            out = self.keep[0](*a, **k)
            self.ancestors.append(out.clone())
            return out

        def normal(mean, std, *a, **k):
            before = torch.get_rng_state()
            out = self.keep[1](mean, std, *a, **k)
            after = torch.get_rng_state()
            torch.set_rng_state(before)
            self.eps.append(torch.randn(mean.shape))
            torch.set_rng_state(after)
            return out

        torch.multinomial, torch.normal = multinomial, normal
        return self

    def __exit__(self, *exc):
        torch.multinomial, torch.normal = self.keep


def build(var_y: float, seed: int):
    r"""(meta, arrays, ok) of one candidate (var_y, seed)."""
    cfg = mg.UNET_CFGS["unet_group"]
    wrapped = mg.TimeWrapped(mg.make_unet(cfg), "unet", cfg["mod_features"]).eval()
    meta = {"unet_shapes": mg.load_synth(wrapped, seed=6), "unet_cfg": cfg, "unet_weight_seed": 6, "steps": STEPS, "var_y": var_y,
            "seed": seed}
    usd = {k: v.clone() for k, v in wrapped.state_dict().items()}
    usd64 = {k: v.double() for k, v in usd.items()}
    den = KarrasDenoiser(wrapped, VPSchedule()).eval()
    omean = lambda x, t: sampling.karras_mean(lambda a, c: nets.time_wrapped_unet(usd, cfg, a, c), x, t)  # noqa: E731
    omean64 = lambda x, t: sampling.karras_mean(lambda a, c: nets.time_wrapped_unet(usd64, cfg, a, c), x, t, backbone_dtype=torch.float64)  # noqa: E731

    g = torch.Generator().manual_seed(seed)
    truth = torch.randn(1, 3, H, W, generator=g)
    mask = (torch.rand(1, 1, H, W, generator=g) < 0.4).float()
    t, s = torch.tensor(0.6), torch.tensor(0.5)
    x_t = 0.8 * truth + 0.6 * torch.randn(K, 3, H, W, generator=g)
    x1 = torch.randn(K, 3, H, W, generator=g)
    arrays = {"mask": mask, "x_t": x_t, "t": t, "s": s, "x1": x1}
    ops = {"mask": tc.go.mask_op(mask)[0], "pool": tc.go.pool_op(H, W)[0]}
    for name, A in ops.items():
        arrays[f"{name}_y"] = A(truth) + var_y**0.5 * torch.randn(A(truth).shape, generator=g)
    twists = tc.make_twists(arrays, var_y)
    arr64 = {k: (v.double() if v.is_floating_point() else v) for k, v in arrays.items()}
    twists64 = tc.make_twists(arr64, var_y)
    e_ref: dict = {}
    ok = True

    for tag in tc.CASES:
        name, kind = tag.split("_")
        smp = TDSSampler(den, twists[name], steps=STEPS, silent=True)
        torch.manual_seed(seed + tc.SEED[tag])
        with Recorder() as rec:
            if kind == "step":
                carry: dict = {}
                ref_x, ref_log_w = smp.step(x_t, t, s, carry), None
                ref_log_w = carry["log_w"]
            else:
                ref_x = smp(x1)
        torch.manual_seed(seed + tc.SEED[tag])
        mine = tc.run_case(tag, omean, twists, arrays, STEPS)
        fed = tc.run_case(tag, omean, twists, arrays, STEPS, rec.ancestors, rec.eps)
        wide = tc.run_case(tag, omean64, twists64, arr64, STEPS, rec.ancestors, [e.double() for e in rec.eps])
        mg.same(ref_x, mine[-1]["x_s"], tag)
        if kind == "step":
            mg.same(ref_log_w, mine[-1]["log_w"], tag + " log_w")
        for a, b, c in zip(mine, fed, rec.ancestors):
            mg.same(a["x_s"], b["x_s"], tag + " fed")
            mg.same(a["log_w"], b["log_w"], tag + " fed log_w")
            mg.same(a["ancestors"], c, tag + " ancestors")
        arrays[f"{tag}_x"] = ref_x
        arrays[f"{tag}_ancestors"] = torch.stack([m["ancestors"] for m in mine])
        arrays[f"{tag}_log_w"] = torch.stack([m["log_w"] for m in mine])
        arrays[f"{tag}_log_p"] = torch.stack([m["log_p"] for m in mine])
        e_x = max(float((a["x_s"].double() - b["x_s"]).abs().max() / b["x_s"].abs().max()) for a, b in zip(mine, wide))
        e_w = max(float((a["log_w"].double() - b["log_w"]).abs().max() / max(1.0, float(b["log_w"].abs().max())))
                  for a, b in zip(mine, wide))
        e_ref[tag] = {"x_s": e_x, "log_w": e_w}
        if kind == "loop":
            distinct = [len(set(a.tolist())) for a in rec.ancestors]
            ok = ok and max(distinct) >= 2 and min(distinct) < K
            print(f"var_y {var_y} seed {seed} {tag}: distinct ancestors per step {distinct}")
    meta.update({"e_ref": e_ref, "signature": signature()})
    return meta, arrays, ok


def main() -> None:
    for var_y, seed in SEARCH:
        meta, arrays, ok = build(var_y, seed)
        if ok:
            break
    assert ok, "no candidate keeps the ancestors diverse"
    for tag in tc.CASES:
        if tag.endswith("loop"):
            distinct = [len(set(a.tolist())) for a in arrays[f"{tag}_ancestors"]]
            assert max(distinct) >= 2 and min(distinct) < K, (tag, distinct)
        print(f"{tag}: e_ref {meta['e_ref'][tag]}")
    mg.save("g29_tds", meta, **arrays)


if __name__ == "__main__":
    main()
