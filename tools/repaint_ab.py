r"""Same-process A/B of ``DDIMSampler`` against ``RePaintSampler`` on one bench configuration (default C2: the 320.5 M-parameter
UNet, batch 4, 3 x 256 x 256, DDIM-64), both on the captured loop.

    python tools/repaint_ab.py [--config c2] [--iterations 3] [--rounds 5]
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/repaint_ab.py --profile

After one warm-up call of each (plan, weight packing, graph capture), the two samplers run alternately ``--rounds`` times;
the line printed is the median time per backbone evaluation of each, and ``ratio`` = RePaint call / (iterations x DDIM call),
which is 1 when the RePaint kernels cost nothing.  ``--profile``: one call of each after the warm-up, nothing timed (for a
kernel trace, whose stats give the repaint / gather / relayout kernels' average durations).
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2", choices=[k for k, v in bench.CONFIGS.items() if v["kind"] == "unet"])
    ap.add_argument("--iterations", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()

    from azula_amd.guidance import RePaintSampler
    from azula_amd.sample import DDIMSampler

    torch.set_grad_enabled(False)
    dev = torch.device("cuda", 0)
    cfg = bench.CONFIGS[args.config]
    den = bench.build_denoiser(cfg, dev)
    shape = (cfg["batch"], *cfg["shape"])
    g = torch.Generator().manual_seed(3)
    truth = torch.randn(shape, generator=g).clamp(-1, 1)
    mask = torch.zeros(1, 1, *shape[2:], dtype=torch.bool)
    H, W = shape[2:]
    mask[..., : H // 2, :] = True  # the upper half observed: inpaint the lower half
    y, mask = (truth * mask).to(dev), mask.to(dev)
    torch.manual_seed(1)
    x1 = torch.randn(shape, device=dev)
    steps = cfg["steps"]
    samplers = {
        "ddim": (DDIMSampler(den, steps=steps, silent=True), 1),
        "repaint": (RePaintSampler(den, y, mask, iterations=args.iterations, steps=steps, silent=True), args.iterations),
    }
    for name, (smp, _) in samplers.items():  # warm-up: plan, packing, capture
        smp(x1)
        assert len(smp._fused_cache) == 1, f"{name}: the captured loop was not taken"
    torch.cuda.synchronize(dev)
    if args.profile:
        for smp, _ in samplers.values():
            smp(x1)
        torch.cuda.synchronize(dev)
        return
    times: dict = {k: [] for k in samplers}
    for r in range(args.rounds):
        for name in (samplers if r % 2 == 0 else reversed(list(samplers))):
            smp, _ = samplers[name]
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            smp(x1)
            torch.cuda.synchronize(dev)
            times[name].append(time.perf_counter() - t0)
    med = {k: statistics.median(v) for k, v in times.items()}
    out = {
        "config": args.config, "steps": steps, "iterations": args.iterations, "rounds": args.rounds,
        "ddim_ms_per_eval": 1e3 * med["ddim"] / steps,
        "repaint_ms_per_eval": 1e3 * med["repaint"] / (steps * args.iterations),
        "ratio": med["repaint"] / (args.iterations * med["ddim"]),
        "ddim_call_s": times["ddim"], "repaint_call_s": times["repaint"],
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
