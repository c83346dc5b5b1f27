r"""The VDM plugin on one GPU: ms per denoise step and images/s of ``imagenet_128`` (128 x 128, batch 8, DDIM-50) in the three
``AZ_FP32_MFMA`` modes, the share of a step spent outside the convolution kernels (per launch family, timed launch by launch
with events), and the achieved GB/s of ``az_fourier_planes_f32`` and ``az_upsample_bilinear2x_f32`` at 8 x 128 x 128 x 20 and
8 x 64 x 64 x 256.

    python tools/vdm_micro.py [--steps 50] [--batch 8] [--size 128] [--base-channels C] [--out FILE]

Weights are random (timing does not depend on them).  The sampling figure is the median of 3 whole sampler calls after one
warm-up call (which builds the plan and captures the graph); kernel figures are medians over 20 launches between events.
"""

from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def event_ms(fn, reps: int = 20) -> float:
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def family(name: str) -> str:
    if name.startswith("az_conv2d"):
        return "conv"
    if name.startswith("az_attention"):
        return "attention"
    if name.startswith("az_absmax"):
        return "absmax"
    return {"az_affine_act_f32": "avgpool / norm apply", "az_fourier_planes_f32": "fourier planes",
            "az_upsample_bilinear2x_f32": "bilinear"}.get(name, "other")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--model", default="imagenet_128")
    ap.add_argument("--base-channels", type=int, default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from azula_amd import _lib, engine
    from azula_amd.plugins import vdm
    from azula_amd.sample import DDIMSampler

    lines = [f"device: {torch.cuda.get_device_name()}  torch {torch.__version__}  {args.model} {args.size}x{args.size} batch {args.batch} DDIM-{args.steps}"]
    torch.manual_seed(0)
    kw = {} if args.base_channels is None else {"base_channels": args.base_channels}
    den = vdm.make_model(args.model, **kw).cuda().eval()
    x1 = torch.randn(args.batch, 3, args.size, args.size, device="cuda")
    for mode in ("f16x2", "bf16x3", "native"):
        engine.FP32_MFMA = mode
        smp = DDIMSampler(den, steps=args.steps, silent=True)
        smp(x1)  # plan + capture
        torch.cuda.synchronize()
        runs = []
        for _ in range(3):
            t0 = time.perf_counter()
            smp(x1)
            torch.cuda.synchronize()
            runs.append(time.perf_counter() - t0)
        sec = statistics.median(runs)
        lines.append(f"{mode}: {1e3 * sec / args.steps:.2f} ms per denoise step, {args.batch / sec:.2f} images/s")
        # one backbone evaluation launch by launch (un-fused plan, same kernels): where the time goes
        plan = den.backbone.plan(args.batch, args.size, args.size, x1.device)
        s = _lib.stream_ptr()
        per: dict[str, float] = {}
        for fn, a, name in plan.tape.ops:
            per[family(name)] = per.get(family(name), 0.0) + event_ms(lambda fn=fn, a=a: fn(*a, s), reps=5)
        total = sum(per.values())
        lines.append(f"  launch by launch: {total:.2f} ms; outside the convolutions {100 * (1 - per.get('conv', 0.0) / total):.1f} %  ("
                     + ", ".join(f"{k} {v:.3f} ms" for k, v in sorted(per.items(), key=lambda kv: -kv[1])) + ")")
        den.backbone._plans.clear()
        del smp, plan
    # the two new kernels
    for B, H, W, cs in ((8, 128, 128, 20), (8, 64, 64, 256)):
        dst = torch.zeros(B, H * W, cs, device="cuda")
        w, t = torch.randn(8, device="cuda"), torch.full((1,), 0.3, device="cuda")
        ms = event_ms(lambda: _lib.call("az_fourier_planes_f32", dst.data_ptr(), B, H * W, cs, 3, w.data_ptr(), 8, t.data_ptr(), 0, 1, _lib.stream_ptr()))
        lines.append(f"az_fourier_planes_f32 {B}x{H}x{W}x{cs}: {1e3 * ms:.1f} us, {B * H * W * 16 * 4 / ms / 1e6:.0f} GB/s written")
        src = torch.randn(B, H // 2, W // 2, cs, device="cuda")
        up = torch.empty(B, H, W, cs, device="cuda")
        ms = event_ms(lambda: _lib.call("az_upsample_bilinear2x_f32", up.data_ptr(), src.data_ptr(), B, H // 2, W // 2, cs, _lib.stream_ptr()))
        lines.append(f"az_upsample_bilinear2x_f32 -> {B}x{H}x{W}x{cs}: {1e3 * ms:.1f} us, {(src.numel() + up.numel()) * 4 / ms / 1e6:.0f} GB/s (read once + written)")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
