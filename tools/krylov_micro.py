r"""Per-iteration cost of the Krylov kernels (``azula_amd.linalg``) against the reference's torch op sequence, one process.

    python tools/krylov_micro.py [--reps 20] [--no-diffpir]

b is 4 x 3 x 256 x 256 fp32, state fp64, solved as rows of 256 (the DiffPIR case: one system per image row) and as rows of
196608 (a flattened image per row).  The operator returns a precomputed tensor, so only the solver is timed; the
per-iteration time is (t(K iterations) - t(1 iteration)) / (K - 1), median over ``--reps`` runs, CUDA events.  The HBM floor
of a CG iteration is its 56 bytes per element (Ap32 in, x / r / p read and written, p32 out) at the rate of a 1 GiB device copy.
Then one DiffPIR evaluation (C2's UNet, batch 4, a pixel-mask operator, gmres and cg with 1 iteration) beside one plain
evaluation of the same denoiser.  Prints one JSON line.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def timed(fn, reps: int) -> float:
    r"""Median milliseconds of fn() over reps runs (after one warm-up)."""
    fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def per_iteration_us(solve, A, b, K: int, reps: int) -> float:
    t1 = timed(lambda: solve(A, b, iterations=1), reps)
    tk = timed(lambda: solve(A, b, iterations=K), reps)
    return 1e3 * (tk - t1) / (K - 1)


def copy_rate_gbs(n_bytes: int, reps: int) -> float:
    src = torch.empty(n_bytes // 4, device="cuda")
    dst = torch.empty_like(src)
    ms = timed(lambda: dst.copy_(src), reps)
    return 2 * n_bytes / ms / 1e6


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-diffpir", action="store_true")
    args = ap.parse_args()

    from azula_amd.linalg import cg, gmres, solve

    torch.set_grad_enabled(False)
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    shape = (4, 3, 256, 256)
    n = 4 * 3 * 256 * 256
    result = {"shape": list(shape), "state": "float64"}
    rate = copy_rate_gbs(1 << 30, args.reps)  # sustained HBM rate: a copy far larger than the caches
    result["copy_GBps"] = round(rate, 1)
    result["cg_floor_us"] = round(56 * n / rate / 1e3, 2)
    for rows_of, bshape in (("256", shape), ("196608", (4, 3 * 256 * 256))):
        b = torch.randn(bshape, generator=g).to(dev)
        Ap = (0.5 * b + 0.1 * torch.randn(bshape, generator=g).to(dev)).contiguous()
        A = lambda v: Ap  # noqa: E731  (the operator's own cost is not the solver's)
        for name, kern, ops, K in (("cg", cg, solve._cg_ops, 9), ("gmres", gmres, solve._gmres_ops, 5)):
            k_us = per_iteration_us(kern, A, b, K, args.reps)
            t_us = per_iteration_us(lambda A_, b_, iterations: ops(A_, b_, None, iterations, torch.float64), A, b, K, args.reps)
            result[f"{name}_rows{rows_of}"] = {"kernel_us": round(k_us, 2), "torch_us": round(t_us, 2),
                                               "speedup": round(t_us / k_us, 2), "iterations_timed": f"1..{K}"}

    if not args.no_diffpir:
        import bench

        from azula_amd.guidance import DiffPIRDenoiser

        cfg = bench.CONFIGS["c2"]
        den = bench.build_denoiser(cfg, dev)
        B = cfg["batch"]
        x = torch.randn(B, *cfg["shape"], generator=g).to(dev)
        mask = (torch.rand(1, 1, *cfg["shape"][1:], generator=g) < 0.5).float().to(dev)
        y = (torch.randn(B, *cfg["shape"], generator=g).to(dev) * mask)
        t = torch.tensor(0.5, device=dev)
        result["eval_ms"] = round(timed(lambda: den(x, t), args.reps), 3)
        for solver in ("gmres", "cg"):
            dp = DiffPIRDenoiser(den, y, lambda v: v * mask, 0.05, solver=solver, iterations=1)
            result[f"diffpir_{solver}_ms"] = round(timed(lambda: dp(x, t), args.reps), 3)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
