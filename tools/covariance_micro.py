r"""Covariance applies on one GPU: per-apply time of the kernels (``csrc/covariance.hip``) beside the device torch op
sequence of the same covariance and beside the HBM byte floor, then GaussianDenoiser's captured DDIM-64 loop against the
generic loop, then one JFPS evaluation on C2's UNet beside one plain evaluation.

    python tools/covariance_micro.py [--out FILE]

x is 4 x 3 x 256 x 256 fp32 (Full: 64 x 3 x 32 x 32, N = 3072).  The floor counts x read once, y written once and the
factors read once, at 5.3 TB/s (a measured copy rate, printed too)."""

from __future__ import annotations

import argparse
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def timed(fn, reps: int) -> float:
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def copy_rate_gbs(n_bytes: int, reps: int = 50) -> float:
    a = torch.empty(n_bytes // 4, device="cuda")
    b = torch.empty_like(a)
    return 2 * n_bytes / timed(lambda: b.copy_(a), reps) / 1e9


def orth(n, dtype=torch.float32):
    Q, _ = torch.linalg.qr(torch.randn(n, n, dtype=torch.float64))
    return Q.to(dtype).contiguous().cuda()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from azula_amd.linalg import covariance as cv

    lines = [f"device: {torch.cuda.get_device_name()}  torch {torch.__version__}"]
    rate = copy_rate_gbs(256 << 20)
    lines.append(f"copy rate: {rate:.0f} GB/s (read + write of 256 MiB)")
    torch.manual_seed(0)
    shape = (3, 256, 256)
    n = math.prod(shape)
    D = (0.5 + torch.rand(shape)).cuda()

    def dplr(r):
        return cv.DPLRCovariance(D, 0.3 / math.sqrt(r) * torch.randn(*shape, r).cuda())

    cases = [
        ("diagonal", cv.DiagonalCovariance(D), 4, shape),
        ("dplr r16", dplr(16), 4, shape),
        ("dplr r64", dplr(64), 4, shape),
        ("kronecker diag L", cv.KroneckerCovariance([orth(m) for m in shape], cv.DiagonalCovariance(D)), 4, shape),
        ("kronecker dplr-8 L", cv.KroneckerCovariance([orth(m) for m in shape], dplr(8)), 4, shape),
        ("full N=3072", cv.FullCovariance(orth(3072).reshape(3, 32, 32, 3072), 0.5 + torch.rand(3072).cuda()), 64, (3, 32, 32)),
    ]
    lines.append(f"{'case':22s} {'kernels us':>11s} {'torch us':>10s} {'floor us':>9s}")
    for name, cov, B, shp in cases:
        x = torch.randn(B, *shp).cuda()
        fac = sum(t.numel() * 4 for t in cov.__dict__.values() if torch.is_tensor(t))
        if isinstance(cov, cv.KroneckerCovariance):
            fac = sum(Q.numel() * 4 for Q in cov.Qs) + sum(t.numel() * 4 for t in cov.L.__dict__.values())
        floor = (2 * x.numel() * 4 + fac) / (rate * 1e9 / 1) * 1e6
        k_us = timed(lambda: cov @ x, 50) * 1e6
        orig = cv._kernels_take
        cv._kernels_take = lambda *a: False
        try:
            t_us = timed(lambda: cov @ x, 20) * 1e6
        finally:
            cv._kernels_take = orig
        lines.append(f"{name:22s} {k_us:11.1f} {t_us:10.1f} {floor:9.1f}")

    # GaussianDenoiser: captured DDIM-64 against the generic loop
    from azula_amd import sample
    from azula_amd.denoise import GaussianDenoiser
    from azula_amd.noise import VPSchedule

    for name, cov, _, _ in cases[:1] + cases[3:4]:
        den = GaussianDenoiser(torch.zeros(shape).cuda(), cov, VPSchedule())
        s = sample.DDIMSampler(den, steps=64, silent=True)
        x = torch.randn(4, *shape).cuda()
        fused = timed(lambda: s(x), 5) * 1e3 / 64
        orig = sample.Sampler._fusable
        sample.Sampler._fusable = lambda self, x: False
        try:
            generic = timed(lambda: s(x), 3) * 1e3 / 64
        finally:
            sample.Sampler._fusable = orig
        lines.append(f"GaussianDenoiser DDIM-64 {name}: captured {fused:.3f} ms/step, generic {generic:.3f} ms/step")

    # one JFPS evaluation on C2's UNet against a plain evaluation
    import bench
    from azula_amd.guidance import JFPSDenoiser

    den = bench.build_denoiser(bench.CONFIGS["c2"], torch.device("cuda"))
    mask = (torch.rand(shape) > 0.5).float().cuda()
    A = lambda v: v * mask  # noqa: E731
    x = torch.randn(4, *shape).cuda()
    t = torch.tensor(0.5).cuda()
    y = A(torch.randn(4, *shape).cuda())
    jf = JFPSDenoiser(den, y, A, cv.IsotropicCovariance(0.05), cv.DiagonalCovariance(D), solver="cg", iterations=1)
    with torch.no_grad():
        plain = timed(lambda: den(x, t), 5) * 1e3
        jfps = timed(lambda: jf(x, t), 5) * 1e3
        ok = bool(torch.isfinite(jf(x, t).mean).all())
    lines.append(f"C2 evaluation: plain {plain:.2f} ms, JFPS (Diagonal cov_x, cg 1) {jfps:.2f} ms, finite {ok}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
