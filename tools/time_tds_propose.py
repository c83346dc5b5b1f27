r"""Time ``az_tds_propose_f32`` against the reference's torch op sequence for ``tds.py:80-102`` on the same device tensors.

    python tools/time_tds_propose.py [K] [C] [H] [W]

HIP events around ``REPS`` back-to-back launches after a warm-up, both forms alternating over ``ROUNDS`` rounds; prints the
median time per call of each, the kernel's share of the HBM roofline (five K x N fp32 streams over the measured copy
bandwidth of the MI355X, 6.29 TB/s) and one JSON line.  The figures in DESIGN.md come from this script.
"""

from __future__ import annotations

import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
from torch.distributions import Normal  # noqa: E402

from azula_amd import _lib  # noqa: E402
from azula_amd.noise import VPSchedule  # noqa: E402

HBM = 6.29e12
REPS, ROUNDS, WARMUP = 50, 7, 10


def torch_sequence(x_t, x_hat, score, log_p, k, alpha_t, sigma_t, alpha_s, sigma_s):
    r"""What the kernel replaces, as eager torch ops: four gathers, two ``Normal`` objects sharing their scale, one ``sample``,
    two ``log_prob`` and three per-particle sums."""
    x_t, x_hat, log_p, score = x_t[k], x_hat[k], log_p[k], score[k]
    ratio = (alpha_t / alpha_s * sigma_s / sigma_t) ** 2
    spread = sigma_s * torch.sqrt(1 - ratio)

    def transition(mean):
        noise = (x_t - alpha_t * mean) / sigma_t
        return Normal(alpha_s * mean + sigma_s * torch.sqrt(ratio) * noise, spread, validate_args=False)

    plain, twisted = transition(x_hat), transition(x_hat + sigma_t**2 / alpha_t * score)
    x_s = twisted.sample()
    return x_s, plain.log_prob(x_s).flatten(1).sum(1) - twisted.log_prob(x_s).flatten(1).sum(1) - log_p


def timed(fn) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / REPS


def main() -> None:
    K, Cc, H, W = (int(v) for v in (sys.argv[1:5] + ["16", "3", "256", "256"][len(sys.argv) - 1:]))
    N = Cc * H * W
    dev = "cuda"
    torch.manual_seed(0)
    x_t, x_hat, score, z = (torch.randn(K, Cc, H, W, device=dev) for _ in range(4))
    log_p = torch.randn(K, device=dev)
    k = torch.randint(K, (K,), device=dev)
    sch = VPSchedule()
    t, s = torch.tensor(0.5, device=dev), torch.tensor(0.4375, device=dev)
    (alpha_t, sigma_t), (alpha_s, sigma_s) = sch(t), sch(s)
    tau = (alpha_t / alpha_s * sigma_s / sigma_t) ** 2
    scale = sigma_s * torch.sqrt(1 - tau)
    coef = torch.stack([alpha_t, alpha_s, sigma_t**2 / alpha_t, sigma_s * torch.sqrt(tau) / sigma_t, scale, 1 / scale]).float().contiguous()
    chunks = _lib.lib().az_tds_chunks(K, N)
    x_s, log_w = torch.empty_like(x_t), torch.empty(K, device=dev)
    work = torch.empty(K * chunks, dtype=torch.float64, device=dev)
    a = _lib.AzTdsProposeArgs(x_t=_lib.ptr(x_t), x_hat=_lib.ptr(x_hat), score=_lib.ptr(score), z=_lib.ptr(z), ancestors=_lib.ptr(k),
                              log_p=_lib.ptr(log_p), coef=_lib.ptr(coef), x_s=_lib.ptr(x_s), log_w_next=_lib.ptr(log_w),
                              workspace=work.data_ptr(), K=K, N=N, chunks=chunks)
    stream = _lib.stream_ptr()
    kernel = lambda: _lib.call("az_tds_propose_f32", C.byref(a), stream)  # noqa: E731
    ops = lambda: torch_sequence(x_t, x_hat, score, log_p, k, alpha_t, sigma_t, alpha_s, sigma_s)  # noqa: E731
    for _ in range(WARMUP):
        kernel()
        ops()
    torch.cuda.synchronize()
    tk, to_ = [], []
    for _ in range(ROUNDS):
        tk.append(timed(kernel))
        to_.append(timed(ops))
    mk, mo = statistics.median(tk), statistics.median(to_)
    floor = 5 * K * N * 4 / HBM
    print(f"K {K} N {N}: kernel {mk * 1e6:.1f} us (min {min(tk) * 1e6:.1f}, max {max(tk) * 1e6:.1f}), torch ops {mo * 1e6:.1f} us "
          f"(min {min(to_) * 1e6:.1f}, max {max(to_) * 1e6:.1f}), roofline {floor * 1e6:.1f} us -> {floor / mk:.1%} of the HBM roofline")
    print(json.dumps({"K": K, "N": N, "kernel_us": mk * 1e6, "torch_ops_us": mo * 1e6, "roofline_us": floor * 1e6, "hbm_fraction": floor / mk}))


if __name__ == "__main__":
    main()
