r"""Time ``az_op_blur_f32`` (through ``BlurOperator``) against torch-op forms of the same blur on the same device tensor.

    python tools/time_operators.py [taps] [B] [C] [H] [W]

Default: the 61-tap Gaussian of DPS's deblurring setup on 4 x 3 x 256 x 256.  HIP events around back-to-back calls after a
warm-up, the forms alternating over ``ROUNDS`` rounds; prints the median time per call of

* the operator (one launch of the kernel),
* the package's torch path (the separable shift-and-add a non-fp32 tensor takes: ``2 * taps`` slices), and
* the oracle of the tests (``tests/operator_oracle.py``: the two-dimensional shift-and-add, ``taps^2`` slices),

the kernel's share of the HBM roofline (one fp32 read and one write per element over the measured copy bandwidth of the MI355X,
6.29 TB/s) and one JSON line.  The figures in DESIGN.md section 9c come from this script.
"""

from __future__ import annotations

import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import operator_oracle as oo  # noqa: E402
from azula_amd.guidance import BlurOperator, gaussian_taps  # noqa: E402

HBM = 6.29e12
ROUNDS, WARMUP = 7, 3


def timed(fn, reps: int) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / reps


def main() -> None:
    n, B, Cc, H, W = (int(v) for v in (sys.argv[1:6] + ["61", "4", "3", "256", "256"][len(sys.argv) - 1:]))
    if not torch.cuda.is_available():
        raise SystemExit("time_operators.py measures on the GPU: no device visible")
    torch.manual_seed(0)
    x = torch.randn(B, Cc, H, W, device="cuda")
    taps = gaussian_taps(n / 6.0, n)
    A = BlurOperator(taps)
    td = taps.cuda()
    forms = {"kernel": (lambda: A(x), 200), "torch_path": (lambda: A._torch(x, "apply"), 5),
             "oracle": (lambda: oo.blur(x, td, td, False), 2)}
    ref = oo.blur(x.double(), td.double(), td.double(), False)
    err = {k: float((fn().double() - ref).abs().max()) for k, (fn, _) in forms.items()}
    for fn, _ in forms.values():
        for _ in range(WARMUP):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(ROUNDS):
        for k, (fn, reps) in forms.items():
            times[k].append(timed(fn, reps))
    med = {k: statistics.median(v) for k, v in times.items()}
    floor = 2 * x.numel() * 4 / HBM
    for k in forms:
        print(f"{k}: {med[k] * 1e6:.1f} us per call (min {min(times[k]) * 1e6:.1f}, max {max(times[k]) * 1e6:.1f}), "
              f"max|d| to fp64 {err[k]:.2e}")
    print(f"HBM floor {floor * 1e6:.2f} us -> the kernel runs at {floor / med['kernel']:.1%} of the HBM roofline")
    print(json.dumps({"taps": n, "shape": [B, Cc, H, W], **{f"{k}_us": med[k] * 1e6 for k in forms}, "hbm_floor_us": floor * 1e6,
                      "hbm_fraction": floor / med["kernel"]}))


if __name__ == "__main__":
    main()
