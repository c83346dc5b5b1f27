r"""The shapes, angle sets and data of the ``RadonOperator`` tests (``test_operators_radon_host.py``, ``test_gpu_operators_radon.py``)."""

import torch

import radon_oracle as ro

# exact: multiples of 90 degrees have weights 0, 1/2 and 1 only, so integer data is projected exactly
RIGHT_ANGLES = (0.0, 90.0, 180.0, 270.0)
EXACT_HWD = [(4, 4, 4), (4, 4, 5), (5, 3, 7), (3, 5, 6), (8, 8, 13), (8, 8, 5)]  # (the last one truncates)
EXACT_BC = [(1, 1), (2, 3)]
MANY_PLANES = 70_000  # of 4 x 4: more planes than the launch has workgroups

# the accuracy rule
EVEN = tuple(i * 180.0 / 37 for i in range(37))
HARD = (44.999, 45.0, 45.001, 134.99, 135.0, 359.0, -30.0, 720.5)  # the switch of the major axis, a wrap, a negative angle
ANGLES = EVEN + HARD
SIZES = [(1, 1), (1, 17), (17, 1), (16, 16), (33, 47), (64, 64), (65, 63)]
BIG = ((128, 128), tuple(i * 2.0 for i in range(90)))  # one 128 x 128 with 90 angles: two detector tiles of the projector
SPACINGS = (1.0, 1.5, 2.0, 8.0)
DET_COUNTS = ("default", 3, "twice")
DATA = ("randn", "offset", "impulse")


def det_count(kind, H: int, W: int, d: float) -> int:
    default = ro.default_det_count(H, W, d)
    return {"default": default, "twice": 2 * default}.get(kind, kind)


def exact_planes(B: int, C: int, H: int, W: int, seed: int) -> torch.Tensor:
    r"""Integers in -8 .. 8 as fp32."""
    return torch.randint(-8, 9, (B, C, H, W), generator=torch.Generator().manual_seed(seed)).float()


def planes(kind: str, H: int, W: int, seed: int = 0) -> torch.Tensor:
    r"""One (H, W) fp32 plane of the data kind: randn, randn + 100 (a sum that cancels nothing: the absolute-value bound is
    tight), or a single impulse at the last corner (a missed weight is the whole result)."""
    if kind == "impulse":
        x = torch.zeros(H, W)
        x[-1, -1] = 3.0
        return x
    x = torch.randn(H, W, generator=torch.Generator().manual_seed(1000 * H + W + seed))
    return x + 100.0 if kind == "offset" else x


def phantom(N: int) -> torch.Tensor:
    r"""exp(-r^2 / (2 (N/8)^2)) + 0.5 exp(-((i - N/3)^2 + (j - N/2.5)^2) / (2 (N/12)^2)), r from the image centre; fp64."""
    i, j = torch.meshgrid(torch.arange(N, dtype=torch.float64), torch.arange(N, dtype=torch.float64), indexing="ij")
    r2 = (i - (N - 1) / 2) ** 2 + (j - (N - 1) / 2) ** 2
    return torch.exp(-r2 / (2 * (N / 8) ** 2)) + 0.5 * torch.exp(-((i - N / 3) ** 2 + (j - N / 2.5) ** 2) / (2 * (N / 12) ** 2))


def inner(N: int) -> torch.Tensor:
    r"""The pixels with r < N / 2 - 2."""
    i, j = torch.meshgrid(torch.arange(N, dtype=torch.float64), torch.arange(N, dtype=torch.float64), indexing="ij")
    return (i - (N - 1) / 2) ** 2 + (j - (N - 1) / 2) ** 2 < (N / 2 - 2) ** 2
