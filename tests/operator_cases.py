r"""Shapes, tap patterns and data of the measurement-operator tests -- TEST INFRASTRUCTURE.

Exact data: integers of magnitude at most 8 and taps ``(((7 i) mod 5) + 1) / 2^k`` -- distinct neighbours, not symmetric, so a
dropped, shifted or un-flipped tap changes the result.  In units of the common denominator every partial sum of a blur of up to
65 x 65 such taps is an integer of at most 65 * 5 * 65 * 5 * 8 = 845 000 < 2^24, and every pooling window sums to at most
16 * 16 * 8: fp32 is exact in any order, and a kernel must EQUAL the fp64 oracle."""

from __future__ import annotations

import torch

TAP_SHIFT = 3  # k

# blur
BLUR_RADII = [(0, 0), (1, 0), (0, 2), (1, 2), (3, 1), (32, 0), (32, 32)]
BLUR_PLANES = [1, 3, 5]
PADDINGS = ["zeros", "circular"]


def blur_sizes(th: int, tw: int) -> list[tuple[int, int]]:
    r"""(H, W) around the edges of the launch's th x tw output tile."""
    return [(1, 1), (1, 7), (7, 1), (5, 3), (th - 1, tw + 1), (th, tw), (th + 1, tw - 1), (2 * th + 3, tw + 5)]


# pooling
POOL_FACTORS = [(1, 1), (2, 2), (4, 4), (8, 8), (2, 4)]
POOL_FACTORS_RANDOM = POOL_FACTORS + [(3, 3), (2, 3)]
POOL_OUTPUTS = [(1, 1), (1, 5), (3, 1), (7, 9), (33, 65)]
POOL_MANY_PLANES = 70_000  # of 2 x 2 pixels at factor 2: more planes than a grid dimension holds


def exact_taps(n: int, k: int = TAP_SHIFT) -> torch.Tensor:
    return torch.tensor([((7 * i) % 5 + 1) / 2**k for i in range(n)], dtype=torch.float32)


def exact_image(*shape: int, seed: int = 0) -> torch.Tensor:
    gen = torch.Generator().manual_seed(seed)
    return torch.randint(-8, 9, shape, generator=gen).to(torch.float32)


def random_image(*shape: int, seed: int = 0) -> torch.Tensor:
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=gen)


def random_taps(n: int, seed: int = 0) -> torch.Tensor:
    gen = torch.Generator().manual_seed(1000 + seed)
    return torch.randn(n, generator=gen)


def split_planes(planes: int) -> tuple[int, int]:
    r"""(B, C) with B * C = planes."""
    return (1, planes) if planes < 4 else (planes, 1)
