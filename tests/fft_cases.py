r"""Shapes and data of the Fourier-operator tests, shared by the host and the GPU file."""

import math

import torch

NORMS = ("ortho", "backward", "forward")

# (real input, real output only) of az_op_fft2_f32 with the direction each is measured in.  Real -> real takes the inverse
# direction so that its fp64 reference is the conjugate of real -> complex's, and the complex inputs share one: a 1024 x 1024
# dense-matrix reference is computed twice per data kind, not four times.  Both directions of every form: the exact test.
FORMS = {"r2c": (True, False, False), "r2r": (True, True, True), "c2c": (False, False, True), "c2r": (False, True, True)}

EXACT_SIZES = [(h, w) for h in (1, 2, 4) for w in (1, 2, 4)]
EXACT_BC = [(1, 1), (2, 3)]

SQUARES = [(n, n) for n in (8, 16, 32, 64, 128, 256, 512, 1024)]
RECTANGLES = [(1, 1024), (1024, 1), (2, 1024), (1024, 2), (8, 256), (256, 8)]
# Either side of every switch of the kernel.  It picks its form from H W alone: at most 1024 points run whole in 8 KiB of LDS,
# at most 8192 whole in 64 KiB, more in two launches -- rows, 8192 / W lines per workgroup, then tiles of 8192 / H columns.
SWITCHES = [
    ((32, 32), "1024 points: the last plane of the 8 KiB whole-plane form"),
    ((32, 64), "2048 points: the first plane of the 64 KiB whole-plane form, odd log2 H W"),
    ((64, 32), "the same, transposed: a radix-2 stage in the columns and none in the rows"),
    ((64, 128), "8192 points: the last whole plane"),
    ((128, 64), "8192 points, transposed"),
    ((128, 128), "16384 points: the first two-pass plane; 64 lines per workgroup, tiles of 64 columns"),
    ((16, 1024), "two passes with 8 lines per workgroup (the fewest) and tiles of 512 columns (the widest)"),
    ((1024, 16), "two passes with 512 lines per workgroup (the most) and tiles of 8 columns (the narrowest)"),
    ((512, 32), "tiles of 16 columns: half a wave per row of the tile, odd log2 H"),
    ((256, 64), "tiles of 32 columns: one half wave per row of the tile"),
    ((64, 256), "tiles of 128 columns, 32 lines per workgroup"),
]
ACCURACY_SIZES = list(dict.fromkeys(SQUARES + RECTANGLES + [s for s, _ in SWITCHES]))
WHOLE_PLANE_POINTS = 8192  # (az_op_fft2_work is 0 up to here)

DATA = ("randn", "offset", "impulse", "exponential")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def planes(kind: str, H: int, W: int, seed: int = 0):
    r"""(re, im) fp32 planes of shape (H, W): randn; randn + 100 (a large DC term); one impulse off the origin; one pure complex
    exponential (its transform is one bin, the leakage into the others is rounding)."""
    g = _gen(1000 * H + W + seed)
    if kind == "randn":
        return torch.randn(H, W, generator=g), torch.randn(H, W, generator=g)
    if kind == "offset":
        return torch.randn(H, W, generator=g) + 100, torch.randn(H, W, generator=g) + 100
    if kind == "impulse":
        re, im = torch.zeros(H, W), torch.zeros(H, W)
        re[(H // 3 + 1) % H, (2 * W // 5 + 1) % W] = 1.5
        im[(H // 3 + 1) % H, (2 * W // 5 + 1) % W] = -0.75
        return re, im
    assert kind == "exponential"
    k, l = (H // 4 + 1) % H, (3 * W // 8 + 1) % W
    ang = 2 * math.pi * (k * torch.arange(H, dtype=torch.float64)[:, None] / H + l * torch.arange(W, dtype=torch.float64)[None, :] / W)
    return torch.cos(ang).float(), torch.sin(ang).float()


def exact_planes(B: int, C: int, H: int, W: int, seed: int = 0) -> torch.Tensor:
    r"""Integers of magnitude at most 8 as fp32 (B, C, H, W)."""
    return torch.randint(-8, 9, (B, C, H, W), generator=_gen(seed + 17 * H + W)).float()


def symmetric_mask(H: int, W: int, seed: int = 0, weighted: bool = False) -> torch.Tensor:
    r"""A (H, W) mask that is symmetric under k -> -k mod (H, W): 0/1, or dyadic weights in {0, 0.5, 1, 2}."""
    m = torch.randint(0, 4, (H, W), generator=_gen(seed)).float()
    m = torch.maximum(m, m.flip(0, 1).roll((1, 1), (0, 1)))
    if weighted:
        return torch.tensor([0.0, 0.5, 1.0, 2.0])[m.long()]
    return (m >= 2).float()
