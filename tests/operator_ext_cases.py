r"""Shapes and data of the PSF, decimation and channel-mix operator tests -- TEST INFRASTRUCTURE.

Exact data: integers of magnitude at most 8 (``operator_cases.exact_image``) and PSF entries ``(((7 (i + 3 p)) mod 5) + 1) / 2^3``
over the flattened tap index ``i`` of PSF number ``p`` -- distinct neighbours, not symmetric, another pattern per PSF, so a dropped,
shifted or un-flipped tap and a wrong PSF stride all change the result.  In units of 1 / 8 every partial sum of up to 65 x 65 such
taps is an integer of at most 65 * 65 * 5 * 8 = 169 000 < 2^24: fp32 is exact in any order, and a kernel must EQUAL the fp64
oracle.  Channel-mix matrices are dyadic with at most 16 entries of magnitude at most 2 per row: sums below 2^9 in units of 1 / 4."""

from __future__ import annotations

import torch

import operator_cases as oc

# ------------------------------------------------------------------------------------------------------------------ PSF
PSF_RADII = [(0, 0), (1, 0), (0, 2), (1, 2), (3, 1), (32, 0), (0, 32), (30, 30), (32, 32)]
PSF_BC = [(1, 1), (1, 3), (5, 1), (2, 3)]
PSF_FORMS = ["shared", "per_channel", "per_sample", "per_plane"]
PSF_COUNT = 6  # PSFs and images of the reference set: the largest plane count of PSF_BC
PSF_MANY_PLANES = 70_000  # of 2 x 2 pixels at 3 x 3 taps
PSF_GRID_PLANES = (1 << 16) + 3  # of 1 x 1 pixels: more tiles than the launch has workgroups (2^16)
PSF_TILE = (16, 64)  # az_op_psf_tile for every PSF size (the tests assert it): the sizes below sit around its edges
psf_sizes = oc.blur_sizes  # (H, W) around the edges of the launch's th x tw output tile


def psf_exact_cases() -> list[tuple[tuple[int, int], str, tuple[int, int]]]:
    r"""(radii, padding, (H, W)): every radius pair, padding and size around the tile; circular only above the radii (below them
    the operator is not defined and refuses the input).  One case per size: the fp64 reference of a 65 x 65 PSF takes a second."""
    return [(r, p, s) for r in PSF_RADII for p in oc.PADDINGS for s in psf_sizes(*PSF_TILE)
            if p == "zeros" or (r[0] < s[0] and r[1] < s[1])]


def exact_psf(kh: int, kw: int, p: int = 0) -> torch.Tensor:
    return torch.tensor([((7 * (i + 3 * p)) % 5 + 1) / 8 for i in range(kh * kw)], dtype=torch.float32).reshape(kh, kw)


def exact_psfs(kh: int, kw: int, count: int = PSF_COUNT) -> torch.Tensor:
    r"""(count, kh, kw): PSF number p at index p."""
    return torch.stack([exact_psf(kh, kw, p) for p in range(count)])


def psf_number(form: str, b: int, c: int, C: int) -> int:
    r"""The number of the PSF that plane (b, c) of a (B, C) input meets under ``form``."""
    return {"shared": 0, "per_channel": c, "per_sample": b, "per_plane": b * C + c}[form]


def psf_argument(psfs: torch.Tensor, form: str, B: int, C: int) -> torch.Tensor:
    r"""The constructor argument of ``form`` for a (B, C) input, cut from ``psfs`` (count, kh, kw)."""
    kh, kw = psfs.shape[1:]
    if form == "shared":
        return psfs[0]
    if form == "per_channel":
        return psfs[:C]
    if form == "per_sample":
        return psfs[:B].reshape(B, 1, kh, kw)
    return psfs[:B * C].reshape(B, C, kh, kw)


def psf_pairs() -> list[tuple[int, int]]:
    r"""Every (PSF number, image number) that some form meets on some (B, C) of PSF_BC, image number = plane index."""
    pairs = {(psf_number(f, b, c, C), b * C + c) for B, C in PSF_BC for f in PSF_FORMS for b in range(B) for c in range(C)}
    return sorted(pairs)


# ----------------------------------------------------------------------------------------------------------- decimation
DEC_FACTORS = [(1, 1), (2, 2), (4, 4), (2, 4), (3, 3)]
DEC_OUTPUTS = [(1, 1), (1, 5), (3, 1), (7, 9), (33, 65)]


def offsets(fh: int, fw: int) -> list[tuple[int, int]]:
    return [(a, b) for a in range(fh) for b in range(fw)]


# ---------------------------------------------------------------------------------------------------------- channel mix
MIX_CHANNELS = [(3, 1), (1, 3), (3, 3), (4, 2), (16, 16)]  # (Cin, Cout)
MIX_HW = [(1, 1), (1, 3), (2, 2), (7, 1), (1, 64 * 64 + 1)]  # (H, W) with H W in {1, 3, 4, 7, 64 * 64 + 1}
# matrices whose pseudo-inverse is dyadic too (checked on the CPU by the host test): a row selection, a sum of two channels
# ([[1,0,0],[0,1,1]]^+ = [[1,0],[0,1/2],[0,1/2]]), a scaled identity and a single channel spread over three
MIX_PINV = [
    [[0, 1, 0], [1, 0, 0]],
    [[1, 0, 0], [0, 1, 1]],
    [[2, 0, 0], [0, 0.5, 0], [0, 0, 4]],
    [[1], [1], [0]],
]
# their pseudo-inverses by hand (torch.linalg.pinv returns them to an fp64 ulp or so; the operator's rounding to fp32 removes that)
MIX_PINV_BY_HAND = [
    [[0, 1], [1, 0], [0, 0]],
    [[1, 0], [0, 0.5], [0, 0.5]],
    [[0.5, 0, 0], [0, 2, 0], [0, 0, 0.25]],
    [[0.5, 0.5, 0]],
]


def exact_matrix(Cout: int, Cin: int, seed: int = 0) -> torch.Tensor:
    r"""Dyadic entries in {-2, -1.75, ..., 2}, fp64."""
    gen = torch.Generator().manual_seed(2000 + seed)
    return torch.randint(-8, 9, (Cout, Cin), generator=gen).double() / 4


def random_matrix(Cout: int, Cin: int, seed: int = 0) -> torch.Tensor:
    gen = torch.Generator().manual_seed(3000 + seed)
    return torch.randn(Cout, Cin, generator=gen)


def random_psf(*shape: int, seed: int = 0) -> torch.Tensor:
    gen = torch.Generator().manual_seed(4000 + seed)
    return torch.randn(shape, generator=gen)
