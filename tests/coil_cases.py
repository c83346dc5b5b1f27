r"""Shapes and data of the multi-coil MRI tests, shared by ``test_operators_coil_host.py`` and ``test_gpu_operators_coil.py``."""

import torch

NORMS = ("ortho", "backward", "forward")

# The two entries.  An item is 4 consecutive pixels: HW = 1, 2 are one partial item, 7 a whole and a partial one (the scalar
# tail), 16 and 8 * 16 take the 16-byte form (one item per lane; more than one wave).  K = 1, 3, 8: a single coil, an odd count
# (K HW % 4 != 0 with HW = 2, so per-sample maps and batches start misaligned), and more coils than the loop's unrolling.
ENTRY_B, ENTRY_K, ENTRY_HW = (1, 2), (1, 3, 8), (1, 2, 7, 16, 8 * 16)
FLOAT_K = (1, 4, 15)
SWEEP = (2, 2, 1024 * 1024)  # (B, K, HW): 2^19 items against the capped grid's 2^18 threads

# The operator: 8 x 8 runs the FFT's 8 KiB whole-plane form, 32 x 64 its 64 KiB form, 128 x 128 its two passes.
OPERATOR_SIZES = [(8, 8), (32, 64), (128, 128)]
OPERATOR_B, OPERATOR_K = 2, 4
E_REF_MAX = 4e-7  # what the torch fp32 host path may lose per plane on the operator tests' data (the accuracy rule's premise)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def ints(*shape, seed=0):
    r"""Integers of magnitude at most 8 as fp32."""
    return torch.randint(-8, 9, shape, generator=_gen(seed)).float()


def randn(*shape, seed=0, dtype=torch.float32):
    return torch.randn(*shape, generator=_gen(seed), dtype=dtype)


def exact_maps(K, H, W, seed=0, batch=None):
    r"""Gaussian-integer maps (re, im), fp32 (K, H, W) or (batch, K, H, W), whose ``sum_k |S_k|^2`` is 0 or a power of two at
    every pixel, so that the normalised combine is exact too: at a pixel, m of the K coils (m in {0, 1, 2, 4}, at most K) are
    nonzero, all units (+-1, +-i) or all of the form +-1 +- i."""
    g = _gen(1000 + seed)
    lead = () if batch is None else (batch,)
    one = (*lead, 1, H, W)
    full = (*lead, K, H, W)
    allowed = torch.tensor([m for m in (0, 1, 2, 4) if m <= K])
    m = allowed[torch.randint(0, allowed.numel(), one, generator=g)]
    rank = torch.rand(full, generator=g).argsort(-3).argsort(-3)
    keep = (rank < m).float()
    diagonal = torch.randint(0, 2, one, generator=g).bool()
    unit = torch.randint(0, 4, full, generator=g)
    u_re, u_im = torch.tensor([1.0, -1.0, 0.0, 0.0])[unit], torch.tensor([0.0, 0.0, 1.0, -1.0])[unit]
    d_re = torch.randint(0, 2, full, generator=g).float() * 2 - 1
    d_im = torch.randint(0, 2, full, generator=g).float() * 2 - 1
    return torch.where(diagonal, d_re, u_re) * keep, torch.where(diagonal, d_im, u_im) * keep


def operator_case(H, W, per_sample, complex_image):
    r"""(x, w, maps, mask) of the operator tests: randn image (B, 1 or 2, H, W) and randn observation (B, 2 K, H, W), birdcage
    maps rounded to complex64 (one set, or one per sample from coils at two radii) and ``cartesian_mask(H, W, 4)``."""
    from azula_amd.guidance import birdcage_maps, cartesian_mask

    B, K = OPERATOR_B, OPERATOR_K
    x = randn(B, 2 if complex_image else 1, H, W, seed=H + W)
    w = randn(B, 2 * K, H, W, seed=H + W + 1)
    maps = birdcage_maps(K, H, W)
    if per_sample:
        maps = torch.stack([maps, birdcage_maps(K, H, W, radius=2.0)])
    return x, w, maps.to(torch.complex64), cartesian_mask(H, W, 4)


def argument_errors(lib):
    r"""Every argument error of the two entries returns its code, and nothing below may launch: each call fails its validation
    (the pointers are never dereferenced) or is empty."""
    P, P2, X, X2, S, S2, Q = 0x100000, 0x900000, 0x1100000, 0x1900000, 0x2100000, 0x2900000, 0x500002
    NULL, SHAPE, ALIGN = -1, -2, -3

    def expand(dre=P, dim=P2, dbs=192, xre=X, xim=X2, xbs=64, sre=S, sim=S2, sbs=0, B=1, K=3, HW=64):
        return lib.az_op_coil_expand_f32(dre, dim, dbs, xre, xim, xbs, sre, sim, sbs, B, K, HW, None)

    def combine(dre=X, dim=X2, dbs=64, zre=P, zim=P2, zbs=192, sre=S, sim=S2, sbs=0, B=1, K=3, HW=64, normalize=0):
        return lib.az_op_coil_combine_f32(dre, dim, dbs, zre, zim, zbs, sre, sim, sbs, B, K, HW, normalize, None)

    for fn in (expand, combine):
        assert fn(K=0) == SHAPE and fn(K=-1) == SHAPE  # K < 1
        assert fn(B=-1) == SHAPE and fn(HW=-1) == SHAPE  # negative sizes
        assert fn(dbs=-192) == SHAPE and fn(sbs=-1) == SHAPE and fn(sbs=100) == SHAPE  # strides: maps are shared (0) or K HW apart
        assert fn(B=0) == 0 and fn(HW=0) == 0 and fn(B=0, dre=None) == 0  # empty: nothing to do
        assert fn(dre=None) == NULL and fn(sre=None) == NULL and fn(sim=None) == NULL  # required pointers
        for name in ("dre", "dim", "sre", "sim"):
            assert fn(**{name: Q}) == ALIGN, name  # not a float's address
        assert fn(dre=S) == SHAPE and fn(dre=S + 4 * 191) == SHAPE and fn(dim=S2 + 64) == SHAPE  # a destination over the maps
        assert fn(dim=P if fn is expand else X) == SHAPE  # the two destinations over each other
    # expand: the product with a complex map is complex, so dst_im is required; a real image (x_im = NULL) is fine but x_re is not
    assert expand(dim=None) == NULL and expand(xre=None) == NULL and expand(xre=None, xim=None) == NULL
    assert expand(xre=Q) == ALIGN and expand(xim=Q) == ALIGN
    assert expand(B=2, dbs=191) == SHAPE and expand(B=2, dbs=192, xbs=63) == SHAPE  # a tensor's own samples overlap
    assert expand(dre=X) == SHAPE and expand(dim=X2 + 4 * 63) == SHAPE and expand(xim=None, dim=X) == SHAPE  # dst over x
    assert expand(dre=X - 4 * 191) == SHAPE and expand(xre=P + 4 * 100) == SHAPE
    # combine: coil data is complex, so z_im is required; dst_im = NULL (the real part only) is fine
    assert combine(zim=None) == NULL and combine(zre=None) == NULL
    assert combine(zre=Q) == ALIGN and combine(zim=Q) == ALIGN
    assert combine(normalize=2) == SHAPE and combine(normalize=-1) == SHAPE
    assert combine(B=2, dbs=63) == SHAPE and combine(B=2, zbs=191) == SHAPE
    assert combine(dre=P) == SHAPE and combine(dim=P2 + 4 * 191) == SHAPE and combine(dim=None, dre=P2) == SHAPE  # dst over z
    # the halves of one (B, 2 K, H, W) tensor interleave and are not an overlap; a tensor misplaced among them is one
    assert expand(B=2, dim=P + 4 * 192, dbs=384, xre=P + 4 * 100, xbs=384) == SHAPE
    assert combine(B=2, zim=P + 4 * 192, zbs=384, dre=P + 4 * 380, dbs=384) == SHAPE
