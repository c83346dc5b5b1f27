r"""The arithmetic behind the structured-source rule of the x3 / f16x2 Winograd kernel (csrc/conv_shared.h: x3_structured_mask),
on the CPU: in float32, B^T d B of every 4 x 4 patch of a nearest-upsampled even-sized map has exact zeros at frequency index 2
in both directions; on an odd, narrowed map it has not; and the host entry az_winograd_x3_structured_mask agrees on a table of
shapes.  No device is touched."""

import ctypes as C

import pytest
import torch
import torch.nn.functional as F

BT = torch.tensor([[1.0, 0.0, -1.0, 0.0], [0.0, 1.0, 1.0, 0.0], [0.0, -1.0, 1.0, 0.0], [0.0, 1.0, 0.0, -1.0]])


def transformed_patches(x, periodic):
    r"""B^T d B of the 4 x 4 patch of every 2 x 2 output tile of the (B, C, H, W) map x, with the additions in the kernel's order
    (row_transform / nu_store of csrc/wino_x3.hip): (B, C, tiles_h, tiles_w, xi, nu)."""
    H, W = x.shape[-2:]
    th, tw = (H + 1) // 2, (W + 1) // 2
    if periodic:
        xp = F.pad(x, (1, 1, 1, 1), mode="circular")
        xp = F.pad(xp, (0, 2 * tw - W, 0, 2 * th - H))  # (tiles past an odd edge are masked: zeros)
    else:
        xp = F.pad(x, (1, 1 + 2 * tw - W, 1, 1 + 2 * th - H))
    d = xp.unfold(2, 4, 2).unfold(3, 4, 2)  # (B, C, th, tw, 4, 4)
    d0, d1, d2, d3 = d.unbind(-2)
    r = torch.stack((d0 - d2, d1 + d2, d2 - d1, d1 - d3), -2)
    u0, u1, u2, u3 = r.unbind(-1)
    return torch.stack((u0 - u2, u1 + u2, u2 - u1, u1 - u3), -1)


def nearest(x, up, H, W):
    return x.repeat_interleave(1 << up, 2).repeat_interleave(1 << up, 3)[:, :, :H, :W]


def test_the_transform_is_the_winograd_input_transform():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(1, 2, 6, 8, generator=g, dtype=torch.float64)
    v = transformed_patches(x, False)
    d = F.pad(x, (1, 1, 1, 1)).unfold(2, 4, 2).unfold(3, 4, 2)
    ref = BT.double() @ d @ BT.double().T
    assert torch.allclose(v, ref, atol=1e-12)


@pytest.mark.parametrize("periodic", [False, True])
@pytest.mark.parametrize("up", [1, 2])
@pytest.mark.parametrize("H,W", [(8, 8), (16, 12), (20, 36)])
def test_frequency_two_is_exactly_zero_on_even_upsampled_maps(H, W, up, periodic):
    g = torch.Generator().manual_seed(H * 100 + W + up)
    lo = torch.randn(2, 3, (H + (1 << up) - 1) >> up, (W + (1 << up) - 1) >> up, generator=g) * 1e3
    v = transformed_patches(nearest(lo, up, H, W), periodic)
    assert v.dtype == torch.float32
    assert (v[..., 2, :] == 0).all() and (v[..., :, 2] == 0).all()
    assert not torch.signbit(v[..., 2, :]).any() and not torch.signbit(v[..., :, 2]).any()  # (+0: x - x, never -0)
    kept = [(xi, nu) for xi in (0, 1, 3) for nu in (0, 1, 3)]
    assert all((v[..., xi, nu] != 0).any() for xi, nu in kept)  # (the other 9 frequencies carry the data)


@pytest.mark.parametrize("periodic", [False, True])
def test_an_odd_narrowed_map_breaks_it(periodic):
    r"""15 x 13 cut out of a 16 x 14 upsampling: the last tile row / column has patch index 1 inside the map and index 2 outside."""
    g = torch.Generator().manual_seed(3)
    lo = torch.randn(2, 3, 8, 7, generator=g)
    v = transformed_patches(nearest(lo, 1, 15, 13), periodic)
    assert (v[..., 2, :] != 0).any() and (v[..., :, 2] != 0).any()
    assert (v[:, :, :-1, :-1, 2, :] == 0).all() and (v[:, :, :-1, :-1, :, 2] == 0).all()  # (only the edge tiles)


def test_a_plain_map_has_no_zero_frequency():
    g = torch.Generator().manual_seed(4)
    v = transformed_patches(torch.randn(1, 2, 8, 8, generator=g), False)
    assert (v[..., 2, :] != 0).any() and (v[..., :, 2] != 0).any()


def host_mask(**kw):
    from azula_amd import _lib

    a = _lib.AzConvArgs()
    a.batch, a.ksize, a.stride, a.pad = 2, 3, 1, 1
    fake = 4096  # (the entry dereferences no pointer: only whether src1 / in_affine are set)
    src1, aff = kw.pop("src1", False), kw.pop("in_affine", False)
    for k, v in kw.items():
        setattr(a, k, v)
    a.hout, a.wout = a.hin, a.win
    a.src0 = fake
    if src1:
        a.src1, a.c1s = fake, 16
    if aff:
        a.in_affine = fake
    m, lm = C.c_int32(-1), C.c_int32(-1)
    assert _lib.lib().az_winograd_x3_structured_mask(C.byref(a), C.addressof(m), C.addressof(lm)) == 0
    assert lm.value == m.value  # (no A/B switch is set here)
    return m.value


@pytest.mark.parametrize(
    "kw,mask",
    [
        (dict(hin=16, win=16), 0),                                       # no upsampling
        (dict(hin=16, win=16, up0=1), 1),                                # whole-launch form
        (dict(hin=16, win=12, up0=2), 1),                                # any shift >= 1
        (dict(hin=16, win=16, up1=1, src1=True), 2),                     # merge form
        (dict(hin=16, win=16, up0=1, up1=1, src1=True), 3),              # both sources
        (dict(hin=16, win=16, up0=1, src1=True), 0),                     # a structured source in front of a plain one: plain
        (dict(hin=16, win=16, up1=1), 0),                                # up1 without a second source means nothing
        (dict(hin=15, win=16, up1=1, src1=True), 0),                     # odd height
        (dict(hin=16, win=13, up0=1), 0),                                # odd width
        (dict(hin=16, win=16, up0=1, pad_mode=1), 1),                    # circular padding keeps it
        (dict(hin=16, win=16, up0=1, in_affine=True), 0),                # the UPS kernels take no in-gather affine
        (dict(hin=16, win=16, up0=1, up0_w=0, aniso=1), 0),              # anisotropic shift
        (dict(hin=16, win=16, up1=1, up1_w=1, aniso=1, src1=True), 0),   # the anisotropic descriptor, whatever its shifts
    ],
)
def test_the_host_entry_on_a_table_of_shapes(kw, mask):
    assert host_mask(**kw) == mask


@pytest.mark.parametrize("H,W,up,periodic", [(16, 12, 1, False), (20, 36, 2, True), (15, 13, 1, False), (16, 13, 1, True)])
def test_the_host_entry_agrees_with_the_arithmetic(H, W, up, periodic):
    g = torch.Generator().manual_seed(H + W)
    lo = torch.randn(1, 2, (H + (1 << up) - 1) >> up, (W + (1 << up) - 1) >> up, generator=g)
    v = transformed_patches(nearest(lo, up, H, W), periodic)
    zeros = bool((v[..., 2, :] == 0).all() and (v[..., :, 2] == 0).all())
    assert (host_mask(hin=H, win=W, up0=up, pad_mode=int(periodic)) == 1) == zeros
