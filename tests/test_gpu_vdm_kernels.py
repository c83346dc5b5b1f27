r"""``az_fourier_planes_f32`` and ``az_upsample_bilinear2x_f32`` (csrc/vdm.hip) on the GPU, through ctypes.

Fourier planes: against fp64, ``|err| <= 16 * 2^-24 * (1 + |f|)`` with ``f = 2 pi u w`` the fp64 argument -- about six fp32
operations ahead of the cosine, each moving ``f`` by at most ``2^-24`` relative, with slack for ``logf`` / ``cosf``.  The bound is
first checked on the CPU (tests/test_vdm_host.py) for torch's own fp32 evaluation of the reference formula: it holds (<= 0.11 x)
everywhere but at (mode 1, t = 0.9936), where ``log(cos^2 / sin^2)`` is ill conditioned and torch's fp32 is at 1.95 x; the
kernel evaluates the features in fp64 and is held to the bound as stated, at every time.  Channels outside the written range keep
a sentinel.

Bilinear x2: against ``F.interpolate`` on the CPU, ``|err| <= 2^-22 * max |x|`` -- two roundings of a convex combination per axis.
"""

import itertools
import math

import pytest
import torch
import torch.nn.functional as F

import vdm_cases as vc
from azula_amd import _lib

pytestmark = pytest.mark.gpu
U, TIMES = vc.U, vc.TIMES
fourier_case, fourier_reference = vc.fourier_case, vc.fourier_reference
SENTINEL = -12345.5


@pytest.mark.parametrize("cs,t_stride,mode,std", itertools.product((20, 32), (0, 1), (0, 1), (0.2, 1.0)))
def test_fourier_planes(cs, t_stride, mode, std):
    B, HW, c_lo, nh = 2, 5 * 7, 3, 8
    worst = 0.0
    for pair in range(len(TIMES)):
        w, t = fourier_case(std, mode, t_stride, pair)
        dst = torch.full((B, HW, cs), SENTINEL, device="cuda")
        wd, td = w.cuda(), t.cuda()
        _lib.call("az_fourier_planes_f32", _lib.ptr(dst), B, HW, cs, c_lo, _lib.ptr(wd), nh, _lib.ptr(td), t_stride, mode, _lib.stream_ptr())
        got = dst.cpu()
        exact, f = fourier_reference(t.double().expand(B) if not t_stride else t.double(), w.double(), mode)
        planes = got[:, :, c_lo : c_lo + 2 * nh].double()
        err = (planes - exact[:, None, :]).abs()
        bound = 16 * U * (1 + f.abs())[:, None, :]
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (pair, float((err / bound).max()))
        rest = torch.cat([got[:, :, :c_lo], got[:, :, c_lo + 2 * nh :]], dim=-1)
        assert (rest == SENTINEL).all(), "a channel outside [c_lo, c_lo + 2 nh) was written"
    print(f"cs {cs} t_stride {t_stride} mode {mode} std {std}: worst err / bound {worst:.3f}")


@pytest.mark.parametrize("hw,cs,mag", itertools.product(((1, 1), (3, 5), (4, 4)), (4, 20, 64), (1e-3, 1.0, 1e3)))
def test_upsample_bilinear2x(hw, cs, mag):
    B, (H, W) = 2, hw
    x = vc.tensor(f"bilinear/{H}x{W}/{cs}", (B, H, W, cs), mag)
    ref = F.interpolate(x.permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    xd = x.cuda()
    dst = torch.full((B, 2 * H, 2 * W, cs), SENTINEL, device="cuda")
    _lib.call("az_upsample_bilinear2x_f32", _lib.ptr(dst), _lib.ptr(xd), B, H, W, cs, _lib.stream_ptr())
    err = float((dst.cpu().double() - ref.double()).abs().max())
    bound = 2.0**-22 * float(x.abs().max())
    print(f"{H}x{W} cs {cs} mag {mag}: err {err:.3e} bound {bound:.3e}")
    assert err <= bound


def test_argument_errors():
    lib, s = _lib.lib(), _lib.stream_ptr()
    d = torch.zeros(2 * 35 * 20 + 4, device="cuda")
    w, t = torch.zeros(8, device="cuda"), torch.zeros(2, device="cuda")
    p, pw, pt = d.data_ptr(), w.data_ptr(), t.data_ptr()
    E_NULL, E_SHAPE, E_ALIGN, E_UNSUPPORTED = -1, -2, -3, -4
    fp = lib.az_fourier_planes_f32
    assert fp(None, 2, 35, 20, 3, pw, 8, pt, 0, 0, s) == E_NULL
    assert fp(p, 2, 35, 20, 3, None, 8, pt, 0, 0, s) == E_NULL
    assert fp(p, 2, 35, 20, 3, pw, 8, None, 0, 0, s) == E_NULL
    assert fp(p, 0, 35, 20, 3, pw, 8, pt, 0, 0, s) == E_SHAPE
    assert fp(p, 2, 35, 18, 3, pw, 8, pt, 0, 0, s) == E_SHAPE  # cs % 4
    assert fp(p, 2, 35, 20, 5, pw, 8, pt, 0, 0, s) == E_SHAPE  # the range leaves the pixel
    assert fp(p, 2, 35, 20, 3, pw, 0, pt, 0, 0, s) == E_SHAPE
    assert fp(p, 2, 35, 20, 3, pw, 8, pt, 2, 0, s) == E_SHAPE  # t_stride
    assert fp(p, 2, 35, 20, 3, pw, 8, pt, 0, 2, s) == E_UNSUPPORTED  # mode
    assert fp(p + 4, 2, 35, 20, 3, pw, 8, pt, 0, 0, s) == E_ALIGN
    up = lib.az_upsample_bilinear2x_f32
    src = torch.zeros(2 * 3 * 5 * 8 + 4, device="cuda")
    dst = torch.zeros(4 * 2 * 3 * 5 * 8 + 4, device="cuda")
    ps, pd = src.data_ptr(), dst.data_ptr()
    assert up(None, ps, 2, 3, 5, 8, s) == E_NULL
    assert up(pd, None, 2, 3, 5, 8, s) == E_NULL
    assert up(pd, ps, 2, 0, 5, 8, s) == E_SHAPE
    assert up(pd, ps, 2, 3, 5, 6, s) == E_SHAPE  # cs % 4
    assert up(pd, pd, 2, 3, 5, 8, s) == E_SHAPE  # in place
    assert up(pd + 4, ps, 2, 3, 5, 8, s) == E_ALIGN
    assert up(pd, ps + 4, 2, 3, 5, 8, s) == E_ALIGN
    torch.cuda.synchronize()
