r"""The oracle of the multi-coil MRI tests: an fp64 restatement of ``y_k = M F (S_k . x)``, its transpose and the coil-combined
zero-filled reconstruction, with the complex products written out on split planes and the dense DFT matrices of
``fft_oracle.dft2``.  Independent of ``torch.fft`` and of ``azula_amd``.  Maps are split planes ``(K, ...)`` or ``(B, K, ...)``."""

import torch

import fft_oracle as fo

F64 = torch.float64
U = 2.0**-24


def _maps(s_re, s_im, batched_ndim):
    r"""The maps as fp64 with a batch axis (of 1 for a shared set)."""
    c, d = s_re.to(F64), s_im.to(F64)
    return (c, d) if c.ndim == batched_ndim else (c[None], d[None])


def expand(x_re, x_im, s_re, s_im):
    r"""``S . x``: x planes (B, ...) and maps (K, ...) or (B, K, ...) give (B, K, ...) re and im."""
    c, d = _maps(s_re, s_im, x_re.ndim + 1)
    a = x_re.to(F64)[:, None]
    if x_im is None:
        return a * c, a * d
    b = x_im.to(F64)[:, None]
    return a * c - b * d, a * d + b * c


def expand_bound(x_re, x_im, s_re, s_im):
    r"""|a c| + |b d| and |a d| + |b c|: what the issue's bound 2 u (.) of an expanded component multiplies."""
    c, d = _maps(s_re, s_im, x_re.ndim + 1)
    a = x_re.to(F64)[:, None].abs()
    b = torch.zeros_like(a) if x_im is None else x_im.to(F64)[:, None].abs()
    return a * c.abs() + b * d.abs(), a * d.abs() + b * c.abs()


def density(s_re, s_im):
    r"""``sum_k |S_k|^2`` of (K, H, W) or (B, K, H, W) maps, without the coil axis."""
    c, d = s_re.to(F64), s_im.to(F64)
    return (c * c + d * d).sum(-3)


def combine(z_re, z_im, s_re, s_im, normalize=False):
    r"""``sum_k conj(S_k) . z_k`` of (B, K, ...) planes: (re, im), divided by ``sum_k |S_k|^2`` (0 where that is 0) on request."""
    c, d = _maps(s_re, s_im, z_re.ndim)
    p, q = z_re.to(F64), z_im.to(F64)
    re, im = (c * p + d * q).sum(1), (c * q - d * p).sum(1)
    if normalize:
        D = (c * c + d * d).sum(1)
        safe = torch.where(D != 0, D, torch.ones_like(D))
        re, im = torch.where(D != 0, re / safe, torch.zeros_like(re)), torch.where(D != 0, im / safe, torch.zeros_like(im))
    return re, im


def combine_bound(z_re, z_im, s_re, s_im):
    r"""(T_re, T_im, D): the sums of the absolute values of the 2 K products that enter each component, and ``sum_k |S_k|^2``."""
    c, d = _maps(s_re, s_im, z_re.ndim)
    p, q = z_re.to(F64).abs(), z_im.to(F64).abs()
    return (c.abs() * p + d.abs() * q).sum(1), (c.abs() * q + d.abs() * p).sum(1), (c * c + d * d).sum(1).expand(p[:, 0].shape)


def _mask(mask, inverse=False):
    m = mask.to(F64)
    return torch.where(m != 0, 1 / torch.where(m != 0, m, torch.ones_like(m)), torch.zeros_like(m)) if inverse else m


def apply(x, mask, s_re, s_im, norm="ortho", transpose_of_zero_filled=False):
    r"""``MultiCoilMRIOperator(...)(x)`` in fp64: (B, 1 or 2, H, W) -> (B, 2 K, H, W).  ``transpose_of_zero_filled``: the
    transpose of ``zero_filled`` instead -- x / sum |S|^2 first, the pinv's scale, and M^+."""
    t = transpose_of_zero_filled
    x = x.to(F64)
    x_re, x_im = x[:, 0], x[:, 1] if x.shape[1] == 2 else None
    if t:
        D = density(s_re, s_im)
        inv = _mask(D, True)
        x_re, x_im = x_re * inv, None if x_im is None else x_im * inv
    c_re, c_im = expand(x_re, x_im, s_re, s_im)
    f = fo.dft2(c_re, c_im, scale=fo.scale_of(norm, x.shape[-2] * x.shape[-1], t))
    return torch.cat([f.real, f.imag], dim=1) * _mask(mask, t)


def adjoint(y, mask, s_re, s_im, norm="ortho", complex_image=True, zero_filled=False):
    r"""``.adjoint(y)`` (``zero_filled``: ``.zero_filled(y)``) in fp64: (B, 2 K, H, W) -> (B, 1 or 2, H, W)."""
    K = y.shape[1] // 2
    v = y.to(F64) * _mask(mask, zero_filled)
    z = fo.dft2(v[:, :K], v[:, K:], inverse=True, scale=fo.scale_of(norm, y.shape[-2] * y.shape[-1], zero_filled))
    re, im = combine(z.real, z.imag, s_re, s_im, zero_filled)
    return torch.stack([re, im], dim=1) if complex_image else re[:, None]


def plane_loss(got, ref):
    r"""(the 2-norm of ``got - ref`` and of ``ref``) per (b, c) plane, in fp64."""
    return (got.to(F64) - ref).pow(2).sum((-2, -1)).sqrt(), ref.pow(2).sum((-2, -1)).sqrt()


def rule(ref, ref32):
    r"""The accuracy rule of ``test_gpu_operators_fft.py`` per output plane: (S, e_ref, the bound ``max(4 e_ref, 2 * 2^-24) S`` on
    ``||got - ref||_2``) with ``e_ref`` the relative loss of ``ref32``, the operator's torch path on fp32 host tensors."""
    err, S = plane_loss(ref32, ref)
    e_ref = err / S.clamp_min(1e-300)
    return S, e_ref, torch.maximum(4 * e_ref, torch.full_like(e_ref, 2 * U)) * S
