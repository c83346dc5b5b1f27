r"""The oracle of the Fourier operators: dense fp64 DFT matrices, independent of ``torch.fft``, in the split-complex layout
(re in channels [0, C), im in [C, 2 C)), for any size.  Multiples of a quarter turn are exactly 0 / +-1, so on integer data of
sizes up to 4 the oracle is exact."""

import math

import torch

F64 = torch.float64
EPS = 2.0**-24


def dft_matrix(n: int, inverse: bool = False) -> torch.Tensor:
    r"""``exp(-+ 2 pi i k m / n)`` as a complex128 (n, n) matrix; ``k m`` is reduced modulo ``n`` in integers first."""
    k = torch.arange(n)
    r = (k[:, None] * k[None, :]) % n
    ang = 2 * math.pi * r.to(F64) / n
    cos, sin = torch.cos(ang), torch.sin(ang)
    quarter = (4 * r) % n == 0
    q = (4 * r) // n
    cos = torch.where(quarter, torch.tensor([1.0, 0.0, -1.0, 0.0], dtype=F64)[q % 4], cos)
    sin = torch.where(quarter, torch.tensor([0.0, 1.0, 0.0, -1.0], dtype=F64)[q % 4], sin)
    return torch.complex(cos, sin if inverse else -sin)


def dft2(re: torch.Tensor, im: torch.Tensor | None = None, inverse: bool = False, scale: float = 1.0) -> torch.Tensor:
    r"""The complex128 2-D DFT over the last two axes of ``re + i im``."""
    z = torch.complex(re.to(F64), torch.zeros_like(re, dtype=F64) if im is None else im.to(F64))
    fh, fw = dft_matrix(z.shape[-2], inverse), dft_matrix(z.shape[-1], inverse)
    return torch.einsum("...kn,ln->...kl", torch.einsum("km,...mn->...kn", fh, z), fw) * scale


def scale_of(norm: str, hw: int, pinv: bool = False) -> float:
    if norm == "ortho":
        return 1.0 / math.sqrt(hw)
    if norm == "backward":
        return 1.0 / hw if pinv else 1.0
    return 1.0 if pinv else 1.0 / hw


def apply(x: torch.Tensor, norm: str = "ortho", pinv_scale: bool = False) -> torch.Tensor:
    r"""``FourierOperator(norm)(x)`` in fp64: (B, C, H, W) -> (B, 2 C, H, W)."""
    f = dft2(x, scale=scale_of(norm, x.shape[-2] * x.shape[-1], pinv_scale))
    return torch.cat([f.real, f.imag], dim=1)


def adjoint(z: torch.Tensor, norm: str = "ortho", pinv: bool = False) -> torch.Tensor:
    r"""``FourierOperator(norm).adjoint(z)`` (``pinv``: ``.pinv(z)``) in fp64: (B, 2 C, H, W) -> (B, C, H, W)."""
    c = z.shape[1] // 2
    return dft2(z[:, :c], z[:, c:], inverse=True, scale=scale_of(norm, z.shape[-2] * z.shape[-1], pinv)).real


def mri(x: torch.Tensor, mask: torch.Tensor, norm: str = "ortho") -> torch.Tensor:
    return apply(x, norm) * mask.to(F64)


def mri_adjoint(z: torch.Tensor, mask: torch.Tensor, norm: str = "ortho") -> torch.Tensor:
    return adjoint(z * mask.to(F64), norm)


def torch_fft32(re: torch.Tensor, im: torch.Tensor | None, inverse: bool) -> torch.Tensor:
    r"""torch's own fp32 CPU transform of the same plane(s), unscaled, as complex128."""
    z = re.float() if im is None else torch.complex(re.float(), im.float())
    out = torch.fft.ifft2(z, norm="forward") if inverse else torch.fft.fft2(z)
    return out.to(torch.complex128)


def plane_norm(z: torch.Tensor) -> torch.Tensor:
    r"""The 2-norm of every plane (the last two axes) of a real or complex tensor, in fp64."""
    return (z.real**2 + z.imag**2 if z.is_complex() else z.to(F64) ** 2).sum((-2, -1)).sqrt()


def rule(ref: torch.Tensor, re: torch.Tensor, im: torch.Tensor | None, inverse: bool):
    r"""The accuracy rule's per-plane pieces for the unscaled transform ``ref`` (complex128) of ``re + i im``: ``S``, the norm of
    the full complex result; ``e_ref``, what torch's fp32 CPU transform loses against it, relative to ``S``; and the bound
    ``max(4 e_ref, 2 * 2^-24) * S`` on ``||got - ref||_2``."""
    S = plane_norm(ref)
    e_ref = plane_norm(torch_fft32(re, im, inverse) - ref) / S
    return S, e_ref, torch.maximum(4 * e_ref, torch.full_like(e_ref, 2 * EPS)) * S


def worst_case(H: int, W: int) -> float:
    r"""The worst-case relative error of a radix-2 fp32 transform: ``8 * 2^-24 * (log2 H + log2 W + 1)``."""
    return 8 * EPS * (math.log2(H) + math.log2(W) + 1)
