r"""Measurement operators for the guidance methods: pixel mask, average-pool downsampling, separable blur, general 2-D PSF
(motion blur), decimation (bicubic super-resolution), per-pixel channel mix (colourisation), the 2-D Fourier transform (k-space
undersampling: accelerated MRI), the parallel-beam Radon transform (sparse-view and limited-angle CT) and zero padding, with exact
adjoints and (where one exists) the pseudo-inverse; and the nonlinear ones on :class:`NonlinearOperator`, whose derivative depends
on where it is taken: the magnitude of a split-complex image (Fourier phase retrieval), saturation (HDR) and quantisation.

The guidance classes take the operator :math:`A` of :math:`y = A x + n` as a callable and differentiate it with
``torch.autograd.grad`` (DPS, TMPD, MMPS, JFPS, DiffPIR) and ``torch.func.jvp`` (MMPS, JFPS).  The operators below are such
callables whose maps are kernels of ``csrc/operators.hip``, ``csrc/fft.hip``, ``csrc/coil.hip``, ``csrc/radon.hip`` and
``csrc/nonlinear.hip``: no autograd graph of torch ops, no atomics (two runs give the same bits) and a fixed launch sequence.  The project's own extension: the
reference has no operator library.

    A = DownsampleOperator(2, flatten=True) @ BlurOperator.gaussian(1.0, 5)
    DiffPIRDenoiser(denoiser, y, A, var_y)              # y: (B, D)
    PGDMSampler(denoiser, y, M, M.pinv)                 # M = MaskOperator(mask)
    PSFOperator(motion_psf(31.0, 30.0, 61), flatten=True)                        # motion deblurring
    DecimateOperator(4, 2, flatten=True) @ BlurOperator(bicubic_taps(4))         # bicubic super-resolution x4
    ChannelMixOperator.grayscale(flatten=True)                                   # colourisation
    MRIOperator(cartesian_mask(256, 256, 4), flatten=True)                       # 4x accelerated single-coil MRI
    MultiCoilMRIOperator(cartesian_mask(256, 256, 4), birdcage_maps(8, 256, 256), flatten=True)   # 8-coil SENSE MRI
    RadonOperator(radon_angles(30), (256, 256), flatten=True)                    # sparse-view CT, 30 views
    DPSSampler(denoiser, y, PhaseRetrievalOperator(64, flatten=True))            # phase retrieval, 128 -> 256: 2x oversampling
    DPSSampler(denoiser, y, ClipOperator(gain=2.0, flatten=True))                # HDR: saturation of a twice over-exposed image
    PGDMSampler(denoiser, y, QuantizeOperator(16), lambda y: y)                  # 4-bit images: no derivative of A is taken

Two paths, as ``RePaintSampler`` has them:

* contiguous fp32 device tensors: the kernels, through ONE ``torch.autograd.Function`` whose ``backward`` and ``jvp`` are
  applications of itself (the maps are linear), so ``autograd.grad``, ``torch.func.jvp`` / ``vjp`` and double differentiation all
  end in the same launches;
* everything else (host tensors, fp64 and half tensors): a plain torch op sequence in the tensor's own dtype -- padding, slices,
  reshapes and elementwise ops -- which torch differentiates itself.

How to add an operator: subclass :class:`LinearOperator` and state facts; the base class dispatches, differentiates, checks
shapes and caches.  ``_out_shape`` / ``_in_shape_of`` give the observation's shape and back, and raise for what the operator
cannot take.  ``_kernel(x, mode)`` is the map as launches through :func:`_launch`, ``_torch(x, mode)`` the same map as torch
ops.  ``_TRANSPOSE`` lists every mode the two implement with the mode that is its transpose: ``backward`` looks it up.
``_STRIDED = True`` sends strided fp32 device tensors to the kernels too (made contiguous first) where the torch path has no
use for them, and ``_check_kernel_input`` refuses what the kernels cannot take.  Device constants come from ``_constant``; a
public map of an observation (``pinv``, ``fbp``) is one call of ``_from_observation``.

A nonlinear operator subclasses :class:`NonlinearOperator` the same way, with the map as ``_kernel(x)`` / ``_torch(x)`` and its
linearisation at ``x`` as ``_jac_kernel(x, v, mode)`` / ``_jac_torch(x, v, mode)``; ``N.jacobian(x)`` is a :class:`LinearOperator`,
and ``@`` chains operators of both kinds.
"""

from __future__ import annotations

import ctypes as C
import functools
import math
from collections.abc import Sequence

import torch
import torch.nn.functional as F
from torch import Tensor

from .. import _lib
from .._lib import device_context
from .repaint import _aligned, _broadcasts_to

__all__ = ["LinearOperator", "MaskOperator", "DownsampleOperator", "BlurOperator", "gaussian_taps", "PSFOperator", "motion_psf",
           "DecimateOperator", "bicubic_taps", "ChannelMixOperator", "FourierOperator", "MRIOperator", "cartesian_mask",
           "MultiCoilMRIOperator", "birdcage_maps", "RadonOperator", "radon_angles", "PadOperator", "NonlinearOperator",
           "MagnitudeOperator", "PhaseRetrievalOperator", "ClipOperator", "QuantizeOperator"]

MAX_FACTOR, MAX_TAPS = 16, 65  # (the limits of az_op_avgpool_f32 / az_op_decimate_f32 and of az_op_blur_f32 / az_op_psf_f32)
MAX_CHANNELS = 16  # (the limit of az_op_chanmix_f32)
MAX_FFT = 1024  # (AZ_OP_FFT2_MAX: the largest height or width of az_op_fft2_f32)
MAX_RADON_SIZE, MAX_RADON_DET, MAX_RADON_ANGLES = 1024, 2048, 4096  # (AZ_OP_RADON_MAX_SIZE / _DET / _ANGLES)
MAX_PAD = 1 << 20  # (the limit of az_op_pad_f32 per side)
MAX_LEVELS = 1 << 24  # (QuantizeOperator: the level index is an exact fp32 integer)


def _launch(name: str, *args) -> None:
    r"""Every kernel launch of this module: entry ``name`` of the C ABI on torch's current stream."""
    _lib.call(name, *args, _lib.stream_ptr())


def _use_kernels(x: Tensor) -> bool:
    return x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()


def _to_kernels(x: Tensor, strided: bool) -> bool:
    r"""Whether ``x`` goes to the kernels: a contiguous fp32 device tensor does, a strided one where the caller makes it
    contiguous first."""
    return _use_kernels(x) or (strided and x.is_cuda and x.dtype == torch.float32)


_WITH_PINV = {"apply": "adjoint", "adjoint": "apply", "pinv": "pinv_t", "pinv_t": "pinv"}  # the _TRANSPOSE of a map with a pinv


def _reciprocal_or_zero(t: Tensor) -> Tensor:
    r"""``1 / t`` where ``t`` is nonzero, 0 elsewhere."""
    return torch.where(t != 0, 1 / torch.where(t != 0, t, torch.ones_like(t)), torch.zeros_like(t))


class _Apply(torch.autograd.Function):
    r"""``op``'s map ``mode``, a key of ``op._TRANSPOSE``: on the kernels for the tensors they take (made contiguous and aligned,
    with ``x``'s device current), else as ``op._product``.

    Two reasons for one shape.  ``forward`` always receives plain tensors; ``backward`` and ``jvp`` do NOT: under
    ``torch.func.jvp`` / ``vjp`` theirs are functorch wrappers without storage, so neither may launch on what it receives.
    And ``torch.sparse.mm``, of which :class:`RadonOperator`'s ``_product`` is made, has a backward but no forward-mode rule,
    while ``MMPSDenoiser`` calls ``torch.func.jvp``.  So both are applications of this Function -- the tangent map of a linear
    map is the map, its pullback the transposed map -- which unwraps level by level down to ``forward``."""

    @staticmethod
    def forward(x: Tensor, op: LinearOperator, mode: str) -> Tensor:
        if op._product is not None and not _to_kernels(x, True):  # (without a _product only the kernels' tensors come here)
            return op._product(x, mode)
        with device_context(x):
            return op._kernel(_aligned(x.contiguous(), 16), mode)

    @staticmethod
    def setup_context(ctx, inputs, output) -> None:
        _, ctx.op, ctx.mode = inputs

    @staticmethod
    def backward(ctx, g: Tensor):
        return ctx.op._transposed(g, ctx.mode), None, None

    @staticmethod
    def jvp(ctx, tx: Tensor, *_):
        return _Apply.apply(tx, ctx.op, ctx.mode)


class LinearOperator:
    r"""A linear map on images :math:`(B, C, H, W)` with its adjoint.

    Arguments:
        flatten: Whether the observation is flattened to :math:`(B, D)`, the convention of ``MMPSDenoiser``, ``JFPSDenoiser``
            and ``DiffPIRDenoiser``.  ``adjoint`` and ``pinv`` then accept the flat or the image shape.
        in_shape: The shape :math:`(C, H, W)` of an input, needed to un-flatten an observation.  Taken from the last forward
            call when not given.

    ``A(x)`` applies the operator, ``A.adjoint(v)`` its transpose, ``A.T`` is the transposed operator, ``A.pinv(y)`` the
    pseudo-inverse where one is defined, and ``A2 @ A1`` the composition :math:`x \mapsto A_2(A_1(x))`.
    """

    def __init__(self, flatten: bool = False, in_shape: Sequence[int] | None = None) -> None:
        self.flatten = bool(flatten)
        self.in_shape = None if in_shape is None else tuple(int(s) for s in in_shape)
        if self.in_shape is not None and len(self.in_shape) != 3:
            raise ValueError(f"in_shape is (C, H, W), got {self.in_shape}")
        self._cache: dict = {}

    # -- what a subclass defines ----------------------------------------------------------------------------------------
    _TRANSPOSE: dict[str, str] = {"apply": "adjoint", "adjoint": "apply"}  # every mode of _kernel / _torch -> its transpose
    _STRIDED = False  # whether strided fp32 device tensors go to the kernels (else the torch path takes them without a copy)

    def _out_shape(self, in_shape: tuple) -> tuple:
        r"""(C', H', W') of the observation of a (C, H, W) input; raises ``ValueError`` for an input the operator cannot take."""
        return in_shape

    def _in_shape_of(self, out_shape: tuple) -> tuple:
        r"""(C, H, W) of the input whose observation is (C', H', W')."""
        return out_shape

    def _kernel(self, x: Tensor, mode: str) -> Tensor:
        r"""The map ``mode`` of a contiguous, 16-byte aligned fp32 tensor, as launches through :func:`_launch`."""
        raise NotImplementedError

    def _torch(self, x: Tensor, mode: str) -> Tensor:
        r"""The same map as torch ops in ``x``'s dtype."""
        raise NotImplementedError

    # ``_product(x, mode)``: the map for a tensor that enters :class:`_Apply` and is not the kernels'.  Only an operator whose
    # ``_torch`` is an application of the Function has one.
    _product = None

    def _check_kernel_input(self, x: Tensor) -> None:
        r"""Raises for a tensor that is bound for the kernels and that they cannot take."""

    # -- what the base class does with it -------------------------------------------------------------------------------
    def _transposed(self, g: Tensor, mode: str) -> Tensor:
        r"""The transpose of the map ``mode`` applied to ``g``, as an application of :class:`_Apply`."""
        if mode not in self._TRANSPOSE:
            raise NotImplementedError(f"{type(self).__name__} has no pseudo-inverse")
        return _Apply.apply(g, self, self._TRANSPOSE[mode])

    def _run(self, x: Tensor, mode: str) -> Tensor:
        r"""THE choice between the kernels and the torch path."""
        if _to_kernels(x, self._STRIDED):
            self._check_kernel_input(x)
            return _Apply.apply(x, self, mode)
        return self._torch(x, mode)

    def _constant(self, x: Tensor, tag, make) -> Tensor | tuple:
        r"""The constant ``make()``, a tensor or a tuple of tensors, in ``x``'s dtype on its device, contiguous and 16-byte
        aligned: made and moved once per ``tag``, device and dtype."""
        key = (tag, x.device, x.dtype)
        c = self._cache.get(key)
        if c is None:
            def moved(t: Tensor) -> Tensor:
                t = t.to(device=x.device, dtype=x.dtype)
                return t if t.is_sparse else _aligned(t.contiguous(), 16)

            c = make()
            c = self._cache[key] = moved(c) if torch.is_tensor(c) else tuple(moved(t) for t in c)
        return c

    def _from_observation(self, y: Tensor, mode: str) -> Tensor:
        r"""The map ``mode`` of an observation, flat or in its image shape: the body of the public method of that name."""
        y = self._image(y, mode)
        self._out_shape(self._in_shape_of(tuple(y.shape[1:])))
        return self._run(y, mode)

    def _image(self, v: Tensor, what: str) -> Tensor:
        r"""An observation in its image shape: (B, C', H', W') as it is, (B, D) un-flattened with the recorded input shape."""
        if v.ndim == 4:
            return v
        if v.ndim != 2:
            raise ValueError(f"{what} takes a (B, C, H, W) or a flat (B, D) tensor, got {tuple(v.shape)}")
        if self.in_shape is None:
            raise ValueError(f"{what} of a flat {tuple(v.shape)} tensor needs the image shape: call the operator once or pass "
                             "in_shape=(C, H, W)")
        out = self._out_shape(self.in_shape)
        if v.shape[1] != math.prod(out):
            raise ValueError(f"{what}: {tuple(v.shape)} is not a flattened (B, {', '.join(map(str, out))}) observation")
        return v.unflatten(1, out)

    # -- the public maps ------------------------------------------------------------------------------------------------
    def __call__(self, x: Tensor) -> Tensor:
        if x.ndim != 4:
            raise ValueError(f"{type(self).__name__} takes a (B, C, H, W) tensor, got {tuple(x.shape)}")
        in_shape = tuple(x.shape[1:])
        self._out_shape(in_shape)
        self.in_shape = in_shape
        y = self._run(x, "apply")
        return y.flatten(1) if self.flatten else y

    def adjoint(self, v: Tensor) -> Tensor:
        return self._from_observation(v, "adjoint")

    def pinv(self, y: Tensor) -> Tensor:
        raise NotImplementedError(f"{type(self).__name__} has no pseudo-inverse")

    @property
    def T(self) -> LinearOperator:
        return _Transposed(self)

    def __matmul__(self, other: LinearOperator) -> LinearOperator:
        if not isinstance(other, LinearOperator):
            return NotImplemented
        return _Composition(self, other)


class _Transposed(LinearOperator):
    r"""``A.T``: the call is ``A.adjoint``, the adjoint is ``A``, and ``.T`` is ``A`` itself."""

    def __init__(self, base: LinearOperator) -> None:
        super().__init__()
        self.base = base

    def __call__(self, v: Tensor) -> Tensor:
        return self.base.adjoint(v)

    def adjoint(self, x: Tensor) -> Tensor:
        return self.base(x)

    @property
    def T(self) -> LinearOperator:
        return self.base


class _Composition(LinearOperator):
    r"""``A2 @ A1``: :math:`x \mapsto A_2(A_1(x))`; the adjoint runs the two adjoints in reverse.  No pseudo-inverse."""

    def __init__(self, outer: LinearOperator, inner: LinearOperator) -> None:
        super().__init__()
        self.outer, self.inner = outer, inner

    def __call__(self, x: Tensor) -> Tensor:
        return self.outer(self.inner(x))

    def adjoint(self, v: Tensor) -> Tensor:
        return self.inner.adjoint(self.outer.adjoint(v))


# ------------------------------------------------------------------------------------------------------------------ mask
class MaskOperator(LinearOperator):
    r"""Creates the pixel mask :math:`x \mapsto m \odot x` (inpainting).  Self-adjoint.

    Arguments:
        mask: The mask :math:`m`, bool or float, broadcastable to the input.
        flatten, in_shape: See :class:`LinearOperator`.

    ``pinv`` multiplies by :math:`1 / m` where :math:`m \neq 0` and by 0 elsewhere.  The factor is made once per device, dtype
    and (where it has to be expanded) input shape: build a new operator for a new mask rather than editing ``mask`` in place.
    """

    _TRANSPOSE = {"apply": "adjoint", "adjoint": "apply", "pinv": "pinv"}  # (diagonal maps: "adjoint" is "apply")

    def __init__(self, mask: Tensor, flatten: bool = False, in_shape: Sequence[int] | None = None) -> None:
        super().__init__(flatten, in_shape)
        if not torch.is_tensor(mask) or mask.ndim > 4:
            raise ValueError("mask is a tensor of at most 4 dimensions")
        self.mask = mask

    def _factor(self, x: Tensor, inverse: bool, kernels: bool) -> Tensor:
        r"""The factor in ``x``'s dtype, on ``x``'s device.  For the kernels: either a suffix of ``x``'s shape (the kernel indexes
        it modulo its size) or expanded to ``x``'s shape, then made once per shape as well."""
        core = tuple(self.mask.shape)
        while core and core[0] == 1:
            core = core[1:]
        suffix = core == tuple(x.shape[x.ndim - len(core):])

        def make() -> Tensor:
            m = self.mask.to(device=x.device, dtype=x.dtype)  # (first: the reciprocal is taken in x's dtype)
            if inverse:
                m = _reciprocal_or_zero(m)
            return (m.reshape(core) if suffix else m.expand(x.shape)) if kernels else m

        return self._constant(x, ("factor", inverse, kernels, tuple(x.shape) if kernels and not suffix else None), make)

    def _out_shape(self, in_shape: tuple) -> tuple:
        if not _broadcasts_to(self.mask.shape[-3:], in_shape):  # (the batch dimension: _check_batch)
            raise ValueError(f"a mask of shape {tuple(self.mask.shape)} does not broadcast to (B, {', '.join(map(str, in_shape))})")
        return in_shape

    def _check_batch(self, x: Tensor) -> None:
        if not _broadcasts_to(self.mask.shape, x.shape):
            raise ValueError(f"a mask of shape {tuple(self.mask.shape)} does not broadcast to {tuple(x.shape)}")

    def _kernel(self, x: Tensor, mode: str) -> Tensor:
        self._check_batch(x)
        m = self._factor(x, mode == "pinv", True)
        y = torch.empty_like(x)
        if x.numel():
            _launch("az_op_mul_f32", y.data_ptr(), x.data_ptr(), m.data_ptr(), x.numel(), m.numel())
        return y

    def _torch(self, x: Tensor, mode: str) -> Tensor:
        self._check_batch(x)
        return x * self._factor(x, mode == "pinv", False)

    def pinv(self, y: Tensor) -> Tensor:
        return self._from_observation(y, "pinv")


# ------------------------------------------------------------------------------------------------------------ downsample
def _pair(v, what: str) -> tuple:
    pair = (v, v) if isinstance(v, int) else tuple(v) if isinstance(v, Sequence) else ()
    if len(pair) != 2 or not all(isinstance(a, int) for a in pair):
        raise ValueError(f"{what} is an int or a pair of ints, got {v}")
    return pair


class _SubsampleOperator(LinearOperator):
    r"""What :class:`DownsampleOperator` and :class:`DecimateOperator` share: the factor and the two shapes."""

    _NAME = ""  # (the operator's own word in the "multiples" message)

    def __init__(self, factor: int | Sequence[int], flatten: bool = False, in_shape: Sequence[int] | None = None) -> None:
        super().__init__(flatten, in_shape)
        fh, fw = _pair(factor, "factor")
        if not (1 <= fh <= MAX_FACTOR and 1 <= fw <= MAX_FACTOR):
            raise ValueError(f"factor is an int or a pair of ints in 1 .. {MAX_FACTOR}, got {factor}")
        self.factor = (fh, fw)

    def _out_shape(self, in_shape: tuple) -> tuple:
        (c, h, w), (fh, fw) = in_shape, self.factor
        if h % fh or w % fw:
            raise ValueError(f"{self._NAME} by {self.factor} needs a height and width that are multiples of it, got {h} x {w}")
        return (c, h // fh, w // fw)

    def _in_shape_of(self, out_shape: tuple) -> tuple:
        return (out_shape[0], out_shape[1] * self.factor[0], out_shape[2] * self.factor[1])


class DownsampleOperator(_SubsampleOperator):
    r"""Creates the average-pool downsampling by ``factor`` (super-resolution).

    Arguments:
        factor: The factor, an int or ``(fh, fw)``, each in 1 .. 16.  The input's height and width are multiples of it.
        flatten, in_shape: See :class:`LinearOperator`.

    ``pinv`` is nearest up-sampling, :math:`f_h f_w` times the adjoint.
    """

    _NAME = "downsampling"
    _TRANSPOSE = _WITH_PINV

    def _kernel(self, x: Tensor, mode: str) -> Tensor:
        (B, c, h, w), (fh, fw) = x.shape, self.factor
        if mode in ("apply", "pinv_t"):
            y = x.new_empty(B, c, h // fh, w // fw)
            if y.numel():
                _launch("az_op_avgpool_f32", y.data_ptr(), x.data_ptr(), B * c, h, w, fh, fw)
            # "pinv_t" is (fh fw A^T)^T = fh fw A.  The entry has no scale argument, so the factor is a torch multiply and the
            # launch sequence stays az_op_avgpool_f32 alone.
            return y * float(fh * fw) if mode == "pinv_t" else y
        y = x.new_empty(B, c, h * fh, w * fw)
        if y.numel():
            scale = 1.0 if mode == "pinv" else 1.0 / (fh * fw)
            _launch("az_op_avgpool_adj_f32", y.data_ptr(), x.data_ptr(), B * c, h * fh, w * fw, fh, fw, scale)
        return y

    def _torch(self, x: Tensor, mode: str) -> Tensor:
        (B, c, h, w), (fh, fw) = x.shape, self.factor
        if mode in ("apply", "pinv_t"):
            win = x.reshape(B, c, h // fh, fh, w // fw, fw)
            acc = None
            for a in range(fh):  # (the kernel's order of summation)
                for b in range(fw):
                    acc = win[:, :, :, a, :, b] if acc is None else acc + win[:, :, :, a, :, b]
            y = acc * (1.0 / (fh * fw))
            return y * float(fh * fw) if mode == "pinv_t" else y  # (as the kernel path: the apply map, then the factor)
        up = x[:, :, :, None, :, None].expand(B, c, h, fh, w, fw).reshape(B, c, h * fh, w * fw)
        return up if mode == "pinv" else up * (1.0 / (fh * fw))

    def pinv(self, y: Tensor) -> Tensor:
        return self._from_observation(y, "pinv")


# ------------------------------------------------------------------------------------------------------------------ blur
def gaussian_taps(sigma: float, size: int) -> Tensor:
    r"""``size`` samples of a centred Gaussian of standard deviation ``sigma`` (in pixels), computed in fp64, normalised to sum 1
    and then rounded to fp32."""
    if size < 1 or sigma <= 0:
        raise ValueError(f"gaussian_taps needs size >= 1 and sigma > 0, got size {size}, sigma {sigma}")
    pos = torch.arange(size, dtype=torch.float64) - (size - 1) / 2
    k = torch.exp(-0.5 * (pos / sigma) ** 2)
    return (k / k.sum()).to(torch.float32)


def _padding(padding: str) -> str:
    if padding not in ("zeros", "circular"):
        raise ValueError(f"padding is 'zeros' or 'circular', got {padding!r}")
    return padding


def _pad(x: Tensor, rh: int, rw: int, padding: str) -> Tensor:
    r"""``x`` with ``rh`` rows and ``rw`` columns of ``padding`` on every side, for the torch paths."""
    return F.pad(x, (rw, rw, rh, rh), mode="circular") if padding == "circular" else F.pad(x, (rw, rw, rh, rh))


def _tile(entry: str, nh: int, nw: int) -> tuple[int, int]:
    th, tw = C.c_int32(0), C.c_int32(0)
    _lib.call(entry, nh, nw, C.byref(th), C.byref(tw))
    return th.value, tw.value


class BlurOperator(LinearOperator):
    r"""Creates a separable blur of the input's size: the correlation
    :math:`y_{ij} = \sum_a h_a \sum_b w_b \, \tilde x_{i + a - r_h, j + b - r_w}` with the radii :math:`r = \lfloor n / 2 \rfloor`.

    Arguments:
        taps_h: The vertical taps, an odd number of them, at most 65.  Any values: symmetry is not assumed.
        taps_w: The horizontal taps (``taps_h`` when ``None``).
        padding: ``"zeros"`` (:math:`\tilde x = 0` outside the image) or ``"circular"`` (wrapped; the radii are smaller than the
            image).
        flatten, in_shape: See :class:`LinearOperator`.

    The adjoint is the same correlation with both tap vectors reversed, for both paddings.  There is no ``pinv``.
    """

    def __init__(self, taps_h, taps_w=None, padding: str = "zeros", flatten: bool = False,
                 in_shape: Sequence[int] | None = None) -> None:
        super().__init__(flatten, in_shape)
        self.padding = _padding(padding)
        taps = []
        for t in (taps_h, taps_h if taps_w is None else taps_w):
            t = torch.as_tensor(t).detach().to(device="cpu", dtype=torch.float32).contiguous()
            if t.ndim != 1 or t.numel() % 2 == 0 or t.numel() > MAX_TAPS:
                raise ValueError(f"taps are 1-d vectors of an odd length of at most {MAX_TAPS}, got shape {tuple(t.shape)}")
            taps.append(t)
        self.taps_h, self.taps_w = taps

    @classmethod
    def gaussian(cls, sigma: float, size: int, **kwargs) -> BlurOperator:
        r"""A Gaussian blur: ``gaussian_taps(sigma, size)`` along both axes."""
        return cls(gaussian_taps(sigma, size), **kwargs)

    def _taps(self, x: Tensor, mode: str) -> tuple[Tensor, Tensor]:
        hw = self.taps_h, self.taps_w
        return self._constant(x, ("taps", mode), lambda: hw if mode == "apply" else tuple(t.flip(0) for t in hw))

    def _out_shape(self, in_shape: tuple) -> tuple:
        _, h, w = in_shape
        rh, rw = self.taps_h.numel() // 2, self.taps_w.numel() // 2
        if self.padding == "circular" and (rh >= h or rw >= w):
            raise ValueError(f"circular padding needs radii ({rh}, {rw}) smaller than the image, got {h} x {w}")
        return in_shape

    def _kernel(self, x: Tensor, mode: str) -> Tensor:
        B, c, h, w = x.shape
        th, tw = self._taps(x, mode)
        y = torch.empty_like(x)
        if x.numel():
            _launch("az_op_blur_f32", y.data_ptr(), x.data_ptr(), th.data_ptr(), th.numel(), tw.data_ptr(), tw.numel(), B * c, h, w,
                    int(self.padding == "circular"))
        return y

    def _torch(self, x: Tensor, mode: str) -> Tensor:
        h, w = x.shape[2:]
        th, tw = self._taps(x, mode)
        xp = _pad(x, th.numel() // 2, tw.numel() // 2, self.padding)
        rows = None
        for b in range(tw.numel()):  # (the kernel's two passes; torch rounds the product where the kernel fuses it)
            term = tw[b] * xp[:, :, :, b:b + w]
            rows = term if rows is None else rows + term
        out = None
        for a in range(th.numel()):
            term = th[a] * rows[:, :, a:a + h, :]
            out = term if out is None else out + term
        return out


def blur_tile(nh: int, nw: int) -> tuple[int, int]:
    r"""The output tile (rows, columns) of one workgroup of ``az_op_blur_f32`` for these tap counts."""
    return _tile("az_op_blur_tile", nh, nw)


# ------------------------------------------------------------------------------------------------------------------- PSF
def motion_psf(length: float, angle: float, size: int) -> Tensor:
    r"""A ``size`` x ``size`` line PSF (linear motion blur): a centred segment that covers ``length`` pixels, at ``angle``
    degrees counter-clockwise from the horizontal axis, rasterised bilinearly -- 8 samples per pixel of length, each shared
    between its four neighbouring pixels -- in fp64, normalised to sum 1 and then rounded to fp32.  Deterministic: no random
    numbers.  ``angle = 0`` gives one row."""
    if size < 1 or size % 2 == 0 or not 1 <= length <= size:
        raise ValueError(f"motion_psf needs an odd size >= 1 and 1 <= length <= size, got size {size}, length {length}")
    n = 8 * math.ceil(length) + 1
    s = torch.linspace(-0.5, 0.5, n, dtype=torch.float64) * (length - 1)
    rad = math.radians(angle)
    right = {0.0: (1.0, 0.0), 90.0: (0.0, 1.0), 180.0: (-1.0, 0.0), 270.0: (0.0, -1.0)}  # (cos(pi / 2) is 6e-17 in fp64)
    cos, sin = right.get(angle % 360.0, (math.cos(rad), math.sin(rad)))
    c = (size - 1) / 2
    px, py = c + s * cos, c - s * sin
    x0, y0 = px.floor(), py.floor()
    fx, fy = px - x0, py - y0
    k = torch.zeros(size * size, dtype=torch.float64)
    for dy, wy in ((0, 1 - fy), (1, fy)):
        for dx, wx in ((0, 1 - fx), (1, fx)):
            xi, yi = (x0 + dx).long(), (y0 + dy).long()
            keep = (xi >= 0) & (xi < size) & (yi >= 0) & (yi < size)  # (a weight-0 neighbour may lie outside)
            k.index_add_(0, (yi * size + xi)[keep], (wy * wx)[keep])
    return (k / k.sum()).reshape(size, size).to(torch.float32)


class PSFOperator(LinearOperator):
    r"""Creates the blur by a general two-dimensional point-spread function (motion deblurring): the correlation
    :math:`y_{bcij} = \sum_a \sum_{b'} k_{bc, a b'} \, \tilde x_{bc, i + a - r_h, j + b' - r_w}` of the input's size, with
    the radii :math:`r = \lfloor k / 2 \rfloor`.

    Arguments:
        psf: The PSF: :math:`(k_h, k_w)` (one for all planes), :math:`(C, k_h, k_w)` (one per channel),
            :math:`(B, 1, k_h, k_w)` (one per sample) or :math:`(B, C, k_h, k_w)` (one per plane).  Odd sizes of at most 65,
            any values.  See :func:`motion_psf`.
        padding: ``"zeros"`` or ``"circular"``, as for :class:`BlurOperator`.
        flatten, in_shape: See :class:`LinearOperator`.

    Every output is one chain of :math:`k_h k_w` fused multiply-adds from 0, over :math:`a` and then :math:`b'`, ascending.  The
    adjoint is the same correlation with the PSF flipped along both axes, for both paddings.  There is no ``pinv``.
    """

    def __init__(self, psf: Tensor, padding: str = "zeros", flatten: bool = False, in_shape: Sequence[int] | None = None) -> None:
        super().__init__(flatten, in_shape)
        self.padding = _padding(padding)
        k = torch.as_tensor(psf).detach().to(device="cpu", dtype=torch.float32)
        if k.ndim not in (2, 3, 4) or k.shape[-2] % 2 == 0 or k.shape[-1] % 2 == 0 or max(k.shape[-2:]) > MAX_TAPS or k.numel() == 0:
            raise ValueError("psf is (kh, kw), (C, kh, kw), (B, 1, kh, kw) or (B, C, kh, kw) with odd kh, kw of at most "
                             f"{MAX_TAPS}, got shape {tuple(k.shape)}")
        self.psf = k.reshape((1,) * (4 - k.ndim) + tuple(k.shape)).contiguous()  # (Bp, Cp, kh, kw)

    def _taps(self, x: Tensor, mode: str) -> Tensor:
        return self._constant(x, ("taps", mode), lambda: self.psf if mode == "apply" else self.psf.flip(2, 3))

    def _out_shape(self, in_shape: tuple) -> tuple:
        c, h, w = in_shape
        (_, cp, kh, kw) = self.psf.shape
        if cp not in (1, c):
            raise ValueError(f"a psf of shape {tuple(self.psf.shape)} is for {cp} channels, got {c}")
        if self.padding == "circular" and (kh // 2 >= h or kw // 2 >= w):
            raise ValueError(f"circular padding needs radii ({kh // 2}, {kw // 2}) smaller than the image, got {h} x {w}")
        return in_shape

    def _check_batch(self, x: Tensor) -> None:
        if self.psf.shape[0] not in (1, x.shape[0]):
            raise ValueError(f"a psf of shape {tuple(self.psf.shape)} is for a batch of {self.psf.shape[0]}, got {tuple(x.shape)}")

    def _kernel(self, x: Tensor, mode: str) -> Tensor:
        self._check_batch(x)
        B, c, h, w = x.shape
        k = self._taps(x, mode)
        bp, cp, kh, kw = k.shape
        y = torch.empty_like(x)
        if x.numel():
            _launch("az_op_psf_f32", y.data_ptr(), x.data_ptr(), k.data_ptr(), kh, kw, cp if bp > 1 else 0, int(cp > 1), B, c, h, w,
                    int(self.padding == "circular"))
        return y

    def _torch(self, x: Tensor, mode: str) -> Tensor:
        self._check_batch(x)
        h, w = x.shape[2:]
        k = self._taps(x, mode)
        kh, kw = k.shape[2:]
        xp = _pad(x, kh // 2, kw // 2, self.padding)
        out = None
        for a in range(kh):  # (the kernel's order; torch rounds the product where the kernel fuses it)
            for b in range(kw):
                term = k[:, :, a, b, None, None] * xp[:, :, a:a + h, b:b + w]
                out = term if out is None else out + term
        return out


def psf_tile(kh: int, kw: int) -> tuple[int, int]:
    r"""The output tile (rows, columns) of one workgroup of ``az_op_psf_f32`` for this PSF size."""
    return _tile("az_op_psf_tile", kh, kw)


# ------------------------------------------------------------------------------------------------------------- decimation
def bicubic_taps(factor: int) -> Tensor:
    r"""The ``4 factor + 1`` taps of the bicubic low-pass of a down-sampling by ``factor``: the Keys kernel (:math:`a = -0.5`)
    stretched by ``factor`` and sampled at the integers :math:`-2 f .. 2 f` (the two end taps are 0: the count stays odd),
    computed in fp64, normalised to sum 1 and then rounded to fp32."""
    if not (isinstance(factor, int) and 1 <= factor <= MAX_FACTOR):
        raise ValueError(f"bicubic_taps needs an int factor in 1 .. {MAX_FACTOR}, got {factor}")
    t = (torch.arange(-2 * factor, 2 * factor + 1, dtype=torch.float64) / factor).abs()
    a = -0.5
    k = torch.where(t <= 1, ((a + 2) * t - (a + 3)) * t * t + 1, ((a * t - 5 * a) * t + 8 * a) * t - 4 * a)
    k = torch.where(t < 2, k, torch.zeros_like(k))
    return (k / k.sum()).to(torch.float32)


class DecimateOperator(_SubsampleOperator):
    r"""Creates the decimation :math:`y_{ij} = x_{i f_h + o_h, j f_w + o_w}`: keep every ``factor``-th pixel, starting at
    ``offset`` (where :class:`DownsampleOperator` averages each window).

    Arguments:
        factor: The factor, an int or ``(fh, fw)``, each in 1 .. 16.  The input's height and width are multiples of it.
        offset: The first kept row and column, an int or ``(oh, ow)`` with ``0 <= oh < fh`` and ``0 <= ow < fw``.
        flatten, in_shape: See :class:`LinearOperator`.

    The adjoint stuffs zeros between the values.  :math:`A A^\top = I`, so ``pinv`` is the adjoint.

    Bicubic super-resolution by ``f`` is ``DecimateOperator(f, f // 2) @ BlurOperator(bicubic_taps(f))``: the bicubic low-pass,
    then every ``f``-th pixel.  The composition computes :math:`f^2` times more blur outputs than it keeps; a fused strided
    blur is not provided.
    """

    _NAME = "decimation"

    def __init__(self, factor: int | Sequence[int], offset: int | Sequence[int] = 0, flatten: bool = False,
                 in_shape: Sequence[int] | None = None) -> None:
        super().__init__(factor, flatten, in_shape)
        oh, ow = _pair(offset, "offset")
        if not (0 <= oh < self.factor[0] and 0 <= ow < self.factor[1]):
            raise ValueError(f"offset is an int or a pair of ints with 0 <= offset < factor, got {offset} for factor {factor}")
        self.offset = (oh, ow)

    def _kernel(self, x: Tensor, mode: str) -> Tensor:
        (B, c, h, w), (fh, fw), (oh, ow) = x.shape, self.factor, self.offset
        if mode == "apply":
            y = x.new_empty(B, c, h // fh, w // fw)
            if y.numel():
                _launch("az_op_decimate_f32", y.data_ptr(), x.data_ptr(), B * c, h, w, fh, fw, oh, ow)
            return y
        y = x.new_empty(B, c, h * fh, w * fw)
        if y.numel():
            _launch("az_op_decimate_adj_f32", y.data_ptr(), x.data_ptr(), B * c, h * fh, w * fw, fh, fw, oh, ow)
        return y

    def _torch(self, x: Tensor, mode: str) -> Tensor:
        (B, c, h, w), (fh, fw), (oh, ow) = x.shape, self.factor, self.offset
        if mode == "apply":
            return x[:, :, oh::fh, ow::fw]
        win = F.pad(x[:, :, :, None, :, None], (ow, fw - 1 - ow, 0, 0, oh, fh - 1 - oh))  # (B, c, h, fh, w, fw)
        return win.reshape(B, c, h * fh, w * fw)

    def pinv(self, y: Tensor) -> Tensor:
        return self.adjoint(y)


# ------------------------------------------------------------------------------------------------------------ channel mix
class ChannelMixOperator(LinearOperator):
    r"""Creates the per-pixel channel mix :math:`y_{b o p} = \sum_c M_{o c} \, x_{b c p}` (colourisation: 3 channels to 1).

    Arguments:
        matrix: The matrix :math:`M`, of shape :math:`(C_{out}, C_{in})`, each at most 16.
        flatten, in_shape: See :class:`LinearOperator`.

    Every output is a chain of fused multiply-adds from 0 with :math:`c` ascending.  The adjoint mixes with :math:`M^\top`;
    ``pinv`` mixes with :math:`M^+`, ``torch.linalg.pinv`` of the matrix in fp64, computed once on the host.
    """

    _TRANSPOSE = _WITH_PINV

    def __init__(self, matrix, flatten: bool = False, in_shape: Sequence[int] | None = None) -> None:
        super().__init__(flatten, in_shape)
        m = torch.as_tensor(matrix).detach().to(device="cpu", dtype=torch.float64)
        if m.ndim != 2 or not (1 <= m.shape[0] <= MAX_CHANNELS and 1 <= m.shape[1] <= MAX_CHANNELS):
            raise ValueError(f"matrix is (Cout, Cin) with 1 .. {MAX_CHANNELS} channels each, got shape {tuple(m.shape)}")
        self.matrix = m.contiguous()

    @classmethod
    def grayscale(cls, weights: Sequence[float] = (1 / 3, 1 / 3, 1 / 3), **kwargs) -> ChannelMixOperator:
        r"""The colourisation operator: one channel, the weighted sum of the input's ``len(weights)`` channels."""
        return cls(torch.tensor([list(weights)], dtype=torch.float64), **kwargs)

    def _matrix(self, x: Tensor, mode: str) -> Tensor:
        def make() -> Tensor:
            m = self.matrix if mode in ("apply", "adjoint") else torch.linalg.pinv(self.matrix).T  # M or (M^+)^T: (Cout, Cin)
            return m.T if mode in ("adjoint", "pinv") else m

        return self._constant(x, ("matrix", mode), make)

    def _out_shape(self, in_shape: tuple) -> tuple:
        if in_shape[0] != self.matrix.shape[1]:
            raise ValueError(f"a matrix of shape {tuple(self.matrix.shape)} mixes {self.matrix.shape[1]} channels, got {in_shape[0]}")
        return (self.matrix.shape[0], *in_shape[1:])

    def _in_shape_of(self, out_shape: tuple) -> tuple:
        if out_shape[0] != self.matrix.shape[0]:
            raise ValueError(f"a matrix of shape {tuple(self.matrix.shape)} gives {self.matrix.shape[0]} channels, got {out_shape[0]}")
        return (self.matrix.shape[1], *out_shape[1:])

    def _kernel(self, x: Tensor, mode: str) -> Tensor:
        B, c, h, w = x.shape
        m = self._matrix(x, mode)
        y = x.new_empty(B, m.shape[0], h, w)
        if y.numel():
            _launch("az_op_chanmix_f32", y.data_ptr(), x.data_ptr(), m.data_ptr(), B, c, m.shape[0], h * w)
        return y

    def _torch(self, x: Tensor, mode: str) -> Tensor:
        m = self._matrix(x, mode)
        rows = []
        for o in range(m.shape[0]):
            acc = None
            for c in range(m.shape[1]):  # (the kernel's order; torch rounds the product where the kernel fuses it)
                term = m[o, c] * x[:, c]
                acc = term if acc is None else acc + term
            rows.append(acc)
        return torch.stack(rows, dim=1)

    def pinv(self, y: Tensor) -> Tensor:
        return self._from_observation(y, "pinv")


# --------------------------------------------------------------------------------------------------------------- Fourier
def _fft_kernel_size(n: int) -> bool:
    return 1 <= n <= MAX_FFT and n & (n - 1) == 0


def _check_fft_input(op: LinearOperator, x: Tensor) -> None:
    r"""``_check_kernel_input`` of the operators on ``az_op_fft2_f32``."""
    h, w = x.shape[2:]
    if not (_fft_kernel_size(h) and _fft_kernel_size(w)):
        raise NotImplementedError(f"{type(op).__name__} on an fp32 device tensor needs a height and width that are powers of two "
                                  f"of at most {MAX_FFT}, got {h} x {w}; host and fp64 tensors take any size")


# Planes as ``az_op_fft2_f32`` and the coil entries receive them are a triple (re pointer, im pointer, floats from one sample to the
# next); real planes have the im pointer ``None``.  A split-complex (B, 2 C, H, W) buffer is (tensors, planes): the two halves of
# ONE tensor where both start 16-byte aligned, else two tensors of (B, C, H, W).  Plain tuples, unpacked into names where they are
# made: the host side of a call costs as much time as its launch, and a class instance per buffer adds a tenth to it.
def _halves_aligned(n: int) -> bool:
    return n % 4 == 0  # (n = C H W floats per half and sample)


def _split_empty(x: Tensor, B: int, c: int, h: int, w: int) -> tuple[tuple, tuple]:
    r"""An uninitialised split-complex (B, 2 c, h, w) buffer like ``x``: (tensors, planes)."""
    n = c * h * w
    if _halves_aligned(n):
        whole = _aligned(x.new_empty(B, 2 * c, h, w), 16)
        return (whole,), (whole.data_ptr(), whole.data_ptr() + 4 * n, 2 * n)
    re, im = _aligned(x.new_empty(B, c, h, w), 16), _aligned(x.new_empty(B, c, h, w), 16)
    return (re, im), (re.data_ptr(), im.data_ptr(), n)


def _split_of(v: Tensor, c: int, n: int) -> tuple[tuple, tuple]:
    r"""The contiguous, aligned (B, 2 c, h, w) tensor ``v``, ``n = c h w``, as a split-complex buffer, (tensors, planes): in
    place, or its halves copied."""
    if _halves_aligned(n):
        return (v,), (v.data_ptr(), v.data_ptr() + 4 * n, 2 * n)
    re, im = _aligned(v[:, :c].contiguous(), 16), _aligned(v[:, c:].contiguous(), 16)
    return (re, im), (re.data_ptr(), im.data_ptr(), n)


def _whole(tensors: tuple) -> Tensor:
    r"""The (B, 2 C, H, W) tensor of a split-complex buffer's tensors."""
    return tensors[0] if len(tensors) == 1 else _aligned(torch.cat(tensors, dim=1), 16)


def _fft2(dst: tuple, src: tuple, like: Tensor, B: int, c: int, h: int, w: int, inverse: int, scale: float) -> None:
    r"""One ``az_op_fft2_f32`` launch on ``B c`` planes from the planes ``src`` to the planes ``dst``.  Real ``dst`` planes (the real
    part of an inverse transform) need scratch: ``az_op_fft2_work`` says how much, and it is made like ``like``."""
    work = None
    if dst[1] is None:
        floats = C.c_int64(0)
        _lib.call("az_op_fft2_work", B, c, h, w, C.byref(floats))
        work = _aligned(like.new_empty(floats.value), 16) if floats.value else None
    _launch("az_op_fft2_f32", *dst, *src, None if work is None else work.data_ptr(), B, c, h, w, inverse, scale)


class FourierOperator(LinearOperator):
    r"""Creates the 2-D discrete Fourier transform of a real image in split-complex form: a :math:`(B, C, H, W)` input gives a
    :math:`(B, 2 C, H, W)` observation whose channels :math:`[0, C)` are :math:`\Re F x` and :math:`[C, 2 C)` are
    :math:`\Im F x`, with :math:`(F x)_{kl} = s \sum_{mn} x_{mn} e^{-2 \pi i (k m / H + l n / W)}`.  The DC term is at
    :math:`[0, 0]`: there is no shift.  Everything stays real and 4-D, so :class:`MaskOperator`, ``flatten`` and compositions
    apply to the observation as to any other.

    Arguments:
        norm: As in ``torch.fft``: ``"ortho"`` (:math:`s = 1 / \sqrt{H W}`, :math:`A^\top A = I` and ``pinv`` is the
            adjoint), ``"backward"`` (:math:`s = 1`, ``pinv`` is the adjoint divided by :math:`H W`) or ``"forward"``
            (:math:`s = 1 / (H W)`, ``pinv`` is :math:`H W` times the adjoint).
        flatten, in_shape: See :class:`LinearOperator`.

    The adjoint maps :math:`(B, 2 C, H, W)` to :math:`(B, C, H, W)` as :math:`s \, \Re F^H (z_{re} + i z_{im})`: one inverse
    transform whose imaginary part is never written.

    Every fp32 device tensor takes ``az_op_fft2_f32`` (made contiguous and aligned first), whose heights and widths are powers
    of two up to 1024; any other size of such a tensor raises ``NotImplementedError`` -- there is no vendor-FFT fallback on that
    path.  Host and fp64 tensors run ``torch.fft`` in their own dtype at any size; half precision is not provided.

    Out of scope: non-power-of-two sizes on the device, ``fftshift``-ed layouts, nonlinear phase retrieval, 3-D transforms, and
    an FFT-based ``pinv`` for the circular :class:`BlurOperator`.  Coil sensitivity maps: :class:`MultiCoilMRIOperator`.
    """

    _TRANSPOSE = _WITH_PINV
    _STRIDED = True  # (a strided view too: the Function makes it contiguous)
    _check_kernel_input = _check_fft_input

    def __init__(self, norm: str = "ortho", flatten: bool = False, in_shape: Sequence[int] | None = None) -> None:
        super().__init__(flatten, in_shape)
        if norm not in ("ortho", "backward", "forward"):
            raise ValueError(f"norm is 'ortho', 'backward' or 'forward', got {norm!r}")
        self.norm = norm

    def _scale(self, hw: int, mode: str) -> float:
        r"""The factor of the map ``mode``; "pinv_t" is the transpose of "pinv": the apply map at the pinv's scale."""
        if self.norm == "ortho":
            return 1.0 / math.sqrt(hw)
        if mode in ("apply", "adjoint"):
            return 1.0 if self.norm == "backward" else 1.0 / hw
        return 1.0 / hw if self.norm == "backward" else 1.0

    def _out_shape(self, in_shape: tuple) -> tuple:
        return (2 * in_shape[0], *in_shape[1:])

    def _in_shape_of(self, out_shape: tuple) -> tuple:
        if out_shape[0] % 2:
            raise ValueError(f"a split-complex observation has an even channel count (re, then im), got {out_shape[0]}")
        return (out_shape[0] // 2, *out_shape[1:])

    def _kernel(self, x: Tensor, mode: str) -> Tensor:
        B, c, h, w = x.shape
        scale = self._scale(h * w, mode)
        if mode in ("apply", "pinv_t"):  # real -> split complex
            y, y_planes = _split_empty(x, B, c, h, w)
            if x.numel():
                _fft2(y_planes, (x.data_ptr(), None, c * h * w), x, B, c, h, w, 0, scale)
            return _whole(y)
        c //= 2  # split complex -> real: the inverse transform's real part
        y = _aligned(x.new_empty(B, c, h, w), 16)
        if y.numel():
            z, z_planes = _split_of(x, c, c * h * w)  # (z: the halves stay alive until the launch is queued)
            _fft2((y.data_ptr(), None, c * h * w), z_planes, x, B, c, h, w, 1, scale)
        return y

    def _torch(self, x: Tensor, mode: str) -> Tensor:
        if x.dtype not in (torch.float32, torch.float64):
            raise NotImplementedError(f"FourierOperator runs in fp32 and fp64, got {x.dtype}")
        h, w = x.shape[2:]
        scale = self._scale(h * w, mode)
        if mode in ("apply", "pinv_t"):
            f = torch.fft.fft2(x)
            return torch.cat([f.real, f.imag], dim=1) * scale
        c = x.shape[1] // 2
        return torch.fft.ifft2(torch.complex(x[:, :c], x[:, c:]), norm="forward").real * scale  # ("forward": unscaled inverse)

    def pinv(self, y: Tensor) -> Tensor:
        return self._from_observation(y, "pinv")


def cartesian_mask(H: int, W: int, acceleration: float, center_fraction: float = 0.08, seed: int = 0) -> Tensor:
    r"""A :math:`(H, W)` 0/1 fp32 mask of whole columns in DFT order (column :math:`l` is the frequency :math:`l` for
    :math:`l \le W / 2` and :math:`l - W` above): Cartesian undersampling of k-space by about ``acceleration``.

    The band :math:`|f| \le c`, :math:`c = \lfloor n_c / 2 \rfloor` with :math:`n_c` = ``center_fraction * W`` rounded half
    up, is always kept: :math:`\min(W, 2 c + 1)` columns that hold the :math:`n_c` lowest frequencies.  The others are drawn in
    pairs :math:`\pm f`, :math:`c < f < W / 2` (the Nyquist column has no partner and is never drawn), without replacement by a
    CPU ``torch.Generator`` seeded with ``seed``: the mask is symmetric under :math:`l \to -l \bmod W` and the same on every
    machine.  With :math:`P = \max(0, \lfloor (W - 1) / 2 \rfloor - c)` such pairs and :math:`n` = ``W / acceleration`` rounded
    half up, the number of kept columns is :math:`\min(W, 2 c + 1) + 2 \min(P, \max(0, \lfloor (n - (2 c + 1)) / 2 \rfloor))`
    (:func:`cartesian_columns`)."""
    cols = cartesian_columns(W, acceleration, center_fraction)  # (validates)
    if H < 1:
        raise ValueError(f"cartesian_mask needs H >= 1, got {H}")
    c = int(math.floor(center_fraction * W + 0.5)) // 2
    band = min(W, 2 * c + 1)
    row = torch.zeros(W, dtype=torch.float32)
    f = torch.arange(W)
    row[torch.minimum(f, W - f) <= c] = 1.0
    pairs = torch.arange(c + 1, max(c + 1, (W - 1) // 2 + 1))
    order = torch.randperm(pairs.numel(), generator=torch.Generator().manual_seed(seed))
    chosen = pairs[order[:(cols - band) // 2]]
    row[chosen] = 1.0
    row[W - chosen] = 1.0
    return row.expand(H, W).contiguous()


def cartesian_columns(W: int, acceleration: float, center_fraction: float = 0.08) -> int:
    r"""The number of columns :func:`cartesian_mask` keeps."""
    if W < 1 or acceleration < 1 or not 0 <= center_fraction <= 1:
        raise ValueError(f"cartesian_mask needs W >= 1, acceleration >= 1 and 0 <= center_fraction <= 1, got W {W}, acceleration "
                         f"{acceleration}, center_fraction {center_fraction}")
    c = int(math.floor(center_fraction * W + 0.5)) // 2
    n = int(math.floor(W / acceleration + 0.5))
    pairs = max(0, (W - 1) // 2 - c)
    return min(W, 2 * c + 1) + 2 * min(pairs, max(0, (n - (2 * c + 1)) // 2))


def _check_kspace_mask(mask: Tensor) -> None:
    r"""The rules of a sampling mask on a split-complex observation (:class:`MRIOperator`, :class:`MultiCoilMRIOperator`)."""
    if mask.ndim < 2:
        raise ValueError(f"mask is (H, W) or broadcasts to (B, 2 C, H, W), got shape {tuple(mask.shape)}")
    if mask.ndim >= 3 and mask.shape[-3] > 1:
        half = mask.shape[-3] // 2
        if mask.shape[-3] % 2 or not torch.equal(mask[..., :half, :, :], mask[..., half:, :, :]):
            raise ValueError("a mask with a channel axis has the same values on the real and the imaginary half of the 2 C "
                             f"channels, got shape {tuple(mask.shape)}")


class MRIOperator(LinearOperator):
    r"""Creates single-coil Cartesian k-space undersampling :math:`A = M F`: ``MaskOperator(mask) @ FourierOperator(norm)`` as
    one operator, so that it has a pseudo-inverse.  A :math:`(B, C, H, W)` input gives a :math:`(B, 2 C, H, W)` observation.

    Arguments:
        mask: The sampling mask :math:`M` in DFT order (DC at :math:`[0, 0]`): :math:`(H, W)`, :math:`(1, H, W)` or anything
            that broadcasts to :math:`(B, 2 C, H, W)` with the same values on the real and the imaginary half.  Bool, 0/1 or
            weights.  See :func:`cartesian_mask`.
        norm: See :class:`FourierOperator`.
        flatten, in_shape: See :class:`LinearOperator`.

    The adjoint is :math:`F^\top M`.  ``pinv`` is :math:`F^+ M^+` (:math:`F^\top M^+` for ``"ortho"``), the zero-filled
    reconstruction.  It is the Moore--Penrose inverse exactly when the mask is symmetric under :math:`k \to -k \bmod (H, W)`:
    :math:`F F^+` projects onto the Hermitian-symmetric spectra and commutes with :math:`M` only then.  The symmetry is checked
    once, at construction; ``pinv`` of an unsymmetric mask raises ``NotImplementedError``.

    Out of scope: see :class:`FourierOperator`.  Complex images and coil sensitivity maps: :class:`MultiCoilMRIOperator`.
    """

    _TRANSPOSE = _WITH_PINV  # (the modes of _run: the composition has no _kernel / _torch of its own)

    def __init__(self, mask: Tensor, norm: str = "ortho", flatten: bool = False, in_shape: Sequence[int] | None = None) -> None:
        super().__init__(flatten, in_shape)
        self.fourier = FourierOperator(norm)
        self.sampling = MaskOperator(mask)
        _check_kspace_mask(mask)
        self.symmetric = bool(torch.equal(mask, mask.flip(-2, -1).roll((1, 1), (-2, -1))))

    @property
    def mask(self) -> Tensor:
        return self.sampling.mask

    def _out_shape(self, in_shape: tuple) -> tuple:
        return self.sampling._out_shape(self.fourier._out_shape(in_shape))

    def _in_shape_of(self, out_shape: tuple) -> tuple:
        return self.fourier._in_shape_of(self.sampling._out_shape(out_shape))

    def _run(self, x: Tensor, mode: str) -> Tensor:
        r"""No dispatch of its own: the two operators' ``_run``, each with its own choice.  "pinv_t" completes the table and is
        reached by direct calls only: a gradient runs through the two operators' own Functions."""
        factor = "pinv" if mode in ("pinv", "pinv_t") else "apply"
        if mode in ("apply", "pinv_t"):
            return self.sampling._run(self.fourier._run(x, mode), factor)
        return self.fourier._run(self.sampling._run(x, factor), mode)

    def pinv(self, y: Tensor) -> Tensor:
        if not self.symmetric:
            raise NotImplementedError("MRIOperator.pinv is the Moore-Penrose inverse only for a mask that is symmetric under "
                                      "k -> -k mod (H, W): F F^+ does not commute with this one")
        return self._from_observation(y, "pinv")


# ------------------------------------------------------------------------------------------------------------ multi-coil
def birdcage_maps(coils: int, H: int, W: int, radius: float = 1.5) -> Tensor:
    r"""``coils`` synthetic sensitivity maps of a birdcage array, a ``complex128`` tensor :math:`(K, H, W)` for tests and demos,
    computed on the CPU in fp64 without random numbers.  Pixel centres span :math:`(-1, 1)^2` (units of the half field of view);
    coil :math:`k` sits at the angle :math:`2 \pi k / K` on a circle of ``radius``.  A map's magnitude is 1 / distance to its
    coil and its phase the angle of the vector from the pixel to the coil; the set is normalised so that
    :math:`\sum_k |S_k|^2 = 1` at every pixel.  ``radius`` exceeds :math:`\sqrt 2`, so no coil lies inside the image."""
    if not (isinstance(coils, int) and coils >= 1 and H >= 1 and W >= 1 and radius > math.sqrt(2.0)):
        raise ValueError(f"birdcage_maps needs coils, H, W >= 1 and radius > sqrt(2), got coils {coils}, {H} x {W}, radius {radius}")
    y = ((torch.arange(H, dtype=torch.float64) - (H - 1) / 2) / (H / 2))[None, :, None]
    x = ((torch.arange(W, dtype=torch.float64) - (W - 1) / 2) / (W / 2))[None, None, :]
    ang = (2 * math.pi / coils) * torch.arange(coils, dtype=torch.float64)[:, None, None]
    dx, dy = radius * torch.cos(ang) - x, radius * torch.sin(ang) - y
    dist = torch.hypot(dx, dy)
    s = torch.complex(dx, dy) / (dist * dist)  # exp(i phase) / distance
    return s / (s.real**2 + s.imag**2).sum(0, keepdim=True).sqrt()


class MultiCoilMRIOperator(LinearOperator):
    r"""Creates multi-coil Cartesian k-space undersampling (SENSE parallel imaging):
    :math:`y_k = M F (S_k \odot x)`, :math:`k = 0 .. K - 1`, with complex coil sensitivity maps :math:`S_k`.

    Arguments:
        mask: The sampling mask :math:`M` in DFT order, by the rules of :class:`MRIOperator`: :math:`(H, W)` or anything that
            broadcasts to :math:`(B, 2 K, H, W)` with equal real and imaginary halves.  See :func:`cartesian_mask`.
        maps: The sensitivity maps, a ``complex64`` or ``complex128`` tensor :math:`(K, H, W)` (one set for every sample) or
            :math:`(B, K, H, W)` (one per sample), finite.  Kept as split planes and moved to an input's device and dtype on first
            use: build a new operator for new maps rather than editing them in place.  See :func:`birdcage_maps`.
        norm: See :class:`FourierOperator`.
        complex_image: The input is :math:`(B, 2, H, W)` = :math:`\Re x \,|\, \Im x` (``True``) or a real image
            :math:`(B, 1, H, W)` (``False``).
        flatten, in_shape: See :class:`LinearOperator`.

    The observation is :math:`(B, 2 K, H, W)`: channel :math:`k` is :math:`\Re y_k` and channel :math:`K + k` is
    :math:`\Im y_k`, :class:`FourierOperator`'s convention with :math:`C = K`, so :class:`MaskOperator`, ``flatten`` and
    ``A2 @ A1`` apply unchanged.  The adjoint is :math:`\sum_k \bar S_k \odot F^H M y_k` (its real part for a real image): as a
    real-linear map on split-complex vectors, multiplication by :math:`\bar S` is the transpose of multiplication by :math:`S`,
    so this is the exact transpose.

    ``zero_filled(y)`` is the coil-combined zero-filled reconstruction
    :math:`\sum_k \bar S_k \odot F^+ M^+ y_k \,/\, \sum_k |S_k|^2` (0 where the maps vanish), with :math:`F^+` at the scale of
    :class:`FourierOperator`'s ``pinv``: what ``PGDMSampler(denoiser, y, A, A.zero_filled)`` takes.  It is the Moore--Penrose
    inverse exactly under full sampling with :math:`\sum_k |S_k|^2 > 0` everywhere, for both image kinds; under undersampling it
    is the standard APPROXIMATION, not the pseudo-inverse.
    ``pinv`` raises ``NotImplementedError``: solve the normal equations with ``linalg.cg`` where the exact one is needed.

    Every fp32 device tensor takes the kernels -- ``az_op_coil_expand_f32``, ``az_op_fft2_f32``, ``az_op_mul_f32`` and, on the
    way back, ``az_op_coil_combine_f32`` -- with two :math:`(B, 2 K, H, W)` intermediate buffers per call (the FFT entry is not
    in place); heights and widths are powers of two up to 1024 there.  Host and fp64 tensors run ``torch.complex`` /
    ``torch.fft`` in their own dtype at any size; half precision is not provided.

    Out of scope: fusing the coil product into the FFT's row loads, ESPIRiT calibration of the maps, ``fftshift``-ed layouts,
    non-Cartesian trajectories, more than one complex image per sample, and non-power-of-two sizes on the device.
    """

    _TRANSPOSE = {"apply": "adjoint", "adjoint": "apply", "zero_filled": "zero_filled_t", "zero_filled_t": "zero_filled"}
    _STRIDED = True  # (a strided view too: the Function makes it contiguous)
    _check_kernel_input = _check_fft_input

    def __init__(self, mask: Tensor, maps: Tensor, norm: str = "ortho", complex_image: bool = True, flatten: bool = False,
                 in_shape: Sequence[int] | None = None) -> None:
        super().__init__(flatten, in_shape)
        self.fourier = FourierOperator(norm)
        self.sampling = MaskOperator(mask)
        _check_kspace_mask(mask)
        if not torch.is_tensor(maps) or maps.dtype not in (torch.complex64, torch.complex128):
            raise ValueError("maps is a complex64 or complex128 tensor, got "
                             f"{maps.dtype if torch.is_tensor(maps) else type(maps).__name__}")
        if maps.ndim not in (3, 4) or maps.shape[-3] < 1 or 0 in maps.shape:
            raise ValueError(f"maps is (K, H, W) or (B, K, H, W) with K >= 1, got shape {tuple(maps.shape)}")
        maps = maps.detach().to(device="cpu", dtype=torch.complex128)
        if not (torch.isfinite(maps.real).all() and torch.isfinite(maps.imag).all()):
            raise ValueError("maps has a non-finite value")
        self.maps_re, self.maps_im = maps.real.contiguous(), maps.imag.contiguous()  # fp64 split planes
        self.complex_image = bool(complex_image)

    @property
    def mask(self) -> Tensor:
        return self.sampling.mask

    @property
    def coils(self) -> int:
        return self.maps_re.shape[-3]

    # -- shapes ---------------------------------------------------------------------------------------------------------
    def _out_shape(self, in_shape: tuple) -> tuple:
        out = self._cache.get(("out", in_shape))  # (a shape is checked once: broadcast_shapes costs more than a launch)
        if out is None:
            out = self._cache[("out", in_shape)] = self._checked_out_shape(in_shape)
        return out

    def _checked_out_shape(self, in_shape: tuple) -> tuple:
        c = 2 if self.complex_image else 1
        if in_shape[0] != c:
            raise ValueError(f"MultiCoilMRIOperator(complex_image={self.complex_image}) takes {c} channel{'s' * (c - 1)} "
                             f"({'re, then im' if c == 2 else 'a real image'}), got {in_shape[0]}")
        if tuple(in_shape[1:]) != tuple(self.maps_re.shape[-2:]):
            raise ValueError(f"the maps are {self.maps_re.shape[-2]} x {self.maps_re.shape[-1]}, got an image of {in_shape[1]} x "
                             f"{in_shape[2]}")
        return self.sampling._out_shape((2 * self.coils, *in_shape[1:]))

    def _in_shape_of(self, out_shape: tuple) -> tuple:
        if out_shape[0] != 2 * self.coils:
            raise ValueError(f"an observation of {self.coils} coils has {2 * self.coils} channels (re, then im), got {out_shape[0]}")
        if ("in", out_shape) not in self._cache:
            self.sampling._out_shape(out_shape)
            self._cache[("in", out_shape)] = True
        return (2 if self.complex_image else 1, *out_shape[1:])

    def _check_batch(self, x: Tensor) -> None:
        if self.maps_re.ndim == 4 and self.maps_re.shape[0] != x.shape[0]:
            raise ValueError(f"maps of shape {tuple(self.maps_re.shape)} are for a batch of {self.maps_re.shape[0]}, got "
                             f"{tuple(x.shape)}")

    def _check_mask_batch(self, y: Tensor) -> None:
        r"""``MaskOperator._check_batch`` of an observation, once per shape."""
        key = ("mask", tuple(y.shape))
        if key not in self._cache:
            self.sampling._check_batch(y)
            self._cache[key] = True

    def _maps(self, x: Tensor, normalized: bool) -> tuple[Tensor, Tensor]:
        r"""(re, im) of :math:`S`, or of :math:`S / \sum_k |S_k|^2` (0 where that is 0), in ``x``'s dtype on its device."""
        def make() -> tuple[Tensor, Tensor]:
            re, im = self.maps_re, self.maps_im
            if normalized:
                inv = _reciprocal_or_zero((re * re + im * im).sum(-3, keepdim=True))
                re, im = re * inv, im * inv
            return re, im

        return self._constant(x, ("maps", normalized), make)

    # -- the kernels ----------------------------------------------------------------------------------------------------
    def _kernel(self, x: Tensor, mode: str) -> Tensor:
        self._check_batch(x)
        B, _, h, w = x.shape
        K, hw = self.coils, h * w
        s_re, s_im = self._maps(x, mode == "zero_filled_t")
        maps = s_re.data_ptr(), s_im.data_ptr(), K * hw if s_re.ndim == 4 else 0  # (re, im, sample stride)
        c = 2 if self.complex_image else 1
        if mode in ("apply", "zero_filled_t"):  # image -> coil images -> k-space -> mask
            if not x.numel():
                return x.new_empty(B, 2 * K, h, w)
            coil, coil_planes = _split_empty(x, B, K, h, w)
            _launch("az_op_coil_expand_f32", *coil_planes, x.data_ptr(), x.data_ptr() + 4 * hw if c == 2 else None, c * hw, *maps, B, K,
                    hw)
            k, k_planes = _split_empty(x, B, K, h, w)
            _fft2(k_planes, coil_planes, x, B, K, h, w, 0, self.fourier._scale(hw, "apply" if mode == "apply" else "pinv_t"))
            y = _whole(k)
            self._check_mask_batch(y)
            m = self.sampling._factor(y, mode == "zero_filled_t", True)
            _launch("az_op_mul_f32", y.data_ptr(), y.data_ptr(), m.data_ptr(), y.numel(), m.numel())  # (in place: y is ours)
            return y
        # k-space -> mask -> coil images -> image
        out = _aligned(x.new_empty(B, c, h, w), 16)
        if not out.numel():
            return out
        self._check_mask_batch(x)
        m = self.sampling._factor(x, mode == "zero_filled", True)
        v = _aligned(torch.empty_like(x), 16)
        _launch("az_op_mul_f32", v.data_ptr(), x.data_ptr(), m.data_ptr(), x.numel(), m.numel())
        (k, k_planes), (coil, coil_planes) = _split_of(v, K, K * hw), _split_empty(x, B, K, h, w)
        _fft2(coil_planes, k_planes, x, B, K, h, w, 1, self.fourier._scale(hw, "adjoint" if mode == "adjoint" else "pinv"))
        _launch("az_op_coil_combine_f32", out.data_ptr(), out.data_ptr() + 4 * hw if c == 2 else None, c * hw, *coil_planes, *maps,
                B, K, hw, int(mode == "zero_filled"))
        return out

    # -- the torch path -------------------------------------------------------------------------------------------------
    def _torch(self, x: Tensor, mode: str) -> Tensor:
        if x.dtype not in (torch.float32, torch.float64):
            raise NotImplementedError(f"MultiCoilMRIOperator runs in fp32 and fp64, got {x.dtype}")
        self._check_batch(x)
        h, w = x.shape[2:]
        K = self.coils
        s = torch.complex(*self._maps(x, mode == "zero_filled_t"))
        if mode in ("apply", "zero_filled_t"):
            img = torch.complex(x[:, 0], x[:, 1]) if self.complex_image else x[:, 0]
            f = torch.fft.fft2(s * img[:, None]) * self.fourier._scale(h * w, "apply" if mode == "apply" else "pinv_t")
            return self.sampling._torch(torch.cat([f.real, f.imag], dim=1), "pinv" if mode == "zero_filled_t" else "apply")
        v = self.sampling._torch(x, "pinv" if mode == "zero_filled" else "apply")
        z = torch.fft.ifft2(torch.complex(v[:, :K], v[:, K:]), norm="forward")  # ("forward": unscaled inverse)
        z = z * self.fourier._scale(h * w, "adjoint" if mode == "adjoint" else "pinv")
        img = (s.conj() * z).sum(1, keepdim=True)
        if mode == "zero_filled":
            D = (s.real * s.real + s.imag * s.imag).sum(-3, keepdim=True)
            img = torch.where(D != 0, img / torch.where(D != 0, D, torch.ones_like(D)), torch.zeros_like(img))
        return torch.cat([img.real, img.imag], dim=1) if self.complex_image else img.real

    # -- the public maps ------------------------------------------------------------------------------------------------
    def pinv(self, y: Tensor) -> Tensor:
        raise NotImplementedError("MultiCoilMRIOperator has no closed-form pseudo-inverse under undersampling; zero_filled is the "
                                  "coil-combined zero-filled reconstruction (exact under full sampling), and linalg.cg solves the "
                                  "normal equations")

    def zero_filled(self, y: Tensor) -> Tensor:
        r"""The coil-combined zero-filled reconstruction of a :math:`(B, 2 K, H, W)` or flat observation:
        :math:`\sum_k \bar S_k \odot F^+ M^+ y_k \,/\, \sum_k |S_k|^2`."""
        return self._from_observation(y, "zero_filled")


# ----------------------------------------------------------------------------------------------------------------- Radon
def radon_angles(n: int, span: float = 180.0) -> Tensor:
    r"""``n`` evenly spaced angles in :math:`[0, \text{span})`, in degrees (fp64): ``span = 180`` with a small ``n`` is sparse-view
    CT, a smaller ``span`` limited-angle CT."""
    if n < 1 or not span > 0:
        raise ValueError(f"radon_angles needs n >= 1 and span > 0, got n {n}, span {span}")
    return torch.arange(n, dtype=torch.float64) * (float(span) / n)


def _cos_sin_degrees(deg: float) -> tuple[float, float]:
    r"""(cos, sin) of an angle in degrees, fp64: reduced modulo 360, evaluated within the octant and rotated by quadrants, so
    that multiples of 90 give exactly 0 / +-1 and 45 gives two equal numbers."""
    r = math.fmod(deg, 360.0)
    if r < 0:
        r += 360.0
    q, r = divmod(r, 90.0)
    if r == 45.0:
        c = s = math.sqrt(0.5)
    elif r < 45.0:
        c, s = math.cos(math.radians(r)), math.sin(math.radians(r))
    else:
        c, s = math.sin(math.radians(90.0 - r)), math.cos(math.radians(90.0 - r))
    for _ in range(int(q) % 4):
        c, s = -s, c
    return c + 0.0, s + 0.0  # (+ 0.0: no negative zero)


class RadonOperator(LinearOperator):
    r"""Creates the parallel-beam Radon transform (computed tomography): a :math:`(B, C, H, W)` input gives the sinogram
    :math:`(B, C, A, D)` of :math:`A` angles and :math:`D` detector bins, :math:`(A x)_{ak} = \sum_{ij} w_{akij} x_{ij}`.

    Arguments:
        theta: The :math:`A` projection angles in degrees (the convention of ``skimage.transform.radon``), a sequence or a
            tensor; any finite values, at most 4096 of them.  See :func:`radon_angles`.
        size: The image size :math:`(H, W)`, each at most 1024.  Required: the sinogram's shape does not determine it.
        det_count: :math:`D`, at most 2048.  The default, :math:`2 \lceil \sqrt{H^2 + W^2} / (2 d) \rceil + 1`, covers the image
            at every angle; a smaller count truncates the projections.
        det_spacing: The bin spacing :math:`d` in pixels, :math:`1 \le d \le 8`.  Below 1 the pixel-driven model leaves combs of
            empty bins, and filtered back-projection of it is useless.
        flatten: See :class:`LinearOperator`.  A flat :math:`(B, C A D)` observation is un-flattened without a recorded input
            shape: :math:`A D` is known.

    The model is pixel driven with linear interpolation on the detector, and its weights are fp32 by definition.  Per angle the
    host reduces :math:`\theta` modulo 360 in fp64, takes cosine and sine within the octant, rotates by quadrants and rounds to
    fp32: multiples of 90 degrees give exactly 0 / :math:`\pm 1`, 45 degrees two equal numbers.  With
    :math:`x = j - (W - 1) / 2`, :math:`y = i - (H - 1) / 2`, the position on the detector is
    :math:`p = ((x c + y s) \cdot (1 / d)) + (D - 1) / 2`, every operation rounded to fp32 on its own, and the weight of bin
    :math:`k` is :math:`w = \max(0, 1 - |p - k|)`.  Projector and back-projector (``csrc/radon.hip``) evaluate :math:`w` with
    one device function, so ``adjoint`` is the exact transpose of the call -- what ``cg`` in ``DiffPIRDenoiser`` and
    ``MMPSDenoiser`` assumes -- and the kernels add only the rounding of their sums.  No atomics: two runs give the same bits.

    ``fbp(y)`` is filtered back-projection, :math:`(\pi / A) A^\top (h * y)` with the Ram-Lak taps :math:`h_0 = 1 / (4 d^2)`,
    :math:`h_n = -1 / (\pi n d)^2` for odd :math:`n` and 0 for even :math:`n`, applied along the detector over its full length
    with zero padding: an APPROXIMATE inverse for angles that evenly cover 180 degrees, and what ``PGDMSampler(denoiser, y, A,
    A.fbp)`` takes.  There is no Moore--Penrose ``pinv``.

    Every fp32 device tensor takes the kernels (made contiguous and aligned first).  Host and fp64 tensors take products with the
    sparse matrix of the same fp32 weights, cast to the tensor's dtype and built once per device and dtype; half tensors take
    the fp32 product and round its result (``torch.sparse.mm`` has no half-precision form on the device).  ``torch.sparse.mm``
    has no forward-mode rule either, so that path goes through the same ``autograd.Function`` as the kernels: its ``backward``
    and ``jvp`` are products with the same matrices.

    Out of scope: fan-beam and cone-beam geometry, ray-driven (Siddon, Joseph) weights, :math:`d < 1`, other filters, a
    pseudo-inverse, half-precision kernels, 3-D.
    """

    _TRANSPOSE = {"apply": "adjoint", "adjoint": "apply", "fbp": "fbp_t", "fbp_t": "fbp"}
    _STRIDED = True  # (a strided view too: the Function makes it contiguous)

    def __init__(self, theta, size: Sequence[int], det_count: int | None = None, det_spacing: float = 1.0,
                 flatten: bool = False) -> None:
        super().__init__(flatten)
        theta = torch.as_tensor(theta, dtype=torch.float64).detach().to(device="cpu").reshape(-1)  # (a list of floats stays fp64)
        if not 1 <= theta.numel() <= MAX_RADON_ANGLES or not torch.isfinite(theta).all():
            raise ValueError(f"theta is 1 .. {MAX_RADON_ANGLES} finite angles in degrees, got {theta.numel()}")
        size = tuple(size) if isinstance(size, Sequence) else ()
        if len(size) != 2 or not all(isinstance(n, int) and 1 <= n <= MAX_RADON_SIZE for n in size):
            raise ValueError(f"size is (H, W), two ints in 1 .. {MAX_RADON_SIZE}, got {size}")
        d = float(det_spacing)
        if not 1.0 <= d <= 8.0:
            raise ValueError("det_spacing is between 1 and 8 pixels (below 1 the pixel-driven model leaves empty bins), got "
                             f"{det_spacing}")
        D = 2 * math.ceil(math.hypot(*size) / d / 2) + 1 if det_count is None else det_count
        if not (isinstance(D, int) and 1 <= D <= MAX_RADON_DET):
            raise ValueError(f"det_count is an int in 1 .. {MAX_RADON_DET}, got {D}")
        self.theta, self.size, self.det_count, self.det_spacing = theta, size, D, d
        self.table = torch.tensor([_cos_sin_degrees(float(t)) for t in theta], dtype=torch.float64).to(torch.float32)  # (A, 2)
        n = torch.arange(D, dtype=torch.float64)
        taps = torch.zeros(D, dtype=torch.float64)
        taps[0] = 1.0 / (4.0 * d * d)
        taps[1::2] = -1.0 / (math.pi * n[1::2] * d) ** 2
        self.taps = taps.to(torch.float32)
        self.fbp_scale = float(torch.tensor(math.pi / theta.numel(), dtype=torch.float32))  # (pi / A as the kernel receives it)

    @property
    def angles(self) -> int:
        return self.theta.numel()

    # -- shapes ---------------------------------------------------------------------------------------------------------
    def _out_shape(self, in_shape: tuple) -> tuple:
        if tuple(in_shape[1:]) != self.size:
            raise ValueError(f"this RadonOperator projects {self.size[0]} x {self.size[1]} images, got {in_shape[1]} x {in_shape[2]}")
        return (in_shape[0], self.angles, self.det_count)

    def _in_shape_of(self, out_shape: tuple) -> tuple:
        if tuple(out_shape[1:]) != (self.angles, self.det_count):
            raise ValueError(f"a sinogram of this RadonOperator is {self.angles} x {self.det_count} (angles x bins), got "
                             f"{out_shape[1]} x {out_shape[2]}")
        return (out_shape[0], *self.size)

    def _image(self, v: Tensor, what: str) -> Tensor:
        if v.ndim == 2:  # (the channel count follows from A D: no recorded input shape is needed)
            n = self.angles * self.det_count
            if v.shape[1] == 0 or v.shape[1] % n:
                raise ValueError(f"{what}: {tuple(v.shape)} is not a flattened (B, C, {self.angles}, {self.det_count}) sinogram")
            return v.unflatten(1, (v.shape[1] // n, self.angles, self.det_count))
        return super()._image(v, what)

    # -- the kernels ----------------------------------------------------------------------------------------------------
    def _on(self, x: Tensor, what: str) -> Tensor:
        r"""The angle table ("table") or the filter taps ("taps") on ``x``'s device, uploaded once."""
        return self._constant(x, what, lambda: getattr(self, what))

    def _project(self, x: Tensor) -> Tensor:
        (B, c, H, W), A, D = x.shape, self.angles, self.det_count
        y = _aligned(x.new_empty(B, c, A, D), 16)
        if y.numel():
            floats = C.c_int64(0)
            _lib.call("az_op_radon_work", B * c, H, W, C.byref(floats))
            work = _aligned(x.new_empty(max(floats.value, 4)), 16)  # (the transposed planes of the column-major angles)
            _launch("az_op_radon_f32", y.data_ptr(), x.data_ptr(), self._on(x, "table").data_ptr(), work.data_ptr(), B * c, H, W, A, D,
                    1.0 / self.det_spacing)
        return y

    def _backproject(self, v: Tensor, scale: float) -> Tensor:
        (B, c, A, D), (H, W) = v.shape, self.size
        x = _aligned(v.new_empty(B, c, H, W), 16)
        if x.numel():
            _launch("az_op_radon_adj_f32", x.data_ptr(), v.data_ptr(), self._on(v, "table").data_ptr(), B * c, H, W, A, D,
                    1.0 / self.det_spacing, scale)
        return x

    def _filter(self, v: Tensor, scale: float) -> Tensor:
        B, c, A, D = v.shape
        y = _aligned(torch.empty_like(v), 16)
        if y.numel():
            _launch("az_op_radon_filter_f32", y.data_ptr(), v.data_ptr(), self._on(v, "taps").data_ptr(), B * c * A, D, scale)
        return y

    def _kernel(self, x: Tensor, mode: str) -> Tensor:
        if mode == "apply":
            return self._project(x)
        if mode == "adjoint":
            return self._backproject(x, 1.0)
        scale = self.fbp_scale
        if mode == "fbp":
            return self._backproject(self._filter(x, 1.0), scale)
        return self._filter(self._project(x), scale)  # "fbp_t": the filter is symmetric Toeplitz, so (A^T F)^T = F A

    # -- the torch path -------------------------------------------------------------------------------------------------
    @functools.cached_property
    def _weights(self) -> tuple[Tensor, Tensor, Tensor]:
        r"""The nonzero weights as (row a D + k, column i W + j, fp32 value): the kernels' arithmetic, one rounded operation at
        a time, on the bins floor(p) and floor(p) + 1 -- all that can have a weight."""
        (H, W), D, f = self.size, self.det_count, torch.float32
        x = (torch.arange(W, dtype=f) - (W - 1) / 2)[None, :]
        y = (torch.arange(H, dtype=f) - (H - 1) / 2)[:, None]
        inv, off = torch.tensor(1.0 / self.det_spacing, dtype=f), torch.tensor((D - 1) / 2, dtype=f)
        rows, cols, vals = [], [], []
        for a in range(self.angles):
            p = ((x * self.table[a, 0] + y * self.table[a, 1]) * inv + off).reshape(-1)  # (eager fp32 ops: nothing is fused)
            k0 = p.floor()
            for k in (k0, k0 + 1):
                wk = (1 - (p - k).abs()).clamp_min(0)
                keep = ((k >= 0) & (k < D) & (wk > 0)).nonzero()[:, 0]
                rows.append(a * D + k[keep].long())
                cols.append(keep)
                vals.append(wk[keep])
        return torch.cat(rows), torch.cat(cols), torch.cat(vals)

    def _matrices(self, x: Tensor) -> tuple[Tensor, Tensor, Tensor]:
        r"""(M, M^T, the Toeplitz matrix of the taps) in ``x``'s dtype on its device, built once per device and dtype."""
        def make() -> tuple[Tensor, Tensor, Tensor]:  # (the sparse matrices on x's device at once: it coalesces faster)
            rows, cols, vals = self._weights
            (H, W), A, D = self.size, self.angles, self.det_count
            vals = vals.to(device=x.device, dtype=x.dtype)
            rows, cols = rows.to(x.device), cols.to(x.device)
            M = torch.sparse_coo_tensor(torch.stack([rows, cols]), vals, (A * D, H * W)).coalesce()
            Mt = torch.sparse_coo_tensor(torch.stack([cols, rows]), vals, (H * W, A * D)).coalesce()
            idx = (torch.arange(D)[:, None] - torch.arange(D)[None, :]).abs()
            return M, Mt, self.taps[idx]

        return self._constant(x, "matrix", make)

    def _product(self, x: Tensor, mode: str) -> Tensor:
        if x.dtype not in (torch.float32, torch.float64):  # (torch has no half-precision sparse product on the device)
            return self._product(x.float(), mode).to(x.dtype)
        M, Mt, T = self._matrices(x)
        (H, W), A, D = self.size, self.angles, self.det_count
        B, c = x.shape[:2]
        scale = self.fbp_scale
        if mode == "fbp":
            x = x @ T
        if mode in ("apply", "fbp_t"):
            y = torch.sparse.mm(M, x.reshape(B * c, H * W).T).T.reshape(B, c, A, D)
            return (y @ T) * scale if mode == "fbp_t" else y
        y = torch.sparse.mm(Mt, x.reshape(B * c, A * D).T).T.reshape(B, c, H, W)
        return y * scale if mode == "fbp" else y

    def _torch(self, x: Tensor, mode: str) -> Tensor:
        r"""The sparse products, inside the Function: ``torch.sparse.mm`` has no forward-mode rule of its own.  For the tensors
        ``_run`` sends here, that is: the Function gives an fp32 device tensor to the kernels, so the products of such a tensor
        are ``_product``."""
        return _Apply.apply(x, self, mode)

    # -- the public maps ------------------------------------------------------------------------------------------------
    def pinv(self, y: Tensor) -> Tensor:
        raise NotImplementedError("RadonOperator has no pseudo-inverse; fbp is filtered back-projection, an approximate inverse for "
                                  "angles that evenly cover 180 degrees")

    def fbp(self, y: Tensor) -> Tensor:
        r"""Filtered back-projection of a :math:`(B, C, A, D)` or flat sinogram: :math:`(\pi / A) A^\top (h * y)`."""
        return self._from_observation(y, "fbp")


# --------------------------------------------------------------------------------------------------------------- padding
class PadOperator(LinearOperator):
    r"""Creates the zero padding of every plane from :math:`H \times W` to
    :math:`(t + H + b) \times (l + W + r)` (the support constraint of phase retrieval: oversampling of the spectrum).

    Arguments:
        pad: The number of zeros on each side, an int or ``(top, bottom, left, right)``, none negative.
        flatten, in_shape: See :class:`LinearOperator`.

    The adjoint is the crop.  :math:`P^\top P = I`, so ``pinv`` is the crop too.
    """

    _TRANSPOSE = _WITH_PINV
    _STRIDED = True  # (a strided view too: the Function makes it contiguous)

    def __init__(self, pad: int | Sequence[int], flatten: bool = False, in_shape: Sequence[int] | None = None) -> None:
        super().__init__(flatten, in_shape)
        sides = (pad,) * 4 if isinstance(pad, int) else tuple(pad) if isinstance(pad, Sequence) else ()
        if len(sides) != 4 or not all(isinstance(p, int) and 0 <= p <= MAX_PAD for p in sides):
            raise ValueError(f"pad is an int or (top, bottom, left, right), each in 0 .. {MAX_PAD}, got {pad}")
        self.pad = sides

    def _out_shape(self, in_shape: tuple) -> tuple:
        (c, h, w), (t, b, l, r) = in_shape, self.pad
        return (c, h + t + b, w + l + r)

    def _in_shape_of(self, out_shape: tuple) -> tuple:
        (c, h, w), (t, b, l, r) = out_shape, self.pad
        if h < t + b or w < l + r:
            raise ValueError(f"a plane padded by {self.pad} is at least {t + b} x {l + r}, got {h} x {w}")
        return (c, h - t - b, w - l - r)

    def _kernel(self, x: Tensor, mode: str) -> Tensor:
        crop = mode in ("adjoint", "pinv")
        B, c = x.shape[:2]
        _, h, w = self._in_shape_of(tuple(x.shape[1:])) if crop else x.shape[1:]
        y = _aligned(x.new_empty(B, c, h, w) if crop else x.new_empty(B, *self._out_shape((c, h, w))), 16)
        if y.numel():
            _launch("az_op_pad_f32", y.data_ptr(), x.data_ptr(), B * c, h, w, *self.pad, int(crop))
        return y

    def _torch(self, x: Tensor, mode: str) -> Tensor:
        t, b, l, r = self.pad
        if mode in ("apply", "pinv_t"):
            return F.pad(x, (l, r, t, b))
        return x[:, :, t:x.shape[2] - b, l:x.shape[3] - r]

    def pinv(self, y: Tensor) -> Tensor:
        return self._from_observation(y, "pinv")


# ------------------------------------------------------------------------------------------------------------- nonlinear
class _Map(torch.autograd.Function):
    r"""``op``'s map: :class:`_Apply` for a :class:`NonlinearOperator`.  ``backward`` and ``jvp`` are applications of
    :class:`_Linearised` at the saved ``x``.  What :class:`_Apply` says about ``torch.func`` holds here and more: the saved ``x`` is
    a wrapper without storage too, so it is handed to :class:`_Linearised` as a TENSOR ARGUMENT, which functorch unwraps level by
    level down to ``forward``; an operating point kept on the operator object would stay a wrapper."""

    @staticmethod
    def forward(x: Tensor, op: NonlinearOperator) -> Tensor:
        if not _to_kernels(x, True):  # (reached through NonlinearOperator._function only)
            return op._torch(x)
        with device_context(x):
            return op._kernel(_aligned(x.contiguous(), 16))

    @staticmethod
    def setup_context(ctx, inputs, output) -> None:
        x, ctx.op = inputs
        ctx.save_for_backward(x)
        ctx.save_for_forward(x)

    @staticmethod
    def backward(ctx, g: Tensor):
        return _linearised(g, ctx.saved_tensors[0], ctx.op, "adjoint"), None

    @staticmethod
    def jvp(ctx, tx: Tensor, *_):
        return _linearised(tx, ctx.saved_tensors[0], ctx.op, "apply")


class _FirstOrderOnly(torch.autograd.Function):
    r"""The identity on an operating point ``x`` on its way into :class:`_Linearised`, whose derivative raises: a second derivative
    of the operator is not implemented on the kernel path, and must not silently be zero.  A node of its own, so that it raises
    only where a derivative THROUGH ``x`` is asked for: autograd never reaches it while it differentiates a Jacobian with respect
    to what it is applied to."""

    @staticmethod
    def forward(x: Tensor, op: NonlinearOperator) -> Tensor:
        return x.view_as(x)

    @staticmethod
    def setup_context(ctx, inputs, output) -> None:
        ctx.op = inputs[1]

    @staticmethod
    def backward(ctx, *_):
        raise NotImplementedError(f"a derivative of {type(ctx.op).__name__}'s Jacobian with respect to the point where it is taken "
                                  "(a second derivative of the operator) is not implemented on the kernel path")

    jvp = backward


class _Linearised(torch.autograd.Function):
    r"""``op``'s Jacobian at ``x`` ("apply") or its transpose ("adjoint") applied to ``v``.  Linear in ``v``: the tangent map with
    respect to ``v`` is the same map, its pullback the transposed one, both at the same ``x``.  ``x`` comes through
    :class:`_FirstOrderOnly` (:func:`_linearised`), which answers every derivative with respect to it."""

    @staticmethod
    def forward(v: Tensor, x: Tensor, op: NonlinearOperator, mode: str) -> Tensor:
        if not (_to_kernels(x, True) and _to_kernels(v, True)):  # (reached through NonlinearOperator._function only)
            return op._jac_torch(x, v, mode)
        with device_context(x):
            return op._jac_kernel(_aligned(x.contiguous(), 16), _aligned(v.contiguous(), 16), mode)

    @staticmethod
    def setup_context(ctx, inputs, output) -> None:
        _, x, ctx.op, ctx.mode = inputs
        ctx.save_for_backward(x)
        ctx.save_for_forward(x)

    @staticmethod
    def backward(ctx, g: Tensor):
        x = ctx.saved_tensors[0]
        # x's slot: a stand-in that autograd hands on to _FirstOrderOnly.backward, and only where x's derivative is asked for
        gx = g.new_zeros(()).expand_as(x) if ctx.needs_input_grad[1] else None
        return _Linearised.apply(g, x, ctx.op, _TRANSPOSED[ctx.mode]), gx, None, None

    @staticmethod
    def jvp(ctx, tv: Tensor, tx, *_):
        if tv is None:  # (only x moves: _FirstOrderOnly.jvp has raised before this is reached)
            raise NotImplementedError("a derivative with respect to the operating point of a Jacobian is not implemented")
        return _Linearised.apply(tv, ctx.saved_tensors[0], ctx.op, ctx.mode)


def _linearised(v: Tensor, x: Tensor, op: NonlinearOperator, mode: str) -> Tensor:
    r"""Every application of :class:`_Linearised` from outside itself."""
    return _Linearised.apply(v, _FirstOrderOnly.apply(x, op), op, mode)


_TRANSPOSED = {"apply": "adjoint", "adjoint": "apply"}


def _chw(in_shape: Sequence[int] | None) -> tuple | None:
    r"""An ``in_shape`` argument as a tuple (C, H, W), or ``None``."""
    if in_shape is None:
        return None
    shape = tuple(int(s) for s in in_shape)
    if len(shape) != 3:
        raise ValueError(f"in_shape is (C, H, W), got {shape}")
    return shape


class NonlinearOperator:
    r"""A differentiable map :math:`N` on images :math:`(B, C, H, W)` whose derivative depends on where it is taken: what
    ``DPSSampler``, ``TDSSampler`` (through its twist) and ``PGDMSampler`` take as a general callable ``A``.  Beside
    :class:`LinearOperator`, not under it: there is no adjoint of the map itself.

    Arguments:
        flatten: Whether the observation is flattened to :math:`(B, D)`.
        in_shape: The shape :math:`(C, H, W)` of an input.  Taken from the last forward call when not given.

    ``N(x)`` is the observation.  ``N.jacobian(x)`` is the linearisation at ``x``, a :class:`LinearOperator`:
    ``N.jacobian(x)(t)`` is the directional derivative, ``.adjoint(w)`` the pullback (of a flat or an image-shaped ``w``), with
    ``.T`` and ``@`` as usual.  ``N @ A``, ``A @ N`` and ``N2 @ N1`` chain operators of either kind; the chain's Jacobian is the
    chain rule.

    Dispatch is the file's one rule.  Contiguous fp32 device tensors (strided ones too, made contiguous first) go to the kernels
    through one ``torch.autograd.Function`` whose ``backward(g)`` is ``jacobian(x).adjoint(g)`` and whose ``jvp(t)`` is
    ``jacobian(x)(t)``, so ``autograd.grad``, ``torch.func.vjp`` and ``torch.func.jvp`` end in the same launches.  Everything
    else (host, fp64, half) takes a plain torch op sequence that torch differentiates itself.  On the kernel path a second
    derivative through ``x`` raises ``NotImplementedError``.

    A subclass states ``_out_shape`` / ``_in_shape_of`` as a :class:`LinearOperator` does, the map as ``_kernel(x)`` and
    ``_torch(x)``, and its Jacobian (``mode`` "apply") and the transpose ("adjoint") as ``_jac_kernel(x, v, mode)`` and
    ``_jac_torch(x, v, mode)``.
    """

    def __init__(self, flatten: bool = False, in_shape: Sequence[int] | None = None) -> None:
        self.flatten = bool(flatten)
        self.in_shape = _chw(in_shape)

    # -- what a subclass defines ----------------------------------------------------------------------------------------
    def _out_shape(self, in_shape: tuple) -> tuple:
        return in_shape

    def _in_shape_of(self, out_shape: tuple) -> tuple:
        return out_shape

    def _kernel(self, x: Tensor) -> Tensor:
        raise NotImplementedError

    def _torch(self, x: Tensor) -> Tensor:
        raise NotImplementedError

    def _jac_kernel(self, x: Tensor, v: Tensor, mode: str) -> Tensor:
        raise NotImplementedError

    def _jac_torch(self, x: Tensor, v: Tensor, mode: str) -> Tensor:
        raise NotImplementedError

    # -- what the base class does with it -------------------------------------------------------------------------------
    def _function(self, x: Tensor) -> Tensor:
        r"""The map through the Function of the kernel path, whatever ``x`` is (a host or fp64 tensor runs the torch ops inside
        it): how the Function's rules are tested without a device."""
        return _Map.apply(x, self)

    def _checked(self, x: Tensor) -> None:
        if x.ndim != 4:
            raise ValueError(f"{type(self).__name__} takes a (B, C, H, W) tensor, got {tuple(x.shape)}")
        self._out_shape(tuple(x.shape[1:]))

    # -- the public maps ------------------------------------------------------------------------------------------------
    def __call__(self, x: Tensor) -> Tensor:
        self._checked(x)
        self.in_shape = tuple(x.shape[1:])
        y = _Map.apply(x, self) if _to_kernels(x, True) else self._torch(x)
        return y.flatten(1) if self.flatten else y

    def jacobian(self, x: Tensor) -> LinearOperator:
        r"""The linearisation of the operator at ``x``."""
        self._checked(x)
        return _Jacobian(self, x)

    def __matmul__(self, other):
        if not isinstance(other, (LinearOperator, NonlinearOperator)):
            return NotImplemented
        return _Chain(self, other)

    def __rmatmul__(self, other):  # (a LinearOperator on the left: its own __matmul__ returns NotImplemented for us)
        if not isinstance(other, LinearOperator):
            return NotImplemented
        return _Chain(other, self)


class _Jacobian(LinearOperator):
    r"""``N.jacobian(x)``.  The operating point is a tensor argument of every application of :class:`_Linearised`.  Every shape
    comes from ``x``: the kernels take their counts from it, so what the Jacobian is applied to has exactly the shape of ``x``
    ("apply") or of ``N(x)`` ("adjoint"), and nothing a call receives replaces the recorded one."""

    def __init__(self, op: NonlinearOperator, x: Tensor) -> None:
        super().__init__(op.flatten, tuple(x.shape[1:]))
        self.op, self.x = op, x
        self._out_shape, self._in_shape_of = op._out_shape, op._in_shape_of

    def _run(self, v: Tensor, mode: str) -> Tensor:
        x = self.x
        want = (x.shape[0], *(self.in_shape if mode == "apply" else self._out_shape(self.in_shape)))
        if tuple(v.shape) != want:
            raise ValueError(f"the Jacobian of {type(self.op).__name__} at a point of shape {tuple(x.shape)} "
                             f"{'takes' if mode == 'apply' else 'pulls back'} a tensor of shape {want}, got {tuple(v.shape)}")
        if _to_kernels(x, True) and _to_kernels(v, True):
            return _linearised(v, x, self.op, mode)
        return self.op._jac_torch(x, v, mode)

    def __call__(self, t: Tensor) -> Tensor:
        y = self._run(t, "apply")
        return y.flatten(1) if self.flatten else y

    def adjoint(self, w: Tensor) -> Tensor:
        return self._run(self._image(w, "adjoint"), "adjoint")


class _Chain(NonlinearOperator):
    r"""``P_k @ ... @ P_1`` with at least one nonlinear part: :math:`x \mapsto P_k(\dots P_1(x))`, every part with its own dispatch
    and its own Function.  The Jacobian at ``x`` is the composition of the parts' Jacobians (a linear part is its own), each taken
    at the point the parts before it map ``x`` to: the chain rule, as the ``A2 @ A1`` of :class:`LinearOperator` s.  Only the
    outermost part may flatten."""

    def __init__(self, *parts, in_shape: Sequence[int] | None = None) -> None:  # (outermost first, as written)
        self.in_shape = _chw(in_shape)  # (no flatten of its own: the outermost part's)
        self.parts = tuple(q for p in parts for q in (p.parts if isinstance(p, _Chain) else (p,)))
        if any(p.flatten for p in self.parts[1:]):
            raise ValueError("only the outermost operator of a composition may flatten its observation")

    @property
    def flatten(self) -> bool:
        return self.parts[0].flatten

    def _out_shape(self, in_shape: tuple) -> tuple:
        for p in reversed(self.parts):
            in_shape = p._out_shape(in_shape)
        return in_shape

    def _in_shape_of(self, out_shape: tuple) -> tuple:
        for p in self.parts:
            out_shape = p._in_shape_of(out_shape)
        return out_shape

    def __call__(self, x: Tensor) -> Tensor:
        self._checked(x)
        self.in_shape = tuple(x.shape[1:])
        for p in reversed(self.parts):
            x = p(x)
        return x

    def jacobian(self, x: Tensor) -> LinearOperator:
        self._checked(x)
        J = None
        for k, p in enumerate(reversed(self.parts)):
            Jp = p.jacobian(x) if isinstance(p, NonlinearOperator) else p
            J = Jp if J is None else Jp @ J
            if k + 1 < len(self.parts):
                x = p(x)  # (the next part's operating point: the forward launches again, nothing is kept between calls)
            elif isinstance(p, LinearOperator):
                p.in_shape = tuple(x.shape[1:])  # (what a call would record: a flat cotangent is un-flattened with it)
        return J


class MagnitudeOperator(NonlinearOperator):
    r"""Creates the magnitude :math:`|z|` (or the intensity :math:`|z|^2`) of a split-complex image: a :math:`(B, 2 C, H, W)` input
    whose channels :math:`[0, C)` are :math:`\Re z` and :math:`[C, 2 C)` are :math:`\Im z`, as :class:`FourierOperator` writes
    them, gives :math:`(B, C, H, W)`.

    Arguments:
        squared: Whether the observation is the intensity :math:`|z|^2`.
        flatten, in_shape: See :class:`NonlinearOperator`.

    The Jacobian at :math:`z` maps :math:`t` to :math:`(\Re z \, t_{re} + \Im z \, t_{im}) / |z|` and its transpose :math:`w` to
    :math:`w \, (\Re z, \Im z) / |z|`; both are exactly 0 where :math:`z = 0` (torch's ``sgn`` convention for ``abs`` of a complex
    tensor).  ``squared``: :math:`2 (\Re z \, t_{re} + \Im z \, t_{im})` and :math:`2 w (\Re z, \Im z)`.  The kernels
    (``az_op_cmag_f32`` and its ``_vjp`` / ``_jvp``) scale by a power of two first, so nothing overflows or underflows wherever
    :math:`|z|` is a normal number.  Half precision is not provided.
    """

    def __init__(self, squared: bool = False, flatten: bool = False, in_shape: Sequence[int] | None = None) -> None:
        super().__init__(flatten, in_shape)
        self.squared = bool(squared)

    def _out_shape(self, in_shape: tuple) -> tuple:
        if in_shape[0] % 2:
            raise ValueError(f"a split-complex image has an even channel count (re, then im), got {in_shape[0]}")
        return (in_shape[0] // 2, *in_shape[1:])

    def _in_shape_of(self, out_shape: tuple) -> tuple:
        return (2 * out_shape[0], *out_shape[1:])

    def _kernel(self, x: Tensor) -> Tensor:
        B, c2, h, w = x.shape
        n = c2 // 2 * h * w
        y = _aligned(x.new_empty(B, c2 // 2, h, w), 16)
        if y.numel():
            _launch("az_op_cmag_f32", y.data_ptr(), n, x.data_ptr(), x.data_ptr() + 4 * n, 2 * n, B, n, int(self.squared))
        return y

    def _jac_kernel(self, x: Tensor, v: Tensor, mode: str) -> Tensor:
        B, c2, h, w = x.shape
        n = c2 // 2 * h * w
        z = x.data_ptr(), x.data_ptr() + 4 * n, 2 * n  # (re, im, sample stride)
        if mode == "apply":
            y = _aligned(x.new_empty(B, c2 // 2, h, w), 16)
            if y.numel():
                _launch("az_op_cmag_jvp_f32", y.data_ptr(), n, v.data_ptr(), v.data_ptr() + 4 * n, 2 * n, *z, B, n, int(self.squared))
            return y
        d = _aligned(torch.empty_like(x), 16)
        if d.numel():
            _launch("az_op_cmag_vjp_f32", d.data_ptr(), d.data_ptr() + 4 * n, 2 * n, v.data_ptr(), n, *z, B, n, int(self.squared))
        return d

    def _parts(self, x: Tensor) -> tuple[Tensor, Tensor]:
        if x.dtype not in (torch.float32, torch.float64):
            raise NotImplementedError(f"MagnitudeOperator runs in fp32 and fp64, got {x.dtype}")
        c = x.shape[1] // 2
        return x[:, :c], x[:, c:]

    def _torch(self, x: Tensor) -> Tensor:
        re, im = self._parts(x)
        return re * re + im * im if self.squared else torch.complex(re, im).abs()

    def _jac_torch(self, x: Tensor, v: Tensor, mode: str) -> Tensor:
        re, im = self._parts(x)
        if self.squared:
            u_re, u_im = 2 * re, 2 * im
        else:
            inv = _reciprocal_or_zero(torch.complex(re, im).abs())
            u_re, u_im = re * inv, im * inv
        if mode == "apply":
            c = x.shape[1] // 2
            return u_re * v[:, :c] + u_im * v[:, c:]
        return torch.cat([v * u_re, v * u_im], dim=1)


def _finite(*values: float) -> bool:
    return all(isinstance(v, (int, float)) and math.isfinite(v) for v in values)


class _ClampedOperator(NonlinearOperator):
    r"""What :class:`ClipOperator` and :class:`QuantizeOperator` share: the bounds, and the Jacobian of
    ``clamp(gain * x, low, high)`` -- ``gain`` where ``low <= gain * x <= high`` (bounds inclusive, ``torch.clamp``'s backward),
    0 elsewhere and where ``x`` is NaN.  Diagonal, so its own transpose: one kernel entry, ``az_op_clip_jac_f32``."""

    gain = 1.0

    def __init__(self, low: float, high: float, flatten: bool, in_shape: Sequence[int] | None) -> None:
        super().__init__(flatten, in_shape)
        if not _finite(low, high) or not low < high:
            raise ValueError(f"{type(self).__name__} needs finite bounds with low < high, got low {low}, high {high}")
        self.low, self.high = float(low), float(high)

    def _jac_kernel(self, x: Tensor, v: Tensor, mode: str) -> Tensor:
        d = _aligned(torch.empty_like(x), 16)
        if d.numel():
            _launch("az_op_clip_jac_f32", d.data_ptr(), v.data_ptr(), x.data_ptr(), x.numel(), self.gain, self.low, self.high)
        return d

    def _jac_torch(self, x: Tensor, v: Tensor, mode: str) -> Tensor:
        u = self.gain * x
        return torch.where((u >= self.low) & (u <= self.high), v, torch.zeros_like(v)) * self.gain


class ClipOperator(_ClampedOperator):
    r"""Creates sensor saturation :math:`x \mapsto \min(\max(g x, l), h)`.  The HDR task of the DPS paper is
    ``ClipOperator(gain=2.0)``.

    Arguments:
        low, high: The bounds :math:`l < h`, finite.
        gain: The factor :math:`g`, finite.
        flatten, in_shape: See :class:`NonlinearOperator`.

    The Jacobian at :math:`x` is diagonal: :math:`g` where :math:`l \le g x \le h` -- the bounds are inclusive, as in
    ``torch.clamp``'s backward -- and 0 elsewhere.  A NaN stays NaN and passes no cotangent.
    """

    def __init__(self, low: float = -1.0, high: float = 1.0, gain: float = 1.0, flatten: bool = False,
                 in_shape: Sequence[int] | None = None) -> None:
        super().__init__(low, high, flatten, in_shape)
        if not _finite(gain):
            raise ValueError(f"ClipOperator needs a finite gain, got {gain}")
        self.gain = float(gain)

    def _kernel(self, x: Tensor) -> Tensor:
        y = _aligned(torch.empty_like(x), 16)
        if y.numel():
            _launch("az_op_clip_f32", y.data_ptr(), x.data_ptr(), x.numel(), self.gain, self.low, self.high)
        return y

    def _torch(self, x: Tensor) -> Tensor:
        return torch.clamp(self.gain * x, self.low, self.high)


class QuantizeOperator(_ClampedOperator):
    r"""Creates bit-depth reduction: ``levels`` evenly spaced values from ``low`` to ``high``,
    :math:`x \mapsto \mathrm{rint}((u - l) / s) \, s + l` with :math:`u = \min(\max(x, l), h)` and the step
    :math:`s = (h - l) / (\text{levels} - 1)` rounded to fp32; halves round to even.

    Arguments:
        levels: The number of values, at least 2 (256: 8 bits).
        low, high: The range :math:`l < h`, finite.
        flatten, in_shape: See :class:`NonlinearOperator`.

    The map is piecewise constant: its derivative is 0 almost everywhere.  ``jacobian(x)`` is therefore the STRAIGHT-THROUGH one,
    the clamp's -- 1 where :math:`l \le x \le h`, 0 elsewhere (``az_op_clip_jac_f32`` with gain 1) -- which is what gradient
    guidance (``DPSSampler``) then follows.  ``PGDMSampler(denoiser, y, Q, lambda y: y)`` needs no derivative of the operator at
    all: it only calls ``Q`` and ``A_inv``.
    """

    def __init__(self, levels: int, low: float = -1.0, high: float = 1.0, flatten: bool = False,
                 in_shape: Sequence[int] | None = None) -> None:
        super().__init__(low, high, flatten, in_shape)
        if not (isinstance(levels, int) and 2 <= levels <= MAX_LEVELS):
            raise ValueError(f"levels is an int in 2 .. {MAX_LEVELS}, got {levels}")
        self.levels = levels
        self.step = float(torch.tensor((self.high - self.low) / (levels - 1), dtype=torch.float32))  # (as the kernel receives it)
        if not self.step > 0:
            raise ValueError(f"the step of {levels} levels from {low} to {high} is not a positive fp32 number")

    def _kernel(self, x: Tensor) -> Tensor:
        y = _aligned(torch.empty_like(x), 16)
        if y.numel():
            _launch("az_op_quantize_f32", y.data_ptr(), x.data_ptr(), x.numel(), self.low, self.high, self.step)
        return y

    def _torch(self, x: Tensor) -> Tensor:
        r"""The kernel's sequence.  ``round`` has a zero derivative, so the straight-through rule is written out: the value of
        the sequence, the gradient of the clamp."""
        u = torch.clamp(x, self.low, self.high)
        q = torch.round((u - self.low) / self.step) * self.step + self.low
        return q.detach() + (u - u.detach())  # (q + 0 exactly; a NaN stays NaN)


class PhaseRetrievalOperator(_Chain):
    r"""Creates Fourier phase retrieval, the task of the DPS paper: the magnitude of the oversampled spectrum of a real image,
    exactly ``MagnitudeOperator(squared) @ FourierOperator(norm) @ PadOperator(pad)``.  A :math:`(B, C, H, W)` input gives
    :math:`(B, C, t + H + b, l + W + r)`.

    Arguments:
        pad: The zero padding, see :class:`PadOperator`.  ``PhaseRetrievalOperator(H // 2)`` is 2x oversampling of an
            :math:`H \times H` image.
        norm: See :class:`FourierOperator`.
        squared: See :class:`MagnitudeOperator`.
        flatten, in_shape: See :class:`NonlinearOperator`.

    On fp32 device tensors the PADDED size follows :class:`FourierOperator`'s rule: powers of two up to 1024, else
    ``NotImplementedError``.  The launches are ``az_op_pad_f32``, ``az_op_fft2_f32`` and ``az_op_cmag_f32``, and
    ``az_op_cmag_vjp_f32`` / ``az_op_cmag_jvp_f32`` with the first two again for a derivative.

    Out of scope: non-power-of-two transforms on the device, half-precision kernel paths (half tensors take the torch path where
    it has one), JPEG and other block-transform degradations, and second derivatives through the operating point.
    """

    def __init__(self, pad: int | Sequence[int], norm: str = "ortho", squared: bool = False, flatten: bool = False,
                 in_shape: Sequence[int] | None = None) -> None:
        super().__init__(MagnitudeOperator(squared, flatten), FourierOperator(norm), PadOperator(pad), in_shape=in_shape)
