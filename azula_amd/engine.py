r"""Host-side execution engine: kernel tapes, static activation pools and hipGraph replay.

A backbone forward is compiled ONCE per input shape into a :class:`Tape` -- a flat list of
C-ABI calls whose every argument (device pointers, sizes, POD structs) is static.  Per-step
scalars live in device memory (``AzStepCoef``), so the same tape -- and the hipGraph captured
from it -- serves every sampling step.  Python is only the builder; replay is one
``hipGraphLaunch`` per step.
"""

from __future__ import annotations

import ctypes as C
import math
import os
from typing import NamedTuple

import torch

from . import _lib
from ._lib import AzConvArgs, AzNormFinalizeArgs, AzTransitionArgs


def pad4(c: int) -> int:
    return (c + 3) // 4 * 4


def pad8(c: int) -> int:
    return (c + 7) // 8 * 8


# Modules cast to half precision (.bfloat16() / .half()): "1" (default since round 6) = their activations live in HBM in the module's
# own type between the layers, as in the reference (azula/denoise.py:314-320 casts the backbone input to the module's dtype, so every
# tensor of the forward is a half tensor); statistics, softmax, gates and residual ADDS are evaluated in fp32 registers.  "0" = fp32
# activations in HBM, converted per tile (rounds 2 - 5).  Only plans whose every kernel has the typed form take it (ViT / DiT).
HALF_ACT = os.environ.get("AZ_HALF_ACT", "1") != "0"


class Tape:
    r"""A recorded sequence of C-ABI kernel launches with static arguments."""

    def __init__(self) -> None:
        self.ops: list[tuple] = []
        self.keep: list = []  # tensors / structs that must outlive the tape

    def add(self, name: str, *args, keep=()) -> None:
        fn = getattr(_lib.lib(), name)
        self.ops.append((fn, args, name))
        self.keep.extend(keep)

    def extend(self, other: "Tape") -> None:
        self.ops.extend(other.ops)
        self.keep.extend(other.keep)

    def run(self, stream: int | None = None) -> None:
        if stream is None:
            stream = _lib.stream_ptr()
        for fn, args, name in self.ops:
            rc = fn(*args, stream)
            if rc != 0:
                _lib.check(rc, name)

    def __len__(self) -> int:
        return len(self.ops)


class StepGraph:
    r"""hipGraph captured from a tape (on a private capture stream), launched on torch's stream."""

    def __init__(self, tape: Tape, device: torch.device) -> None:
        self.tape = tape
        self.handle = C.c_void_p()
        side = torch.cuda.Stream(device=device)
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side):
            _lib.call("az_graph_begin", side.cuda_stream)
            try:
                tape.run(side.cuda_stream)
            finally:
                _lib.call("az_graph_end", side.cuda_stream, C.byref(self.handle))
        torch.cuda.current_stream(device).wait_stream(side)
        self._side = side

    def launch(self) -> None:
        _lib.call("az_graph_launch", self.handle, _lib.stream_ptr())

    @property
    def num_nodes(self) -> int:
        n = C.c_int64()
        _lib.call("az_graph_num_nodes", self.handle, C.byref(n))
        return n.value

    def __del__(self) -> None:
        try:
            if self.handle:
                _lib.lib().az_graph_destroy(self.handle)
        except Exception:
            pass


class Pool:
    r"""Static activation buffers with explicit reuse (a graph needs fixed addresses)."""

    def __init__(self, device: torch.device) -> None:
        self.device = device
        self.free: dict[int, list[torch.Tensor]] = {}
        self.all: list[torch.Tensor] = []

    def alloc(self, numel: int, dtype: torch.dtype = torch.float32) -> torch.Tensor:
        lst = self.free.get((numel, dtype))
        if lst:
            return lst.pop()
        t = torch.empty(numel, dtype=dtype, device=self.device)
        self.all.append(t)
        return t

    def release(self, t: torch.Tensor) -> None:
        self.free.setdefault((t.numel(), t.dtype), []).append(t)

    @property
    def bytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in self.all)


class Act:
    r"""An NHWC activation: ``buf`` holds (B, H, W, cs) floats, ``C`` real channels."""

    __slots__ = ("buf", "B", "H", "W", "C", "cs", "pinned", "gn_quads", "affine", "qk_prepared", "bounded", "absmax")

    @property
    def half(self) -> bool:
        r"""The buffer holds a 2-byte type (the activations of a module cast to half precision, engine.HALF_ACT)."""
        return self.buf.dtype != torch.float32

    def __init__(self, buf: torch.Tensor, B: int, H: int, W: int, C_: int, cs: int, pinned: bool = False) -> None:
        self.buf, self.B, self.H, self.W, self.C, self.cs, self.pinned = buf, B, H, W, C_, cs, pinned
        # bounded: this tensor is the DIRECT output of a normalisation's apply (GroupNorm, LayerNorm, RMSNorm, with modulation and a
        # fused activation, or a pending in-gather affine, Act.affine): |x| <= |1 + a| sqrt(n) + |b| per element, whatever the
        # weights before it produced.  The f16x2 kernels with the FIXED activation scale (|x| < ~1e6, include/azula_amd.h) take
        # only such inputs.  Outputs of convolutions, attention, SwiGLU and upsampling are NOT bounded, even over bounded inputs:
        # their magnitude is set by trained weights (a 1e6 gain in a UNet FFN turns the fixed-scale split into NaN), so those
        # consumers go through choose_conv's dynamic rule -- the f16x2 kernels with a measured (az_absmax_f32) or producer-moment
        # bound (az_absmax_from_moments_f32) scale, or the bf16x3 kernels, whose domain is all of fp32.  Default False.
        # Set by Builder.wrote (and view()).  Content facts below end in the serial of the write they describe (Builder.fact).
        self.bounded = False
        self.absmax = None  # (AZ_ABSMAX_SLOTS floats written by az_absmax_f32 / ..._from_moments_f32, serial): Builder.absmax_of
        self.gn_quads = None  # (partials tensor, chunks per image, serial): GroupNorm moments written by the producing conv
        self.qk_prepared = False  # a fused qkv projection whose q / k are already normalised / gained / rotated (AzConvArgs.act = 5)
        self.affine = None    # ([scale | shift] tensor, act): a normalisation whose apply pass has not run -- the values are
        #                       act(buf * scale + shift); Builder.conv evaluates it inside the Winograd gather or materialises it

    @property
    def ptr(self) -> int:
        return self.buf.data_ptr()

    def view(self, B: int | None = None, H: int | None = None, W: int | None = None, C_: int | None = None, cs: int | None = None,
             *, buf: torch.Tensor | None = None, pinned: bool = True, bounded: bool | None = None, gn_quads: tuple | None = None) -> "Act":
        r"""Another shape over this allocation (``buf``: a slice of it).  Carries ``bounded``; carries GroupNorm moments only as the
        record the caller passes, re-chunked for the new shape -- content facts of the old shape do not describe the new one."""
        v = Act(self.buf if buf is None else buf, self.B if B is None else B, self.H if H is None else H, self.W if W is None else W,
                self.C if C_ is None else C_, self.cs if cs is None else cs, pinned)
        v.bounded = self.bounded if bounded is None else bounded
        v.gn_quads = gn_quads
        return v


class SharedResidual:
    r"""Marks the residual Act of :meth:`Builder.conv` as batch-shared (the epilogue's ``res_bcast``)."""

    def __init__(self, act: Act) -> None:
        self.act = act


def param_versions(module: torch.nn.Module) -> tuple:
    r"""What a compiled plan of ``module`` is valid for: (address, in-place version, dtype) of every parameter."""
    return tuple((p.data_ptr(), p._version, p.dtype) for p in module.parameters())


def mod_rows(mod: torch.Tensor | None, B: int, D: int, what: str = "module", tokens: bool = False) -> int:
    r"""Rows of a modulation vector ``mod`` -- (D) or (B, D) [``tokens``: (*, D) with the leading shape of x] -- for a batch of B:
    0 without modulation (``D == 0``), 1 when the samples share it, else B."""
    if D == 0:
        return 0
    assert mod is not None, f"this {what} is modulated: pass mod"
    rows = 1 if mod.ndim == 1 else (mod.numel() // mod.shape[-1] if tokens else mod.shape[0])
    assert rows in (1, B), "mod must be (D) or (*, D) with the leading shape of x"
    return rows


# Winograd for stride-1 3x3 convs (see conv.hip): "1" = exact F(2x2,3x3) where it pays (default), "0" = never,
# "2" = F(2x2) wherever it is legal (used by the parity tests to push whole networks through it),
# "4" = the faster but inexact F(4x4,3x3) on layers with >= WINOGRAD4_MIN_TILES tiles, "1" elsewhere
WINOGRAD = os.environ.get("AZ_WINOGRAD", "1")
# How fp32 convolutions / token GEMMs that run on the DIRECT kernel (1 x 1 convolutions, token linears, stride-2 and small-map
# 3 x 3) use the matrix pipe.  "bf16x3" (default since round 4, by the round-3 reviewer's ruling): every fp32 operand split
# EXACTLY into three bf16 pieces, the six largest partial products accumulated in fp32 on v_mfma_f32_32x32x16_bf16
# (az_conv2d_x3_f32) -- measured MORE accurate against fp64 than the fp32 MFMA (tests/test_gpu_kernels.py::
# test_conv2d_x3_accuracy) at 0.375 x its matrix-pipe time: DiT-B/2 54.7 -> 70.1 images/s, JiT-B/16 43.6 -> 58.4.
# "native": v_mfma_f32_32x32x2_f32 everywhere.  The stride-1 3 x 3 convolutions run the Winograd kernel in both modes (bf16x3: WINO_X3 below).
# "f16x2" (default since round 6): every fp32 operand as TWO IEEE half pieces (activations: h and the residual scaled by 2^11, of
# x / 16; weights: wh, wl and wh / 2^11 of w times a power of two fixed at pack time), three partial products on
# v_mfma_f32_32x32x16_f16 in one fp32 accumulator -- half the matrix instructions of bf16x3, measured the MOST accurate of the
# modes against fp64 (half as many fp32 accumulation steps: rms 5.2e-7 against 6.7e-7 bf16x3 / 7.5e-7 fp32 MFMA on the K = 2304
# layer of test_conv2d_x3_accuracy), on a STATED range of its activation operand, |x| < ~1e6 (beyond it NaN, never a wrong finite
# value: include/azula_amd.h).  With that FIXED scale it takes only BOUNDED inputs (Act.bounded: direct outputs of normalisations);
# every other input runs it with a measured / moment-bounded scale (F16X2_DYNAMIC below) or the bf16x3 kernels.
# C2 16.95 -> 15.2 ms per denoise step, C3 85 -> 107+ images/s, C5 32.1 -> 28.5 ms, C6 63.6 -> 84 images/s (profiles/r06_f16x2_gate*.txt).
FP32_MFMA = os.environ.get("AZ_FP32_MFMA", "f16x2")
assert FP32_MFMA in ("native", "bf16x3", "f16x2"), FP32_MFMA


def moments_for_scale() -> bool:
    r"""A consumer's f16x2 activation scale may be bounded from its producer's moments (F16X2_DYNAMIC / F16X2_MOMENTS below):
    producers without a GroupNorm after them ask for moments (Builder.conv(gn_stats=...)) only then."""
    return FP32_MFMA == "f16x2" and F16X2_DYNAMIC and F16X2_MOMENTS


def pieces() -> bool:
    r"""fp32 operands as 2-byte pieces on the bf16 / f16 pipe (read per plan: bench.py flips FP32_MFMA between plans)."""
    return FP32_MFMA in ("bf16x3", "f16x2")


# f16x2 mode, layers whose input is NOT bounded (residual / input streams, outputs of convolutions and attention): "1" (default) =
# f16x2 kernels too where it pays, with the activation scale taken from the sources' largest magnitude (one streaming az_absmax_f32
# pass per source tensor and step, shared by its consumers; AzConvArgs.in_absmax0 / in_absmax1: no stated range) -- the UNet's
# strided, skip-merge and second FFN convolutions, the token GEMMs behind attention / an FFN; "0" = bf16x3
F16X2_DYNAMIC = os.environ.get("AZ_F16X2_DYNAMIC", "1") != "0"
# ... and where the tensor's producer left GroupNorm moments (Act.gn_quads), the maximum is BOUNDED from them instead of measured
# (az_absmax_from_moments_f32: no pass over the tensor) -- ADM's 1x1 skip projections, whose pass would cost what it saves, and the
# UNet FFN's SiLU(conv) hidden tensor, whose Winograd producer leaves them for its consumer ("0": measure)
F16X2_MOMENTS = os.environ.get("AZ_F16X2_MOMENTS", "1") != "0"
ATTN_H2 = os.environ.get("AZ_ATTN_H2", "1") != "0"  # f16x2 mode: the attention contractions in that form too ("0": bf16x3 attention -- A/B)
ATTN_X3 = os.environ.get("AZ_ATTN_X3", "1") != "0"  # bf16x3 mode: attention contractions on the bf16 pipe too (az_attention_x3_f32)
# The stride-1 3 x 3 layers in bf16x3 mode: "1" (default since round 5) = the Winograd kernel with its 16 frequency GEMMs on the bf16 pipe
# as exact 3 x bf16 splits too (az_conv2d_winograd_x3_f32, csrc/wino_x3.hip: same transforms, same epilogue, 1.19 - 1.28 x the fp32
# stream on the UNet / ADM layers, profiles/r05_wx3_*); "0" = the fp32-MFMA Winograd stream (always the one in "native" mode).
WINO_X3 = os.environ.get("AZ_WINO_X3", "1") != "0"
X3_MIN_CHANNELS = 32  # bf16x3 only where both channel counts fill a K tile / an MFMA tile
WINOGRAD4_MIN_TILES = int(os.environ.get("AZ_WINOGRAD4_MIN_TILES", "1024"))
# q / k RMS norm, gains and RoPE of an attention layer in the epilogue of its qkv projection ("0": inside the attention kernel)
QK_PREP = os.environ.get("AZ_QK_PREP", "1") != "0"
# GroupNorm statistics from the producing convolution's epilogue ("1", default) or always by the separate pass ("0")
GN_FUSED = os.environ.get("AZ_GN_FUSED", "1") != "0"
# GroupNorm apply pass (y = x * S + T) inside the consuming Winograd convolution's gather ("0": always the separate pass)
# The first convolution reads the latent planar (az_conv2d_stem_f32) instead of an NHWC copy of it ("0": the NHWC path)
STEM_PLANAR = os.environ.get("AZ_STEM_PLANAR", "1") != "0"
AFFINE_FUSED = os.environ.get("AZ_AFFINE_FUSED", "1") != "0"
GN_FUSED_SPLITK = os.environ.get("AZ_GN_FUSED", "1") != "epilogue"  # ("epilogue": only the Winograd epilogue's moments -- A/B)

# Every switch above that a plan bakes in at build time: what :func:`plan_mode` reads
PLAN_SWITCHES = ("FP32_MFMA", "WINOGRAD", "WINO_X3", "F16X2_DYNAMIC", "F16X2_MOMENTS", "GN_FUSED", "GN_FUSED_SPLITK", "HALF_ACT", "QK_PREP",
                 "STEM_PLANAR", "AFFINE_FUSED", "ATTN_H2", "ATTN_X3", "WINOGRAD4_MIN_TILES", "X3_MIN_CHANNELS")


def plan_mode() -> tuple:
    r"""The arithmetic mode a plan built now would bake in (read per call: tests and ``bench.py`` assign to these names)."""
    g = globals()
    return tuple(g[name] for name in PLAN_SWITCHES)


class PlanCache(dict):
    r"""The compiled plans of one module, ``key -> plan`` in build order (a plain dict to everything that reads it).  A plan is
    valid for its *stamp*: the module's :func:`param_versions`, :func:`plan_mode` and whatever else its builder bakes in
    (``extra``).  At most ``max_live`` plans are kept, oldest built dropped first (a hit does not reorder); a plan that a
    captured loop or a pullback still holds lives on with its holder, and a later lookup builds it again."""

    def __init__(self, max_live: int = 4) -> None:
        super().__init__()
        self.max_live = max_live
        self.stamps: dict = {}

    def get(self, key, make, module: torch.nn.Module, extra=()):
        r"""The plan under ``key`` while its stamp is the current one, else ``make()`` -- after dropping every plan with
        another stamp, none of which can become valid again."""
        stamp = (param_versions(module), plan_mode(), extra)
        if key in self and self.stamps.get(key) == stamp:
            return self[key]
        for k in [k for k in self if self.stamps.get(k) != stamp]:
            del self[k]
        self[key] = plan = make()
        while len(self) > self.max_live:
            del self[next(iter(self))]
        self.stamps = dict.fromkeys(self, stamp)
        return plan


def content_key(module: torch.nn.Module, *tensors) -> tuple:
    r"""Cache-key element for tensors that a plan bakes in by CONTENT (positions -> RoPE / embedding tables, mask bytes): per
    tensor ``None`` or (shape, dtype, bytes).  Bytes compare by value, so no hash collision can hand out a plan built for other
    values.  The last two argument sets are remembered on the module by identity -- same objects, storage, shape and version
    counter, the tensors kept alive so that their storage cannot pass to others -- and recognised without another copy to the
    host: a steady-state call does not synchronise the device."""
    seen = module.__dict__.setdefault("_plan_seen", {})
    ik = tuple(None if t is None else (t.data_ptr(), t._version, tuple(t.shape), str(t.dtype), str(t.device)) for t in tensors)
    hit = seen.get(ik)
    if hit is not None and all(a is b for a, b in zip(hit[1], tensors)):
        return hit[0]
    content = tuple(None if t is None else (tuple(t.shape), str(t.dtype), t.detach().cpu().reshape(-1).view(torch.uint8).numpy().tobytes())
                    for t in tensors)
    if len(seen) >= 2:
        seen.clear()
    seen[ik] = (content, tensors)
    return content


WINO_X3_NAMES = ("az_conv2d_winograd_x3_f32", "az_conv2d_winograd_f16x2_f32")  # wino_x3.hip: the piece forms of the Winograd kernel
H2_NAMES = ("az_conv2d_winograd_f16x2_f32", "az_conv2d_f16x2_f32")
PACKED = {"az_conv2d_winograd4_f32": "winograd4", "az_conv2d_winograd_f32": "winograd", "az_conv2d_winograd_x3_f32": "winograd_x3",  # ConvWeights
          "az_conv2d_winograd_f16x2_f32": "winograd_f16x2", "az_conv2d_x3_f32": "direct_x3", "az_conv2d_f16x2_f32": "direct_f16x2",
          "az_conv2d_f32": "direct"}
# Builder.conv(winograd=...): None = the policy below; False / 0 = never Winograd, True / 1 / 2 = Winograd where legal, 4 = F(4x4,3x3);
# "x3" / "wx3": the bf16x3 kernels, "h2" / "wh2": the f16x2 ones, "h2d" / "wh2d": those with the activation scale measured from the
# sources (az_absmax_f32), whatever the mode ("w...": the Winograd form) -- kernel tests
CONV_OVERRIDES = (None, False, True, 0, 1, 2, 4, "x3", "wx3", "h2", "wh2", "h2d", "wh2d")


# What the kernel choice reads of one source of a convolution: its real channels, the elements of its buffer (what an az_absmax_f32
# pass streams), Act.bounded, a pending normalisation (Act.affine), and whether a maximum (Builder.absmax_of) / its producer's
# GroupNorm moments (Act.gn_quads) of its current contents are recorded
ConvSource = NamedTuple("ConvSource", [("C", int), ("numel", int), ("bounded", bool), ("affine", bool), ("absmax", bool), ("moments", bool)])
# ... and of the convolution: geometry (aniso: a stride / upsampling per axis), channel strides, one depth tap of a 3-D convolution,
# Builder.half, the winograd= override (CONV_OVERRIDES), the sources and whether the weights' range fits the f16x2 packing
ConvLayer = NamedTuple("ConvLayer", [
    ("ks", int), ("stride", int), ("aniso", bool), ("B", int), ("hout", int), ("wout", int), ("c0s", int), ("c1s", int), ("cout", int),
    ("cout_s", int), ("up0", int), ("depth", bool), ("half", "torch.dtype | None"), ("winograd", object), ("src0", ConvSource),
    ("src1", "ConvSource | None"), ("w_h2", bool)])
ConvLayer.__new__.__defaults__ = (True,)  # w_h2: the weights' range fits the f16x2 packing (ConvWeights.h2_range)
# the C entry, the f16x2 form (H2_NAMES), with the activation scale from the sources' maxima (AzConvArgs.in_absmax0 / in_absmax1)
ConvChoice = NamedTuple("ConvChoice", [("name", str), ("h2", bool), ("dyn", bool)])


def sources_bounded(src0, src1) -> bool:
    r"""Every source of a convolution (Act or ConvSource) bounded; a pending normalisation is applied in the gather / materialised."""
    return bool(src0.bounded or src0.affine) and (src1 is None or src1.bounded)


def choose_conv(l: ConvLayer) -> ConvChoice:
    r"""Kernel and arithmetic of one convolution.  Pure: reads the module switches at call time (bench.py flips FP32_MFMA between
    plans), calls nothing on the device."""
    w = l.winograd
    if w not in CONV_OVERRIDES:
        raise ValueError(f"winograd={w!r}: one of {CONV_OVERRIDES}")
    srcs = [s for s in (l.src0, l.src1) if s is not None]
    cin_s = l.c0s + l.c1s
    # (half-precision modules: the direct bf16 / f16 kernel; one factor per axis: the direct kernel's loaders only)
    legal = l.ks == 3 and l.stride == 1 and not l.aniso and l.half is None
    # image head (<= 4 output channels) on a map that fills the chip with 16 x 16-pixel workgroups:
    # az_conv2d_f32 runs its narrow-output VALU kernel (104 vs 342 us at 4 x 256^2, 256 -> 3)
    head = (w is None and legal and l.cout_s == 4 and l.src1 is None and l.up0 == 0 and l.c0s % 16 == 0
            and l.B * ((l.hout + 15) // 16) * ((l.wout + 15) // 16) >= 256 and not l.depth)
    wino_ok = legal and not head and w not in ("x3", "h2", "h2d")
    tiles4 = l.B * ((l.hout + 3) // 4) * ((l.wout + 3) // 4)
    use_f4 = wino_ok and not l.depth and (w == 4 or (w is None and WINOGRAD == "4" and tiles4 >= WINOGRAD4_MIN_TILES))
    use_wino = wino_ok and not use_f4 and ((WINOGRAD != "0") if w is None else bool(w))
    if use_wino and w is None and WINOGRAD in ("1", "4") and l.B * ((l.hout + 1) // 2) * ((l.wout + 1) // 2) < 64:
        use_wino = False  # less than one 64-tile block (measured: 8x8 at batch < 4): the direct kernel wins
    # bf16x3 mode replaces the DIRECT fp32 kernel (1x1 convs / token GEMMs, stride 2, small maps: 147-181 vs 113-128
    # TF/s); the 3x3 stride-1 layers stay on the fp32 Winograd kernel, which executes 2.25x fewer multiplies
    # (221 vs 181 TF/s algorithmic at 4 x 256^2, 256 -> 256).
    use_x3 = l.half is None and (
        w in ("x3", "h2", "h2d")
        or (w is None and pieces() and not head and not use_wino and not use_f4 and cin_s >= X3_MIN_CHANNELS and l.cout_s >= X3_MIN_CHANNELS)
    )
    h2 = w in ("h2", "wh2", "h2d", "wh2d") or (w not in ("x3", "wx3") and FP32_MFMA == "f16x2" and l.w_h2 and sources_bounded(l.src0, l.src1))
    dyn = w in ("h2d", "wh2d")
    if (not h2 and w is None and FP32_MFMA == "f16x2" and F16X2_DYNAMIC and l.w_h2 and l.half is None and not l.depth
            and (use_wino or use_x3) and not use_f4 and not any(s.affine for s in srcs)):
        # unbounded sources: f16x2 with the scale measured per step, where the pass over the sources costs clearly less than the
        # matrix instructions it saves (~12 % of a Winograd layer at ~350 TF/s algorithmic, ~25 % of a direct one at ~190);
        # never on a pending normalisation (its maximum is not that of the stored tensor)
        flops = 2.0 * l.B * l.hout * l.wout * l.cout * sum(s.C for s in srcs) * l.ks * l.ks
        gain_s = 0.12 * flops / 350e12 if use_wino else 0.25 * flops / 190e12
        cost_s = sum(4e-6 + (0.0 if (s.moments and F16X2_MOMENTS) else s.numel * 4 / 5.0e12) for s in srcs if not s.absmax)
        dyn = h2 = gain_s > 1.5 * cost_s
    if use_f4:
        name = "az_conv2d_winograd4_f32"
    elif use_wino and l.wout >= 3 and (w in ("wx3", "wh2", "wh2d") or (w is None and WINO_X3 and pieces())):
        # the frequency GEMMs on the bf16 pipe as exact 3 x bf16 splits (wino_x3.hip); same descriptor, 16-channel steps
        # (f16x2: the same kernel with two half pieces per operand and three products)
        name = "az_conv2d_winograd_f16x2_f32" if h2 else "az_conv2d_winograd_x3_f32"
    elif use_wino:
        name = "az_conv2d_winograd_f32"
    elif use_x3:
        name = "az_conv2d_f16x2_f32" if h2 else "az_conv2d_x3_f32"
    elif l.half is not None:
        name = "az_conv2d_f16_f32" if l.half == torch.float16 else "az_conv2d_bf16_f32"
    else:
        name = "az_conv2d_f32"
    h2 = name in H2_NAMES
    return ConvChoice(name, h2, dyn and h2)


# The f16x2 attention kernel's stated domain (include/azula_amd.h): |k| < 4094, |q * scale * log2 e| < 1e6; choose_attention takes it
# only for RMS-normalised q / k whose plan-time bound (attention_qk_bound) is below these limits with a factor 2 to spare
ATTN_H2_K_MAX = 4094.0 / 2
ATTN_H2_QS_MAX = 1.0e6 / 2


def attention_qk_bound(dim: int, norm_dim: int, scale: float, qk_weight: tuple | None) -> tuple[float, float]:
    r"""(max |k|, max |q * scale * log2 e|) of RMS-normalised q / k rows: a normalised row has 2-norm sqrt(n) (n = norm_dim or
    dim; eps only shrinks it), the learned gains multiply it by at most max |g|, RoPE turns channel pairs without changing their
    norm -- so no element exceeds sqrt(n) max |g|.  Read at plan time from the gain tensors."""
    n = norm_dim or dim
    gq, gk = (1.0, 1.0) if qk_weight is None else (float(qk_weight[0].detach().abs().max()), float(qk_weight[1].detach().abs().max()))
    return math.sqrt(n) * gk, math.sqrt(n) * gq * abs(scale) * 1.4426950408889634


def qk_in_h2_domain(qk_rmsnorm: bool, dim: int, norm_dim: int, scale: float, qk_weight: tuple | None) -> bool:
    r"""q / k are RMS-normalised with a plan-time bound inside the f16x2 attention kernel's domain (``choose_attention(qk_normed=)``)."""
    if not qk_rmsnorm:
        return False
    kmax, qsmax = attention_qk_bound(dim, norm_dim, scale, qk_weight)
    return kmax < ATTN_H2_K_MAX and qsmax < ATTN_H2_QS_MAX


def _token_strides(a, L: int, **tensors) -> None:
    r"""Batch / token / head strides (in elements) of an attention descriptor's operands: ``name=(token Act of L tokens, head stride)``."""
    for name, (t, hstride) in tensors.items():
        setattr(a, name + "_bstride", L * t.cs)
        setattr(a, name + "_tstride", t.cs)
        setattr(a, name + "_hstride", hstride)


def qkv_layout(order: str, Cq: int, dim: int) -> tuple[tuple, int]:
    r"""(channel offsets of q, k, v in a fused token row of 3 Cq channels, head stride) for ``order``: "nHC" = azula '(n H C)'
    (attention.py:90) and "3HC" = ADM's new order (unet.py:371), "H3C" = ADM legacy (unet.py:338)."""
    if order in ("nHC", "3HC"):
        return (0, Cq, 2 * Cq), dim
    if order == "H3C":
        return (0, dim, 2 * dim), 3 * dim
    raise ValueError(order)


def choose_attention(dim: int, qk_normed: bool, half: torch.dtype | None) -> str:
    r"""C entry of an attention layer (head size ``dim``, Builder.half); ``qk_normed``: q and k are RMS-normalised (in the kernel or
    in the projection epilogue) with a bound inside the f16x2 kernel's domain (attention_qk_bound).  Reads the switches at call time."""
    if half is not None:  # module cast to half precision: contractions on the bf16 / f16 MFMA
        return "az_attention_f16_f32" if half == torch.float16 else "az_attention_bf16_f32"
    if pieces() and ATTN_X3 and dim in (16, 32, 64, 80):
        # the two contractions as 3 x bf16 pieces / 6 partial products: fp32 accuracy, 0.375 x the pipe time (64 x 12 heads x 256
        # tokens x 64: 140 -> 111 us; head_dim 128 needs one wave per SIMD there and measured slower, 458 vs 516 us: fp32 kernel).
        # The f16x2 form only on normalised q / k: un-normalised keys (ADM, qk_norm=False ViTs) reach its |k| < 4094 limit.
        return "az_attention_f16x2_f32" if FP32_MFMA == "f16x2" and ATTN_H2 and qk_normed else "az_attention_x3_f32"
    return "az_attention_f32"


class ConvWeights:
    r"""Convolution / linear weights in the layouts the kernels consume."""

    def __init__(self, bld: "Builder", weight: torch.Tensor, bias: torch.Tensor | None, cin0: int | None) -> None:
        w = weight.detach().to(device=bld.device, dtype=torch.float32)
        if w.ndim == 2:
            w = w[:, :, None, None]
        elif w.ndim == 3 and w.shape[2] == 1:  # Conv1d k=1 (ADM attention projections)
            w = w[:, :, :, None]
        elif w.ndim == 3:  # Conv1d with k taps on a one-row image: the taps are the middle row of a k x k filter whose
            k = w.shape[2]  # other rows only ever multiply padding (spatial = 1 UNets, azula/nn/layers.py:25-50)
            w2 = torch.zeros(w.shape[0], w.shape[1], k, k, dtype=w.dtype, device=w.device)
            w2[:, :, k // 2, :] = w
            w = w2
        if w.shape[2] != w.shape[3]:  # anisotropic odd kernel (kh, kw): centred in a square one; with 'same' padding the
            kh, kw_ = w.shape[2], w.shape[3]  # extra zero rows / columns only ever add zeros
            assert kh % 2 == 1 and kw_ % 2 == 1, "odd kernel sizes only"
            k = max(kh, kw_)
            w2 = torch.zeros(w.shape[0], w.shape[1], k, k, dtype=w.dtype, device=w.device)
            w2[:, :, (k - kh) // 2 : (k - kh) // 2 + kh, (k - kw_) // 2 : (k - kw_) // 2 + kw_] = w
            w = w2
        self.w = w.contiguous()
        self.cout, self.cin, self.ks, kw = self.w.shape
        assert self.ks == kw
        self.cin0 = self.cin if cin0 is None else cin0
        self.c0s, self.c1s = bld.pad(self.cin0), bld.pad(self.cin - self.cin0)
        self.cout_s = bld.pad(self.cout)
        self.device = bld.device
        self.bias = None
        if bias is not None:
            self.bias = torch.zeros(self.cout_s, dtype=torch.float32, device=bld.device)
            self.bias[: self.cout] = bias.detach().to(device=bld.device, dtype=torch.float32)
        self._forms: dict = {}  # packed layouts, made on first use
        self._amax = None
        self._h2_range = None

    def _form(self, key, numel: int, dtype: torch.dtype, pack: str, *args) -> torch.Tensor:
        r"""The layout ``key``: a (numel,) tensor written by the C packing entry ``pack(dst, w, *args, stream)``, made once."""
        if key not in self._forms:
            t = torch.empty(numel, dtype=dtype, device=self.device)
            _lib.call(pack, t.data_ptr(), self.w.data_ptr(), *args, _lib.stream_ptr())
            self._forms[key] = t
        return self._forms[key]

    def _direct_args(self, pieces: int) -> tuple:
        cin_s = self.c0s + self.c1s
        return pieces * self.ks * self.ks * self.cout_s * cin_s, (self.cout, self.cin, self.ks, self.cout_s, self.cin0, self.c0s, cin_s)

    def direct(self) -> torch.Tensor:
        r"""[tap][cout_s][cin_s] (K contiguous), zero padded (az_pack_conv_weight_f32)."""
        n, args = self._direct_args(1)
        return self._form("direct", n, torch.float32, "az_pack_conv_weight_f32", *args)

    def stem(self) -> torch.Tensor:
        r"""(3, 3, cin, cout_s): tap-major, output channels contiguous (``az_conv2d_stem_f32``)."""
        if "stem" not in self._forms:
            w = torch.zeros(self.ks, self.ks, self.cin, self.cout_s, dtype=torch.float32, device=self.device)
            w[..., : self.cout] = self.w.permute(2, 3, 1, 0)
            self._forms["stem"] = w.contiguous()
        return self._forms["stem"]

    def direct_half(self, f16: bool) -> torch.Tensor:
        r"""The direct layout in bf16 (``f16=False``) or IEEE half, for ``az_conv2d_{bf16,f16}_f32``."""
        n, args = self._direct_args(1)
        return self._form(("half", f16), n, torch.int16, "az_pack_conv_weight_half_f32", *args, int(f16))

    def direct_x3(self) -> torch.Tensor:
        r"""The direct layout as three bf16 planes (w = w1 + w2 + w3 exactly), for ``az_conv2d_x3_f32``."""
        n, args = self._direct_args(3)
        return self._form("x3", n, torch.int16, "az_pack_conv_weight_x3_f32", *args)

    def w_scale(self, winograd: bool) -> float:
        r"""The power of two the f16x2 packings multiply the weights by (``az_f16x2_weight_scale``: the largest magnitude -- of
        the Winograd-domain filter when ``winograd`` -- lands in [2^13, 2^14)); handed to the kernels as ``AzConvArgs.w_scale``."""
        if self._amax is None:
            self._amax = float(self.w.abs().max()) if self.w.numel() else 0.0
        return float(_lib.lib().az_f16x2_weight_scale(self._amax, int(winograd)))

    def h2_range(self) -> bool:
        r"""Every output row's largest |w| within 2^16 of the tensor's (rows of exact zeros aside).  The f16x2 packings scale the
        WHOLE tensor by one power of two, so a row further down has subnormal low pieces and loses precision (a fused q | k | v
        projection whose keys carry a gain the queries give back: tests/test_gpu_magnitudes.py); such layers run bf16x3."""
        if self._h2_range is None:
            r = self.w.abs().amax(dim=(1, 2, 3))
            r = r[r > 0]
            self._h2_range = bool(r.numel() == 0 or float(r.min()) * 2.0 ** 16 >= float(r.max()))
        return self._h2_range

    def direct_f16x2(self) -> torch.Tensor:
        r"""The direct layout as three IEEE half planes [wh | wl | wh / 2^11] of w * w_scale, for ``az_conv2d_f16x2_f32``."""
        n, args = self._direct_args(3)
        return self._form("h2", n, torch.int16, "az_pack_conv_weight_f16x2_f32", *args, self.w_scale(False))

    def _wino_args(self, step: int, pieces: int) -> tuple:
        nk0, nk1 = (self.c0s + step - 1) // step, (self.c1s + step - 1) // step
        cb = (self.cout_s + 63) // 64
        return (nk0 + nk1) * cb * 16 * 64 * step * pieces, (self.cout, self.cin, self.cin0, nk0, nk0 + nk1, cb)

    def winograd_f16x2(self) -> torch.Tensor:
        r"""The x3 Winograd filter layout with the f16x2 pieces of U * w_scale, for ``az_conv2d_winograd_f16x2_f32``."""
        n, args = self._wino_args(16, 3)
        return self._form("wino_h2", n, torch.int16, "az_winograd_pack_filter_f16x2_f32", *args, self.w_scale(True))

    def winograd(self) -> torch.Tensor:
        r"""Filter transform U = G g G^T (az_winograd_pack_filter_f32: fp64 accumulate, one-off) laid out
        [8-channel chunk][64-cout block][16 frequencies][64][8]; source 1 starts on a chunk boundary."""
        n, args = self._wino_args(8, 1)
        return self._form("wino", n, torch.float32, "az_winograd_pack_filter_f32", *args)

    def winograd_x3(self) -> torch.Tensor:
        r"""The same filter transform as three bf16 pieces in MFMA fragment order, 16-channel steps
        (az_winograd_pack_filter_x3_f32), for ``az_conv2d_winograd_x3_f32``; source 1 starts on a step boundary."""
        n, args = self._wino_args(16, 3)
        return self._form("wino_x3", n, torch.int16, "az_winograd_pack_filter_x3_f32", *args)

    def winograd4(self) -> torch.Tensor:
        r"""F(4x4,3x3) filter transform (az_winograd4_pack_filter_f32) laid out
        [4-channel chunk][64-cout block][36 frequencies][64][4]."""
        nk, cb = (self.c0s + self.c1s) // 4, (self.cout_s + 63) // 64
        return self._form("wino4", nk * cb * 36 * 64 * 4, torch.float32, "az_winograd4_pack_filter_f32",
                          self.cout, self.cin, self.cin0, self.c0s, nk, cb)


class Builder:
    r"""Emits kernels onto a tape; owns the pool, packed weights and the split-K workspace."""

    def __init__(self, device: torch.device, half: torch.dtype | None = None, half_act: bool = False) -> None:
        r"""``half``: torch.bfloat16 / torch.float16 routes every conv / token GEMM through the half-operand MFMA
        kernel (fp32 accumulate) -- set by the plans of modules cast to half precision.  ``half_act``: the plan also keeps its
        activations in HBM in that type (HALF_ACT; channel strides are then multiples of 8)."""
        self.device = device
        self.half = half if half in (torch.bfloat16, torch.float16) else None
        self.half_act = bool(half_act) and self.half is not None and HALF_ACT
        self.tape = Tape()
        self.pool = Pool(device)
        self._ws_need = 0
        self._ws_users: list[AzConvArgs] = []
        self.workspace: torch.Tensor | None = None
        self._writes = 0  # launches that reported a write (Builder.wrote) so far
        self._last_write: dict[int, int] = {}  # allocation (storage address) -> serial of its last write

    # -- buffers ---------------------------------------------------------------------------
    def pad(self, c: int) -> int:
        r"""Channel stride of this plan's activations: multiples of 4 floats, or of 8 two-byte values (16-byte vectors either way)."""
        return pad8(c) if self.half_act else pad4(c)

    def new_act(self, B: int, H: int, W: int, C_: int, pinned: bool = False, f32: bool = False) -> Act:
        r"""``f32``: an fp32 tensor also in a half-activation plan (the plan's input / output tensors)."""
        cs = self.pad(C_)
        dtype = self.half if (self.half_act and not f32) else torch.float32
        return Act(self.pool.alloc(B * H * W * cs, dtype), B, H, W, C_, cs, pinned)

    def free(self, a: Act) -> None:
        if not a.pinned:
            self.pool.release(a.buf)

    def const(self, t: torch.Tensor) -> torch.Tensor:
        t = t.detach().to(device=self.device, dtype=torch.float32).contiguous()
        self.tape.keep.append(t)
        return t

    def empty(self, *shape) -> torch.Tensor:
        t = torch.empty(*shape, dtype=torch.float32, device=self.device)
        self.tape.keep.append(t)
        return t

    # -- weights ---------------------------------------------------------------------------
    def pack_conv(self, weight: torch.Tensor, bias: torch.Tensor | None, cin0: int | None = None) -> "ConvWeights":
        r"""Wraps torch (cout, cin, k, k) [or (cout, cin) / (cout, cin, 1)] weights; the kernel-specific
        packed forms (direct implicit GEMM, Winograd) are materialised on first use."""
        cw = ConvWeights(self, weight, bias, cin0)
        self.tape.keep.append(cw)
        return cw

    # -- kernels ---------------------------------------------------------------------------
    def conv(
        self,
        src0: Act,
        packed,
        cout: int,
        *,
        src1: Act | None = None,
        up0: int = 0,
        up1: int = 0,
        hin: int | None = None,
        win: int | None = None,
        stride: int | tuple = 1,
        act: int = 0,
        gate: torch.Tensor | None = None,
        gate_off: int = 0,
        gate_bstride: int = 0,
        res: Act | None = None,
        res_up: int = 0,
        dst_nchw: torch.Tensor | None = None,
        winograd: bool | int | None = None,
        periodic: bool = False,
        gn_stats: bool = False,
        out: Act | None = None,
        depth: tuple | None = None,
        qk_prep: dict | None = None,
        out_f32: bool = False,
    ) -> Act | None:
        ks, bias = packed.ks, packed.bias
        pad = ks // 2
        B = src0.B
        # (height, width) pairs select the anisotropic descriptor (a stride sequence such as (2, 1), unet.py:159-186)
        (stride, stride_w), (up0, up0_w), (up1, up1_w) = (v if isinstance(v, (tuple, list)) else (v, v) for v in (stride, up0, up1))
        aniso = stride != stride_w or up0 != up0_w or up1 != up1_w
        hin = src0.H << up0 if hin is None else hin
        win = src0.W << up0_w if win is None else win
        hout = (hin + 2 * pad - ks) // stride + 1
        wout = (win + 2 * pad - ks) // stride_w + 1
        a = AzConvArgs()
        a.src0, a.c0s, a.up0, a.h0, a.w0 = src0.ptr, src0.cs, up0, src0.H, src0.W
        if aniso:
            a.aniso, a.stride_w, a.up0_w, a.up1_w = 1, stride_w, up0_w, up1_w
        if src1 is not None:
            a.src1, a.c1s, a.up1, a.h1, a.w1 = src1.ptr, src1.cs, up1, src1.H, src1.W
        assert (a.c0s, a.c1s) == (packed.c0s, packed.c1s), "weights were packed for different source strides"
        a.batch, a.hin, a.win = B, hin, win
        if depth is not None:  # (planes per volume, depth tap offset[, circular]): one depth tap of a 3-D convolution over all planes at once
            assert (src1 is None or src1.B == B) and B % depth[0] == 0
            a.depth, a.depth_shift = depth[0], depth[1]
            a.depth_wrap = int(bool(depth[2])) if len(depth) > 2 else 0
        a.bias = bias.data_ptr() if bias is not None else None
        a.cout_s = self.pad(cout)
        if self.half_act:  # typed tensors (AzConvArgs.src_dtype / dst_dtype): sources as they are, the destination in the module's type
            assert src1 is None or src1.half == src0.half, "both sources in one element type"
            a.src_dtype = int(src0.half)
        a.ksize, a.stride, a.pad = ks, stride, pad
        a.pad_mode = 1 if (periodic and pad > 0) else 0
        a.hout, a.wout = hout, wout
        a.act = act
        if gate is not None:
            a.gate = gate.data_ptr() + 4 * gate_off
            a.gate_bstride = gate_bstride
        if res is not None:
            if isinstance(res, SharedResidual):  # (a positional embedding table)
                res = res.act
                a.res_bcast = 1
            a.res, a.res_up, a.hres, a.wres = res.ptr, res_up, res.H, res.W
            assert res.cs == a.cout_s
        if dst_nchw is not None:
            out = None
            a.dst, a.dst_nchw, a.dst_c = dst_nchw.data_ptr(), 1, cout
        else:
            if out is None:
                if act == 4:  # SwiGLU epilogue: half the channels come out (y[c] = x[2c] * silu(x[2c+1]))
                    assert cout % 8 == 0 and gate is None and res is None, "SwiGLU epilogue: cout % 8 == 0, no gate / residual"
                    assert not self.half_act or cout % 16 == 0
                    out = self.new_act(B, hout, wout, cout // 2, f32=out_f32)
                else:
                    out = self.new_act(B, hout, wout, cout, f32=out_f32)
            else:  # caller-owned destination (a plane range of a volume; may alias `res`: in-place accumulation)
                assert (out.B, out.H, out.W, out.C, out.cs) == (B, hout, wout, cout, self.pad(cout)), "destination shape"
            a.dst = out.ptr
            a.dst_dtype = int(out.half)
            if res is not None:
                assert res.half == out.half, "the residual has the destination's element type"
        npix = B * hout * wout
        cin_s = a.c0s + a.c1s
        lib = _lib.lib()
        ch = choose_conv(ConvLayer(ks, stride, aniso, B, hout, wout, a.c0s, a.c1s, cout, a.cout_s, up0, depth is not None, self.half,
                                   winograd, self._source(src0), self._source(src1) if src1 is not None else None,
                                   self.half is not None or FP32_MFMA != "f16x2" or packed.h2_range()))
        name = ch.name
        a.weight = (packed.direct_half(self.half == torch.float16) if self.half is not None else getattr(packed, PACKED[name])()).data_ptr()
        if ch.h2:
            a.w_scale = packed.w_scale(name == "az_conv2d_winograd_f16x2_f32")
        if name == "az_conv2d_winograd4_f32":
            a.splitk = lib.az_conv2d_winograd4_suggest_splitk(B, hout, wout, a.cout_s, cin_s)
        elif name in ("az_conv2d_winograd_f32", *WINO_X3_NAMES):
            a.splitk = lib.az_conv2d_winograd_suggest_splitk(B, hout, wout, a.cout_s, cin_s)
        elif name in ("az_conv2d_x3_f32", "az_conv2d_f16x2_f32") or (self.half is not None and a.c0s % 64 == 0 and a.c1s % 64 == 0):
            a.splitk = lib.az_conv2d_x3_suggest_splitk(C.byref(a))  # (the 256 x 256-tile kernel has its own rule where it takes the launch)
        else:
            a.splitk = lib.az_conv2d_suggest_splitk(npix, a.cout_s, cin_s, ks)
        if ch.dyn:
            a.in_absmax0 = self.absmax_of(src0).data_ptr()
            a.in_absmax1 = self.absmax_of(src1).data_ptr() if src1 is not None else None
        tmp_src = None
        if src0.affine is not None:  # a normalisation whose apply pass has not run (group_norm(lazy=True))
            ST, in_act = src0.affine
            # the apply pass inside the gather (the fp32 kernel on a source of the output's size only; the x3 kernel's patch masks
            # live in output coordinates, so it also reads a nearest-upsampled source)
            if src1 is None and a.c0s % 8 == 0 and not aniso and (
                    name in WINO_X3_NAMES or (name == "az_conv2d_winograd_f32" and up0 == 0)):
                a.in_affine, a.in_act = ST.data_ptr(), in_act
            else:
                tmp_src = self.materialize(src0)
                a.src0 = tmp_src.ptr
        moments = None
        if gn_stats and GN_FUSED and out is not None and cout == a.cout_s:
            if (name in ("az_conv2d_winograd_f32", *WINO_X3_NAMES) and a.splitk == 1 and cout % 64 == 0 and hout % 2 == 0
                    and wout % 2 == 0 and ((hout // 2) * (wout // 2)) % 64 == 0):
                # the output feeds a GroupNorm: its epilogue also writes per-(tile block, channel quad) moments
                moments = self._moments(a, B, cout, ((hout // 2) * (wout // 2)) // 64)
            elif GN_FUSED_SPLITK and a.splitk > 1 and name != "az_conv2d_winograd4_f32" and not (name == "az_conv2d_f32" and a.cout_s == 4):
                # split-K layers (the small maps): the combine kernel leaves the moments, one partial per (image, pixel chunk, quad)
                hw = hout * wout
                # a workgroup of the combine kernel = 256 // quads pixel slots; about 2 pixels per thread (each costs splitk
                # dependent-latency loads: parallelism, not bandwidth, decides), at most 128 partials per image (two finalize passes)
                cpix = 2 * max(1, 256 // (cout // 4))
                chunks = max(1, min(128, (hw + cpix - 1) // cpix))
                while (hw + chunks - 1) // chunks * (chunks - 1) >= hw:
                    chunks -= 1
                moments = self._moments(a, B, cout, chunks)
        if (qk_prep is not None and QK_PREP and name in ("az_conv2d_f32", "az_conv2d_bf16_f32", "az_conv2d_f16_f32", "az_conv2d_x3_f32", "az_conv2d_f16x2_f32")
                and a.splitk == 1 and act == 0 and gate is None and res is None and out is not None and a.cout_s == cout
                and qk_prep["head_dim"] in (32, 64, 128) and cout == 3 * qk_prep["heads"] * qk_prep["head_dim"]):
            self._qk_prep(a, qk_prep, name, hout * wout)
        if a.splitk > 1:
            self._ws_need = max(self._ws_need, a.splitk * npix * a.cout_s)
            self._ws_users.append(a)
        a._flops = 2 * npix * cout * (src0.C + (src1.C if src1 is not None else 0)) * ks * ks  # algorithmic
        a._algo = name
        self.tape.add(name, C.byref(a), keep=[a] if gate is None else [gate, a])  # the descriptor holds raw addresses
        if tmp_src is not None:
            self.free(tmp_src)
        if out is not None:
            # (not bounded, whatever its sources: the weights set its magnitude -- Act.bounded)
            self.wrote(out, bounded=False, moments=moments)
            out.qk_prepared = a.act == 5
        return out

    def _source(self, s: Act) -> ConvSource:
        return ConvSource(s.C, s.buf.numel(), s.bounded, s.affine is not None, self.fact(s, s.absmax) is not None,
                          self.fact(s, s.gn_quads) is not None)

    def _moments(self, a: AzConvArgs, B: int, cout: int, chunks: int) -> tuple:
        r"""Per-(image, chunk, channel quad) GroupNorm moments of the output, written by the launch of ``a``."""
        quads = self.empty(B * chunks * (cout // 4) * 4)
        a.gn_quads, a.gn_chunks = quads.data_ptr(), chunks
        return quads, chunks

    def _qk_prep(self, a: AzConvArgs, qk_prep: dict, name: str, tokens: int) -> None:
        r"""The fused q | k | v projection of an attention layer: q / k RMS norm, gains and RoPE in THIS epilogue, once per
        layer, instead of in every workgroup of the attention kernel (three per head at 288 tokens: 123 -> 163 us)."""
        a.act = 5
        if name != "az_conv2d_f32" and _lib.lib().az_conv2d_x3_suggest_splitk(C.byref(a)) != 1:
            a.act = 0  # (the tile plan of THIS epilogue wants a split K walk, which the epilogue cannot take: plain projection)
            return
        a.qk_head_dim, a.qk_heads, a.qk_tokens = qk_prep["head_dim"], qk_prep["heads"], tokens
        a.qk_rmsnorm, a.qk_eps = int(qk_prep["rmsnorm"]), qk_prep["eps"]
        for key, fields in (("weight", ("qk_q_weight", "qk_k_weight")), ("rope", ("qk_rope_cos", "qk_rope_sin"))):
            if qk_prep.get(key) is not None:
                for f, t in zip(fields, qk_prep[key]):
                    setattr(a, f, t.data_ptr())
                self.tape.keep.extend(qk_prep[key])

    def conv_stem(self, x: torch.Tensor, B: int, cin: int, H: int, W: int, packed: "ConvWeights", cout: int, *,
                  periodic: bool = False, gn_stats: bool = False) -> Act:
        r"""The network's first 3 x 3 convolution reading its <= 4 input channels PLANAR -- ``x`` is the (B, cin, H, W) latent
        as the sampler holds it (``az_conv2d_stem_f32``): no NHWC copy of the latent, no matrix kernel for 27 multiplies."""
        assert packed.ks == 3 and 1 <= cin <= 4 and packed.cin == cin and cout % 4 == 0 and self.half is None
        a = AzConvArgs()
        a.src0, a.c0s, a.h0, a.w0 = x.data_ptr(), cin, H, W
        a.batch, a.hin, a.win, a.hout, a.wout = B, H, W, H, W
        a.weight = packed.stem().data_ptr()
        a.bias = packed.bias.data_ptr() if packed.bias is not None else None
        a.cout_s, a.ksize, a.stride, a.pad, a.splitk = cout, 3, 1, 1, 1
        a.pad_mode = 1 if periodic else 0
        out = self.new_act(B, H, W, cout)
        a.dst = out.ptr
        moments = self._moments(a, B, cout, ((H + 7) // 8) * ((W + 31) // 32)) if gn_stats and GN_FUSED else None
        a._flops = 0  # (27 multiplies per output on the vector ALUs: a store-bound pass, accounted by its bytes in bench.py)
        a._algo = "az_conv2d_stem_f32"
        self.tape.add("az_conv2d_stem_f32", C.byref(a), keep=[a, x])
        return self.wrote(out, bounded=False, moments=moments)

    # -- content facts -------------------------------------------------------------------------
    def wrote(self, y: Act, *, bounded: bool, moments: tuple | None = None) -> Act:
        r"""Every launch that writes an activation reports here, after it is on the tape.  Facts recorded about the allocation's
        earlier contents (through any view of it) go stale; ``bounded`` states the producer's rule for the new contents
        (Act.bounded), ``moments`` the (partials, chunks) GroupNorm record the same launch wrote of them."""
        self._writes += 1
        self._last_write[y.buf.untyped_storage().data_ptr()] = self._writes
        y.bounded, y.absmax = bounded, None
        y.gn_quads = (*moments, self._writes) if moments is not None else None
        return y

    def fact(self, x: Act, rec: tuple | None) -> tuple | None:
        r"""``rec`` (x.absmax / x.gn_quads) if it still describes what x's allocation holds, else None."""
        return rec if rec is not None and rec[-1] == self._last_write.get(x.buf.untyped_storage().data_ptr()) else None

    def absmax_of(self, x: Act) -> torch.Tensor:
        r"""The AZ_ABSMAX_SLOTS partial maxima of |x| (``az_absmax_f32``: one streaming pass, recorded once per tensor contents and
        shared by its consumers) -- the activation scale of an f16x2 launch on an unbounded input (``AzConvArgs.in_absmax0 / in_absmax1``)."""
        if self.fact(x, x.absmax) is None:
            assert not x.half and x.affine is None
            slots = self.empty(256)
            moments = self.fact(x, x.gn_quads)
            if moments is not None and F16X2_MOMENTS:
                # the producing convolution left GroupNorm moments of this tensor: |x| <= |mean| + sqrt(M2) per record -- an upper
                # bound of the maximum for the price of reading the records (az_absmax_from_moments_f32)
                self.tape.add("az_absmax_from_moments_f32", slots.data_ptr(), moments[0].data_ptr(), moments[0].numel() // 4, keep=[moments[0]])
            else:
                self.tape.add("az_absmax_f32", slots.data_ptr(), x.ptr, x.B * x.H * x.W * x.cs, keep=[x.buf])
            x.absmax = (slots, self._last_write.get(x.buf.untyped_storage().data_ptr()))
        return x.absmax[0]

    def upsample_nearest(self, x: Act, sh: int, sw: int, hout: int, wout: int) -> Act:
        r"""``narrow(Upsample(scale_factor=(sh, sw), mode="nearest")(x), (hout, wout))`` as a pass of its own -- only for
        factors that are not powers of two (those are a shift inside the consuming convolution's gather)."""
        y = self.new_act(x.B, hout, wout, x.C)
        self.tape.add("az_upsample_nearest_f32", y.ptr, x.ptr, x.B, x.H, x.W, x.cs, sh, sw, hout, wout)
        return self.wrote(y, bounded=False)

    # -- input gradient (csrc/backward.hip) --------------------------------------------------------------------
    # Every tensor below is a cotangent: it has no natural range, so every gradient Act is ``bounded=False`` and the
    # fixed-scale f16x2 kernels never see one (choose_conv gives them the measured-scale f16x2 form or bf16x3).
    def conv_dgrad(self, g: Act, conv, *, cin_lo: int = 0, cin_hi: int | None = None, res: Act | None = None,
                   dst_nchw: torch.Tensor | None = None, cache: dict | None = None, winograd=None) -> Act | None:
        r"""Data gradient of a stride-1 'same' convolution ``conv`` (a module holding ``weight`` of shape (cout, cin, k...)): the
        forward convolution kernels over the cotangent ``g`` with the weight transposed (cin <-> cout) and flipped by 180 degrees,
        for the input channels [cin_lo, cin_hi) (one source of a concatenation); ``res`` is added in the epilogue (a tensor
        consumed twice: its cotangents add).  A strided convolution takes the zero-stuffed cotangent (:meth:`zero_stuff`).
        The packed weight is made once per (module, channel range) and plan (``cache``)."""
        w = conv.weight
        cin_hi = w.shape[1] if cin_hi is None else cin_hi
        key = (id(conv), cin_lo, cin_hi)
        packed = None if cache is None else cache.get(key)
        if packed is None:
            wt = w.detach()[:, cin_lo:cin_hi].transpose(0, 1).flip(*range(2, w.ndim)).contiguous()
            packed = self.pack_conv(wt, None)
            if cache is not None:
                cache[key] = packed
        assert g.C == w.shape[0], "the cotangent has the convolution's output channels"
        return self.conv(g, packed, cin_hi - cin_lo, res=res, dst_nchw=dst_nchw, winograd=winograd)

    def channel_scale(self, x: Act, s: torch.Tensor, s_off: int, bstride: int, out: Act | None = None) -> Act:
        r"""y = x * s[b, c] per (sample, channel): the gate of ``out = x + c * y`` on the way back."""
        y = self.new_act(x.B, x.H, x.W, x.C) if out is None else out
        self.tape.add("az_channel_scale_f32", y.ptr, x.ptr, s.data_ptr() + 4 * s_off, bstride, x.B, x.H * x.W, x.C, x.cs, keep=[s])
        return self.wrote(y, bounded=False)

    def silu_bwd(self, g: Act, p: Act) -> Act:
        r"""g <- g * silu'(p) in place (``p``: the kept PRE-activation)."""
        assert (g.B, g.H, g.W, g.cs) == (p.B, p.H, p.W, p.cs)
        self.tape.add("az_silu_bwd_f32", g.ptr, g.ptr, p.ptr, g.B * g.H * g.W * g.cs, keep=[p.buf])
        return self.wrote(g, bounded=False)

    def silu(self, x: Act) -> Act:
        r"""y = silu(x) as a pass of its own (the forward-keep tape keeps the pre-activation and applies SiLU behind it)."""
        y = self.new_act(x.B, x.H, x.W, x.C)
        self.tape.add("az_silu_f32", y.ptr, x.ptr, x.B * x.H * x.W * x.cs)
        return self.wrote(y, bounded=False)

    def group_norm_bwd(self, x: Act, g: Act, saved: dict, *, scale=None, scale_off=0, bstride=0, res: Act | None = None) -> Act:
        r"""Pullback of ``(1 + scale) * GN(x) + shift`` w.r.t. x, plus ``res``; ``saved`` from :meth:`group_norm`."""
        B, HW = x.B, x.H * x.W
        nchunks = int(min(512, max(1, (HW * x.cs * 4) // 65536)))
        bpart = self.empty(B * nchunks * saved["groups"] * 4)
        sp = scale.data_ptr() + 4 * scale_off if scale is not None else None
        fp, fchunks = saved["partials"], saved["nchunks"]
        self.tape.add("az_groupnorm_bwd_stats_f32", bpart.data_ptr(), x.ptr, g.ptr, sp, bstride, fp.data_ptr(), fchunks, B, HW, x.C, x.cs,
                      saved["groups"], nchunks, saved["eps"], keep=[fp, scale, x.buf])
        y = self.new_act(B, x.H, x.W, x.C)
        self.tape.add("az_groupnorm_bwd_apply_f32", y.ptr, x.ptr, g.ptr, res.ptr if res is not None else None, sp, bstride,
                      fp.data_ptr(), fchunks, bpart.data_ptr(), nchunks, B, HW, x.C, x.cs, saved["groups"], saved["eps"])
        return self.wrote(y, bounded=False)

    def row_norm_bwd(self, x: Act, g: Act, kind: int, *, scale=None, scale_off=0, bstride=0, res: Act | None = None, eps=1e-5,
                     weight: torch.Tensor | None = None) -> Act:
        r"""Pullback of ``(1 + scale) * weight * norm(x) + shift`` over the channel axis (kind 0: layer, unbiased variance; 1: rms),
        plus ``res``.  ``weight``: a learned per-channel gain (C floats on the device) -> ``az_rownorm_bwd_w_f32``."""
        y = self.new_act(x.B, x.H, x.W, x.C)
        sp = scale.data_ptr() + 4 * scale_off if scale is not None else None
        rp = res.ptr if res is not None else None
        if weight is None:
            self.tape.add("az_rownorm_bwd_f32", y.ptr, x.ptr, g.ptr, rp, sp, bstride, x.B * x.H * x.W, x.H * x.W, x.C, x.cs,
                          kind, eps, keep=[scale, x.buf])
        else:
            assert weight.numel() == x.C and weight.dtype == torch.float32
            self.tape.add("az_rownorm_bwd_w_f32", y.ptr, x.ptr, g.ptr, rp, sp, bstride, weight.data_ptr(), x.B * x.H * x.W, x.H * x.W,
                          x.C, x.cs, kind, eps, keep=[scale, x.buf, weight])
        return self.wrote(y, bounded=False)

    def zero_stuff(self, g: Act, sh: int, sw: int, H: int, W: int) -> Act:
        r"""The cotangent of a convolution with stride (sh, sw) on the zero-filled (H, W) grid of its input."""
        y = self.new_act(g.B, H, W, g.C)
        self.tape.add("az_zero_stuff_f32", y.ptr, g.ptr, g.B, g.H, g.W, g.cs, sh, sw, H, W)
        return self.wrote(y, bounded=False)

    def upsample_nearest_bwd(self, g: Act, sh: int, sw: int, h: int, w: int) -> Act:
        r"""Pullback of ``narrow(Upsample(nearest, (sh, sw)))``: (B, hn, wn) cotangent -> (B, h, w) window sums."""
        y = self.new_act(g.B, h, w, g.C)
        self.tape.add("az_upsample_nearest_bwd_f32", y.ptr, g.ptr, g.B, h, w, g.cs, sh, sw, g.H, g.W)
        return self.wrote(y, bounded=False)

    # -- input gradient through attention (csrc/attention_bwd.hip) and the DiT block's FFN activations -----------------
    def act(self, x: Act, kind: int) -> Act:
        r"""y = act(x) as a pass of its own (kind 1: silu, 2: relu, 3: relu^2) behind a kept pre-activation."""
        y = self.new_act(x.B, x.H, x.W, x.C)
        self.tape.add("az_act_f32", y.ptr, x.ptr, x.B * x.H * x.W * x.cs, kind)
        return self.wrote(y, bounded=False)

    def act_bwd(self, g: Act, p: Act, kind: int) -> Act:
        r"""g <- g * act'(p) in place (``p``: the kept PRE-activation; kinds of :meth:`act`)."""
        assert (g.B, g.H, g.W, g.cs) == (p.B, p.H, p.W, p.cs)
        self.tape.add("az_act_bwd_f32", g.ptr, g.ptr, p.ptr, g.B * g.H * g.W * g.cs, kind, keep=[p.buf])
        return self.wrote(g, bounded=False)

    def swiglu(self, x: Act) -> Act:
        r"""y[c] = x[2c] * silu(x[2c+1]) as a pass of its own (``x``: the kept pre-activation)."""
        y = self.new_act(x.B, x.H, x.W, x.C // 2)
        self.tape.add("az_swiglu_f32", y.ptr, x.ptr, x.B * x.H * x.W, x.C // 2, x.cs, y.cs)
        return self.wrote(y, bounded=False)

    def swiglu_bwd(self, g: Act, p: Act) -> Act:
        r"""Cotangent of the SwiGLU output -> cotangent of its (twice as wide) kept pre-activation ``p``."""
        assert (g.B, g.H, g.W, 2 * g.C) == (p.B, p.H, p.W, p.C)
        y = self.new_act(p.B, p.H, p.W, p.C)
        self.tape.add("az_swiglu_bwd_f32", y.ptr, g.ptr, p.ptr, p.B * p.H * p.W, g.C, p.cs, g.cs, keep=[p.buf])
        return self.wrote(y, bounded=False)

    def _attn_mask(self, mask: torch.Tensor, B: int, heads: int, L: int) -> tuple:
        r"""(byte mask on the device, batch stride, head stride) of a boolean mask -- (L, L) or (B | 1, 1 | H, L, L), True = attend
        (reference attention.py:97-104) -- as the attention kernels read it."""
        m = mask[None, None] if mask.ndim == 2 else mask
        if m.ndim != 4 or m.shape[-2:] != (L, L) or m.shape[0] not in (1, B) or m.shape[1] not in (1, heads):
            raise ValueError(f"attention mask of shape {tuple(mask.shape)} does not broadcast to ({B}, {heads}, {L}, {L})")
        m8 = (m != 0).to(device=self.device, dtype=torch.uint8).contiguous()
        self.tape.keep.append(m8)
        return m8, (m8.stride(0) if m.shape[0] > 1 else 0), (m8.stride(1) if m.shape[1] > 1 else 0)

    def attention_keep(self, qkv: Act, heads: int, qk_rmsnorm: bool, scale: float, eps: float = 1e-5, rope: tuple | None = None,
                       mask: torch.Tensor | None = None, norm_dim: int = 0, order: str = "3HC", skip_prep: bool = False,
                       qk_weight: tuple | None = None) -> tuple[Act, dict]:
        r"""The forward of :meth:`attention` ('(n H C)' order, fp32) with what :meth:`attention_bwd` reads kept: q^ | k^ =
        rope(rms_norm(q | k)) go out of place into a buffer of their own (``az_qk_prep_f32``), then the forward attention entry
        :func:`choose_attention` picks runs on (q^, k^, v) with no norm and no tables.  Returns (out, record); ``qkv``, q^ | k^
        and ``out`` must stay alive for the pullback (the caller does not free them).  ``order``: the token layout of ``qkv`` as in
        :meth:`attention` ("3HC" / "nHC", or "H3C": guided-diffusion's legacy order).  ``skip_prep``: without RMS norm and RoPE
        q^ = q and k^ = k, so the copy is skipped and the kernels read q and k where they lie (they take any strides).
        ``qk_weight = (wq, wk)``: learned gains of head_dim floats between the RMS norm and the rotation, as in :meth:`attention`
        (``az_qk_prep_w_f32``); the record carries them to :meth:`attention_bwd`."""
        from ._lib import AzAttnArgs

        Cq = qkv.C // 3
        dim = Cq // heads
        assert qkv.cs == qkv.C and dim * heads == Cq and not qkv.half and self.half is None
        assert dim in ATTN_GRAD_HEAD_DIMS, dim
        B, L = qkv.B, qkv.H * qkv.W
        offs, hs = qkv_layout(order, Cq, dim)
        cos, sin = rope if rope is not None else (None, None)
        prep = not (skip_prep and not qk_rmsnorm and rope is None and qk_weight is None)
        qk = None
        if qk_weight is not None:
            assert all(w.numel() == dim and w.dtype == torch.float32 for w in qk_weight)
        if prep:
            qk = self.new_act(B, qkv.H, qkv.W, 2 * Cq, pinned=True)
            args = (qk.ptr, qk.ptr + 4 * Cq, qkv.ptr + 4 * offs[0], qkv.ptr + 4 * offs[1], B, L, heads, dim,
                    L * qkv.cs, qkv.cs, hs, L * qk.cs, qk.cs, dim, int(qk_rmsnorm), norm_dim, eps,
                    cos.data_ptr() if cos is not None else None, sin.data_ptr() if sin is not None else None)
            if qk_weight is None:
                self.tape.add("az_qk_prep_f32", *args, keep=[qkv.buf, cos, sin])
            else:
                self.tape.add("az_qk_prep_w_f32", *args, qk_weight[0].data_ptr(), qk_weight[1].data_ptr(),
                              keep=[qkv.buf, cos, sin, *qk_weight])
            self.wrote(qk, bounded=False)
        out = self.new_act(B, qkv.H, qkv.W, Cq)
        a = AzAttnArgs()
        qt, qo, ko, qh = (qk, 0, Cq, dim) if prep else (qkv, offs[0], offs[1], hs)  # (q^ | k^, or q and k where they lie)
        a.q, a.k, a.v, a.out = qt.ptr + 4 * qo, qt.ptr + 4 * ko, qkv.ptr + 4 * offs[2], out.ptr
        a.batch, a.heads, a.tokens, a.head_dim = B, heads, L, dim
        _token_strides(a, L, q=(qt, qh), k=(qt, qh), v=(qkv, hs), o=(out, dim))
        a.scale, a.qk_rmsnorm, a.eps, a.norm_dim = scale, 0, eps, 0
        rec = dict(qkv=qkv, qk=qk, out=out, heads=heads, dim=dim, scale=scale, eps=eps, rms=bool(qk_rmsnorm), norm_dim=norm_dim,
                   rope=rope, mask=None, offs=offs, hs=hs, qk_weight=qk_weight)
        if mask is not None:
            m8, mb, mh = rec["mask"] = self._attn_mask(mask, B, heads, L)
            a.mask, a.mask_bstride, a.mask_hstride = m8.data_ptr(), mb, mh
        a._flops = 4 * B * heads * L * L * dim
        self.tape.add(choose_attention(dim, qk_in_h2_domain(qk_rmsnorm, dim, norm_dim, scale, qk_weight), None), C.byref(a),
                      keep=[a, qk.buf if prep else qkv.buf])
        return self.wrote(out, bounded=False), rec

    def attention_bwd(self, g: Act, rec: dict) -> Act:
        r"""Cotangent ``g`` of the attention output -> cotangent of the fused q | k | v token tensor: ``az_attention_bwd_f32``
        (dq^ | dk^ into a temporary, dv straight into its third) and ``az_qk_prep_bwd_f32`` (the q and k thirds); one launch where
        q^ = q and k^ = k."""
        from ._lib import AzAttnBwdArgs

        qkv, qk, out, heads, dim = rec["qkv"], rec["qk"], rec["out"], rec["heads"], rec["dim"]
        Cq = heads * dim
        offs, hs = rec.get("offs", (0, Cq, 2 * Cq)), rec.get("hs", dim)
        B, L = qkv.B, qkv.H * qkv.W
        assert (g.B, g.H, g.W, g.C) == (out.B, out.H, out.W, out.C)
        dqkv = self.new_act(B, qkv.H, qkv.W, 3 * Cq)
        if qk is None:  # in place (attention_keep(skip_prep=True)): q^ | k^ and their cotangents live in qkv / dqkv themselves
            qt, dqt, qh, qo, ko = qkv, dqkv, hs, offs[0], offs[1]
        else:  # q^ | k^ in a buffer of their own: dq^ | dk^ into a temporary, az_qk_prep_bwd_f32 takes them to the q and k thirds
            qt, dqt, qh, qo, ko = qk, self.new_act(B, qkv.H, qkv.W, 2 * Cq), dim, 0, Cq
        a = AzAttnBwdArgs()
        a.q, a.k, a.v, a.out, a.dout = qt.ptr + 4 * qo, qt.ptr + 4 * ko, qkv.ptr + 4 * offs[2], out.ptr, g.ptr
        a.dq, a.dk, a.dv = dqt.ptr + 4 * qo, dqt.ptr + 4 * ko, dqkv.ptr + 4 * offs[2]
        a.workspace = self.empty(2 * B * heads * L).data_ptr()
        a.batch, a.heads, a.tokens, a.head_dim, a.scale = B, heads, L, dim, rec["scale"]
        _token_strides(a, L, q=(qt, qh), k=(qt, qh), v=(qkv, hs), o=(out, dim), do=(g, dim), dq=(dqt, qh), dk=(dqt, qh), dv=(dqkv, hs))
        if rec["mask"] is not None:
            m8, mb, mh = rec["mask"]
            a.mask, a.mask_bstride, a.mask_hstride = m8.data_ptr(), mb, mh
        a._flops = 16 * B * heads * L * L * dim
        self.tape.add("az_attention_bwd_f32", C.byref(a), keep=[a, qt.buf, qkv.buf, out.buf, rec["mask"]])
        if qk is None:
            return self.wrote(dqkv, bounded=False)
        dqk = self.wrote(dqt, bounded=False)
        cos, sin = rec["rope"] if rec["rope"] is not None else (None, None)
        args = (dqkv.ptr + 4 * offs[0], dqkv.ptr + 4 * offs[1], dqk.ptr, dqk.ptr + 4 * Cq, qkv.ptr + 4 * offs[0],
                qkv.ptr + 4 * offs[1], B, L, heads,
                dim, L * dqk.cs, dqk.cs, dim, L * qkv.cs, qkv.cs, hs, L * dqkv.cs, dqkv.cs, hs, int(rec["rms"]), rec["norm_dim"],
                rec["eps"], cos.data_ptr() if cos is not None else None, sin.data_ptr() if sin is not None else None)
        gains = rec.get("qk_weight")
        if gains is None:
            self.tape.add("az_qk_prep_bwd_f32", *args, keep=[cos, sin])
        else:
            self.tape.add("az_qk_prep_bwd_w_f32", *args, gains[0].data_ptr(), gains[1].data_ptr(), keep=[cos, sin, *gains])
        self.free(dqk)
        return self.wrote(dqkv, bounded=False)

    # -- input gradient of the ADM norm pass (csrc/backward_adm.hip; the forward is group_norm(saved=)) ------------------------------------------------------
    def group_norm_keep_bwd(self, g: Act, rec: dict, *, res0: Act | None = None, res1: Act | None = None) -> tuple[Act, Act | None]:
        r"""Cotangent ``g`` of the output of :meth:`group_norm` with ``saved=rec`` (on the pooled grid) -> the cotangents of ``x`` and ``x1``, plus
        ``res0`` / ``res1`` (a tensor consumed twice: its cotangents add): ``az_norm_affine_bwd_{stats,apply}_f32``."""
        x, x1, cs, groups = rec["x"], rec["x1"], rec["cs"], rec["groups"]
        B, HW = x.B, x.H * x.W
        assert g.cs == cs and g.B == B
        nchunks = int(min(256, max(1, HW // 32)))
        bpart = self.empty(B * nchunks * groups * 4)
        ST, fp = rec["ST"], rec["partials"]
        S, T = ST.data_ptr(), ST.data_ptr() + 4 * B * cs
        w, sc = rec["weight"], rec["scale"]
        wp = w.data_ptr() if w is not None else None
        sp = sc.data_ptr() + 4 * rec["scale_off"] if sc is not None else None
        x1p = x1.ptr if x1 is not None else None
        self.tape.add("az_norm_affine_bwd_stats_f32", bpart.data_ptr(), x.ptr, x1p, rec["c0s"], g.ptr, S, T, wp, sp, rec["bstride"],
                      fp.data_ptr(), rec["nchunks"], B, x.H, x.W, rec["C"], cs, groups, nchunks, rec["act"], rec["pool"], rec["eps"],
                      keep=[ST, fp, w, sc, x.buf, x1.buf if x1 is not None else None])
        dx0 = self.new_act(B, x.H, x.W, x.C)
        dx1 = self.new_act(B, x.H, x.W, x1.C) if x1 is not None else None
        self.tape.add("az_norm_affine_bwd_apply_f32", dx0.ptr, dx1.ptr if dx1 is not None else None,
                      res0.ptr if res0 is not None else None, res1.ptr if res1 is not None else None, x.ptr, x1p, rec["c0s"], g.ptr, S, T,
                      wp, sp, rec["bstride"], fp.data_ptr(), rec["nchunks"], bpart.data_ptr(), nchunks, B, x.H, x.W, rec["C"], cs, groups,
                      rec["act"], rec["pool"], rec["eps"])
        self.wrote(dx0, bounded=False)
        if dx1 is not None:
            self.wrote(dx1, bounded=False)
        return dx0, dx1

    def add(self, a: Act, b: Act) -> Act:
        r"""a + b (two cotangents of one tensor) as a tensor of its own."""
        assert (a.B, a.H, a.W, a.cs) == (b.B, b.H, b.W, b.cs)
        y = self.new_act(a.B, a.H, a.W, a.C)
        one = self.const(torch.ones(1))
        self.tape.add("az_axpby_f32", y.ptr, one.data_ptr(), a.ptr, one.data_ptr(), b.ptr, 1, a.B * a.H * a.W * a.cs, 0, keep=[one])
        return self.wrote(y, bounded=False)

    def avgpool(self, x: Act, pool: int, depth: int = 1) -> Act:
        r"""The pooling-only pass of the ADM plans (the elementwise pass with S = 1, T = 0; ``pool`` as in :meth:`group_norm`).
        ``depth``: ``x`` holds B volumes of ``depth`` planes each, pooled in-plane -- a sample is one (depth H) x W image."""
        B = x.B // depth
        ones, zeros = self.const(torch.ones(B * x.cs)), self.const(torch.zeros(B * x.cs))
        y = self.new_act(x.B, x.H // 2 if pool == 1 else x.H, x.W // 2, x.C)
        return self._affine_act(y, x, None, 0, ones.data_ptr(), zeros.data_ptr(), B, depth * x.H, x.W, x.cs, 0, pool, bounded=False)

    def avgpool_bwd(self, g: Act, pool: int, H: int, W: int, res: Act | None = None) -> Act:
        r"""Pullback of :meth:`avgpool` onto the (H, W) grid, plus ``res``."""
        y = self.new_act(g.B, H, W, g.C)
        self.tape.add("az_avgpool_bwd_f32", y.ptr, g.ptr, res.ptr if res is not None else None, g.B, H, W, g.cs, pool)
        return self.wrote(y, bounded=False)

    def finish(self) -> None:
        r"""Allocates the shared split-K workspace and patches it into the recorded convs."""
        if self._ws_need and (self.workspace is None or self.workspace.numel() < self._ws_need):
            self.workspace = torch.empty(self._ws_need, dtype=torch.float32, device=self.device)
        for a in self._ws_users:
            a.workspace = self.workspace.data_ptr()
        self._ws_users = []

    def linear_small(self, y, ldy, x, ldx, W, bias, M, N, K, in_act=0, out_act=0, y_off=0) -> None:
        self.tape.add(
            "az_linear_small_f32", y.data_ptr() + 4 * y_off, ldy, x.data_ptr(), ldx, W.data_ptr(),
            bias.data_ptr() if bias is not None else None, M, N, K, in_act, out_act, keep=[y, x, W, bias],
        )

    def materialize(self, x: Act) -> Act:
        r"""The apply pass of a lazy normalisation (``Act.affine``) as a tensor of its own."""
        ST, act = x.affine
        n = x.B * x.cs
        y = self.new_act(x.B, x.H, x.W, x.C, f32=not x.half)
        return self._affine_act(y, x, None, 0, ST.data_ptr(), ST.data_ptr() + 4 * n, x.B, x.H, x.W, x.cs, act, 0, bounded=True)

    def _affine_act(self, y: Act, x: Act, x1p, c0s: int, S: int, T: int, B: int, H: int, W: int, cs: int, act: int, pool: int, *,
                    bounded: bool) -> Act:
        r"""y = act(x * S + T) (optionally pooled) on fp32 tensors or on tensors in the module's 2-byte type (x, x1, y alike)."""
        if x.half:
            assert y.half
            self.tape.add("az_affine_act_h16", y.ptr, x.ptr, x1p, c0s, S, T, B, H, W, cs, act, pool, 2 if x.buf.dtype == torch.float16 else 1)
        else:
            self.tape.add("az_affine_act_f32", y.ptr, x.ptr, x1p, c0s, S, T, B, H, W, cs, act, pool)
        return self.wrote(y, bounded=bounded)

    def group_norm(
        self, x: Act, groups: int, *, weight=None, bias=None, scale=None, shift=None, scale_off=0, shift_off=0,
        bstride=0, act=0, pool=0, eps=1e-5, x1: Act | None = None, lazy: bool = False, saved: dict | None = None,
    ) -> Act:
        r"""y = act((GN(x)*w + b) * (1 + scale) + shift), optionally 2x2 average pooled.  With ``x1`` the
        input is the channel concatenation [x | x1], read in place (never materialised).  ``saved``: a dict that receives what
        :meth:`group_norm_bwd` and :meth:`group_norm_keep_bwd` read (fp32 plans): the statistics pass always runs then, and its
        records, the ``S | T`` tables, ``x`` and ``x1`` must stay alive for the pullback.  No pre-activation is kept: the pullbacks
        recompute ``act'`` from x."""
        B, HW = x.B, x.H * x.W
        x1p, c0s, x0 = None, 0, x
        srcs = [x] + ([x1] if x1 is not None else [])
        src_quads = [self.fact(s, s.gn_quads) for s in srcs]
        src_channels = [s.C for s in srcs]
        if x1 is not None:
            assert x.C == x.cs and x1.C == x1.cs and (x1.H, x1.W) == (x.H, x.W) and x1.half == x.half
            x1p, c0s = x1.ptr, x.cs
            x = x.view(C_=x.C + x1.C, cs=x.cs + x1.cs)
        ST = self.empty(2 * B * x.cs)  # [scale | shift]: one buffer (AzConvArgs.in_affine reads both through one descriptor)
        S, T = ST[: B * x.cs], ST[B * x.cs :]
        f = AzNormFinalizeArgs()
        Cg = x.C // groups
        fused = saved is None and Cg % 4 == 0 and x.C == x.cs and all(q is not None for q in src_quads) and all((c // 4) % (Cg // 4) == 0 for c in src_channels)
        if fused:  # every source was produced by a convolution that left its moments of what it holds now: no statistics pass
            nchunks = src_quads[0][1]
            f.partials = src_quads[0][0].data_ptr()
            if len(src_quads) > 1:
                f.partials1, f.nchunks1 = src_quads[1][0].data_ptr(), src_quads[1][1]
            f.quads_per_group, f.quads0 = Cg // 4, src_channels[0] // 4
        else:
            nchunks = int(min(512, max(1, (HW * x.cs * 4) // 65536)))  # ~64 KB of x per workgroup
            partials = self.empty(B * nchunks * groups * 4)
            if x.half:
                self.tape.add("az_groupnorm_stats_h16", partials.data_ptr(), x.ptr, x1p, c0s, B, HW, x.C, x.cs, groups, nchunks,
                              2 if x.buf.dtype == torch.float16 else 1)
            else:
                self.tape.add("az_groupnorm_stats_f32", partials.data_ptr(), x.ptr, x1p, c0s, B, HW, x.C, x.cs, groups, nchunks)
            f.partials = partials.data_ptr()
            if saved is not None:
                assert not x.half and self.half is None
                saved.update(x=x0, x1=x1, c0s=c0s, C=x.C, cs=x.cs, ST=ST, partials=partials, nchunks=nchunks, groups=groups, eps=eps,
                             weight=weight, scale=scale, scale_off=scale_off, bstride=bstride, act=act, pool=pool)
        f.S, f.T = S.data_ptr(), T.data_ptr()
        f.weight = weight.data_ptr() if weight is not None else None
        f.bias = bias.data_ptr() if bias is not None else None
        f.scale = scale.data_ptr() + 4 * scale_off if scale is not None else None
        f.shift = shift.data_ptr() + 4 * shift_off if shift is not None else None
        f.scale_bstride = bstride
        f.B, f.C, f.cs, f.groups, f.nchunks, f.eps = B, x.C, x.cs, groups, nchunks, eps
        # (the descriptor holds raw addresses: the tensors behind them must live as long as the tape)
        self.tape.add("az_groupnorm_finalize_f32", C.byref(f), keep=[f, weight, bias, scale, shift])
        if (lazy and AFFINE_FUSED and x1 is None and not pool and act == 0 and x.C == x.cs and x.cs % 8 == 0
                and self.half is None):
            # no apply pass: the consumer (Builder.conv) reads x and applies scale / shift itself
            y = x.view(bounded=True)  # (the values the consumer sees: act(buf * scale + shift))
            y.affine = (ST, act)
            return y
        if pool:  # 1: 2x2, 2: along the width only (a 1-D signal held as a one-row image)
            y = self.new_act(B, x.H // 2 if pool == 1 else x.H, x.W // 2, x.C, f32=not x.half)
        else:
            y = self.new_act(B, x.H, x.W, x.C, f32=not x.half)
        assert y.cs == x.cs, "the apply pass writes the source's channel stride: the source must be on this plan's stride"
        return self._affine_act(y, x, x1p, c0s, S.data_ptr(), T.data_ptr(), B, x.H, x.W, x.cs, act, pool, bounded=True)

    def row_norm(self, x: Act, kind: int, *, weight=None, scale=None, shift=None, scale_off=0, shift_off=0, bstride=0,
                 eps=1e-5):
        y = self.new_act(x.B, x.H, x.W, x.C, f32=not x.half)
        assert y.cs == x.cs, "the row norm writes the source's channel stride: the source must be on this plan's stride"
        rows = x.B * x.H * x.W
        args = (y.ptr, x.ptr, weight.data_ptr() if weight is not None else None,
                scale.data_ptr() + 4 * scale_off if scale is not None else None,
                shift.data_ptr() + 4 * shift_off if shift is not None else None,
                bstride, rows, x.H * x.W, x.C, x.cs, kind, eps)
        if x.half:  # rows in the module's 2-byte type (fp32 statistics / modulation)
            if x.C % 8 or x.C != x.cs or x.C > 4096 or bstride % 4:  # (az_rownorm_mod_h16 would answer AZ_E_UNSUPPORTED at run time)
                raise ValueError(f"row_norm on 2-byte rows of width {x.C} (stride {x.cs}, modulation stride {bstride}): "
                                 "az_rownorm_mod_h16 takes widths that are multiples of 8, unpadded, at most 4096")
            self.tape.add("az_rownorm_mod_h16", *args, 2 if x.buf.dtype == torch.float16 else 1, keep=[weight, scale, shift])
        else:
            self.tape.add("az_rownorm_mod_f32", *args, keep=[weight, scale, shift])
        return self.wrote(y, bounded=True)

    def attention(self, qkv: Act, heads: int, order: str, qk_rmsnorm: bool, scale: float, eps: float = 1e-5,
                  rope: tuple | None = None, qk_weight: tuple | None = None, mask: torch.Tensor | None = None,
                  norm_dim: int = 0) -> Act:
        r"""softmax(q k^T * scale) v over a fused-QKV token tensor (B, L, 1, 3*heads*dim).

        order: "nHC" = azula '(n H C)' (attention.py:90), "H3C" = ADM legacy (unet.py:338),
        "3HC" = ADM new order (unet.py:371).  Output (B, L, 1, heads*dim) laid out '(H C)'.
        ``norm_dim``: the real head size of zero-padded heads (see ATTN_HEAD_DIMS)."""
        from ._lib import AzAttnArgs

        Cq = qkv.C // 3
        dim = Cq // heads
        assert qkv.cs == qkv.C and dim * heads == Cq
        L = qkv.H * qkv.W
        out = self.new_act(qkv.B, qkv.H, qkv.W, Cq, f32=not qkv.half)
        a = AzAttnArgs()
        a.io_dtype = int(qkv.half)  # (q, k, v, out in the module's 2-byte type: the bf16 / f16 entries only)
        es = 2 if qkv.half else 4
        base = qkv.ptr
        offs, hs = qkv_layout(order, Cq, dim)
        a.q, a.k, a.v, a.out = base + es * offs[0], base + es * offs[1], base + es * offs[2], out.ptr
        a.batch, a.heads, a.tokens, a.head_dim = qkv.B, heads, L, dim
        _token_strides(a, L, q=(qkv, hs), k=(qkv, hs), v=(qkv, hs), o=(out, dim))
        a.scale, a.qk_rmsnorm, a.eps, a.norm_dim = scale, int(qk_rmsnorm), eps, norm_dim
        # q / k RMS-normalised here or by the projection's epilogue (qk_rmsnorm is the layer's flag either way), with gains in range
        qk_normed = qk_in_h2_domain(qk_rmsnorm, dim, norm_dim, scale, qk_weight)
        if qkv.qk_prepared:  # the projection's epilogue has normalised / gained / rotated q and k already (Builder.conv(qk_prep=...))
            assert order in ("nHC", "3HC")
            a.qk_rmsnorm, rope, qk_weight = 0, None, None
        if rope is not None:  # (cos, sin) tables of shape (L, heads * dim / 2)
            a.rope_cos, a.rope_sin = rope[0].data_ptr(), rope[1].data_ptr()
            self.tape.keep.extend(rope)
        if qk_weight is not None:  # learned (dim,) gains of the q / k RMS norms
            a.q_weight, a.k_weight = qk_weight[0].data_ptr(), qk_weight[1].data_ptr()
            self.tape.keep.extend(qk_weight)
        if mask is not None:
            m8, a.mask_bstride, a.mask_hstride = self._attn_mask(mask, qkv.B, heads, L)
            a.mask = m8.data_ptr()
        a._flops = 4 * qkv.B * heads * L * L * dim
        self.tape.add(choose_attention(dim, qk_normed, self.half), C.byref(a), keep=[a])
        return self.wrote(out, bounded=False)  # (a convex combination of the values: as large as the weights make them)


# ------------------------------------------------------------------------------- AdaZero modulation helpers
def ada_zero_triple(bld: "Builder", ada_zero, channels: int, D: int, mod_rows: int, mod_jobs: list):
    r"""(abc buffer, batch stride) of one block's modulation triple (a, b, c), each padded to ``pad4(channels)``.
    ``ada_zero`` is the block's ``Linear(D, D) -> SiLU -> Linear(D, 3C)`` (then the MLP is queued on ``mod_jobs`` and
    emitted by :func:`mod_front_tape` for all blocks at once) or its raw ``(3, C, ...)`` parameter
    (reference ``azula/nn/unet.py:63-75``, ``azula/nn/dit.py:57-68``)."""
    cs, device = pad4(channels), bld.device
    if not isinstance(ada_zero, torch.nn.Parameter):
        abc = bld.empty(max(mod_rows, 1), 3 * cs)
        l0, l2 = ada_zero[0], ada_zero[2]
        w2 = torch.zeros(3 * cs, D, dtype=torch.float32, device=device)
        b2 = torch.zeros(3 * cs, dtype=torch.float32, device=device)
        for n in range(3):
            w2[n * cs : n * cs + channels] = l2.weight.detach()[n * channels : (n + 1) * channels]
            b2[n * cs : n * cs + channels] = l2.bias.detach()[n * channels : (n + 1) * channels]
        mod_jobs.append((l0, bld.const(w2), bld.const(b2), abc, 3 * cs))
        return abc, (3 * cs if mod_rows > 1 else 0)
    abc = torch.zeros(3 * cs, dtype=torch.float32, device=device)
    for n in range(3):
        abc[n * cs : n * cs + channels] = ada_zero.detach()[n].flatten()
    return bld.const(abc), 0


def linear_groups(jobs: list):
    r"""The ``AzLinearGroup`` array of ``(y, x, W, bias, ldy, ldx, N, K)`` jobs (addresses as integers, ``bias`` may be None) for
    ``az_linear_small_grouped_f32``.  The descriptors are read on the device, so the entry cannot validate them, and its kernel has
    only the 16-byte form (no scalar fallback): what ``az_linear_small_f32`` decides per launch is an error here, raised before
    anything is launched."""
    from ._lib import AzLinearGroup

    groups = (AzLinearGroup * len(jobs))()
    for i, (y, x, W, bias, ldy, ldx, N, K) in enumerate(jobs):
        if not (y and x and W):
            raise ValueError(f"grouped linear, group {i}: null y / x / W")
        if not (N > 0 and K > 0 and ldy >= N and ldx >= K):
            raise ValueError(f"grouped linear, group {i}: N {N}, K {K}, ldy {ldy}, ldx {ldx} are not a (M, K) x (N, K) product")
        if K % 4 or ldx % 4 or x % 16 or W % 16:
            raise ValueError(f"grouped linear, group {i}: the kernel reads x and W as 16-byte vectors and needs K % 4 == 0, ldx % 4 == 0 "
                             f"and 16-byte aligned x / W (K {K}, ldx {ldx}, x % 16 = {x % 16}, W % 16 = {W % 16})")
        g = groups[i]
        g.y, g.x, g.W, g.bias = y, x, W, bias
        g.ldy, g.ldx, g.N, g.K = ldy, ldx, N, K
    return groups


def mod_front_tape(bld: "Builder", mod_jobs: list, mod_buf: torch.Tensor, mod_rows: int, D: int) -> Tape:
    r"""h_i = silu(W0_i mod + b0_i) for ALL queued blocks as one GEMV, abc_i = W2_i h_i + b2_i as one grouped GEMV."""
    nj, rows = len(mod_jobs), max(mod_rows, 1)
    w0 = bld.const(torch.cat([j[0].weight.detach() for j in mod_jobs]))
    b0 = bld.const(torch.cat([j[0].bias.detach() for j in mod_jobs]))
    h_all = bld.empty(rows, nj * D)
    groups = linear_groups([(abc.data_ptr(), h_all.data_ptr() + 4 * i * D, w2.data_ptr(), b2.data_ptr(), n_out, nj * D, n_out, D)
                            for i, (_, w2, b2, abc, n_out) in enumerate(mod_jobs)])
    gdev = torch.frombuffer(bytearray(bytes(groups)), dtype=torch.uint8).to(bld.device)
    pre = Tape()
    pre.add("az_linear_small_f32", h_all.data_ptr(), nj * D, mod_buf.data_ptr(), D, w0.data_ptr(), b0.data_ptr(), rows, nj * D, D, 0, 1)
    pre.add("az_linear_small_grouped_f32", gdev.data_ptr(), nj, max(j[4] for j in mod_jobs), rows, 0, 0, keep=[gdev, w0, b0, h_all])
    return pre


def transition_args(**kw) -> AzTransitionArgs:
    a = AzTransitionArgs()
    for k, v in kw.items():
        setattr(a, k, v)
    return a



# ------------------------------------------------------------------------------- token-path helpers
# Head sizes.  The reference accepts any channels // attention_heads (azula/nn/attention.py:35-51; guided-diffusion any
# num_head_channels); the gfx950 attention kernels are instantiated for 16 / 32 / 64 / 80 / 128 (the fp32 kernel also for 8).  Any
# other size d <= 128 runs ZERO-PADDED to the next instantiated size d': the q | k | v projection is packed with d' - d zero rows
# (and zero bias) per head, so the padded channels of q, k and v are exact zeros -- they change neither q.k nor p.v --, the output
# projection with d' - d zero input columns per head; the scale stays 1 / sqrt(d), the q / k RMS norm averages over d
# (AzAttnArgs.norm_dim), padded RoPE pairs do not turn (theta = 0) and padded gains are 1.  (G24: 24, 48, 96.)
ATTN_HEAD_DIMS = (16, 32, 64, 80, 128)


# The attention backward kernels (csrc/attention_bwd.hip) are instantiated for these four: a gradient plan pads to the next of THEM
# (80 -> 128), through the same zero-padded packing -- the padded gradient rows meet zero weight columns in the data-gradient GEMM.
ATTN_GRAD_HEAD_DIMS = (16, 32, 64, 128)


def attn_grad_padded_dim(d: int) -> int:
    for v in ATTN_GRAD_HEAD_DIMS:
        if d <= v:
            return v
    raise NotImplementedError(f"attention head size {d}: the gfx950 attention backward kernels go up to 128 channels per head")


class LinearView:
    r"""A linear layer's (possibly head-padded) weight as the (cout, cin, 1, 1) ``.weight`` :meth:`Builder.conv_dgrad` takes."""

    def __init__(self, weight: torch.Tensor) -> None:
        self.weight = weight.detach().reshape(weight.shape[0], -1)[:, :, None, None]


def attn_padded_dim(d: int, half=None) -> int:
    if d == 8 and half is None:
        return 8
    for v in ATTN_HEAD_DIMS:
        if d <= v:
            return v
    raise NotImplementedError(f"attention head size {d}: the gfx950 attention kernels go up to 128 channels per head")


def pad_qkv_heads(w: torch.Tensor, b: torch.Tensor | None, heads: int, d: int, dp: int, order: str):
    r"""(3 heads d, Cin[, 1]) q | k | v projection weights (and bias) -> (3 heads dp, Cin): dp - d zero rows behind every head's d.
    ``order`` as in Builder.attention: "nHC" / "3HC" = rows (n, head, c), "H3C" = rows (head, n, c)."""
    w = w.detach().float().reshape(3 * heads * d, -1)
    lead = (3, heads) if order in ("nHC", "3HC") else (heads, 3)
    wp = w.new_zeros(*lead, dp, w.shape[1])
    wp[:, :, :d] = w.reshape(*lead, d, w.shape[1])
    bp = None
    if b is not None:
        bp = w.new_zeros(*lead, dp)
        bp[:, :, :d] = b.detach().float().reshape(*lead, d)
        bp = bp.reshape(-1)
    return wp.reshape(3 * heads * dp, w.shape[1]), bp


def pad_proj_heads(w: torch.Tensor, heads: int, d: int, dp: int) -> torch.Tensor:
    r"""(Cout, heads d[, 1]) output projection -> (Cout, heads dp): zero columns for the padded channels of every head."""
    w = w.detach().float().reshape(w.shape[0], heads, d)
    wp = w.new_zeros(w.shape[0], heads, dp)
    wp[:, :, :d] = w
    return wp.reshape(w.shape[0], heads * dp)


def pad_head_table(t: torch.Tensor, heads: int, n: int, n_pad: int, fill: float = 0.0) -> torch.Tensor:
    r"""(..., heads n) per-head table (RoPE angles with n = d / 2) -> (..., heads n_pad), padded with ``fill``."""
    lead = t.shape[:-1]
    tp = t.new_full((*lead, heads, n_pad), fill)
    tp[..., :n] = t.reshape(*lead, heads, n)
    return tp.reshape(*lead, heads * n_pad)
