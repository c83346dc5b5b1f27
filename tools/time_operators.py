r"""Time ``az_op_blur_f32`` (through ``BlurOperator``), ``az_op_psf_f32`` (through ``PSFOperator``) or ``az_op_fft2_f32`` (through
``FourierOperator``) against torch-op forms of the same map on the same device tensor.

    python tools/time_operators.py [taps] [B] [C] [H] [W]          # blur
    python tools/time_operators.py psf [size] [B] [C] [H] [W]      # general PSF
    python tools/time_operators.py fft [B] [C] [H] [W]             # 2-D Fourier transform
    python tools/time_operators.py radon [B] [C] [H] [W] [angles]  # parallel-beam Radon transform
    python tools/time_operators.py sense [B] [K] [H] [W]           # multi-coil (SENSE) MRI
    python tools/time_operators.py nonlinear [B] [C] [H] [W]       # magnitude, clip, quantize entries and their linearisations

Blur, default: the 61-tap Gaussian of DPS's deblurring setup on 4 x 3 x 256 x 256.  HIP events around back-to-back calls after a
warm-up, the forms alternating over ``ROUNDS`` rounds; prints the median time per call of

* the operator (one launch of the kernel),
* the package's torch path (the separable shift-and-add a non-fp32 tensor takes: ``2 * taps`` slices), and
* the oracle of the tests (``tests/operator_oracle.py``: the two-dimensional shift-and-add, ``taps^2`` slices),

the kernel's share of the HBM roofline (one fp32 read and one write per element over the measured copy bandwidth of the MI355X,
6.29 TB/s) and one JSON line.

PSF, default: ``motion_psf(size / 2, 30, size)`` with size 61 on 4 x 3 x 256 x 256, once shared by all planes and once with one
PSF per sample (angles 30 + 15 b).  The same method; the forms are

* the operator (one launch),
* ``F.conv2d(groups = planes)`` on the same device tensor -- what a user writes today, and
* the package's torch path (``size^2`` slices; fewer repetitions: it takes tens of milliseconds),

and the yardstick is the vector-fp32 FMA peak of the MI355X, 157.3 TFLOP/s: ``2 size^2 B C H W`` FLOP per call.

FFT, default: ``FourierOperator()`` apply (real -> split complex) and adjoint (split complex -> real) on 4 x 3 x 256 x 256; run it
on 16 4 64 64 for the whole-plane form.  The same method; the forms are the operator, the C entry alone on buffers made once (the
difference is what the operator adds: the autograd Function and the allocations) and the ``torch.fft`` lambda a user writes today
(the vendor library, with the rearrangement to the split layout).  The yardstick is the bytes model of ``csrc/fft.hip`` at the
same 6.29 TB/s: 12 bytes per element where a plane runs whole in LDS (at most 8192 points), else 28.

Radon, default: ``RadonOperator(radon_angles(180), (256, 256))`` apply, adjoint and ``fbp`` on 4 x 3 x 256 x 256 (``radon B C H W
angles``).  The same method; the comparison is what a user can write today on the same device tensor, ``torch.sparse.mm`` with
the same matrix (the operator's own path for fp64 and half tensors), and the yardstick the vector-fp32 peak over the operation
counts ``A D max(H, W) window`` (apply, window 5 at spacing 1) and ``2 A H W`` (adjoint) fused multiply-adds per plane.

SENSE, default: ``MultiCoilMRIOperator(cartesian_mask(H, W, 4), birdcage_maps(K, H, W))`` apply and adjoint on a complex image,
4 x 8 x 256 x 256 (``sense B K H W``; run it on 16 4 64 64 for the whole-plane FFT form).  The same method; the forms are the
operator, the two coil entries alone on buffers made once, and the torch lambda a user writes today (complex multiply,
``torch.fft``, mask, with the rearrangement to the split layout).  The yardsticks are the byte models of ``csrc/coil.hip`` at the
same 6.29 TB/s: ``8 + 16 K`` bytes per pixel for either entry, and for the operator the sum over its three launches (the entry,
the FFT's 24 or 56 bytes per coil pixel complex to complex, the mask's 16 bytes per coil pixel).

Nonlinear, default 4 x 3 x 512 x 512 elements (``nonlinear B C H W``; run it on 16 3 1024 1024 for tensors that no longer fit the
256 MB Infinity Cache): the six elementwise entries of ``csrc/nonlinear.hip`` alone on buffers made once, each against its byte
model (12 / 20 / 20 / 8 / 12 / 8 bytes per element) as GB/s, and ``PhaseRetrievalOperator`` / ``ClipOperator`` as a user calls
them against the torch lambda a user writes today.

The figures in DESIGN.md sections 9c, 9d, 9e, 9f and 9g come from this script.
"""

from __future__ import annotations

import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import operator_oracle as oo  # noqa: E402
from azula_amd import _lib  # noqa: E402
from azula_amd.guidance import BlurOperator, FourierOperator, PSFOperator, gaussian_taps, motion_psf  # noqa: E402
from azula_amd.guidance import MultiCoilMRIOperator, birdcage_maps, cartesian_mask  # noqa: E402
from azula_amd.guidance import RadonOperator, radon_angles  # noqa: E402
from azula_amd.guidance import ClipOperator, PhaseRetrievalOperator  # noqa: E402

HBM = 6.29e12
FP32_PEAK = 157.3e12  # vector fp32, FLOP/s
ROUNDS, WARMUP = 7, 3


def timed(fn, reps: int) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / reps


def measure(forms: dict) -> dict:
    r"""name -> the per-call times of ``ROUNDS`` rounds, the forms alternating, after ``WARMUP`` calls of each."""
    for fn, _ in forms.values():
        for _ in range(WARMUP):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(ROUNDS):
        for k, (fn, reps) in forms.items():
            times[k].append(timed(fn, reps))
    return times


def report(forms: dict, times: dict, err: dict) -> dict:
    med = {k: statistics.median(v) for k, v in times.items()}
    for k in forms:
        print(f"{k}: {med[k] * 1e6:.1f} us per call (min {min(times[k]) * 1e6:.1f}, max {max(times[k]) * 1e6:.1f}), "
              f"max|d| to fp64 {err[k]:.2e}")
    return med


def blur(args: list[str]) -> None:
    n, B, Cc, H, W = (int(v) for v in (args + ["61", "4", "3", "256", "256"][len(args):]))
    x = torch.randn(B, Cc, H, W, device="cuda")
    taps = gaussian_taps(n / 6.0, n)
    A = BlurOperator(taps)
    td = taps.cuda()
    forms = {"kernel": (lambda: A(x), 200), "torch_path": (lambda: A._torch(x, "apply"), 5),
             "oracle": (lambda: oo.blur(x, td, td, False), 2)}
    ref = oo.blur(x.double(), td.double(), td.double(), False)
    err = {k: float((fn().double() - ref).abs().max()) for k, (fn, _) in forms.items()}
    times = measure(forms)
    med = report(forms, times, err)
    floor = 2 * x.numel() * 4 / HBM
    print(f"HBM floor {floor * 1e6:.2f} us -> the kernel runs at {floor / med['kernel']:.1%} of the HBM roofline")
    print(json.dumps({"taps": n, "shape": [B, Cc, H, W], **{f"{k}_us": med[k] * 1e6 for k in forms}, "hbm_floor_us": floor * 1e6,
                      "hbm_fraction": floor / med["kernel"]}))


def psf(args: list[str]) -> None:
    n, B, Cc, H, W = (int(v) for v in (args + ["61", "4", "3", "256", "256"][len(args):]))
    x = torch.randn(B, Cc, H, W, device="cuda")
    flop = 2.0 * n * n * x.numel()
    for what in ("shared", "per_sample"):
        k = motion_psf(n / 2, 30.0, n) if what == "shared" else \
            torch.stack([motion_psf(n / 2, 30.0 + 15.0 * b, n) for b in range(B)])[:, None]
        A = PSFOperator(k)
        # conv2d correlates, as the operator does: one group per plane, the plane's PSF as its only filter
        weight = k.expand(B, Cc, n, n).reshape(B * Cc, 1, n, n).contiguous().cuda()
        conv = lambda: F.conv2d(x.reshape(1, B * Cc, H, W), weight, padding=n // 2, groups=B * Cc).reshape(B, Cc, H, W)  # noqa: E731, B023
        forms = {"kernel": (lambda: A(x), 20), "conv2d_groups": (conv, 5), "torch_path": (lambda: A._torch(x, "apply"), 1)}  # noqa: B023
        ref = A._torch(x.double(), "apply")
        try:
            conv()
        except RuntimeError as e:  # (the convolution library may have no kernel for a filter this large)
            print(f"conv2d_groups is not timed: {str(e).splitlines()[0]}")
            del forms["conv2d_groups"]
        err = {k_: float((fn().double() - ref).abs().max()) for k_, (fn, _) in forms.items()}
        times = measure(forms)
        print(f"-- {n} x {n} motion PSF, {what}, on {B} x {Cc} x {H} x {W}")
        med = report(forms, times, err)
        peak = flop / FP32_PEAK
        print(f"{flop / 1e9:.2f} GFLOP: {peak * 1e6:.1f} us at the vector fp32 peak -> the kernel runs at "
              f"{peak / med['kernel']:.1%} of it ({flop / med['kernel'] / 1e12:.1f} TFLOP/s)")
        print(json.dumps({"psf": n, "form": what, "shape": [B, Cc, H, W], **{f"{k_}_us": med[k_] * 1e6 for k_ in forms},
                          **{f"{k_}_min_us": min(times[k_]) * 1e6 for k_ in forms},
                          **{f"{k_}_max_us": max(times[k_]) * 1e6 for k_ in forms}, "fp32_peak_us": peak * 1e6,
                          "fp32_peak_fraction": peak / med["kernel"]}))


def fft(args: list[str]) -> None:
    B, Cc, H, W = (int(v) for v in (args + ["4", "3", "256", "256"][len(args):]))
    x, z = torch.randn(B, Cc, H, W, device="cuda"), torch.randn(B, 2 * Cc, H, W, device="cuda")
    A = FourierOperator()

    def lam(v):
        f = torch.fft.fft2(v, norm="ortho")
        return torch.cat([f.real, f.imag], dim=1)

    def lam_t(v):
        return torch.fft.ifft2(torch.complex(v[:, :Cc], v[:, Cc:]), norm="ortho").real

    # the C entry alone on buffers made once: what the operator adds (the autograd Function, the allocation of the output and of
    # `work`) is the difference
    n, y, xo = Cc * H * W, torch.empty_like(z), torch.empty_like(x)
    floats = C.c_int64(0)
    _lib.call("az_op_fft2_work", B, Cc, H, W, C.byref(floats))
    work = torch.empty(max(floats.value, 4), device="cuda")
    scale, stream = 1.0 / (H * W) ** 0.5, _lib.stream_ptr()
    entry = lambda: _lib.call("az_op_fft2_f32", y.data_ptr(), y.data_ptr() + 4 * n, 2 * n, x.data_ptr(), None, n, None, B, Cc, H,  # noqa: E731
                              W, 0, scale, stream)
    entry_t = lambda: _lib.call("az_op_fft2_f32", xo.data_ptr(), None, n, z.data_ptr(), z.data_ptr() + 4 * n, 2 * n,  # noqa: E731
                                work.data_ptr(), B, Cc, H, W, 1, scale, stream)
    forms = {"apply": (lambda: A(x), 200), "adjoint": (lambda: A.adjoint(z), 200), "entry_apply": (lambda: (entry(), y)[1], 200),
             "entry_adjoint": (lambda: (entry_t(), xo)[1], 200), "torch_fft_apply": (lambda: lam(x), 200),
             "torch_fft_adjoint": (lambda: lam_t(z), 200)}
    ref, ref_t = lam(x.double()), lam_t(z.double())
    err = {k: float((fn().double() - (ref_t if "adjoint" in k else ref)).abs().max()) for k, (fn, _) in forms.items()}
    times = measure(forms)
    med = report(forms, times, err)
    per_element = 12 if H * W <= 8192 else 28
    floor = per_element * x.numel() / HBM
    print(f"{per_element} B per element: {floor * 1e6:.2f} us at {HBM / 1e12:.2f} TB/s -> apply runs at {floor / med['apply']:.1%} "
          f"of the model, adjoint at {floor / med['adjoint']:.1%}; the entry alone at {floor / med['entry_apply']:.1%} and "
          f"{floor / med['entry_adjoint']:.1%}")
    print(json.dumps({"fft": [B, Cc, H, W], **{f"{k}_us": med[k] * 1e6 for k in forms},
                      **{f"{k}_min_us": min(times[k]) * 1e6 for k in forms}, "bytes_per_element": per_element,
                      "model_us": floor * 1e6, "model_fraction_apply": floor / med["apply"],
                      "model_fraction_adjoint": floor / med["adjoint"]}))


def radon(args: list[str]) -> None:
    B, Cc, H, W, n = (int(v) for v in (args + ["4", "3", "256", "256", "180"][len(args):]))
    A = RadonOperator(radon_angles(n), (H, W))
    D = A.det_count
    x, v = torch.randn(B, Cc, H, W, device="cuda"), torch.randn(B, Cc, n, D, device="cuda")
    # what a user can write today on the same device tensor: torch.sparse.mm with the same matrix (the operator's torch path,
    # called as `_product`: inside the Function an fp32 device tensor is the kernels')
    forms = {"apply": (lambda: A(x), 20), "adjoint": (lambda: A.adjoint(v), 20), "fbp": (lambda: A.fbp(v), 20),
             "sparse_mm_apply": (lambda: A._product(x, "apply"), 5), "sparse_mm_adjoint": (lambda: A._product(v, "adjoint"), 5)}
    ref, ref_t, ref_f = (A._torch(t.double(), m) for t, m in ((x, "apply"), (v, "adjoint"), (v, "fbp")))
    refs = {"apply": ref, "sparse_mm_apply": ref, "adjoint": ref_t, "sparse_mm_adjoint": ref_t, "fbp": ref_f}
    err = {k: float((fn().double() - refs[k]).abs().max()) for k, (fn, _) in forms.items()}
    times = measure(forms)
    med = report(forms, times, err)
    planes, window = B * Cc, 5  # (the candidates per line at spacing 1)
    flop = {"apply": 2.0 * planes * n * D * max(H, W) * window, "adjoint": 2.0 * planes * 2 * n * H * W}
    for k in ("apply", "adjoint"):
        print(f"{k}: {flop[k] / 2e6:.1f} M fused multiply-adds: {flop[k] / FP32_PEAK * 1e6:.1f} us at the vector fp32 peak -> "
              f"{flop[k] / FP32_PEAK / med[k]:.1%} of it; {med['sparse_mm_' + k] / med[k]:.1f} x faster than torch.sparse.mm")
    print(json.dumps({"radon": [B, Cc, H, W, n, D], **{f"{k}_us": med[k] * 1e6 for k in forms},
                      **{f"{k}_min_us": min(times[k]) * 1e6 for k in forms},
                      **{f"fp32_peak_fraction_{k}": flop[k] / FP32_PEAK / med[k] for k in flop}}))


def sense(args: list[str]) -> None:
    B, K, H, W = (int(v) for v in (args + ["4", "8", "256", "256"][len(args):]))
    hw, n = H * W, K * H * W
    maps, m = birdcage_maps(K, H, W), cartesian_mask(H, W, 4)
    A = MultiCoilMRIOperator(m, maps)
    x, z = torch.randn(B, 2, H, W, device="cuda"), torch.randn(B, 2 * K, H, W, device="cuda")
    sd, md = maps.to(torch.complex64).cuda(), m.cuda()

    def lam(v):  # what a user writes today
        f = torch.fft.fft2(sd * torch.complex(v[:, 0], v[:, 1])[:, None], norm="ortho")
        return torch.cat([f.real, f.imag], dim=1) * md

    def lam_t(v):
        v = v * md
        img = (sd.conj() * torch.fft.ifft2(torch.complex(v[:, :K], v[:, K:]), norm="ortho")).sum(1)
        return torch.stack([img.real, img.imag], dim=1)

    # the two entries alone on buffers made once
    s_re, s_im = sd.real.contiguous(), sd.imag.contiguous()
    coil, img, stream = torch.empty_like(z), torch.empty_like(x), _lib.stream_ptr()
    entry = lambda: _lib.call("az_op_coil_expand_f32", coil.data_ptr(), coil.data_ptr() + 4 * n, 2 * n, x.data_ptr(),  # noqa: E731
                              x.data_ptr() + 4 * hw, 2 * hw, s_re.data_ptr(), s_im.data_ptr(), 0, B, K, hw, stream)
    entry_t = lambda: _lib.call("az_op_coil_combine_f32", img.data_ptr(), img.data_ptr() + 4 * hw, 2 * hw, z.data_ptr(),  # noqa: E731
                                z.data_ptr() + 4 * n, 2 * n, s_re.data_ptr(), s_im.data_ptr(), 0, B, K, hw, 0, stream)
    forms = {"apply": (lambda: A(x), 200), "adjoint": (lambda: A.adjoint(z), 200), "entry_expand": (lambda: (entry(), coil)[1], 200),
             "entry_combine": (lambda: (entry_t(), img)[1], 200), "torch_apply": (lambda: lam(x), 200),
             "torch_adjoint": (lambda: lam_t(z), 200)}
    s64 = maps.cuda()
    c64 = s64 * torch.complex(x[:, 0].double(), x[:, 1].double())[:, None]
    g64 = (s64.conj() * torch.complex(z[:, :K].double(), z[:, K:].double())).sum(1)
    f64 = torch.fft.fft2(c64, norm="ortho")
    zm = z.double() * md
    a64 = (s64.conj() * torch.fft.ifft2(torch.complex(zm[:, :K], zm[:, K:]), norm="ortho")).sum(1)
    refs = {"apply": torch.cat([f64.real, f64.imag], dim=1) * md, "adjoint": torch.stack([a64.real, a64.imag], dim=1),
            "entry_expand": torch.cat([c64.real, c64.imag], dim=1), "entry_combine": torch.stack([g64.real, g64.imag], dim=1)}
    refs["torch_apply"], refs["torch_adjoint"] = refs["apply"], refs["adjoint"]
    err = {k: float((fn().double() - refs[k]).abs().max()) for k, (fn, _) in forms.items()}
    times = measure(forms)
    med = report(forms, times, err)
    entry_floor = (8 + 16 * K) * B * hw / HBM
    op_floor = entry_floor + ((24 if hw <= 8192 else 56) + 16) * B * n / HBM
    print(f"{8 + 16 * K} B per pixel: {entry_floor * 1e6:.2f} us at {HBM / 1e12:.2f} TB/s -> expand runs at "
          f"{entry_floor / med['entry_expand']:.1%} of the model, combine at {entry_floor / med['entry_combine']:.1%}")
    print(f"operator (entry + FFT + mask): {op_floor * 1e6:.2f} us -> apply runs at {op_floor / med['apply']:.1%} of the model, adjoint "
          f"at {op_floor / med['adjoint']:.1%}; {med['torch_apply'] / med['apply']:.2f} x and {med['torch_adjoint'] / med['adjoint']:.2f} "
          "x the speed of the torch lambda")
    print(json.dumps({"sense": [B, K, H, W], **{f"{k}_us": med[k] * 1e6 for k in forms},
                      **{f"{k}_min_us": min(times[k]) * 1e6 for k in forms}, "entry_model_us": entry_floor * 1e6,
                      "operator_model_us": op_floor * 1e6, "model_fraction_expand": entry_floor / med["entry_expand"],
                      "model_fraction_combine": entry_floor / med["entry_combine"]}))


def nonlinear(args: list[str]) -> None:
    B, Cc, H, W = (int(v) for v in (args + ["4", "3", "512", "512"][len(args):]))
    n, stream = Cc * H * W, _lib.stream_ptr()
    z, t = torch.randn(B, 2 * Cc, H, W, device="cuda"), torch.randn(B, 2 * Cc, H, W, device="cuda")
    g, y, d = torch.randn(B, Cc, H, W, device="cuda"), torch.empty(B, Cc, H, W, device="cuda"), torch.empty_like(z)
    zp, tp, dp = ((v.data_ptr(), v.data_ptr() + 4 * n, 2 * n) for v in (z, t, d))  # (re, im, sample stride): the halves in place
    x = z[:, :Cc].contiguous()
    step = float(torch.tensor(2 / 255, dtype=torch.float32))
    entries = {  # name -> (call, bytes per element)
        "cmag": (lambda: _lib.call("az_op_cmag_f32", y.data_ptr(), n, *zp, B, n, 0, stream), 12),
        "cmag_squared": (lambda: _lib.call("az_op_cmag_f32", y.data_ptr(), n, *zp, B, n, 1, stream), 12),
        "cmag_vjp": (lambda: _lib.call("az_op_cmag_vjp_f32", *dp, g.data_ptr(), n, *zp, B, n, 0, stream), 20),
        "cmag_jvp": (lambda: _lib.call("az_op_cmag_jvp_f32", y.data_ptr(), n, *tp, *zp, B, n, 0, stream), 20),
        "clip": (lambda: _lib.call("az_op_clip_f32", y.data_ptr(), x.data_ptr(), B * n, 2.0, -1.0, 1.0, stream), 8),
        "clip_jac": (lambda: _lib.call("az_op_clip_jac_f32", y.data_ptr(), g.data_ptr(), x.data_ptr(), B * n, 2.0, -1.0, 1.0, stream), 12),
        "quantize": (lambda: _lib.call("az_op_quantize_f32", y.data_ptr(), x.data_ptr(), B * n, -1.0, 1.0, step, stream), 8),
    }
    times = measure({k: (fn, 50) for k, (fn, _) in entries.items()})
    out = {"nonlinear": [B, Cc, H, W]}
    for k, (_, nbytes) in entries.items():
        med = statistics.median(times[k])
        out[f"{k}_us"], out[f"{k}_GBps"] = med * 1e6, nbytes * B * n / med / 1e9
        print(f"{k}: {med * 1e6:.1f} us per call (min {min(times[k]) * 1e6:.1f}, max {max(times[k]) * 1e6:.1f}), {nbytes} B per element: "
              f"{nbytes * B * n / med / 1e9:.0f} GB/s, {nbytes * B * n / med / HBM:.1%} of {HBM / 1e12:.2f} TB/s")
    if H == W and H <= 512 and H & (H - 1) == 0:  # the operators as a user calls them, against the lambda a user writes today
        A, Hc = PhaseRetrievalOperator(H // 2), ClipOperator(gain=2.0)
        lam = lambda v: torch.fft.fft2(F.pad(v, (H // 2,) * 4), norm="ortho").abs()  # noqa: E731
        forms = {"phase_retrieval": (lambda: A(x), 50), "torch_phase_retrieval": (lambda: lam(x), 50), "hdr": (lambda: Hc(x), 50),
                 "torch_hdr": (lambda: torch.clamp(2.0 * x, -1.0, 1.0), 50)}
        ref = lam(x.double())
        err = {"phase_retrieval": float((A(x).double() - ref).abs().max()), "torch_phase_retrieval": float((lam(x).double() - ref).abs().max()),
               "hdr": float((Hc(x) - torch.clamp(2.0 * x, -1.0, 1.0)).abs().max()), "torch_hdr": 0.0}
        med = report(forms, measure(forms), err)
        out.update({f"{k}_us": v * 1e6 for k, v in med.items()})
    print(json.dumps(out))


def main() -> None:
    if not torch.cuda.is_available():
        raise SystemExit("time_operators.py measures on the GPU: no device visible")
    torch.manual_seed(0)
    if sys.argv[1:2] == ["radon"]:
        radon(sys.argv[2:7])
    elif sys.argv[1:2] == ["nonlinear"]:
        nonlinear(sys.argv[2:6])
    elif sys.argv[1:2] == ["sense"]:
        sense(sys.argv[2:6])
    elif sys.argv[1:2] == ["psf"]:
        psf(sys.argv[2:7])
    elif sys.argv[1:2] == ["fft"]:
        fft(sys.argv[2:6])
    else:
        blur(sys.argv[1:6])


if __name__ == "__main__":
    main()
