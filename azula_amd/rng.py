r"""The sliced Philox draw of sharded sampling (``Sampler._draw_noise``): a rank's elements of the full-batch ``torch.randn``,
bit for bit, without drawing the rest (``az_randn_slice_f32``), and the one-time self-check that guards it."""

from __future__ import annotations

import warnings

import torch
from torch import Tensor

from . import _lib

_SLICE_VERIFIED: dict = {}  # (device index, torch version) -> bool


def _randn_slice_verified(dev: torch.device) -> bool:
    r"""One-time self-check per (device, torch version): :func:`_randn_slice` re-derives ATen's launch policy (grid rule, unroll 4,
    offset arithmetic) from the torch it was written against.  A torch whose policy differs would still hand out valid noise,
    but the 1-GPU == N-GPU bit-reproducibility of ``parallel.py`` would break silently.  So the first sharded draw on a device
    compares two slices -- a tensor under one grid's worth of elements and one that spans several grid iterations -- and the
    generator's offset afterwards against ``torch.randn`` of the full shape, under a saved / restored generator state; on any
    mismatch it warns once and every later sharded draw takes the draw-and-slice path."""
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    key = (idx, torch.__version__)
    ok = _SLICE_VERIFIED.get(key)
    if ok is None:
        gen = torch.cuda.default_generators[idx]
        saved = gen.get_state()
        ok = True
        try:
            for total, world, rank in ((3 * 1000, 3, 1), (3 * (1 << 20) + 3 * 4096, 3, 2), (2 * 65536, 2, 0)):
                gen.manual_seed(1234567)
                gen.set_offset(8)
                full = torch.randn(total, device=dev)
                off_full = gen.get_offset()
                gen.manual_seed(1234567)
                gen.set_offset(8)
                n = total // world
                mine = _randn_slice(torch.empty(n, device=dev), rank, world)
                ok = ok and gen.get_offset() == off_full and bool(torch.equal(mine, full[rank * n : (rank + 1) * n]))
        except Exception:  # noqa: BLE001  (a generator API that moved: same verdict)
            ok = False
        finally:
            gen.set_state(saved)
        _SLICE_VERIFIED[key] = ok
        if not ok:
            warnings.warn(
                f"azula_amd: the sliced Philox draw does not reproduce torch.randn on torch {torch.__version__} (device {idx}); "
                "sharded sampling falls back to drawing the full batch on every rank and slicing (same result, more work)",
                RuntimeWarning, stacklevel=3)
    return ok


def _randn_slice(like: Tensor, rank: int, world: int, out: Tensor | None = None) -> Tensor:
    r"""Elements [rank n, (rank + 1) n) of ``torch.randn(world * n)`` on ``like``'s device, without drawing the rest: ATen's
    launch policy for the FULL tensor (``ATen/native/cuda/DistributionTemplates.h: calc_execution_policy``) fixes which Philox
    subsequence / call / component produces every element; the kernel evaluates exactly those."""
    dev = like.device
    gen = torch.cuda.default_generators[dev.index if dev.index is not None else torch.cuda.current_device()]
    n = like.numel()
    total = world * n
    props = torch.cuda.get_device_properties(dev)
    grid = min(props.multi_processor_count * (props.max_threads_per_multi_processor // 256), (total + 255) // 256)
    threads = 256 * grid
    seed, offset = gen.initial_seed(), gen.get_offset()
    dst = out if (out is not None and out.is_contiguous()) else torch.empty_like(like, memory_format=torch.contiguous_format)
    with torch.cuda.device(dev):
        _lib.call("az_randn_slice_f32", dst.data_ptr(), seed, offset, threads, rank * n, n, _lib.stream_ptr())
    gen.set_offset(offset + ((total - 1) // (threads * 4) + 1) * 4)  # (the full draw's counter_offset)
    if out is not None and dst is not out:
        out.copy_(dst)
        return out
    return dst
