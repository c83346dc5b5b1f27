r"""Hashable keys for what a captured sampling loop bakes in: the denoiser's state (``module_fingerprint``), a sampler's or a
schedule's scalar attributes (``_attr_key``, ``_schedule_key``), the structure of the keyword arguments (``_kwargs_signature``).
``Sampler._call_fused`` keys the loop on them, ``_FusedLoop._upload_table`` the coefficient table."""

from __future__ import annotations

import weakref

import torch


def module_fingerprint(module: torch.nn.Module) -> tuple:
    r"""Identity of a module's state as the compiled plans see it: (address, in-place version, dtype) of every
    parameter and buffer plus the train/eval flags.  Packed weight copies (direct, Winograd, half) are valid exactly
    as long as this tuple is unchanged."""
    tensors = tuple((t.data_ptr(), t._version, t.dtype) for t in (*module.parameters(), *module.buffers()))
    return tensors + tuple(m.training for m in module.modules())


def _schedule_key(sched) -> tuple:
    r"""Scalar attributes of a schedule object (alpha_min, sigma_min, gamma, ...) and, for ``nn.Module`` schedules,
    the fingerprint of their tensors."""
    return _attr_key(getattr(sched, "__dict__", {})) + (module_fingerprint(sched) if isinstance(sched, torch.nn.Module) else ())


def _value_key(v):
    r"""A hashable stand-in for one attribute value, or ``_SKIP``: numbers / strings / dtypes by value, small tensors by
    VALUE (eta, temperature, alpha_min held as 0-d or short tensors: the reference re-reads them on every call), larger
    tensors by (address, version), tuples / lists recursively.  Modules and other objects are not hyper-parameters."""
    if isinstance(v, (int, float, bool, str, type(None), torch.dtype)):
        return v
    if torch.is_tensor(v):
        if v.numel() <= 16:
            # `.tolist()` on a device tensor is a blocking sync: read the value only when the tensor's identity
            # (object, storage address, version counter) changes.  Writes through `.data` do not bump the version counter and
            # are NOT tracked -- neither here nor by the (address, version) key of larger tensors (documented in DESIGN.md).
            ident = (v.data_ptr(), v._version, tuple(v.shape), v.dtype, v.device)
            hit = _SMALL_VALUES.get(id(v))
            if hit is None or hit[0] != ident or hit[1]() is not v:
                if len(_SMALL_VALUES) > 256:
                    for k in [k for k, h in _SMALL_VALUES.items() if h[1]() is None]:
                        del _SMALL_VALUES[k]
                hit = (ident, weakref.ref(v), tuple(v.detach().reshape(-1).tolist()))
                _SMALL_VALUES[id(v)] = hit
            return ("t", tuple(v.shape), str(v.dtype), hit[2])
        return ("T", v.data_ptr(), v._version, tuple(v.shape), str(v.dtype))
    if isinstance(v, (tuple, list)):
        items = tuple(_value_key(x) for x in v)
        return _SKIP if any(x is _SKIP for x in items) else ("seq", items)
    return _SKIP


_SKIP = object()
_SMALL_VALUES: dict = {}  # id(tensor) -> ((address, version, shape, dtype, device), weakref, value tuple)


def _attr_key(attrs: dict) -> tuple:
    out = []
    for k, v in sorted(attrs.items()):
        if k.startswith("_fused") or isinstance(v, torch.nn.Module):
            continue
        kv = _value_key(v)
        if kv is not _SKIP:
            out.append((k, kv))
    return tuple(out)


def _kwargs_signature(kw) -> tuple:
    r"""Structure of the keyword arguments (names, nesting, which values are None) -- not their values: label and
    guidance VALUES are uploaded per call, their presence decides which programs exist."""
    if isinstance(kw, dict):
        return tuple((k, _kwargs_signature(v)) for k, v in sorted(kw.items()))
    if kw is None:
        return ("none",)
    if torch.is_tensor(kw):
        return ("tensor", tuple(kw.shape))
    return ("value",)
