r"""The cases of ``tests/golden/g28_guidance_vjp.npz`` as calls of the restatement (``guidance_vjp_oracle``) -- shared by the
host test (fp32, bit for bit against the fixture) and the GPU test (fp64, against the device) -- TEST INFRASTRUCTURE."""

from __future__ import annotations

import torch

import guidance_vjp_oracle as go
from oracle import nets, sampling, synth


def setup(g, dtype=torch.float32):
    r"""(mean_fn, operators, arrays cast to ``dtype``) of the fixture ``g``."""
    cfg = g.meta["unet_cfg"]
    sd = synth.synth_state_dict({k: tuple(v) for k, v in g.meta["unet_shapes"].items()}, g.meta["unet_weight_seed"])
    sdd = {k: v.to(dtype) for k, v in sd.items()}
    mean = lambda x, t: sampling.karras_mean(lambda a, c: nets.time_wrapped_unet(sdd, cfg, a, c), x, t, backbone_dtype=dtype)  # noqa: E731
    ops = {"mask": go.mask_op(g["mask"]), "pool": go.pool_op(16, 16)}
    arr = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in g.arrays.items()}
    return mean, ops, arr, sd, cfg


def run_case(tag: str, mean, ops, arr, steps: int, var_y: float, eps=None, x_t=None, x1=None):
    r"""The restatement's result for the fixture case ``tag`` (``eps`` / ``x_t`` / ``x1``: replacements of the stored ones)."""
    eps = arr["eps"] if eps is None else eps
    x_t = arr["x_t"] if x_t is None else x_t
    x1 = arr["x1"] if x1 is None else x1
    t, s = arr["t"], arr["s"]
    kind, name, *rest = tag.split("_")
    A, A_inv = ops[name]
    y = arr[f"{name}_y"]
    if kind == "dps":
        if rest[0] == "loop":
            return go.loop(lambda **a: go.dps_step(mean, **a, y=y, A=A, zeta=1.0), x1, list(eps), steps)
        return go.dps_step(mean, x_t, t, s, eps[0], y=y, A=A, zeta=float(rest[0][4:]))
    if kind == "pgdm":
        if rest[0] == "loop":
            return go.loop(lambda **a: go.pgdm_step(mean, **a, y=y, A=A, A_inv=A_inv, eta=0.0), x1, list(eps), steps)
        return go.pgdm_step(mean, x_t, t, s, eps[0], y=y, A=A, A_inv=A_inv, eta=float(rest[0][3:]))
    if kind == "tmpd":
        return go.tmpd_mean(mean, x_t, t, y, A, var_y)
    if kind == "mmps":
        return go.mmps_mean(mean, x_t, t, y, A, lambda v: var_y * v, rest[0], int(rest[1][2:]))
    raise ValueError(tag)
