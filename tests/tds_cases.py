r"""Cases and setup shared by the host and the GPU tests of the twisted diffusion sampler -- TEST INFRASTRUCTURE.

* the cases of ``tests/golden/g29_tds.npz`` as calls of the restatement (``tds_oracle``);
* the inputs of the resampling kernel's test (log-weights and uniforms, chosen by seed search so that every uniform keeps a
  margin to every fp64 CDF value: the host test asserts the margin, the GPU test then demands equal indices);
* the inputs of the proposal kernel's test.
"""

from __future__ import annotations

import math

import torch

import guidance_vjp_oracle as go
import tds_oracle as to
from oracle import nets, sampling, synth

CASES = ["mask_step", "mask_loop", "pool_step", "pool_loop"]
SEED = {"mask_step": 0, "mask_loop": 1, "pool_step": 2, "pool_loop": 3}  # offsets to the fixture's seed, one stream per case


def setup(g, dtype=torch.float32):
    r"""(mean_fn, twists, arrays cast to ``dtype``, state dict, config) of the fixture ``g``."""
    cfg = g.meta["unet_cfg"]
    sd = synth.synth_state_dict({k: tuple(v) for k, v in g.meta["unet_shapes"].items()}, g.meta["unet_weight_seed"])
    sdd = {k: v.to(dtype) for k, v in sd.items()}
    mean = lambda x, t: sampling.karras_mean(lambda a, c: nets.time_wrapped_unet(sdd, cfg, a, c), x, t, backbone_dtype=dtype)  # noqa: E731
    arr = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in g.arrays.items()}
    twists = make_twists(arr, g.meta["var_y"])
    return mean, twists, arr, sd, cfg


def make_twists(arr: dict, var_y: float) -> dict:
    ops = {"mask": go.mask_op(arr["mask"])[0], "pool": go.pool_op(16, 16)[0]}
    return {name: to.gaussian_twist(arr[f"{name}_y"], A, var_y) for name, A in ops.items()}


def run_case(tag: str, mean, twists, arr, steps: int, ancestors=None, eps=None):
    r"""The restatement on the fixture case ``tag``: a list of per-step dicts (one entry for a ``_step`` case).  Without
    ``ancestors`` / ``eps`` the caller seeds the CPU generator and the restatement draws like the reference."""
    name, kind = tag.split("_")
    if kind == "step":
        carry: dict = {}
        x_s = to.tds_step(mean, twists[name], arr["x_t"], arr["t"], arr["s"], carry, None if ancestors is None else ancestors[0],
                          None if eps is None else eps[0])
        return [{"x_s": x_s, "log_w": carry["log_w"], "ancestors": carry["ancestors"], "w": carry["w"], "log_p": carry["log_p"]}]
    return to.tds_loop(mean, twists[name], arr["x1"], steps, ancestors, eps)[1]


# ------------------------------------------------------------------------------------------------------- resample kernel
RESAMPLE_K = (1, 2, 5, 64, 257)
RESAMPLE_KINDS = ("randn3", "dominant", "neginf")
RESAMPLE_MARGIN = 1e-5
RESAMPLE_CASES = [(K, kind, prev) for K in RESAMPLE_K for kind in RESAMPLE_KINDS for prev in (False, True)]


def _resample_draw(K: int, kind: str, prev: bool, seed: int):
    g = torch.Generator().manual_seed(seed)
    log_p = 3 * torch.randn(K, generator=g)
    log_w_prev = 3 * torch.randn(K, generator=g) if prev else None
    if kind == "dominant":
        log_p[int(torch.randint(K, (1,), generator=g))] += 50.0
    elif kind == "neginf" and K > 1:  # several particles of weight 0, the first and the last among them where K allows
        dead = torch.randperm(K, generator=g)[: max(1, K // 3)].tolist() + ([0, K - 1] if K > 4 else [])
        log_p[dead] = -math.inf
    u = torch.rand(K, generator=g)
    return log_p, log_w_prev, u


def resample_case(K: int, kind: str, prev: bool):
    r"""``(log_p, log_w_prev or None, u)``: the first seed whose uniforms all lie at least ``RESAMPLE_MARGIN`` from every fp64
    CDF value (and from 0 and 1)."""
    base = 1000 * K + 10 * RESAMPLE_KINDS.index(kind) + int(prev)
    for seed in range(base, base + 1000):
        log_p, log_w_prev, u = _resample_draw(K, kind, prev, seed)
        log_w = log_p.double() if log_w_prev is None else log_p.double() + log_w_prev.double()
        _, _, c = to.inverse_cdf(log_w, u)
        edges = torch.cat([torch.zeros(1, dtype=torch.float64), c])
        if float(to.cdf_margin(edges, u).min()) >= 2 * RESAMPLE_MARGIN:
            return log_p, log_w_prev, u
    raise AssertionError((K, kind, prev))


# -------------------------------------------------------------------------------------------------------- propose kernel
# (K, N): one element; odd sizes (4-byte path); one float4 group short of a span; more than one span and chunk on the 4-byte
# path; whole spans + a float4 remainder + several chunks; more spans than chunks (a workgroup strides over its row)
PROPOSE_SHAPES = [(1, 1), (3, 7), (5, 1024), (4, 4099), (2, 16387), (3, 8200), (700, 8200)]
PROPOSE_ANCESTORS = ("identity", "equal", "permutation", "repeats")
PROPOSE_SCORE_SCALES = (1e-3, 1.0, 1e3)
PROPOSE_TIMES = ((1.0, 0.875), (0.125, 0.0))
PROPOSE_C = 8  # csrc/tds.hip: 1 rounding per term + 5 dependent fp32 adds + 1 for the fp64 -> fp32 result, rounded up


def propose_coef(t: float, s: float) -> torch.Tensor:
    r"""The kernel's coefficient array from the VP schedule at (t, s), in fp32 as the sampler forms it."""
    a_t, s_t = sampling.vp_schedule(torch.tensor(t))
    a_s, s_s = sampling.vp_schedule(torch.tensor(s))
    tau = (a_t / a_s * s_s / s_t) ** 2
    scale = s_s * torch.sqrt(1 - tau)
    return torch.stack([a_t, a_s, s_t**2 / a_t, s_s * torch.sqrt(tau) / s_t, scale, 1 / scale]).float()


def propose_ancestors(kind: str, K: int, g: torch.Generator) -> torch.Tensor:
    if kind == "identity":
        return torch.arange(K)
    if kind == "equal":
        return torch.full((K,), K - 1)
    if kind == "permutation":
        return torch.randperm(K, generator=g)
    return torch.randint(K, (K,), generator=g)


def propose_inputs(K: int, N: int, score_scale: float, seed: int = 0):
    g = torch.Generator().manual_seed(seed + 7 * K + N)
    x_t = torch.randn(K, N, generator=g)
    x_hat = 1e2 * torch.randn(K, N, generator=g)
    score = score_scale * torch.randn(K, N, generator=g)
    z = torch.randn(K, N, generator=g)
    log_p = 3 * torch.randn(K, generator=g)
    return x_t, x_hat, score, z, log_p, g


def propose_reference(x_t, x_hat, score, z, k, log_p, coef):
    r"""fp64: ``(x_s, log_w_next, x_s error scale per element, log_w error scale per particle)`` from the fp32 inputs."""
    a_t, a_s, c_s, k_x, scale, _ = coef.double().tolist()
    xt, xh, sc, zd = x_t.double()[k], x_hat.double()[k], score.double()[k], z.double()
    m = xh + c_s * sc
    x_s = a_s * m + k_x * (xt - a_t * m) + scale * zd
    x_mag = (a_s * m).abs() + (k_x * xt).abs() + (k_x * a_t * m).abs() + (scale * zd).abs()
    gq = (a_s - k_x * a_t) * c_s * sc / scale
    term = zd * gq + gq * gq / 2
    lp = log_p.double()[k]
    return x_s, -term.sum(1) - lp, x_mag, term.abs().sum(1) + lp.abs()


def two_sum_form(x_t, x_hat, score, z, k, log_p, coef):
    r"""The reference's own form (``tds.py:83-102``) in the dtype and on the device of its inputs: two summed log-densities."""
    a_t, a_s, c_s, k_x, scale, _ = coef.unbind()
    x_t, x_hat, log_p, score = x_t[k], x_hat[k], log_p[k], score[k]
    loc_of = lambda x: a_s * x + k_x * (x_t - a_t * x)  # noqa: E731
    loc, loc_y = loc_of(x_hat), loc_of(x_hat + c_s * score)
    x_s = loc_y + scale * z
    lq = lambda mu: (-((x_s - mu) ** 2) / (2 * scale**2) - scale.log() - math.log(math.sqrt(2 * math.pi))).sum(1)  # noqa: E731
    return lq(loc) - lq(loc_y) - log_p
