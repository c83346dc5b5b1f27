r"""Cases of the attention backward tests (``az_attention_bwd_f32``), shared by ``test_attention_bwd_cases_host.py`` (their
conditions, on the CPU) and ``test_gpu_attention_bwd.py`` (the kernel).  Batch 2, heads 2, the fused '(n H C)' token layout: q^ | k^
live in a (B, L, 2 H D) buffer and v in the last third of a (B, L, 3 H D) one, so token and head strides differ from the head size.
Token counts 9 / 70 / 130: ragged 32-row tiles, one / two / three key tiles of 64, several query tiles.

The reference is ``torch.nn.functional.scaled_dot_product_attention`` under fp64 autograd; ``e_ref`` is what the same function
loses under fp32 autograd on the same quantity.  Both are computed once per case and shared.
"""

import functools
import math

import torch
import torch.nn.functional as F

B, H = 2, 2

# name -> (head_dim, tokens, mask kind, amplitude of q and k)
CASES = {
    "d16_l9": (16, 9, None, 1.0),
    "d32_l70": (32, 70, None, 1.0),
    "d64_l130": (64, 130, None, 1.0),
    "d128_l70": (128, 70, None, 1.0),
    "d128_l9": (128, 9, None, 1.0),
    "d16_l130": (16, 130, None, 1.0),
    "logits30_d64_l130": (64, 130, None, 2.7),  # scale q.k reaches +-30; the row maxima sit in different key tiles
    "causal_d32_l70": (32, 70, "causal", 1.0),
    "batch_mask_d64_l70": (64, 70, "batch", 1.0),
    "head_mask_d16_l130": (16, 130, "head", 1.0),
    "tile_mask_d64_l130": (64, 130, "tile", 1.0),
    "tile_mask_d128_l130": (128, 130, "tile", 1.0),
    "wave_mask_d32_l70": (32, 70, "wave", 1.0),  # whole 32 x 32 tiles without a live pair: the wave-level skip
}


def make_mask(kind, L: int, gen: torch.Generator):
    r"""Boolean masks (True = attend) broadcastable to (B, H, L, L); every query keeps at least one live key."""
    if kind is None:
        return None
    if kind == "causal":
        return torch.ones(L, L, dtype=torch.bool).tril()
    if kind in ("batch", "head"):
        shape = (B, 1, L, L) if kind == "batch" else (1, H, L, L)
        m = torch.rand(shape, generator=gen) < 0.6
        m |= torch.eye(L, dtype=torch.bool)  # (the diagonal stays live)
        return m
    if kind == "tile":
        # queries 0, 3, 6, ...: the whole key tile [0, 64) is blank -- before their first live key; queries 1, 4, 7, ...: the whole
        # tile [64, 128) is blank -- after their first live key; the others see every key
        m = torch.ones(L, L, dtype=torch.bool)
        m[0::3, :64] = False
        m[1::3, 64:128] = False
        return m
    if kind == "wave":
        # the 32 consecutive queries [32, 64) of one wave share a blank LEADING key tile [0, 32): the statistics and dQ passes skip a
        # tile before the first live key; the queries [0, 32) lose the keys [32, 64): a blank tile after it.  In the dK / dV pass
        # the waves of the keys [0, 32) and [32, 64) skip the matching query tiles.
        m = torch.ones(L, L, dtype=torch.bool)
        m[32:64, :32] = False
        m[:32, 32:64] = False
        return m
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def make_case(name: str):
    r"""-> dict(q, k, v, dout: (B, H, L, D) fp32; mask; scale; D; L)."""
    D, L, kind, amp = CASES[name]
    gen = torch.Generator().manual_seed(1000 + sorted(CASES).index(name))
    q = torch.randn(B, H, L, D, generator=gen) * amp
    k = torch.randn(B, H, L, D, generator=gen) * amp
    v = torch.randn(B, H, L, D, generator=gen)
    dout = torch.randn(B, H, L, D, generator=gen)
    return dict(q=q, k=k, v=v, dout=dout, mask=make_mask(kind, L, gen), scale=1.0 / math.sqrt(D), D=D, L=L)


def sdpa_grads(q, k, v, dout, mask, scale, dtype):
    r"""(out, dq, dk, dv) of scaled_dot_product_attention under autograd in ``dtype``, returned as fp64."""
    qq, kk, vv = (t.detach().to(dtype).clone().requires_grad_() for t in (q, k, v))
    with torch.enable_grad():
        out = F.scaled_dot_product_attention(qq, kk, vv, attn_mask=mask, scale=scale)
        grads = torch.autograd.grad(out, (qq, kk, vv), dout.to(dtype))
    return (out.detach().double(), *(g.double() for g in grads))


@functools.lru_cache(maxsize=None)
def reference(name: str):
    r"""-> (out, dq, dk, dv) in fp64 and e_ref = (e_dq, e_dk, e_dv): the fp32 autograd's error relative to the fp64 result's
    largest magnitude."""
    c = make_case(name)
    r64 = sdpa_grads(c["q"], c["k"], c["v"], c["dout"], c["mask"], c["scale"], torch.float64)
    r32 = sdpa_grads(c["q"], c["k"], c["v"], c["dout"], c["mask"], c["scale"], torch.float32)
    e_ref = tuple(float((a - b).abs().max() / b.abs().max()) for a, b in zip(r32[1:], r64[1:]))
    return r64, e_ref


def logits(name: str) -> torch.Tensor:
    c = make_case(name)
    return c["scale"] * c["q"].double() @ c["k"].double().transpose(-1, -2)
