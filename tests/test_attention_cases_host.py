r"""Conditions on the inputs of test_gpu_attention.py, checked on the CPU: the GPU tests cannot pass by testing nothing.
Every family of tests/attention_cases.py is asserted to reach the branch of the kernels' online softmax it was written for
(``lazy_trace`` emulates the rule documented in attention_x3_kernel), to stay inside the f16x2 entry's stated domain, and the
fp64 reference is compared with torch's own SDPA."""

import math

import pytest
import torch

import attention_cases as ac

torch.set_grad_enabled(False)

GRID_SHAPES = [(2, 2, 200, 64), (1, 3, 300, 16), (2, 1, 129, 64), (1, 2, 64, 16)]  # test_softmax_dynamics
WAVE_GRID_SHAPES = [(2, 2, 256, 16), (2, 2, 512, 64), (2, 2, 256, 64), (2, 2, 288, 64)]  # (T, D) of test_eight_wave_form, few slices
RMS_SHAPES = [(T, D) for D in (32, 64, 80, 128) for T in (100, 288)] + [(256, 80)]
MASK_T = (72, 150, 257)


def mixed_within_a_wave(late):
    r"""min < max late jumps within at least one block of 32 consecutive queries (one wave of the kernels)."""
    T = late.shape[-1]
    return any(bool((late[..., i:i + 32].amin(-1) < late[..., i:i + 32].amax(-1)).any()) for i in range(0, T, 32))


def check_profile(name, late, pmax, T, min_big):
    if name == "ramp_small" and T >= 128:  # (two sub-tiles 4 apart cannot reach either condition)
        assert 128 < pmax.max().item() <= 256 and late.min().item() >= 1, (pmax.max().item(), late.min().item())
    elif name == "ramp_big":
        assert late.min().item() >= min_big, (late.min().item(), min_big)
    elif name == "threshold":
        assert mixed_within_a_wave(late)
        assert pmax.max().item() <= 256
    elif name in ("descend", "spike_first"):
        assert late.max().item() == 0
    elif name == "spike_last":
        assert late.min().item() == 1 and late.max().item() == 1


@pytest.mark.parametrize("B,H,T,D", GRID_SHAPES + WAVE_GRID_SHAPES)
@pytest.mark.parametrize("name", ac.PROFILES)
def test_grid_families(name, B, H, T, D):
    """Grid inputs: exact in bf16 / f16 and in the fp32 q k^T; each profile drives the lazy maximum as intended; the stated element
    ranges; S_abs <= 1.5 max |s| (the q_term of the bound stays near 1e-5); inside the f16x2 entry's domain."""
    q, k, v, scale = ac.grid_inputs(name, B, H, T, D)
    assert D in ac.GRID_DIMS and math.log2(scale) == round(math.log2(scale))
    assert ac.grid_is_exact(q, k, v)
    for t, step, lim in ((q, 0.125, 15.0), (k[..., 1:], 0.125, 15.0), (k[..., :1], 0.5, 63.0), (v, 0.125, 2.0)):
        assert bool((t / step == (t / step).round()).all()) and t.abs().max().item() <= lim
    assert q[..., 1:].abs().max() <= 1 and k[..., 1:].abs().max() <= 1 and bool((q[..., 0] == 15).all())
    late, pmax = ac.lazy_trace(q, k, scale)
    check_profile(name, late, pmax, T, T // 32 - 1)
    s = (q.double() @ k.double().transpose(-1, -2)) * scale * ac.LOG2E
    assert ac.s_abs(q, k, scale) <= 1.5 * s.abs().max().item()
    assert k.abs().max() < 4094 and (q * scale * ac.LOG2E).abs().max() < 1e6 and v.abs().max() < 1e6


@pytest.mark.parametrize("T,D", RMS_SHAPES)
@pytest.mark.parametrize("name", ["ramp_small", "ramp_big", "threshold"])
def test_rms_families(name, T, D):
    """Generic RMS-normed inputs: the normalised, gained scores move the maximum (where the profile had to be compressed, D = 32 at
    T = 288, ramp_big still jumps in at least 3 sub-tiles for every query), the scale is above 1 / sqrt(D), and the plan-time bound
    the engine routes by stays inside the f16x2 limits."""
    from azula_amd import engine

    q, k, v, scale, gains = ac.rms_inputs(name, 2, 2, T, D)
    assert 1 / math.sqrt(D) < scale <= 1.0
    qe, ke = ac.effective_qk(q.double(), k.double(), ac.RMS_EPS, gains)
    late, pmax = ac.lazy_trace(qe, ke, scale)
    check_profile(name, late, pmax, T, min(3, T // 32))
    if name == "ramp_small":
        assert late.min().item() >= 1
    kmax, qsmax = engine.attention_qk_bound(D, 0, scale, gains)
    assert kmax < engine.ATTN_H2_K_MAX and qsmax < engine.ATTN_H2_QS_MAX
    assert ke.abs().max().item() <= kmax and (qe * scale * ac.LOG2E).abs().max().item() <= qsmax  # (the bound is a bound)


def dead_tiles(mask):
    r"""(some query has a fully dead leading 64-key tile, ... 32-key sub-tile, ... trailing 64-key tile) of a (..., T, T) mask."""
    T = mask.shape[-1]
    last = ac.TILE * ((T - 1) // ac.TILE)
    lead = ~mask[..., :, :ac.TILE].any(-1)
    lead_sub = ~mask[..., :, :ac.SUB].any(-1)
    trail = ~mask[..., :, last:].any(-1)
    return bool(lead.any()), bool(lead_sub.any()), bool(trail.any())


@pytest.mark.parametrize("T", MASK_T)
@pytest.mark.parametrize("kind", ac.MASK_SHAPES)
@pytest.mark.parametrize("family", ac.MASKS)
def test_mask_families(family, kind, T):
    """Every query keeps a live key (except the chosen dead rows); the banded families leave whole key tiles dead.

    A fully dead leading 64-key tile needs a query whose first live key is >= 64: band (|i - j| <= 20) and blocks (block 48) have
    one from T = 150 on; at T = 72 they are held to a fully dead leading 32-key sub-tile.  anticausal (key >= query) always
    attends to the last key, so it has dead leading tiles only; the dead trailing tiles of that pair come from causal."""
    B, H = 2, 3
    m = ac.make_mask(family, kind, B, H, T)
    assert m.dtype == torch.bool and tuple(m.shape) == {"LL": (T, T), "B1LL": (B, 1, T, T), "1HLL": (1, H, T, T), "BHLL": (B, H, T, T)}[kind]
    full = ac.expand_mask(m, B, H)
    if kind != "LL" and family != "lone_tail":  # a different draw per batch / head
        flat = m.reshape(-1, T, T)
        assert all(not torch.equal(flat[0], flat[i]) for i in range(1, flat.shape[0]))
    live = full.any(-1)
    if family == "dead_rows":
        nb, nh = (1, 1) if kind == "LL" else (m.shape[0], m.shape[1])
        for b in range(B):
            for h in range(H):
                idx = (b if nb > 1 else 0) * nh + (h if nh > 1 else 0)
                assert torch.nonzero(~live[b, h]).flatten().tolist() == ac.dead_rows(T, idx)
        rows = ac.dead_rows(T, 0)
        assert rows[0] < 32 and rows[-1] >= T - 32 and any(T // 2 - 32 <= r <= T // 2 + 32 for r in rows)
    else:
        assert bool(live.all())
    lead, lead_sub, trail = dead_tiles(full)
    if family in ("band", "blocks"):
        assert trail and (lead if T >= 150 else lead_sub)
    if family == "anticausal":
        assert lead
    if family == "causal":
        assert trail
    if family == "lone_tail":
        assert bool((full.sum(-1) == 1).all()) and bool(full[..., T - 1].all())
    if family == "masked_spike":
        spike = ~full.any(-2)
        assert bool(spike.any(-1).all())  # every slice has spiked (dead) keys
        for D in (16, 64, 80):
            q, k, v, scale = ac.grid_inputs("flat", B, H, T, D, spike=spike)
            s = (q.double() @ k.double().transpose(-1, -2)) * scale * ac.LOG2E
            gap = s[spike[:, :, None, :].expand_as(s)].min() - s[full].max()
            assert gap > 90  # a maximum taken before the mask underflows every live term (2^-90)
            assert k.abs().max() < 4094
            if D in ac.GRID_DIMS:
                assert ac.grid_is_exact(q, k, v) and k[..., 0].abs().max() <= 63


def test_causal_with_a_rising_maximum():
    """causal + ramp_big: the live maximum rises by 12 per sub-tile while the trailing tiles are dead; late queries jump in every
    live sub-tile."""
    T = 150
    q, k, v, scale = ac.grid_inputs("ramp_big", 2, 2, T, 64)
    m = ac.make_mask("causal", "LL", 2, 2, T)
    late, _ = ac.lazy_trace(q, k, scale, m)
    assert late[..., T - 1].min().item() == 4 and late[..., :32].max().item() == 0


@pytest.mark.parametrize("case", ["masked", "rms"])
def test_reference_against_torch_sdpa(case):
    """``reference`` (explicit softmax) equals F.scaled_dot_product_attention in float64."""
    import torch.nn.functional as F

    g = torch.Generator().manual_seed(5)
    B, H, T, D = 2, 3, 70, 16
    q, k, v = (torch.randn(B, H, T, D, generator=g) for _ in range(3))
    if case == "masked":
        m = ac.make_mask("bernoulli", "BHLL", B, H, T)
        got, want = ac.reference(q, k, v, 0.3, mask=m), ac.sdpa_check(q, k, v, 0.3, m)
    else:
        gains = (1 + 0.2 * torch.randn(D, generator=g), 1 + 0.2 * torch.randn(D, generator=g))
        qn, kn = (F.rms_norm(t.double(), (D,), eps=1e-5) * w.double() for t, w in ((q, gains[0]), (k, gains[1])))
        got, want = ac.reference(q, k, v, 0.7, rms=True, gains=gains), ac.sdpa_check(qn, kn, v, 0.7, None)
    assert got.dtype == torch.float64 and (got - want).abs().max().item() < 1e-13
    # a row without a live key is NaN, and only that row
    m = torch.ones(T, T, dtype=torch.bool)
    m[5] = False
    out = ac.reference(q, k, v, 0.3, mask=m)
    assert bool(torch.isnan(out[:, :, 5]).all()) and bool(torch.isfinite(out[:, :, [4, 6]]).all())


def test_bounds_are_the_derived_ones():
    """The figures of the bound: M, eps_q and the half units; q_term at the widest profile stays near 1e-5 (f32) / 4e-5 (f16x2)."""
    assert ac.FP32_CLASS == {"az_attention_f32": (4, 2.0 ** -24), "az_attention_x3_f32": (4, 2.0 ** -24), "az_attention_f16x2_f32": (16, 2.0 ** -22)}
    assert ac.HALF_UNIT == {"az_attention_bf16_f32": 2.0 ** -8, "az_attention_f16_f32": 2.0 ** -11}
    assert ac.bound_fp32_class("az_attention_f32", 1e-7, 2.0) == max(4e-7, 2.0 ** -19)
    assert ac.bound_fp32_class("az_attention_f16x2_f32", 1e-5, 2.0) == 16e-5
    assert ac.bound_half_grid("az_attention_bf16_f32", 1e-7, 2.0) == 2.0 ** -6 + 4e-7
    q, k, v, scale = ac.grid_inputs("ramp_big", 1, 3, 300, 16)
    sabs, vmax = ac.s_abs(q, k, scale), v.abs().max().item()
    assert ac.bound_fp32_class("az_attention_f32", 0.0, vmax, sabs) - 2.0 ** -20 * vmax < 2e-5
    assert ac.bound_fp32_class("az_attention_f16x2_f32", 0.0, vmax, sabs) - 2.0 ** -20 * vmax < 8e-5
