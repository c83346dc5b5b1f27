r"""The five attention entries against a float64 reference where their online softmax has work to do: score profiles that move
the running maximum (every sub-tile, never, at the lazy rule's threshold, from one late key), boolean masks that cross the
32-key sub-tile and the 64-key LDS tile (dead leading / middle / trailing tiles, dead rows, per-batch and per-head strides), and
the 8-wave workgroup form of attention_x3_kernel on both sides of its launcher's rule.  Inputs and the reference live in
tests/attention_cases.py; test_attention_cases_host.py asserts on the CPU that each family reaches what it is for.

Nothing is compared with a kernel's own output.  Every case computes ``ref`` (float64) and ``e32`` = max |float32 torch on the
CPU - ref| on the same inputs and asserts max |out - ref| <= bound:

* fp32-class entries: max(M e32, 2^-20 max|v|) + q_term, M = 4 (az_attention_f32, az_attention_x3_f32) or 16
  (az_attention_f16x2_f32); q_term on grid inputs only (attention_cases.bound_fp32_class has the derivation);
* 2-byte entries: 2 u max|v| + 4 e32 on grid inputs, u = 2^-8 (bf16) / 2^-11 (f16) (attention_cases.bound_half_grid); on randn
  inputs test_attention_half_kernel's bars, 3e-2 / 4e-3 x max(1, max|ref|).

Each case prints ``err``, ``e32`` and their ratio; DESIGN.md (section 4) holds the largest ratio per entry.  The entries are forced
per test (test_attention_kernel's swap of the tape's entry), so AZ_FP32_MFMA does not change what runs."""

import functools
import math

import pytest
import torch

import attention_cases as ac

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

HALF_OF = {"az_attention_bf16_f32": torch.bfloat16, "az_attention_f16_f32": torch.float16}
HALF_BAR = {"az_attention_bf16_f32": 3e-2, "az_attention_f16_f32": 4e-3}  # test_attention_half_kernel's, x max(1, max|ref|)


def run_entry(monkeypatch, entry, q, k, v, scale, order="nHC", rms=False, gains=None, mask=None, planned=None):
    r"""(B, H, T, D) q, k, v through Builder.attention and the tape on ``entry`` -> (B, H, T, D) float64 on the CPU.
    ``planned``: the entry the engine itself must have put on the tape (f16x2 mode) before a forced one replaces it."""
    from azula_amd import _lib, engine
    from azula_amd.engine import Act, Builder

    monkeypatch.setattr(engine, "ATTN_X3", True)
    monkeypatch.setattr(engine, "FP32_MFMA", "f16x2")
    B, H, T, D = q.shape
    qkv = ac.pack_qkv(q, k, v, order)
    bld = Builder(torch.device("cuda"), half=HALF_OF.get(entry))
    act = Act(qkv.cuda().reshape(-1), B, T, 1, 3 * H * D, 3 * H * D, True)
    act.bounded = True
    qkw = None if gains is None else (bld.const(gains[0]), bld.const(gains[1]))
    out = bld.attention(act, H, order, bool(rms), scale, eps=ac.RMS_EPS, qk_weight=qkw, mask=mask)
    name = bld.tape.ops[-1][2]
    if entry in HALF_OF:
        assert name == entry
    else:
        assert name in ac.FP32_CLASS and (planned is None or name == planned), name
        bld.tape.ops[-1] = (getattr(_lib.lib(), entry), bld.tape.ops[-1][1], entry)
    bld.tape.run()
    torch.cuda.synchronize()
    return out.buf[: B * T * H * D].reshape(B, T, H, D).permute(0, 2, 1, 3).double().cpu()


def check(tag, entry, got, ref, e32, bound):
    r"""NaN exactly where the reference is NaN (rows without a live key), max |got - ref| <= bound elsewhere."""
    assert torch.equal(torch.isnan(got), torch.isnan(ref)), (tag, entry, "NaN pattern differs")
    err = ac.max_abs_err(got, ref)
    print(f"ATTN {entry} {tag}: err {err:.3e} e32 {e32:.3e} err/e32 {err / max(e32, 1e-300):.2f} bound {bound:.3e}")
    assert err <= bound, (tag, entry, err, e32, bound)
    return err


def bound_for(entry, ref, e32, vmax, sabs=None, grid=False):
    if entry in ac.FP32_CLASS:
        return ac.bound_fp32_class(entry, e32, vmax, sabs if grid else None)
    if grid:
        return ac.bound_half_grid(entry, e32, vmax)
    return HALF_BAR[entry] * max(1.0, ref[torch.isfinite(ref)].abs().max().item())


def refs(q, k, v, scale, mask=None, rms=None, gains=None):
    ref = ac.reference(q, k, v, scale, mask, rms, gains)
    r32 = ac.reference_fp32(q, k, v, scale, mask, rms, gains)
    assert torch.equal(torch.isnan(r32), torch.isnan(ref))
    return ref, ac.max_abs_err(r32, ref)


# ------------------------------------------------------------------------------------------------ score dynamics
GRID_SHAPES = [(2, 2, 200, 64), (1, 3, 300, 16), (2, 1, 129, 64), (1, 2, 64, 16)]  # two to ten sub-tiles, ragged and exact ends


@functools.lru_cache(maxsize=None)
def grid_case(name, B, H, T, D):
    q, k, v, scale = ac.grid_inputs(name, B, H, T, D)
    ref, e32 = refs(q, k, v, scale)
    return q, k, v, scale, ref, e32, ac.s_abs(q, k, scale), v.abs().max().item()


@functools.lru_cache(maxsize=None)
def rms_case(name, B, H, T, D):
    q, k, v, scale, gains = ac.rms_inputs(name, B, H, T, D)
    ref, e32 = refs(q, k, v, scale, None, ac.RMS_EPS, gains)
    return q, k, v, scale, gains, ref, e32, v.abs().max().item()


@pytest.mark.parametrize("B,H,T,D", GRID_SHAPES)
@pytest.mark.parametrize("order", ["nHC", "H3C"])
@pytest.mark.parametrize("name", ac.PROFILES)
@pytest.mark.parametrize("entry", ac.ENTRIES)
def test_softmax_dynamics(monkeypatch, entry, name, order, B, H, T, D):
    """Exact-score grid inputs: the maximum rises below the lazy threshold (probabilities up to 2^8 before a rescale), above it
    (a rescale every sub-tile), at it (jumping and resting lanes in one wave), falls (later terms underflow), or one key 2^60
    above the rest arrives first or last (inside the ragged tail).

    az_attention_f32 missed ramp_big at 2 x 2 x 200 x 64 (err 9.49e-6, bound 8.14e-6) while it scaled q by the whole of
    scale log2 e before the contraction: every accumulation step rounded a partial score of up to 38 log2 units.  It now scales
    q by the power of two only and the score by the mantissa; this case is its regression test."""
    q, k, v, scale, ref, e32, sabs, vmax = grid_case(name, B, H, T, D)
    got = run_entry(monkeypatch, entry, q, k, v, scale, order)
    check(f"grid {name} {order} {B}x{H}x{T}x{D}", entry, got, ref, e32, bound_for(entry, ref, e32, vmax, sabs, grid=True))


@pytest.mark.parametrize("T", [100, 288])
@pytest.mark.parametrize("D", [32, 64, 80, 128])
@pytest.mark.parametrize("name", ["ramp_small", "ramp_big", "threshold"])
@pytest.mark.parametrize("entry", list(ac.FP32_CLASS))
def test_softmax_dynamics_rms_normed(monkeypatch, entry, name, D, T):
    """Generic rows, RMS norm and learned gains in the kernel, a scale above 1 / sqrt(D): the route production takes to
    az_attention_f16x2_f32 (asserted on the tape up to head size 80; 128 plans the fp32 kernel and the others are forced)."""
    q, k, v, scale, gains, ref, e32, vmax = rms_case(name, 2, 2, T, D)
    planned = "az_attention_f16x2_f32" if D <= 80 else "az_attention_f32"
    got = run_entry(monkeypatch, entry, q, k, v, scale, "nHC", ac.RMS_EPS, gains, planned=planned)
    check(f"rms {name} 2x2x{T}x{D}", entry, got, ref, e32, bound_for(entry, ref, e32, vmax))


# ------------------------------------------------------------------------------------------------ masks
@functools.lru_cache(maxsize=None)
def mask_case(family, kind, T, D):
    B, H = 2, 3
    mask = ac.make_mask(family, kind, B, H, T)
    grid = False
    if family == "masked_spike":  # the masked keys 2^100 above the live ones: a maximum taken before the mask underflows every live term
        q, k, v, scale = ac.grid_inputs("flat", B, H, T, D, spike=~ac.expand_mask(mask, B, H).any(-2))
        grid = D in ac.GRID_DIMS
    else:
        g = torch.Generator().manual_seed(T * 131 + D)
        q, k, v = (torch.randn(B, H, T, D, generator=g) for _ in range(3))
        scale = 1.0 / math.sqrt(D)
    ref, e32 = refs(q, k, v, scale, mask)
    return q, k, v, scale, mask, ref, e32, ac.s_abs(q, k, scale), v.abs().max().item(), grid


@pytest.mark.parametrize("D", [16, 64, 80])
@pytest.mark.parametrize("T", [72, 150, 257])
@pytest.mark.parametrize("kind", ac.MASK_SHAPES)
@pytest.mark.parametrize("family", ac.MASKS)
def test_masks_across_tiles(monkeypatch, family, kind, T, D):
    """All five entries under masks that cross sub-tiles and LDS tiles, in every broadcast shape (mask_bstride / mask_hstride 0
    and not), each slice its own draw.  dead_rows: NaN on exactly the rows without a live key in every batch and head, finite and
    within the bound elsewhere (``check`` compares the NaN pattern with the reference's in every case)."""
    q, k, v, scale, mask, ref, e32, sabs, vmax, grid = mask_case(family, kind, T, D)
    if family == "dead_rows":
        full = ac.expand_mask(mask, 2, 3)
        assert torch.equal(torch.isnan(ref).all(-1), ~full.any(-1)) and bool(torch.isnan(ref).any())
    for entry in ac.ENTRIES:
        got = run_entry(monkeypatch, entry, q, k, v, scale, "nHC", mask=mask)
        check(f"mask {family} {kind} T{T} D{D}", entry, got, ref, e32, bound_for(entry, ref, e32, vmax, sabs, grid))


@pytest.mark.parametrize("kind", ["LL", "BHLL"])
@pytest.mark.parametrize("entry", ac.ENTRIES)
def test_causal_mask_under_a_rising_maximum(monkeypatch, entry, kind):
    """causal + ramp_big: the live maximum rises by 2^12 per sub-tile while the trailing tiles are dead."""
    B, H, T, D = 2, 2, 150, 64
    q, k, v, scale, _, _, sabs, vmax = grid_case("ramp_big", B, H, T, D)
    mask = ac.make_mask("causal", kind, B, H, T)
    ref, e32 = refs(q, k, v, scale, mask)
    got = run_entry(monkeypatch, entry, q, k, v, scale, "nHC", mask=mask)
    check(f"mask causal+ramp_big {kind}", entry, got, ref, e32, bound_for(entry, ref, e32, vmax, sabs, grid=True))


# ------------------------------------------------------------------------------------------------ the 8-wave form
def takes_eight_waves(B, H, T, D):
    r"""attention_x3_launch: ``wide = head_dim <= 80 && tokens % 256 == 0 && batch * heads * (tokens / 256) >= 512``."""
    return D <= 80 and T % 256 == 0 and B * H * (T // 256) >= 512


WAVE_SHAPES = [(32, 16, 256, 16), (16, 16, 512, 64), (32, 16, 256, 80), (31, 16, 256, 64), (32, 16, 288, 64)]
WAVE_CASES = [(s, p, False) for s in WAVE_SHAPES for p in ("randn", "ramp_big", "threshold")] + [((32, 16, 256, 16), "randn", True)]


@pytest.mark.parametrize("shape,name,masked", WAVE_CASES, ids=lambda x: "x".join(map(str, x)) if isinstance(x, tuple) else str(x))
def test_eight_wave_form(monkeypatch, shape, name, masked):
    """az_attention_x3_f32 and az_attention_f16x2_f32 on both sides of the launcher's rule: the first three shapes take
    attention_x3_kernel<D, 8, .> (product exactly 512), (31, 16, 256, 64) has 496 blocks and (32, 16, 288, 64) no whole 256-query
    blocks.  Where the 8-wave form ran, the same entry on the first two batches alone (64 blocks: the 4-wave form) must agree with
    it within the same bound.  Head size 80 has no power-of-two scale: its profiles come from the RMS-normed family."""
    B, H, T, D = shape
    assert takes_eight_waves(B, H, T, D) == (shape in WAVE_SHAPES[:3]) and not takes_eight_waves(2, H, T, D)
    rms, gains, sabs, grid, mask = None, None, None, False, None
    if name == "randn":
        g = torch.Generator().manual_seed(T + D)
        q, k, v = (torch.randn(B, H, T, D, generator=g) for _ in range(3))
        scale = 1.0 / math.sqrt(D)
    elif D in ac.GRID_DIMS:
        q, k, v, scale = ac.grid_inputs(name, B, H, T, D)
        sabs, grid = ac.s_abs(q, k, scale), True
    else:
        q, k, v, scale, gains = ac.rms_inputs(name, B, H, T, D)
        rms = ac.RMS_EPS
    if masked:
        mask = torch.rand(B, H, T, T, generator=torch.Generator().manual_seed(9)) < 0.5
        mask |= torch.eye(T, dtype=torch.bool)
    ref, e32 = refs(q, k, v, scale, mask, rms, gains)
    vmax = v.abs().max().item()
    for entry in ("az_attention_x3_f32", "az_attention_f16x2_f32"):
        bound = bound_for(entry, ref, e32, vmax, sabs, grid)
        got = run_entry(monkeypatch, entry, q, k, v, scale, "nHC", rms, gains, mask)
        check(f"waves {name} {B}x{H}x{T}x{D} masked={masked}", entry, got, ref, e32, bound)
        if takes_eight_waves(B, H, T, D):
            four = run_entry(monkeypatch, entry, q[:2], k[:2], v[:2], scale, "nHC", rms, gains, None if mask is None else mask[:2])
            check(f"waves {name} {B}x{H}x{T}x{D} 4-wave slices", entry, four, ref[:2], e32, bound)
            d = (got[:2] - four).abs().max().item()
            print(f"ATTN {entry} 8-wave vs 4-wave max|d| {d:.3e}")
            assert d <= bound, (entry, d, bound)


# ------------------------------------------------------------------------------------------------ padded heads under a mask
@pytest.mark.parametrize("mask_kind", ["causal", "bernoulli"])
@pytest.mark.parametrize("d,dp", [(24, 32), (48, 64)])
def test_padded_heads_with_masks(d, dp, mask_kind):
    """MultiheadSelfAttention with head sizes the kernels are not instantiated for (zero-padded, AzAttnArgs.norm_dim) under a mask,
    L = 150, against ``reference`` with the module's own weights applied in float64.  Bound: the module-level bar of
    test_standalone_attention_with_masks, 2e-5 x max(1, max|ref|) (two projections around the kernel)."""
    from azula_amd import engine
    from azula_amd.nn import MultiheadSelfAttention

    assert engine.attn_padded_dim(d, None) == dp
    heads, B, L = 4, 2, 150
    Cc = heads * d
    torch.manual_seed(d)
    msa = MultiheadSelfAttention(Cc, attention_heads=heads)
    x = torch.randn(B, L, Cc)
    mask = ac.make_mask(mask_kind, "LL" if mask_kind == "causal" else "BHLL", B, heads, L)

    def forward(dtype):
        w, b, wy = msa.qkv_proj.weight.detach().to(dtype), msa.qkv_proj.bias.detach().to(dtype), msa.y_proj.weight.detach().to(dtype)
        qkv = (x.to(dtype) @ w.T + b).reshape(B, L, 3, heads, d).permute(2, 0, 3, 1, 4)  # '(n H C)'
        att = ac._attention(qkv[0], qkv[1], qkv[2], 1.0 / math.sqrt(d), mask, 1e-5, None, dtype)
        return att.transpose(1, 2).reshape(B, L, Cc) @ wy.T

    ref = forward(torch.float64)
    e32 = (forward(torch.float32).double() - ref).abs().max().item()
    got = msa.cuda().eval()(x.cuda(), None, mask.cuda()).double().cpu()
    err, sc = (got - ref).abs().max().item(), max(1.0, ref.abs().max().item())
    print(f"ATTN padded heads {d}->{dp} {mask_kind}: err {err:.3e} e32 {e32:.3e} scale {sc:.2f}")
    assert got.shape == ref.shape and err <= 2e-5 * sc, (err, sc)
