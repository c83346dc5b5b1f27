r"""The kernel choice (engine.choose_conv / choose_attention) and the builder's content facts, on the host.

The expected entries of the tables were read off one-layer Builder plans of the code before the choice became a function of
its own: the choice moved, it did not change."""

import pytest
import torch

from azula_amd import engine
from azula_amd.engine import Builder, ConvLayer, ConvSource, choose_attention, choose_conv, pad4

HEAD = dict(B=4, H=256, W=256, cin=256, cout=256, ks=3)  # the headline 3 x 3, 256 -> 256 layer at 4 x 256^2
SKIP = dict(B=4, H=64, W=64, cin=768, cout=256, ks=1)  # an ADM-sized 1 x 1 skip projection
WINO, WX3, WH2 = "az_conv2d_winograd_f32", "az_conv2d_winograd_x3_f32", "az_conv2d_winograd_f16x2_f32"
X3, H2, F32 = "az_conv2d_x3_f32", "az_conv2d_f16x2_f32", "az_conv2d_f32"

CONV_TABLE = [  # (row, switches, layer, entry, dynamic scale)
    ("headline_f16x2_bounded", {}, dict(HEAD, bounded=True), WH2, False),
    ("headline_f16x2_unbounded", {}, dict(HEAD), WH2, True),
    ("headline_bf16x3_bounded", dict(FP32_MFMA="bf16x3"), dict(HEAD, bounded=True), WX3, False),
    ("headline_bf16x3_unbounded", dict(FP32_MFMA="bf16x3"), dict(HEAD), WX3, False),
    ("headline_native_bounded", dict(FP32_MFMA="native"), dict(HEAD, bounded=True), WINO, False),
    ("headline_native_unbounded", dict(FP32_MFMA="native"), dict(HEAD), WINO, False),
    ("headline_unbounded_no_dynamic", dict(F16X2_DYNAMIC=False), dict(HEAD), WX3, False),
    ("skip_1x1_moments", {}, dict(SKIP, moments=True), H2, True),
    ("skip_1x1_no_moments", {}, dict(SKIP), X3, False),
    ("skip_1x1_moments_switch_off", dict(F16X2_MOMENTS=False), dict(SKIP, moments=True), X3, False),
    ("stride2_unbounded", {}, dict(HEAD, stride=2), H2, True),
    ("stride2_bounded_bf16x3", dict(FP32_MFMA="bf16x3"), dict(HEAD, stride=2, bounded=True), X3, False),
    ("small_map_b1", {}, dict(B=1, H=8, W=8, cin=256, cout=256, ks=3, bounded=True), H2, False),
    ("small_map_b1_native", dict(FP32_MFMA="native"), dict(B=1, H=8, W=8, cin=256, cout=256, ks=3, bounded=True), F32, False),
    ("image_head", {}, dict(HEAD, cout=3, bounded=True), F32, False),
    ("bf16_module", {}, dict(B=4, H=64, W=64, cin=256, cout=256, ks=3, half=torch.bfloat16), "az_conv2d_bf16_f32", False),
    ("f16_module", {}, dict(B=4, H=64, W=64, cin=256, cout=256, ks=3, half=torch.float16), "az_conv2d_f16_f32", False),
    ("depth_tap", {}, dict(B=4, H=64, W=64, cin=256, cout=256, ks=3, depth=True), WX3, False),
    ("winograd4", dict(WINOGRAD="4"), dict(HEAD, bounded=True), "az_conv2d_winograd4_f32", False),
    ("winograd4_few_tiles", dict(WINOGRAD="4"), dict(B=1, H=32, W=32, cin=256, cout=256, ks=3, bounded=True), WH2, False),
    ("below_x3_min_channels", {}, dict(B=4, H=64, W=64, cin=16, cout=16, ks=1, bounded=True), F32, False),
    ("override_x3", {}, dict(HEAD, winograd="x3"), X3, False),
    ("override_wh2", {}, dict(HEAD, winograd="wh2"), WH2, False),
    ("override_h2d", {}, dict(HEAD, winograd="h2d"), H2, True),
    ("override_false", {}, dict(HEAD, winograd=False), F32, False),
    ("override_false_bounded", {}, dict(HEAD, winograd=False, bounded=True), F32, False),
    ("two_sources_one_unbounded", {}, dict(B=4, H=64, W=64, cin=512, cin1=256, cout=256, ks=3, bounded=True), WX3, False),
    # conv-over-conv sources (a convolution's / attention's output is never bounded: Act.bounded): the UNet FFN's second 3 x 3
    # convolution over SiLU(conv), whose producer left moments; the same without them on a small map; a DiT-B/2 token GEMM
    # behind attention / an FFN at batch 64 (16384 tokens: the measured pass pays) and at batch 2 (it does not)
    ("ffn_second_conv_moments", {}, dict(HEAD, moments=True), WH2, True),
    ("ffn_second_conv_moments_bf16x3", dict(FP32_MFMA="bf16x3"), dict(HEAD, moments=True), WX3, False),
    ("conv_over_conv_small_map", {}, dict(B=1, H=16, W=16, cin=64, cout=64, ks=3), WX3, False),
    ("token_gemm_after_attention", {}, dict(B=64, H=256, W=1, cin=768, cout=768, ks=1), H2, True),
    ("token_gemm_after_attention_b2", {}, dict(B=2, H=256, W=1, cin=768, cout=768, ks=1), X3, False),
    # weights whose rows span more than 2^16 (ConvWeights.h2_range): bf16x3, bounded source or not
    ("weight_range_bounded", {}, dict(HEAD, bounded=True, w_h2=False), WX3, False),
    ("weight_range_unbounded", {}, dict(SKIP, moments=True, w_h2=False), X3, False),
]

ATTN_TABLE = [  # (switches, head size, q / k normalised within the f16x2 key limit, half, entry)
    *[({}, 64, b, None, "az_attention_f16x2_f32" if b else "az_attention_x3_f32") for b in (True, False)],
    *[(dict(FP32_MFMA="bf16x3"), 64, b, None, "az_attention_x3_f32") for b in (True, False)],
    *[(dict(FP32_MFMA=m), 128, b, None, "az_attention_f32") for m in ("f16x2", "bf16x3", "native") for b in (True, False)],
    *[(dict(FP32_MFMA="native"), 64, b, None, "az_attention_f32") for b in (True, False)],
    ({}, 64, True, torch.bfloat16, "az_attention_bf16_f32"),
    ({}, 64, True, torch.float16, "az_attention_f16_f32"),
]

DEFAULTS = dict(FP32_MFMA="f16x2", F16X2_DYNAMIC=True, F16X2_MOMENTS=True, WINOGRAD="1", WINO_X3=True, ATTN_X3=True, ATTN_H2=True,
                WINOGRAD4_MIN_TILES=1024, X3_MIN_CHANNELS=32)


def switches(monkeypatch, env):
    for k, v in {**DEFAULTS, **env}.items():
        monkeypatch.setattr(engine, k, v)


def source(B, H, W, C, bounded=False, affine=False, moments=False):
    return ConvSource(C, B * H * W * pad4(C), bounded, affine, False, moments)


def layer(B, H, W, cin, cout, ks, stride=1, cin1=0, bounded=False, moments=False, depth=False, winograd=None, half=None, affine=False,
          w_h2=True):
    hout, wout = (H + 2 * (ks // 2) - ks) // stride + 1, (W + 2 * (ks // 2) - ks) // stride + 1
    return ConvLayer(ks, stride, False, B, hout, wout, pad4(cin), pad4(cin1), cout, pad4(cout), 0, depth, half, winograd,
                     source(B, H, W, cin, bounded, affine, moments), source(B, H, W, cin1) if cin1 else None, w_h2)


@pytest.mark.parametrize("row, env, spec, name, dyn", CONV_TABLE, ids=[r[0] for r in CONV_TABLE])
def test_choose_conv(monkeypatch, row, env, spec, name, dyn):
    switches(monkeypatch, env)
    ch = choose_conv(layer(**spec))
    assert (ch.name, ch.dyn) == (name, dyn)
    assert ch.h2 == (name in engine.H2_NAMES)


@pytest.mark.parametrize("env, dim, qk_normed, half, name", ATTN_TABLE)
def test_choose_attention(monkeypatch, env, dim, qk_normed, half, name):
    switches(monkeypatch, env)
    assert choose_attention(dim, qk_normed, half) == name


def qkv_act(bld, B=1, T=32, H=2, D=64):
    a = bld.new_act(B, T, 1, 3 * H * D)
    return bld.wrote(a, bounded=True)  # (even a bounded projection: the routing reads q / k normalisation, not Act.bounded)


@pytest.mark.parametrize("rms, gk, gq, name", [
    (True, None, None, "az_attention_f16x2_f32"),  # azula ViT / DiT with qk_norm: |k| <= sqrt(64) = 8
    (False, None, None, "az_attention_x3_f32"),  # ADM, ViT(qk_norm=False): un-normalised keys
    (True, 200.0, 1.0, "az_attention_f16x2_f32"),  # 8 x 200 = 1600 < 4094 / 2
    (True, 300.0, 1.0, "az_attention_x3_f32"),  # 8 x 300 = 2400: inside 4094 but not with the factor 2 to spare
    (True, 1.0, 1e6, "az_attention_x3_f32"),  # |q * scale * log2 e| up to 8 x 1e6 / 8 x 1.44 > 1e6 / 2
])
def test_attention_routing_reads_the_qk_normalisation(bld, rms, gk, gq, name):
    D = 64
    qk_weight = None if gk is None else (torch.full((D,), gq), torch.full((D,), -gk))
    out = bld.attention(qkv_act(bld, D=D), 2, "nHC", rms, 1.0 / D ** 0.5, qk_weight=qk_weight)
    assert ops(bld) == [name]
    assert not out.bounded  # (attention output: a convex combination of values as large as the weights make them)


def test_weight_range_of_the_f16x2_packing(bld):
    w = torch.randn(8, 4, 3, 3)
    assert bld.pack_conv(w, None).h2_range()
    w[3] *= 1e-6  # (one row ~1e6 below the rest: beyond 2^16)
    assert not bld.pack_conv(w, None).h2_range()
    w[3] = 0.0  # rows of exact zeros (zero-padded heads) are exact in any packing
    assert bld.pack_conv(w, None).h2_range()


def test_qk_bound_of_padded_heads(bld):
    r"""Zero-padded heads (ATTN_HEAD_DIMS): the RMS norm averages over the real size, so that is the sqrt(n) of the bound."""
    kmax, qsmax = engine.attention_qk_bound(64, 48, 48 ** -0.5, None)
    assert kmax == pytest.approx(48 ** 0.5) and qsmax == pytest.approx(1.4426950408889634)


def test_choice_reads_the_switches_at_call_time(monkeypatch):
    switches(monkeypatch, {})
    spec = layer(**HEAD, bounded=True)
    assert choose_conv(spec).name == WH2
    monkeypatch.setattr(engine, "FP32_MFMA", "native")  # (bench.py flips it between plans)
    assert choose_conv(spec).name == WINO


def test_a_recorded_maximum_makes_the_dynamic_scale_cheaper(monkeypatch):
    switches(monkeypatch, {})
    spec = layer(**SKIP)
    assert not choose_conv(spec).dyn  # a pass over the 768-channel source costs more than it saves
    assert choose_conv(spec._replace(src0=spec.src0._replace(absmax=True))).dyn  # already measured for another consumer


def test_no_dynamic_scale_on_a_pending_normalisation(monkeypatch):
    r"""A lazily normalised source (Act.affine) beside an unbounded one: its stored tensor is not what the kernel sees, so
    its maximum is no scale; the choice falls back to the bf16x3 form instead of asking for one."""
    switches(monkeypatch, {})
    ch = choose_conv(layer(B=4, H=64, W=64, cin=512, cin1=512, cout=512, ks=3, affine=True))
    assert (ch.name, ch.dyn) == (WX3, False)
    assert not choose_conv(layer(B=4, H=64, W=64, cin=512, cout=512, ks=3, affine=True)).dyn  # (alone: bounded, fixed scale)


@pytest.mark.parametrize("bad", ["h3", "X3", 3, "auto"])
def test_unknown_override_raises(monkeypatch, bad):
    switches(monkeypatch, {})
    with pytest.raises(ValueError):
        choose_conv(layer(**HEAD, winograd=bad))


# -- content facts: a record of what an allocation held is stale after any later write to it -----------------------------------
def produced(bld, B=2, H=16, W=16, C=64, chunks=4):
    r"""An activation as a convolution with GroupNorm moments leaves it (the launch itself is not needed to record the facts)."""
    y = bld.new_act(B, H, W, C)
    return bld.wrote(y, bounded=False, moments=(bld.empty(B * chunks * (C // 4) * 4), chunks))


def ops(bld):
    return [n for _, _, n in bld.tape.ops]


@pytest.fixture
def bld(monkeypatch):
    switches(monkeypatch, {})
    monkeypatch.setattr(engine, "GN_FUSED", True)
    return Builder(torch.device("cpu"))


def test_facts_hold_until_the_allocation_is_written(bld):
    y = produced(bld)
    s = bld.absmax_of(y)
    assert bld.absmax_of(y) is s and ops(bld) == ["az_absmax_from_moments_f32"]  # shared by consumers, bounded from the moments
    bld.group_norm(y, 8)
    assert "az_groupnorm_stats_f32" not in ops(bld)  # the producer's moments: no statistics pass


@pytest.mark.parametrize("how", ["same view", "second view", "other planes"])
def test_a_write_through_any_view_invalidates_the_facts(bld, how):
    y = produced(bld)
    bld.absmax_of(y)
    n = y.H * y.W * y.cs
    other = {"same view": y, "second view": y.view(1, 2 * y.H), "other planes": y.view(1, buf=y.buf[n:])}[how]
    bld.wrote(other, bounded=False)  # (e.g. az_token_copy_f32 into the allocation)
    assert bld.fact(y, y.absmax) is None and bld.fact(y, y.gn_quads) is None
    del bld.tape.ops[:]
    bld.absmax_of(y)
    bld.group_norm(y, 8)
    assert ops(bld)[0] == "az_absmax_f32"  # measured again, over what the tensor holds now
    assert "az_groupnorm_stats_f32" in ops(bld)  # the statistics pass, not the stale moments


def test_a_view_carries_bounded_and_only_the_moments_it_is_given(bld):
    y = produced(bld)
    bld.wrote(y, bounded=True, moments=y.gn_quads[:2])
    v = y.view(1, 2 * y.H)
    assert v.bounded and v.gn_quads is None and v.absmax is None
    q = y.gn_quads
    v = y.view(1, 2 * y.H, gn_quads=(q[0], 2 * q[1], q[2]))  # (ADM's planes -> volume re-chunking)
    assert bld.fact(v, v.gn_quads) is not None
    assert not y.view(bounded=False).bounded


@pytest.mark.parametrize("half", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("C", [12, 100, 4104])
def test_row_norm_names_a_width_the_2_byte_kernel_refuses(half, C):
    """az_rownorm_mod_h16 takes C % 8 == 0, C == cs, C <= 4096 and answers AZ_E_UNSUPPORTED otherwise -- at run time, from inside
    a tape.  Builder.row_norm says so while the plan is built, with the width in the message; a width it takes goes on the tape."""
    b = Builder(torch.device("cpu"), half=half, half_act=True)
    with pytest.raises(ValueError, match=f"width {C} "):
        b.row_norm(b.new_act(2, 3, 1, C), 1)
    assert not b.tape.ops
    b.row_norm(b.new_act(2, 3, 1, 4096), 0)
    assert ops(b) == ["az_rownorm_mod_h16"]
