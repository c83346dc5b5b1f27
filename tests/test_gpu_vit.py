r"""Attention kernel + ViT/DiT backbone parity on the GPU (oracle / reference golden vectors)."""

import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import max_err
from oracle import nets, sampling, synth

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


ATTN_SHAPES = [(2, 4, 16, 16), (1, 2, 64, 32), (2, 3, 256, 64), (1, 2, 100, 64), (1, 1, 1024, 64), (1, 2, 40, 128), (2, 2, 72, 80)]
ATTN_LAYOUTS = [("nHC", True), ("nHC", False), ("H3C", False), ("3HC", False)]
# f16x2 mode with un-normalised q / k at a head size the x3 / f16x2 kernels serve: the engine routes these to az_attention_x3_f32
# (test_attention_kernel_unnormalised_keys); every other combination keeps its entry
ATTN_CASES = [pytest.param(B, H, T, D, order, rms, x3, id=f"{x3}-{order}-{rms}-{B}-{H}-{T}-{D}")
              for x3 in (True, False, "f16x2") for order, rms in ATTN_LAYOUTS for B, H, T, D in ATTN_SHAPES
              if not (x3 == "f16x2" and not rms and D <= 80)]


@pytest.mark.parametrize("B,H,T,D,order,rms,x3", ATTN_CASES)
def test_attention_kernel(monkeypatch, B, H, T, D, order, rms, x3):
    """az_attention_x3_f32 (the contractions as 3 x bf16 pieces / 6 partial products on the bf16 MFMA), az_attention_f16x2_f32
    (2 x f16 pieces / 3 partial products on the f16 MFMA) and az_attention_f32 (fp32 MFMA), all against torch's SDPA at the same bound.
    Scores here are O(1): moving maxima, masks across tiles and the 8-wave form live in test_gpu_attention.py."""
    from azula_amd import engine
    from azula_amd.engine import Act, Builder

    monkeypatch.setattr(engine, "ATTN_X3", bool(x3))
    monkeypatch.setattr(engine, "FP32_MFMA", "f16x2" if x3 == "f16x2" else "bf16x3")
    xname = "az_attention_f16x2_f32" if x3 == "f16x2" else "az_attention_x3_f32"

    g = torch.Generator().manual_seed(B * T + D)
    q, k, v = (torch.randn(B, H, T, D, generator=g) for _ in range(3))
    if order in ("nHC", "3HC"):
        qkv = torch.stack((q, k, v), dim=0).permute(1, 3, 0, 2, 4).reshape(B, T, 3 * H * D)  # (n H C)
    else:
        qkv = torch.stack((q, k, v), dim=2).permute(0, 3, 1, 2, 4).reshape(B, T, 3 * H * D)  # (H 3 C)
    qn, kn = (F.rms_norm(q, (D,), eps=1e-5), F.rms_norm(k, (D,), eps=1e-5)) if rms else (q, k)
    ref = F.scaled_dot_product_attention(qn, kn, v)  # default scale 1/sqrt(D)
    ref = ref.transpose(1, 2).reshape(B, T, H * D)
    bld = Builder(torch.device("cuda"))
    act = Act(qkv.cuda().contiguous().reshape(-1), B, T, 1, 3 * H * D, 3 * H * D, True)
    act.bounded = True  # (a projection of normalised tokens: what the f16x2 form is chosen for)
    out = bld.attention(act, H, order, rms, 1.0 / math.sqrt(D))
    assert [n for _, _, n in bld.tape.ops] == [xname if x3 and D <= 80 else "az_attention_f32"]
    if x3 and D > 80:  # the engine keeps head_dim 128 on the fp32 kernel (faster there); the entry point itself takes it
        from azula_amd import _lib

        _, args, _ = bld.tape.ops[0]
        bld.tape.ops[0] = (getattr(_lib.lib(), xname), args, xname)
    bld.tape.run()
    got = out.buf.reshape(B, T, H * D)
    assert max_err(got, ref) < 2e-5, max_err(got, ref)


@pytest.mark.parametrize("B,H,T,D", [s for s in ATTN_SHAPES if s[3] <= 80])
@pytest.mark.parametrize("order", ["nHC", "H3C", "3HC"])
def test_attention_kernel_unnormalised_keys(monkeypatch, B, H, T, D, order):
    """f16x2 mode, q / k without RMS norm (ADM, ViT(qk_norm=False)): the engine takes az_attention_x3_f32, whose domain is all of
    fp32, even for a bounded q | k | v tensor -- un-normalised keys reach the f16x2 form's |k| < 4094.  Both entries on the same
    data against torch's SDPA: the x3 entry the plan holds, and the f16x2 entry itself (its arithmetic inside its domain)."""
    from azula_amd import _lib, engine
    from azula_amd.engine import Act, Builder

    monkeypatch.setattr(engine, "ATTN_X3", True)
    monkeypatch.setattr(engine, "FP32_MFMA", "f16x2")
    g = torch.Generator().manual_seed(B * T + D)
    q, k, v = (torch.randn(B, H, T, D, generator=g) for _ in range(3))
    if order in ("nHC", "3HC"):
        qkv = torch.stack((q, k, v), dim=0).permute(1, 3, 0, 2, 4).reshape(B, T, 3 * H * D)  # (n H C)
    else:
        qkv = torch.stack((q, k, v), dim=2).permute(0, 3, 1, 2, 4).reshape(B, T, 3 * H * D)  # (H 3 C)
    ref = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B, T, H * D)
    for name in ("az_attention_x3_f32", "az_attention_f16x2_f32"):
        bld = Builder(torch.device("cuda"))
        act = Act(qkv.cuda().contiguous().reshape(-1), B, T, 1, 3 * H * D, 3 * H * D, True)
        act.bounded = True
        out = bld.attention(act, H, order, False, 1.0 / math.sqrt(D))
        assert [n for _, _, n in bld.tape.ops] == ["az_attention_x3_f32"]
        bld.tape.ops[0] = (getattr(_lib.lib(), name), bld.tape.ops[0][1], name)
        bld.tape.run()
        got = out.buf.reshape(B, T, H * D)
        assert max_err(got, ref) < 2e-5, (name, max_err(got, ref))


@pytest.mark.parametrize("B,H,T,D", [(2, 4, 48, 32), (2, 3, 288, 64), (1, 2, 100, 128), (3, 12, 64, 64)])
@pytest.mark.parametrize("rms,gains,rope", [(True, False, False), (True, True, True), (False, False, True)])
@pytest.mark.parametrize("half", [None, torch.bfloat16])
def test_qk_preparation_in_the_projection_epilogue(B, H, T, D, rms, gains, rope, half):
    """AzConvArgs.act = 5: the fused q | k | v projection's epilogue applies the q / k RMS norm, the learned gains and RoPE
    once per layer (azula/nn/attention.py:92-95); the attention kernel then takes q and k as they are.  Checked against
    torch (linear -> rms_norm -> gain -> rotate -> SDPA) and against the in-kernel path (AZ_QK_PREP off)."""
    from azula_amd import engine
    from azula_amd.engine import Act, Builder

    Cin, HC = 64, H * D
    g = torch.Generator().manual_seed(B * T + D + H)
    x = torch.randn(B, T, Cin, generator=g)
    w = torch.randn(3 * HC, Cin, generator=g) / math.sqrt(Cin)
    bias = torch.randn(3 * HC, generator=g) * 0.1
    qw, kw = (1 + 0.2 * torch.randn(D, generator=g) for _ in range(2))
    theta = torch.randn(T, H * D // 2, generator=g) * 2
    qkv = F.linear(x, w, bias)
    q, k, v = (t.reshape(B, T, H, D).transpose(1, 2) for t in qkv.chunk(3, dim=-1))
    if rms:
        q, k = F.rms_norm(q, (D,), eps=1e-6), F.rms_norm(k, (D,), eps=1e-6)
    if gains:
        q, k = q * qw, k * kw
    if rope:
        cs, sn = (f(theta).reshape(T, H, D // 2).transpose(0, 1) for f in (torch.cos, torch.sin))

        def rot(t):
            re, im = t[..., 0::2], t[..., 1::2]
            return torch.stack((re * cs - im * sn, re * sn + im * cs), dim=-1).flatten(-2)

        q, k = rot(q), rot(k)
    ref = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B, T, HC)
    outs = {}
    for mode in (True, False):
        engine.QK_PREP = mode
        try:
            bld = Builder(torch.device("cuda"))
            bld.half = half
            xa = Act(x.cuda().reshape(-1), B, T, 1, Cin, Cin, True)
            tabs = (bld.const(torch.cos(theta)), bld.const(torch.sin(theta))) if rope else None
            gw = (bld.const(qw), bld.const(kw)) if gains else None
            prep = dict(heads=H, head_dim=D, rmsnorm=rms, eps=1e-6, rope=tabs, weight=gw)
            y = bld.conv(xa, bld.pack_conv(w.cuda(), bias.cuda()), 3 * HC, qk_prep=prep)
            assert y.qk_prepared == mode and bld.tape.keep and (bld.tape.ops[-1][1][0]._obj.act == (5 if mode else 0))
            out = bld.attention(y, H, "3HC", rms, 1.0 / math.sqrt(D), eps=1e-6, rope=tabs, qk_weight=gw)
            bld.finish()
            bld.tape.run()
            outs[mode] = out.buf.reshape(B, T, HC).clone()
        finally:
            engine.QK_PREP = True
    tol = 3e-5 if half is None else 3e-2
    e_ref, e_ab = max_err(outs[True], ref), max_err(outs[True], outs[False])
    assert e_ref < tol and e_ab < tol, (e_ref, e_ab)


ATTN_FORMS = ("az_attention_f16x2_f32", "az_attention_x3_f32", "az_attention_f32")
ATTN_H2_K_LIMIT = 4094.0  # include/azula_amd.h: |k| < 4094, |v| and |q * scale * log2 e| < 1.0e6 for az_attention_f16x2_f32
ATTN_H2_V_LIMIT = 65520.0 * 16  # (the values enter as two half pieces of v / 2^4)
ATTN_H2_QS_LIMIT = 1.0e6


def _attention_cases(case, B, H, T, D, g):
    r"""(q, k, v, mask, the (B, H, T, D) outputs that must turn NaN in the f16x2 form or None) for one magnitude case; fp64 tensors."""
    q, k, v = (torch.randn(B, H, T, D, generator=g, dtype=torch.float64) for _ in range(3))
    mask, bad = None, None
    scale = 1.0 / math.sqrt(D)
    if case in ("k_in", "k_out"):  # one key element at 0.95 / 1.05 x the limit, the rest of its row O(1), queries small
        k[0, 1, 5, 3] = (0.95 if case == "k_in" else 1.05) * ATTN_H2_K_LIMIT
        q *= 1e-3
        if case == "k_out":  # every query of head (0, 1) reads that key: all its outputs
            bad = torch.zeros(B, H, T, D, dtype=torch.bool)
            bad[0, 1] = True
    elif case in ("v_half", "v_in", "v_out"):  # values near the limit in one row (v_half: the whole tensor at 0.5 x)
        if case == "v_half":
            v = torch.sign(v) * (0.5 * ATTN_H2_V_LIMIT)
        else:
            v[0, 0, 7, 2] = (0.95 if case == "v_in" else 1.05) * ATTN_H2_V_LIMIT
        if case == "v_out":  # channel 2 of every output of head (0, 0)
            bad = torch.zeros(B, H, T, D, dtype=torch.bool)
            bad[0, 0, :, 2] = True
    elif case in ("qs_in", "qs_out"):  # one query channel at the limit of q * scale * log2 e, whose key channel is zero: scores unchanged
        q[1, 0, 9, 4] = (0.95 if case == "qs_in" else 1.05) * ATTN_H2_QS_LIMIT / (scale * math.log2(math.e))
        k[:, :, :, 4] = 0.0
        if case == "qs_out":  # that query's row
            bad = torch.zeros(B, H, T, D, dtype=torch.bool)
            bad[1, 0, 9] = True
    elif case == "one_hot":  # scores along one channel whose keys are s / T: consecutive scores 100 apart, so every row is one-hot
        k[:, :, :, 0] = torch.arange(T, dtype=torch.float64) / T  # (on the last key for q > 0, on the first for q < 0)
        q.zero_()
        q[:, :, :, 0] = torch.where(torch.rand(B, H, T, generator=g) < 0.5, -1.0, 1.0).double() * (101.0 * T / scale)
        k[:, :, :, 1:] = 0.0
    elif case == "near_tie":  # pairs of keys that differ by 1e-6: two scores per row within 1e-6, sharp rows
        k[:, :, 1::2] = k[:, :, 0::2][:, :, : T // 2] + 1e-6 * torch.randn(B, H, T // 2, D, generator=g, dtype=torch.float64)
        q = q * 4.0
    elif case == "masked_tiles":  # keys 0 .. 63 (a whole key tile) and the ragged last tile masked out for every query
        mask = torch.rand(T, T, generator=g) < 0.7
        mask[:, :64] = False
        mask[:, 64 * (T // 64):] = False
        mask[:, 64] = True  # (every query keeps a key: an all-masked row is NaN in the reference too)
    return q, k, v, mask, bad


@pytest.mark.parametrize("D", [16, 32, 64, 80])
@pytest.mark.parametrize("case", ["k_in", "k_out", "v_half", "v_in", "v_out", "qs_in", "qs_out", "one_hot", "near_tie", "masked_tiles"])
def test_attention_magnitudes(monkeypatch, case, D):
    """The three fp32 attention forms on the same data at the f16x2 form's stated limits (include/azula_amd.h), T = 141 (not a
    multiple of a tile), against fp64 SDPA: inside a limit every form within 2e-5 of max |v|; outside it the f16x2 form turns
    exactly the outputs that read the offending value into NaN and keeps the others, while the x3 and fp32 forms (whose domain is all
    of fp32) stay correct; saturated (one-hot) and near-tie softmax rows and fully masked key tiles in every form."""
    from azula_amd import _lib, engine
    from azula_amd.engine import Act, Builder

    monkeypatch.setattr(engine, "FP32_MFMA", "f16x2")
    B, H, T = 2, 2, 141
    g = torch.Generator().manual_seed(D * 31 + len(case))
    q, k, v, mask, bad = _attention_cases(case, B, H, T, D, g)
    ref = F.scaled_dot_product_attention(q, k, v, attn_mask=mask)  # fp64, scale 1 / sqrt(D)
    qkv = torch.stack((q, k, v), dim=0).permute(1, 3, 0, 2, 4).reshape(B, T, 3 * H * D).float()  # (n H C)
    for name in ATTN_FORMS:
        bld = Builder(torch.device("cuda"))
        act = Act(qkv.cuda().contiguous().reshape(-1), B, T, 1, 3 * H * D, 3 * H * D, True)
        act.bounded = True
        out = bld.attention(act, H, "nHC", False, 1.0 / math.sqrt(D), mask=mask)
        assert bld.tape.ops[0][2] == "az_attention_x3_f32"  # (un-normalised keys: never the f16x2 form by choice)
        bld.tape.ops[0] = (getattr(_lib.lib(), name), bld.tape.ops[0][1], name)
        bld.tape.run()
        got = out.buf.reshape(B, T, H, D).permute(0, 2, 1, 3).double().cpu()
        ok = torch.ones(B, H, T, D, dtype=torch.bool) if bad is None or name != ATTN_FORMS[0] else ~bad
        if bad is not None and name == ATTN_FORMS[0]:
            assert torch.isnan(got[bad]).all(), (name, case)
        assert torch.isfinite(got[ok]).all(), (name, case)
        err, sc = (got[ok] - ref[ok]).abs().max().item(), v.abs().max().item()
        print(name, case, D, "error / max|v|", err / sc)
        assert err <= 2e-5 * sc, (name, case, err, sc)


def test_attention_routing_by_qk_normalisation(monkeypatch):
    """engine: the f16x2 attention form only for RMS-normalised q / k whose gains keep sqrt(d) max |g| inside its key limit
    (un-normalised keys: ADM, ViT(qk_norm=False) -> the x3 form, whose domain is all of fp32)."""
    from azula_amd import engine
    from azula_amd.engine import Act, Builder

    monkeypatch.setattr(engine, "FP32_MFMA", "f16x2")
    B, H, T, D = 1, 2, 32, 64
    qkv = torch.zeros(B * T * 3 * H * D, device="cuda")
    ones = torch.ones(D, device="cuda")
    for rms, gains, name in ((True, None, "az_attention_f16x2_f32"), (False, None, "az_attention_x3_f32"),
                             (True, (ones, ones * 100), "az_attention_f16x2_f32"), (True, (ones, ones * 1000), "az_attention_x3_f32")):
        bld = Builder(torch.device("cuda"))
        act = Act(qkv, B, T, 1, 3 * H * D, 3 * H * D, True)
        act.bounded = True
        bld.attention(act, H, "nHC", rms, 1.0 / math.sqrt(D), qk_weight=gains)
        assert bld.tape.ops[0][2] == name, (rms, gains is not None and gains[1][0].item())


def test_attention_spiked_scores():
    """Online-softmax rescale path: one key dominates from a late tile (guide rule 26)."""
    from azula_amd.engine import Act, Builder

    g = torch.Generator().manual_seed(0)
    B, H, T, D = 1, 1, 256, 64
    q, k, v = (torch.randn(B, H, T, D, generator=g) for _ in range(3))
    k[0, 0, 200] = 6.0 * q[0, 0, 3]  # spike in the 4th key tile for query 3
    qkv = torch.stack((q, k, v), dim=0).permute(1, 3, 0, 2, 4).reshape(B, T, 3 * D)
    ref = F.scaled_dot_product_attention(q.double(), k.double(), v.double()).float().transpose(1, 2).reshape(B, T, D)
    bld = Builder(torch.device("cuda"))
    out = bld.attention(Act(qkv.cuda().contiguous().reshape(-1), B, T, 1, 3 * D, 3 * D, True), 1, "nHC", False, 1 / 8.0)
    bld.tape.run()
    assert max_err(out.buf.reshape(B, T, D), ref) < 2e-5


def test_patchify_roundtrip():
    from azula_amd import _lib

    x = torch.randn(2, 3, 8, 12, device="cuda")
    p, cs = 2, 12
    tok = torch.empty(2, 4 * 6, cs, device="cuda")
    _lib.call("az_patchify_f32", tok.data_ptr(), x.data_ptr(), None, 2, 3, 8, 12, p, cs, _lib.stream_ptr())
    ref = x.reshape(2, 3, 4, p, 6, p).permute(0, 2, 4, 1, 3, 5).reshape(2, 24, 12)
    assert torch.equal(tok, ref)
    back = torch.empty_like(x)
    _lib.call("az_unpatchify_f32", back.data_ptr(), tok.data_ptr(), 2, 3, 8, 12, p, cs, _lib.stream_ptr())
    assert torch.equal(back, x)


def build_vit(cfg):
    from azula_amd.nn import ViT

    return ViT(
        cfg["in_channels"], cfg["out_channels"], hid_channels=cfg["hid_channels"], hid_blocks=cfg["hid_blocks"],
        attention_heads=cfg["attention_heads"], patch_size=cfg["patch_size"], mod_features=cfg["mod_features"],
    )


def test_vit_forward_matches_reference(golden):
    g = golden("g5_vit")
    cfg = g.meta["cfg"]
    net = build_vit(cfg)
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == {k: tuple(v) for k, v in g.meta["shapes"].items()}
    net.load_state_dict(synth.synth_state_dict({k: tuple(v) for k, v in g.meta["shapes"].items()}, g.meta["weight_seed"]))
    net = net.cuda().eval()
    x = g["x"].cuda()
    for tag in ("modB", "mod1"):
        y = net(x, g[tag].cuda())
        err, sc = max_err(y, g["y_" + tag]), g["y_" + tag].abs().max().item()
        print("vit", tag, "max|d|", err, "scale", sc)
        assert err < 1e-4 * max(1.0, sc)


@pytest.mark.parametrize("mode,entry", [("bf16x3", "az_conv2d_x3_f32"), ("f16x2", "az_conv2d_f16x2_f32")])
def test_vit_ddim50_through_bf16x3(golden, monkeypatch, mode, entry):
    """DDIM-50 of the golden ViT with every token GEMM on the bf16 MFMA as 3 x bf16 pieces / 6 partial products
    (AZ_FP32_MFMA=bf16x3) or on the f16 MFMA as 2 x f16 pieces / 3 partial products (f16x2): same tolerance as the native fp32 run
    (hid_channels = 64 >= 32, so the GEMMs qualify)."""
    from azula_amd import engine
    from azula_amd.denoise import KarrasDenoiser
    from azula_amd.nn import TimeModulated
    from azula_amd.noise import VPSchedule
    from azula_amd.sample import DDIMSampler

    monkeypatch.setattr(engine, "FP32_MFMA", mode)
    g = golden("g6_vit_loop")
    cfg = g.meta["cfg"]
    w = TimeModulated(build_vit(cfg), cfg["mod_features"], name="vit")
    w.load_state_dict(synth.synth_state_dict({k: tuple(v) for k, v in g.meta["shapes"].items()}, g.meta["weight_seed"]))
    den = KarrasDenoiser(w, VPSchedule()).cuda().eval()
    smp = DDIMSampler(den, steps=50, silent=True)
    x0 = smp(g["x1"].cuda())
    loop = next(iter(smp._fused_cache.values()))
    assert any(name_ == entry for _, _, name_ in loop.tape.ops)
    err, sc = max_err(x0, g["ddim50"]), g["ddim50"].abs().max().item()
    print("ViT DDIM-50", mode, "max|d| vs reference:", err, "scale", sc)
    assert err < 5e-4 * max(1.0, sc)


def test_dit_token_forward_matches_oracle(golden):
    from azula_amd.nn import DiT

    g = golden("g5_vit")
    shapes = {k: tuple(v) for k, v in g.meta["shapes"].items()}
    shapes["pos_embedding.2.weight"] = (64, 64)  # pos_channels = 1 for the plain DiT
    sd = synth.synth_state_dict(shapes, 17)
    net = DiT(16, 16, mod_features=32, hid_channels=64, hid_blocks=2, attention_heads=4)
    net.load_state_dict(sd)
    net = net.cuda().eval()
    gen = torch.Generator().manual_seed(5)
    x, mod = torch.randn(2, 24, 16, generator=gen), torch.randn(2, 32, generator=gen)
    ref = nets.dit_forward(sd, dict(hid_channels=64, hid_blocks=2, attention_heads=4), x, mod)
    y = net(x.cuda(), mod.cuda())
    assert max_err(y, ref) < 1e-4 * max(1.0, ref.abs().max().item())


def test_vit_ddim50_fused_matches_reference(golden):
    from azula_amd.denoise import KarrasDenoiser
    from azula_amd.nn import TimeModulated
    from azula_amd.noise import VPSchedule
    from azula_amd.sample import DDIMSampler

    g = golden("g6_vit_loop")
    cfg = g.meta["cfg"]
    w = TimeModulated(build_vit(cfg), cfg["mod_features"], name="vit")
    w.load_state_dict(synth.synth_state_dict({k: tuple(v) for k, v in g.meta["shapes"].items()}, g.meta["weight_seed"]))
    den = KarrasDenoiser(w, VPSchedule()).cuda().eval()
    smp = DDIMSampler(den, steps=50, silent=True)
    x0 = smp(g["x1"].cuda())
    assert next(iter(smp._fused_cache.values())).graph is not None
    err, sc = max_err(x0, g["ddim50"]), g["ddim50"].abs().max().item()
    print("ViT DDIM-50 fused max|d| vs reference:", err, "scale", sc)
    assert err < 5e-4 * max(1.0, sc)


@pytest.mark.parametrize("name", ["vit_rope_swiglu", "vit_relu2_noqknorm", "vit_relu", "g24_vit_hd48_rope", "g24_vit_hd96_noqknorm", "g24_vit_hd24"])
def test_vit_variants_match_reference(golden, name):
    """RoPE (attention.py:112-156), SwiGLU / ReLU^2 / ReLU FFNs (layers.py:71-110), qk_norm=False; G24: head sizes 48 (RoPE +
    q/k norm), 96 and 24 -- run zero-padded to 64 / 128 / 32 (engine.ATTN_HEAD_DIMS; azula/nn/attention.py:35-51 takes any)."""
    from azula_amd.nn import ViT

    g = golden(name if name.startswith("g24_") else "g5_" + name)
    cfg = g.meta["cfg"]
    extra = {k: cfg[k] for k in ("rope", "ffn_activation", "qk_norm") if k in cfg}
    net = ViT(cfg["in_channels"], cfg["out_channels"], hid_channels=cfg["hid_channels"], hid_blocks=cfg["hid_blocks"],
              attention_heads=cfg["attention_heads"], patch_size=cfg["patch_size"], mod_features=cfg["mod_features"], **extra)
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == {k: tuple(v) for k, v in g.meta["shapes"].items()}
    net.load_state_dict(synth.synth_state_dict({k: tuple(v) for k, v in g.meta["shapes"].items()}, g.meta["weight_seed"]))
    net = net.cuda().eval()
    y = net(g["x"].cuda(), g["modB"].cuda())
    err, sc = max_err(y, g["y_modB"]), g["y_modB"].abs().max().item()
    print(name, "max|d|", err, "scale", sc)
    assert err < 1e-4 * max(1.0, sc)
    if name.startswith("g24_"):
        ops = [a for _, a, n in next(iter(net._plans.values())).tape.ops if n.startswith("az_attention")]
        hd = cfg["hid_channels"] // cfg["attention_heads"]
        assert ops and all(a[0]._obj.norm_dim == hd and a[0]._obj.head_dim > hd for a in ops)  # (padded heads, norm over the real size)
