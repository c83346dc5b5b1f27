r"""``JiT.vjp`` / ``JITDenoiser._az_vjp`` / ``CFGDenoiser._az_vjp`` without a GPU: the scope errors, the argument codes of the new
C entries, and the input condition the GPU test of the CFG pullback on ADM relies on."""

import pytest
import torch

from azula_amd import _lib
from oracle import sampling, synth
from test_gpu_adm_vjp import backbone_fn

JIT_KW = dict(input_size=16, patch_size=4, hidden_size=32, depth=1, num_heads=2, num_classes=4, bottleneck_dim=8, in_context_len=2,
              in_context_start=0)


def test_scope_errors():
    from azula_amd.denoise import Denoiser
    from azula_amd.guidance import CFGDenoiser
    from azula_amd.plugins import jit

    x, t, y = torch.zeros(1, 3, 16, 16), torch.tensor([0.5]), torch.tensor([1])
    with pytest.raises(NotImplementedError, match="CPU tensors"):
        jit.JiT(**JIT_KW).vjp(x, t, y)
    with pytest.raises(NotImplementedError, match="half-precision"):
        jit.JiT(**JIT_KW).half().vjp(x.half(), t, y)
    with pytest.raises(NotImplementedError, match="half-precision"):
        jit.JiT(**JIT_KW).half().vjp(x, t, y)
    den = jit.JITDenoiser(jit.JiT(**JIT_KW), num_classes=4)
    with pytest.raises(NotImplementedError, match="device tensors"):
        den._az_vjp(x, torch.tensor(0.5))
    cfg = CFGDenoiser(den)
    with pytest.raises(NotImplementedError, match="CFG"):
        cfg._az_vjp(x, torch.tensor(0.5), positive={"label": y})  # CPU tensors
    with pytest.raises(NotImplementedError, match="CFG"):
        cfg._az_vjp(x, torch.tensor(0.5), positive={"label": y, "extra": 1})
    with pytest.raises(NotImplementedError, match="CFG"):
        cfg._az_vjp(x, torch.tensor(0.5))  # no `positive`

    class Plain(Denoiser):
        schedule = den.schedule

    with pytest.raises(NotImplementedError, match="CFG"):
        CFGDenoiser(Plain())._az_vjp(x, torch.tensor(0.5), positive={"label": y})


def test_new_entries_validate_their_arguments():
    from azula_amd.csrc import build

    build.build()
    lib = _lib.lib()
    P, Q = 0x1000, 0x1004  # aligned / misaligned addresses (never dereferenced: validation comes first)
    rn = lambda *a: lib.az_rownorm_bwd_w_f32(*a, None)  # noqa: E731
    #  dx x g res scale bstride weight rows rows_per_batch C cs kind eps
    assert rn(None, P, P, None, None, 0, P, 4, 4, 8, 8, 1, 1e-6) == -1
    assert rn(P, P, None, None, None, 0, P, 4, 4, 8, 8, 1, 1e-6) == -1
    assert rn(P, P, P, None, None, 0, P, 0, 4, 8, 8, 1, 1e-6) == -2  # rows == 0
    assert rn(P, P, P, None, None, 0, P, 4, 4, 8, 6, 1, 1e-6) == -2  # cs < C
    assert rn(P, P, P, None, None, 0, P, 4, 4, 6, 6, 1, 1e-6) == -2  # cs % 4
    assert rn(P, P, P, None, None, 0, P, 4, 4, 8, 8, 2, 1e-6) == -2  # kind
    assert rn(P, P, P, None, None, 0, P, 4, 4, 1, 4, 0, 1e-6) == -2  # unbiased variance of one channel
    assert rn(Q, P, P, None, None, 0, P, 4, 4, 8, 8, 1, 1e-6) == -3
    assert rn(P, P, P, Q, None, 0, P, 4, 4, 8, 8, 1, 1e-6) == -3
    assert rn(P, P, P, Q, None, 0, None, 4, 4, 8, 8, 1, 1e-6) == -3  # weight = NULL shares the validation
    fw = lambda *a: lib.az_qk_prep_w_f32(*a, None)  # noqa: E731
    #  q^ k^ q k batch tokens heads head_dim in_b in_t in_h out_b out_t out_h rms norm_dim eps cos sin wq wk
    assert fw(None, P, P, P, 1, 4, 2, 32, 768, 192, 32, 256, 64, 32, 1, 0, 1e-6, None, None, P, P) == -1
    assert fw(P, P, P, P, 1, 4, 2, 32, 768, 192, 32, 256, 64, 32, 1, 0, 1e-6, P, None, P, P) == -1  # cos without sin
    assert fw(P, P, P, P, 1, 0, 2, 32, 768, 192, 32, 256, 64, 32, 1, 0, 1e-6, None, None, P, P) == -2  # tokens == 0
    assert fw(P, P, P, P, 1, 4, 2, 32, 768, 192, 32, 256, 64, 32, 1, 33, 1e-6, None, None, P, P) == -2  # norm_dim > head_dim
    assert fw(P, P, P, P, 1, 4, 2, 48, 768, 192, 48, 256, 96, 48, 1, 0, 1e-6, None, None, P, P) == -4  # head_dim 48
    assert fw(P, Q, P, P, 1, 4, 2, 32, 768, 192, 32, 256, 64, 32, 1, 0, 1e-6, None, None, P, P) == -3
    assert fw(P, P, P, P, 1, 4, 2, 32, 768, 190, 32, 256, 64, 32, 1, 0, 1e-6, None, None, P, P) == -3  # stride % 4
    assert fw(P, P, P, P, 1, 4, 2, 32, 768, 192, 32, 256, 64, 32, 1, 0, 1e-6, None, None, Q, P) == -3  # misaligned gain
    assert fw(P, P, P, P, 1, 4, 2, 32, 768, 192, 32, 256, 64, 32, 1, 0, 1e-6, None, None, None, Q) == -3
    bw = lambda *a: lib.az_qk_prep_bwd_w_f32(*a, None)  # noqa: E731
    #  dq dk dq^ dk^ q k batch tokens heads head_dim g_b g_t g_h in_b in_t in_h out_b out_t out_h rms norm_dim eps cos sin wq wk
    assert bw(P, P, None, P, P, P, 1, 4, 2, 32, 256, 64, 32, 768, 192, 32, 768, 192, 32, 1, 0, 1e-6, None, None, P, P) == -1
    assert bw(P, P, P, P, P, P, 1, 4, 0, 32, 256, 64, 32, 768, 192, 32, 768, 192, 32, 1, 0, 1e-6, None, None, P, P) == -2  # heads == 0
    assert bw(P, P, P, P, P, P, 1, 4, 2, 80, 256, 64, 32, 768, 192, 32, 768, 192, 32, 1, 0, 1e-6, None, None, P, P) == -4
    assert bw(P, P, P, P, Q, P, 1, 4, 2, 32, 256, 64, 32, 768, 192, 32, 768, 192, 32, 1, 0, 1e-6, None, None, P, P) == -3
    assert bw(P, P, P, P, P, P, 1, 4, 2, 32, 256, 62, 32, 768, 192, 32, 768, 192, 32, 1, 0, 1e-6, None, None, P, P) == -3
    assert bw(P, P, P, P, P, P, 1, 4, 2, 32, 256, 64, 32, 768, 192, 32, 768, 192, 32, 1, 0, 1e-6, None, None, P, Q) == -3
    assert lib.az_cfg_split_f32(None, P, P, 16, None) == -1
    assert lib.az_cfg_split_f32(P, P, None, 16, None) == -1
    assert lib.az_cfg_split_f32(P, P, P, 0, None) == -2
    assert lib.az_cfg_split_f32(Q, P, P, 16, None) == -3
    assert lib.az_cfg_split_f32(P, Q, P, 16, None) == -3


def test_adm_cfg_clip_mask_input_conditions(golden):
    r"""At ``x_t = 0.5 x``, ``t = 0.3`` the fp64 oracle clips a real share of BOTH branch means of the class-conditional ADM
    fixture, and no unclipped element lies so close to +-1 that the forward's round-off (5e-6) could flip its mask:
    ``tests/test_gpu_jit_vjp.py`` asserts mask EQUALITY on the stacked batch.  Measured: shares 0.342 (y) and 0.333
    (neg_label), minimum distances 4.2e-4 and 1.2e-3."""
    g = golden("g5_adm_cond_neworder")
    cfg = g.meta["cfg"]
    sd = synth.synth_state_dict({k: tuple(v) for k, v in g.meta["shapes"].items()}, g.meta["weight_seed"])
    sig = sampling.adm_sigmas(cfg["discrete_schedule"], cfg["discrete_steps"]).double()
    for key in ("y", "neg_label"):
        with torch.no_grad():
            raw = sampling.adm_posterior(backbone_fn(sd, cfg, torch.float64), 0.5 * g["x"].double(), torch.tensor(0.3, dtype=torch.float64),
                                         sig, label=g[key], clip_mean=False)[0]
        share = float((raw.abs() >= 1).double().mean())
        dist = float((raw.abs() - 1).abs().min())
        print(key, f"clipped share {share:.3f}, minimum distance to +-1 {dist:.3e}")
        assert 0.2 <= share <= 0.6
        assert dist > 5e-5
