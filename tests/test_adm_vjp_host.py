r"""``UNetModel.vjp`` / ``AblatedDenoiser._az_vjp`` without a GPU: the input conditions the GPU test relies on, the scope errors
and the argument codes of the new C entries."""

import pytest
import torch

from azula_amd import _lib
from oracle import sampling, synth
from test_gpu_adm_vjp import backbone_fn


@pytest.mark.parametrize("name", ["g5_adm_uncond", "g5_adm_cond_neworder"])
def test_clip_mask_input_conditions(golden, name):
    r"""At ``x_t = 0.5 x``, ``t = 0.3`` the fp64 oracle clips a real share of the mean, and no unclipped element lies so close to
    +-1 that the forward's round-off (5e-6) could flip its mask: ``tests/test_gpu_adm_vjp.py`` asserts mask EQUALITY."""
    g = golden(name)
    cfg = g.meta["cfg"]
    sd = synth.synth_state_dict({k: tuple(v) for k, v in g.meta["shapes"].items()}, g.meta["weight_seed"])
    label = g["y"] if "y" in g else None
    sig = sampling.adm_sigmas(cfg["discrete_schedule"], cfg["discrete_steps"]).double()
    with torch.no_grad():
        raw = sampling.adm_posterior(backbone_fn(sd, cfg, torch.float64), 0.5 * g["x"].double(), torch.tensor(0.3, dtype=torch.float64),
                                     sig, label=label, clip_mean=False)[0]
    share = float((raw.abs() >= 1).double().mean())
    dist = float((raw.abs() - 1).abs().min())
    print(name, f"clipped share {share:.3f}, minimum distance to +-1 {dist:.3e}")
    assert 0.2 <= share <= 0.6
    assert dist > 5e-5


def test_scope_errors():
    from azula_amd.guidance import CFGDenoiser, DPSSampler
    from azula_amd.plugins import adm
    from azula_amd.plugins.adm.unet import UNetModel

    kw = dict(image_size=8, in_channels=2, model_channels=32, out_channels=2, num_res_blocks=1, attention_resolutions=())
    t = torch.tensor([3])
    with pytest.raises(NotImplementedError, match="dims = 3"):
        UNetModel(dims=3, **kw).vjp(torch.zeros(1, 2, 2, 8, 8), t)
    with pytest.raises(NotImplementedError, match="half-precision"):
        UNetModel(**kw).half().vjp(torch.zeros(1, 2, 8, 8), t)
    with pytest.raises(NotImplementedError, match="CPU tensors"):
        UNetModel(**kw).vjp(torch.zeros(1, 2, 8, 8), t)
    den = adm.make_model(image_size=8, image_channels=2, num_channels=32, channel_mult=(1,), num_res_blocks=1, attention_resolutions=())
    x = torch.zeros(1, 2, 8, 8)
    with pytest.raises(NotImplementedError, match="device tensors"):
        den._az_vjp(x, torch.tensor(0.5))
    A = lambda v: v.flatten(1)  # noqa: E731
    with pytest.raises(NotImplementedError, match="CFG"):
        DPSSampler(CFGDenoiser(den), A(x), A, steps=2, silent=True).step(x, torch.tensor(0.5), torch.tensor(0.4))


def test_new_entries_validate_their_arguments():
    from azula_amd.csrc import build

    build.build()
    lib = _lib.lib()
    P, Q = 0x1000, 0x1004  # aligned / misaligned addresses (never dereferenced: validation comes first)
    inf = float("inf")
    st = lambda *a: lib.az_norm_affine_bwd_stats_f32(*a, None)  # noqa: E731
    #  bpart x0 x1 c0s g S T weight scale bstride fpart fchunks B H W C cs groups nchunks act pool eps
    assert st(None, P, None, 0, P, P, P, None, None, 0, P, 1, 1, 4, 4, 8, 8, 2, 1, 1, 0, 1e-5) == -1
    assert st(P, P, None, 0, P, P, P, None, None, 0, None, 1, 1, 4, 4, 8, 8, 2, 1, 1, 0, 1e-5) == -1
    assert st(P, P, None, 0, P, P, P, None, None, 0, P, 1, 1, 4, 4, 8, 8, 3, 1, 1, 0, 1e-5) == -2  # C % groups
    assert st(P, P, None, 0, P, P, P, None, None, 0, P, 1, 1, 4, 4, 6, 6, 2, 1, 1, 0, 1e-5) == -2  # cs % 4
    assert st(P, P, None, 0, P, P, P, None, None, 0, P, 1, 1, 4, 4, 8, 8, 2, 1, 2, 0, 1e-5) == -2  # act
    assert st(P, P, None, 0, P, P, P, None, None, 0, P, 1, 1, 3, 4, 8, 8, 2, 1, 1, 1, 1e-5) == -2  # 2x2 pool of an odd height
    assert st(P, P, P, 6, P, P, P, None, None, 0, P, 1, 1, 4, 4, 8, 8, 2, 1, 1, 0, 1e-5) == -2  # c0s % 4
    assert st(P, P, P, 4, P, P, P, None, None, 0, P, 1, 1, 4, 4, 8, 12, 2, 1, 1, 0, 1e-5) == -2  # two sources: C == cs
    assert st(P, Q, None, 0, P, P, P, None, None, 0, P, 1, 1, 4, 4, 8, 8, 2, 1, 1, 0, 1e-5) == -3
    assert st(P, P, Q, 4, P, P, P, None, None, 0, P, 1, 1, 4, 4, 8, 8, 2, 1, 1, 0, 1e-5) == -3
    ap = lambda *a: lib.az_norm_affine_bwd_apply_f32(*a, None)  # noqa: E731
    #  dx0 dx1 res0 res1 x0 x1 c0s g S T weight scale bstride fpart fchunks bpart nchunks B H W C cs groups act pool eps
    assert ap(None, None, None, None, P, None, 0, P, P, P, None, None, 0, P, 1, P, 1, 1, 4, 4, 8, 8, 2, 1, 0, 1e-5) == -1
    assert ap(P, None, None, None, P, P, 4, P, P, P, None, None, 0, P, 1, P, 1, 1, 4, 4, 8, 8, 2, 1, 0, 1e-5) == -1  # x1 without dx1
    assert ap(P, None, None, None, P, None, 0, P, P, P, None, None, 0, P, 1, None, 1, 1, 4, 4, 8, 8, 2, 1, 0, 1e-5) == -1
    assert ap(P, None, None, None, P, None, 0, P, P, P, None, None, 0, P, 0, P, 1, 1, 4, 4, 8, 8, 2, 1, 0, 1e-5) == -2  # fchunks == 0
    assert ap(P, None, None, None, P, None, 0, P, P, P, None, None, 0, P, 1, P, 1, 1, 4, 4, 8, 8, 2, 1, 3, 1e-5) == -2  # pool
    assert ap(Q, None, None, None, P, None, 0, P, P, P, None, None, 0, P, 1, P, 1, 1, 4, 4, 8, 8, 2, 1, 0, 1e-5) == -3
    assert ap(P, None, Q, None, P, None, 0, P, P, P, None, None, 0, P, 1, P, 1, 1, 4, 4, 8, 8, 2, 1, 0, 1e-5) == -3
    assert lib.az_avgpool_bwd_f32(None, P, None, 1, 4, 4, 8, 1, None) == -1
    assert lib.az_avgpool_bwd_f32(P, P, None, 1, 3, 4, 8, 1, None) == -2  # odd height under a 2x2 pool
    assert lib.az_avgpool_bwd_f32(P, P, None, 1, 4, 4, 8, 0, None) == -2  # mode
    assert lib.az_avgpool_bwd_f32(P, P, None, 1, 4, 4, 6, 2, None) == -2  # cs % 4
    assert lib.az_avgpool_bwd_f32(P, Q, None, 1, 4, 4, 8, 1, None) == -3
    assert lib.az_avgpool_bwd_f32(P, P, Q, 1, 4, 4, 8, 1, None) == -3
    assert lib.az_adm_precond_bwd_out_f32(P, None, P, P, 0, 1, 3, 6, 16, -1.0, 1.0, None) == -1
    assert lib.az_adm_precond_bwd_out_f32(P, P, P, P, 0, 1, 3, 2, 16, -1.0, 1.0, None) == -2  # F < C
    assert lib.az_adm_precond_bwd_out_f32(P, P, P, P, 0, 1, 3, 6, 16, 1.0, -1.0, None) == -2  # lo >= hi
    assert lib.az_adm_precond_bwd_in_f32(P, P, P, P, None, P, 0, 1, 48, -inf, inf, None) == -1
    assert lib.az_adm_precond_bwd_in_f32(P, P, P, P, P, P, 0, 1, 0, -inf, inf, None) == -2
