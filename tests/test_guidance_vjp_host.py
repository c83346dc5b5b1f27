r"""DPS / PGDM / TMPD / MMPS without a GPU: the restatement against the reference's recorded results (bit for bit), the
constructor signatures against the reference's, the error for a backbone without an input-gradient path, and the argument
codes of the new C entries."""

import inspect

import pytest
import torch

import guidance_vjp_cases as gc
from azula_amd import _lib

CASES = [f"{k}_{op}_{r}" for op in ("mask", "pool") for k, r in
         [("dps", "zeta1.0_step"), ("dps", "zeta0.3_step"), ("dps", "loop"), ("pgdm", "eta0.0_step"), ("pgdm", "eta0.5_step"),
          ("pgdm", "loop"), ("mmps", "cg_it1"), ("mmps", "cg_it3"), ("mmps", "gmres_it1"), ("mmps", "gmres_it3")]] + ["tmpd_mask", "tmpd_pool"]


def test_fixture_holds_every_case(golden):
    g = golden("g28_guidance_vjp")
    assert sorted(g.meta["e_ref"]) == sorted(CASES)
    assert all(0 < v < 0.05 for v in g.meta["e_ref"].values())
    assert all(torch.isfinite(g[c]).all() for c in CASES)


@pytest.mark.parametrize("tag", CASES)
def test_restatement_matches_reference_bitwise(golden, tag):
    g = golden("g28_guidance_vjp")
    mean, ops, arr, _, _ = gc.setup(g)
    out = gc.run_case(tag, mean, ops, arr, g.meta["steps"], g.meta["var_y"])
    assert torch.equal(out, g[tag])


SIGNATURES = {
    "DPSSampler": [("denoiser", None), ("y", None), ("A", None), ("zeta", "1.0"), ("kwargs", None)],
    "PGDMSampler": [("denoiser", None), ("y", None), ("A", None), ("A_inv", None), ("kwargs", None)],
    "TMPDenoiser": [("denoiser", None), ("y", None), ("A", None), ("var_y", None)],
    "MMPSDenoiser": [("denoiser", None), ("y", None), ("A", None), ("cov_y", None), ("solver", "'gmres'"), ("iterations", "1")],
}


def test_constructor_signatures(golden):
    import azula_amd.guidance as G

    recorded = {}
    for cls, name, kind, default in golden("g28_guidance_vjp").meta["signature"]:
        recorded.setdefault(cls, []).append((name, default))
    assert recorded == SIGNATURES  # (the reference's, as the fixture script read them)
    for cls, want in SIGNATURES.items():
        params = list(inspect.signature(getattr(G, cls).__init__).parameters.values())[1:]
        got = [(p.name, None if p.default is inspect.Parameter.empty else repr(p.default)) for p in params]
        assert got == want, cls
        assert params[-1].kind is (inspect.Parameter.VAR_KEYWORD if want[-1][0] == "kwargs" else inspect.Parameter.POSITIONAL_OR_KEYWORD)
    with pytest.raises(ValueError, match="Unknown solver"):
        G.MMPSDenoiser(None, None, None, None, solver="lu")


def test_backbone_without_vjp_is_an_error():
    r"""No silent torch fallback: a ViT-backed denoiser (no input-gradient kernels) raises, naming the backbone."""
    from azula_amd.denoise import KarrasDenoiser, SimpleDenoiser
    from azula_amd.guidance import DPSSampler, MMPSDenoiser, PGDMSampler, TMPDenoiser
    from azula_amd.linalg.covariance import IsotropicCovariance
    from azula_amd.nn import ViT
    from azula_amd.noise import VPSchedule

    vit = ViT(3, 3, hid_channels=32, hid_blocks=1, attention_heads=2, patch_size=2, spatial=2)
    x, t, s = torch.zeros(1, 3, 8, 8), torch.tensor(0.5), torch.tensor(0.4)
    A = lambda v: v.flatten(1)  # noqa: E731
    for Den in (KarrasDenoiser, SimpleDenoiser):
        den = Den(vit, VPSchedule())
        with pytest.raises(NotImplementedError, match="ViT|device tensors"):
            den._az_vjp(x, t)
        for obj, call in ((DPSSampler(den, A(x), A, steps=2, silent=True), lambda o: o.step(x, t, s)),
                          (PGDMSampler(den, A(x), A, lambda y: y.reshape(x.shape), steps=2, silent=True), lambda o: o.step(x, t, s)),
                          (TMPDenoiser(den, A(x), A, 1.0), lambda o: o(x, t)),
                          (MMPSDenoiser(den, A(x), A, IsotropicCovariance(1.0)), lambda o: o(x, t))):
            with pytest.raises(NotImplementedError):
                call(obj)


def test_backbone_error_names_the_backbone(monkeypatch):
    from azula_amd import denoise
    from azula_amd.nn import ViT
    from azula_amd.noise import VPSchedule

    vit = ViT(3, 3, hid_channels=32, hid_blocks=1, attention_heads=2, patch_size=2, spatial=2)
    den = denoise.KarrasDenoiser(vit, VPSchedule())

    class FakeDevice(torch.Tensor):
        is_cuda = True

    with pytest.raises(NotImplementedError, match="backbone ViT has no input-gradient"):
        denoise._vjp_preconditioned(den, torch.zeros(1, 3, 8, 8).as_subclass(FakeDevice), None, None, None, None, {})


def test_new_entries_validate_their_arguments():
    from azula_amd.csrc import build

    build.build()
    lib = _lib.lib()
    P, Q = 0x1000, 0x1004  # aligned / misaligned addresses (never dereferenced: validation comes first)
    gs = lambda *a: lib.az_groupnorm_bwd_stats_f32(*a, None)  # noqa: E731
    assert gs(None, P, P, None, 0, P, 1, 1, 16, 8, 8, 2, 1, 1e-5) == -1
    assert gs(P, P, P, None, 0, P, 1, 1, 16, 8, 8, 3, 1, 1e-5) == -2  # C % groups
    assert gs(P, P, P, None, 0, P, 1, 1, 16, 6, 6, 2, 1, 1e-5) == -2  # cs % 4
    assert gs(P, Q, P, None, 0, P, 1, 1, 16, 8, 8, 2, 1, 1e-5) == -3
    ga = lambda *a: lib.az_groupnorm_bwd_apply_f32(*a, None)  # noqa: E731
    assert ga(P, P, P, None, None, 0, P, 1, None, 1, 1, 16, 8, 8, 2, 1e-5) == -1
    assert ga(P, P, P, None, None, 0, P, 0, P, 1, 1, 16, 8, 8, 2, 1e-5) == -2  # fchunks == 0
    assert ga(P, P, P, Q, None, 0, P, 1, P, 1, 1, 16, 8, 8, 2, 1e-5) == -3
    rn = lambda *a: lib.az_rownorm_bwd_f32(*a, None)  # noqa: E731
    assert rn(P, None, P, None, None, 0, 4, 4, 8, 8, 0, 1e-5) == -1
    assert rn(P, P, P, None, None, 0, 4, 4, 8, 8, 2, 1e-5) == -2  # kind
    assert rn(P, P, P, None, None, 0, 4, 4, 1, 4, 0, 1e-5) == -2  # unbiased variance of one channel
    assert rn(Q, P, P, None, None, 0, 4, 4, 8, 8, 0, 1e-5) == -3
    assert lib.az_silu_bwd_f32(P, P, None, 16, None) == -1
    assert lib.az_silu_bwd_f32(P, P, P, 18, None) == -2
    assert lib.az_silu_bwd_f32(P, Q, P, 16, None) == -3
    assert lib.az_channel_scale_f32(P, P, None, 0, 1, 16, 8, 8, None) == -1
    assert lib.az_channel_scale_f32(P, P, P, 0, 1, 16, 9, 8, None) == -2  # C > cs
    assert lib.az_channel_scale_f32(P, Q, P, 0, 1, 16, 8, 8, None) == -3
    assert lib.az_zero_stuff_f32(None, P, 1, 4, 4, 8, 2, 2, 8, 8, None) == -1
    assert lib.az_zero_stuff_f32(P, P, 1, 5, 4, 8, 2, 2, 8, 8, None) == -2  # (5 - 1) * 2 > 8 - 1: would write outside G
    assert lib.az_zero_stuff_f32(Q, P, 1, 4, 4, 8, 2, 2, 8, 8, None) == -3
    assert lib.az_upsample_nearest_bwd_f32(P, None, 1, 4, 4, 8, 2, 2, 8, 8, None) == -1
    assert lib.az_upsample_nearest_bwd_f32(P, P, 1, 4, 4, 8, 2, 2, 9, 8, None) == -2  # narrowed map larger than the upsampled one
    assert lib.az_upsample_nearest_bwd_f32(P, Q, 1, 4, 4, 8, 2, 2, 8, 8, None) == -3
