r"""``TDSSampler`` without a GPU: the restatement against the reference's recorded results (bit for bit), the constructor
signature against the reference's, the error paths, the argument codes of the new C entries, and the input conditions that the
GPU tests rest on (margins between the test uniforms and the fp64 CDF, ancestor diversity of the fixture)."""

import ctypes
import inspect

import pytest
import torch

import tds_cases as tc
import tds_oracle as to
from azula_amd import _lib


def test_fixture_holds_every_case(golden):
    g = golden("g29_tds")
    assert sorted(g.meta["e_ref"]) == sorted(tc.CASES)
    for tag in tc.CASES:
        assert 0 < g.meta["e_ref"][tag]["x_s"] < 1e-5 and 0 < g.meta["e_ref"][tag]["log_w"] < 1e-3
        assert torch.isfinite(g[f"{tag}_x"]).all() and torch.isfinite(g[f"{tag}_log_w"]).all()
        assert g[f"{tag}_ancestors"].shape == (g.meta["steps"] if tag.endswith("loop") else 1, 4)


@pytest.mark.parametrize("tag", tc.CASES)
def test_restatement_matches_reference_bitwise(golden, tag):
    r"""Under the fixture's CPU seed the restatement draws what the reference drew: same ancestors, same bits."""
    g = golden("g29_tds")
    mean, twists, arr, _, _ = tc.setup(g)
    torch.manual_seed(g.meta["seed"] + tc.SEED[tag])
    trace = tc.run_case(tag, mean, twists, arr, g.meta["steps"])
    assert torch.equal(trace[-1]["x_s"], g[f"{tag}_x"])
    assert torch.equal(torch.stack([s["ancestors"] for s in trace]), g[f"{tag}_ancestors"])
    assert torch.equal(torch.stack([s["log_w"] for s in trace]), g[f"{tag}_log_w"])
    assert torch.equal(torch.stack([s["log_p"] for s in trace]), g[f"{tag}_log_p"])


def test_fixture_ancestors_are_diverse(golden):
    r"""Over each loop at least one step selects two or more distinct ancestors and at least one repeats one."""
    g = golden("g29_tds")
    for tag in tc.CASES:
        if tag.endswith("loop"):
            distinct = [len(set(a.tolist())) for a in g[f"{tag}_ancestors"]]
            assert max(distinct) >= 2 and min(distinct) < 4, (tag, distinct)


def test_fixture_cdf_leaves_room_for_the_ancestor_check(golden):
    r"""``tests/test_gpu_tds.py`` compares the device's ancestors with the fp64 inverse CDF wherever a uniform lies at least 1e-3
    from every CDF value.  Whatever the device draws, that has to cover most pairs: per step of the fixture the uniforms that
    lie closer than that fill less than a quarter of [0, 1), and under the fixture's own weights a fixed grid of uniforms
    keeps three quarters of the (step, particle) pairs."""
    g = golden("g29_tds")
    u = (torch.arange(4, dtype=torch.float64) + 0.37) / 4
    for tag in tc.CASES:
        log_p, log_w = g[f"{tag}_log_p"].double(), g[f"{tag}_log_w"].double()
        kept = 0
        for n in range(len(log_p)):
            _, _, c = to.inverse_cdf(log_p[n] + (log_w[n - 1] if n else 0), u)
            assert 2e-3 * len(c) < 0.25
            kept += int((to.cdf_margin(c, u) >= 1e-3).sum())
        assert kept >= 0.75 * log_p.numel(), (tag, kept)


@pytest.mark.parametrize("K,kind,prev", tc.RESAMPLE_CASES)
def test_resample_cases_keep_their_margin(K, kind, prev):
    r"""Every uniform of the resampling kernel's test lies at least 1e-5 from every fp64 CDF value: an fp32 CDF (error at most
    about K 2^-24 = 1.5e-5 at K = 257, the kernel's fp64 one far less) cannot flip an index."""
    log_p, log_w_prev, u = tc.resample_case(K, kind, prev)
    log_w = log_p.double() + (log_w_prev.double() if prev else 0)
    k, w, c = to.inverse_cdf(log_w, u)
    assert float(to.cdf_margin(c, u).min()) >= tc.RESAMPLE_MARGIN
    assert (w[k] > 0).all() and torch.isfinite(w).all()
    if kind == "neginf" and K > 1:
        assert (w == 0).sum() >= 1
    if kind == "dominant":
        assert float(w.max()) > 1 - 1e-9


def test_constructor_signature(golden):
    from azula_amd.guidance import TDSSampler

    recorded = [(name, kind, default) for _, name, kind, default in golden("g29_tds").meta["signature"]]
    assert recorded == [("denoiser", "POSITIONAL_OR_KEYWORD", None), ("twist", "POSITIONAL_OR_KEYWORD", None), ("kwargs", "VAR_KEYWORD", None)]
    params = list(inspect.signature(TDSSampler.__init__).parameters.values())[1:]
    assert [(p.name, p.kind.name, None if p.default is inspect.Parameter.empty else repr(p.default)) for p in params] == recorded


def _host_denoiser():
    from azula_amd.denoise import KarrasDenoiser
    from azula_amd.nn import UNet
    from azula_amd.noise import VPSchedule

    return KarrasDenoiser(UNet(3, 3, hid_channels=(8,), hid_blocks=(1,)), VPSchedule())


def test_error_paths_on_host_tensors():
    r"""No eager fallback: a backbone without an input-gradient path, host or non-fp32 tensors, a sharded batch and more than
    65536 particles are errors."""
    from azula_amd.denoise import KarrasDenoiser
    from azula_amd.guidance import TDSSampler
    from azula_amd.nn import ViT
    from azula_amd.noise import VPSchedule

    twist = lambda x_hat, lam: -(x_hat**2).flatten(1)  # noqa: E731
    x, t, s = torch.zeros(2, 3, 8, 8), torch.tensor(0.5), torch.tensor(0.4)
    vit = KarrasDenoiser(ViT(3, 3, hid_channels=32, hid_blocks=1, attention_heads=2, patch_size=2, spatial=2), VPSchedule())
    with pytest.raises(NotImplementedError):
        TDSSampler(vit, twist, steps=2, silent=True).step(x, t, s, {})

    class Plain(torch.nn.Module):  # a denoiser without the _az_vjp protocol
        schedule = VPSchedule()

    with pytest.raises(NotImplementedError, match="_az_vjp"):
        TDSSampler(Plain(), twist, steps=2, silent=True).step(x, t, s, {})

    smp = TDSSampler(_host_denoiser(), twist, steps=2, silent=True)
    with pytest.raises(NotImplementedError, match="fp32 device tensors"):
        smp.step(x, t, s, {})
    with pytest.raises(NotImplementedError, match="fp32 device tensors"):
        smp(x.double())
    with pytest.raises(ValueError, match="65536"):
        smp.step(torch.zeros(65537, 1, 1, 1), t, s, {})
    smp.shard = (0, 2)
    with pytest.raises(NotImplementedError, match="coupled across the batch"):
        smp.step(x, t, s, {})


def test_new_entries_validate_their_arguments():
    from azula_amd.csrc import build

    build.build()
    lib = _lib.lib()
    P, Q = 0x10000, 0x10004  # aligned / misaligned addresses (never dereferenced: validation comes first)
    rs = lambda *a: lib.az_tds_resample_f32(*a, None)  # noqa: E731
    assert rs(None, None, P, P, P, 4) == -1 and rs(P, None, None, P, P, 4) == -1 and rs(P, None, P, None, P, 4) == -1
    assert rs(P, None, P, P, P, 0) == -2 and rs(P, None, P, P, P, 65537) == -2
    assert rs(P + 2, None, P, P, P, 4) == -3 and rs(P, None, P, Q, P, 4) == -3  # (ancestors are 8-byte integers)
    assert lib.az_tds_chunks(4, 768) == 1 and lib.az_tds_chunks(16, 3 * 256 * 256) == 48 and lib.az_tds_chunks(700, 8200) == 2
    assert lib.az_tds_chunks(65536, 1 << 20) == 1 and lib.az_tds_chunks(0, 5) == 0

    def args(**kw):
        d = dict(x_t=0x100000, x_hat=0x200000, score=0x300000, z=0x400000, ancestors=P, log_p=P, coef=P, x_s=0x500000,
                 log_w_next=P, workspace=P, K=4, N=768, chunks=1)
        d.update(kw)
        return ctypes.byref(_lib.AzTdsProposeArgs(**d))

    pr = lambda **kw: lib.az_tds_propose_f32(args(**kw), None)  # noqa: E731
    assert lib.az_tds_propose_f32(None, None) == -1
    for name in ("x_t", "x_hat", "score", "z", "ancestors", "log_p", "coef", "x_s", "log_w_next", "workspace"):
        assert pr(**{name: None}) == -1, name
    assert pr(K=0) == -2 and pr(N=0) == -2 and pr(K=65537) == -2 and pr(chunks=2) == -2
    for name in ("x_t", "x_hat", "score", "z"):  # x_s aliases or overlaps a gathered input (the rows are 4 * 768 * 4 bytes)
        assert pr(**{name: 0x500000}) == -2 and pr(**{name: 0x500000 + 4 * 768 * 4 - 16}) == -2, name
    assert pr(x_t=0x100004) == -3 and pr(x_s=0x500008) == -3 and pr(workspace=Q) == -3 and pr(ancestors=Q) == -3
