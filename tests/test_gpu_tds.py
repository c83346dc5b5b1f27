r"""``TDSSampler`` on the GPU against the restatement of ``tests/tds_oracle.py`` run on the host in fp64 with the device's own
ancestors and noise.

For every case of ``tests/golden/g29_tds.npz`` (one step and the 8-step loop, Gaussian twists over a pixel mask and over a 2x
average pooling) the test drives ``step`` itself over ``sampler.timesteps``, reads ``carry["ancestors"]`` after each step and
replays the device's ``rand`` / ``randn_like`` draws under the same seed; the fp64 restatement gets those ancestors and normals.
``x_s`` and ``carry["log_w"]`` are compared after every step -- ``x_s`` relative to the largest magnitude, ``log_w`` as an
absolute error over ``max(1, max |log_w|)`` -- within ``max(4 e_ref, 1e-4)``: ``e_ref`` is what the REFERENCE loses in fp32 on
that case against fp64 (``tools/make_golden_tds.py``), 1e-4 the forward tolerance of the same UNet (``tests/test_gpu_unet.py``).
The device's ancestors equal the inverse CDF of the fp64 weights on the replayed uniforms wherever a uniform lies at least 1e-3
from every fp64 CDF value (the weights carry the network's 1e-4 error); at least three quarters of the pairs are checked.
"""

import pytest
import torch

import tds_cases as tc
import tds_oracle as to
from test_gpu_guidance_vjp import device_denoiser

pytestmark = pytest.mark.gpu
SEED = 4321


def device_twists(g):
    arr = {k: v.cuda() for k, v in g.arrays.items()}
    return tc.make_twists(arr, g.meta["var_y"])


def drive(smp, x, pairs):
    r"""The loop by hand: ``(per-step x_s, log_w, ancestors, w)``."""
    carry: dict = {}
    out = []
    for t, s in pairs:
        x = smp.step(x, t, s, carry)
        out.append({k: v.clone() for k, v in (("x_s", x), ("log_w", carry["log_w"]), ("ancestors", carry["ancestors"]), ("w", carry["w"]))})
    return out


@pytest.mark.parametrize("tag", tc.CASES)
def test_tds_matches_fp64_restatement(golden, tag):
    from azula_amd.guidance import TDSSampler

    g = golden("g29_tds")
    mean64, twists64, arr64, sd, cfg = tc.setup(g, torch.float64)
    den = device_denoiser(sd, cfg)
    name, kind = tag.split("_")
    steps = g.meta["steps"]
    smp = TDSSampler(den, device_twists(g)[name], steps=steps, silent=True)
    if kind == "step":
        x0, pairs = g["x_t"].cuda(), [(g["t"].cuda(), g["s"].cuda())]
    else:
        x0, pairs = g["x1"].cuda(), list(smp.timesteps.unfold(0, 2, 1).cuda().unbind())
    K = x0.shape[0]
    torch.manual_seed(SEED)
    draws = [(torch.rand(K, dtype=torch.float32, device="cuda").cpu(), torch.randn_like(x0).cpu()) for _ in pairs]
    torch.manual_seed(SEED)
    trace = drive(smp, x0, pairs)
    assert trace[0]["ancestors"].dtype == torch.int64 and trace[0]["w"].shape == (K,)
    ancestors = [s["ancestors"].cpu() for s in trace]
    ref = tc.run_case(tag, mean64, twists64, arr64, steps, ancestors, [z.double() for _, z in draws])

    e_ref = g.meta["e_ref"][tag]
    checked = 0
    for n, (dev, r) in enumerate(zip(trace, ref)):
        ex = float((dev["x_s"].double().cpu() - r["x_s"]).abs().max() / r["x_s"].abs().max())
        ew = float((dev["log_w"].double().cpu() - r["log_w"]).abs().max() / max(1.0, float(r["log_w"].abs().max())))
        print(f"{tag} step {n}: x_s {ex:.3e} (e_ref {e_ref['x_s']:.3e}) log_w {ew:.3e} (e_ref {e_ref['log_w']:.3e}) "
              f"ancestors {ancestors[n].tolist()}")
        assert torch.isfinite(dev["x_s"]).all() and torch.isfinite(dev["log_w"]).all()
        assert ex < max(4 * e_ref["x_s"], 1e-4)  # measured: see DESIGN.md, "twisted diffusion sampler" (MI355X)
        assert ew < max(4 * e_ref["log_w"], 1e-4)
        # the fp64 weights of this step (the restatement's log_p + its previous log_w) against the device's choice
        log_w = r["log_p"] + (ref[n - 1]["log_w"] if n else 0)
        k64, w64, c = to.inverse_cdf(log_w, draws[n][0])
        safe = to.cdf_margin(c, draws[n][0]) >= 1e-3
        assert torch.equal(ancestors[n][safe], k64[safe])
        checked += int(safe.sum())
        # softmax is 2-Lipschitz in the largest log-weight error, which is at most the two bounds above (log_p, previous log_w)
        tol_w = 4 * max(4 * e_ref["log_w"], 1e-4) * max(1.0, float(log_w.abs().max()))
        assert float((dev["w"].double().cpu() - w64).abs().max()) < tol_w
    assert checked >= 0.75 * K * len(trace)


def test_call_equals_the_hand_driven_loop_and_is_repeatable(golden):
    r"""``sampler(x1)`` is the hand-driven loop bit for bit, on the generic path (no captured plan), repeatable under a seed."""
    from azula_amd.guidance import TDSSampler

    g = golden("g29_tds")
    _, _, _, sd, cfg = tc.setup(g)
    den = device_denoiser(sd, cfg)
    smp = TDSSampler(den, device_twists(g)["mask"], steps=4, silent=True)
    x1 = g["x1"].cuda()
    torch.manual_seed(1)
    a = smp(x1)
    torch.manual_seed(1)
    b = smp(x1)
    torch.manual_seed(1)
    c = drive(smp, x1, list(smp.timesteps.unfold(0, 2, 1).cuda().unbind()))[-1]["x_s"]
    assert torch.equal(a, b) and torch.equal(a, c) and not smp._fused_cache
    assert torch.isfinite(a).all()


def test_vit_backbone_is_an_error():
    from azula_amd.denoise import KarrasDenoiser
    from azula_amd.guidance import TDSSampler
    from azula_amd.nn import ViT
    from azula_amd.noise import VPSchedule

    vit = ViT(3, 3, hid_channels=32, hid_blocks=1, attention_heads=2, patch_size=2, spatial=2)
    den = KarrasDenoiser(vit, VPSchedule()).cuda()
    smp = TDSSampler(den, lambda x_hat, lam: -(x_hat**2).flatten(1), steps=2, silent=True)
    with pytest.raises(NotImplementedError, match="ViT"):
        smp(torch.zeros(2, 3, 8, 8, device="cuda"))
