r"""``DPSSampler``, ``PGDMSampler``, ``TMPDenoiser`` and ``MMPSDenoiser`` on the GPU (the network part of every gradient is the
HIP pullback of the UNet) against the restatement of ``tests/guidance_vjp_oracle.py`` run on the host in fp64 with the
device's own noise draws copied over.

Every case of ``tests/golden/g28_guidance_vjp.npz`` runs: one step and the 8-step loop of DPS and PGDM, one ``forward`` of
TMPD and of MMPS (``cg`` / ``gmres``, 1 and 3 iterations), with the pixel mask and with the 2x average pooling; non-default
``zeta`` and ``eta`` once each.  Bound per case: ``max(4 e_ref, 1e-4)`` relative to the largest magnitude of the fp64 result;
``e_ref`` is what the REFERENCE loses in fp32 on that case against fp64 (measured on the CPU by
``tools/make_golden_guidance_vjp.py``, stored in the fixture), 1e-4 the forward tolerance of the same UNet
(``tests/test_gpu_unet.py``).  ``mmps_*_cg_it3`` is ill-conditioned in the reference itself (e_ref 1e-3 .. 1e-2: the synthetic
network's Jacobian is not symmetric, so the third CG iteration amplifies rounding); it is held to its own e_ref like the rest.
"""

import pytest
import torch

import guidance_vjp_cases as gc
from test_guidance_vjp_host import CASES

pytestmark = pytest.mark.gpu
SEED = 321


def device_denoiser(sd, cfg):
    from azula_amd.denoise import KarrasDenoiser
    from azula_amd.nn import TimeModulated, UNet
    from azula_amd.noise import VPSchedule

    net = UNet(cfg["in_channels"], cfg["out_channels"], hid_channels=cfg["hid_channels"], hid_blocks=cfg["hid_blocks"],
               norm=cfg["norm"], groups=cfg["groups"], mod_features=cfg["mod_features"])
    w = TimeModulated(net, cfg["mod_features"], name="unet")
    w.load_state_dict(sd)
    return KarrasDenoiser(w, VPSchedule()).cuda().eval()


def run_device(tag, den, ops, g):
    r"""(device result, the eps the device drew) of the fixture case ``tag``."""
    from azula_amd.guidance import DPSSampler, MMPSDenoiser, PGDMSampler, TMPDenoiser
    from azula_amd.linalg.covariance import IsotropicCovariance

    steps, var_y = g.meta["steps"], g.meta["var_y"]
    kind, name, *rest = tag.split("_")
    A, A_inv = ops[name]
    y = g[f"{name}_y"].cuda()
    x_t, x1, t, s = g["x_t"].cuda(), g["x1"].cuda(), g["t"].cuda(), g["s"].cuda()
    torch.manual_seed(SEED)
    eps = torch.stack([torch.randn_like(x1) for _ in range(steps)]).cpu()
    torch.manual_seed(SEED)
    if kind in ("dps", "pgdm"):
        if kind == "dps":
            smp = DPSSampler(den, y, A, steps=steps, silent=True) if rest[0] == "loop" else \
                DPSSampler(den, y, A, zeta=float(rest[0][4:]), steps=steps, silent=True)
        else:
            smp = PGDMSampler(den, y, A, A_inv, steps=steps, silent=True) if rest[0] == "loop" else \
                PGDMSampler(den, y, A, A_inv, eta=float(rest[0][3:]), steps=steps, silent=True)
        out = smp(x1) if rest[0] == "loop" else smp.step(x_t, t, s)
    elif kind == "tmpd":
        out = TMPDenoiser(den, y, A, var_y)(x_t, t).mean
    else:
        cov = IsotropicCovariance(torch.tensor(var_y, device="cuda"))
        out = MMPSDenoiser(den, y, A, cov, solver=rest[0], iterations=int(rest[1][2:]))(x_t, t).mean
    return out, eps


@pytest.mark.parametrize("tag", CASES)
def test_guidance_matches_fp64_restatement(golden, tag):
    g = golden("g28_guidance_vjp")
    mean64, ops, arr64, sd, cfg = gc.setup(g, torch.float64)
    den = device_denoiser(sd, cfg)
    out, eps = run_device(tag, den, ops, g)
    ref = gc.run_case(tag, mean64, ops, arr64, g.meta["steps"], g.meta["var_y"], eps=eps.double())
    assert out.shape == ref.shape and torch.isfinite(out).all()
    err = float((out.double().cpu() - ref).abs().max() / ref.abs().max())
    e_ref = g.meta["e_ref"][tag]
    print(f"{tag}: err {err:.3e} e_ref {e_ref:.3e} bound {max(4 * e_ref, 1e-4):.3e}")
    assert err < max(4 * e_ref, 1e-4)  # measured: see DESIGN.md, "input gradient" (MI355X)


def test_loop_runs_the_generic_path_and_is_repeatable(golden):
    r"""The guided samplers override ``step``: no captured plan; two runs from the same seed give the same bits."""
    from azula_amd.guidance import DPSSampler

    g = golden("g28_guidance_vjp")
    _, ops, _, sd, cfg = gc.setup(g)
    den = device_denoiser(sd, cfg)
    smp = DPSSampler(den, g["mask_y"].cuda(), ops["mask"][0], steps=4, silent=True)
    x1 = g["x1"].cuda()
    torch.manual_seed(1)
    a = smp(x1)
    torch.manual_seed(1)
    b = smp(x1)
    assert torch.equal(a, b) and not smp._fused_cache
