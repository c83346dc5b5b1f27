r"""The guidance classes on a DiT backbone: ``KarrasDenoiser(TimeModulated(DiT))`` on (2, 16, 16) token tensors against the
restatement of ``tests/guidance_vjp_oracle.py`` over an fp64 posterior-mean function built from ``oracle.nets`` pieces (the time
embedding as in ``nets.time_wrapped_vit``, ``dit_forward``, Karras preconditioning).

Bound per check: ``max(4 e_ref, 1e-4)`` relative to the largest magnitude of the fp64 result; ``e_ref`` is what the SAME function
loses on the fp32 ``mean_fn`` against the fp64 one, measured here on the CPU.
"""

import pytest
import torch
import torch.nn.functional as F

import guidance_vjp_oracle as go
from oracle import nets, sampling, synth

pytestmark = pytest.mark.gpu

CFG = {"hid_channels": 64, "hid_blocks": 2, "attention_heads": 4}
D = 32
VAR_Y = 0.01


def rel(a, ref):
    return float((a.double().cpu() - ref).abs().max() / ref.abs().max())


@pytest.fixture(scope="module")
def setup():
    from azula_amd.denoise import KarrasDenoiser
    from azula_amd.nn import DiT, TimeModulated
    from azula_amd.noise import VPSchedule

    w = TimeModulated(DiT(16, 16, mod_features=D, **CFG), D, name="dit")
    sd = synth.synth_state_dict({k: tuple(v.shape) for k, v in w.state_dict().items()}, 77)
    w.load_state_dict(sd)
    den = KarrasDenoiser(w, VPSchedule()).cuda().eval()

    def mean_fn(dtype):
        sdd = {k: v.to(dtype) for k, v in sd.items()}
        sub = {k[len("dit."):]: v for k, v in sdd.items() if k.startswith("dit.")}

        def backbone(x, c_time):
            mod = F.linear(c_time[..., None], sdd["time_embedding.0.weight"], sdd["time_embedding.0.bias"])
            mod = F.linear(F.silu(mod), sdd["time_embedding.2.weight"], sdd["time_embedding.2.bias"])
            return nets.dit_forward(sub, CFG, x, mod)

        return lambda x, t: sampling.karras_mean(backbone, x, t, backbone_dtype=dtype)

    gen = torch.Generator().manual_seed(78)
    x_t = torch.randn(2, 16, 16, generator=gen)
    mask = (torch.rand(1, 16, 16, generator=gen) < 0.5).float()
    A = lambda x: (x * mask.to(x)).flatten(1)  # noqa: E731
    y = A(torch.randn(2, 16, 16, generator=gen))
    return dict(den=den, mean=mean_fn, x_t=x_t, y=y, A=A, t=torch.tensor(0.6), s=torch.tensor(0.5))


def both(fn, s):
    r"""fn(mean_fn, cast) in fp64 and fp32 -> (fp64 result, e_ref)."""
    r64 = fn(s["mean"](torch.float64), lambda v: v.double())
    r32 = fn(s["mean"](torch.float32), lambda v: v.float())
    return r64.double(), rel(r32, r64.double())


def test_denoiser_pullback(setup):
    s = setup
    v = torch.randn(2, 16, 16, generator=torch.Generator().manual_seed(79))

    def fn(mean, cast):
        x = cast(s["x_t"]).requires_grad_()
        with torch.enable_grad():
            m = mean(x, cast(s["t"]))
            return torch.cat((m.detach().flatten(), torch.autograd.grad(m, x, cast(v))[0].flatten()))

    ref, e_ref = both(fn, s)
    mean, pull = s["den"]._az_vjp(s["x_t"].cuda(), s["t"].cuda())
    got = torch.cat((mean.flatten(), pull(v.cuda()).flatten()))
    err = rel(got, ref)
    print(f"_az_vjp: err {err:.3e} e_ref {e_ref:.3e}")
    assert err < max(4 * e_ref, 1e-4)  # measured 3.4e-7 (e_ref 3.0e-7) (MI355X)


def test_dps_step(setup):
    from azula_amd.guidance import DPSSampler

    s = setup
    A = s["A"]
    smp = DPSSampler(s["den"], s["y"].cuda(), lambda x: A(x), steps=8, silent=True)
    torch.manual_seed(5)
    eps = torch.randn_like(s["x_t"].cuda()).cpu()
    torch.manual_seed(5)
    out = smp.step(s["x_t"].cuda(), s["t"].cuda(), s["s"].cuda())
    ref, e_ref = both(lambda mean, cast: go.dps_step(mean, cast(s["x_t"]), cast(s["t"]), cast(s["s"]), cast(eps), cast(s["y"]), A), s)
    err = rel(out, ref)
    print(f"DPS step: err {err:.3e} e_ref {e_ref:.3e}")
    assert out.shape == ref.shape and torch.isfinite(out).all()
    assert err < max(4 * e_ref, 1e-4)  # measured 1.9e-7 (e_ref 1.6e-7) (MI355X)


def test_mmps_denoiser(setup):
    from azula_amd.guidance import MMPSDenoiser
    from azula_amd.linalg.covariance import IsotropicCovariance

    s = setup
    A = s["A"]
    cov = IsotropicCovariance(torch.tensor(VAR_Y, device="cuda"))
    out = MMPSDenoiser(s["den"], s["y"].cuda(), lambda x: A(x), cov, solver="gmres", iterations=2)(s["x_t"].cuda(), s["t"].cuda()).mean
    ref, e_ref = both(lambda mean, cast: go.mmps_mean(mean, cast(s["x_t"]), cast(s["t"]), cast(s["y"]), A, lambda v: VAR_Y * v, "gmres", 2), s)
    err = rel(out, ref)
    print(f"MMPS (gmres, 2 iterations): err {err:.3e} e_ref {e_ref:.3e}")
    assert out.shape == ref.shape and torch.isfinite(out).all()
    assert err < max(4 * e_ref, 1e-4)  # measured 3.2e-7 (e_ref 3.0e-7) (MI355X)
