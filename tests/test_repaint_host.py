r"""RePaintSampler (reference ``azula/guidance/repaint.py:20-63``) without a GPU: the public API against the reference's recorded
signature, host runs and the per-step scalar table of the captured loop, the loop's rows and generator order, and the C ABI of
``az_repaint_f32``.

Host results are checked two ways.  Bit for bit, output dtype and generator state included, against the restatement of
``tests/repaint_oracle.py`` run on the same machine (``tools/make_golden_repaint.py`` pins that restatement bit for bit to the
reference before it writes G25).  And against the reference's own numbers in G25 within a round-off bound: torch's CPU kernels
(exp, sqrt, the vectorised normal draw, GEMM) round differently on different CPUs, so a fixture recorded on one CPU is not
bit-reproducible on every other one.
"""

import ctypes
import inspect
import os
import subprocess
import tempfile

import pytest
import torch

import repaint_oracle
from conftest import ROOT, max_err
from oracle import nets, sampling, synth

TOY_CASES = ["toy_eta0_it3", "toy_eta06_it2_bcast", "toy_f64"]


class ToyMLP(torch.nn.Module):
    r"""The fixture's backbone (the reference tests' Dummy): Linear -> + SineEncoding(t) -> ReLU -> Linear."""

    def __init__(self, features: int = 5) -> None:
        super().__init__()
        from azula_amd.nn.layers import SineEncoding

        self.l1 = torch.nn.Linear(features, 64)
        self.l2 = torch.nn.Linear(64, features)
        self.time_encoding = SineEncoding(64)

    def forward(self, x_t, t):
        return self.l2(torch.relu(self.l1(x_t) + self.time_encoding(t)))


def toy_denoiser(g):
    from azula_amd.denoise import KarrasDenoiser
    from azula_amd.noise import VPSchedule

    net = ToyMLP(5)
    net.load_state_dict(synth.synth_state_dict({k: tuple(v) for k, v in g.meta["toy_shapes"].items()}, g.meta["toy_weight_seed"]),
                        strict=False)
    return KarrasDenoiser(net, VPSchedule()).eval()


def toy_mean(g):
    r"""The restated posterior mean of the fixture's denoiser (KarrasDenoiser(ToyMLP), azula/denoise.py:293-324)."""
    sd = synth.synth_state_dict({k: tuple(v) for k, v in g.meta["toy_shapes"].items()}, g.meta["toy_weight_seed"])

    def backbone(x, c_time):
        h = torch.nn.functional.linear(x, sd["l1.weight"], sd["l1.bias"]) + nets.sine_encoding(c_time, 64)
        return torch.nn.functional.linear(torch.relu(h), sd["l2.weight"], sd["l2.bias"])

    return lambda x, t: sampling.karras_mean(backbone, x, t)  # noqa: E731


def restated(g, case):
    r"""(x0, generator state after sampling) of the restatement on this machine, under the fixture's seed."""
    kw = g.meta["cases"][case]
    dtype = getattr(torch, kw["dtype"].split(".")[-1]) if "dtype" in kw else None
    torch.manual_seed(g.meta["loop_seed"])
    x0 = repaint_oracle.sample_repaint(toy_mean(g), g[f"{case}_x1"], g[f"{case}_y"], g[f"{case}_mask"], steps=kw["steps"],
                                       iterations=kw["iterations"], eta=kw["eta"], dtype=dtype)
    return x0, torch.get_rng_state()


def close_to_reference(x: torch.Tensor, ref: torch.Tensor) -> bool:
    r"""Within the round-off of torch's CPU kernels on another CPU: 2e-6 x 5.8 measured across ATen's CPU paths, bound 5 x."""
    return x.dtype == ref.dtype and max_err(x, ref) < 2e-6 * max(1.0, ref.abs().max().item())


def make(den, g, case, **extra):
    from azula_amd.guidance import RePaintSampler

    kw = dict(g.meta["cases"][case])
    if "dtype" in kw:
        kw["dtype"] = getattr(torch, kw["dtype"].split(".")[-1])
    return RePaintSampler(den, g[f"{case}_y"], g[f"{case}_mask"], silent=True, **kw, **extra)


def test_api_mirrors_the_reference_signature(golden):
    from azula_amd.guidance import RePaintSampler
    from azula_amd.sample import DDIMSampler, Sampler

    g = golden("g25_repaint")
    ours = {"RePaintSampler": RePaintSampler, "DDIMSampler": DDIMSampler, "Sampler": Sampler}
    for cls_name, name, kind, default in g.meta["signature"]:
        p = inspect.signature(ours[cls_name].__init__).parameters[name]
        assert p.kind.name == kind, (cls_name, name)
        assert (None if p.default is inspect.Parameter.empty else repr(p.default)) == default, (cls_name, name)
    ref_names = [n for c, n, _, _ in g.meta["signature"] if c == "RePaintSampler"]
    assert list(inspect.signature(RePaintSampler.__init__).parameters)[1:] == ref_names
    s = RePaintSampler(None, torch.zeros(2), torch.ones(2, dtype=torch.bool), eta=0.5, steps=7)
    assert (s.iterations, s.eta, s.steps) == (3, 0.5, 7) and isinstance(s, DDIMSampler)


@pytest.mark.parametrize("case", TOY_CASES)
def test_host_run_equals_the_reference(golden, case):
    g = golden("g25_repaint")
    smp = make(toy_denoiser(g), g, case)
    torch.manual_seed(g.meta["loop_seed"])
    x0 = smp(g[f"{case}_x1"])
    state = torch.get_rng_state()
    after = torch.randn(4)
    ox0, ostate = restated(g, case)
    assert x0.dtype == ox0.dtype and torch.equal(x0, ox0), (x0 - ox0).abs().max()
    assert torch.equal(state, ostate)  # every one of the 3 * iterations draws per step, in order
    ref = g[f"{case}_x0"]
    assert close_to_reference(x0, ref), max_err(x0, ref)
    assert torch.allclose(after, g[f"{case}_randn_after"], rtol=1e-6, atol=1e-6)  # (the reference's generator state)


def test_a_subclass_that_overrides_step_computes_the_same(golden):
    from azula_amd.guidance import RePaintSampler

    class Logged(RePaintSampler):
        def step(self, x_t, t, s, **kw):
            return super().step(x_t, t, s, **kw)

    g = golden("g25_repaint")
    case = "toy_eta06_it2_bcast"
    kw = dict(g.meta["cases"][case])
    smp = Logged(toy_denoiser(g), g[f"{case}_y"], g[f"{case}_mask"], silent=True, **kw)
    assert not smp._fusable(torch.zeros(64, 5))
    torch.manual_seed(g.meta["loop_seed"])
    x0 = smp(g[f"{case}_x1"])
    assert torch.equal(x0, restated(g, case)[0]) and close_to_reference(x0, g[f"{case}_x0"])


def test_without_rng_parity_only_the_unread_draws_go(golden, monkeypatch):
    g = golden("g25_repaint")
    case = "toy_eta0_it3"
    smp = make(toy_denoiser(g), g, case)
    shapes = []
    orig = type(smp)._draw_noise
    monkeypatch.setattr(type(smp), "_draw_noise", lambda self, like, out=None: shapes.append(tuple(like.shape)) or orig(self, like, out))
    smp(g[f"{case}_x1"])
    steps, it = smp.steps, smp.iterations
    assert len(shapes) == 3 * it * steps and shapes[:3] == [(64, 5)] * 3
    shapes.clear()
    smp.rng_parity = False
    smp(g[f"{case}_x1"])
    # the host DDIM step draws its (unread, eta = 0) noise as before; only the discarded re-noise of the last iteration goes
    assert len(shapes) == (3 * it - 1) * steps


@pytest.mark.parametrize("case", ["toy_eta0_it3", "toy_eta06_it2_bcast", "unet_it3"])
def test_scalar_table_equals_the_reference_values(golden, case):
    from azula_amd.guidance import RePaintSampler
    from azula_amd.noise import VPSchedule

    g = golden("g25_repaint")
    den = type("D", (), {"schedule": VPSchedule()})()
    steps = g.meta["cases"][case]["steps"]
    smp = RePaintSampler(den, None, None, steps=steps)
    table = smp._repaint_table()
    assert table.dtype == torch.float32 and torch.equal(table, repaint_oracle.scalar_table(sampling.vp_schedule, steps=steps))
    assert torch.allclose(table, g[f"{case}_scalars"], rtol=1e-6, atol=0)  # (a few ulp: exp / sqrt of another CPU)


def test_fp64_clock_scalars_equal_the_reference_values(golden):
    from azula_amd.guidance import RePaintSampler
    from azula_amd.noise import VPSchedule

    g = golden("g25_repaint")
    den = type("D", (), {"schedule": VPSchedule()})()
    smp = RePaintSampler(den, None, None, steps=16, dtype=torch.float64)
    rows = torch.stack([torch.stack(smp._repaint_scalars(t, s)) for t, s in smp.timesteps.unfold(0, 2, 1).unbind()])
    assert rows.dtype == torch.float64
    assert torch.equal(rows, repaint_oracle.scalar_table(sampling.vp_schedule, steps=16, dtype=torch.float64))
    assert torch.allclose(rows, g["toy_f64_scalars"], rtol=1e-14, atol=0)


@pytest.mark.parametrize("eta,iterations,parity", [(0.0, 3, True), (0.5, 3, True), (0.0, 2, False), (0.7, 1, False), (0.0, 1, True)])
def test_captured_loop_rows_and_generator_order(golden, eta, iterations, parity):
    r"""What the captured loop would lay out, checked on the host: ``iterations`` table rows per step at time t whose c_in_next
    chains to c_in(t) between iterations and to c_in(s) after the last, and per step the draws [e_k or dummy, n_y_k, n_x_k
    or dummy] -- the unread ones only under ``rng_parity``."""
    from types import SimpleNamespace

    from azula_amd._lib import COEF_FIELDS
    from azula_amd.guidance import RePaintSampler
    from azula_amd.sample import FusedDenoiser

    g = golden("g25_repaint")
    den = toy_denoiser(g)
    smp = RePaintSampler(den, torch.zeros(4, 5), torch.zeros(1, 5, dtype=torch.bool), iterations=iterations, eta=eta, steps=5)
    smp.rng_parity = parity
    fused = FusedDenoiser(coefficients=den.host_coefficients, programs=[])
    rows = smp._host_table(fused)
    col = {n: i for i, n in enumerate(COEF_FIELDS)}
    assert rows.shape[0] == 5 * iterations
    ts = torch.linspace(1.0, 0.0, 6)
    for i in range(5):
        c_t = den.host_coefficients(*den.schedule(ts[i]))["c_in"]
        for k in range(iterations):
            r = rows[i * iterations + k]
            assert r[col["c_in"]] == c_t and r.view(torch.int32)[col["step"]] == i
            if i < 4 or k < iterations - 1:
                nxt = c_t if k < iterations - 1 else den.host_coefficients(*den.schedule(ts[i + 1]))["c_in"]
                assert r[col["c_in_next"]] == nxt.float()
    # generator order of one step
    n_read = smp._noise_draws()
    assert n_read == iterations * (2 + (eta != 0)) - 1
    bufs = [torch.empty(1) for _ in range(n_read)]
    loop = SimpleNamespace(noise=list(bufs), x=torch.zeros(4, 5), keep=[], cur=torch.zeros(16), table=torch.zeros(1, 16),
                           counter=torch.zeros(1), n_rows=1)
    it = iter(bufs)
    loop.rp_eps = [next(it) for _ in range(iterations)] if eta != 0 else [None] * iterations
    loop.rp_ny = [next(it) for _ in range(iterations)]
    loop.rp_nx = [next(it) for _ in range(iterations - 1)] + [None]
    loop.rp_dummy = torch.empty(1) if parity else None
    draws = smp._fused_draws(loop)
    expect = []
    for k in range(iterations):
        expect += [loop.rp_eps[k] if eta != 0 else loop.rp_dummy, loop.rp_ny[k],
                   loop.rp_nx[k] if k < iterations - 1 else loop.rp_dummy]
    expect = [b for b in expect if b is not None]
    assert [id(b) for b in draws] == [id(b) for b in expect]
    assert len(draws) == (3 * iterations if parity else n_read)


def test_default_draw_order_of_the_existing_samplers_is_unchanged():
    from types import SimpleNamespace

    from azula_amd.sample import DDIMSampler, PCSampler

    a, b, d = torch.empty(1), torch.empty(1), torch.empty(1)
    assert DDIMSampler(None)._fused_draws(SimpleNamespace(noise=[], dummy=d)) == [d]
    assert [id(x) for x in PCSampler(None, corrections=2)._fused_draws(SimpleNamespace(noise=[a, b], dummy=None))] == [id(a), id(b)]


def test_fusable_only_where_the_captured_loop_applies():
    from azula_amd.guidance import RePaintSampler

    x = torch.zeros(2, 3, 8, 8)
    y, m = torch.zeros_like(x), torch.zeros(1, 1, 8, 8, dtype=torch.bool)
    assert RePaintSampler(None, y, m)._fusable(x)
    assert RePaintSampler(None, y, m.expand(2, 3, 8, 8).clone())._fusable(x)
    assert not RePaintSampler(None, y[:1], m)._fusable(x)  # y of another shape: generic loop
    assert not RePaintSampler(None, y.double(), m)._fusable(x)
    assert not RePaintSampler(None, y, m.float())._fusable(x)
    assert RePaintSampler(None, y, torch.zeros(3, 1, 1, dtype=torch.bool))._fusable(x)  # (a per-channel mask)
    assert not RePaintSampler(None, y, torch.zeros(5, 1, 1, 1, dtype=torch.bool))._fusable(x)
    assert not RePaintSampler(None, y, torch.zeros(1, 2, 3, 8, 8, dtype=torch.bool))._fusable(x)  # would grow x
    assert not RePaintSampler(None, y, m, dtype=torch.float64)._fusable(x)
    assert not RePaintSampler(None, y, m, iterations=0)._fusable(x)
    # y and mask are copied per call: their values never key the coefficient table, hyper-parameters do
    s = RePaintSampler(None, y, m)
    h = s._hyper()
    s.y, s.mask = y + 1, ~m
    assert s._hyper() == h
    s.iterations = 2
    assert s._hyper() != h


def test_repaint_struct_size_matches_c():
    from azula_amd import _lib

    prog = '#include <stdio.h>\n#include "azula_amd.h"\nint main(void){printf("%zu\\n", sizeof(AzRepaintArgs));return 0;}'
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(src, "w").write(prog)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        size = int(subprocess.run([exe], check=True, capture_output=True, text=True).stdout)
    assert ctypes.sizeof(_lib.AzRepaintArgs) == size == 72


def test_repaint_entry_is_exported_prototyped_and_validates():
    from azula_amd import _lib
    from azula_amd.csrc import build

    handle = ctypes.CDLL(build.build())
    assert hasattr(handle, "az_repaint_f32") and "az_repaint_f32" in _lib.PROTOTYPES
    lib = _lib.lib()
    A = _lib.AzRepaintArgs
    ok = dict(x_s=0x1000, y=0x1000, mask=0x1000, n_y=0x1000, n_x=0x1000, x_s_out=0x1000, x_t_out=0x1000, coef=0x1000, n=16)
    call = lambda **kw: lib.az_repaint_f32(ctypes.byref(A(**{**ok, **kw})), None)  # noqa: E731
    assert call(y=None) == -1 and call(coef=None) == -1
    assert call(x_s_out=None, x_t_out=None) == -1  # no output at all
    assert call(n_x=None) == -1  # x_t' needs its noise
    assert call(n=0) == -2
    assert call(y=0x1004) == -3 and call(x_t_out=0x1008) == -3 and call(mask=0x1002) == -3
