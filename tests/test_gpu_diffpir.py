r"""``azula_amd.linalg`` and ``DiffPIRDenoiser`` on the GPU: the Krylov kernels against the device torch op sequence (short
and long rows, every leading shape, ``x0``, iterations up to the GMRES cap, b = 0), batch and run invariance, the fallbacks,
and DiffPIR on the UNet / ADM / CFG denoisers against the restatement of ``tests/diffpir_oracle.py``, in a DDIM loop fed the
noise the device drew, and under an fp64 clock.

The operators are well away from convergence at the iteration counts tested: past it, GMRES's later basis vectors are
rounding noise in the reference as much as here, and two reduction orders would agree only through the tiny weights the
back-substitution gives them."""

import pytest
import torch

import diffpir_oracle as do
from conftest import max_err
from oracle import nets, sampling, synth

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------- operators
def _diag(D, gen, dtype, spread):
    return (10 ** (-spread * torch.rand(D, generator=gen)) if spread else 0.5 + torch.rand(D, generator=gen)).to(dtype).cuda()


def _spd(D, dtype=torch.float32, seed=0, spread=0.0):
    r"""x -> d * x + (x . u) u per row: symmetric positive definite, any row length."""
    gen = torch.Generator().manual_seed(seed)
    d = _diag(D, gen, dtype, spread)
    u = (torch.randn(D, generator=gen) / D**0.5).to(dtype).cuda()
    return lambda x: d.to(x) * x + (x @ u.to(x))[..., None] * u.to(x)


def _nonsym(D, dtype=torch.float32, seed=1, spread=0.0):
    r"""x -> d * x + (x . u) w per row: non-symmetric."""
    gen = torch.Generator().manual_seed(seed)
    d = _diag(D, gen, dtype, spread)
    u, w = ((torch.randn(D, generator=gen) / D**0.5).to(dtype).cuda() for _ in range(2))
    return lambda x: d.to(x) * x + (x @ u.to(x))[..., None] * w.to(x)


def _local(solver, D):
    r"""Elementwise operators (no reduction inside A, so its output does not depend on the batch either): a symmetric
    circulant for CG, a non-symmetric one for GMRES."""
    gen = torch.Generator().manual_seed(D)
    d = (0.5 + torch.rand(D, generator=gen)).cuda()
    if solver == "cg":
        return lambda x: (d + 0.6) * x + 0.2 * (torch.roll(x, 1, -1) + torch.roll(x, -1, -1))
    return lambda x: d * x + 0.3 * torch.roll(x, 1, -1)


def _ops(solver):
    from azula_amd.linalg import solve

    return solve._cg_ops if solver == "cg" else solve._gmres_ops


def _kernel(solver):
    from azula_amd.linalg import cg, gmres

    return cg if solver == "cg" else gmres


def _bound(b_dtype, state):
    if b_dtype == torch.float64:
        return 1e-12  # fp64 throughout: only the reduction order differs
    return 4e-7 if state == torch.float64 else 2e-5  # fp32 output: one rounding of an fp64 state; fp32 state: its round-off


def _spy(monkeypatch):
    from azula_amd import _lib

    names, call = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (names.append(name), call(name, *a))[1])
    return names


@pytest.mark.parametrize("solver", ["cg", "gmres"])
@pytest.mark.parametrize("D", [1, 37, 64, 256, 1000, 1024, 1025, 5000])
@pytest.mark.parametrize("lead", [(), (3,), (2, 5)])
def test_kernels_match_the_device_op_sequence(solver, D, lead):
    gen = torch.Generator().manual_seed(D)
    b = torch.randn(*lead, D, generator=gen).cuda()
    x0 = 0.1 * torch.randn(*lead, D, generator=gen).cuda()
    A = (_spd if solver == "cg" else _nonsym)(D)
    for state in (torch.float64, torch.float32):
        for it, with_x0 in ((1, False), (1, True), (3, True), (6, False)):
            if it > D:
                continue
            kw = dict(x0=x0 if with_x0 else None, iterations=it, dtype=state)
            out, ref = _kernel(solver)(A, b, **kw), _ops(solver)(A, b, **kw)
            assert out.shape == b.shape and out.dtype == b.dtype
            err, sc = max_err(out, ref), max(1.0, ref.abs().max().item())
            assert err <= _bound(b.dtype, state) * sc, (solver, D, lead, state, it, with_x0, err)


@pytest.mark.parametrize("solver", ["cg", "gmres"])
def test_long_rows_and_fp64_b(solver):
    r"""Rows of 196608 (a flattened 3 x 256 x 256 image): the segmented regime; and fp64 b with fp64 state."""
    D = 3 * 256 * 256
    gen = torch.Generator().manual_seed(9)
    make = _spd if solver == "cg" else _nonsym
    A = make(D)
    b = torch.randn(2, D, generator=gen).cuda()
    for it in (1, 4):
        out, ref = _kernel(solver)(A, b, iterations=it), _ops(solver)(A, b, None, it, torch.float64)
        assert max_err(out, ref) <= 4e-7 * max(1.0, ref.abs().max().item()), (it, max_err(out, ref))
    for Dn, rows in ((D, 2), (256, 7)):
        bb = torch.randn(rows, Dn, generator=gen, dtype=torch.float64).cuda()
        A64 = make(Dn, torch.float64)
        out, ref = _kernel(solver)(A64, bb, x0=0.1 * bb, iterations=3), _ops(solver)(A64, bb, 0.1 * bb, 3, torch.float64)
        assert out.dtype == torch.float64
        assert max_err(out, ref) <= 1e-12 * max(1.0, ref.abs().max().item()), (Dn, max_err(out, ref))


@pytest.mark.parametrize("D", [256, 4000])
def test_gmres_up_to_the_cap(D):
    from azula_amd.linalg import gmres, solve

    gen = torch.Generator().manual_seed(D)
    b = torch.randn(4, D, generator=gen).cuda()
    A = _nonsym(D, spread=3.0)  # spectrum over three decades: far from converged at 32 iterations
    for it in (2, 8, 16, solve.GMRES_MAX):
        out, ref = gmres(A, b, iterations=it), _ops("gmres")(A, b, None, it, torch.float64)
        assert max_err(out, ref) <= 4e-7 * max(1.0, ref.abs().max().item()), (it, max_err(out, ref))


@pytest.mark.parametrize("solver", ["cg", "gmres"])
@pytest.mark.parametrize("D", [256, 3000])
def test_zero_rhs_gives_no_nan(solver, D):
    b = torch.zeros(3, D, device="cuda")
    A = (_spd if solver == "cg" else _nonsym)(D)
    for state in (torch.float64, torch.float32):
        out = _kernel(solver)(A, b, iterations=3, dtype=state)
        assert torch.equal(out, torch.zeros_like(b))
        assert torch.equal(out, _ops(solver)(A, b, None, 3, state))


@pytest.mark.parametrize("solver", ["cg", "gmres"])
@pytest.mark.parametrize("D", [100, 256, 2500])
def test_a_row_is_solved_the_same_in_any_batch_and_run(solver, D):
    gen = torch.Generator().manual_seed(D + 1)
    b = torch.randn(9, D, generator=gen).cuda()
    A = _local(solver, D)
    full = _kernel(solver)(A, b, iterations=4)
    assert torch.equal(full, _kernel(solver)(A, b, iterations=4))
    for r in (0, 4, 8):
        alone = _kernel(solver)(A, b[r].clone(), iterations=4)
        assert torch.equal(alone, full[r]), (r, max_err(alone, full[r]))
    part = _kernel(solver)(A, b[3:6].contiguous().reshape(3, 1, D), iterations=4)
    assert torch.equal(part.reshape(3, D), full[3:6])


def test_kernel_entries_run_on_the_device(monkeypatch):
    from azula_amd.linalg import cg, gmres

    names = _spy(monkeypatch)
    b = torch.randn(4, 256, device="cuda")
    cg(_spd(256), b, iterations=3)
    gmres(_nonsym(256), b, iterations=3)
    assert names == ["az_cg_init"] + ["az_cg_step"] * 3 + ["az_gmres_init"] + ["az_gmres_arnoldi"] * 3 + ["az_gmres_finish"]


@pytest.mark.parametrize("case", ["over_cap", "half_b", "b64_state32", "strided", "grad"])
def test_cases_the_kernels_do_not_take_match_the_fallback(case, monkeypatch):
    from azula_amd.linalg import gmres, solve

    names = _spy(monkeypatch)
    gen = torch.Generator().manual_seed(3)
    b = torch.randn(4, 64, generator=gen).cuda()
    A, it, dtype = _nonsym(64), 2, None
    if case == "over_cap":
        it = solve.GMRES_MAX + 1
    elif case == "half_b":
        b = b.half()
    elif case == "b64_state32":
        b, dtype = b.double(), torch.float32
    elif case == "strided":
        b = torch.randn(64, 4, generator=gen).cuda().mT
    with torch.enable_grad():
        if case == "grad":
            b.requires_grad_()
        out = gmres(A, b, iterations=it, dtype=dtype)
        ref = _ops("gmres")(A, b, None, it, dtype or torch.float64)
    assert not names and torch.equal(out, ref)


def test_operator_output_of_another_dtype():
    r"""``A`` returning fp64 (or fp16) for an fp32 input: promoted as the reference's ``.to(dtype)``."""
    from azula_amd.linalg import cg

    b = torch.randn(5, 300, device="cuda")
    base = _spd(300)
    for A in (lambda v: base(v).double(), lambda v: base(v).half()):
        out, ref = cg(A, b, iterations=3), _ops("cg")(A, b, None, 3, torch.float64)
        assert max_err(out, ref) <= 4e-7 * max(1.0, ref.abs().max().item())


# ------------------------------------------------------------------------------------------------------------- DiffPIR
def _unet(golden):
    from test_gpu_fp64 import unet_denoiser

    g = golden("g26_diffpir")
    cfg = g.meta["unet_cfg"]
    sd = synth.synth_state_dict({k: tuple(v) for k, v in g.meta["unet_shapes"].items()}, g.meta["unet_weight_seed"])
    omean = lambda x, t: sampling.karras_mean(lambda a, c: nets.time_wrapped_unet(sd, cfg, a, c), x, t)  # noqa: E731
    return g, unet_denoiser(g), omean


def _operators(g, device="cuda"):
    return {"mask": do.pixel_mask(g["dp_mask"].to(device)), "pool": do.avg_pool2, "rows": do.row_matrix(g["dp_rows"].to(device))}


@pytest.mark.parametrize("solver", ["cg", "gmres"])
@pytest.mark.parametrize("op", ["mask", "pool", "rows"])
def test_diffpir_on_the_unet_matches_the_restatement(golden, solver, op, monkeypatch):
    from azula_amd.guidance import DiffPIRDenoiser

    g, den, omean = _unet(golden)
    x_t, t = g["dp_x_t"], g["dp_t"]
    alpha_t, sigma_t = sampling.vp_schedule(t)
    mean = omean(x_t, t)
    names = _spy(monkeypatch)
    for it in (1, 4):
        for var_y in (0.05, torch.tensor(0.05)):
            dp = DiffPIRDenoiser(den, g[f"dp_{op}_y"].cuda(), _operators(g)[op], var_y, solver=solver, iterations=it)
            out = dp(x_t.cuda(), t.cuda()).mean
            ref = do.diffpir_mean(mean, alpha_t, sigma_t, g[f"dp_{op}_y"], _operators(g, "cpu")[op], var_y, 10.0, solver, it)
            err, sc = max_err(out, ref), max(1.0, ref.abs().max().item())
            print(f"DiffPIR {op} {solver} it {it}: max|d|", err, "scale", sc)
            assert out.dtype == torch.float32 and err < 5e-4 * sc
    assert f"az_{solver}_init" in names and not out.requires_grad


def test_diffpir_on_adm_and_cfg(golden):
    from test_gpu_adm import _adm_oracle, build

    from azula_amd.guidance import CFGDenoiser, DiffPIRDenoiser

    g = golden("g5_adm_uncond")
    den, sd, cfg = build(g)
    omean, sched = _adm_oracle(g, sd, cfg)
    x = g["x1"]
    t = torch.tensor(0.5)
    gen = torch.Generator().manual_seed(2)
    mask = (torch.rand(1, 1, *x.shape[2:], generator=gen) < 0.5).float()
    y = (torch.rand(x.shape, generator=gen) - 0.5) * mask
    alpha_t, sigma_t = sched(t)
    for solver in ("cg", "gmres"):
        out = DiffPIRDenoiser(den, y.cuda(), do.pixel_mask(mask.cuda()), 0.1, solver=solver, iterations=2)(x.cuda(), t.cuda()).mean
        ref = do.diffpir_mean(omean(x, t), alpha_t, sigma_t, y, do.pixel_mask(mask), 0.1, 10.0, solver, 2)
        err, sc = max_err(out, ref), max(1.0, ref.abs().max().item())
        print(f"ADM DiffPIR {solver}: max|d|", err, "scale", sc)
        assert err < 5e-4 * sc

    # a CFG inner denoiser: the keyword arguments reach it; the result is DiffPIR of the guided mean
    gc = golden("g5_adm_cond_neworder")
    den_c, _, _ = build(gc)
    cfgden = CFGDenoiser(den_c)
    xc = gc["x1"].cuda()
    kwargs = dict(positive={"label": gc["y"].cuda()}, negative={"label": gc["neg_label"].cuda()}, guidance=2.0)
    yc = do.avg_pool2(torch.zeros_like(xc) + 0.3)
    out = DiffPIRDenoiser(cfgden, yc, do.avg_pool2, 0.1, solver="gmres", iterations=2)(xc, t.cuda(), **kwargs).mean
    q = cfgden(xc, t.cuda(), **kwargs).mean
    a_t, s_t = (v.double().cpu() for v in cfgden.schedule(t.cuda()))
    ref = do.diffpir_mean(q.double().cpu(), a_t, s_t, yc.double().cpu(), do.avg_pool2, 0.1, 10.0, "gmres", 2)
    err = max_err(out, ref)
    print("CFG DiffPIR vs restatement on the device's guided mean: max|d|", err)
    assert err < 1e-4 * max(1.0, ref.abs().max().item())


def _device_noise(seed, steps, shape, dtype=torch.float32):
    r"""The DDIM loop's randn_like per step, drawn on the device (an fp64 clock: fp64 from the second step on)."""
    torch.manual_seed(seed)
    return [torch.randn(shape, device="cuda", dtype=torch.float32 if i == 0 else dtype).cpu() for i in range(steps)]


def test_ddim_loop_with_diffpir_matches_the_restatement(golden, monkeypatch):
    from azula_amd.guidance import DiffPIRDenoiser
    from azula_amd.sample import DDIMSampler

    g, den, omean = _unet(golden)
    lp = g.meta["loop"]
    names = _spy(monkeypatch)
    dp = DiffPIRDenoiser(den, g["loop_y"].cuda(), _operators(g)[lp["op"]], lp["var_y"], lmbda=lp["lmbda"],
                         solver=lp["solver"], iterations=lp["iterations"])
    smp = DDIMSampler(dp, steps=lp["steps"], eta=lp["eta"], silent=True)
    torch.manual_seed(lp["seed"])
    x0 = smp(g["loop_x1"].cuda())
    assert not smp._fused_cache  # DiffPIR runs the generic loop: never captured
    assert names.count("az_gmres_arnoldi") == lp["steps"] * lp["iterations"] and "az_step_begin" not in names
    noise = _device_noise(lp["seed"], lp["steps"], g["loop_x1"].shape)
    fn = do.diffpir_fn(omean, g["loop_y"], _operators(g, "cpu")[lp["op"]], lp["var_y"], lmbda=lp["lmbda"],
                       solver=lp["solver"], iterations=lp["iterations"])
    ref = sampling.sample(fn, g["loop_x1"], steps=lp["steps"], eta=lp["eta"], eps_list=noise)
    err, sc = max_err(x0, ref), max(1.0, ref.abs().max().item())
    print("DDIM-8 DiffPIR vs restatement: max|d|", err, "scale", sc)
    assert err < 5e-4 * sc


def test_fp64_clock(golden):
    from azula_amd.guidance import DiffPIRDenoiser
    from azula_amd.sample import DDIMSampler

    g, den, omean = _unet(golden)
    lp = g.meta["loop"]
    dp = DiffPIRDenoiser(den, g["loop_y"].cuda(), _operators(g)[lp["op"]], lp["var_y"], solver="cg", iterations=2)
    smp = DDIMSampler(dp, steps=4, eta=lp["eta"], silent=True, dtype=torch.float64)
    torch.manual_seed(3)
    x0 = smp(g["loop_x1"].cuda())
    assert x0.dtype == torch.float64 and not smp._fused_cache
    noise = _device_noise(3, 4, g["loop_x1"].shape, dtype=torch.float64)
    fn = do.diffpir_fn(omean, g["loop_y"], _operators(g, "cpu")[lp["op"]], lp["var_y"], solver="cg", iterations=2)
    ref = sampling.sample(fn, g["loop_x1"], steps=4, eta=lp["eta"], eps_list=noise, dtype=torch.float64)
    err, sc = max_err(x0, ref), max(1.0, ref.abs().max().item())
    print("fp64 clock DiffPIR vs restatement: max|d|", err, "scale", sc)
    assert ref.dtype == torch.float64 and err < 5e-4 * sc
