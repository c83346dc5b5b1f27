r"""``azula_amd.linalg`` (``cg``, ``gmres``) and ``DiffPIRDenoiser`` (reference ``azula/linalg/solve.py``,
``azula/guidance/diffpir.py``) without a GPU: the public API against the reference's recorded signatures, host runs against
the restatement of ``tests/diffpir_oracle.py`` bit for bit and against G26 within round-off, the solvers' own properties,
and the C ABI of the Krylov entries.
"""

import ctypes
import inspect
import os
import subprocess
import tempfile

import pytest
import torch

import diffpir_oracle as do
from conftest import ROOT, max_err
from oracle import nets, sampling, synth

G = "g26_diffpir"


def close_to_reference(x: torch.Tensor, ref: torch.Tensor, rel: float = 1e-5) -> bool:
    r"""Within the round-off of torch's CPU kernels on another CPU (the outputs are fp32: a few ulp of the scale, bound 1e-5;
    the Krylov solves amplify the operator's rounding by at most the condition of the small systems)."""
    return x.dtype == ref.dtype and x.shape == ref.shape and max_err(x, ref) < rel * max(1.0, ref.abs().max().item())


def _solve_inputs(g, case):
    kw = g.meta["cases"][case]
    M = g[f"op_{kw['op']}"]
    b = g[f"solve_{kw['batch']}_b"]
    x0 = g[f"solve_{kw['batch']}_x0"] if kw["x0"] else None
    dtype = getattr(torch, kw["dtype"].split(".")[-1])
    return kw, do.row_matrix(M), b, x0, dtype


def _solve_cases(g):
    return [c for c in g.meta["cases"] if c.startswith("solve_")]


def test_api_mirrors_the_reference_signature(golden):
    from azula_amd.guidance import DiffPIRDenoiser
    from azula_amd.linalg import cg, gmres

    g = golden(G)
    ours = {"DiffPIRDenoiser.__init__": DiffPIRDenoiser.__init__, "cg": cg, "gmres": gmres}
    for qual, name, kind, default in g.meta["signature"]:
        p = inspect.signature(ours[qual]).parameters[name]
        assert p.kind.name == kind, (qual, name)
        assert (None if p.default is inspect.Parameter.empty else repr(p.default)) == default, (qual, name)
    for qual, fn in ours.items():
        names = [n for q, n, _, _ in g.meta["signature"] if q == qual]
        params = list(inspect.signature(fn).parameters)
        assert (params[1:] if qual.endswith("__init__") else params) == names, qual


def test_unknown_solver_raises():
    from azula_amd.guidance import DiffPIRDenoiser

    with pytest.raises(ValueError, match="Unknown solver 'lsqr'"):
        DiffPIRDenoiser(None, torch.zeros(3), lambda x: x, 1.0, solver="lsqr")
    d = DiffPIRDenoiser(None, torch.zeros(3), lambda x: x, 1.0, solver="cg", iterations=3)
    assert d.solve.keywords == {"iterations": 3} and d.lmbda == 10.0


def test_diffpir_is_exported_and_never_fused():
    import azula_amd.guidance as guidance
    from azula_amd.denoise import Denoiser

    assert "DiffPIRDenoiser" in dir(guidance)
    d = guidance.DiffPIRDenoiser(None, torch.zeros(3), lambda x: x, 1.0)
    assert isinstance(d, Denoiser) and d._az_fused(torch.zeros(2, 3), {}, None) is None


def test_host_solvers_equal_the_restatement_and_the_reference(golden):
    from azula_amd.linalg import cg, gmres

    g = golden(G)
    ours = {"cg": cg, "gmres": gmres}
    cases = _solve_cases(g)
    assert len(cases) >= 30
    for case in cases:
        kw, A, b, x0, dtype = _solve_inputs(g, case)
        x = ours[kw["solver"]](A, b, x0=x0, iterations=kw["iterations"], dtype=dtype)
        ox = do.SOLVERS[kw["solver"]](A, b, x0=x0, iterations=kw["iterations"], dtype=dtype)
        assert x.dtype == b.dtype and torch.equal(x, ox), case
        assert close_to_reference(x, g[case]), (case, max_err(x, g[case]))


@pytest.mark.parametrize("solver", ["cg", "gmres"])
@pytest.mark.parametrize("batch", [(), (64,), (3, 5)])
def test_exact_solve_at_iterations_equal_to_rank(golden, solver, batch):
    r"""b in the range of a rank-3 operator: the Krylov space has dimension 3, so three iterations solve exactly."""
    from azula_amd import linalg

    g = golden(G)
    rank = g.meta["rank"]
    M = g["op_spd" if solver == "cg" else "op_nonsym"].double()
    gen = torch.Generator().manual_seed(len(batch))
    x_true = torch.randn(*batch, g.meta["D"], generator=gen, dtype=torch.float64) @ (M.mT @ M)  # in the row space
    b = x_true @ M.mT
    x = getattr(linalg, solver)(lambda v: v @ M.mT, b, iterations=rank)
    assert max_err(x @ M.mT, b) < 1e-10 * max(1.0, b.abs().max().item())
    assert max_err(getattr(linalg, solver)(lambda v: v @ M.mT, b, iterations=rank - 1) @ M.mT, b) > 1e-6


@pytest.mark.parametrize("solver", ["cg", "gmres"])
def test_one_iteration_from_the_solution_stays_there(solver):
    from azula_amd import linalg

    gen = torch.Generator().manual_seed(4)
    Q = torch.randn(6, 6, generator=gen, dtype=torch.float64)
    M = Q @ Q.mT + torch.eye(6, dtype=torch.float64)
    x = torch.randn(5, 6, generator=gen, dtype=torch.float64)
    b = x @ M.mT
    out = getattr(linalg, solver)(lambda v: v @ M.mT, b, x0=x, iterations=1)
    assert max_err(out, x) < 1e-12
    assert torch.isfinite(getattr(linalg, solver)(lambda v: v @ M.mT, torch.zeros_like(b), iterations=2)).all()  # b = 0


@pytest.mark.parametrize("solver", ["cg", "gmres"])
def test_zero_iterations_and_type_promotion_follow_the_reference(solver):
    from azula_amd import linalg

    gen = torch.Generator().manual_seed(5)
    b = torch.randn(4, 6, generator=gen)
    M = torch.randn(6, 6, generator=gen) + 4 * torch.eye(6)
    out = getattr(linalg, solver)(lambda v: (v @ M.mT).double(), b, iterations=2, dtype=torch.float32)
    ref = do.SOLVERS[solver](lambda v: (v @ M.mT).double(), b, iterations=2, dtype=torch.float32)
    assert out.dtype == torch.float32 and torch.equal(out, ref)


# ------------------------------------------------------------------------------------------------------------- DiffPIR
class MeanDenoiser(torch.nn.Module):
    r"""A host denoiser from a posterior-mean function (the restated small UNet of the fixture)."""

    def __init__(self, mean_fn):
        super().__init__()
        from azula_amd.noise import VPSchedule

        self.mean_fn = mean_fn
        self.schedule = VPSchedule()

    def forward(self, x_t, t, **kwargs):
        from azula_amd.denoise import DiracPosterior

        return DiracPosterior(mean=self.mean_fn(x_t, t, **kwargs))


def unet_mean(g):
    cfg = g.meta["unet_cfg"]
    sd = synth.synth_state_dict({k: tuple(v) for k, v in g.meta["unet_shapes"].items()}, g.meta["unet_weight_seed"])
    return lambda x, t: sampling.karras_mean(lambda a, c: nets.time_wrapped_unet(sd, cfg, a, c), x, t)  # noqa: E731


def dp_operator(g, name):
    return {"mask": do.pixel_mask(g["dp_mask"]), "pool": do.avg_pool2, "rows": do.row_matrix(g["dp_rows"])}[name]


def test_host_diffpir_equals_the_restatement_and_the_reference(golden):
    from azula_amd.guidance import DiffPIRDenoiser

    g = golden(G)
    omean = unet_mean(g)
    x_t, t = g["dp_x_t"], g["dp_t"]
    mean = omean(x_t, t)
    alpha_t, sigma_t = sampling.vp_schedule(t)
    cases = [c for c in g.meta["cases"] if c.startswith("dp_")]
    assert len(cases) == 18
    for case in cases:
        kw = g.meta["cases"][case]
        A, y = dp_operator(g, kw["op"]), g[f"dp_{kw['op']}_y"]
        var_y = 0.05 if kw["var_y"] == "float" else torch.tensor(0.05)
        den = DiffPIRDenoiser(MeanDenoiser(omean), y, A, var_y, solver=kw["solver"], iterations=kw["iterations"])
        out = den(x_t, t).mean
        ref = do.diffpir_mean(mean, alpha_t, sigma_t, y, A, var_y, 10.0, kw["solver"], kw["iterations"])
        assert torch.equal(out, ref), case
        assert close_to_reference(out, g[case]), (case, max_err(out, g[case]))


def test_host_ddim_loop_with_diffpir(golden):
    from azula_amd.guidance import DiffPIRDenoiser
    from azula_amd.sample import DDIMSampler

    g = golden(G)
    lp = g.meta["loop"]
    omean = unet_mean(g)
    A = dp_operator(g, lp["op"])
    den = DiffPIRDenoiser(MeanDenoiser(omean), g["loop_y"], A, lp["var_y"], lmbda=lp["lmbda"], solver=lp["solver"],
                          iterations=lp["iterations"])
    torch.manual_seed(lp["seed"])
    x0 = DDIMSampler(den, steps=lp["steps"], eta=lp["eta"], silent=True)(g["loop_x1"])
    torch.manual_seed(lp["seed"])
    ref = sampling.sample(do.diffpir_fn(omean, g["loop_y"], A, lp["var_y"], lmbda=lp["lmbda"], solver=lp["solver"],
                                        iterations=lp["iterations"]), g["loop_x1"], steps=lp["steps"], eta=lp["eta"])
    assert torch.equal(x0, ref)
    assert close_to_reference(x0, g["loop_x0"], rel=1e-4), max_err(x0, g["loop_x0"])


def test_y_A_and_var_y_are_read_on_every_call(golden):
    from azula_amd.guidance import DiffPIRDenoiser

    g = golden(G)
    omean = unet_mean(g)
    x_t, t = g["dp_x_t"], g["dp_t"]
    den = DiffPIRDenoiser(MeanDenoiser(omean), g["dp_mask_y"], dp_operator(g, "mask"), 0.05)
    first = den(x_t, t).mean
    den.y, den.A, den.var_y = g["dp_pool_y"], do.avg_pool2, torch.tensor(0.05)
    alpha_t, sigma_t = sampling.vp_schedule(t)
    ref = do.diffpir_mean(omean(x_t, t), alpha_t, sigma_t, g["dp_pool_y"], do.avg_pool2, torch.tensor(0.05))
    out = den(x_t, t).mean
    assert torch.equal(out, ref) and not torch.equal(out, first)


# ------------------------------------------------------------------------------------------------------------- C ABI
def test_krylov_struct_layouts_match_c():
    from azula_amd import _lib

    names = ["AzCgArgs", "AzGmresArgs"]
    prog = '#include <stdio.h>\n#include "azula_amd.h"\nint main(void){' + "".join(
        f'printf("%zu\\n", sizeof({n}));' for n in names) + 'printf("%d\\n", AZ_KRYLOV_GMRES_MAX);return 0;}'
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(src, "w").write(prog)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        vals = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    for n, sz in zip(names, vals):
        assert ctypes.sizeof(getattr(_lib, n)) == sz, n
    from azula_amd.linalg import solve

    assert vals[2] == solve.GMRES_MAX


@pytest.fixture(scope="module")
def built_lib():
    from azula_amd.csrc import build

    return build.build()


def test_krylov_symbols_and_argument_errors(built_lib):
    from azula_amd import _lib

    lib = _lib.lib()
    for name in ("az_krylov_segments", "az_cg_init", "az_cg_step", "az_gmres_init", "az_gmres_arnoldi", "az_gmres_finish"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
    seg = lib.az_krylov_segments
    assert (seg(0), seg(1), seg(256), seg(1024), seg(1025), seg(196608)) == (0, 1, 1, 1, 2, 192)
    P = 0x1000
    cg = _lib.AzCgArgs(r0=P, x=P, r=P, p=P, rr=P, rr_out=P + 8, p_io=P, rows=4, dim=256)
    assert lib.az_cg_init(None, None) == -1
    cg.dim = 0
    assert lib.az_cg_init(ctypes.byref(cg), None) == -2  # AZ_E_SHAPE
    cg.dim, cg.state_dtype, cg.io_dtype = 256, 0, 1
    assert lib.az_cg_init(ctypes.byref(cg), None) == -4  # fp64 io with fp32 state
    cg.state_dtype, cg.in_dtype = 1, 2
    assert lib.az_cg_init(ctypes.byref(cg), None) == -4  # unknown dtype code
    cg.in_dtype, cg.dim = 0, 4096
    assert lib.az_cg_init(ctypes.byref(cg), None) == -1  # long rows need the partial-sum scratch
    cg.dim = 256
    assert lib.az_cg_step(ctypes.byref(cg), None) == -1  # no Ap
    cg.Ap, cg.rr_out = P, P
    assert lib.az_cg_step(ctypes.byref(cg), None) == -4  # rr_out aliases rr
    gm = _lib.AzGmresArgs(r0=P, V=P, H=P, cs=P, ss=P, B=P, v_io=P, w=P, rows=4, dim=256, iterations=33)
    assert lib.az_gmres_init(ctypes.byref(gm), None) == -4  # over AZ_KRYLOV_GMRES_MAX
    gm.iterations, gm.j = 4, 4
    assert lib.az_gmres_arnoldi(ctypes.byref(gm), None) == -2  # j >= iterations
    gm.j, gm.dim = 0, 2048
    assert lib.az_gmres_arnoldi(ctypes.byref(gm), None) == -1  # long rows: partial and work
    gm.dim = 256
    assert lib.az_gmres_finish(ctypes.byref(gm), None) == -1  # no out
