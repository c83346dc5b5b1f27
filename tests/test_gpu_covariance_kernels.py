r"""``az_cov_scale``, ``az_cov_project``, ``az_cov_expand`` and ``az_cov_mode`` (csrc/covariance.hip) on the GPU, through ctypes, at
shapes on both sides of every tile constant and in all four (x, factor) dtype pairs.  Cases, input families, references and the
bound live in tests/covariance_cases.py (the derivation is in its docstring); test_covariance_host.py shows on the CPU that the
exact cases notice a dropped, doubled or misplaced term and that the hard bound can be met.

Every case runs in both families: ``exact`` (small integers: the device must EQUAL the integer reference) and ``hard`` (three
decades of magnitude: ``|out - ref| <= gamma_k S`` per output against the long-double reference).  Every call reads its operands
from slices that start at an odd element of a buffer otherwise full of NaN and writes into slices of buffers otherwise full of a
sentinel: afterwards every guard element still holds the sentinel and no output element does (``P`` and ``partial`` included),
and a second run gives the same bits.  Nothing is compared with a kernel's own output except for that and for the batch
invariance.  Each hard case prints ``err``, its worst ratio err / bound and the entry's worst so far; DESIGN.md holds the largest
ratio per entry."""

import ctypes as C

import numpy as np
import pytest
import torch

import covariance_cases as cc
from azula_amd import _lib

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

F32, F64 = torch.float32, torch.float64
SENTINEL = -12345.5  # no integer and no quarter below 2^24 in size: never a value of the exact family
PAD = 5              # guard elements behind a slice; 1 or 3 in front
WORST = {}           # entry -> largest err / bound of the hard cases run so far


def bits(t):
    return t.view(torch.int32 if t.dtype == F32 else torch.int64)


def dev_in(t, off=1):
    r"""``t`` on the device as a slice that starts ``off`` (odd) elements into a buffer of NaN."""
    if t is None:
        return None
    buf = torch.full((off + t.numel() + PAD,), float("nan"), dtype=t.dtype, device="cuda")
    view = buf[off : off + t.numel()]
    view.copy_(t.reshape(-1))
    return view


class Out:
    def __init__(self, shape, dtype, off=3):
        self.shape, self.numel, self.off = tuple(shape), int(np.prod(shape)), off
        self.buf = torch.full((off + self.numel + PAD,), SENTINEL, dtype=dtype, device="cuda")
        self.view = self.buf[off : off + self.numel]

    def ptr(self):
        return self.view.data_ptr()

    def check(self, name):
        assert bool((self.buf[: self.off] == SENTINEL).all()) and bool((self.buf[self.off + self.numel :] == SENTINEL).all()), (
            name, "a guard element was written")
        assert not bool((self.view == SENTINEL).any()), (name, "an output element was not written")

    def cpu(self):
        return self.view.reshape(self.shape).cpu()


def ptr(t):
    return None if t is None else t.data_ptr()


def launch(entry, args):
    _lib.call(entry, C.byref(args), _lib.stream_ptr())


def run_project(case, inp):
    rows, (n, r) = inp["x"].shape[0], inp["W"].shape
    od = cc.out_dtype(case)
    x, W, c = dev_in(inp["x"]), dev_in(inp["W"], 3), dev_in(inp["c"])
    nseg = _lib.lib().az_cov_segments(n)
    assert nseg == cc.segments(n)
    outs = {"P": Out((rows, r), od)}
    if nseg > 1:
        outs["partial"] = Out((nseg, rows, r), od, off=1)
    a = _lib.AzCovLowRankArgs(x=ptr(x), W=ptr(W), c=ptr(c), P=outs["P"].ptr(), partial=outs["partial"].ptr() if nseg > 1 else None,
                              rows=rows, n=n, r=r, x_dtype=cc.CODE[inp["x"].dtype], f_dtype=cc.CODE[inp["W"].dtype],
                              out_dtype=cc.CODE[od])
    launch("az_cov_project", a)
    return outs


def run_expand(case, inp):
    rows, (n, r) = inp["P"].shape[0], inp["W"].shape
    od = cc.out_dtype(case)
    assert inp["P"].dtype == od
    ops = {k: dev_in(inp[k], off) for k, off in (("x", 1), ("W", 3), ("a", 1), ("d", 3), ("g", 1), ("P", 3))}
    outs = {"y": Out((rows, n), od)}
    a = _lib.AzCovLowRankArgs(x=ptr(ops["x"]), W=ptr(ops["W"]), a=ptr(ops["a"]), d=ptr(ops["d"]), g=ptr(ops["g"]), P=ptr(ops["P"]),
                              y=outs["y"].ptr(), d0=inp["d0"], s=inp["s"], rows=rows, n=n, r=r, x_dtype=cc.CODE[cc.DT[case.xd]],
                              f_dtype=cc.CODE[inp["W"].dtype], out_dtype=cc.CODE[od])
    launch("az_cov_expand", a)
    return outs


def run_mode(case, inp):
    outer, n, inner = inp["x"].shape
    od = cc.out_dtype(case)
    x, Q = dev_in(inp["x"]), dev_in(inp["Q"], 3)
    outs = {"y": Out((outer, n, inner), od)}
    a = _lib.AzCovModeArgs(x=ptr(x), Q=ptr(Q), y=outs["y"].ptr(), outer=outer, n=n, inner=inner, transpose=case.transpose,
                           x_dtype=cc.CODE[inp["x"].dtype], f_dtype=cc.CODE[inp["Q"].dtype], out_dtype=cc.CODE[od])
    launch("az_cov_mode", a)
    return outs


def run_scale(case, inp):
    rows, n = inp["x"].shape
    od = cc.out_dtype(case)
    e, u, v, k_dev, rho_dev = (dev_in(inp[k], off) for k, off in (("e", 3), ("u", 1), ("v", 3), ("k_dev", 1), ("rho_dev", 3)))
    if case.alias:  # y starts out holding x
        y = Out((rows, n), od)
        y.view.copy_(inp["x"].reshape(-1))
        x = y.view
    else:
        y, x = Out((rows, n), od), dev_in(inp["x"])
    a = _lib.AzCovScaleArgs(x=ptr(x), e=ptr(e), u=ptr(u), v=ptr(v), k_dev=ptr(k_dev), rho_dev=ptr(rho_dev), y=y.ptr(), k=inp["k"],
                            rho=inp["rho"], rows=rows, n=n, e_len=1 if e is None else e.numel(), h=case.h,
                            x_dtype=cc.CODE[inp["x"].dtype], f_dtype=cc.CODE[cc.DT[case.fd]], out_dtype=cc.CODE[od],
                            scalar_dtype=cc.CODE[cc.DT[case.sd]])
    launch("az_cov_scale", a)
    return {"y": y}


RUN = {"project": run_project, "expand": run_expand, "mode": run_mode, "scale": run_scale}
MAIN = {"project": "P", "expand": "y", "mode": "y", "scale": "y"}


def run_twice(case, inp):
    r"""The main output on the CPU (and all outputs), after the guard checks and a second run with the same bits."""
    entry = cc.entry_of(case)
    outs, again = RUN[entry](case, inp), RUN[entry](case, inp)
    torch.cuda.synchronize()
    for name, o in outs.items():
        o.check(name)
        assert torch.equal(bits(o.buf), bits(again[name].buf)), (name, "a second run differs")
    got = outs[MAIN[entry]].cpu()
    assert got.dtype == cc.out_dtype(case)
    return got, outs


def check_exact(case):
    inp = cc.inputs(case, "exact")
    got, outs = run_twice(case, inp)
    ref = torch.from_numpy(np.ascontiguousarray(cc.reference(case, inp, dt=np.float64)))
    assert got.shape == ref.shape
    if not torch.equal(got.double(), ref):
        bad = (got.double() != ref).nonzero()
        raise AssertionError((cc.case_id(case), "differs from the integer reference", len(bad), "outputs, first at", bad[0].tolist()))
    if "partial" in outs:
        assert torch.equal(outs["partial"].cpu().double(), torch.from_numpy(cc.project_partials(inp)))


def check_hard(case):
    inp = cc.inputs(case, "hard")
    got, _ = run_twice(case, inp)
    assert bool(torch.isfinite(got).all())
    ratio, err = cc.worst_ratio(got, cc.reference(case, inp), cc.bound(case, inp))
    entry = "az_cov_" + cc.entry_of(case)
    WORST[entry] = max(WORST.get(entry, 0.0), ratio)
    print(f"COV {entry} {cc.case_id(case)}: err {err:.3e} worst err / bound {ratio:.4f} (entry so far {WORST[entry]:.4f})")
    assert ratio <= 1.0, (cc.case_id(case), err, ratio)


@pytest.mark.parametrize("case", cc.PROJECT_CASES, ids=cc.case_id)
def test_project(case):
    check_exact(case)
    check_hard(case)


@pytest.mark.parametrize("case", cc.EXPAND_CASES, ids=cc.case_id)
def test_expand(case):
    check_exact(case)
    check_hard(case)


@pytest.mark.parametrize("case", cc.MODE_CASES, ids=cc.case_id)
def test_mode(case):
    check_exact(case)
    check_hard(case)


@pytest.mark.parametrize("case", cc.SCALE_CASES, ids=cc.case_id)
def test_scale(case):
    check_exact(case)
    check_hard(case)


# ---------------------------------------------------------------------------------------------------- the gridDim.x stride
def test_scale_strides_over_the_feature_blocks():
    r"""One row of 256 * 65536 + 5 features: the last five are reached only by the grid stride.  Integer data built on the device
    (periods 9, 7, 5 and 11: 2^24 is no multiple of any), the reference from torch's fp64 elementwise ops on the device."""
    n = cc.STRIDE_X_N
    i = torch.arange(n, device="cuda")
    x, e, u, v = (i % 9 - 4).float(), (i % 2 * 2 + 1).float(), (i % 7 - 3).float(), (i % 5 - 2).float()  # e in {1, 3}
    del i
    case = cc.Scale(n, 1, cc.H_POSTERIOR, "n", 1, 1, "host", "host", "f32", 0, "f32", "f32")
    ref = cc.scale_eval(case, F64, x=x, e=e.double(), u=u.double(), v=v.double(), k=-2.0, rho=1.0, k_dev=None, rho_dev=None)
    outs = []
    for _ in range(2):
        y = Out((1, n), F32)
        a = _lib.AzCovScaleArgs(x=ptr(x), e=ptr(e), u=ptr(u), v=ptr(v), y=y.ptr(), k=-2.0, rho=1.0, rows=1, n=n, e_len=n, h=case.h)
        launch("az_cov_scale", a)
        outs.append(y)
    torch.cuda.synchronize()
    outs[0].check("y")
    assert torch.equal(outs[0].view.double(), ref.reshape(-1)), "differs from the fp64 evaluation (every value is a quarter: exact)"
    assert torch.equal(bits(outs[0].buf), bits(outs[1].buf))
    assert float(ref.reshape(-1)[-5:].abs().max()) > 0


# ------------------------------------------------------------------------------------------------------- special values
@pytest.mark.parametrize("h,what", [(cc.H_INV, "zero_e"), (cc.H_POSTERIOR, "zero_e_and_rho"), (cc.H_SQRT, "negative_e")])
def test_scale_special_values_follow_torch(h, what):
    r"""e = 0 under 1 / e, e = rho = 0 under e / (e + rho), e < 0 under the square root: NaN and the infinities (with their
    signs) where torch's fp32 evaluation of the same expression on the device has them, position for position; the bound
    elsewhere."""
    n, rows = 257, 3
    case = cc.Scale(n, rows, h, "n", 1, 1, "host", "host", "f32", 0, "f32", "f32")
    inp = dict(cc.inputs(case, "hard"))
    e = inp["e"].clone()
    hit = torch.arange(n) % 3 == 0
    e[hit] = -e[hit].abs() if what == "negative_e" else 0.0
    inp["e"] = e
    inp["x"], inp["u"] = inp["x"].clone(), inp["u"].clone()
    inp["x"][0, 0], inp["u"][0] = 2.0, 2.0 * inp["k"]  # k x - u = 0 exactly, against an infinite h
    if what == "zero_e_and_rho":
        inp["rho"] = 0.0
    got, _ = run_twice(case, inp)
    model = cc.scale_eval(case, F32, **{k: (t.cuda() if torch.is_tensor(t) else t) for k, t in inp.items()}).cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(model))
    inf = torch.isinf(model)
    assert torch.equal(torch.isinf(got), inf) and torch.equal(got[inf], model[inf])
    special = torch.isnan(model) | inf
    assert bool(special[:, hit].all()) and not bool(special[:, ~hit].any()) and bool(torch.isnan(got[0, 0]))
    ok = ~special
    ref, allowed = cc.scale_ref(inp, case, want_bound=True)
    allowed = allowed * (cc.U[F32] / (1 - 6 * cc.U[F32]))
    ok_np = ok.numpy()
    ratio, err = cc.worst_ratio(got[ok], ref[ok_np], allowed[ok_np])
    assert ratio <= 1.0, (err, ratio)


# ------------------------------------------------------------------------------------------------------ batch invariance
INVARIANCE = [cc.Project(1100, 65, 0, 1, "f32", "f32"), cc.Expand(130, 65, 0, "d", 1, 1, -1, "f32", "f32"),
              cc.Mode(65, 7, 0, 1, "f32", "f32"), cc.Mode(65, 70, 0, 0, "f32", "f32")]


@pytest.mark.parametrize("case", INVARIANCE, ids=cc.case_id)
def test_a_row_has_the_same_bits_alone(case):
    r"""Row b of a launch with 31, 32, 33 and 70 rows (``outer`` for the mode entry) against that row computed alone, hard family."""
    entry = cc.entry_of(case)
    name = MAIN[entry]
    batched = ("x", "P") if entry == "expand" else ("x",)
    for rows in cc.INVARIANCE_ROWS:
        inp = cc.inputs(case, "hard", rows)
        full = RUN[entry](case, inp)[name].cpu()
        for b in sorted({0, 1, 30, 31, 32, 33, 63, 64, rows - 1}):
            if b >= rows:
                continue
            one = dict(inp)
            for k in batched:
                one[k] = inp[k][b : b + 1].contiguous()
            assert torch.equal(bits(RUN[entry](case, one)[name].cpu()[0]), bits(full[b])), (rows, b)


# ------------------------------------------------------------------------------------------------------------- contract
def test_entries_reject_what_the_contract_excludes():
    lib = _lib.lib()
    t = torch.zeros(64, device="cuda")
    p = t.data_ptr()
    E_NULL, E_SHAPE, E_UNSUPPORTED = -1, -2, -4
    a = _lib.AzCovLowRankArgs(x=p, W=p, P=p, y=p, rows=1, n=600, r=2)
    assert lib.az_cov_project(C.byref(a), None) == E_NULL  # two segments and no partial
    a.n, a.x = 4, None
    assert lib.az_cov_project(C.byref(a), None) == E_NULL
    a.x, a.y = p, None
    assert lib.az_cov_expand(C.byref(a), None) == E_NULL
    a.y, a.out_dtype = p, 1
    assert lib.az_cov_expand(C.byref(a), None) == E_UNSUPPORTED  # fp32 operands do not promote to fp64
    a.out_dtype, a.r = 0, 0
    assert lib.az_cov_project(C.byref(a), None) == E_SHAPE and lib.az_cov_expand(C.byref(a), None) == E_SHAPE
    m = _lib.AzCovModeArgs(x=p, Q=p, y=p + 256, outer=1, n=2, inner=0)
    assert lib.az_cov_mode(C.byref(m), None) == E_SHAPE
    m.inner, m.f_dtype = 1, 1
    assert lib.az_cov_mode(C.byref(m), None) == E_UNSUPPORTED  # an fp64 factor promotes to fp64, not fp32
    s = _lib.AzCovScaleArgs(x=p, y=p, rows=1, n=4, scalar_dtype=2)
    assert lib.az_cov_scale(C.byref(s), None) == E_UNSUPPORTED
    s.scalar_dtype, s.y = 0, None
    assert lib.az_cov_scale(C.byref(s), None) == E_NULL


# ------------------------------------------------------------------------------------------------------------ API level
@pytest.mark.parametrize("kind,shape,rank,batch", [("kronecker", (5, 100, 7), 0, (4,)), ("dplr", (1100,), 65, (33,))])
@pytest.mark.parametrize("dtype", [F32, F64])
def test_applies_match_the_host_fp64_off_the_image_shapes(kind, shape, rank, batch, dtype, monkeypatch):
    r"""Two cases in the style of test_gpu_covariance.test_applies_match_the_host_fp64, at its bounds: a Kronecker axis of 100
    (a ragged second tile) between axes of 5 and 7, and a DPLR of 1100 features (a ragged tile in the third segment), rank 65,
    33 rows."""
    import test_gpu_covariance as tg

    host = tg._make(kind, shape, rank)
    dev = host.to(device="cuda", dtype=dtype)
    x = torch.randn(*batch, *shape, generator=torch.Generator().manual_seed(7), dtype=F64)
    names = tg._spy(monkeypatch)
    for op, fn in tg._ops(dev).items():
        names.clear()
        tg._check(fn(x.to(device="cuda", dtype=dtype)), tg._ops(host)[op](x), dtype, op)
        assert any(n.startswith("az_cov_") for n in names), op
