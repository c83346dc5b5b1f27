r"""``az_tds_resample_f32`` and ``az_tds_propose_f32`` on the GPU against fp64, without a network.

Test A (resample): on the uniforms of ``tds_cases.resample_case`` -- each at least 1e-5 from every fp64 CDF value, asserted by
``tests/test_tds_host.py`` -- the ancestors EQUAL the fp64 inverse CDF; at K = 4096 with stratified uniforms the count of each
index is within 3 of ``K w_i`` (1 is exact for stratified points, one more point may move at each end through rounding of the
boundary); ``w`` matches the fp64 softmax to 1e-6 of its maximum; particles of weight 0 are never chosen; the degenerate
conventions hold; two runs give the same bits.

Test B (propose): ``x_s`` per element within ``8 * 2^-24`` of the summed magnitudes of its four terms, ``log_w_next`` within
``c * 2^-24 * (sum_i |term_i| + |log_p[k]|)`` with ``c = 8`` from the kernel's stated accumulation (``csrc/tds.hip``: one
rounding per term, at most five dependent fp32 adds, one rounding of the result; everything else fp64).  A dropped or doubled
element moves the sum by about ``sum / N >= sum / 16387``, four times the bound.  The reference's own form -- two fp32 sums of
log-densities -- is evaluated with torch on the device, and at N = 16387 the kernel's error may not exceed it.
"""

import ctypes as C
import math

import pytest
import torch

import tds_cases as tc
import tds_oracle as to
from azula_amd import _lib

pytestmark = pytest.mark.gpu
U = 2.0**-24


def resample(log_p, log_w_prev, u):
    K = len(log_p)
    anc = torch.full((K,), -7, dtype=torch.int64, device="cuda")
    w = torch.full((K,), -7.0, device="cuda")
    _lib.call("az_tds_resample_f32", _lib.ptr(log_p), None if log_w_prev is None else _lib.ptr(log_w_prev), _lib.ptr(u),
              _lib.ptr(anc), _lib.ptr(w), K, _lib.stream_ptr())
    return anc, w


@pytest.mark.parametrize("K,kind,prev", tc.RESAMPLE_CASES)
def test_resample_equals_fp64_inverse_cdf(K, kind, prev):
    log_p, log_w_prev, u = tc.resample_case(K, kind, prev)
    k_ref, w_ref, _ = to.inverse_cdf(log_p.double() + (log_w_prev.double() if prev else 0), u)
    dev = [None if v is None else v.cuda() for v in (log_p, log_w_prev, u)]
    anc, w = resample(*dev)
    anc2, w2 = resample(*dev)
    assert torch.equal(anc, anc2) and torch.equal(w, w2)
    assert torch.equal(anc.cpu(), k_ref)
    err = float((w.double().cpu() - w_ref).abs().max() / w_ref.max())
    print(f"K {K} {kind} prev {prev}: w err {err:.2e}")
    assert err < 1e-6
    assert (w_ref[anc.cpu()] > 0).all() and (w.cpu()[w_ref == 0] == 0).all()


@pytest.mark.parametrize("kind", ["randn3", "dominant", "neginf"])
def test_resample_stratified_counts(kind):
    K = 4096
    log_p, log_w_prev, _ = tc._resample_draw(K, kind, True, 5)
    u = (torch.arange(K, dtype=torch.float64) + 0.5) / K
    _, w_ref, _ = to.inverse_cdf(log_p.double() + log_w_prev.double(), u)
    anc, w = resample(log_p.cuda(), log_w_prev.cuda(), u.float().cuda())
    anc = anc.cpu()
    assert int(anc.min()) >= 0 and int(anc.max()) < K and (anc[1:] >= anc[:-1]).all()
    counts = torch.bincount(anc, minlength=K).double()
    dev = float((counts - K * w_ref).abs().max())
    print(f"{kind}: largest count deviation {dev:.3f}")
    assert dev <= 3
    assert (counts[w_ref == 0] == 0).all()
    assert float((w.double().cpu() - w_ref).abs().max() / w_ref.max()) < 1e-6


def test_resample_degenerate_inputs():
    r"""All -inf, or any NaN: ``w`` is NaN and every particle keeps itself (the reference raises in ``torch.multinomial``)."""
    K = 70
    u = torch.rand(K, device="cuda")
    for log_p in (torch.full((K,), -math.inf), torch.randn(K).index_fill_(0, torch.tensor([33]), math.nan)):
        anc, w = resample(log_p.cuda(), None, u)
        assert torch.isnan(w).all() and torch.equal(anc.cpu(), torch.arange(K))
    anc, w = resample(torch.randn(K, device="cuda"), torch.full((K,), -math.inf, device="cuda"), u)
    assert torch.isnan(w).all() and torch.equal(anc.cpu(), torch.arange(K))


def propose(x_t, x_hat, score, z, k, log_p, coef):
    K, N = x_t.shape
    chunks = _lib.lib().az_tds_chunks(K, N)
    x_s = torch.full_like(x_t, math.nan)
    log_w = torch.full((K,), math.nan, device="cuda")
    work = torch.full((K * chunks,), math.nan, dtype=torch.float64, device="cuda")
    a = _lib.AzTdsProposeArgs(x_t=_lib.ptr(x_t), x_hat=_lib.ptr(x_hat), score=_lib.ptr(score), z=_lib.ptr(z), ancestors=_lib.ptr(k),
                              log_p=_lib.ptr(log_p), coef=_lib.ptr(coef), x_s=_lib.ptr(x_s), log_w_next=_lib.ptr(log_w),
                              workspace=work.data_ptr(), K=K, N=N, chunks=chunks)
    _lib.call("az_tds_propose_f32", C.byref(a), _lib.stream_ptr())
    return x_s, log_w


def check_propose(K, N, kind, score_scale, times):
    x_t, x_hat, score, z, log_p, g = tc.propose_inputs(K, N, score_scale)
    k = tc.propose_ancestors(kind, K, g)
    coef = tc.propose_coef(*times)
    x_ref, w_ref, x_mag, w_mag = tc.propose_reference(x_t, x_hat, score, z, k, log_p, coef)
    dev = [v.cuda() for v in (x_t, x_hat, score, z, k, log_p, coef)]
    x_s, log_w = propose(*dev)
    x_s2, log_w2 = propose(*dev)
    assert torch.equal(x_s, x_s2) and torch.equal(log_w, log_w2)
    ex = float(((x_s.double().cpu() - x_ref).abs() / x_mag.clamp_min(1e-300)).max() / U)
    ew = (log_w.double().cpu() - w_ref).abs()
    two = (tc.two_sum_form(*dev).double().cpu() - w_ref).abs()
    print(f"({K}, {N}) {kind} score {score_scale:g} t {times}: x_s {ex:.2f} u, log_w {float((ew / w_mag).max() / U):.2f} u "
          f"(two-sum form {float((two / w_mag).max() / U):.1f} u)")
    assert ex <= 8
    assert (ew <= tc.PROPOSE_C * U * w_mag).all()
    return ew, two


@pytest.mark.parametrize("K,N", tc.PROPOSE_SHAPES[:-1])
@pytest.mark.parametrize("times", tc.PROPOSE_TIMES)
def test_propose_matches_fp64(K, N, times):
    assert tc.PROPOSE_C <= 64
    for kind in tc.PROPOSE_ANCESTORS:
        for score_scale in tc.PROPOSE_SCORE_SCALES:
            ew, two = check_propose(K, N, kind, score_scale, times)
            if N == 16387:  # the cancellation-free form has to show against the difference of two fp32 sums
                assert float(ew.max()) <= float(two.max())


def test_propose_strided_rows():
    r"""More spans than chunks: a workgroup strides over its row (700 x 8200: 3 spans in 2 chunks)."""
    K, N = tc.PROPOSE_SHAPES[-1]
    assert _lib.lib().az_tds_chunks(K, N) < -(-N // 4096)
    check_propose(K, N, "repeats", 1.0, tc.PROPOSE_TIMES[0])


def test_propose_argument_errors_and_bad_ancestors():
    x_t, x_hat, score, z, log_p, _ = tc.propose_inputs(3, 8, 1.0)
    coef = tc.propose_coef(*tc.PROPOSE_TIMES[0])
    dev = [v.cuda() for v in (x_t, x_hat, score, z, torch.tensor([0, 5, -1]), log_p, coef)]
    x_s, log_w = propose(*dev)  # ancestors outside [0, K) read nothing: NaN for that particle only
    assert torch.isfinite(x_s[0]).all() and torch.isfinite(log_w[0])
    assert torch.isnan(x_s[1:]).all() and torch.isnan(log_w[1:]).all()
    lib = _lib.lib()
    ok = dict(x_t=_lib.ptr(dev[0]), x_hat=_lib.ptr(dev[1]), score=_lib.ptr(dev[2]), z=_lib.ptr(dev[3]), ancestors=_lib.ptr(dev[4]),
              log_p=_lib.ptr(dev[5]), coef=_lib.ptr(dev[6]), x_s=_lib.ptr(x_s), log_w_next=_lib.ptr(log_w),
              workspace=torch.empty(3, dtype=torch.float64, device="cuda").data_ptr(), K=3, N=8, chunks=1)
    call = lambda **kw: lib.az_tds_propose_f32(C.byref(_lib.AzTdsProposeArgs(**{**ok, **kw})), _lib.stream_ptr())  # noqa: E731
    assert call(x_s=ok["x_t"]) == -2 and call(x_s=ok["score"] + 16) == -2  # returned, not raised
    assert call(chunks=3) == -2 and call(x_s=None) == -1 and call(x_s=ok["x_s"] + 4) == -3
    torch.cuda.synchronize()
