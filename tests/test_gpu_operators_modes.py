r"""The ``_TRANSPOSE`` table on the GPU: for the instances of ``operator_mode_cases.py`` and every mode ``m`` the table lists,
the gradient of the Function in mode ``m`` EQUALS the kernels run directly in mode ``T[m]``, its forward-mode tangent EQUALS the
kernels in mode ``m``, and ``backward`` launches exactly what the direct call launches.  No tolerance: backward and jvp are
applications of the same launches.

``MRIOperator`` is a composition of two operators' ``_run`` with no ``_kernel`` of its own: there the Function is reached through
``_run`` and the direct call is ``_run`` without a graph.
"""

import pytest
import torch

import operator_cases as oc
from operator_mode_cases import B, domain, instances

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _grad_mode_on():
    r"""Some modules of the suite switch grad mode off for the whole process; these tests differentiate."""
    with torch.enable_grad():
        yield


def _spy(monkeypatch):
    from azula_amd.guidance import operators as ops

    names, launch = [], ops._launch
    monkeypatch.setattr(ops, "_launch", lambda name, *a: (names.append(name), launch(name, *a))[1])
    return names


def _maps(A):
    r"""(the map as the Function, the map as its kernels alone), each of (tensor, mode)."""
    from azula_amd.guidance import MRIOperator
    from azula_amd.guidance.operators import _Apply

    if isinstance(A, MRIOperator):
        return A._run, lambda t, m: A._run(t.detach(), m)
    return lambda t, m: _Apply.apply(t, A, m), A._kernel


@pytest.mark.parametrize("name, A, in_shape", instances(), ids=lambda v: v if isinstance(v, str) else "")
def test_grad_and_jvp_of_every_mode_are_the_kernels_of_the_table(name, A, in_shape, monkeypatch):
    names = _spy(monkeypatch)
    function, kernels = _maps(A)
    T = A._TRANSPOSE
    for k, m in enumerate(T):
        x = oc.random_image(B, *domain(A, in_shape, m), seed=2 * k).cuda().requires_grad_()
        w = oc.random_image(B, *domain(A, in_shape, T[m]), seed=2 * k + 1).cuda()
        tx = oc.random_image(*x.shape, seed=2 * k + 50).cuda()
        y = function(x, m)
        assert y.shape == w.shape and names, (name, m)
        del names[:]
        g = torch.autograd.grad(y, x, w)[0]
        launched = list(names)
        del names[:]
        want = kernels(w, T[m])
        assert launched == names and launched, (name, m, launched, names)
        assert torch.equal(g, want), (name, m)
        out, tangent = torch.func.jvp(lambda t, m=m: function(t, m), (x.detach(),), (tx,))
        assert torch.equal(out, y) and torch.equal(tangent, kernels(tx, m)), (name, m)
