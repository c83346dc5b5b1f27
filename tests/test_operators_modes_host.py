r"""The ``_TRANSPOSE`` table of every operator class without a GPU: for one instance of each class and every mode ``m`` the table
lists, ``<A_m x, w> == <x, A_{T[m]} w>`` on the torch path in fp64 -- what ``backward`` of the Function relies on when it looks
the transposed mode up.  The modes that only ``backward`` reaches (``pinv_t``, ``zero_filled_t``, ``fbp_t``) are run here directly.
"""

import pytest
import torch

import operator_cases as oc
from azula_amd.guidance import MRIOperator
from operator_mode_cases import B, domain, instances

F64 = torch.float64


def host_map(A, x, mode):
    r"""The torch path; ``MRIOperator`` has it as the composition in ``_run``, which a host tensor takes to the ``_torch`` of its two
    operators."""
    return A._run(x, mode) if isinstance(A, MRIOperator) else A._torch(x, mode)


@pytest.mark.parametrize("name, A, in_shape", instances(), ids=lambda v: v if isinstance(v, str) else "")
def test_every_mode_and_its_table_entry_are_transposes_in_fp64(name, A, in_shape):
    T = A._TRANSPOSE
    assert "apply" in T and "adjoint" in T
    for k, m in enumerate(T):
        assert T[T[m]] == m, (name, m)  # an involution
        x = oc.random_image(B, *domain(A, in_shape, m), seed=2 * k).double()
        w = oc.random_image(B, *domain(A, in_shape, T[m]), seed=2 * k + 1).double()
        y, g = host_map(A, x, m), host_map(A, w, T[m])
        assert y.dtype == F64 and y.shape == w.shape and g.shape == x.shape, (name, m)
        lhs, rhs = float((y * w).sum()), float((x * g).sum())
        bound = 1e-12 * float(y.abs().sum() * w.abs().max())
        print(f"{name} {m}: |<A_m x, w> - <x, A_T[m] w>| = {abs(lhs - rhs):.3e}, bound {bound:.3e}")
        assert abs(lhs - rhs) <= bound, (name, m)
