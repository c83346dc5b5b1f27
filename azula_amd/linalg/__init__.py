r"""Linear algebra (reference ``azula/linalg``): the Krylov solvers of ``solve`` and the structured covariances of
``covariance``, on HIP kernels for device tensors."""

from . import covariance  # noqa: F401
from .solve import cg, gmres  # noqa: F401
