r"""Linear algebra (reference ``azula/linalg``): the Krylov solvers of ``solve``, on HIP kernels for device tensors."""

from .solve import cg, gmres  # noqa: F401
