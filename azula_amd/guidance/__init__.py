r"""Guidance (reference ``azula/guidance``): classifier-free guidance and RePaint inpainting on the HIP path."""

from .cfg import CFGDenoiser  # noqa: F401
from .repaint import RePaintSampler  # noqa: F401
