r"""Guidance (reference ``azula/guidance``): classifier-free guidance, RePaint inpainting, DiffPIR restoration and JFPS
posterior sampling on the HIP path."""

from .cfg import CFGDenoiser  # noqa: F401
from .diffpir import DiffPIRDenoiser  # noqa: F401
from .jfps import JFPSDenoiser  # noqa: F401
from .repaint import RePaintSampler  # noqa: F401
