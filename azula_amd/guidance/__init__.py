r"""Guidance (reference ``azula/guidance``): classifier-free guidance, RePaint inpainting, DiffPIR restoration, JFPS
posterior sampling, the gradient-based methods DPS / PGDM / TMPD / MMPS (the network part of their gradients is the HIP
input-gradient pass of the UNet) and the twisted SMC sampler TDS (the same pass, then fused resample / proposal kernels) on
the HIP path.  ``operators`` (the project's own) holds the measurement operators these methods take as ``A``: mask, downsample,
separable blur, general PSF, decimation, channel mix, the 2-D Fourier transform (k-space undersampling: single-coil and multi-coil SENSE MRI) and the
parallel-beam Radon transform (sparse-view CT) with exact adjoints on HIP kernels, and the nonlinear ones -- Fourier phase
retrieval, saturation (HDR), quantisation -- with their Jacobians on HIP kernels."""

from .cfg import CFGDenoiser  # noqa: F401
from .diffpir import DiffPIRDenoiser  # noqa: F401
from .dps import DPSSampler  # noqa: F401
from .jfps import JFPSDenoiser  # noqa: F401
from .mmps import MMPSDenoiser  # noqa: F401
from .operators import BlurOperator, DownsampleOperator, LinearOperator, MaskOperator, gaussian_taps  # noqa: F401
from .operators import ChannelMixOperator, DecimateOperator, PSFOperator, bicubic_taps, motion_psf  # noqa: F401
from .operators import FourierOperator, MRIOperator, cartesian_mask  # noqa: F401
from .operators import MultiCoilMRIOperator, birdcage_maps  # noqa: F401
from .operators import RadonOperator, radon_angles  # noqa: F401
from .operators import ClipOperator, MagnitudeOperator, NonlinearOperator, PadOperator  # noqa: F401
from .operators import PhaseRetrievalOperator, QuantizeOperator  # noqa: F401
from .pgdm import PGDMSampler  # noqa: F401
from .repaint import RePaintSampler  # noqa: F401
from .tds import TDSSampler  # noqa: F401
from .tmpd import TMPDenoiser  # noqa: F401
