"""Model families built on the DFT ops: FourCastNet AFNO, FNO, the spherical FNO and DISCO convolutions."""
from .afno import AFNOConfig, AFNONet, afno2d_reference, flops_per_sample, fourcastnet_config  # noqa: F401
from .disco import DiscreteContinuousConvS2, DiscreteContinuousConvTransposeS2  # noqa: F401
from .fno import FNO2d, FNOBlock, FNOConfig, SpectralConv2d, fno_block_flops, spectral_conv2d_reference  # noqa: F401
from .sfno import (InverseRealSHT, InverseRealVectorSHT, RealSHT, RealVectorSHT, SFNOBlock, SFNOConfig,  # noqa: F401
                   SFNONet, SphericalConv2d)
