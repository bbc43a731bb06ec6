"""tensorrt_dft_plugins_amd -- MI355X-native DFT inference-op library.

Same capabilities as DistributedSpectrum/tensorrt-dft-plugins (``load_plugins()``, the
ONNX-contrib ``com.microsoft::Rfft`` / ``Irfft`` operators, export -> engine -> run), built
for AMD Instinct MI355X (gfx950): hand-written HIP Stockham FFT kernels registered as
PyTorch-ROCm custom ops, MFMA spectral-layer kernels, hipGraph engines and RCCL
data-parallel inference.
"""
from ._loader import (  # noqa: F401
    NativeLibraryMissing, build_info, get_plugin_creator, is_loaded, load_plugins, native_library_path, plugin_names,
    plugin_registry,
)
from .ops.dft import (  # noqa: F401
    contrib_irfft, contrib_rfft, fft, fftn, ifft, ifftn, irfft, irfft2, irfftn, rfft, rfft2, rfftn,
)
from .ops.attention_s2 import (  # noqa: F401
    attention_s2, attention_s2_global, attention_s2_global_tables, attention_s2_tables,
)
from .ops.disco import (  # noqa: F401
    disco, disco_spectral, disco_spectral_tables, disco_spectral_transpose, disco_spectral_transpose_tables,
    disco_tables, disco_transpose, disco_transpose_tables,
)
from .ops.sht import isht, ivsht, sht, vsht  # noqa: F401

__version__ = "1.0.0"
PLUGIN_VERSION = "1"
