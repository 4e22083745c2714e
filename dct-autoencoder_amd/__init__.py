"""MI355X-native drop-in for the feature-extraction hot path of
theAdamColton/dct-autoencoder (RGB -> IPT -> DCT -> spectral patches ->
PatchNorm -> LFQ and back), running on hand-written gfx950 HIP kernels
(libdctae.so, C ABI in include/dctae.h).

Import name: ``dct_autoencoder_amd`` (the directory is dct-autoencoder_amd/;
see _pkgload.py at the repository root)."""
from ._lib import DCTAEError, DCTAEUnavailable, load_library  # noqa: F401
from .dct_patches import DCTPatches, build_attn_mask, from_dict, to_dict  # noqa: F401
from .feature_extraction import DCTAutoencoderFeatureExtractor, GroupPatchesState  # noqa: F401
from .lfq import LFQ  # noqa: F401
from .losses import (LFQDistance, calculate_perplexity, compute_entropy_loss, masked_mean,  # noqa: F401
                     masked_perplexity, pixel_loss, reconstruction_losses, step_losses)
from .model import CLIPEncoderConfig, DCTAutoencoder, DCTAutoencoderConfig  # noqa: F401
from .optim import FusedAdamW  # noqa: F401
from .patchnorm import PatchNorm  # noqa: F401
from .vector_quantize import VectorQuantize  # noqa: F401
from . import packing  # noqa: F401
from . import progressive  # noqa: F401
from .progressive import frame_cuts, image_clip, model_decode_prefixes  # noqa: F401
from . import shards  # noqa: F401

__all__ = ["DCTAutoencoderFeatureExtractor", "DCTPatches", "PatchNorm", "LFQ", "VectorQuantize", "to_dict", "from_dict",
           "DCTAutoencoder", "DCTAutoencoderConfig", "CLIPEncoderConfig", "FusedAdamW",
           "GroupPatchesState", "build_attn_mask", "load_library", "DCTAEError", "DCTAEUnavailable",
           "LFQDistance", "compute_entropy_loss", "masked_mean", "calculate_perplexity",
           "reconstruction_losses", "masked_perplexity", "step_losses", "pixel_loss", "progressive", "frame_cuts",
           "image_clip", "model_decode_prefixes"]
