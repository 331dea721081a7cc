"""irdu_amd — MI355X-native engine for the GGTV/GGLR unrolled graph-filter path of
tamthuc1995/ImageRestoration-Development-Unrolling.

Import as ``irdu_amd`` (the root-level ``irdu_amd.py`` loader maps this hyphenated
directory to that package name).  The public surface mirrors the reference's
module ``deep_multiscale_GGLR_GGTV_v1x0`` so callers can swap the import:

    import irdu_amd as model_structure
    model = model_structure.AbtractMultiScaleGraphFilter(...).cuda()

Importing changes no process-wide setting.  A drop-in training script with its own loop calls
``irdu_amd.miopen_training_defaults()`` before its first convolution (MIOpen's find-db otherwise costs
seconds of host time per step on the v1.0 model's stock convolutions after a box's first run,
DESIGN.md §4.r4); the first training-mode forward of AbtractMultiScaleGraphFilter warns once when
MIOPEN_DEBUG_DISABLE_FIND_DB is unset.  ``irdu_amd.native_convs(True)`` (or GRR_NATIVE_CONVS=1) runs that model's
plain convolutions on libgrr as well; no MIOpen setting matters then and the warning stays silent.
"""
from ._native import GrrError, NativeUnavailable, load as load_native  # noqa: F401
from .graph_filter import (  # noqa: F401
    AbtractMultiScaleGraphFilter,
    CustomLayerNorm,
    Downsampling,
    GLRFast,
    GTVFast,
    LocalGatedLinearBlock,
    LocalLowpassFilteringBlock,
    LocalNonLinearBlock,
    MixtureGTVGLR,
    MultiScaleGraphFilter,
    ReginalPixelEmbeding,
    Upsampling,
    native_convs,
)
from . import kernels  # noqa: F401
from . import glr_v10 as v10  # noqa: F401  (GLR-only drop-ins of lib/model_GLR_GTV_deep_v10.py)
from .glr_v10 import GLRImageFilter, MixtureGLR, MultiScaleGLRImageFilter, MultiScaleMixtureGLR  # noqa: F401
from . import window_graph  # noqa: F401  (window-graph MixtureGTV of lib/model_GLR_GTV_deep_v7.py)
from . import window_graph_v1  # noqa: F401  (multiblock window denoiser of lib/model_GLR_GTV_deep_v1.py)

from .training import miopen_training_defaults  # noqa: F401
from .training import DevicePatchLoader, ImageSuperResolution  # noqa: F401  (the v2 scripts' training set)
from . import restore  # noqa: F401  (whole-image restoration of 8-bit / float images of any size)
from .restore import RestorePlan, evaluate, plan, psnr_u8, restore_image  # noqa: F401
from .restore import ImagePack, pack_images, plan_images, restore_images  # noqa: F401  (lists of images)
from .restore import evaluate_metrics, ssim_u8  # noqa: F401  (SSIM beside the PSNR)
from .restore import psnr_y_u8, ssim_y_u8  # noqa: F401  (the two on the Y channel of RGB images)
from .training import PairedImageRestoration  # noqa: F401  (degraded / clean file pairs)
from .restore import evaluate_pairs  # noqa: F401
from .training import BicubicSuperResolution  # noqa: F401  (bicubic super-resolution pairs made from clean files)
from .restore import bicubic_degrade_u8, bicubic_down_u8, bicubic_up_u8, evaluate_sr  # noqa: F401
from .training import JpegArtifactRemoval  # noqa: F401  (JPEG artifact-removal pairs made from clean files)
from .restore import evaluate_car, jpeg_degrade_u8, psnrb_u8  # noqa: F401
from .training import BayerDemosaicking  # noqa: F401  (demosaicking pairs made from clean files)
from .restore import demosaic_u8, evaluate_demosaic  # noqa: F401
from .training import NoisyBayerDemosaicking  # noqa: F401  (joint denoising and demosaicking: noise on the mosaic)
from .restore import evaluate_jdd, raw_noise_demosaic_u8  # noqa: F401
from .training import GaussianMotionDeblurring  # noqa: F401  (deblurring pairs made from clean files)
from .training import BlurKernel, blur_degrade_u8, box_kernel, gaussian_kernel, motion_kernel  # noqa: F401
from .training import parse_blur_spec, quantise_blur_kernel  # noqa: F401
from .restore import blur_u8, evaluate_deblur  # noqa: F401
from .training import RandomMaskInpainting  # noqa: F401  (inpainting pairs: a drawn mask and its fill, per batch)
from .restore import evaluate_inpaint, mask_fill_u8, psnr_missing_u8  # noqa: F401
from . import losses  # noqa: F401  (training losses on the HIP kernels)
from .losses import SSIMLoss, ssim_loss, ssim_loss_sums  # noqa: F401  (1 - SSIM, forward and reverse in float64)

__version__ = "0.1.0"
