"""motionestimation_amd -- MI355X-native full-search block-matching motion
estimation (drop-in for the hot path of souravBhat/MotionEstimation).

The compute path is libme_hip.so (HIP kernels for gfx950 behind the C ABI of
include/me.h); this package is the host-side mirror of the reference's
interface over that ABI.  There is no CPU fallback.
"""
from ._lib import (ME_COST_SAD, ME_COST_SATD, ME_COST_SSD, ME_COST_SSIM, ME_ECOMM,  # noqa: F401
                   ME_EDEVICE,
                   ME_BIPRED_MAX_Q, ME_PART_2Nx2N, ME_PART_2NxN, ME_PART_KERNEL_FAST,
                   ME_PART_KERNEL_GENERIC, ME_PART_MAX_LAMBDA, ME_PART_MAX_RANGE, ME_PART_Nx2N,
                   ME_PART_NxN, ME_PART_RD_MAX_LAMBDA, ME_PRED_BI, ME_PRED_L0, ME_PRED_L1,
                   ME_QPEL_MAX_MV,
                   ME_RD_FAST_MAX_LAMBDA, ME_RD_KERNEL_FAST, ME_RD_KERNEL_GENERIC,
                   ME_RD_MAX_LAMBDA, ME_RD_MAX_RANGE, MEError, build)
from .engine import (Engine, PartitionFields, PartitionRdFields, candidate_count,  # noqa: F401
                     mv_bits, num_blocks, rd_kernel_variant, partition_counts,
                     partition_kernel_variant, partition_leaf_field, partition_rd_kernel_variant,
                     pinned_frames, last_search_path, plan_stripes, set_kernel_path, version)
from . import io  # noqa: F401
from .reference_api import (Block, PredictionFrame, create_prediction_frame,  # noqa: F401
                            find_best_blk_mse, find_best_blk_ssim, find_best_blks,
                            frame_diff,
                            motion_compensated_frame, output_planes)
