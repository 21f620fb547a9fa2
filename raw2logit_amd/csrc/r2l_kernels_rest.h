// r2l_kernels_rest.h -- the kernels of everything else: the stage-by-stage path, augmentations, corruptions, SSIM / L2, the
// channel sums.
#pragma once
#include "r2l_launch.h"
#include "r2l_staged_kernels.h"
#include "r2l_aux_kernels.h"
#include "r2l_augment_strong.h"
#include "r2l_corruptions.h"
#include "r2l_sums_kernels.h"

R2L_KERNEL(r2l_launch_conv33_fwd, R2LStageArgs, r2l_conv33_fwd_block, 4)
R2L_KERNEL(r2l_launch_conv33_bwd, R2LStageArgs, r2l_conv33_bwd_block, R2L_RED_FLOATS)
R2L_KERNEL(r2l_launch_mix3_fwd, R2LStageArgs, r2l_mix3_fwd_block, 4)
R2L_KERNEL(r2l_launch_mix3_bwd, R2LStageArgs, r2l_mix3_bwd_block, R2L_RED_FLOATS)
R2L_KERNEL(r2l_launch_pconv_fwd, R2LStageArgs, r2l_pconv_fwd_block, 4)
R2L_KERNEL(r2l_launch_pconv_bwd, R2LStageArgs, r2l_pconv_bwd_block, R2L_RED_FLOATS)
R2L_KERNEL(r2l_launch_point, R2LPointArgs, r2l_point_block, R2L_RED_FLOATS)
R2L_KERNEL(r2l_launch_aug, R2LAugArgs, r2l_aug_block, 4)
R2L_KERNEL(r2l_launch_aug_tiled, R2LAugTiledArgs, r2l_aug_tiled_block, R2L_AUG_LDS_FLOATS)
R2L_KERNEL(r2l_launch_axpy, R2LAxpyArgs, r2l_axpy_block, 4)
R2L_KERNEL(r2l_launch_philox_noise, R2LPhiloxArgs, r2l_philox_noise_block, 4)
R2L_KERNEL(r2l_launch_strong_fwd_flat, R2LStrongArgs, r2l_strong_fwd_flat_block, 4)
R2L_KERNEL(r2l_launch_strong_fwd_sharp, R2LStrongArgs, r2l_strong_fwd_sharp_block, R2L_AUGS_LDS_FLOATS)
R2L_KERNEL(r2l_launch_strong_bwd_sharp, R2LStrongBwdArgs, r2l_strong_bwd_sharp_block, 4)
R2L_KERNEL(r2l_launch_strong_bwd_rot, R2LStrongBwdArgs, r2l_strong_bwd_rot_block, 4)
R2L_KERNEL(r2l_launch_corrupt_identity, R2LCorruptArgs, r2l_corrupt_point_block<R2L_CORRUPT_IDENTITY>, 4)
R2L_KERNEL(r2l_launch_corrupt_gaussian_noise, R2LCorruptArgs, r2l_corrupt_point_block<R2L_CORRUPT_GAUSSIAN_NOISE>, 4)
R2L_KERNEL(r2l_launch_corrupt_shot_noise, R2LCorruptArgs, r2l_corrupt_point_block<R2L_CORRUPT_SHOT_NOISE>, 4)
R2L_KERNEL(r2l_launch_corrupt_impulse_noise, R2LCorruptArgs, r2l_corrupt_point_block<R2L_CORRUPT_IMPULSE_NOISE>, 4)
R2L_KERNEL(r2l_launch_corrupt_speckle_noise, R2LCorruptArgs, r2l_corrupt_point_block<R2L_CORRUPT_SPECKLE_NOISE>, 4)
R2L_KERNEL(r2l_launch_corrupt_contrast, R2LCorruptArgs, r2l_corrupt_point_block<R2L_CORRUPT_CONTRAST>, 4)
R2L_KERNEL(r2l_launch_corrupt_brightness, R2LCorruptArgs, r2l_corrupt_point_block<R2L_CORRUPT_BRIGHTNESS>, 4)
R2L_KERNEL(r2l_launch_corrupt_saturate, R2LCorruptArgs, r2l_corrupt_point_block<R2L_CORRUPT_SATURATE>, 4)
R2L_KERNEL(r2l_launch_corrupt_mean, R2LCorruptArgs, r2l_corrupt_mean_block, R2L_CMEAN_LDS_FLOATS)
R2L_KERNEL(r2l_launch_corrupt_blur, R2LCorruptArgs, r2l_corrupt_blur_block, R2L_CBLUR_LDS_FLOATS)
R2L_KERNEL(r2l_launch_corrupt_zoom, R2LCorruptZoomArgs, r2l_corrupt_zoom_block, 4)
R2L_KERNEL(r2l_launch_ssim, R2LSsimArgs, r2l_ssim_block, R2L_SSIM_LDS_FLOATS)
R2L_KERNEL(r2l_launch_ssim_bwd, R2LSsimBwdArgs, r2l_ssim_bwd_block, R2L_SSIM_BWD_LDS_FLOATS)
R2L_KERNEL(r2l_launch_l2, R2LL2Args, r2l_l2_block, R2L_RED_FLOATS_N(1))
R2L_KERNEL(r2l_launch_pack_fold, R2LPackFoldArgs, r2l_pack_fold_block, R2L_P_COUNT + 2)
R2L_KERNEL(r2l_launch_channel_sums, R2LChannelSumsArgs, r2l_channel_sums_block, R2L_SUMS_LDS_FLOATS)
R2L_KERNEL(r2l_launch_sums_finish, R2LSumsFinishArgs, r2l_sums_finish_block, R2L_SUMS_LDS_FLOATS)
