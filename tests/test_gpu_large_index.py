"""The kernels past 2^31 elements, past 2^32 bytes inside one buffer and at the 2^29-pixel frame limit, on the gfx950 build
(tests/large_index_checks.py: periodic batches, block 0 against the float64 oracle, the sums, NaN-poisoned guard-zone arena).
Each shape is the smallest that crosses its line with blocks of 4 frames; each test computes its need in bytes up front, skips
only where the device has less free, and frees everything before it returns.  Run on its own:

    timeout -k 10 1200 python -m pytest tests/test_gpu_large_index.py -q -m gpu

The refusals at the limits are NOT here: a missed refusal would launch out of bounds (tests/test_large_index.py runs them on the
lock-step emulation's sources)."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import large_index_checks as lc  # noqa: E402
import static_half_checks as shc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32


# ---- an element index of a (B,3,H,W) tensor >= 2^31: the fused step -----------------------------------------------------------
def test_step_float32_batchnorm_train_all_gradients():
    """2732x512x512: 2 148 532 224 output elements; forward + backward, float32 planar, all 132 gradients"""
    lc.check_step_case(DEV, 683, 512, 512, True, True)


def test_step_u16_frames_bfloat16_channels_last_batchnorm_eval():
    lc.check_step_case(DEV, 683, 512, 512, True, False, dtype=BF16, channels_last=True, u16=True)


def test_step_float16_planar_no_batchnorm_raw_gradient():
    lc.check_step_case(DEV, 683, 512, 512, False, True, dtype=F16, raw_grad=True)


def test_step_one_strip_frames_batchnorm_train():
    """10924x256x256, the datasets' tile size: W <= 256 takes the split statistics pass"""
    lc.check_step_case(DEV, 2731, 256, 256, True, True)


# ---- a pixel index of a (B,H,W) plane >= 2^31: the static chains' fused kernels, 16-bit frames to bfloat16 ------------------------
@pytest.mark.parametrize('chain', [shc.SHORT_BILINEAR, shc.DEFAULT_CHAIN], ids=['short', 'default'])
def test_static_u16_to_bfloat16_past_2_31_pixels(chain):
    """2052x1024x1024: 4.3 GB in, 12.9 GB out, no workspace (r2l_static_fwd_io)"""
    lc.check_static_case(DEV, 513, 1024, 1024, chain, dtype=BF16, u16=True, frames=(0, 3),
                         kernel=shc.kernel_name(chain, torch.int16, BF16))


# ---- the plane routes -----------------------------------------------------------------------------------------------------------
def test_static_plane_passes_past_2_31_elements():
    """a chain that runs as float64 plane passes (tests/golden/static_routes.txt, 'R planes ... 012 5': bilinear, sharpening_filter,
    5x5 median): 2732x512x512 float32, workspace 16 B/px"""
    lc.check_static_case(DEV, 683, 512, 512, ('bilinear', 'sharpening_filter', 'median_denoising'),
                         options=(('median_kernel_size', 5),), frames=(0, 3), workspace_per_px=16, kernel='r2l_launch_plane_filter')


def test_static_menon2007_past_2_32_bytes_of_float64():
    """176x1024x1024: workspace 64 B/px, a float64 plane of 1.5 GB -- byte offsets past 2^32 from the third plane on; frames 0,
    88 and 175 against the oracle, the rest by periodicity"""
    lc.check_static_case(DEV, 44, 1024, 1024, ('menon2007', 'none', 'none'), frames=(0, 3), workspace_per_px=64,
                         kernel='r2l_launch_static_menon')


# ---- one frame at the 2^29-pixel limit ---------------------------------------------------------------------------------------------
def test_one_frame_of_2_29_pixels_static_short_chain():
    lc.check_tall_static(DEV, 262144, 2048, shc.SHORT_BILINEAR)


def test_one_frame_of_2_29_pixels_step_forward():
    lc.check_tall_step_forward(DEV, 262144, 2048)


# ---- flat n >= 2^31 ------------------------------------------------------------------------------------------------------------------
def test_flat_l2_forward_and_backward():
    lc.check_flat_l2(DEV)


def test_flat_philox_noise():
    lc.check_flat_philox_noise(DEV)


@pytest.mark.parametrize('hflip,vflip,k', [(True, False, 2), (False, True, 1)], ids=['k2', 'k1'])
def test_flat_flip_rot(hflip, vflip, k):
    lc.check_flat_flip_rot(DEV, hflip, vflip, k)


@pytest.mark.parametrize('transform', ['brightness', 'gaussian_noise'])
def test_flat_corruption(transform):
    lc.check_flat_corrupt(DEV, transform)


def test_flat_strong_augmentation_forward_and_backward():
    lc.check_flat_strong_augmentation(DEV)


# ---- a float32 byte offset >= 2^32: SSIM ----------------------------------------------------------------------------------------------
def test_ssim_past_2_32_bytes():
    lc.check_ssim_large(DEV)
