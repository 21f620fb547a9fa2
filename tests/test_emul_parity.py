"""CPU-only: the REAL kernel source (raw2logit_amd/csrc/*.h), compiled by g++ as a host emulation
(tests/emul/r2l_emul.cpp), driven through the product's Python modules and C ABI, against the oracle and
the reference's golden vectors.  This pins tiling, halo, border, reduction and autograd-glue logic
without a GPU; tests/test_gpu_parity.py repeats the same checks on the gfx950 build."""
import pytest

from oracle.golden_cases import PARAM_CASES, STATIC_CASES
import parity_checks as pc

DEVICE_STATIC = list(STATIC_CASES)   # every chain of the golden set is built for the device


@pytest.mark.parametrize('case', PARAM_CASES, ids=[c['name'] for c in PARAM_CASES])
def test_fused_parametrized(case, golden, emulation):
    pc.check_param_case(case, golden, 'cpu')


def test_raw2rgb(golden, emulation):
    pc.check_raw2rgb(golden, 'cpu')


def test_nnprocessing_front_end(golden, emulation):
    pc.check_nnprocessing(golden, 'cpu')


@pytest.mark.parametrize('case', DEVICE_STATIC, ids=[c['name'] for c in DEVICE_STATIC])
def test_static(case, golden, emulation):
    pc.check_static_case(case, golden, 'cpu')


def test_properties(emulation):
    pc.check_ragged_and_properties('cpu')


def test_frame_shapes_around_tile_boundaries(emulation):
    pc.check_frame_shapes('cpu')


def test_harness_logits_and_adam_step(golden, emulation):
    pc.check_harness(golden, 'cpu')


TRACK_CASES = [c for c in PARAM_CASES if c['track']]


@pytest.mark.parametrize('case', TRACK_CASES, ids=[c['name'] for c in TRACK_CASES])
def test_staged_track_stages(case, golden, emulation):
    pc.check_staged_case(case, golden, 'cpu')


def test_reductions_do_not_depend_on_the_grid(emulation):
    pc.check_grid_independence('cpu')


GRAD_RAW_CASES = [c for c in PARAM_CASES if not c['track'] and c['name'] in (
    'drone_bn_train', 'drone_additive_bn', 'micro_bn_train', 'drone_ragged_tile', 'tiny_4x4', 'drone_bn_eval')]


@pytest.mark.parametrize('case', GRAD_RAW_CASES, ids=[c['name'] for c in GRAD_RAW_CASES])
def test_frames_requiring_grad_take_the_staged_kernels(case, golden, emulation):
    pc.check_staged_case(case, golden, 'cpu')


def test_16bit_containers_are_bit_identical_to_host_normalised_frames(emulation):
    pc.check_u16_ingest('cpu')


def test_static_chain_combinations(emulation):
    pc.check_static_combinations('cpu')


def test_static_numeric_arguments(golden, emulation):
    pc.check_static_options(golden, 'cpu')


def test_static_normalize_epilogue(emulation):
    pc.check_static_normalize('cpu')


def test_adversarial_aux_losses(golden, emulation):
    pc.check_aux_losses(golden, 'cpu')


def test_static_per_image_wrappers(golden, emulation):
    pc.check_static_wrappers(golden, 'cpu')


def test_weak_augmentation(emulation):
    pc.check_augmentation('cpu')


def test_error_behaviour(emulation):
    pc.check_error_behaviour('cpu')


def test_tile_walk_covers_every_tile_once_in_even_shares(emulation):
    """the persistent kernels' tile walk (r2l_walk_init / r2l_walk_next): every tile exactly once, whatever the grid; on
    BASELINE config 2's shape every workgroup takes 8 tiles"""
    import ctypes
    import numpy as np
    lib = emulation.cdll
    walk = lib.r2l_test_tile_walk
    walk.restype = ctypes.c_int
    walk.argtypes = [ctypes.c_int] * 4 + [ctypes.c_void_p] * 2
    for (B, H, W) in ((64, 512, 512), (3, 200, 520), (1, 64, 64), (16, 1024, 1024), (128, 256, 256), (5, 70, 70)):
        ntiles = B * ((H + 63) // 64) * ((W + 63) // 64)
        for nblk in (512, 256, 24, 8, 7, 1):
            owner = np.empty(ntiles, dtype=np.int32)
            visits = np.empty(ntiles, dtype=np.int32)
            most = walk(B, H, W, nblk, owner.ctypes.data_as(ctypes.c_void_p), visits.ctypes.data_as(ctypes.c_void_p))
            assert np.all(visits == 1), (B, H, W, nblk, int((visits != 1).sum()))
            assert owner.min() >= 0 and owner.max() < nblk
            if (B, H, W, nblk) == (64, 512, 512, 512):
                counts = np.bincount(owner, minlength=nblk)
                assert counts.min() == counts.max() == 8
                assert most == counts.max()


# ---- the flat grid-stride kernels past one grid pass (R2L_GRID_FLAT: min(computed grid, cap)) and the shapes around them ----
def test_staged_kernels_walk_several_pixels_per_lane(golden, emulation):
    pc.check_staged_multipass(golden, 'cpu')


def test_raw2rgb_walks_several_items_per_lane(emulation):
    pc.check_raw2rgb_multipass('cpu')


def test_permutation_shapes(emulation):
    pc.check_permutation_shapes('cpu')


@pytest.mark.parametrize('shapes', [pc.STATIC_PLANE_SHAPES[:4], pc.STATIC_PLANE_SHAPES[4:]], ids=['first-four', 'last-four'])
@pytest.mark.parametrize('chain', pc.STATIC_PLANE_CHAINS, ids=['|'.join(c) + ('|5x5' if o else '') for c, o in pc.STATIC_PLANE_CHAINS])
def test_static_plane_pass_shapes_around_the_fast_path(chain, shapes, emulation):
    pc.check_static_plane_shapes('cpu', shapes=shapes, chains=[chain])
