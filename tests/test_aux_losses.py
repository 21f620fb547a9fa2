"""CPU-only: the SSIM / L2 loss kernels (raw2logit_amd/csrc/r2l_aux_kernels.h) as the host emulation runs them, on the paths
training takes -- more tiles than workgroups, more elements than one trip of the grid-stride loop -- and on the inputs where
the SSIM formula is ill conditioned in float32.  The checks and the origin of every limit are in tests/aux_checks.py;
tests/test_gpu_aux_losses.py repeats them on the gfx950 build."""
import pytest

import aux_checks as ac


@pytest.mark.parametrize('grid', ac.WALK_GRIDS)
def test_ssim_tile_walk_does_not_depend_on_the_grid(grid, emulation):
    ac.walk_under_hook('cpu', grid)


@pytest.mark.parametrize('shape', ac.PRODUCT_WALK_SHAPES, ids=['696_tiles', '1050_tiles'])
def test_ssim_with_more_tiles_than_workgroups(shape, emulation):
    ac.walk_on_product('cpu', shape)


@pytest.mark.parametrize('C,H,W', ac.EDGE_CASES, ids=[f'{C}x{H}x{W}' for C, H, W in ac.EDGE_CASES])
def test_ssim_tile_and_halo_edges(C, H, W, emulation):
    ac.edges('cpu', C, H, W)


@pytest.mark.parametrize('kind', ac.KINDS)
def test_float32_oracle_yields_usable_limits(kind):
    ac.kind_oracle_is_usable(kind)


@pytest.mark.parametrize('kind', ac.KINDS)
def test_ssim_input_kinds(kind, emulation):
    ac.kinds('cpu', kind)


@pytest.mark.parametrize('grid', ac.L2_HOOK_GRIDS, ids=['default', 'grid1', 'grid3'])
def test_l2_grid_stride_loop_under_the_hook(grid, emulation):
    trips = ac.l2_case('cpu', ac.L2_HOOK_N, grid, hook=True)
    assert trips == {None: 1, 1: 8, 3: 3}[grid]


def test_l2_single_lane(emulation):
    assert ac.l2_case('cpu', ac.L2_PRODUCT_NS[0]) == 1


def test_abi_promises(emulation):
    ac.abi_behaviour('cpu')


@pytest.mark.parametrize('batch_norm', (False, True), ids=['plain', 'batchnorm_train'])
def test_aux_loss_parameter_gradients(batch_norm, emulation):
    ac.aux_loss_values('cpu', batch_norm)
