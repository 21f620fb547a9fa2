"""The SSIM / L2 loss kernels on the MI355X: the checks of tests/aux_checks.py on libr2l_isp.so (and, where a launch shape is
overridden, on its diagnostic twin) -- the tile walk and the grid-stride loop at sizes where they take more than one trip,
tile and halo edges, ill-conditioned inputs, the guarded arena, AuxLoss with values."""
import pytest
import torch

import aux_checks as ac

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from raw2logit_amd import _lib
    assert _lib.device_library().is_device
    return 'cuda:0'


@pytest.mark.parametrize('grid', ac.WALK_GRIDS)
def test_ssim_tile_walk_does_not_depend_on_the_grid(grid, dev):
    ac.walk_under_hook(dev, grid)


@pytest.mark.parametrize('shape', ac.PRODUCT_WALK_SHAPES, ids=['696_tiles', '1050_tiles'])
def test_ssim_with_more_tiles_than_workgroups(shape, dev):
    ac.walk_on_product(dev, shape)


@pytest.mark.parametrize('C,H,W', ac.EDGE_CASES, ids=[f'{C}x{H}x{W}' for C, H, W in ac.EDGE_CASES])
def test_ssim_tile_and_halo_edges(C, H, W, dev):
    ac.edges(dev, C, H, W)


@pytest.mark.parametrize('kind', ac.KINDS)
def test_ssim_input_kinds(kind, dev):
    ac.kinds(dev, kind)


@pytest.mark.parametrize('grid', ac.L2_HOOK_GRIDS, ids=['default', 'grid1', 'grid3'])
def test_l2_grid_stride_loop_under_the_hook(grid, dev):
    trips = ac.l2_case(dev, ac.L2_HOOK_N, grid, hook=True)
    assert trips == {None: 1, 1: 8, 3: 3}[grid]


@pytest.mark.parametrize('n', ac.L2_PRODUCT_NS, ids=['single_lane', 'both_launches_loop'])
def test_l2_on_the_shipped_library(n, dev):
    trips = ac.l2_case(dev, n)
    assert trips == (1 if n == 4 else 3)


def test_abi_promises(dev):
    ac.abi_behaviour(dev)


def test_multi_trip_launches_stay_inside_their_allocations(dev):
    ac.guarded_multi_trip(dev)


@pytest.mark.parametrize('batch_norm', (False, True), ids=['plain', 'batchnorm_train'])
def test_aux_loss_parameter_gradients(batch_norm, dev):
    ac.aux_loss_values(dev, batch_norm)
