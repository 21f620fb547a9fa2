"""The common-corruption kernels on the MI355X: the checks of tests/corruption_checks.py at batch shapes, and the sweep's
chain end to end (static ISP -> corruption -> Normalize on the device) against the oracle on the host."""
import numpy as np
import pytest
import torch

import corruption_checks as cc
import corruption_oracle as co
import parity_checks as pc

pytestmark = pytest.mark.gpu

SHAPES = ((4, 3, 130, 130), (2, 3, 66, 130), (8, 3, 256, 256))


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from raw2logit_amd import _lib
    assert _lib.device_library().is_device
    return 'cuda:0'


def test_kernels_match_the_reference_goldens(dev):
    cc.check_goldens(dev)


@pytest.mark.parametrize('transform', cc.DETERMINISTIC)
def test_kernels_match_the_oracle(dev, transform):
    cc.check_oracle_parity(dev, transform, SHAPES)


def test_identity_and_noise_identities(dev):
    cc.check_identity(dev)
    for shape in SHAPES:
        cc.check_noise_identities(dev, shape)


def test_launch_shape_independence(dev):
    for shape in SHAPES:
        cc.check_launch_shape_independence(dev, shape)


def test_impulse_noise_distribution(dev):
    cc.check_impulse_distribution(dev)


def test_shot_noise_distribution(dev):
    cc.check_shot_distribution(dev)


def test_errors_and_dtypes(dev):
    cc.check_errors(dev)
    cc.check_dtypes(dev)


@pytest.mark.parametrize('transform', ('contrast', 'zoom_blur'))
def test_sweep_chain_end_to_end(dev, transform):
    """Compose([RawProcessingPipeline, Distortions(3, t), Normalize]) as the library runs it -- the batched static chain, then
    one corruption launch with the Normalize in its stores, all on the device -- against RawProcessingPipeline's own output
    image by image, fed through the oracle on the host"""
    from oracle import isp_oracle as orc
    from raw2logit_amd import corruptions as C
    from raw2logit_amd import functional as F_
    from raw2logit_amd.processing.pipeline_numpy import RawProcessingPipeline
    raw = orc.synth_raw(4, 256, 256, seed=9, kind='scene')
    chain = ('bilinear', 'sharpening_filter', 'gaussian_denoising')
    rgb = F_.static_pipeline(torch.from_numpy(raw).to(dev), orc.DRONE_CAMERA_PARAMS, *chain)
    y = C.corrupt(rgb, transform, 3, mean=cc.MEAN, std=cc.STD).cpu().numpy()
    per_image = RawProcessingPipeline(orc.DRONE_CAMERA_PARAMS, *chain)
    host = np.stack([per_image(raw[i].copy()).numpy() for i in range(raw.shape[0])])
    ref = co.normalize(co.apply(host, transform, 3), cc.MEAN, cc.STD)
    err = np.abs(y.astype(np.float64) - ref).max()
    pc.report(f'static chain -> {transform} s3 -> Normalize, 4x256x256 [{dev}]', err, cc.ATOL / min(cc.STD))
    assert err <= cc.ATOL / min(cc.STD), (transform, err)
