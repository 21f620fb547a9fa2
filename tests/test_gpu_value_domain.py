"""The step off its usual parameters, buffers and value range on the gfx950 build: the checks of tests/value_domain_checks.py with the
route asserted from the launch record (the streaming forward at 1, 2, 4 and 8 wavefronts per row, the plane passes and the recomputing
BatchNorm sums behind a 16-bit / channels-last cotangent, the reduced passes of the selective backward, d/d raw on the fused kernels).
`timeout -k 10 900 python -m pytest tests/test_gpu_value_domain.py -q -m gpu`"""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import value_domain_checks as vd  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from raw2logit_amd import _lib
    assert _lib.device_library().is_device
    return 'cuda:0'


@pytest.mark.parametrize('route,setting,bn,bits', vd.setting_cases(True))
def test_setting_on_route(dev, route, setting, bn, bits):
    vd.check_setting(route, setting, bn, dev, bits)


@pytest.mark.parametrize('route,bn', vd.outlier_cases(True))
def test_frames_outside_the_unit_range(dev, route, bn):
    vd.check_outliers(route, bn, dev)


@pytest.mark.parametrize('bn', vd.BN_MODES)
@pytest.mark.parametrize('cot_type', list(vd.COT_TYPES))
@pytest.mark.parametrize('position', list(vd.COT_POSITIONS))
@pytest.mark.parametrize('value', list(vd.NONFINITE))
def test_nonfinite_cotangent_is_neither_swallowed_nor_spread(dev, value, position, cot_type, bn):
    vd.check_cotangent(value, position, cot_type, bn, dev, raw_grad=True)


@pytest.mark.parametrize('bn', vd.BN_MODES)
def test_overflowed_float16_cotangent_reaches_the_gradients(dev, bn):
    vd.check_grad_scaler(dev, bn)


@pytest.mark.parametrize('route,value,position', vd.frame_value_cases())
def test_nonfinite_frame_value(dev, route, value, position):
    vd.check_frame_value(route, value, position, dev)
