"""The step off its usual parameters, buffers and value range without a GPU: the checks of tests/value_domain_checks.py on the serial
emulation (the tile forms of the kernels, the staged path, the Python wrappers)."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import value_domain_checks as vd  # noqa: E402

DEV = 'cpu'


@pytest.mark.parametrize('route,setting,bn,bits', vd.setting_cases(False))
def test_setting_on_route(emulation, route, setting, bn, bits):
    vd.check_setting(route, setting, bn, DEV, bits)


@pytest.mark.parametrize('route,bn', vd.outlier_cases(False))
def test_frames_outside_the_unit_range(emulation, route, bn):
    vd.check_outliers(route, bn, DEV)


@pytest.mark.parametrize('bn', vd.BN_MODES)
@pytest.mark.parametrize('cot_type', list(vd.COT_TYPES))
@pytest.mark.parametrize('position', list(vd.COT_POSITIONS))
@pytest.mark.parametrize('value', list(vd.NONFINITE))
def test_nonfinite_cotangent_is_not_swallowed(emulation, value, position, cot_type, bn):
    """(d/d raw on the fused kernels, and with it the containment half, needs the plane passes: GPU only)"""
    vd.check_cotangent(value, position, cot_type, bn, DEV, raw_grad=False)


@pytest.mark.parametrize('bn', vd.BN_MODES)
def test_overflowed_float16_cotangent_reaches_the_gradients(emulation, bn):
    vd.check_grad_scaler(DEV, bn)


@pytest.mark.parametrize('route,value,position', vd.frame_value_cases())
def test_nonfinite_frame_value(emulation, route, value, position):
    vd.check_frame_value(route, value, position, DEV)


def test_integration_document_states_what_is_asserted():
    with open(os.path.join(os.path.dirname(HERE), 'INTEGRATION.md')) as f:
        text = ' '.join(f.read().split())
    section = text[text.index('## Values outside the ordinary'):]
    for sentence in vd.DOC_NONFINITE_FRAME + vd.DOC_OTHER_ROWS:
        assert sentence in section, sentence
