"""BatchNorm off its defaults (eps, momentum, track_running_stats, mode, sequences of steps, frame content) without a GPU: the checks
of tests/bn_checks.py on the serial emulation (the tile forms of the kernels, the stand-alone finalize launch, the staged path, the
Python mode choice), and the device forms -- the streaming statistics kernel's own finalization among them -- under the sanitizers
in subcommand `bn_settings` of the stand-alone driver program (tests/emul/r2l_bn_settings_lockstep.cpp)."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import bn_checks as bc  # noqa: E402
import lockstep_driver  # noqa: E402

DEV = 'cpu'


@pytest.mark.parametrize('route,setting,grads', bc.setting_cases())
def test_setting_on_route(emulation, route, setting, grads):
    bc.check_setting(route, setting, DEV, grads)


@pytest.mark.parametrize('setting', (1, 2))
@pytest.mark.parametrize('route', bc.FULL_ROUTES)
def test_sequence_of_steps(emulation, route, setting):
    bc.check_sequence(route, setting, DEV)


@pytest.mark.parametrize('which', ('bf16', 'nhwc'))
def test_opt_in_output_types(emulation, which):
    bc.check_opt_in_io(which, DEV)


@pytest.mark.parametrize('setting', ('default', 2))
@pytest.mark.parametrize('shape', bc.CONTENT_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('kind', bc.CONTENT_KINDS)
def test_frame_content(emulation, kind, shape, setting):
    bc.check_frame_content(kind, shape, bc.DEFAULT if setting == 'default' else bc.SETTINGS[setting], DEV)


@pytest.mark.parametrize('setting', (1, 2, 3, 4))
def test_phase_a_finalize_phase_b_through_the_c_abi(emulation, setting):
    bc.check_abi_phases(setting, DEV)


@pytest.mark.parametrize('setting', (1, 2, 3, 4))
def test_fwd_stats_bn_through_the_c_abi(emulation, setting):
    bc.check_abi_stats_bn(setting, DEV)


def test_bn_finalize_against_the_closed_form(emulation):
    bc.check_finalize_direct(DEV)


def test_device_forms_under_the_sanitizers():
    """`r2l_lockstep_drivers bn_settings`: r2l_isp_step_fwd with BN_NONE, then BN_TRAIN (whole step, and phase A + r2l_bn_finalize +
    phase B) at the case's eps / momentum / buffers, three steps in a row in a malloc workspace of exactly the queried size, against
    long-double statistics of the library's own pre-normalisation output"""
    r = lockstep_driver.run('bn_settings', timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert 'Sanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr[-3000:]
    lines = [line for line in r.stdout.splitlines() if line.startswith('case ')]
    assert len(lines) == 24 and all(line.endswith(' ok') for line in lines), r.stdout[-3000:]
