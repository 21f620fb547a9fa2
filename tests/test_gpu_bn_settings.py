"""BatchNorm off its defaults on the gfx950 build: the checks of tests/bn_checks.py (settings x routes with the route asserted from
the launch record, sequences of steps, opt-in output types, frame content on the streaming shapes too, the C ABI's phase A /
r2l_bn_finalize / phase B and r2l_isp_fwd_stats_bn, r2l_bn_finalize against its closed form) and one whole step as a HIP graph under
momentum=None.  `timeout -k 10 600 python -m pytest tests/test_gpu_bn_settings.py -q -m gpu`"""
import copy
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import bn_checks as bc  # noqa: E402
from oracle import isp_oracle as orc  # noqa: E402
from raw2logit_amd.processing import pipeline_torch as ppt  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from raw2logit_amd import _lib
    assert _lib.device_library().is_device
    return 'cuda:0'


@pytest.mark.parametrize('route,setting,grads', bc.setting_cases())
def test_setting_on_route(dev, route, setting, grads):
    bc.check_setting(route, setting, dev, grads)


@pytest.mark.parametrize('setting', (1, 2))
@pytest.mark.parametrize('route', bc.FULL_ROUTES)
def test_sequence_of_steps(dev, route, setting):
    bc.check_sequence(route, setting, dev)


@pytest.mark.parametrize('which', ('bf16', 'nhwc'))
def test_opt_in_output_types(dev, which):
    bc.check_opt_in_io(which, dev)


@pytest.mark.parametrize('setting', ('default', 2))
@pytest.mark.parametrize('shape', bc.CONTENT_SHAPES + bc.CONTENT_SHAPES_GPU, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('kind', bc.CONTENT_KINDS)
def test_frame_content(dev, kind, shape, setting):
    bc.check_frame_content(kind, shape, bc.DEFAULT if setting == 'default' else bc.SETTINGS[setting], dev)


@pytest.mark.parametrize('setting', (1, 2, 3, 4))
def test_phase_a_finalize_phase_b_through_the_c_abi(dev, setting):
    bc.check_abi_phases(setting, dev)


@pytest.mark.parametrize('setting', (1, 2, 3, 4))
def test_fwd_stats_bn_through_the_c_abi(dev, setting):
    bc.check_abi_stats_bn(setting, dev)


def test_bn_finalize_against_the_closed_form(dev):
    bc.check_finalize_direct(dev)


def test_whole_step_as_one_hip_graph_under_cumulative_momentum(dev):
    """StepGraph with nn.BatchNorm2d(momentum=None, eps=1e-3): three replays on new buffer contents equal three eager steps bit for
    bit -- output, gradients, running statistics, and num_batches_tracked == 3 after both modules were reset to a common state: the
    factor 1 / num_batches_tracked is read on the device at replay time, not frozen into the graph at capture (the warm-up and the
    capture themselves ran at other counter values)."""
    from raw2logit_amd.graphs import StepGraph
    B, S = 6, 96
    raws = [torch.from_numpy(orc.synth_raw(B, S, S, seed=50 + i, kind='scene')).to(dev) for i in range(3)]
    cots = [torch.randn((B, 3, S, S), device=dev, generator=torch.Generator(dev).manual_seed(7 + i)) for i in range(3)]
    m = ppt.ParametrizedProcessing(orc.DRONE_CAMERA_PARAMS, batch_norm_output=True)
    m.batch_norm = bc.new_bn(bc.SETTINGS[1])
    m = m.to(dev).train()
    m2 = copy.deepcopy(m)
    raw, cot = raws[0].clone(), cots[0].clone()
    g = StepGraph(m2, raw, cot)
    assert int(m2.batch_norm.num_batches_tracked) > 0      # the warm-up steps and the capture counted
    m2.load_state_dict(m.state_dict())                     # both modules from the same state: counter 0, statistics (0, 1)
    assert int(m2.batch_norm.num_batches_tracked) == 0
    for i in range(3):
        raw.copy_(raws[i])
        cot.copy_(cots[i])
        for p in m.parameters():
            p.grad = None
        y0 = m(raws[i])
        y0.backward(cots[i])
        y1 = g.replay()
        assert torch.equal(y0, y1)
        for p, q in zip(m.parameters(), m2.parameters()):
            assert torch.equal(p.grad, q.grad)
        for k, v in m.state_dict().items():
            assert torch.equal(v, m2.state_dict()[k]), (i, k, v, m2.state_dict()[k])
    assert int(m.batch_norm.num_batches_tracked) == 3 and int(m2.batch_norm.num_batches_tracked) == 3
    # ... and the eager steps are those of a float64 nn.BatchNorm2d under the cumulative average (factor 1, 1/2, 1/3)
    ref = bc.new_bn(bc.SETTINGS[1], torch.float64)
    P64 = bc.parameters(0, perturbed=False).astype(np.float64)
    for i in range(3):
        ref(torch.from_numpy(orc.parametrized_forward(raws[i].cpu().numpy(), P64, bn=None)[0]))
    bc.compare_stats('bn/step_graph', m2.batch_norm, ref)
