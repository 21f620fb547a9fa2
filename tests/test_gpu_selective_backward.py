"""The backward of a subset of the gradients (ParametrizedProcessing.selective_backward, r2l_isp_step_bwd_select) on the gfx950
build: the launch record of every route, the routes against the full backward and the float64 oracle (tests/selective_bwd_checks.py),
the fall-backs, the unchanged default, a StepGraph replay, and the reduced passes inside the guard-zone arena."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import guarded_arena as ga  # noqa: E402
import parity_checks as pc  # noqa: E402
import raw_grad_checks as rc  # noqa: E402
import selective_bwd_checks as sc  # noqa: E402
from oracle import isp_oracle as orc  # noqa: E402
from raw2logit_amd.graphs import StepGraph  # noqa: E402
from raw2logit_amd.processing import pipeline_torch as ppt  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.mark.parametrize('bn,training', rc.BN_MODES[1:], ids=['bn_train', 'bn_eval'])
@pytest.mark.parametrize('route', list(sc.ROUTES))
def test_launch_record_of_the_selective_routes(route, bn, training):
    sc.check_launches(route, bn, training, DEV, 64, 256, 256)      # (4 Mi px: the plane passes of the shipped build)


@pytest.mark.parametrize('case', rc.FUSED_CASES, ids=[c['name'] for c in rc.FUSED_CASES])
def test_selective_routes_on_the_golden_cases(case):
    sc.check_golden_case(case, DEV, routes=tuple(sc.ROUTES))


@pytest.mark.parametrize('H,W', pc.FRAME_SHAPES_PLANES + [s[1:] for s in sc.SHAPES_EXTRA] + [(70, 2048)])
def test_selective_routes_on_the_plane_frame_shapes(H, W):
    bn, training = rc.BN_MODES[(H + W) % 3]
    with pc.env_overrides(DEV, sc.PLANES):
        sc.check_shape(2, H, W, bn, training, DEV, routes=tuple(sc.ROUTES))


@pytest.mark.parametrize('H', [256, 512])
@pytest.mark.parametrize('bn,training', rc.BN_MODES[1:], ids=['bn_train', 'bn_eval'])
def test_selective_routes_at_the_benchmark_shapes(H, bn, training):
    """shipped build, no diagnostic setting: the selective routes against the full backward (grad_raw bit for bit)"""
    sc.check_shape(64, H, H, bn, training, DEV, routes=tuple(sc.ROUTES), with_oracle=False)


def test_sixteen_bit_frames_and_the_output_epilogue():
    with pc.env_overrides(DEV, sc.PLANES):
        sc.check_u16_and_epilogue(DEV)
    sc.check_u16_and_epilogue(DEV, 64, 256, 256)


def test_fall_backs_are_the_full_backward():
    sc.check_fallbacks(DEV, plane_px=True)
    sc.check_epilogue_with_raw_grad(DEV)
    # 64x256x256 with white_balance trainable: the shipped build's plane passes, attribute on and off
    raw_np = orc.synth_raw(64, 256, 256, seed=4, kind='scene')
    cot = np.random.default_rng(4).standard_normal((64, 3, 256, 256)).astype(np.float32)
    res = []
    for sel in (False, True):
        m = sc.set_trainable(rc.make_plain_module(True, DEV, True), ('white_balance', 'gamma_correct'))
        m.selective_backward = sel
        res.append(sc.step(m, raw_np, cot, DEV, True))
    sc._same(*res)
    assert any('bwd2_sums' in k for k in res[1][3])


def test_default_is_unchanged():
    sc.check_default_unchanged(DEV)
    sc.check_default_unchanged(DEV, 64, 256, 256)


@pytest.mark.parametrize('route', ['raw', 'gamma', 'blur_gamma', 'raw_blur_gamma'])
def test_step_graph_replays_the_selective_step(route):
    """a replay of the captured selective step: output, grad_raw and the asked gradients bit-identical to the eager step"""
    B, H, W = 64, 256, 256
    raw_np = orc.synth_raw(B, H, W, seed=5, kind='scene')
    cot_np = np.random.default_rng(5).standard_normal((B, 3, H, W)).astype(np.float32)
    raw_grad, names = sc.ROUTES[route]
    o_e, gr_e, g_e, k_e = sc.step(sc.plain_module(True, True, DEV, route, True), raw_np, cot_np, DEV, raw_grad)
    assert any('_sel_' in k for k in k_e)
    m = sc.plain_module(True, True, DEV, route, True)
    raw = torch.from_numpy(raw_np).to(DEV).requires_grad_(raw_grad)
    g = StepGraph(m, raw, torch.from_numpy(cot_np).to(DEV), warmup=1)
    # the captured step ACCUMULATES into the frames' gradient (raw.grad existed since the warm-up: one in-place add per replay,
    # the parameters' gradients are overwritten): zero it in place, so that the replay leaves exactly its own d/d raw there
    graw = raw.grad
    if raw_grad:
        assert graw is not None
        graw.zero_()
    out = g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.detach().cpu().numpy(), o_e)
    if raw_grad:
        assert raw.grad is graw and np.array_equal(graw.cpu().numpy(), gr_e)
    for k in names:
        assert np.array_equal(pc.NAME2ATTR[k](m).grad.cpu().numpy(), g_e[k]), k
    assert all(f(m).grad is None for k, f in pc.NAME2ATTR.items() if k not in names and k != 'additive_layer')


@pytest.mark.parametrize('route', list(sc.ROUTES))
def test_selective_passes_inside_the_guarded_arena(route):
    """every allocation of the call between poisoned guard zones: no byte outside them written, results independent of the poison"""
    B, H, W = 2, 70, 260
    raw_np = orc.synth_raw(B, H, W, seed=6, kind='scene')
    cot_np = np.random.default_rng(6).standard_normal((B, 3, H, W)).astype(np.float32)
    raw_grad, names = sc.ROUTES[route]

    def fn(arena):
        m = sc.plain_module(True, True, DEV, route, True)
        raw = arena.place(raw_np, 'raw').requires_grad_(raw_grad)
        cot = arena.place(cot_np, 'cot')
        y = m(raw)
        assert isinstance(m.stages, ppt._LazyStages)
        y.backward(cot)
        res = {'out': y, **{k: pc.NAME2ATTR[k](m).grad for k in names}}
        if raw_grad:
            res['grad_raw'] = raw.grad
        return res
    with pc.env_overrides(DEV, sc.PLANES):
        res = ga.run_both(DEV, 64 << 20, fn, f'selective {route} {B}x{H}x{W}')
    assert all(torch.isfinite(v).all() for v in res.values())
