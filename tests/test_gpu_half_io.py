"""16-bit output and cotangent of the fused step (ParametrizedProcessing.output_dtype = torch.bfloat16 / torch.float16,
r2l_isp_step_fwd_io / r2l_isp_step_bwd_io) on the gfx950 build: forward and backward bit for bit against the float32 step
(tests/half_io_checks.py), the reference's golden cases within the derived rounding margin, the fall-backs, the unchanged default, a
StepGraph replay and one case inside the guard-zone arena."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import guarded_arena as ga  # noqa: E402
import half_io_checks as hc  # noqa: E402
import parity_checks as pc  # noqa: E402
import raw_grad_checks as rc  # noqa: E402
import selective_bwd_checks as sc  # noqa: E402
from oracle import isp_oracle as orc  # noqa: E402
from raw2logit_amd.graphs import StepGraph  # noqa: E402
from raw2logit_amd.processing import pipeline_torch as ppt  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
both = pytest.mark.parametrize('dtype', hc.DTYPES, ids=hc.DTYPE_IDS)

# the smallest shapes that can go wrong: every border row / partial strip / band edge of the plane passes' own list, a last strip of
# one lane, a partially filled strip, 8 wavefronts per row, the smallest frame
SHAPES = [(2, H, W) for H, W in pc.FRAME_SHAPES_PLANES] + list(sc.SHAPES_EXTRA) + [(2, 70, 2048), (1, 4, 4)]


@both
@pytest.mark.parametrize('B,H,W', SHAPES, ids=[f'{b}x{h}x{w}' for b, h, w in SHAPES])
def test_forward_and_backward_bitwise_on_the_frame_shapes(B, H, W, dtype):
    """BatchNorm none / train / eval in turn over the shapes; d/d raw requested on every other one"""
    bn, training = rc.BN_MODES[(H + W) % 3]
    raw_grad = bool((H // 2 + W // 4) & 1)
    names = hc.check_bitwise(hc.plain(bn, training, DEV), hc.frames(B, H, W, 1, DEV), dtype, DEV,
                             f'{B}x{H}x{W} bn={bn} train={training} raw_grad={raw_grad}', raw_grad=raw_grad)
    if raw_grad:
        assert any('bwd1_plane_guv_' in k for k in names) and any('bwd_raw_plane' in k for k in names), names


@both
@pytest.mark.parametrize('bn,training', rc.BN_MODES, ids=['bn_none', 'bn_train', 'bn_eval'])
@pytest.mark.parametrize('u16', [False, True], ids=['f32_frames', 'u16_frames'])
def test_batchnorm_modes_and_frame_containers(bn, training, u16, dtype):
    B, H, W = 2, 70, 260
    names = hc.check_bitwise(hc.plain(bn, training, DEV), hc.frames(B, H, W, 2, DEV, u16=u16), dtype, DEV,
                             f'bn={bn} train={training} u16={u16}')
    sfx = ('_u16' if u16 else '') + ('_bf16' if dtype is torch.bfloat16 else '_f16') + '_kernel'
    want = ['r2l_launch_bwd1_plane' + sfx] + (['r2l_launch_fwd_apply' + sfx, 'r2l_launch_bnr_planes' + sfx] if bn and training
                                              else ['r2l_launch_fwd_stream_w2' + sfx])
    assert all(names.get(k) == 1 for k in want), (want, names)


@both
def test_gamma_mask_alone_fills_all_of_grad_params(dtype):
    hc.check_gamma_mask_fills_everything(dtype, DEV)


@both
@pytest.mark.parametrize('case', rc.FUSED_CASES, ids=[c['name'] for c in rc.FUSED_CASES])
def test_golden_cases_against_the_oracle(case, dtype):
    hc.check_golden_case(case, dtype, DEV)


@both
def test_golden_cases_bitwise(dtype):
    for case in rc.FUSED_CASES:
        B, H, W = case['shape']
        P = pc.build_params(case)
        raw = torch.from_numpy(orc.synth_raw(B, H, W, seed=case['seed'], kind=case['kind'])).to(DEV)

        def make():
            m = pc.make_module(case, P, DEV)
            m.fused_raw_grad = True
            return m
        hc.check_bitwise(make, raw, dtype, DEV, case['name'])


@both
def test_fall_backs_are_the_float32_path_and_a_cast(dtype):
    def additive():
        m = rc.make_plain_module(True, 'cpu', True)
        ppt.append_additive_layer(m)
        return m.to(DEV)

    def tracked():
        m = rc.make_plain_module(True, DEV, True)
        m.track_stages = True
        return m
    hc.check_fallback(additive, hc.frames(1, 256, 256, 3, DEV), dtype, DEV, 'an additive layer')
    hc.check_fallback(hc.plain(True, True, DEV), hc.frames(2, 12, 6, 3, DEV), dtype, DEV, 'W = 6 (ragged)')
    hc.check_fallback(hc.plain(True, True, DEV), hc.frames(2, 12, 264, 3, DEV), dtype, DEV, 'an armed epilogue', arm=(True, False, 2))
    hc.check_fallback(tracked, hc.frames(2, 12, 264, 3, DEV), dtype, DEV, 'track_stages=True')
    # no backward will run: the float32 kernels and a cast as well
    m = rc.make_plain_module(True, DEV, False)
    m.output_dtype = dtype
    raw = hc.frames(2, 12, 264, 3, DEV)
    with torch.no_grad():
        y = m(raw)
        m.output_dtype = None
        assert y.dtype == dtype and torch.equal(y, m(raw).to(dtype))


def test_default_is_unchanged():
    hc.check_default_unchanged(DEV)
    hc.check_default_unchanged(DEV, 64, 256, 256)


def test_bad_dtype_and_half_module_raise():
    from raw2logit_amd import _lib
    m = rc.make_plain_module(True, DEV, True)
    m.output_dtype = torch.float64
    with pytest.raises(_lib.R2LError):
        m(hc.frames(2, 12, 264, 3, DEV))
    m.output_dtype = torch.bfloat16
    with pytest.raises(TypeError):
        m.half()(hc.frames(2, 12, 264, 3, DEV))


def test_step_graph_replays_a_bf16_step():
    """a replay of the captured bfloat16 train-mode step: output and every gradient bit-identical to the eager step"""
    B, H, W = 4, 64, 64
    raw = hc.frames(B, H, W, 5, DEV)
    cot16, _ = hc.cotangent16((B, 3, H, W), 5, torch.bfloat16, DEV)
    me = rc.make_plain_module(True, DEV, True)
    me.output_dtype = torch.bfloat16
    y_e, g_e, _, names = hc.run16(me, raw, cot16)
    m = rc.make_plain_module(True, DEV, True)
    m.output_dtype = torch.bfloat16
    g = StepGraph(m, raw, cot16, warmup=1)
    out = g.replay()
    torch.cuda.synchronize()
    assert out.dtype == torch.bfloat16 and torch.equal(out.detach(), y_e)
    for k, v in g_e.items():
        assert np.array_equal(pc.NAME2ATTR[k](m).grad.cpu().numpy(), v), k


@both
def test_sixteen_bit_step_inside_the_guarded_arena(dtype):
    """every allocation of the call -- the 2-byte output and cotangent among them -- between poisoned guard zones: no byte outside
    them written, results independent of the poison"""
    B, H, W = 2, 70, 260
    raw_np = orc.synth_raw(B, H, W, seed=6, kind='scene')
    cot16, _ = hc.cotangent16((B, 3, H, W), 6, dtype, DEV)

    def fn(arena):
        m = rc.make_plain_module(True, DEV, True)
        m.output_dtype = dtype
        raw = arena.place(raw_np, 'raw').requires_grad_(True)
        cot = arena.place(cot16, 'cot16')
        y = m(raw)
        assert y.dtype == dtype and isinstance(m.stages, ppt._LazyStages)
        y.backward(cot)
        return {'out': y, 'grad_raw': raw.grad, **{k: pc.NAME2ATTR[k](m).grad for k in hc.grads_of(m)}}
    res = ga.run_both(DEV, 64 << 20, fn, f'half-io {dtype} {B}x{H}x{W}')
    assert all(torch.isfinite(v.float()).all() for v in res.values())
