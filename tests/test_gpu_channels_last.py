"""Channels-last output and cotangent of the fused step (ParametrizedProcessing.output_memory_format = torch.channels_last,
r2l_isp_step_fwd_layout / r2l_isp_step_bwd_layout) on the gfx950 build: forward and backward bit for bit against the planar step
(tests/channels_last_checks.py) in float32 / bfloat16 / float16, the cotangent's strides, the reference's golden cases, the
fall-backs, the unchanged default, a StepGraph replay, one case per element type inside the guard-zone arena and one step under a
channels-last ResNet stand-in."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import channels_last_checks as cc  # noqa: E402
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
CL = torch.channels_last
every = pytest.mark.parametrize('dtype', cc.DTYPES, ids=cc.DTYPE_IDS)

# the smallest shapes that can go wrong: every border row / partial strip / band edge of the plane passes' own list, a last strip of
# one lane, a partially filled strip, 8 wavefronts per row, the smallest frame
SHAPES = [(2, H, W) for H, W in pc.FRAME_SHAPES_PLANES] + list(sc.SHAPES_EXTRA) + [(2, 70, 2048), (1, 4, 4)]


@every
@pytest.mark.parametrize('B,H,W', SHAPES, ids=[f'{b}x{h}x{w}' for b, h, w in SHAPES])
def test_forward_and_backward_bitwise_on_the_frame_shapes(B, H, W, dtype):
    """BatchNorm none / train / eval in turn over the shapes; d/d raw requested on every other one.  The launch record holds the
    channels-last kernels and no conversion"""
    bn, training = rc.BN_MODES[(H + W) % 3]
    raw_grad = bool((H // 2 + W // 4) & 1)
    names = cc.check_bitwise(hc.plain(bn, training, DEV), hc.frames(B, H, W, 1, DEV), dtype, DEV,
                             f'{B}x{H}x{W} bn={bn} train={training} raw_grad={raw_grad}', raw_grad=raw_grad)
    sfx = cc.suffix(dtype)
    assert names.get('r2l_launch_bwd1_plane' + ('_guv' if raw_grad else '') + sfx) == 1, names
    if raw_grad:
        assert any('bwd_raw_plane' in k for k in names), names
    if bn and training:
        assert names.get('r2l_launch_fwd_apply' + sfx) == 1 and names.get('r2l_launch_bnr_planes' + sfx) == 1, names
    else:
        nw = 1 if W <= 256 else (2 if W <= 512 else (4 if W <= 1024 else 8))
        assert names.get(f'r2l_launch_fwd_stream_w{nw}' + sfx) == 1, names


@every
@pytest.mark.parametrize('bn,training', rc.BN_MODES, ids=['bn_none', 'bn_train', 'bn_eval'])
@pytest.mark.parametrize('u16', [False, True], ids=['f32_frames', 'u16_frames'])
def test_batchnorm_modes_and_frame_containers(bn, training, u16, dtype):
    B, H, W = 2, 70, 260
    names = cc.check_bitwise(hc.plain(bn, training, DEV), hc.frames(B, H, W, 2, DEV, u16=u16), dtype, DEV,
                             f'bn={bn} train={training} u16={u16}')
    sfx = cc.suffix(dtype, u16)
    want = ['r2l_launch_bwd1_plane' + sfx] + (['r2l_launch_fwd_apply' + sfx, 'r2l_launch_bnr_planes' + sfx] if bn and training
                                              else ['r2l_launch_fwd_stream_w2' + sfx])
    assert all(names.get(k) == 1 for k in want), (want, names)
    assert sorted(k for k in names if cc.is_nhwc_kernel(k)) == sorted(want), names


@every
@pytest.mark.parametrize('layout', ['planar', 'channels_last', 'view'])
def test_cotangent_of_any_strides(layout, dtype):
    """a planar cotangent, a channels-last one and a non-contiguous view all give the gradients of the planar step"""
    B, H, W = 2, 12, 264
    cc.check_bitwise(hc.plain(True, True, DEV), hc.frames(B, H, W, 3, DEV), dtype, DEV, f'cotangent {layout}', raw_grad=True,
                     cot_layout=layout)


@every
@pytest.mark.parametrize('case', rc.FUSED_CASES, ids=[c['name'] for c in rc.FUSED_CASES])
def test_golden_cases_against_the_oracle(case, dtype):
    cc.check_golden_case(case, dtype, DEV)


@every
def test_fall_backs_are_the_default_path_and_a_conversion(dtype):
    def additive():
        m = rc.make_plain_module(True, 'cpu', True)
        ppt.append_additive_layer(m)
        return m.to(DEV)

    def tracked():
        m = rc.make_plain_module(True, DEV, True)
        m.track_stages = True
        return m
    cc.check_fallback(additive, hc.frames(1, 256, 256, 3, DEV), dtype, DEV, 'an additive layer')
    cc.check_fallback(hc.plain(True, True, DEV), hc.frames(2, 12, 6, 3, DEV), dtype, DEV, 'W = 6 (ragged)')
    cc.check_fallback(hc.plain(True, True, DEV), hc.frames(2, 12, 264, 3, DEV), dtype, DEV, 'an armed epilogue', arm=(True, False, 2))
    cc.check_fallback(tracked, hc.frames(2, 12, 264, 3, DEV), dtype, DEV, 'track_stages=True')
    # no backward will run: the planar kernels and a conversion as well
    m = cc.configure(rc.make_plain_module(True, DEV, False), dtype)
    raw = hc.frames(2, 12, 264, 3, DEV)
    with torch.no_grad():
        from raw2logit_amd import _lib
        y, names = pc.kernels_launched(_lib.library_for(raw)[0], lambda: m(raw))
        assert not any(cc.is_nhwc_kernel(k) for k in names), names
        m.output_memory_format = None
        assert y.dtype == dtype and y.is_contiguous(memory_format=CL) and torch.equal(y, m(raw).contiguous(memory_format=CL))


def test_default_is_unchanged():
    """the attribute unset: the kernels and the bits of a module without it -- and those the 16-bit PR's check pins for the same
    shapes (half_io_checks.check_default_unchanged)"""
    for shape in ((2, 12, 264), (64, 256, 256)):
        a = cc.check_default_unchanged(DEV, *shape)
        assert not any('_nhwc' in k or '_bf16' in k or '_f16' in k for k in a[3]), a[3]
        hc.check_default_unchanged(DEV, *shape)


def test_bad_memory_format_raises():
    from raw2logit_amd import _lib
    m = rc.make_plain_module(True, DEV, True)
    m.output_memory_format = torch.channels_last_3d
    with pytest.raises(_lib.R2LError):
        m(hc.frames(2, 12, 264, 3, DEV))


def test_step_graph_replays_a_channels_last_bf16_step():
    """a replay of the captured channels-last bfloat16 train-mode step: output and every gradient bit-identical to the eager step"""
    B, H, W = 4, 64, 64
    dtype = torch.bfloat16
    raw = hc.frames(B, H, W, 5, DEV)
    cot, _ = cc.cotangent((B, 3, H, W), 5, dtype, DEV)
    me = cc.configure(rc.make_plain_module(True, DEV, True), dtype)
    y_e, g_e, _, names = cc.run_cl(me, raw, cot, dtype)
    m = cc.configure(rc.make_plain_module(True, DEV, True), dtype)
    g = StepGraph(m, raw, cot, warmup=1)
    out = g.replay()
    torch.cuda.synchronize()
    assert out.dtype == dtype and out.is_contiguous(memory_format=CL) and torch.equal(out.detach(), y_e)
    for k, v in g_e.items():
        assert np.array_equal(pc.NAME2ATTR[k](m).grad.cpu().numpy(), v), k


@every
def test_channels_last_step_inside_the_guarded_arena(dtype):
    """every allocation of the call -- the interleaved output and cotangent among them -- between poisoned guard zones: no byte
    outside them written, results independent of the poison"""
    B, H, W = 2, 70, 260
    raw_np = orc.synth_raw(B, H, W, seed=6, kind='scene')
    cot, _ = cc.cotangent((B, 3, H, W), 6, dtype, DEV)
    cot_nhwc = cot.permute(0, 2, 3, 1).contiguous()        # the same bytes as a plain (B,H,W,3) block: what the arena places

    def fn(arena):
        m = cc.configure(rc.make_plain_module(True, DEV, True), dtype)
        raw = arena.place(raw_np, 'raw').requires_grad_(True)
        c = arena.place(cot_nhwc, 'cot').permute(0, 3, 1, 2)
        assert c.is_contiguous(memory_format=CL)
        y = m(raw)
        assert y.dtype == dtype and y.is_contiguous(memory_format=CL) and isinstance(m.stages, ppt._LazyStages)
        y.backward(c)
        return {'out': y, 'grad_raw': raw.grad, **{k: pc.NAME2ATTR[k](m).grad for k in hc.grads_of(m)}}
    res = ga.run_both(DEV, 64 << 20, fn, f'channels-last {dtype} {B}x{H}x{W}')
    assert all(torch.isfinite(v.float()).all() for v in res.values())


def test_one_step_under_a_channels_last_resnet():
    """ISP -> ResNet stand-in converted to channels_last, 4x64x64, float32 output: loss and ISP gradients finite, and the ISP's
    parameter gradients those of the run with the attribute unset, within the stand-in's own run-to-run reproducibility, measured
    here by running the unset configuration twice.

    What the unset configuration is: today's channels-last caller, i.e. the planar output made channels-last by the caller
    (x.contiguous(memory_format=torch.channels_last)) in front of the same network, its backward on the plane route that a
    channels-last backward always takes (R2L_BWD_PLANES in the diagnostic build, as in the bitwise checks).  The network then sees
    the same values in the same strides in both configurations.  MIOpen's algorithm choice is pinned for the duration
    (torch.backends.cudnn.deterministic): measured on an MI355X without it, two unset runs differ by 6e-5 .. 1.1e-4 in the
    black-level gradient (scale 63) while any third run differs from the first by 1e-4 .. 4.5e-4 -- one draw of that noise is no
    limit for another draw; with it the unset configuration reproduces exactly (0.0 on all seven gradients), so the limit is 0 and
    the check is bitwise.  (Fed the PLANAR tensor instead, the network's first convolution converts it itself and sums in
    another order: 3.8e-6 on the black-level gradient with the reproducibility at 0.)"""
    import standin_models as sm
    B, H, W = 4, 64, 64
    raw = hc.frames(B, H, W, 8, DEV)
    target = torch.arange(B, device=DEV) % 3

    def step(omf):
        torch.manual_seed(0)
        isp = rc.make_plain_module(True, DEV, True)
        isp.output_memory_format = omf
        net = sm.ResNet18(n_classes=3).to(DEV).to(memory_format=CL).train()
        x = isp(raw)
        assert x.is_contiguous(memory_format=CL) == (omf is CL)
        loss = torch.nn.functional.cross_entropy(net(x.contiguous(memory_format=CL)), target)
        loss.backward()
        return float(loss.detach()), hc.grads_of(isp)
    pinned = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        with pc.env_overrides(DEV, cc.PLANES):
            l0, g0 = step(None)
            l1, g1 = step(None)
            lc, gc = step(CL)
    finally:
        torch.backends.cudnn.deterministic = pinned
    assert np.isfinite(lc) and all(np.isfinite(v).all() for v in gc.values()) and len(gc) == 7
    for k in g0:
        repro = np.abs(g0[k] - g1[k]).max()
        err = np.abs(gc[k] - g0[k]).max()
        pc.report(f'channels-last resnet 4x64x64/grad {k} vs attribute unset (limit: run-to-run of the unset configuration)', err, repro)
        assert err <= repro, (k, float(err), f'measured run-to-run reproducibility of the unset configuration: {float(repro):.3e}')
