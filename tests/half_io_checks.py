"""16-bit output and cotangent of the fused step (ParametrizedProcessing.output_dtype, r2l_isp_step_fwd_io / r2l_isp_step_bwd_io):
the checks tests/test_gpu_half_io.py runs on the gfx950 build.

The contract: the 16-bit module returns float32_module(raw).to(dtype) BIT FOR BIT (round to nearest even is what both do), and
its gradients are those of the float32 module on the plane route -- r2l_isp_step_bwd_raw's, which a 16-bit backward takes at
every size -- given the widened cotangent, bit for bit as well: the arithmetic between the load and the store is the same code."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import parity_checks as pc  # noqa: E402
import raw_grad_checks as rc  # noqa: E402
from oracle import isp_oracle as orc  # noqa: E402
from raw2logit_amd import _lib  # noqa: E402
from raw2logit_amd import functional as F_  # noqa: E402
from raw2logit_amd.processing import pipeline_torch as ppt  # noqa: E402

DTYPES = [torch.bfloat16, torch.float16]
DTYPE_IDS = ['bf16', 'f16']
PLANES = dict(R2L_BWD_PLANES=1)     # diagnostic build: the float32 reference takes the plane passes (and the recomputing BatchNorm sums) below their thresholds too
MANTISSA_BITS = {torch.bfloat16: 8, torch.float16: 11}      # significand bits with the hidden one
MIN_NORMAL_EXP = {torch.bfloat16: -126, torch.float16: -14}


def ulp16(x, dtype):
    """one unit in the last place of `dtype` at the magnitude of x (float64 array): 2^(floor(log2|x|) - p + 1), the subnormal
    spacing below the smallest normal number"""
    a = np.maximum(np.abs(np.asarray(x, np.float64)), 2.0 ** MIN_NORMAL_EXP[dtype])
    return 2.0 ** (np.floor(np.log2(a)) - MANTISSA_BITS[dtype] + 1)


def cotangent16(shape, seed, dtype, device):
    """a cotangent that IS a tensor of `dtype` (what a task model under autocast hands back), and the same values as float32"""
    c = torch.from_numpy(np.random.default_rng(seed).standard_normal(shape).astype(np.float32)).to(device).to(dtype)
    return c, c.float()


def grads_of(m):
    return {k: f(m).grad.detach().cpu().numpy().copy() for k, f in pc.NAME2ATTR.items()
            if k != 'additive_layer' and f(m).grad is not None}


def bn_state(m):
    b = m.batch_norm
    if b is None:
        return ()
    return (b.running_mean.clone(), b.running_var.clone(), b.num_batches_tracked.clone())


def run16(m, raw, cot16, expect_fused=True):
    """forward + backward of a module with output_dtype set; -> (out16, {grads}, grad_raw | None, forward + backward launch record)"""
    lib = _lib.library_for(raw)[0]

    def fn():
        y = m(raw)
        y.backward(cot16)
        return y
    y, names = pc.kernels_launched(lib, fn)
    assert y.dtype == m.output_dtype and y.is_contiguous() and m.buffer['processed_rgb'] is y
    io_kernels = [k for k in names if k.endswith('_bf16_kernel') or k.endswith('_f16_kernel')]
    assert bool(io_kernels) == expect_fused, (expect_fused, names)
    return y.detach(), grads_of(m), (raw.grad.detach().clone() if raw.requires_grad else None), names


def run32(m, raw, cot32):
    y = m(raw)
    y.backward(cot32)
    return y.detach(), grads_of(m), (raw.grad.detach().clone() if raw.requires_grad else None)


def same_grads(g16, g32, label):
    assert sorted(g16) == sorted(g32), (label, sorted(g16), sorted(g32))
    for k in g32:
        assert np.array_equal(g16[k], g32[k]), (label, k, float(np.abs(g16[k] - g32[k]).max()))


def check_bitwise(make, raw_t, dtype, device, label, raw_grad=False, seed=0):
    """make(): a fresh float32 module (fused_raw_grad on).  The 16-bit step against the float32 step of the same build on the plane
    route: out16 == out32.to(dtype), BatchNorm's buffers, every parameter gradient and grad_raw bit for bit"""
    B, H, W = raw_t.shape
    cot16, cot32 = cotangent16((B, 3, H, W), 31 + seed, dtype, device)
    m16, m32 = make(), make()
    m16.output_dtype = dtype
    r16 = raw_t.clone().requires_grad_(True) if raw_grad else raw_t
    # the float32 reference on the route r2l_isp_step_bwd_raw takes: frames that require grad where they can (float32 frames)
    r32 = raw_t.clone().requires_grad_(True) if raw_t.dtype == torch.float32 else raw_t
    with pc.env_overrides(device, PLANES):
        y16, g16, gr16, names = run16(m16, r16, cot16)
        y32, g32, gr32 = run32(m32, r32, cot32)
    assert isinstance(m16.stages, ppt._LazyStages)
    assert torch.equal(y16, y32.to(dtype)), (label, 'forward', float((y16.float() - y32).abs().max()))
    for a, b in zip(bn_state(m16), bn_state(m32)):
        assert torch.equal(a, b), (label, 'BatchNorm buffers')
    same_grads(g16, g32, label)
    assert len(g16) == 7
    if raw_grad:
        assert torch.equal(gr16, gr32), (label, 'grad_raw', float((gr16 - gr32).abs().max()))
    return names


def plain(bn, training, device):
    return lambda: rc.make_plain_module(bn, device, training)


def frames(B, H, W, seed, device, u16=False):
    raw = orc.synth_raw(B, H, W, seed=seed, kind='scene')
    if u16:
        return torch.from_numpy(np.round(raw * 65535.0).astype(np.uint16).view(np.int16)).to(device)
    return torch.from_numpy(raw).to(device)


def check_gamma_mask_fills_everything(dtype, device, B=2, H=12, W=264):
    """C ABI: a grad mask of GAMMA alone still runs the full route and fills every element of grad_params, with the values of the
    mask-free call"""
    from ctypes import c_void_p
    raw = frames(B, H, W, 3, device)
    cot16, _ = cotangent16((B, 3, H, W), 3, dtype, device)
    m = rc.make_plain_module(True, device, True)
    lib, stream = _lib.library_for(raw)
    io = F_.IO_CODES[dtype]
    nws = lib.r2l_isp_workspace_bytes(B, H, W)
    ws = torch.empty(nws, dtype=torch.uint8, device=device)
    out = torch.empty((B, 3, H, W), dtype=dtype, device=device)
    table = (c_void_p * 9)(*[p.data_ptr() for p in (m.black_level, m.white_balance, m.colour_correction, m.gamma_correct,
                                                    m.debayer.weight, m.sharpening_filter.weight, m.gaussian_blur.weight,
                                                    m.M_RGB_2_YUV, m.M_YUV_2_RGB)])
    bn = m.batch_norm
    KEEP = 8
    assert lib.r2l_isp_io_supported(io, 0, 0, B, H, W, KEEP) == 1
    lib.check(lib.r2l_isp_step_fwd_io(_lib.ptr(raw), 0, 1.0, table, None, F_.BN_TRAIN, _lib.ptr(bn.running_mean),
                                      _lib.ptr(bn.running_var), _lib.ptr(bn.num_batches_tracked), bn.eps, bn.momentum,
                                      _lib.ptr(out), io, _lib.ptr(ws), nws, B, H, W, 1, KEEP, None, stream), 'fwd_io')
    res = []
    for mask in (8, 0):
        gp = torch.full((_lib.R2L_P_NTRAIN,), float('nan'), dtype=torch.float32, device=device)
        _, names = pc.kernels_launched(lib, lambda: lib.check(lib.r2l_isp_step_bwd_io(
            _lib.ptr(raw), 0, 1.0, None, _lib.ptr(cot16), io, None, _lib.ptr(gp), None, F_.BN_TRAIN, _lib.ptr(ws), nws, B, H, W, 1,
            KEEP, None, stream, None, None, 0, mask), 'bwd_io'))
        assert any('bwd2_sums' in k for k in names) and not any('_sel_' in k for k in names), names
        res.append(gp.cpu().numpy())
    assert np.isfinite(res[0]).all() and np.array_equal(res[0], res[1])
    assert np.count_nonzero(res[0]) > 100
    # what the calls refuse: -3 with the reason
    assert lib.r2l_isp_io_supported(io, 0, 0, B, H, W, 0) == 0 and lib.r2l_isp_io_supported(io, 0, 1, B, 256, 256, KEEP) == 0
    assert lib.r2l_isp_io_supported(io, 0, 0, B, H, 6, KEEP) == 0 and lib.r2l_isp_io_supported(io, 0, 0, B, H, W, KEEP | 16) == 0
    e = lib.r2l_isp_step_fwd_io(_lib.ptr(raw), 0, 1.0, table, None, F_.BN_NONE, None, None, None, 1e-5, 0.1, _lib.ptr(out), io,
                                _lib.ptr(ws), nws, B, H, W, 1, 0, None, stream)
    assert e == -3 and b'R2L_STEP_KEEP_LUMA' in lib.r2l_last_error()


def check_golden_case(case, dtype, device):
    """a golden case with the 16-bit boundary against the float64 oracle: the output within the forward limit of check_param_case
    plus one unit in the last place of the type at that magnitude (the rounding of the store: half a unit, and the float32 value
    may sit on the other side of a rounding boundary from the oracle's: at most one unit in all), the gradients -- oracle fed the
    widened cotangent -- at check_param_case's limits"""
    B, H, W = case['shape']
    raw_np = orc.synth_raw(B, H, W, seed=case['seed'], kind=case['kind'])
    P = pc.build_params(case)
    m = pc.make_module(case, P, device)
    m.output_dtype = dtype
    cot16, cot32 = cotangent16((B, 3, H, W), 1000 + case['seed'], dtype, device)
    with pc.env_overrides(device, PLANES):       # (the same build as the bitwise checks; the 16-bit route does not read the setting)
        y16, grads, _, _ = run16(m, torch.from_numpy(raw_np).to(device), cot16)
    P64 = P.astype(np.float64)
    o_out, _, cache = orc.parametrized_forward(raw_np, P64, track_stages=False, bn=pc.oracle_bn(case))
    cot_np = cot32.cpu().numpy()
    nom, lo, hi = (orc.parametrized_backward(P64, cache, cot_np, **kw)[0] for kw in ({}, dict(clip_shift=1e-6), dict(clip_shift=-1e-6)))
    tol = pc.out_tolerance(cache, case['bn']) + ulp16(o_out, dtype)
    err = np.abs(y16.float().cpu().numpy().astype(np.float64) - o_out)
    worst = np.unravel_index((err / tol).argmax(), err.shape)
    name = f'half-io {DTYPE_IDS[DTYPES.index(dtype)]} {case["name"]}'
    pc.report(f'{name}/out16 vs float64 oracle (forward limit + 1 ulp16)', err[worst], tol[worst])
    assert np.all(err <= tol), (name, float(err.max()))
    rtol = case.get('grad_rtol', pc.DEFAULT_GRAD_RTOL)
    for k, og in nom.items():
        if k == 'additive_layer':
            continue
        og = np.asarray(og)
        scale = np.abs(og).max() + 1e-6
        flip = max(np.abs(np.asarray(lo[k]) - og).max(), np.abs(np.asarray(hi[k]) - og).max())
        lim = rtol * scale + flip
        ach = pc.achieved_grad_baseline().get(f'{case["name"]}/{k}')
        if ach is not None:
            lim = min(lim, max(pc.ACHIEVED_K * ach, pc.PLANE_GRAD_RTOL * scale + flip))
        e = np.abs(grads[k].reshape(og.shape) - og).max()
        pc.report(f'{name}/grad {k} vs float64 oracle (widened cotangent)', e, lim)
        assert e <= lim, (name, k, float(e), float(lim))


def check_fallback(make, raw_t, dtype, device, label, arm=None, raw_grad=False):
    """a call the 16-bit kernels do not serve: the float32 path + torch's cast -- f32.to(dtype) bit for bit, no 16-bit kernel in
    the launch record, and the gradients of the float32 module given the widened cotangent"""
    B = raw_t.shape[0]
    m16, m32 = make(), make()
    m16.output_dtype = dtype
    if arm is not None:
        m16.__dict__['_epilogue'] = arm
        m32.__dict__['_epilogue'] = arm
    r16 = raw_t.clone().requires_grad_(True) if raw_grad else raw_t
    r32 = raw_t.clone().requires_grad_(True) if raw_grad else raw_t
    lib = _lib.library_for(raw_t)[0]
    y16, names = pc.kernels_launched(lib, lambda: m16(r16))
    assert not any(k.endswith('_bf16_kernel') or k.endswith('_f16_kernel') for k in names), (label, names)
    y32 = m32(r32)
    assert y16.dtype == dtype and torch.equal(y16.detach(), y32.detach().to(dtype)), label
    assert m16.buffer['processed_rgb'] is y16
    if m16.stages is not None and m16.track_stages:
        assert all(v.dtype == torch.float32 for v in m16.stages.values())
    cot16, cot32 = cotangent16(tuple(y16.shape), 9, dtype, device)
    y16.backward(cot16)
    y32.backward(cot32)
    g16 = {k: f(m16).grad.detach().cpu().numpy() for k, f in pc.NAME2ATTR.items() if f(m16) is not None and f(m16).grad is not None}
    g32 = {k: f(m32).grad.detach().cpu().numpy() for k, f in pc.NAME2ATTR.items() if f(m32) is not None and f(m32).grad is not None}
    same_grads(g16, g32, label)
    assert len(g16) >= 7
    if raw_grad:
        assert torch.equal(r16.grad, r32.grad), label
    del B


def check_default_unchanged(device, B=2, H=12, W=264):
    """output_dtype = None (the default) and torch.float32: the launch record and the results of a module that never heard of the
    attribute (the class default removed from the picture: a subclass-free module with the attribute deleted is the same object)"""
    raw_np = orc.synth_raw(B, H, W, seed=4, kind='scene')
    cot = np.random.default_rng(4).standard_normal((B, 3, H, W)).astype(np.float32)
    import selective_bwd_checks as sc
    res = []
    for odt in ('unset', None, torch.float32):
        m = rc.make_plain_module(True, device, True)
        m.fused_raw_grad = False
        if odt != 'unset':
            m.output_dtype = odt
        assert ppt.ParametrizedProcessing.output_dtype is None
        raw = torch.from_numpy(raw_np).to(device)
        lib = _lib.library_for(raw)[0]
        y, fwd = pc.kernels_launched(lib, lambda: m(raw))
        assert y.dtype == torch.float32
        _, bwd = pc.kernels_launched(lib, lambda: y.backward(torch.from_numpy(cot).to(device)))
        res.append((y.detach().cpu().numpy(), None, grads_of(m), {**fwd, **bwd}))
    for r in res[1:]:
        sc._same(res[0], r)
        assert sorted(r[3]) == sorted(res[0][3]) and not any('_bf16' in k or '_f16' in k for k in r[3]), r[3]
