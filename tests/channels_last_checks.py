"""Channels-last output and cotangent of the fused step (ParametrizedProcessing.output_memory_format = torch.channels_last,
r2l_isp_step_fwd_layout / r2l_isp_step_bwd_layout): the checks tests/test_gpu_channels_last.py runs on the gfx950 build and
tests/test_channels_last.py on the lock-step emulation.

The contract: the channels-last module returns default_module(raw).contiguous(memory_format=torch.channels_last) BIT FOR BIT, in
float32, bfloat16 or float16, and its gradients are those of the planar module on the plane route -- which a channels-last backward
takes at every size, like a 16-bit one -- given the same cotangent values, bit for bit as well: only the addresses of the two
tensors that cross the boundary differ."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import half_io_checks as hc  # noqa: E402
import parity_checks as pc  # noqa: E402
import raw_grad_checks as rc  # noqa: E402
from oracle import isp_oracle as orc  # noqa: E402
from raw2logit_amd import _lib  # noqa: E402
from raw2logit_amd.processing import pipeline_torch as ppt  # noqa: E402

CL = torch.channels_last
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
DTYPE_IDS = ['f32', 'bf16', 'f16']
PLANES = hc.PLANES      # the planar float32 comparison step takes the plane passes (and the recomputing BatchNorm sums) too


def is_nhwc_kernel(name):
    return name.endswith('_nhwc_kernel')


def suffix(dtype, u16=False):
    """of the channels-last kernels' names for an output type and a frame container"""
    return ('_u16' if u16 else '') + {torch.float32: '', torch.bfloat16: '_bf16', torch.float16: '_f16'}[dtype] + '_nhwc_kernel'


def cotangent(shape, seed, dtype, device, layout='channels_last'):
    """a cotangent of `dtype` as a channels-last consumer hands it back (or planar, or a non-contiguous view), and its values
    as planar float32"""
    c = torch.from_numpy(np.random.default_rng(seed).standard_normal(shape).astype(np.float32)).to(device).to(dtype)
    c32 = c.float().contiguous()
    if layout == 'channels_last':
        c = c.contiguous(memory_format=CL)
    elif layout == 'view':      # every other column of a tensor twice as wide: no memory format at all
        wide = torch.zeros(shape[:3] + (2 * shape[3],), dtype=dtype, device=device)
        wide[..., ::2] = c
        c = wide[..., ::2]
        assert not c.is_contiguous() and not c.is_contiguous(memory_format=CL)
    return c, c32


def configure(m, dtype):
    m.output_memory_format = CL
    m.output_dtype = None if dtype is torch.float32 else dtype
    return m


def run_cl(m, raw, cot, dtype, expect_fused=True):
    """forward + backward of a module with output_memory_format = channels_last; -> (out, {grads}, grad_raw | None, launch record)"""
    lib = _lib.library_for(raw)[0]

    def fn():
        y = m(raw)
        y.backward(cot)
        return y
    y, names = pc.kernels_launched(lib, fn)
    assert y.dtype == dtype and tuple(y.shape) == (raw.shape[0], 3, raw.shape[1], raw.shape[2])
    assert y.is_contiguous(memory_format=CL) and m.buffer['processed_rgb'] is y
    nhwc = [k for k in names if is_nhwc_kernel(k)]
    assert bool(nhwc) == expect_fused, (expect_fused, names)
    return y.detach(), hc.grads_of(m), (raw.grad.detach().clone() if raw.requires_grad else None), names


def check_bitwise(make, raw_t, dtype, device, label, raw_grad=False, seed=0, cot_layout='channels_last'):
    """make(): a fresh default module (fused_raw_grad on).  The channels-last step against the planar step of the same element
    type's values on the plane route: the output permuted, BatchNorm's buffers, every parameter gradient and grad_raw bit for bit"""
    B, H, W = raw_t.shape
    cot, cot32 = cotangent((B, 3, H, W), 31 + seed, dtype, device, cot_layout)
    mcl, mpl = configure(make(), dtype), make()
    rcl = raw_t.clone().requires_grad_(True) if raw_grad else raw_t
    # the planar reference on the route r2l_isp_step_bwd_raw takes: frames that require grad where they can (float32 frames)
    rpl = raw_t.clone().requires_grad_(True) if raw_t.dtype == torch.float32 else raw_t
    with pc.env_overrides(device, PLANES):
        ycl, gcl, grcl, names = run_cl(mcl, rcl, cot, dtype)
        ypl, gpl, grpl = hc.run32(mpl, rpl, cot32)
    assert isinstance(mcl.stages, ppt._LazyStages)
    want = ypl.to(dtype)
    pc.report(f'channels-last {DTYPE_IDS[DTYPES.index(dtype)]} {label}/out vs planar out (bitwise)',
              (ycl.float() - want.float()).abs().max(), 0.0)
    assert torch.equal(ycl, want), (label, 'forward')
    assert torch.equal(ycl, want.contiguous(memory_format=CL)) and ycl.stride() == want.contiguous(memory_format=CL).stride()
    for a, b in zip(hc.bn_state(mcl), hc.bn_state(mpl)):
        assert torch.equal(a, b), (label, 'BatchNorm buffers')
    for k in gpl:
        pc.report(f'channels-last {DTYPE_IDS[DTYPES.index(dtype)]} {label}/grad {k} vs planar plane route (bitwise)',
                  np.abs(gcl[k] - gpl[k]).max() if k in gcl else np.inf, 0.0)
    hc.same_grads(gcl, gpl, label)
    assert len(gcl) == 7 and sum(v.size for v in gcl.values()) == _lib.R2L_P_NTRAIN
    if raw_grad:
        assert torch.equal(grcl, grpl), (label, 'grad_raw', float((grcl - grpl).abs().max()))
    # the kernels did the layout: no copy / conversion kernel of the library, and torch was given nothing to convert
    assert not any('permute' in k or 'convert' in k for k in names), names
    return names


def check_golden_case(case, dtype, device):
    """a golden case with the channels-last boundary against the float64 oracle.  float32: the limits the planar step is held to
    (parity_checks.check_param_case: the values are identical); 16 bits: half_io_checks.check_golden_case's derived margin of one
    unit in the last place on the output"""
    B, H, W = case['shape']
    raw_np = orc.synth_raw(B, H, W, seed=case['seed'], kind=case['kind'])
    P = pc.build_params(case)
    m = configure(pc.make_module(case, P, device), dtype)
    cot, cot32 = cotangent((B, 3, H, W), 1000 + case['seed'], dtype, device)
    with pc.env_overrides(device, PLANES):
        y, grads, _, _ = run_cl(m, torch.from_numpy(raw_np).to(device), cot, dtype)
    P64 = P.astype(np.float64)
    o_out, _, cache = orc.parametrized_forward(raw_np, P64, track_stages=False, bn=pc.oracle_bn(case))
    cot_np = cot32.cpu().numpy()
    nom, lo, hi = (orc.parametrized_backward(P64, cache, cot_np, **kw)[0] for kw in ({}, dict(clip_shift=1e-6), dict(clip_shift=-1e-6)))
    tol = pc.out_tolerance(cache, case['bn']) + (0.0 if dtype is torch.float32 else hc.ulp16(o_out, dtype))
    err = np.abs(y.float().cpu().numpy().astype(np.float64) - o_out)
    worst = np.unravel_index((err / tol).argmax(), err.shape)
    name = f'channels-last {DTYPE_IDS[DTYPES.index(dtype)]} {case["name"]}'
    pc.report(f'{name}/out vs float64 oracle (forward limit' + ('' if dtype is torch.float32 else ' + 1 ulp16') + ')', err[worst], tol[worst])
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
        pc.report(f'{name}/grad {k} vs float64 oracle', e, lim)
        assert e <= lim, (name, k, float(e), float(lim))


def check_fallback(make, raw_t, dtype, device, label, arm=None, raw_grad=False):
    """a call the channels-last kernels do not serve: the existing path + torch's conversion -- the default output made
    channels-last bit for bit, no channels-last kernel in the launch record, and the gradients of the default module given the
    same cotangent values"""
    mcl, mpl = configure(make(), dtype), make()
    mpl.output_dtype = mcl.output_dtype
    if arm is not None:
        mcl.__dict__['_epilogue'] = arm
        mpl.__dict__['_epilogue'] = arm
    rcl = raw_t.clone().requires_grad_(True) if raw_grad else raw_t
    rpl = raw_t.clone().requires_grad_(True) if raw_grad else raw_t
    lib = _lib.library_for(raw_t)[0]
    ycl, names = pc.kernels_launched(lib, lambda: mcl(rcl))
    assert not any(is_nhwc_kernel(k) for k in names), (label, names)
    ypl = mpl(rpl)
    assert ycl.dtype == dtype and ycl.is_contiguous(memory_format=CL), label
    assert torch.equal(ycl.detach(), ypl.detach().contiguous(memory_format=CL)), label
    assert mcl.buffer['processed_rgb'] is ycl
    cot, cot32 = cotangent(tuple(ycl.shape), 9, dtype, device)
    ycl.backward(cot)
    ypl.backward(cot32.to(dtype))
    gcl = {k: f(mcl).grad.detach().cpu().numpy() for k, f in pc.NAME2ATTR.items() if f(mcl) is not None and f(mcl).grad is not None}
    gpl = {k: f(mpl).grad.detach().cpu().numpy() for k, f in pc.NAME2ATTR.items() if f(mpl) is not None and f(mpl).grad is not None}
    hc.same_grads(gcl, gpl, label)
    assert len(gcl) >= 7
    if raw_grad:
        assert torch.equal(rcl.grad, rpl.grad), label


def check_default_unchanged(device, B=2, H=12, W=264):
    """output_memory_format = None (the default) and torch.contiguous_format: the launch record and the results of a module that
    never heard of the attribute, and a planar-contiguous output"""
    raw_np = orc.synth_raw(B, H, W, seed=4, kind='scene')
    cot = np.random.default_rng(4).standard_normal((B, 3, H, W)).astype(np.float32)
    import selective_bwd_checks as sc
    res = []
    for omf in ('unset', None, torch.contiguous_format):
        m = rc.make_plain_module(True, device, True)
        m.fused_raw_grad = False
        if omf != 'unset':
            m.output_memory_format = omf
        assert ppt.ParametrizedProcessing.output_memory_format is None
        raw = torch.from_numpy(raw_np).to(device)
        lib = _lib.library_for(raw)[0]
        y, fwd = pc.kernels_launched(lib, lambda: m(raw))
        assert y.dtype == torch.float32 and y.is_contiguous()
        _, bwd = pc.kernels_launched(lib, lambda: y.backward(torch.from_numpy(cot).to(device)))
        res.append((y.detach().cpu().numpy(), None, hc.grads_of(m), {**fwd, **bwd}))
    for r in res[1:]:
        sc._same(res[0], r)
        assert sorted(r[3]) == sorted(res[0][3]) and not any('_nhwc' in k for k in r[3]), r[3]
    return res[0]
