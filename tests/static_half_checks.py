"""16-bit output of the static chains (StaticProcessing.output_dtype, functional.static_pipeline(out_dtype=...), r2l_static_fwd_io):
the checks tests/test_static_half_io.py and tests/test_gpu_static_half_io.py share.

The contract: the 16-bit call returns float32_call(raw).to(dtype) BIT FOR BIT -- the kernels compute and round to float32 exactly
as before (Normalize included) and only then round to nearest even, which is what torch's cast does."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import half_io_checks as hc  # noqa: E402
import parity_checks as pc  # noqa: E402
from oracle import isp_oracle as orc  # noqa: E402
from raw2logit_amd import _lib  # noqa: E402
from raw2logit_amd import functional as F_  # noqa: E402
from raw2logit_amd.processing import pipeline_numpy as ppn  # noqa: E402

DTYPES, DTYPE_IDS = hc.DTYPES, hc.DTYPE_IDS
NEW_SYMBOLS = ('r2l_static_io_supported', 'r2l_static_fwd_io')
MEAN, STD = [0.35, 0.36, 0.35], [0.12, 0.11, 0.12]            # train.py:157-158 (Drone)

SHORT_BILINEAR = ('bilinear', 'none', 'none')
SHORT_MALVAR = ('malvar2004', 'none', 'none')
DEFAULT_CHAIN = ('bilinear', 'sharpening_filter', 'gaussian_denoising')
MALVAR_MEDIAN = ('malvar2004', 'sharpening_filter', 'median_denoising')
UNSHARP_GAUSS = ('bilinear', 'unsharp_masking', 'gaussian_denoising')
CHAINS = [SHORT_BILINEAR, SHORT_MALVAR, DEFAULT_CHAIN, MALVAR_MEDIAN, UNSHARP_GAUSS]


def kernel_name(chain, frames_dtype, dtype):
    """launch-record name of the 16-bit instantiation that serves `chain` on frames of `frames_dtype`"""
    deb, sh, dn = chain
    kind = '_f64' if frames_dtype == torch.float64 else ('' if frames_dtype == torch.float32 else '_u16')
    io = '_bf16' if dtype is torch.bfloat16 else '_f16'
    if sh == 'none' and dn == 'none':
        return f'r2l_launch_static_stream_{"malvar" if deb == "malvar2004" else "bilinear"}{kind}{io}_kernel'
    return ('r2l_launch_static_chain' + ('_malvar' if deb == 'malvar2004' else '') + ('_unsharp' if sh == 'unsharp_masking' else '') +
            ('_median' if dn == 'median_denoising' else '') + kind + io + '_kernel')


def module(chain, norm=False, **options):
    return ppn.StaticProcessing(orc.DRONE_CAMERA_PARAMS, *chain, **(dict(mean=MEAN, std=STD) if norm else {}), **options)


def reaches_both_sides_of_the_clip(out32):
    """the frames of half_io_checks.frames under the Drone camera: values inside (0, 1), at 0 (below the clip) and at 1 (above)"""
    return bool(((out32 > 0) & (out32 < 1)).any() and (out32 == 0).any() and (out32 == 1).any())


def check_served(chain, raw, dtype, label, norm=False, **options):
    """a call the 16-bit kernels serve: out16 == out32.to(dtype) bit for bit; the launch record holds the 16-bit instantiation, once,
    and nothing else (no float32 kernel, no cast kernel -- torch's cast is no kernel of this library, so the record must not hold
    the float32 sibling whose output it would narrow)"""
    m16, m32 = module(chain, norm, **options).to(raw.device), module(chain, norm, **options).to(raw.device)
    m16.output_dtype = dtype
    assert F_.static_io_why(raw, *chain, **options) is None, (label, F_.static_io_why(raw, *chain, **options))
    lib = _lib.library_for(raw)[0]
    y16, names = pc.kernels_launched(lib, lambda: m16(raw))
    y32 = m32(raw)
    assert y16.dtype == dtype and y16.is_contiguous() and m16.buffer['processed_rgb'] is y16 and y32.dtype == torch.float32
    assert names == {kernel_name(chain, raw.dtype, dtype): 1}, (label, names)
    assert torch.equal(y16, y32.to(dtype)), (label, float((y16.float() - y32).abs().max()))
    return y32


def check_fallback(chain, raw, dtype, label, word, **options):
    """a call the 16-bit kernels do not serve: the predicate says why, the C call returns -3 with that reason, and the module runs
    the float32 kernels and casts -- the same bits"""
    why = F_.static_io_why(raw, *chain, **options)
    assert why and word in why, (label, why)
    m16, m32 = module(chain, **options).to(raw.device), module(chain, **options).to(raw.device)
    m16.output_dtype = dtype
    lib = _lib.library_for(raw)[0]
    y16, names = pc.kernels_launched(lib, lambda: m16(raw))
    assert not any(k.endswith('_bf16_kernel') or k.endswith('_f16_kernel') for k in names), (label, names)
    y32 = m32(raw)
    assert y16.dtype == dtype and m16.buffer['processed_rgb'] is y16
    assert torch.equal(y16, y32.to(dtype)), label
    return why


def c_call_io(lib, raw, chain, io, out, stream=None, options=None):
    """r2l_static_fwd_io as C callers see it (float32 / float64 frames, no Normalize) -> return code"""
    import ctypes
    bl, wb, ccm = orc.DRONE_CAMERA_PARAMS
    cam = (ctypes.c_double * 16)(*[float(v) for v in list(bl) + list(wb) + list(ccm)])
    B, H, W = raw.shape
    codes = (F_._DEBAYER[chain[0]], F_._SHARPEN.get(chain[1], 0), F_._DENOISE.get(chain[2], 0))
    ov = (ctypes.c_double * 5)(*options) if options is not None else None
    return lib.r2l_static_fwd_io(_lib.ptr(raw), 2 if raw.dtype == torch.float64 else 0, 1.0, _lib.ptr(out), io, B, H, W, cam, *codes,
                                 2.2, ov, None, None, 0, stream)


def check_golden(case, golden, key, dtype, device):
    """a static golden case through out_dtype: within the case's float32 limit (1e-5, parity_checks.check_static_case /
    check_static_options) plus one unit in the last place of the 16-bit type at the expected value -- the store rounds by half a
    unit, and the float32 value may sit on the other side of a rounding boundary from the reference's: one unit in all"""
    g = golden[key]
    raw_np = g[case['name'] + '/raw']
    if raw_np.shape[-1] % 4 and raw_np.dtype == np.float64:
        return None
    cam = orc.CAMERAS[case['camera']]
    ref = g[case['name'] + '/out_hwc_f64'].transpose(0, 3, 1, 2)
    tol = 1e-5 + hc.ulp16(ref, dtype)
    tag = DTYPE_IDS[DTYPES.index(dtype)]
    variants = [('', torch.from_numpy(raw_np).to(device), {})]
    if case.get('bits'):
        variants.append(('/u16', torch.from_numpy(g[case['name'] + '/u16'].view(np.int16)).to(device), dict(bits=case['bits'])))
    for sfx, raw, kw in variants:
        out = F_.static_pipeline(raw, cam, case['debayer'], case['sharpening'], case['denoising'], out_dtype=dtype, **kw,
                                 **case.get('opts', {}))
        assert out.dtype == dtype
        err = np.abs(out.float().cpu().numpy().astype(np.float64) - ref)
        worst = np.unravel_index((err / tol).argmax(), err.shape)
        pc.report(f'static-half {tag} {key}/{case["name"]}{sfx} (float32 limit + 1 ulp16)', err[worst], tol[worst])
        assert np.all(err <= tol), (case['name'], sfx, float(err[worst]), float(tol[worst]))
    return True
