"""The weak augmentation in the static chains' stores (StaticProcessing.supports_output_epilogue,
functional.static_pipeline(epilogue=...), r2l_static_fwd_epilogue): the checks tests/test_static_epilogue.py and
tests/test_gpu_static_epilogue.py share.

The contract: the call with an epilogue (hflip, vflip, k) returns augmentation.flip_rot(plain_call(raw), hflip, vflip, k) BIT FOR BIT,
narrowed afterwards where a 16-bit output type is set -- a permutation moves values and rounds nothing, so there is no tolerance
anywhere in this file."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import torch  # noqa: E402

import parity_checks as pc  # noqa: E402
import static_half_checks as sh  # noqa: E402
from oracle import isp_oracle as orc  # noqa: E402
from raw2logit_amd import _lib  # noqa: E402
from raw2logit_amd import augmentation as aug  # noqa: E402
from raw2logit_amd import functional as F_  # noqa: E402

NEW_SYMBOLS = ('r2l_static_epilogue_supported', 'r2l_static_fwd_epilogue')
# (hflip, vflip, k): the seven moves with k even that are not the identity -- what one row-streaming kernel stores itself
EVEN_EPILOGUES = [(True, False, 0), (False, True, 0), (True, True, 0), (False, False, 2), (True, False, 2), (False, True, 2),
                  (True, True, 2)]
OUT_DTYPES = [None, torch.bfloat16, torch.float16]
OUT_IDS = ['f32', 'bf16', 'f16']


def net_flips(epilogue):
    """(hflip, vflip) of the plane flip an even-k epilogue amounts to: rot90^2 is both flips"""
    hflip, vflip, k = epilogue
    assert k % 2 == 0
    return (bool(hflip) != (k == 2), bool(vflip) != (k == 2))


def torch_moved(plain, epilogue):
    """rot90^k(vflip(hflip(plain))) by torch's own flip / rot90 (k as in x.rot90(k, dims=(-1, -2))): a reference that shares no code
    with the library's permutation kernel"""
    hflip, vflip, k = epilogue
    y = plain
    if hflip:
        y = y.flip(-1)
    if vflip:
        y = y.flip(-2)
    return y.rot90(k, dims=(-1, -2)).contiguous() if k else y.contiguous()


def kernel_name(chain, frames_dtype, dtype):
    """launch-record name of the epilogue instantiation that serves `chain` on frames of `frames_dtype` with output type `dtype`"""
    deb, shp, dn = chain
    kind = '' if frames_dtype == torch.float32 else '_u16'
    io = {None: '', torch.float32: '', torch.bfloat16: '_bf16', torch.float16: '_f16'}[dtype]
    if shp == 'none' and dn == 'none':
        return f'r2l_launch_static_stream_{"malvar" if deb == "malvar2004" else "bilinear"}{kind}{io}_epi_kernel'
    return ('r2l_launch_static_chain' + ('_malvar' if deb == 'malvar2004' else '') + ('_unsharp' if shp == 'unsharp_masking' else '') +
            ('_median' if dn == 'median_denoising' else '') + kind + io + '_epi_kernel')


def armed_call(m, raw, epilogue):
    """the module's next call with the one-shot epilogue ComposeState.arm leaves in its __dict__"""
    m.__dict__['_epilogue'] = tuple(epilogue)
    y = m(raw)
    assert '_epilogue' not in m.__dict__
    return y


def check_served(chain, raw, epilogue, dtype, label, norm=False, against_torch=False, **options):
    """a call one epilogue kernel serves: one launch, of that kernel, no permutation kernel; the bits of flip_rot(plain call)"""
    why = F_.static_epilogue_why(raw, *chain, epilogue=epilogue, out_dtype=dtype, **options)
    assert why is None, (label, why)
    m, plain_m = sh.module(chain, norm, **options).to(raw.device), sh.module(chain, norm, **options).to(raw.device)
    m.output_dtype = dtype
    lib = _lib.library_for(raw)[0]
    y, names = pc.kernels_launched(lib, lambda: armed_call(m, raw, epilogue))
    assert names == {kernel_name(chain, raw.dtype, dtype): 1}, (label, names)
    plain = plain_m(raw)
    assert plain.dtype == torch.float32
    want = aug.flip_rot(plain, *epilogue)
    want = want if dtype in (None, torch.float32) else want.to(dtype)
    assert y.dtype == want.dtype and y.is_contiguous() and m.buffer['processed_rgb'] is y
    assert torch.equal(y, want), (label, int((y != want).sum()))
    if against_torch:
        t = torch_moved(plain, epilogue)
        assert torch.equal(y, t if dtype in (None, torch.float32) else t.to(dtype)), label
    return plain


def check_fallback(chain, raw, epilogue, dtype, label, word, **options):
    """a call no epilogue kernel serves: the predicate says why, and the module runs the plain kernel(s) and then the permutation
    kernel -- the same bits"""
    why = F_.static_epilogue_why(raw, *chain, epilogue=epilogue, out_dtype=dtype, **options)
    assert why and word in why, (label, why)
    m, plain_m = sh.module(chain, **options).to(raw.device), sh.module(chain, **options).to(raw.device)
    m.output_dtype = dtype
    lib = _lib.library_for(raw)[0]
    plain, plain_names = pc.kernels_launched(lib, lambda: plain_m(raw))
    y, names = pc.kernels_launched(lib, lambda: armed_call(m, raw, epilogue))
    moved = {k: v for k, v in names.items() if k.startswith('r2l_launch_aug')}
    assert sum(moved.values()) == 1 and not any(k.endswith('_epi_kernel') for k in names), (label, names)
    assert {k: v for k, v in names.items() if k not in moved} == plain_names, (label, names, plain_names)
    want = torch_moved(plain, epilogue)
    want = want if dtype in (None, torch.float32) else want.to(dtype)
    assert y.dtype == want.dtype and m.buffer['processed_rgb'] is y
    assert torch.equal(y, want), label
    return why


def c_call(lib, raw, chain, io, out, epilogue_bits, stream=None, plain=False):
    """r2l_static_fwd_epilogue (plain: r2l_static_fwd_io) as C callers see it (float32 / float64 frames, no Normalize) -> return code"""
    import ctypes
    bl, wb, ccm = orc.DRONE_CAMERA_PARAMS
    cam = (ctypes.c_double * 16)(*[float(v) for v in list(bl) + list(wb) + list(ccm)])
    B, H, W = raw.shape
    codes = (F_._DEBAYER[chain[0]], F_._SHARPEN.get(chain[1], 0), F_._DENOISE.get(chain[2], 0))
    args = (_lib.ptr(raw), 2 if raw.dtype == torch.float64 else 0, 1.0, _lib.ptr(out), io, B, H, W, cam, *codes, 2.2, None, None, None, 0, stream)
    return lib.r2l_static_fwd_io(*args) if plain else lib.r2l_static_fwd_epilogue(*args, epilogue_bits)
