"""Channel statistics of the static chains without their output (StaticProcessing.statistics, functional.static_statistics /
channel_sums / mean_std_from_sums, r2l_static_stats / r2l_channel_sums): the checks tests/test_static_stats.py and
tests/test_gpu_static_stats.py share.

sums = float64[7]: per-channel sums of the float32 output values, of their squares, and the pixel count.  Every term is exact in
float64, so the only error is the rounding of the additions: for n terms added in ANY order the result is within
(n - 1) * 2^-53 * sum|t| of the exact sum (each of the n - 1 additions rounds a partial sum that is bounded by sum|t|)."""
import ctypes
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import half_io_checks as hc  # noqa: E402
import parity_checks as pc  # noqa: E402
import static_half_checks as sh  # noqa: E402
from oracle import isp_oracle as orc  # noqa: E402
from raw2logit_amd import _lib  # noqa: E402
from raw2logit_amd import functional as F_  # noqa: E402

CHAINS = sh.CHAINS
NEW_SYMBOLS = ('r2l_static_stats_supported', 'r2l_static_stats_workspace_bytes', 'r2l_static_stats',
               'r2l_channel_sums_workspace_bytes', 'r2l_channel_sums')
FINISH = 'r2l_launch_sums_finish_kernel'
KINDS = ('f32', 'u16', 'f64')


def is_short(chain):
    return chain[1] == 'none' and chain[2] == 'none'


def kernel_name(chain, frames_dtype):
    """launch-record name of the statistics instantiation that serves `chain` on frames of `frames_dtype`"""
    deb, shp, dn = chain
    kind = '_f64' if frames_dtype == torch.float64 else ('' if frames_dtype == torch.float32 else '_u16')
    if is_short(chain):
        return f'r2l_launch_static_stream_{"malvar" if deb == "malvar2004" else "bilinear"}{kind}_stats_kernel'
    return ('r2l_launch_static_chain' + ('_malvar' if deb == 'malvar2004' else '') + ('_unsharp' if shp == 'unsharp_masking' else '') +
            ('_median' if dn == 'median_denoising' else '') + kind + '_stats_kernel')


def scene(B, H, W, seed, device, kind):
    """half_io_checks.frames as float32, 16-bit containers or (the short chains') float64"""
    if kind == 'f64':
        return hc.frames(B, H, W, seed, device).double()
    return hc.frames(B, H, W, seed, device, u16=kind == 'u16')


def constant(B, H, W, device, kind):
    """frames whose every output value is exactly 1.0 under orc.CAMERAS['identity'] on every chain: 8.0, or full containers read as
    12-bit values (65535 / 4095 = 16.0...): far above the clip whatever the stencils' unit-sum weights round to"""
    if kind == 'u16':
        return torch.full((B, H, W), -1, dtype=torch.int16, device=device), dict(bits=12)
    return torch.full((B, H, W), 8.0, dtype=torch.float64 if kind == 'f64' else torch.float32, device=device), {}


def check_every_pixel_once(chain, B, H, W, device, kind, label, **options):
    """check 1: all seven entries equal B*H*W exactly (integers below 2^53: every partial sum is exact in any order)"""
    raw, kw = constant(B, H, W, device, kind)
    sums = F_.static_statistics(raw, orc.CAMERAS['identity'], *chain, **kw, **options).cpu()
    assert sums.dtype == torch.float64 and tuple(sums.shape) == (7,)
    assert sums.tolist() == [float(B * H * W)] * 7, (label, sums.tolist(), B * H * W)


def fsums(out32):
    """math.fsum per channel of a (B,C,H,W) float32 tensor's values, of their exact squares and of the absolute values -> three lists"""
    x = out32.detach().cpu().double()
    C = x.shape[1]
    s1, s2, sa = [], [], []
    for c in range(C):
        v = x[:, c].reshape(-1).tolist()
        s1.append(math.fsum(v))
        s2.append(math.fsum(t * t for t in v))        # (the product of two float32 values is exact in float64)
        sa.append(math.fsum(abs(t) for t in v))
    return s1, s2, sa


def check_sums_against(sums, out32, label):
    """check 2: sums[0:2C] against math.fsum of the float32 values and of their exact squares, within (n - 1) * 2^-53 * sum|t|"""
    sums = sums.cpu().tolist()
    C = out32.shape[1]
    n = out32.shape[0] * out32.shape[2] * out32.shape[3]
    s1, s2, sa = fsums(out32)
    assert sums[2 * C] == float(n), (label, sums[2 * C], n)
    u = (n - 1) * 2.0 ** -53
    rows = [(what, c, abs(got - want), lim) for c in range(C)
            for what, got, want, lim in (('sum', sums[c], s1[c], u * sa[c]), ('sum of squares', sums[C + c], s2[c], u * s2[c]))]
    what, c, err, lim = max(rows, key=lambda r: r[2] / r[3] if r[3] > 0 else float(r[2] > 0))
    pc.report(f'static-stats {label}: worst of the {2 * C} sums ({what}, channel {c}; any-order bound)', err, lim)
    for what, c, err, lim in rows:
        assert err <= lim, (label, c, what, err, lim)


def check_values(chain, raw, label, cam=orc.DRONE_CAMERA_PARAMS, **kw):
    sums = F_.static_statistics(raw, cam, *chain, **kw)
    out32 = F_.static_pipeline(raw, cam, *chain, **kw)
    check_sums_against(sums, out32, label)
    return sums, out32


def check_served(chain, raw, label, **kw):
    """check 4, a served call: exactly one statistics instantiation and the finishing launch, no float32 sibling"""
    assert F_.static_stats_why(raw, *chain) is None, (label, F_.static_stats_why(raw, *chain))
    lib = _lib.library_for(raw)[0]
    sums, names = pc.kernels_launched(lib, lambda: F_.static_statistics(raw, orc.DRONE_CAMERA_PARAMS, *chain, **kw))
    assert names == {kernel_name(chain, raw.dtype): 1, FINISH: 1}, (label, names)
    return sums


def c_call(lib, raw, chain, sums, ws=None, nws=0, stream=None, options=None):
    """r2l_static_stats as C callers see it (float32 / float64 frames) -> return code"""
    bl, wb, ccm = orc.DRONE_CAMERA_PARAMS
    cam = (ctypes.c_double * 16)(*[float(v) for v in list(bl) + list(wb) + list(ccm)])
    B, H, W = raw.shape
    codes = (F_._DEBAYER[chain[0]], F_._SHARPEN.get(chain[1], 0), F_._DENOISE.get(chain[2], 0))
    ov = (ctypes.c_double * 5)(*options) if options is not None else None
    return lib.r2l_static_stats(_lib.ptr(raw), 2 if raw.dtype == torch.float64 else 0, 1.0, _lib.ptr(sums), B, H, W, cam, *codes, 2.2, ov,
                                _lib.ptr(ws), nws, stream)


def check_unserved(chain, raw, label, word, options=None, **kw):
    """check 4, an unserved call: the predicate names the reason, the C call returns -3 with it and leaves `sums` alone, and the
    Python call goes through the float32 kernels and r2l_channel_sums -- and passes check 2"""
    why = F_.static_stats_why(raw, *chain, **kw)
    assert why and word in why, (label, why)
    lib = _lib.library_for(raw)[0]
    sums = torch.full((7,), 7.0, dtype=torch.float64, device=raw.device)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=raw.device)
    assert c_call(lib, raw, chain, sums, ws, ws.numel(), options=options) == -3, label
    assert word.encode() in lib.r2l_last_error(), (label, lib.r2l_last_error())
    assert sums.cpu().tolist() == [7.0] * 7, label
    got, names = pc.kernels_launched(lib, lambda: F_.static_statistics(raw, orc.DRONE_CAMERA_PARAMS, *chain, **kw))
    assert not any(k.endswith('_stats_kernel') and 'static' in k for k in names) and names.get('r2l_launch_channel_sums_kernel') == 1, (label, names)
    check_sums_against(got, F_.static_pipeline(raw, orc.DRONE_CAMERA_PARAMS, *chain, **kw), label)
    return why


def check_repeatable(chain, raw, label, **kw):
    """check 5: two calls give the same 56 bytes"""
    a = F_.static_statistics(raw, orc.DRONE_CAMERA_PARAMS, *chain, **kw).cpu().numpy().tobytes()
    b = F_.static_statistics(raw, orc.DRONE_CAMERA_PARAMS, *chain, **kw).cpu().numpy().tobytes()
    assert len(a) == 56 and a == b, label


def check_golden(case, golden, key, device):
    """check 3: mean / unbiased std of a golden case's reference output against mean_std_from_sums(static_statistics(raw)).  The
    static chains' bar is 1e-5 per pixel: that moves the mean by at most 1e-5 and the population std by at most 1e-5 (the unbiased
    one by sqrt(n / (n - 1)) times that); 2^-23 is the float32 rounding of the returned values, which are below 1"""
    g = golden[key]
    raw_np = g[case['name'] + '/raw']
    if raw_np.shape[-1] % 4 and raw_np.dtype == np.float64:
        return None
    cam = orc.CAMERAS[case['camera']]
    ref = g[case['name'] + '/out_hwc_f64'].transpose(0, 3, 1, 2)
    n = ref.shape[0] * ref.shape[2] * ref.shape[3]
    want_mean, want_std = ref.mean(axis=(0, 2, 3)), ref.std(axis=(0, 2, 3), ddof=1)
    lim_mean, lim_std = 1e-5 + 2.0 ** -23, 1e-5 * math.sqrt(n / (n - 1)) + 2.0 ** -23
    variants = [('', torch.from_numpy(raw_np).to(device), {})]
    if case.get('bits'):
        variants.append(('/u16', torch.from_numpy(g[case['name'] + '/u16'].view(np.int16)).to(device), dict(bits=case['bits'])))
    for sfx, raw, kw in variants:
        sums = F_.static_statistics(raw, cam, case['debayer'], case['sharpening'], case['denoising'], **kw, **case.get('opts', {}))
        mean, std = F_.mean_std_from_sums(sums)
        assert mean.dtype == torch.float32 and std.dtype == torch.float32 and tuple(mean.shape) == (3, 1, 1) == tuple(std.shape)
        e_mean = np.abs(mean.cpu().numpy().reshape(3).astype(np.float64) - want_mean).max()
        e_std = np.abs(std.cpu().numpy().reshape(3).astype(np.float64) - want_std).max()
        pc.report(f'static-stats {key}/{case["name"]}{sfx} mean', e_mean, lim_mean)
        pc.report(f'static-stats {key}/{case["name"]}{sfx} std (unbiased)', e_std, lim_std)
        assert e_mean <= lim_mean and e_std <= lim_std, (case['name'], sfx, e_mean, e_std)
    return True


def check_channel_sums(x, label):
    sums = F_.channel_sums(x)
    assert sums.dtype == torch.float64 and tuple(sums.shape) == (2 * x.shape[1] + 1,) and sums.device == x.device
    check_sums_against(sums, x, label)
    return sums
