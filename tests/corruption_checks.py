"""Checks of the common-corruption kernels (raw2logit_amd/corruptions.py, r2l_corruptions.h) shared by the CPU tests (the
kernel source run by the host emulation) and the GPU tests: parity with the reference's goldens and with the float64 oracle
(tests/corruption_oracle.py), the deterministic properties of the random transforms, and their distributions.

Limits.  Deterministic transforms: the project's static-chain bar, 1e-5 absolute (parity_checks.check_static_case); the
reference evaluated in float32 differs from itself in float64 by <= 4.4e-7 on these frames (tests/tools/make_corruption_golden.py
prints it), so the bar leaves room without hiding a wrong tap or coordinate.  With mean / std: 1e-5 / min(std).  Distribution
checks: 5 sigma of the statistic under the distribution asked for, and the Dvoretzky-Kiefer-Wolfowitz bound at failure
probability 1e-9 -- conditions, not measurements; every check uses one fixed key."""
import functools
import os

import numpy as np
import torch

import corruption_oracle as co
import parity_checks as pc
from raw2logit_amd import _lib
from raw2logit_amd import augmentation as A
from raw2logit_amd import corruptions as C

ATOL = 1e-5
MEAN, STD = [0.35, 0.36, 0.35], [0.12, 0.11, 0.12]           # train.py:157-158 (Drone)
DETERMINISTIC = ('contrast', 'brightness', 'saturate', 'gaussian_blur', 'zoom_blur')
KEY = 0x1234567890ABCDEF >> 2


@functools.lru_cache(maxsize=None)
def golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'corruptions.npz'), allow_pickle=False)


def golden_cases():
    """[(transform, severity, H, x, the reference's float32 result, its float64 evaluation as float32)]"""
    g = golden()
    for name in g.files:
        if name.startswith('ref64_'):
            t, s, H = name[6:].rsplit('_', 2)
            r64 = g[name]
            r32 = (r64.view(np.int32) + g['ulp_' + name[6:]].astype(np.int32)).view(np.float32)
            yield t, int(s[1:]), int(H), g[f'x_{H}'], r32, r64


@functools.lru_cache(maxsize=None)
def frames(shape):
    """uniform in [0, 1] with exact 0, exact 1, black, white and grey pixels and channel ties in every image"""
    x = np.random.default_rng(sum(shape)).random(shape).astype(np.float32)
    H, W = shape[-2:]
    x[:, 0, 0, 0] = 0.0
    x[:, 1, 0, 1] = 1.0
    x[:, :, 1, 2] = 0.0
    x[:, :, 2, 1] = 1.0
    x[:, :, 3, 3] = x[:, :1, 3, 3]
    x[:, :, H - 1, W - 1] = x[:, 1:2, H - 1, W - 1]
    x[:, 2, H - 1, 0] = x[:, 1, H - 1, 0]
    x[:, 0, 0, W - 1] = x[:, 2, 0, W - 1]
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def oracle(shape, transform, severity):
    o = co.apply(frames(shape), transform, severity)
    o.setflags(write=False)
    return o


def check_goldens(device):
    for t, sev, H, x, r32, r64 in golden_cases():
        y = C.corrupt(torch.from_numpy(x).to(device), t, sev).cpu().numpy()
        assert y.shape == x.shape and y.dtype == np.float32
        err = np.abs(y.astype(np.float64) - r32).max()
        pc.report(f'corrupt {t} s{sev} {H}x{H} vs the reference [{device}]', err, ATOL)
        assert err <= ATOL, (t, sev, H, err)


def check_oracle_parity(device, transform, shapes, severities=(1, 3, 5)):
    """kernel vs float64 oracle, plain and with the fused Normalize; the batch bit-equal to its images one by one"""
    for shape in shapes:
        if transform == 'zoom_blur' and shape[-1] != shape[-2]:
            continue
        x = torch.tensor(frames(shape)).to(device)
        for sev in severities:
            o = oracle(shape, transform, sev)
            y = C.corrupt(x, transform, sev)
            err = np.abs(y.cpu().numpy().astype(np.float64) - o).max()
            pc.report(f'corrupt {transform} s{sev} {shape} [{device}]', err, ATOL)
            assert err <= ATOL, (transform, sev, shape, err)
            yn = C.corrupt(x, transform, sev, mean=MEAN, std=STD)
            errn = np.abs(yn.cpu().numpy().astype(np.float64) - co.normalize(o, MEAN, STD)).max()
            pc.report(f'corrupt {transform} s{sev} {shape} + Normalize [{device}]', errn, ATOL / min(STD))
            assert errn <= ATOL / min(STD), (transform, sev, shape, errn)
            # the epilogue is torchvision's arithmetic on the plain result: float32 subtract, then divide
            m, s = torch.tensor(MEAN, device=device).view(1, 3, 1, 1), torch.tensor(STD, device=device).view(1, 3, 1, 1)
            assert torch.equal(yn, (y - m) / s), (transform, sev, shape)
            if shape[0] > 1:
                one = torch.cat([C.corrupt(x[i:i + 1], transform, sev) for i in range(shape[0])])
                assert torch.equal(one, y), (transform, sev, shape, 'an image depends on its batch')
                assert torch.equal(C.corrupt(x[1], transform, sev), y[1])          # (3,H,W) in, (3,H,W) out


def check_identity(device):
    x = torch.from_numpy(frames((2, 3, 18, 18)) * 1.5 - 0.25).to(device)
    assert C.corrupt(x, 'identity', 3) is x and C.Distortions()(x) is x
    yn = C.corrupt(x, 'identity', 1, mean=MEAN, std=STD)                           # no clip: Normalize alone
    m, s = torch.tensor(MEAN, device=device).view(1, 3, 1, 1), torch.tensor(STD, device=device).view(1, 3, 1, 1)
    assert torch.equal(yn, (x - m) / s)


def check_noise_identities(device, shape):
    """gaussian_noise / speckle_noise are the library's Philox deviates at the flat element index"""
    x = torch.from_numpy(frames(shape) * 1.2 - 0.1).to(device)                     # both clip bounds are crossed
    for sev in (1, 5):
        c = C.SEVERITY['gaussian_noise'][sev - 1]
        y = C.corrupt(x, 'gaussian_noise', sev, key=KEY)
        assert torch.equal(y, A.add_gaussian_noise(x, c, KEY).clamp(0, 1)), (shape, sev)
        c = C.SEVERITY['speckle_noise'][sev - 1]
        n = A.add_gaussian_noise(torch.zeros_like(x), 1.0, KEY).double()
        ref = (x.double() + x.double() * c * n).clamp(0, 1)
        err = (C.corrupt(x, 'speckle_noise', sev, key=KEY).double() - ref).abs().max().item()
        pc.report(f'corrupt speckle_noise s{sev} {shape} vs x + x c n [{device}]', err, 1e-6)
        assert err <= 1e-6, (shape, sev, err)
    for t in C.RANDOM:
        a, b = C.corrupt(x, t, 3, key=KEY), C.corrupt(x, t, 3, key=KEY)
        assert torch.equal(a, b), t                                                # same key, same bits
        other = C.corrupt(x, t, 3, key=KEY + 1)
        assert (other != a).float().mean().item() > (0.01 if t == 'impulse_noise' else 0.5), t
        d = C.Distortions(3, t)
        torch.manual_seed(5)
        y1, k1 = d(x), d.last_key
        torch.manual_seed(5)
        y2 = d(x)
        assert d.last_key == k1 and torch.equal(y1, y2) and torch.equal(y1, C.corrupt(x, t, 3, key=k1)), t
        assert y1.dtype == torch.float32 and y1.shape == x.shape
        assert d(x).ne(y1).any() and d.last_key != k1                              # the next call draws a new key


def check_launch_shape_independence(device, shape):
    """every transform (contrast's means included) bit-identical under two launch-shape overrides"""
    x = torch.tensor(frames(shape)).to(device)
    for t in C.KINDS:
        if t == 'identity' or (t == 'zoom_blur' and shape[-1] != shape[-2]):
            continue
        for kw in ({}, {'mean': MEAN, 'std': STD}):
            y0 = C.corrupt(x, t, 5, key=KEY, **kw)
            for grid in ('1', '37'):
                with pc.env_overrides(device, {'R2L_GRID_CORRUPT': grid}):
                    y1 = C.corrupt(x, t, 5, key=KEY, **kw)
                assert torch.equal(y0, y1), (t, grid, kw)


def element_draws(key, n, block=0):
    """the Philox block `block` of the elements 0 .. n - 1 as impulse_noise / shot_noise draw it: counter = (e low, e high |
    block << 8, offset 0), restated on the host with the oracle's Philox4x32-10 -> (n, 4) uint32"""
    from oracle import isp_oracle as orc
    e = np.arange(n, dtype=np.uint64)
    ctr = np.stack([e & np.uint64(0xFFFFFFFF), (e >> np.uint64(32)) | np.uint64(block << 8), np.zeros_like(e), np.zeros_like(e)], 1)
    return orc.philox4x32_10(ctr, (key & 0xFFFFFFFF, key >> 32))


def check_impulse_distribution(device):
    shape = (2, 3, 64, 64)
    rng = np.random.default_rng(11)
    inside = torch.from_numpy((0.25 + 0.5 * rng.random(shape)).astype(np.float32)).to(device)    # a flip is visible
    n = inside.numel()
    for sev in (1, 3, 5):
        c = C.SEVERITY['impulse_noise'][sev - 1]
        y = C.corrupt(inside, 'impulse_noise', sev, key=KEY)
        flipped = y != inside
        assert bool(((y[flipped] == 0) | (y[flipped] == 1)).all())
        nf = int(flipped.sum())
        assert abs(nf - n * c) <= 5 * np.sqrt(n * c * (1 - c)), (sev, nf, n * c)
        salt = int((y[flipped] == 1).sum())
        assert abs(salt - 0.5 * nf) <= 5 * np.sqrt(0.25 * nf), (sev, salt, nf)
        # The flip and the salt choice come from different Philox outputs.  (The salt share above would catch a salt bit that is
        # the flip word's top bit -- every flipped element has a small word -- but not one of its low bits.)  So restate the
        # element's block on the host: flipped <=> output 0 < c 2^32, salt <=> the top bit of output 1
        o = element_draws(KEY, n)
        f = flipped.cpu().numpy().reshape(-1)
        assert np.array_equal(f, o[:, 0] < np.uint32(int(c * 4294967296.0 + 0.5))), sev
        assert np.array_equal(y.cpu().numpy().reshape(-1)[f] == 1, (o[f, 1] >> np.uint32(31)) == 1), sev
        assert not np.array_equal((o[f, 0] & np.uint32(1)) == 1, (o[f, 1] >> np.uint32(31)) == 1)
        # every channel of a pixel flips on its own
        per_pixel = flipped.sum(1)
        assert abs(int((per_pixel == 3).sum()) - n / 3 * c ** 3) <= 5 * np.sqrt(n / 3 * c ** 3) + 1, sev
    wide = torch.from_numpy((rng.random(shape) * 1.4 - 0.2).astype(np.float32)).to(device)
    y = C.corrupt(wide, 'impulse_noise', 5, key=KEY)
    same_mask = C.corrupt(inside, 'impulse_noise', 5, key=KEY) != inside           # the draws do not depend on the values
    assert torch.equal(y[~same_mask], wide.clamp(0, 1)[~same_mask])                # untouched elements: clip(x), exactly
    assert bool(((y[same_mask] == 0) | (y[same_mask] == 1)).all())


def check_shot_distribution(device):
    """Poisson statistics on constant planes at c = 500 (severity 1): the sampler's two regimes (inversion below 10, PTRS above).
    lambda = 450 stands for 500, where the clip at 1 would cut the upper half: P(k > 500 | 450) = 0.9 %, which moves the
    mean by 0.07 (limit 0.96) and the empirical CDF by 0.009 (limit 0.030)"""
    from scipy.stats import poisson
    c, n = 500.0, 3 * 64 * 64
    for lam in (0.0, 0.5, 4.0, 30.0, 100.0, 450.0):
        x = torch.full((1, 3, 64, 64), lam / c, dtype=torch.float32, device=device)
        lam = float(x[0, 0, 0, 0].double() * c)                                    # what the kernel is given
        k = C.corrupt(x, 'shot_noise', 1, key=KEY).double().cpu().numpy().reshape(-1) * c
        assert np.abs(k - np.rint(k)).max() <= 1e-3 and k.min() >= 0, lam
        k = np.rint(k)
        if lam == 0:
            assert not k.any()
            continue
        mean, var = k.mean(), k.var(ddof=1)
        assert abs(mean - lam) <= 5 * np.sqrt(lam / n), (lam, mean)
        assert abs(var - lam) <= 5 * np.sqrt((lam + 2 * lam * lam) / n), (lam, var)
        ks = np.arange(0, int(k.max()) + 2)
        ecdf = np.searchsorted(np.sort(k), ks, side='right') / n
        dkw = np.sqrt(np.log(2e9) / (2 * n))
        sup = np.abs(ecdf - poisson.cdf(ks, lam)).max()
        print(f'[shot_noise {device}] lambda {lam:g}: mean {mean:.4f} var {var:.4f} sup|F^ - F| {sup:.4f} (limit {dkw:.4f})')
        assert sup <= dkw, (lam, sup, dkw)
    # negative inputs are lambda = 0
    assert not C.corrupt(torch.full((1, 3, 8, 8), -0.3, device=device), 'shot_noise', 1, key=KEY).any()
    # per-element counters: lambda differs row by row (both regimes, so the number of draws an element consumes varies); rows of
    # equal lambda are not shifted copies of one another, and changing one row's lambda leaves every other row's bits alone
    rows = torch.tensor([2.0, 30.0] * 16, device=device).view(1, 1, 32, 1).expand(1, 3, 32, 48).contiguous() / c
    y = C.corrupt(rows, 'shot_noise', 1, key=KEY)
    for a in range(0, 4):
        for b in range(a + 2, 32, 2):
            for shift in range(-6, 7):
                assert not torch.equal(y[0, 0, a], torch.roll(y[0, 0, b], shift)), (a, b, shift)
    rows2 = rows.clone()
    rows2[0, :, 5] = 400.0 / c
    y2 = C.corrupt(rows2, 'shot_noise', 1, key=KEY)
    keep = torch.ones(32, dtype=torch.bool)
    keep[5] = False
    assert torch.equal(y2[0, :, keep], y[0, :, keep]) and not torch.equal(y2[0, :, 5], y[0, :, 5])


def check_poisson_sampler_at_the_ends_of_its_uniforms(lib):
    """The sampler on the smallest and the largest Philox outputs (host emulation: r2l_test_corrupt_poisson).  No fixed key
    reaches them in a test-sized batch, a 64 x 3 x 512^2 batch does several times per call.  A uniform is strictly inside (0, 1):
    the largest one asks for the k whose upper tail is 2^-24, never for a bound of the loop; a PTRS candidate at either end is a finite k >= 0 or a rejection"""
    import ctypes
    from scipy.stats import poisson
    f = lib.cdll.r2l_test_corrupt_poisson
    f.restype, f.argtypes = ctypes.c_float, [ctypes.c_float, ctypes.c_uint, ctypes.c_uint]
    top, tiny = 0xFFFFFFFF, 0
    for lam in (1e-3, 0.1, 0.5, 1.0, 2.0, 4.0, 7.0, 9.99):
        assert f(lam, tiny, 0) == poisson.ppf(2.0 ** -24, lam) == 0.0, lam
        hi = f(lam, top, 0)
        assert hi == poisson.ppf(1 - 2.0 ** -24, lam), (lam, hi)                        # the k whose upper tail is 2^-24
        assert f(lam, 0xFFFFFE00, 0) == hi and f(lam, 0x1FF, 0) == 0.0                  # 9 low bits are not used
        mid = [f(lam, o, 0) for o in (0x40000000, 0x80000000, 0xC0000000)]               # u = 1/4, 1/2, 3/4 (+ 2^-24)
        assert mid == [poisson.ppf(q + 2.0 ** -24, lam) for q in (0.25, 0.5, 0.75)], (lam, mid)
    for lam in (10.0, 30.0, 100.0, 450.0, 5000.0):
        for ou in (tiny, top):                                                         # U = -+(1/2 - 2^-24): us = 2^-24
            for ov in (tiny, top, 0x80000000):
                k = f(lam, ou, ov)
                assert k == -1.0 or (np.isfinite(k) and k >= 0 and k == np.floor(k)), (lam, ou, ov, k)
                # so far out in the hat's tail only a negligible share may be accepted (a candidate beyond 1e-9 of either tail)
                assert k == -1.0 or poisson.ppf(1e-9, lam) <= k <= poisson.isf(1e-9, lam), (lam, ou, ov, k)
        assert f(lam, 0x80000000, 0) == np.floor(lam + 0.43)                            # U = 2^-24, inside the squeeze


def check_dtypes(device):
    """Distortions takes any dtype like the reference and returns float32; the functional form wants float32"""
    import pytest
    x = torch.tensor(frames((1, 3, 18, 18))[0]).to(device)
    d = C.Distortions(3, 'contrast')
    y = d(x)
    assert d(x.double()).dtype == torch.float32 and torch.equal(d(x.double()), y) and torch.equal(d(x.half().float()), d(x.half()))
    u8 = (x * 255).to(torch.uint8)
    assert torch.equal(d(u8), d(u8.float())) and d(u8).dtype == torch.float32
    with pytest.raises(TypeError):
        C.corrupt(x.double(), 'contrast', 3)


def check_errors(device):
    import pytest
    x = torch.tensor(frames((1, 3, 18, 18))).to(device)
    for t in C.NOT_BUILT:
        with pytest.raises(_lib.R2LError, match=t):
            C.Distortions(1, t)
        with pytest.raises(_lib.R2LError, match=t):
            C.corrupt(x, t, 1)
    assert set(C.NOT_BUILT) == {'elastic_transform', 'glass_blur', 'defocus_blur', 'motion_blur', 'fog', 'frost', 'snow',
                                'spatter', 'jpeg_compression', 'pixelate'}
    with pytest.raises(_lib.R2LError, match='unknown transform'):
        C.corrupt(x, 'vignette', 1)
    for sev in (0, 6, 2.5, None):
        with pytest.raises(_lib.R2LError, match='severity'):
            C.corrupt(x, 'contrast', sev)
        with pytest.raises(_lib.R2LError, match='severity'):
            C.Distortions(sev, 'contrast')
    with pytest.raises(_lib.R2LError, match='square'):
        C.corrupt(torch.zeros(1, 3, 16, 24, device=device), 'zoom_blur', 1)
    with pytest.raises(_lib.R2LError, match='3 channels'):
        C.corrupt(torch.zeros(1, 4, 16, 16, device=device), 'contrast', 1)
    with pytest.raises(_lib.R2LError, match='go together'):
        C.corrupt(x, 'contrast', 1, mean=MEAN)
    with pytest.raises(_lib.R2LError, match='std'):
        C.corrupt(x, 'contrast', 1, mean=MEAN, std=[0.1, 0.0, 0.1])
    with pytest.raises(TypeError):
        C.corrupt(x.double(), 'contrast', 1)
    # the C ABI's own codes and texts
    lib, stream = _lib.library_for(x)
    y = torch.empty_like(x)
    import ctypes
    one = (ctypes.c_double * 1)(0.5)
    p = _lib.ptr

    def call(xx, yy, C_, H, W, kind, params, nparams, ws=None, nbytes=0):
        return lib.r2l_corrupt(p(xx), p(yy), 1, C_, H, W, kind, params, nparams, 1, 0, None, None, p(ws), nbytes, stream)
    assert call(x, y, 3, 18, 18, 99, one, 1) == -5 and b'unknown kind' in lib.r2l_last_error()
    assert call(x, y, 4, 18, 18, C.KINDS['contrast'], one, 1) == -6 and b'3 channels' in lib.r2l_last_error()
    zt = C.zoom_table(1, 18)
    assert call(x, y, 3, 18, 12, C.KINDS['zoom_blur'], (ctypes.c_double * len(zt))(*zt), len(zt)) == -7
    assert b'zoom_blur' in lib.r2l_last_error() and b'square' in lib.r2l_last_error()
    assert call(x, y, 3, 18, 18, C.KINDS['contrast'], one, 1) == -2 and b'workspace' in lib.r2l_last_error()
    need = lib.r2l_corrupt_workspace_bytes(C.KINDS['contrast'], 1, 3, 18, 18)
    assert need >= 12 and lib.r2l_corrupt_workspace_bytes(C.KINDS['brightness'], 1, 3, 18, 18) == 0
    ws = torch.empty(need, dtype=torch.uint8, device=device)
    assert call(x, y, 3, 18, 18, C.KINDS['contrast'], one, 1, ws, need - 1) == -2
    assert call(x, y, 3, 18, 18, C.KINDS['contrast'], one, 1, ws, need) == 0
    assert call(x, x, 3, 18, 18, C.KINDS['brightness'], one, 1) == -1                # in place
    assert call(x, y, 3, 18, 18, C.KINDS['saturate'], one, 1) == -4                  # takes two numbers
    bad = list(zt)
    bad[0] = 19.0                                                                     # a crop larger than the frame
    assert call(x, y, 3, 18, 18, C.KINDS['zoom_blur'], (ctypes.c_double * len(bad))(*bad), len(bad)) == -4
    taps = (ctypes.c_double * 6)(*([1 / 11] * 6))
    assert call(x, y, 3, 18, 18, C.KINDS['gaussian_blur'], taps, 6) == -4            # radius 5
