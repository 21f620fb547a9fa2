"""Checks of the SSIM / L2 loss kernels (raw2logit_amd/csrc/r2l_aux_kernels.h) on the paths training takes: the persistent tile
walk with its one-tile-ahead prefetch (more tiles than workgroups), the grid-stride loop of the L2 kernel, tile and halo
edges, and the inputs on which the SSIM formula is ill conditioned in float32.  Shared by tests/test_aux_losses.py (host
emulation) and tests/test_gpu_aux_losses.py (gfx950 library).

Where every limit comes from:
  * the reference is orc.ssim(x, y) in float64;
  * orc.ssim(x, y, dtype=np.float32) is the reference's own arithmetic in float32: its distance from the float64 result is the
    float32 conditioning of that input.  A kernel's gradient may be at most 2 x as far from float64 in RMS and 6 x as far in
    the maximum (the criterion of parity_checks.check_float32_distance), each with a floor of PLANE_GRAD_RTOL x max|grad64|
    (the project's bar for a correct float32 kernel; needed where the float32 oracle happens to be exact);
  * the mean SSIM: 6 x the float32 oracle's distance or 5e-6 (the limit check_aux_losses has always used), whichever is larger;
  * L2: the gradient is reproduced bit for bit in numpy float32, the sum is bounded by a rounding count (l2_sum_bound).
No limit is taken from what the kernels produce."""
import numpy as np
import torch

from oracle import isp_oracle as orc
from oracle.golden_cases import aux_inputs
import parity_checks as pc
from raw2logit_amd import _lib
from raw2logit_amd._lib import ptr

f64 = np.float64
TILE = 64                    # R2L_SSIM_T
SSIM_GRID_CAP = 512          # workgroups of the shipped SSIM launches
L2_LANES = 512               # R2L_NT
L2_FWD_CAP, L2_BWD_CAP = 2048, 4096
MEAN_FLOOR = 5e-6            # check_aux_losses' limit on the mean SSIM
L2_SUM_RTOL = 2e-6           # check_aux_losses' limit on the L2 sum
GUP = 2.0                    # upstream gradient of the direct ABI calls (a power of two: it scales every bit pattern exactly)

WALK_SHAPE = (2, 3, 70, 134)                   # 36 tiles
WALK_GRIDS = (1, 3, 8, 35)
PRODUCT_WALK_SHAPES = ((58, 3, 70, 70), (350, 3, 8, 12))    # 696 and 1050 tiles: more than the 512 workgroups
PRODUCT_WALK_TILES = {(58, 3, 70, 70): 696, (350, 3, 8, 12): 1050}
EDGE_HW = ((1, 1), (1, 64), (5, 6), (11, 11), (59, 64), (64, 64), (64, 65), (65, 69), (70, 70), (63, 128), (64, 129),
           (75, 133))
EDGE_CASES = [(C, H, W) for C in (1, 3) for (H, W) in EDGE_HW]
KIND_SHAPE = (1, 3, 70, 134)
KINDS = ('noise', 'identical', 'zeros', 'piecewise', 'hot_pixel', 'batchnorm')
L2_HOOK_N = 4 * 512 * 7 + 4
L2_HOOK_GRIDS = (None, 1, 3)
L2_PRODUCT_NS = (4, 4 * 512 * 4096 + 4 * 512 * 3 + 4)


def ntiles(shape):
    B, C, H, W = shape
    return B * C * ((H + TILE - 1) // TILE) * ((W + TILE - 1) // TILE)


# ---- inputs ---------------------------------------------------------------------------------------------------
def make_inputs(kind, shape, seed=1):
    """(img1, img2), float32.  'noise' is aux_inputs' recipe (uniform + clipped Gaussian noise); the others are the places where
    E11 - mu1^2 cancels (flat fields: B2 collapses to C2 = 9e-4), where S sits on its maximum (identical images), and the
    magnitudes a batch_norm_output=True processor hands to AuxLoss (negative values, |x| of a few)."""
    B, C, H, W = shape
    x, y = aux_inputs(dict(seed=seed, shape=shape, noise=0.05))
    if kind == 'noise':
        return x, y
    if kind == 'identical':
        return x, x.copy()
    if kind == 'zeros':
        return np.zeros(shape, np.float32), np.zeros(shape, np.float32)
    if kind == 'piecewise':
        # two flat levels, a horizontal step at row 23 and a vertical one at column 90 (tile boundaries are multiples of 64)
        r, c = np.arange(H).reshape(H, 1), np.arange(W).reshape(1, W)
        high = (r >= 23) ^ (c >= 90)
        lv = np.array([[0.2, 0.8], [0.35, 0.6], [0.5, 0.9]], np.float32)[np.arange(C) % 3]
        x = np.where(high, lv[:, 1].reshape(1, C, 1, 1), lv[:, 0].reshape(1, C, 1, 1)).astype(np.float32)
        y = np.where(high, lv[:, 1].reshape(1, C, 1, 1) - np.float32(0.1),
                     lv[:, 0].reshape(1, C, 1, 1) + np.float32(0.05)).astype(np.float32)
        return np.broadcast_to(x, shape).copy(), np.broadcast_to(y, shape).copy()
    if kind == 'hot_pixel':
        x = np.full(shape, 0.5, np.float32)
        y = np.full(shape, 0.5, np.float32)
        y[:, :, min(30, H - 1), min(70, W - 1)] = 1.0
        x[:, 0, min(66, H - 1), min(3, W - 1)] = 1.0       # in the first row band of the second tile row: in the halo of the first
        return x, y
    if kind == 'batchnorm':
        def bn(a):
            a = a.astype(f64)
            return ((a - a.mean(axis=(0, 2, 3), keepdims=True)) / a.std(axis=(0, 2, 3), keepdims=True)).astype(np.float32)
        return bn(x), bn(y)
    raise ValueError(kind)


_REFS = {}


def ssim_refs(key, x, y):
    """(value64, grad64, value32, grad32) of d mean-SSIM / d img2, computed once per input and shared"""
    if key not in _REFS:
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(2) as pool:      # (numpy releases the GIL: the two evaluations overlap)
            f32 = pool.submit(orc.ssim, x, y, dtype=np.float32)
            v64, g64 = orc.ssim(x, y)
            v32, g32 = f32.result()
        for a in (g64, g32):
            a.setflags(write=False)
        _REFS[key] = (float(v64), g64, float(v32), g32)
    return _REFS[key]


# ---- limits ---------------------------------------------------------------------------------------------------
def _rms(d):
    return float(np.sqrt(np.mean(np.square(d, dtype=f64))))


def grad_limits(g64, g32):
    """(rms limit, max limit, rms of the float32 oracle, max of the float32 oracle) for |grad - grad64|"""
    d_ref = np.asarray(g32, dtype=f64) - g64
    floor = pc.PLANE_GRAD_RTOL * float(np.abs(g64).max())
    r_ref, m_ref = _rms(d_ref), float(np.abs(d_ref).max())
    return max(2.0 * r_ref, floor), max(6.0 * m_ref, floor), r_ref, m_ref


def mean_limit(v64, v32):
    return max(6.0 * abs(v32 - v64), MEAN_FLOOR)


def check_grad(label, got, g64, g32, gup=1.0):
    """got = gup x (d mean / d img2) from a kernel, against gup x grad64, per pixel; the worst pixel goes into the message"""
    got = np.asarray(got, dtype=f64) / gup
    assert np.isfinite(got).all(), (label, 'non-finite gradient')
    rms_lim, max_lim, r_ref, m_ref = grad_limits(g64, g32)
    d = got - g64
    r, m = _rms(d), float(np.abs(d).max())
    worst = tuple(int(i) for i in np.unravel_index(np.abs(d).argmax(), d.shape))
    pc.report(f'{label} grad vs float64 oracle, rms; float32 oracle rms {r_ref:.2e}', r, rms_lim)
    pc.report(f'{label} grad vs float64 oracle, max; float32 oracle max {m_ref:.2e}', m, max_lim)
    assert r <= rms_lim, (label, 'rms', r, rms_lim, 'float32 oracle', r_ref)
    assert m <= max_lim, (label, 'max', m, max_lim, 'float32 oracle', m_ref, 'worst pixel (b, c, y, x)', worst,
                          'kernel', got[worst], 'float64', g64[worst])


def check_mean(label, got, v64, v32):
    lim = mean_limit(v64, v32)
    pc.report(f'{label} mean vs float64 oracle; float32 oracle {abs(v32 - v64):.2e} away', abs(got - v64), lim)
    assert abs(got - v64) <= lim, (label, 'mean', got, v64, lim)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ---- the C ABI, directly ----------------------------------------------------------------------------------------
class SsimRun:
    """r2l_ssim_fwd / r2l_ssim_bwd on (x, y) through the library that serves `device` at the time of each call"""

    def __init__(self, device, x, y):
        self.x = torch.from_numpy(np.ascontiguousarray(x)).to(device)
        self.y = torch.from_numpy(np.ascontiguousarray(y)).to(device)
        self.shape = tuple(self.x.shape)
        self.n = self.x.numel()
        self.gup = torch.full((1,), GUP, dtype=torch.float32, device=self.x.device)

    def workspace(self, fill=0xFF):
        lib, _ = _lib.library_for(self.x)
        nws = lib.r2l_aux_workspace_bytes(*self.shape)
        return torch.full((nws,), fill, dtype=torch.uint8, device=self.x.device), nws      # 0xFF bytes: float32 NaNs

    def forward(self, keep, ws=None):
        """-> (mean as float64, workspace)"""
        lib, stream = _lib.library_for(self.x)
        if ws is None:
            ws, _ = self.workspace()
        out = torch.zeros(1, dtype=torch.float64, device=self.x.device)
        lib.check(lib.r2l_ssim_fwd(ptr(self.x), ptr(self.y), ptr(out), ptr(ws), ws.numel(), int(keep), *self.shape, stream),
                  'r2l_ssim_fwd')
        return float(out.cpu()[0]), ws

    def backward(self, ws, has_dmaps, grad=None, y=None):
        lib, stream = _lib.library_for(self.x)
        y = self.y if y is None else y
        grad = torch.empty_like(self.y) if grad is None else grad
        lib.check(lib.r2l_ssim_bwd(ptr(self.x), ptr(y), ptr(self.gup), ptr(grad), ptr(ws), ws.numel(), int(has_dmaps),
                                   *self.shape, stream), 'r2l_ssim_bwd')
        return grad.cpu().numpy()

    def dmaps(self, ws):
        """the pairs (D_mu, D_22) and the plane D_12 as the workspace holds them: float32 [3 n]"""
        return ws[ws.numel() - 12 * self.n:].cpu().numpy().view(np.float32).copy()


def oracle_dmaps(x, y):
    """dS/d(mu2, E[y^2], E[xy]) per pixel in float64 (the three maps of orc.ssim's reverse pass)"""
    x, y = np.asarray(x, dtype=f64), np.asarray(y, dtype=f64)
    _, w2 = orc.ssim_window(11, dtype=f64)
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    mu1, mu2 = orc._ssim_blur(x, w2), orc._ssim_blur(y, w2)
    s11 = orc._ssim_blur(x * x, w2) - mu1 * mu1
    s22 = orc._ssim_blur(y * y, w2) - mu2 * mu2
    s12 = orc._ssim_blur(x * y, w2) - mu1 * mu2
    A1, A2 = 2 * mu1 * mu2 + C1, 2 * s12 + C2
    B1, B2 = mu1 * mu1 + mu2 * mu2 + C1, s11 + s22 + C2
    S = A1 * A2 / (B1 * B2)
    dA1, dA2, dB1, dB2 = A2 / (B1 * B2), A1 / (B1 * B2), -S / B1, -S / B2
    return 2 * mu1 * (dA1 - dA2) + 2 * mu2 * (dB1 - dB2), dB2, 2 * dA2


# ---- a. the tile walk under the hook ------------------------------------------------------------------------------
def walk_under_hook(device, grid):
    """One (forward + D maps, backward) pair with the default grid and one with R2L_GRID_AUX = grid, on the diagnostic build:
    every pixel is produced by the same instructions whichever workgroup owns its tile, so the gradient and the three D maps
    are bit-identical; the mean, whose summation order follows the grid, stays within its limit.  A backward that recomputes
    the D maps (workspace_has_dmaps = 0, over a workspace of NaNs) returns the bits of the one that was given them."""
    x, y = make_inputs('noise', WALK_SHAPE, seed=7)
    v64, g64, v32, g32 = ssim_refs(('noise', WALK_SHAPE, 7), x, y)
    assert ntiles(WALK_SHAPE) == 36 and all(g < 36 for g in WALK_GRIDS)
    run = SsimRun(device, x, y)

    def one(env):
        with pc.env_overrides(device, env):
            v, ws = run.forward(keep=1)
            d = run.dmaps(ws)
            g = run.backward(ws, has_dmaps=1)
            ws2, _ = run.workspace()
            g2 = run.backward(ws2, has_dmaps=0)
            d2 = run.dmaps(ws2)
            v0, _ = run.forward(keep=0)
        return v, d, g, g2, d2, v0

    v_a, d_a, g_a, g2_a, d2_a, v0_a = one({})
    tag = f'ssim walk {WALK_SHAPE} [{device}]'
    check_mean(f'{tag} default grid', v_a, v64, v32)
    check_grad(f'{tag} default grid', g_a, g64, g32, GUP)
    dm, d22, d12 = oracle_dmaps(x, y)
    n = x.size
    for name, got, ref in (('D_mu', d_a[0:2 * n:2], dm), ('D_22', d_a[1:2 * n:2], d22), ('D_12', d_a[2 * n:], d12)):
        # layout of the workspace (which map is which): a swap is an error of the maps' own magnitude, not of their rounding
        e = np.abs(got.astype(f64).reshape(ref.shape) - ref).max()
        lim = 1e-3 * np.abs(ref).max()
        pc.report(f'{tag} {name} map vs float64 oracle (layout check)', e, lim)
        assert e <= lim, (name, e, lim)
    assert same_bits(g2_a, g_a) and same_bits(d2_a, d_a), 'recomputed D maps / gradient differ from the kept ones'
    assert v0_a == v_a, ('keep_for_backward changes the mean', v0_a, v_a)
    v_b, d_b, g_b, g2_b, d2_b, v0_b = one({'R2L_GRID_AUX': grid})
    check_mean(f'{tag} R2L_GRID_AUX={grid}', v_b, v64, v32)
    assert v0_b == v_b
    bad = np.nonzero(bits(g_b) != bits(g_a))
    assert same_bits(g_b, g_a), (f'gradient depends on the grid ({grid})', len(bad[0]), [int(i[0]) for i in bad])
    assert same_bits(d_b, d_a), f'D maps depend on the grid ({grid})'
    assert same_bits(g2_b, g_a) and same_bits(d2_b, d_a), f'recompute path depends on the grid ({grid})'


# ---- b. the tile walk of the shipped launch --------------------------------------------------------------------------
def walk_on_product(device, shape):
    assert ntiles(shape) == PRODUCT_WALK_TILES[shape] > SSIM_GRID_CAP
    x, y = make_inputs('noise', shape, seed=11)
    v64, g64, v32, g32 = ssim_refs(('noise', shape, 11), x, y)
    run = SsimRun(device, x, y)
    v, ws = run.forward(keep=1)
    g = run.backward(ws, has_dmaps=1)
    tag = f'ssim {ntiles(shape)} tiles {shape} [{device}]'
    check_mean(tag, v, v64, v32)
    check_grad(tag, g, g64, g32, GUP)


# ---- c. tile and halo edges ------------------------------------------------------------------------------------------
def edges(device, C, H, W):
    shape = (1, C, H, W)
    x, y = make_inputs('noise', shape, seed=3)
    v64, g64, v32, g32 = ssim_refs(('noise', shape, 3), x, y)
    run = SsimRun(device, x, y)
    v, ws = run.forward(keep=1)
    g = run.backward(ws, has_dmaps=1)
    tag = f'ssim edges {shape} [{device}]'
    check_mean(tag, v, v64, v32)
    check_grad(tag, g, g64, g32, GUP)


# ---- d. input kinds ----------------------------------------------------------------------------------------------------
def kind_refs(kind):
    x, y = make_inputs(kind, KIND_SHAPE, seed=1)
    return (x, y) + ssim_refs((kind, KIND_SHAPE, 1), x, y)


def kind_oracle_is_usable(kind):
    """the float32 oracle is finite on this input and the limits it yields are not degenerate: finite, and positive wherever
    the gradient is not identically zero (all-zero images: the gradient is exactly zero in every arithmetic -- each term
    carries a factor x, y, mu1 or mu2 -- so its limit is zero and the kernels must return zeros)"""
    x, y, v64, g64, v32, g32 = kind_refs(kind)
    assert np.isfinite(v32) and np.isfinite(g32).all() and np.isfinite(v64) and np.isfinite(g64).all()
    rms_lim, max_lim, r_ref, m_ref = grad_limits(g64, g32)
    assert np.isfinite([rms_lim, max_lim]).all()
    scale = float(np.abs(g64).max())
    if kind == 'zeros':
        assert scale == 0.0 and not g32.any() and v64 == 1.0
    else:
        assert scale > 0 and rms_lim > 0 and max_lim >= rms_lim
        # ... and not vacuous either: the limit is a small fraction of the gradient's own size except on identical images,
        # where the float64 gradient is itself round-off around zero and the float32 oracle's round-off is the only scale
        if kind != 'identical':
            assert max_lim <= 0.05 * scale, (kind, max_lim, scale)
    if kind == 'identical':
        assert abs(v64 - 1.0) <= 1e-12
    assert mean_limit(v64, v32) <= 1e-3       # (flat fields: the float32 oracle's own mean is 4e-5 off)
    return rms_lim, max_lim, scale


def kinds(device, kind):
    x, y, v64, g64, v32, g32 = kind_refs(kind)
    run = SsimRun(device, x, y)
    v, ws = run.forward(keep=1)
    g = run.backward(ws, has_dmaps=1)
    tag = f'ssim {kind} {KIND_SHAPE} [{device}]'
    check_mean(tag, v, v64, v32)
    if kind == 'identical':
        lim = mean_limit(v64, v32)
        pc.report(f'{tag} mean against 1', abs(v - 1.0), lim)
        assert abs(v - 1.0) <= lim, (tag, v)
    check_grad(tag, g, g64, g32, GUP)


# ---- e. L2 ---------------------------------------------------------------------------------------------------------------
def l2_sum_bound(n, grid):
    """A-PRIORI relative bound of the float32 sum of (x - y)^2 against the float64 one.  Every term is non-negative, so the
    relative error of the sum is at most that of the term with the most roundings on its way to the result, gamma_k =
    k u / (1 - k u) with u = 2^-24 and k counted on the longest path through r2l_l2_block:
        2   d = fl(x - y), squared: (1 + u)^2
        1   the product d * d
        2   (d0^2 + d1^2) + (d2^2 + d3^2): two additions deep
        T   acc += ..., once per trip of the lane's grid-stride loop, T = ceil(n / 4 / (grid * 512))
        32  R2L_BLOCK_REDUCE: a lane's value passes 32 sequential additions of its 16-lane group ...
        16  ... and 16 of the one lane that adds the group sums
    The partials of the workgroups are then added in float64 (r2l_reduce_rows_block: < 2^-40, not counted).  Capped by
    check_aux_losses' 2e-6."""
    trips = -(-(n // 4) // (grid * L2_LANES))
    k = 2 + 1 + 2 + trips + 32 + 16
    u = 2.0 ** -24
    return min(k * u / (1.0 - k * u), L2_SUM_RTOL), trips


def _l2_inputs(n):
    rng = np.random.default_rng(1000 + n % 997)
    x = rng.random(n, dtype=np.float32)
    y = (x + np.float32(0.1) * rng.standard_normal(n, dtype=np.float32)).astype(np.float32)
    return x, y


def l2_case(device, n, grid=None, hook=False):
    """grid: R2L_GRID_AUX (hook=True: the diagnostic build) or None for the launch's own choice"""
    x_np, y_np = _l2_inputs(n)
    gup = np.float32(0.7)
    want = (np.float32(-2.0) * (x_np - y_np)) * gup            # fl(fl(-2 (x - y)) g), float32 throughout
    assert want.dtype == np.float32
    ref_sum = float(np.square(x_np.astype(f64) - y_np.astype(f64)).sum())
    x, y = torch.from_numpy(x_np).to(device), torch.from_numpy(y_np).to(device)
    g_t = torch.full((1,), float(gup), dtype=torch.float32, device=x.device)
    grad = torch.full_like(y, float('nan'))
    out = torch.zeros(1, dtype=torch.float64, device=x.device)
    ctx = pc.env_overrides(device, {'R2L_GRID_AUX': grid} if grid else {}) if hook else None
    if ctx:
        ctx.__enter__()
    try:
        lib, stream = _lib.library_for(x)
        ws = torch.full((lib.r2l_aux_workspace_bytes(1, 1, 2, 2),), 0xFF, dtype=torch.uint8, device=x.device)
        lib.check(lib.r2l_l2_fwd(ptr(x), ptr(y), ptr(out), ptr(ws), ws.numel(), n, stream), 'r2l_l2_fwd')
        lib.check(lib.r2l_l2_bwd(ptr(x), ptr(y), ptr(g_t), ptr(grad), n, stream), 'r2l_l2_bwd')
        got, total = grad.cpu().numpy(), float(out.cpu()[0])
    finally:
        if ctx:
            ctx.__exit__(None, None, None)
    blocks = -(-(n // 4) // L2_LANES)
    g_fwd = min(grid if grid else blocks, L2_FWD_CAP)
    bound, trips = l2_sum_bound(n, g_fwd)
    tag = f'l2 n={n} grid={grid or "default"} ({trips} trips forward) [{device}]'
    bad = np.nonzero(bits(got) != bits(want))[0]
    assert bad.size == 0, (tag, 'gradient bits', int(bad.size), 'first', int(bad[0]), got[bad[0]], want[bad[0]])
    err = abs(total - ref_sum) / ref_sum
    pc.report(f'{tag} sum vs float64, relative', err, bound)
    assert err <= bound, (tag, total, ref_sum, err, bound)
    return trips


# ---- f. what the ABI promises --------------------------------------------------------------------------------------------
def abi_behaviour(device):
    x, y = make_inputs('noise', WALK_SHAPE, seed=7)
    run = SsimRun(device, x, y)
    v1, ws = run.forward(keep=1)
    v0, _ = run.forward(keep=0)
    assert v0 == v1, ('keep_for_backward changes the mean', v0, v1)
    g = run.backward(ws, has_dmaps=1)
    # in place: grad_img2 == img2 (include/r2l_isp.h); from kept D maps and from recomputed ones
    for has in (1, 0):
        y_io = run.y.clone()
        ws_io = ws if has else run.workspace()[0]
        g_io = run.backward(ws_io, has_dmaps=has, grad=y_io, y=y_io)
        assert same_bits(g_io, g), f'in-place backward (workspace_has_dmaps={has}) differs from the out-of-place one'
    # a workspace one byte short: refused, nothing launched
    lib, stream = _lib.library_for(run.x)
    nws = ws.numel()
    out = torch.zeros(1, dtype=torch.float64, device=run.x.device)
    grad = torch.full_like(run.y, 7.0)
    assert lib.r2l_ssim_fwd(ptr(run.x), ptr(run.y), ptr(out), ptr(ws), nws - 1, 1, *run.shape, stream) == -2
    assert lib.r2l_ssim_bwd(ptr(run.x), ptr(run.y), ptr(run.gup), ptr(grad), ptr(ws), nws - 1, 1, *run.shape, stream) == -2
    assert float(out.cpu()[0]) == 0.0 and bool((grad == 7.0).all())
    ws_l2 = torch.zeros(4 * L2_FWD_CAP, dtype=torch.uint8, device=run.x.device)
    assert lib.r2l_l2_fwd(ptr(run.x), ptr(run.y), ptr(out), ptr(ws_l2), ws_l2.numel() - 1, run.n, stream) == -2


# ---- g. memory safety of the multi-trip launches (GPU) ---------------------------------------------------------------------
def guarded_multi_trip(device):
    """losses.SSIM forward + backward at 1050 tiles and l2_regularization at the size where both of its launches loop, each
    over NaN-poisoned and over zero-filled guard zones: nothing written outside the allocations (the workspace with its D
    maps is one of them), every result independent of the poison -- the halo fetches and the r2l_f2 reads of the D-map pairs
    at plane edges included"""
    import guarded_arena as ga
    from raw2logit_amd import losses
    shape = PRODUCT_WALK_SHAPES[1]
    assert ntiles(shape) > 2 * SSIM_GRID_CAP
    x_np, y_np = make_inputs('noise', shape, seed=11)
    v64, g64, v32, g32 = ssim_refs(('noise', shape, 11), x_np, y_np)

    def ssim_fn(arena):
        x = arena.place(x_np, 'img1')
        y = arena.place(y_np, 'img2').requires_grad_(True)
        v = losses.SSIM(window_size=11)(x, y)
        v.backward()
        return {'mean': v.detach(), 'grad': y.grad}
    res = ga.run_both(device, 64 << 20, ssim_fn, 'ssim multi-trip')
    check_mean(f'guarded ssim {shape} [{device}]', float(res['mean']), v64, v32)
    check_grad(f'guarded ssim {shape} [{device}]', res['grad'].numpy(), g64, g32)

    n = L2_PRODUCT_NS[1]
    assert n // 4 > L2_BWD_CAP * L2_LANES
    xl, yl = _l2_inputs(n)

    def l2_fn(arena):
        x = arena.place(xl, 'x')
        y = arena.place(yl, 'y').requires_grad_(True)
        v = losses.l2_regularization(x, y)
        v.backward()
        return {'sum': v.detach(), 'grad': y.grad}
    res = ga.run_both(device, 3 * 4 * n + (8 << 20), l2_fn, 'l2 multi-trip')
    want = (np.float32(-2.0) * (xl - yl)) * np.float32(1.0)
    assert same_bits(res['grad'].numpy(), want)


# ---- h. AuxLoss end to end, with values -------------------------------------------------------------------------------------
def aux_loss_values(device, batch_norm):
    """two ParametrizedProcessing modules at 2x64x72 (perturbed as in check_aux_losses): the seven parameter gradients of the
    adversarial processor against orc.parametrized_backward fed weight x d SSIM / d img2 of the float64 oracle as cotangent, at
    check_param_case's limits for parameter gradients; the default processor gets none"""
    from raw2logit_amd import losses
    from raw2logit_amd.processing import pipeline_torch as ppt
    weight = 0.7
    raw_np = orc.synth_raw(2, 64, 72, seed=31, kind='scene')
    raw = torch.from_numpy(raw_np).to(device)
    p_def = ppt.ParametrizedProcessing(orc.DRONE_CAMERA_PARAMS, batch_norm_output=batch_norm).to(device).train()
    p_adv = ppt.ParametrizedProcessing(orc.DRONE_CAMERA_PARAMS, batch_norm_output=batch_norm).to(device).train()
    with torch.no_grad():
        p_adv.gamma_correct.fill_(2.0)
        p_adv.white_balance.mul_(1.1)

    def params_of(m):
        P = orc.IspParams(orc.DRONE_CAMERA_PARAMS, dtype=f64)
        for k, v in P.by_name().items():
            v[...] = pc.NAME2ATTR[k](m).detach().cpu().numpy().reshape(v.shape)
        return P
    P_def, P_adv = params_of(p_def), params_of(p_adv)
    aux = losses.AuxLoss(losses.SSIM(window_size=11), p_adv, p_def, weight=weight)
    p_adv(raw)
    loss = aux(raw)
    loss.backward()

    bn = dict(training=True, running_mean=np.zeros(3), running_var=np.ones(3)) if batch_norm else None
    o_adv, _, cache = orc.parametrized_forward(raw_np, P_adv, track_stages=False, bn=bn)
    o_def, _, _ = orc.parametrized_forward(raw_np, P_def, track_stages=False, bn=bn)
    _, g64 = orc.ssim(o_def, o_adv)
    tag = f'AuxLoss bn={batch_norm} [{device}]'
    # the value, as check_aux_losses takes it: against the oracle's SSIM of the two outputs the modules produced; the returned
    # scalar is float32(weight x float32(mean)): two more roundings of a number below 1
    with torch.no_grad():
        mine_def, mine_adv = p_def(raw).cpu().numpy(), p_adv.buffer['processed_rgb'].detach().cpu().numpy()
    v64, _ = orc.ssim(mine_def, mine_adv)
    v32, _ = orc.ssim(mine_def, mine_adv, dtype=np.float32)
    lim_v = weight * mean_limit(float(v64), float(v32)) + 2 * 2.0 ** -24
    pc.report(f'{tag} loss vs float64 oracle', abs(loss.item() - weight * v64), lim_v)
    assert abs(loss.item() - weight * v64) <= lim_v, (loss.item(), weight * v64, lim_v)
    cot = weight * g64
    grads, _, _ = orc.parametrized_backward(P_adv, cache, cot)
    lo, _, _ = orc.parametrized_backward(P_adv, cache, cot, clip_shift=1e-6)
    hi, _, _ = orc.parametrized_backward(P_adv, cache, cot, clip_shift=-1e-6)
    assert len(grads) == 7
    for k, og in grads.items():
        og = np.asarray(og)
        got = pc.NAME2ATTR[k](p_adv).grad.detach().cpu().numpy().reshape(og.shape)
        flip = max(np.abs(np.asarray(lo[k]) - og).max(), np.abs(np.asarray(hi[k]) - og).max())
        scale = np.abs(og).max() + 1e-6
        lim = pc.DEFAULT_GRAD_RTOL * scale + flip
        e = np.abs(got - og).max()
        pc.report(f'{tag} grad {k} vs float64 oracle', e, lim)
        assert e <= lim, (tag, k, e, lim, scale, flip)
    assert all(p.grad is None for p in p_def.parameters())
