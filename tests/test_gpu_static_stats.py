"""Channel mean / std of a static chain without its output (r2l_static_stats, r2l_channel_sums) on the gfx950 build: every pixel
exactly once on the frame shapes, the sums against math.fsum of the float32 output within the any-order bound, the routes, the
reference's golden cases, capped grids, more items than one grid pass, and one stream and one chain kernel inside the guard-zone
arena (tests/static_stats_checks.py)."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import guarded_arena as ga  # noqa: E402
import half_io_checks as hc  # noqa: E402
import parity_checks as pc  # noqa: E402
import static_half_checks as sh  # noqa: E402
import static_stats_checks as sc  # noqa: E402
from oracle import isp_oracle as orc  # noqa: E402
from oracle.golden_cases import STATIC_CASES, STATIC_OPT_CASES  # noqa: E402
from raw2logit_amd import _lib  # noqa: E402
from raw2logit_amd import functional as F_  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CHAIN_IDS = ['bilinear_short', 'malvar_short', 'default', 'malvar_median', 'unsharp_gauss']

# every border row / partial strip / band edge of the plane passes' own list, 8 wavefronts per row (the widest served frame), a
# last strip of 4 columns behind four full ones, the smallest frame
SHAPES = [(2, H, W) for H, W in pc.FRAME_SHAPES_PLANES] + [(2, 70, 2048), (1, 14, 1028), (1, 4, 4)]


def _chain_for(i, W):
    """chains rotate over the shapes; unsharp_masking (4 strips at most) on widths <= 1024 only"""
    chain = sc.CHAINS[i % len(sc.CHAINS)]
    return sh.DEFAULT_CHAIN if (chain is sh.UNSHARP_GAUSS and W > 1024) else chain


def _kind_for(i, chain):
    """frame kinds rotate too: float32, 16-bit containers, and float64 where the chain is a short one"""
    kind = sc.KINDS[i % 3]
    return 'f32' if (kind == 'f64' and not sc.is_short(chain)) else kind


@pytest.mark.parametrize('rot', [0, 2], ids=['rotation0', 'rotation2'])
@pytest.mark.parametrize('i', range(len(SHAPES)), ids=[f'{b}x{h}x{w}' for b, h, w in SHAPES])
def test_pixels_values_and_routes_on_the_frame_shapes(i, rot):
    """checks 1, 2, 4 and 5; the two rotations start at different chains: every shape meets two chains"""
    B, H, W = SHAPES[i]
    chain = _chain_for(i + rot, W)
    kind = _kind_for(i + rot // 2, chain)
    label = f'{B}x{H}x{W} {chain} {kind}'
    sc.check_every_pixel_once(chain, B, H, W, DEV, kind, label)
    raw = sc.scene(B, H, W, 1, DEV, kind)
    sums = sc.check_served(chain, raw, label)
    sc.check_sums_against(sums, F_.static_pipeline(raw, orc.DRONE_CAMERA_PARAMS, *chain), label)
    sc.check_repeatable(chain, raw, label)


@pytest.mark.parametrize('kind', sc.KINDS)
@pytest.mark.parametrize('chain', sc.CHAINS, ids=CHAIN_IDS)
def test_every_chain_and_container_at_2x70x260(chain, kind):
    if kind == 'f64' and not sc.is_short(chain):
        why = sc.check_unserved(chain, sc.scene(2, 70, 260, 2, DEV, 'f64'), f'float64 frames on {chain}', 'float64 frames')
        assert 'statistics' in why
        return
    label = f'2x70x260 {chain} {kind}'
    sc.check_every_pixel_once(chain, 2, 70, 260, DEV, kind, label)
    raw = sc.scene(2, 70, 260, 2, DEV, kind)
    sums = sc.check_served(chain, raw, label)
    out32 = F_.static_pipeline(raw, orc.DRONE_CAMERA_PARAMS, *chain)
    sc.check_sums_against(sums, out32, label)
    assert sh.reaches_both_sides_of_the_clip(out32)


def test_unserved_calls_say_why_and_fall_back():
    f = lambda B, H, W: hc.frames(B, H, W, 3, DEV)      # noqa: E731
    sc.check_unserved(('menon2007', 'none', 'none'), f(2, 12, 264), 'Menon2007', 'menon2007')
    sc.check_unserved(('bilinear', 'sharpening_filter', 'fft_denoising'), f(2, 12, 264), 'fft_denoising', 'fft_denoising')
    sc.check_unserved(('bilinear', 'sharpening_filter', 'median_denoising'), f(2, 12, 264), 'median_kernel_size=5', '5x5 median',
                      options=(1.0, 1.0, 0.5, 0.3, 5.0), median_kernel_size=5)
    sc.check_unserved(sh.SHORT_BILINEAR, f(2, 12, 262), 'W = 262 (short chain)', 'W % 4')
    sc.check_unserved(sh.DEFAULT_CHAIN, f(2, 12, 262), 'W = 262 (default chain)', 'W % 4')
    sc.check_unserved(sh.SHORT_MALVAR, f(1, 12, 2052), 'W = 2052 (short chain)', 'W <= 2048')
    sc.check_unserved(sh.DEFAULT_CHAIN, f(1, 12, 2052), 'W = 2052 (default chain)', 'W <= 2048')
    sc.check_unserved(sh.UNSHARP_GAUSS, f(1, 12, 1028), 'unsharp_masking at W = 1028', 'unsharp_masking')
    # the other codes of the C call: a workspace one byte short -2, null pointers -1, what r2l_static_fwd_opts refuses -4
    raw = f(2, 12, 264)
    lib, stream = _lib.library_for(raw)
    sums = torch.full((7,), 7.0, dtype=torch.float64, device=DEV)
    n = lib.r2l_static_stats_workspace_bytes(0, 2, 12, 264, 0, 1, 1, None)
    ws = torch.empty(n, dtype=torch.uint8, device=DEV)
    assert n > 0 and sc.c_call(lib, raw, sh.DEFAULT_CHAIN, sums, ws, n - 1, stream) == -2
    assert sc.c_call(lib, raw, sh.DEFAULT_CHAIN, None, ws, n, stream) == -1
    assert sc.c_call(lib, raw, sh.DEFAULT_CHAIN, sums, ws, n, stream, options=(1.0, 1.0, 0.7, 0.3, 3.0)) == -4
    torch.cuda.synchronize()
    assert sums.cpu().tolist() == [7.0] * 7
    assert sc.c_call(lib, raw, sh.DEFAULT_CHAIN, sums, ws, n, stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(sums, F_.static_statistics(raw, orc.DRONE_CAMERA_PARAMS))


@pytest.mark.parametrize('case', STATIC_CASES, ids=[c['name'] for c in STATIC_CASES])
def test_golden_static_cases(case, golden):
    sc.check_golden(case, golden, 'static_cases', DEV)


@pytest.mark.parametrize('case', STATIC_OPT_CASES, ids=[c['name'] for c in STATIC_OPT_CASES])
def test_golden_static_option_cases(case, golden):
    sc.check_golden(case, golden, 'static_opts', DEV)


@pytest.mark.parametrize('grid', [1, 3])
@pytest.mark.parametrize('chain', [sh.SHORT_BILINEAR, sh.SHORT_MALVAR, sh.DEFAULT_CHAIN, sh.MALVAR_MEDIAN], ids=CHAIN_IDS[:4])
def test_capped_grids_on_the_diagnostic_build(chain, grid):
    """R2L_GRID_STATIC = 1 and 3: a workgroup walks several work items, the finish adds 4 or 12 (2 or 6) partials"""
    with pc.env_overrides(DEV, dict(R2L_GRID_STATIC=grid)):
        label = f'R2L_GRID_STATIC={grid} {chain}'
        sc.check_every_pixel_once(chain, 2, 70, 260, DEV, 'f32', label)
        raw = sc.scene(2, 70, 260, 7, DEV, 'u16' if grid == 3 else 'f32')
        lib = _lib.library_for(raw)[0]
        nws = lib.r2l_static_stats_workspace_bytes(1 if grid == 3 else 0, 2, 70, 260, F_._DEBAYER[chain[0]], F_._SHARPEN.get(chain[1], 0),
                                                   F_._DENOISE.get(chain[2], 0), None)
        # 48 or 28 work items of the short chains, 4 wavefronts per workgroup; 2 bands of the luma chains, 2 strips per workgroup
        assert nws == 48 * (grid * 4 if sc.is_short(chain) else min(grid, 2) * 2)
        sc.check_values(chain, raw, label)


def test_more_work_items_than_one_grid_pass():
    """The statistics launches are capped at 2048 workgroups.  8x512x512: the short bilinear chain has 8 * 2 strips * 86 bands =
    1376 work items = 344 workgroups of 4 wavefronts, the default chain 8 images * 8 bands = 64 workgroups -- below the cap, so every
    workgroup there takes one pass.  The cap counts work items, not pixels, so the smallest shapes that reach it are many small
    frames: 4097x12x8 for the short chains (2 bands per frame: 8194 work items, 8192 wavefronts) and 2049x64x64 for the luma chains
    (one band per frame: 2049 bands, 2048 workgroups) -- on the product build the first workgroup takes a second item there.  At
    8x512x512 the several-passes path runs through the diagnostic build's cap (64 workgroups: 6 passes of the short chains, 1 of the
    default chain)"""
    for chain in (sh.SHORT_BILINEAR, sh.DEFAULT_CHAIN):
        sc.check_every_pixel_once(chain, 8, 512, 512, DEV, 'f32', f'8x512x512 {chain}')
    for chain in (sh.SHORT_BILINEAR, sh.SHORT_MALVAR):
        sc.check_every_pixel_once(chain, 4097, 12, 8, DEV, 'f32', f'4097x12x8 {chain}')
    for chain in (sh.DEFAULT_CHAIN, sh.MALVAR_MEDIAN):
        sc.check_every_pixel_once(chain, 2049, 64, 64, DEV, 'u16', f'2049x64x64 {chain}')
    with pc.env_overrides(DEV, dict(R2L_GRID_STATIC=64)):
        for chain in (sh.SHORT_BILINEAR, sh.SHORT_MALVAR, sh.DEFAULT_CHAIN):
            sc.check_every_pixel_once(chain, 8, 512, 512, DEV, 'u16', f'8x512x512 cap 64 {chain}')


@pytest.mark.parametrize('chain', [sh.SHORT_MALVAR, sh.DEFAULT_CHAIN], ids=['stream_kernel', 'chain_kernel'])
def test_statistics_inside_the_guarded_arena(chain):
    """every allocation of the call -- frames, the workspace of partials, sums[7] -- between poisoned guard zones: no byte outside
    them written, the result independent of the poison (a partial that is read before it is written would differ)"""
    B, H, W = 2, 70, 260
    raw_np = orc.synth_raw(B, H, W, seed=6, kind='scene')

    def fn(arena):
        sums = F_.static_statistics(arena.place(raw_np, 'raw'), orc.DRONE_CAMERA_PARAMS, *chain)
        assert any(e - s == 56 for s, e, _ in arena.blocks)
        return {'sums': sums}
    res = ga.run_both(DEV, 16 << 20, fn, f'static stats {chain}')
    assert torch.equal(res['sums'], F_.static_statistics(torch.from_numpy(raw_np).to(DEV), orc.DRONE_CAMERA_PARAMS, *chain).cpu())


@pytest.mark.parametrize('shape', [(3, 1, 1, 1), (2, 3, 35, 67), (1, 4, 35, 66), (2, 3, 70, 260)], ids=lambda s: 'x'.join(map(str, s)))
def test_channel_sums(shape):
    g = torch.Generator().manual_seed(sum(shape))
    x = (torch.rand(shape, generator=g) * 2.0 - 0.5).to(DEV)
    sums = sc.check_channel_sums(x, f'channel_sums {shape}')
    assert torch.equal(sums, F_.channel_sums(x))
    flat = torch.empty(x.numel() + 1, device=DEV)
    flat[1:] = x.reshape(-1)
    view = flat[1:].view(shape)
    assert view.data_ptr() % 16 == 4
    sc.check_channel_sums(view, f'channel_sums {shape} offset 1')
    for grid in (1, 3):
        with pc.env_overrides(DEV, dict(R2L_GRID_FLAT=grid)):
            assert torch.equal(F_.channel_sums(x), sums), grid


def test_channel_sums_of_the_packed_mosaic():
    """mosaic_mean / mosaic_std of RawToRGB's packed output (train.py:187-189) at 2x70x134: planes of 35 x 67"""
    raw = hc.frames(2, 70, 134, 8, DEV)
    for oc in (3, 4):
        x = F_.raw2rgb(raw, None, True, oc)
        assert tuple(x.shape) == (2, oc, 35, 67)
        sums = sc.check_channel_sums(x, f'raw2rgb 2x{oc}x35x67')
        mean, std = F_.mean_std_from_sums(sums)
        # (float64 on torch's side: what is left is the float32 rounding of the returned values, which are below 1)
        assert (mean.reshape(oc).double() - x.double().mean(dim=(0, 2, 3))).abs().max() <= 2.0 ** -24
        assert (std.reshape(oc).double() - x.double().std(dim=(0, 2, 3))).abs().max() <= 2.0 ** -24
