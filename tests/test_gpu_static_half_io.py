"""16-bit output of the static chains (StaticProcessing.output_dtype = torch.bfloat16 / torch.float16, r2l_static_fwd_io) on the
gfx950 build: bit for bit against the float32 call on the frame shapes, containers and Normalize, the fall-backs, the unchanged
default, the reference's golden cases within the derived rounding margin, and one case of each kernel inside the guard-zone arena
(tests/static_half_checks.py)."""
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
from oracle import isp_oracle as orc  # noqa: E402
from oracle.golden_cases import STATIC_CASES, STATIC_OPT_CASES  # noqa: E402
from raw2logit_amd import _lib  # noqa: E402
from raw2logit_amd import functional as F_  # noqa: E402
from raw2logit_amd.processing import pipeline_numpy as ppn  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
both = pytest.mark.parametrize('dtype', sh.DTYPES, ids=sh.DTYPE_IDS)

# every border row / partial strip / band edge of the plane passes' own list, 8 wavefronts per row (the widest served frame), the
# smallest frame
SHAPES = [(2, H, W) for H, W in pc.FRAME_SHAPES_PLANES] + [(2, 70, 2048), (1, 4, 4)]


def _chain_for(i, W):
    """chains rotate over the shapes; unsharp_masking (4 strips at most) on widths <= 1024 only"""
    chain = sh.CHAINS[i % len(sh.CHAINS)]
    return sh.DEFAULT_CHAIN if (chain is sh.UNSHARP_GAUSS and W > 1024) else chain


@both
@pytest.mark.parametrize('i', range(len(SHAPES)), ids=[f'{b}x{h}x{w}' for b, h, w in SHAPES])
def test_bitwise_on_the_frame_shapes(i, dtype):
    B, H, W = SHAPES[i]
    # (the two output types start the rotation at different chains: every shape meets two chains)
    chain = _chain_for(i + (2 if dtype is torch.float16 else 0), W)
    sh.check_served(chain, hc.frames(B, H, W, 1, DEV, u16=bool(i & 1)), dtype, f'{B}x{H}x{W} {chain}')


@both
@pytest.mark.parametrize('chain', sh.CHAINS, ids=['bilinear_short', 'malvar_short', 'default', 'malvar_median', 'unsharp_gauss'])
def test_every_chain_on_the_widest_frames(chain, dtype):
    """8 wavefronts per row (4 behind unsharp_masking) and the last strip of 4 columns"""
    wide = 1024 if chain is sh.UNSHARP_GAUSS else 2048
    for B, H, W in ((2, 70, wide), (1, 14, 1028 if wide == 2048 else 772)):
        sh.check_served(chain, hc.frames(B, H, W, 4, DEV), dtype, f'{B}x{H}x{W} {chain}')


@both
@pytest.mark.parametrize('norm', [False, True], ids=['plain', 'normalize'])
@pytest.mark.parametrize('container', ['float32', 'uint16', 'float64'])
def test_containers_and_normalize(container, norm, dtype):
    B, H, W = 2, 70, 260
    raw = hc.frames(B, H, W, 2, DEV, u16=container == 'uint16')
    if container == 'float64':
        raw = raw.double()
    for chain in sh.CHAINS[:2] if container == 'float64' else sh.CHAINS:      # float64 frames: short chains only
        y32 = sh.check_served(chain, raw, dtype, f'{container} norm={norm} {chain}', norm=norm)
        if chain is sh.SHORT_BILINEAR and not norm:      # these frames: values inside the clip, below it and above it
            assert sh.reaches_both_sides_of_the_clip(y32)


@both
def test_fall_backs_return_the_same_bits(dtype):
    f = lambda B, H, W: hc.frames(B, H, W, 3, DEV)      # noqa: E731
    sh.check_fallback(('menon2007', 'none', 'none'), f(2, 12, 264), dtype, 'Menon2007', 'menon2007')
    sh.check_fallback(('bilinear', 'sharpening_filter', 'fft_denoising'), f(2, 12, 264), dtype, 'fft_denoising', 'fft_denoising')
    sh.check_fallback(('bilinear', 'sharpening_filter', 'median_denoising'), f(2, 12, 264), dtype, 'median_kernel_size=5', '5x5 median',
                      median_kernel_size=5)
    sh.check_fallback(sh.SHORT_BILINEAR, f(2, 12, 262), dtype, 'W = 262 (short chain)', 'W % 4')
    sh.check_fallback(sh.DEFAULT_CHAIN, f(2, 12, 262), dtype, 'W = 262 (default chain)', 'W % 4')
    sh.check_fallback(sh.SHORT_MALVAR, f(1, 12, 2052), dtype, 'W = 2052 (short chain)', 'W <= 2048')
    sh.check_fallback(sh.DEFAULT_CHAIN, f(1, 12, 2052), dtype, 'W = 2052 (default chain)', 'W <= 2048')
    sh.check_fallback(sh.UNSHARP_GAUSS, f(1, 12, 1028), dtype, 'unsharp_masking at W = 1028', 'unsharp_masking')
    sh.check_fallback(sh.DEFAULT_CHAIN, f(2, 12, 264).double(), dtype, 'float64 frames on the default chain', 'float64 frames')
    # the C call itself: -3 with the predicate's reason, nothing written; an unknown out_io: -1
    raw = f(2, 12, 264)
    lib, stream = _lib.library_for(raw)
    out = torch.full((2, 3, 12, 264), 7.0, dtype=dtype, device=DEV)
    e = sh.c_call_io(lib, raw, ('menon2007', 'none', 'none'), F_.IO_CODES[dtype], out, stream)
    assert e == -3 and b'menon2007' in lib.r2l_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert sh.c_call_io(lib, raw, sh.SHORT_BILINEAR, 9, out, stream) == -1
    # out_io = R2L_IO_F32 is today's call: the same kernel, the same bits
    o32 = torch.empty((2, 3, 12, 264), device=DEV)
    _, names = pc.kernels_launched(lib, lambda: lib.check(sh.c_call_io(lib, raw, sh.DEFAULT_CHAIN, 0, o32, stream), 'fwd_io f32'))
    assert names == {'r2l_launch_static_chain_kernel': 1}, names
    assert torch.equal(o32, F_.static_pipeline(raw, orc.DRONE_CAMERA_PARAMS))


def test_default_is_unchanged():
    """output_dtype never set, None and torch.float32: float32 output, the launch record of a call that never heard of the attribute
    (functional.static_pipeline as the parent commit calls it), bit-identical results"""
    B, H, W = 2, 70, 260
    today = {sh.SHORT_BILINEAR: 'r2l_launch_static_stream_bilinear_kernel', sh.SHORT_MALVAR: 'r2l_launch_static_stream_malvar_kernel',
             sh.DEFAULT_CHAIN: 'r2l_launch_static_chain_kernel', sh.MALVAR_MEDIAN: 'r2l_launch_static_chain_malvar_median_kernel',
             sh.UNSHARP_GAUSS: 'r2l_launch_static_chain_unsharp_kernel'}
    for u16 in (False, True):
        raw = hc.frames(B, H, W, 5, DEV, u16=u16)
        lib = _lib.library_for(raw)[0]
        for chain in sh.CHAINS:
            for norm in (False, True):
                plain, n0 = pc.kernels_launched(lib, lambda: F_.static_pipeline(
                    raw, orc.DRONE_CAMERA_PARAMS, *chain, mean_std=(sh.MEAN + sh.STD) if norm else None))
                want = today[chain].replace('_kernel', '_u16_kernel') if u16 else today[chain]
                assert n0 == {want: 1}, (chain, n0)
                for odt in ('unset', None, torch.float32):
                    m = sh.module(chain, norm).to(DEV)
                    if odt != 'unset':
                        m.output_dtype = odt
                    assert ppn.StaticProcessing.output_dtype is None
                    y, n = pc.kernels_launched(lib, lambda: m(raw))
                    assert y.dtype == torch.float32 and torch.equal(y, plain) and n == n0, (chain, norm, odt, n)


@both
@pytest.mark.parametrize('case', STATIC_CASES, ids=[c['name'] for c in STATIC_CASES])
def test_golden_static_cases(case, golden, dtype):
    sh.check_golden(case, golden, 'static_cases', dtype, DEV)


@both
@pytest.mark.parametrize('case', STATIC_OPT_CASES, ids=[c['name'] for c in STATIC_OPT_CASES])
def test_golden_static_option_cases(case, golden, dtype):
    sh.check_golden(case, golden, 'static_opts', dtype, DEV)


@both
@pytest.mark.parametrize('chain', [sh.SHORT_MALVAR, sh.DEFAULT_CHAIN], ids=['stream_kernel', 'chain_kernel'])
def test_sixteen_bit_output_inside_the_guarded_arena(chain, dtype):
    """every allocation of the call -- the 2-byte output, half the float32 one's size, among them -- between poisoned guard zones:
    no byte outside them written (a store of float32 width, or at a float32 offset, would land in a guard zone), results independent
    of the poison"""
    B, H, W = 2, 70, 260
    raw_np = orc.synth_raw(B, H, W, seed=6, kind='scene')

    def fn(arena):
        m = sh.module(chain, norm=True).to(DEV)
        m.output_dtype = dtype
        y = m(arena.place(raw_np, 'raw'))
        assert y.dtype == dtype and any(e - s == y.numel() * 2 for s, e, _ in arena.blocks)
        return {'out': y}
    res = ga.run_both(DEV, 16 << 20, fn, f'static half-io {dtype} {chain}')
    m32 = sh.module(chain, norm=True).to(DEV)
    assert torch.equal(res['out'], m32(torch.from_numpy(raw_np).to(DEV)).to(dtype).cpu())
