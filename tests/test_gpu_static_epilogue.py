"""The weak augmentation in the static chains' stores (StaticProcessing armed by ComposeState.arm, static_pipeline(epilogue=...),
r2l_static_fwd_epilogue) on the gfx950 build: bit for bit against the plain call followed by the permutation kernel -- both existing
code -- and against torch's own flip, one launch and no permutation kernel where an epilogue kernel serves the call, the fall-backs,
the C call, and one case of each kernel inside the guard-zone arena (tests/static_epilogue_checks.py)."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import guarded_arena as ga  # noqa: E402
import half_io_checks as hc  # noqa: E402
import parity_checks as pc  # noqa: E402
import static_epilogue_checks as se  # noqa: E402
import static_half_checks as sh  # noqa: E402
from oracle import isp_oracle as orc  # noqa: E402
from raw2logit_amd import _lib  # noqa: E402
from raw2logit_amd import augmentation as aug  # noqa: E402
from raw2logit_amd import functional as F_  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
every_type = pytest.mark.parametrize('dtype', se.OUT_DTYPES, ids=se.OUT_IDS)
CHAIN_IDS = ['bilinear_short', 'malvar_short', 'default', 'malvar_median', 'unsharp_gauss']

# every border row / partial strip / band edge of the plane passes' own list; 8 wavefronts per row (the widest served frame); a last
# strip of 4 columns; the smallest frame; two bands of the chain kernel (bands of at least 64 rows: H = 130); 26 rows: 5 bands of
# the short bilinear kernel (6 rows each, the last of 2) and 3 of the short Malvar2004 kernel (10 rows each, the last of 6)
SHAPES = [(2, H, W) for H, W in pc.FRAME_SHAPES_PLANES] + [(2, 70, 2048), (1, 14, 1028), (1, 4, 4), (2, 130, 264), (2, 26, 264)]


def _chain_for(i, W):
    """chains rotate over the shapes; unsharp_masking (4 strips at most) on widths <= 1024 only"""
    chain = sh.CHAINS[i % len(sh.CHAINS)]
    return sh.DEFAULT_CHAIN if (chain is sh.UNSHARP_GAUSS and W > 1024) else chain


@every_type
@pytest.mark.parametrize('i', range(len(SHAPES)), ids=[f'{b}x{h}x{w}' for b, h, w in SHAPES])
def test_bitwise_on_the_frame_shapes(i, dtype):
    B, H, W = SHAPES[i]
    j = se.OUT_DTYPES.index(dtype)
    # (the output types start the rotations at different places: every shape meets three chains and three moves)
    chain = _chain_for(i + 2 * j, W)
    epilogue = se.EVEN_EPILOGUES[(i + 3 * j) % len(se.EVEN_EPILOGUES)]
    raw = hc.frames(B, H, W, 1, DEV, u16=bool((i + j) & 1))
    se.check_served(chain, raw, epilogue, dtype, f'{B}x{H}x{W} {chain} {epilogue}', norm=bool((i >> 1) & 1))


@every_type
@pytest.mark.parametrize('chain', sh.CHAINS, ids=CHAIN_IDS)
def test_every_kernel_meets_every_move(chain, dtype):
    """both containers x the seven even-k moves (hflip, vflip and both among them) on two strips, the second of 4 columns; the first
    move of each kernel against torch's own flip as well; with Normalize on the container frames"""
    for u16 in (False, True):
        raw = hc.frames(2, 70, 260, 2, DEV, u16=u16)
        for n, epilogue in enumerate(se.EVEN_EPILOGUES):
            plain = se.check_served(chain, raw, epilogue, dtype, f'u16={u16} {chain} {epilogue}', norm=u16, against_torch=n == 0)
        if chain is sh.SHORT_BILINEAR and not u16:
            assert sh.reaches_both_sides_of_the_clip(plain)


@every_type
@pytest.mark.parametrize('chain', sh.CHAINS, ids=CHAIN_IDS)
def test_every_chain_on_the_widest_frames(chain, dtype):
    """8 wavefronts per row (4 behind unsharp_masking) and the last strip of 4 columns"""
    wide = 1024 if chain is sh.UNSHARP_GAUSS else 2048
    for n, (B, H, W) in enumerate(((2, 70, wide), (1, 14, 1028 if wide == 2048 else 772))):
        epilogue = se.EVEN_EPILOGUES[(n + se.OUT_DTYPES.index(dtype)) % 3]        # hflip, vflip, both
        se.check_served(chain, hc.frames(B, H, W, 4, DEV), epilogue, dtype, f'{B}x{H}x{W} {chain} {epilogue}')


@pytest.mark.parametrize('chain', [sh.SHORT_BILINEAR, sh.SHORT_MALVAR], ids=['bilinear_short', 'malvar_short'])
def test_stream_kernel_with_forced_bands(chain):
    """the diagnostic build with R2L_STREAM_BANDS = 3: three bands of 14 rows of the short chain's kernel, whatever its own choice"""
    raw = hc.frames(2, 42, 264, 5, DEV)
    with pc.env_overrides(DEV, dict(R2L_STREAM_BANDS=3)):
        for epilogue in se.EVEN_EPILOGUES[:3]:
            se.check_served(chain, raw, epilogue, None, f'3 bands {chain} {epilogue}')


@every_type
def test_fall_backs_return_the_same_bits(dtype):
    f = lambda B, H, W: hc.frames(B, H, W, 3, DEV)      # noqa: E731
    h, v, hv = se.EVEN_EPILOGUES[:3]
    for k, chain in ((1, sh.SHORT_MALVAR), (3, sh.DEFAULT_CHAIN)):
        se.check_fallback(chain, f(2, 64, 64), (True, False, k), dtype, f'k = {k} on a square frame', 'k odd')
    se.check_fallback(('menon2007', 'none', 'none'), f(2, 12, 264), h, dtype, 'Menon2007', 'menon2007')
    se.check_fallback(('bilinear', 'sharpening_filter', 'fft_denoising'), f(2, 12, 264), v, dtype, 'fft_denoising', 'fft_denoising')
    se.check_fallback(sh.SHORT_BILINEAR, f(2, 12, 262), hv, dtype, 'W = 262 (short chain)', 'W % 4')
    se.check_fallback(sh.DEFAULT_CHAIN, f(2, 12, 262), h, dtype, 'W = 262 (default chain)', 'W % 4')
    se.check_fallback(sh.SHORT_MALVAR, f(1, 12, 2052), v, dtype, 'W = 2052 (short chain)', 'W <= 2048')
    se.check_fallback(sh.DEFAULT_CHAIN, f(1, 12, 2052), hv, dtype, 'W = 2052 (default chain)', 'W <= 2048')
    se.check_fallback(sh.SHORT_BILINEAR, f(2, 12, 264).double(), h, dtype, 'float64 frames on the short chain', 'float64')
    se.check_fallback(sh.DEFAULT_CHAIN, f(2, 12, 264).double(), (False, False, 2), dtype, 'float64 frames on the default chain', 'float64')


def test_the_c_call():
    """a call that is not served returns -3 with the predicate's reason and writes nothing; unknown bits -1; epilogue = 0 is
    r2l_static_fwd_io: the same kernel, the same bits"""
    raw = hc.frames(2, 12, 264, 3, DEV)
    lib, stream = _lib.library_for(raw)
    for chain, r, bits, word in ((sh.SHORT_BILINEAR, raw, F_.epilogue_bits((False, False, 1)), b'k odd'),
                                 (('menon2007', 'none', 'none'), raw, F_.epilogue_bits((True, False, 0)), b'menon2007'),
                                 (sh.DEFAULT_CHAIN, raw.double(), F_.epilogue_bits((False, True, 0)), b'float64')):
        out = torch.full((2, 3, 12, 264), 7.0, device=DEV)
        assert se.c_call(lib, r, chain, 0, out, bits, stream) == -3 and word in lib.r2l_last_error(), (chain, lib.r2l_last_error())
        torch.cuda.synchronize()
        assert bool((out == 7.0).all())
    out = torch.full((2, 3, 12, 264), 7.0, device=DEV)
    assert se.c_call(lib, raw, sh.SHORT_BILINEAR, 0, out, 16 | 8, stream) == -1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    o0, o1 = torch.empty((2, 3, 12, 264), device=DEV), torch.empty((2, 3, 12, 264), device=DEV)
    _, names = pc.kernels_launched(lib, lambda: lib.check(se.c_call(lib, raw, sh.DEFAULT_CHAIN, 0, o0, 0, stream), 'fwd_epilogue(0)'))
    assert names == {'r2l_launch_static_chain_kernel': 1}, names
    lib.check(se.c_call(lib, raw, sh.DEFAULT_CHAIN, 0, o1, 0, stream, plain=True), 'fwd_io')
    assert torch.equal(o0, o1)
    # and a served call through the C entry alone: the permutation kernel's bits
    o2 = torch.empty((2, 3, 12, 264), device=DEV)
    _, names = pc.kernels_launched(lib, lambda: lib.check(se.c_call(lib, raw, sh.DEFAULT_CHAIN, 0, o2, F_.epilogue_bits((True, True, 0)), stream),
                                                          'fwd_epilogue'))
    assert names == {'r2l_launch_static_chain_epi_kernel': 1}, names
    assert torch.equal(o2, aug.flip_rot(o1, True, True, 0))


@pytest.mark.parametrize('dtype', [None, torch.bfloat16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('chain', [sh.SHORT_MALVAR, sh.DEFAULT_CHAIN], ids=['stream_kernel', 'chain_kernel'])
def test_epilogue_stores_inside_the_guarded_arena(chain, dtype):
    """every allocation of the call between poisoned guard zones, hflip + vflip on two images of 70 x 260: no byte outside the blocks
    written -- a store based one group off under sc = -1 leaves the first plane of the output's block at its low end -- and results
    independent of the poison"""
    B, H, W = 2, 70, 260
    raw_np = orc.synth_raw(B, H, W, seed=6, kind='scene')
    esz = 4 if dtype is None else 2

    def fn(arena):
        m = sh.module(chain, norm=True).to(DEV)
        m.output_dtype = dtype
        y = se.armed_call(m, arena.place(raw_np, 'raw'), (True, True, 0))
        assert y.is_contiguous() and any(e - s == y.numel() * esz for s, e, _ in arena.blocks)
        return {'out': y}
    res = ga.run_both(DEV, 16 << 20, fn, f'static epilogue {dtype} {chain}')
    plain = sh.module(chain, norm=True).to(DEV)(torch.from_numpy(raw_np).to(DEV))
    want = plain.flip(-1).flip(-2)
    assert torch.equal(res['out'], (want if dtype is None else want.to(dtype)).cpu())
