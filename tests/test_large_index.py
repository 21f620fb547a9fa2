"""The host-only part of the large-index checks (tests/large_index_checks.py; the GPU part: tests/test_gpu_large_index.py): the
comparison logic on synthetic results, the size queries against Python integers at the shapes the GPU cases use, at 2^29-pixel
frames and at 2^40-pixel batches, and the refusals at the documented limits on the lock-step emulation's sources.  No GPU, no large
allocation."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import guarded_arena as ga  # noqa: E402
import large_index_checks as lc  # noqa: E402
import lockstep_driver  # noqa: E402


# ---- the comparison logic ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.float16], ids=['f32', 'bf16', 'f16'])
@pytest.mark.parametrize('channels_last', [False, True], ids=['planar', 'nhwc'])
def test_periodic_check_reports_the_first_differing_block_and_its_element(dtype, channels_last):
    """a synthetic result whose tail blocks differ -- what an image base narrowed to 32 bits leaves behind: the frames past the
    wrap are written over the head or not at all.  The check names the FIRST bad block and the flat offset of its first bad
    element, whatever the chunk size, and passes on the intact tensor"""
    R, shape = 9, (lc.BB, 3, 6, 8)
    logged = len(lc.pc.ERROR_LOG)
    g = torch.Generator().manual_seed(3)
    block = torch.randn(shape, generator=g).to(dtype)
    block[0, 0, 0, 0] = float('nan')                       # bitwise: NaN equals NaN
    if channels_last:
        y = block.permute(0, 2, 3, 1).contiguous().repeat(R, 1, 1, 1).permute(0, 3, 1, 2)
        assert y.is_contiguous(memory_format=torch.channels_last) and not y.is_contiguous()
    else:
        y = block.repeat(R, 1, 1, 1)
    per = block.numel()
    flat = lc.bits(y)
    assert flat.numel() == R * per and flat.data_ptr() == y.data_ptr()
    for chunk in (1, per * y.element_size(), 3 * per * y.element_size() + 1, 1 << 30):
        assert lc.first_mismatch(flat, per, chunk_bytes=chunk) is None
    lc.assert_periodic(y, R, 'intact')
    # the tail: blocks 6, 7, 8 from element 5 of block 6 on
    bad = y.clone(memory_format=torch.preserve_format)
    fb = lc.memory_order(bad)
    assert fb.data_ptr() == bad.data_ptr()
    fb[6 * per + 5:] = 0.25
    want = 6 * per + 5
    while lc.bits(bad)[want] == lc.bits(y)[want]:          # (an element that happened to hold 0.25 already)
        want += 1
    for chunk in (1, per * y.element_size(), 3 * per * y.element_size() + 1, 1 << 30):
        got = lc.first_mismatch(lc.bits(bad), per, chunk_bytes=chunk)
        assert got is not None and got['block'] == 6 and got['offset'] == want, (chunk, got, want)
        assert got['differing'] == int((lc.bits(bad)[6 * per:7 * per] != lc.bits(y)[:per]).sum())
    with pytest.raises(AssertionError, match=f'block 6 of {R} differs from block 0, first at flat element {want} '):
        lc.assert_periodic(bad, R, 'tail')
    # one element of the LAST block; a sign of zero (equal as numbers, different bits)
    one = y.clone(memory_format=torch.preserve_format)
    lc.memory_order(one)[R * per - 1] = -lc.memory_order(one)[R * per - 1] * 0.0
    got = lc.first_mismatch(lc.bits(one), per)
    if lc.bits(one)[R * per - 1] != lc.bits(y)[per - 1]:
        assert got == dict(block=R - 1, offset=R * per - 1, differing=1)
    # a window of periods, as the tall-frame check uses it: periods 1 .. 7 against period 1; period 0 and 8 may differ
    win = y.clone(memory_format=torch.preserve_format)
    lc.memory_order(win)[:per] = 0.5
    lc.memory_order(win)[8 * per:] = 0.5
    assert lc.first_mismatch(lc.bits(win), per, first=1, count=R - 2) is None
    assert lc.first_mismatch(lc.bits(win), per, first=1, count=R - 1)['block'] == 8
    # unwritten elements
    nan = y.clone(memory_format=torch.preserve_format)
    lc.memory_order(nan)[7 * per + 1:7 * per + 4] = float('nan')
    assert lc.count_nan(nan, chunk_bytes=64) == R + 3 and lc.count_nan(y) == R
    del lc.pc.ERROR_LOG[logged:]      # (the synthetic failures above are no rows of the achieved-error table)


def test_guard_zones_are_checked_zone_by_zone():
    """the zone-by-zone form of Arena.check_guards: payloads of odd sizes (zone edges off the 4-byte grid), the zone before the
    first payload, between two, and the unused tail; chunks smaller than a zone"""
    def arena():
        a = ga.Arena('cpu', 1 << 20, 'nan')
        p = a.alloc((1001,), torch.uint8, 'odd')
        q = a.alloc((33, 7), torch.float32, 'q')
        r = a.alloc((5,), torch.bfloat16, 'r')
        for t in (p, q, r):
            t.view(torch.uint8).fill_(1)
        return a
    a = arena()
    assert lc.check_guard_zones(a, 'intact') == 4
    assert lc.check_guard_zones(a, 'intact', chunk_bytes=4096) == 4
    a.check_guards('intact')
    (s0, e0, _), (s1, e1, _), (s2, e2, _) = a.blocks
    assert e0 % 4 and e2 % 4 == 2
    for off in (0, s0 - 1, e0, e0 + 1, e0 + 2, e0 + 3, s1 - 1, e1, e1 + 40000, s2 - 3, e2, e2 + 1, a.nbytes - 1, a.nbytes - 70000):
        b = arena()
        b.buf[off] ^= 0x10
        for chunk in (4096, 1 << 30):
            with pytest.raises(AssertionError, match=f'guard byte {off} overwritten'):
                lc.check_guard_zones(b, 'hit', chunk_bytes=chunk)
        with pytest.raises(AssertionError):
            b.check_guards('hit')
    b = arena()
    b.buf[s1 + 5] ^= 0x10        # inside a payload: not a guard
    lc.check_guard_zones(b, 'payload')


def test_guarded_serves_a_channels_last_output():
    orig = torch.empty
    with lc.guarded('cpu', lc.arena_bytes(2 * 3 * 4 * 6 * 2, 64, 24)) as arena:
        y = torch.empty((2, 3, 4, 6), dtype=torch.bfloat16, device='cpu', memory_format=torch.channels_last)
        z = torch.empty(16, dtype=torch.float32, device='cpu')
        w = torch.empty((2, 3), dtype=torch.float32, device='cpu', memory_format=torch.contiguous_format)
        assert y.is_contiguous(memory_format=torch.channels_last) and tuple(y.shape) == (2, 3, 4, 6)
        assert len(arena.blocks) == 3 and bool(torch.isnan(z).all()) and w.is_contiguous()
        lo = arena.buf.data_ptr()
        assert all(lo <= t.data_ptr() < lo + arena.nbytes for t in (y, z, w))
        assert lc.count_nan(y) == y.numel() // 2       # the float32 poison seen as bfloat16: 0x0000, 0x7FC0
        y.fill_(1.0)
        lc.check_guard_zones(arena, 'channels-last payload')
    assert torch.empty is orig
    assert lc.arena_bytes(10, 20) >= 2 * (ga.GUARD + 256) + ga.GUARD


# ---- the size queries against Python integers -------------------------------------------------------------------------------
def _strictly_increasing(f, B, *rest):
    vals = [f(b, *rest) for b in (B - 1, B, B + 1)]
    assert vals[0] < vals[1] < vals[2], (f, B, rest, vals)


def test_size_queries_are_the_closed_forms(emulation):
    """every workspace / scratch / offset query at the GPU cases' shapes, at frames of 2^29 px and at batches of 2^40 px, against
    the closed form in Python integers (which do not wrap): exact, strictly increasing in B, offsets strictly ordered"""
    lib = emulation
    al = lc.align256
    S = lc.STEP_SLOTS
    small = (1, 4, 4)
    head = lib.r2l_isp_workspace_bytes(*small) - 3 * al(4 * 16)
    fixed = {k: lib.r2l_isp_step_offset(v, *small) for k, v in S.items() if k != 'LUMA'}
    assert 0 < fixed['PACKED'] < fixed['BN'] < fixed['STATS'] < fixed['MOMENTS'] < fixed['BN_SUMS'] < head and head % 256 == 0
    assert fixed['MOMENTS'] == fixed['STATS'] + 64 and fixed['BN_SUMS'] == fixed['STATS'] + 128 and fixed['BN_SUMS'] + 48 <= head
    assert fixed['BN'] - fixed['PACKED'] >= 4 * 150 and fixed['STATS'] - fixed['BN'] >= 64
    opts = {m: (ctypes.c_double * 5)(1.0, 1.0, 0.5, 0.3, float(m)) for m in (3, 5)}
    assert max(b * h * w for b, h, w in lc.QUERY_SHAPES) == 2 ** 40 and sum(h * w == 2 ** 29 for _, h, w in lc.QUERY_SHAPES) >= 3
    for B, H, W in lc.QUERY_SHAPES:
        px = B * H * W
        assert H * W <= 2 ** 29 and px <= 2 ** 40
        plane = al(4 * px)
        assert lib.r2l_isp_workspace_bytes(B, H, W) == head + 3 * plane, (B, H, W)
        _strictly_increasing(lib.r2l_isp_workspace_bytes, B, H, W)
        for k, v in fixed.items():
            assert lib.r2l_isp_step_offset(S[k], B, H, W) == v, (k, B, H, W)
        luma = lib.r2l_isp_step_offset(S['LUMA'], B, H, W)
        assert luma == head + plane and fixed['BN_SUMS'] < luma and luma + 2 * plane == lib.r2l_isp_workspace_bytes(B, H, W)
        assert lib.r2l_isp_raw_grad_scratch_bytes(B, H, W) == 8 * px
        _strictly_increasing(lib.r2l_isp_raw_grad_scratch_bytes, B, H, W)
        # static chains: (debayer, sharpening, denoising) codes of include/r2l_isp.h; routes that do not depend on the build
        for f in (lib.r2l_static_workspace_bytes, lib.r2l_static_workspace_bytes_f64):
            assert f(B, H, W, 0, 0, 0) == 0 and f(B, H, W, 1, 0, 0) == 0             # the short chains: one launch, no workspace
            assert f(B, H, W, 2, 0, 0) == f(B, H, W, 2, 1, 1) == al(64 * px), (B, H, W)     # Menon2007: 8 float64 planes
            _strictly_increasing(f, B, H, W, 2, 0, 0)
        assert lib.r2l_static_workspace_bytes(B, H, W, 0, 1, 1) == 0                   # the default chain
        for frames in (0, 1, 2):
            q = lib.r2l_static_workspace_bytes_opts
            assert q(frames, B, H, W, 0, 1, 2, opts[5]) == 16 * px, (frames, B, H, W)  # a 5x5 median: 2 float64 luma planes
            assert q(frames, B, H, W, 1, 0, 2, opts[5]) == 16 * px
            assert q(frames, B, H, W, 2, 1, 2, opts[5]) == al(64 * px)
            assert q(frames, B, H, W, 0, 0, 0, opts[3]) == 0 and q(frames, B, H, W, 2, 0, 0, None) == al(64 * px)
            _strictly_increasing(lambda b, *r: q(frames, b, *r), B, H, W, 0, 1, 2, opts[5])
        # losses (C = 3 here; B * C <= 2^24) and corruptions
        n = 3 * px
        assert lib.r2l_aux_workspace_bytes(B, 3, H, W) == al(4 * 2048) + 12 * n, (B, H, W)
        _strictly_increasing(lib.r2l_aux_workspace_bytes, B, 3, H, W)
        for kind in range(10):
            want = al(12 * B) if kind == 7 else 0                                      # contrast: a mean per image and channel
            assert lib.r2l_corrupt_workspace_bytes(kind, B, 3, H, W) == want, (kind, B)
    # above 2^32 bytes / 2^31 elements on every shape the GPU cases cross a line with
    assert lib.r2l_isp_workspace_bytes(2732, 512, 512) > 2 ** 32 and 2732 * 3 * 512 * 512 >= 2 ** 31 > 2728 * 3 * 512 * 512
    assert 2052 * 1024 * 1024 >= 2 ** 31 > 2048 * 1024 * 1024 - 1 and 10924 * 3 * 256 * 256 >= 2 ** 31 > 10920 * 3 * 256 * 256
    assert 176 * 1024 * 1024 * 3 * 8 >= 2 ** 32 > 172 * 1024 * 1024 * 3 * 8 - 2 ** 27 and 1368 * 3 * 512 * 512 * 4 >= 2 ** 32 > 1364 * 3 * 512 * 512 * 4


# ---- the refusals at the documented limits ----------------------------------------------------------------------------------
def test_refusals_at_the_documented_limits():
    """tests/emul/r2l_limits_lockstep.cpp (tests/lockstep_driver.py: the lock-step emulation's sources -- the device's host route
    -- + a main under -fsanitize=address,undefined, no Python in the process).  Each call names a shape past a limit and hands over
    buffers of a few bytes: it must come back with the documented code and text before any launch could use the shape"""
    env = {k: v for k, v in os.environ.items() if not k.startswith('R2L_')}
    r = lockstep_driver.run('limits', env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    got = dict(line.split(' -> ', 1) for line in r.stdout.splitlines())
    frame, batch, many = 'frame 2^29 + 2 * 2048 px', 'batch 4097x16384x16384', '2^30 + 2 frames of 4x4'
    want = {}
    for call in ('step_fwd', 'step_bwd', 'static_fwd'):
        want[f'{call} {frame}'] = '-1 [frames above 2^29 pixels are not supported]'
        want[f'{call} {batch}'] = '-1 [batch too large]'
    want['step_fwd frame 2^29 px, workspace of 0 bytes'] = '-2 [r2l_isp_step_fwd: workspace too small (r2l_isp_workspace_bytes)]'
    want['static_fwd frame 2^29 px (Menon2007), workspace of 0 bytes'] = \
        '-2 [r2l_static_fwd: workspace too small (r2l_static_workspace_bytes)]'
    for bn in ('bn none', 'bn train', 'bn eval'):
        want[f'step_fwd {many}, {bn}'] = '-1 [r2l_isp_fwd: batch too large]'
        want[f'step_bwd {many}, {bn}'] = '-1 [r2l_isp_step_bwd: batch too large]'
    for chain in ('000', '011'):
        want[f'static_fwd {many}, chain {chain}'] = '-1 [r2l_static_fwd: batch too large]'
    assert got == want, '\n'.join(f'{k}: got {got.get(k)!r}, want {want.get(k)!r}' for k in sorted(set(got) | set(want))
                                  if got.get(k) != want.get(k))


def test_query_shapes_cover_the_lines_the_issue_names():
    shapes = set(lc.QUERY_SHAPES)
    assert {(2732, 512, 512), (10924, 256, 256), (2052, 1024, 1024), (176, 1024, 1024), (1368, 512, 512), (1, 262144, 2048)} <= shapes
    assert np.prod((1, 262144, 2048), dtype=np.int64) == 2 ** 29
