"""Checks of the kernels past 2^31 elements, past 2^32 bytes inside one buffer and at the 2^29-pixel frame limit
(tests/test_gpu_large_index.py on the gfx950 build; the comparison logic and the closed forms of the size queries also in
tests/test_large_index.py, without a GPU).

A float64 oracle over 7e8 pixels is not affordable, so every large case is built to be checkable:

  * PERIODIC BATCHES.  The input is a block of BB = 4 frames repeated R times (Tensor.repeat on the device), the cotangent likewise.
    Frames are independent, so every block of the output -- and of d/d raw, in float32, 16 bits, planar or channels-last -- must
    equal block 0 BIT FOR BIT (`first_mismatch`, on the device, in chunks of at most 1 GiB); train-mode BatchNorm included: the
    batch statistics of R repeats are the block's.
  * BLOCK 0 AGAINST THE ORACLE at the limits the small-shape suites use (block 0 lies at low addresses, where they vouch for the
    kernels): parity_checks.out_tolerance / DEFAULT_GRAD_RTOL for the step, 1e-5 for the static chains, plus one unit in the last
    place of a 16-bit output type.
  * SUMS.  The 132 parameter gradients are R x the oracle's for the block; BatchNorm's running_var takes its unbiased factor from
    the full pixel count.
  * NOTHING LEFT UNWRITTEN, NOTHING WRITTEN OUTSIDE.  The call runs inside guarded_arena.guarded(..., 'nan'): an element the
    kernels skipped is NaN afterwards, and the guard zones are compared zone by zone (`check_guard_zones`; Arena.check_guards
    clones the whole arena, which a 30 GB footprint cannot afford).

No large tensor crosses to the host: block 0 (<= 50 MB) and 64 Ki-element windows do."""
import contextlib
import functools
import gc
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import guarded_arena as ga  # noqa: E402
import half_io_checks as hc  # noqa: E402
import parity_checks as pc  # noqa: E402
import raw_grad_checks as rc  # noqa: E402
from oracle import isp_oracle as orc  # noqa: E402

GIB = 1 << 30
CHUNK = 1 << 30             # bytes compared per device operation
BB = 4                      # frames of the repeated block
MAX_NEED = 48 * GIB
WINDOW = 64 * 1024          # elements of a window of the flat kernels
_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
CL = torch.channels_last


# ------------------------------------------------------------------------------------------------------------------------
# memory
# ------------------------------------------------------------------------------------------------------------------------
def need_or_skip(nbytes, device):
    """the test's need in bytes, computed up front: skips only where the device reports less free memory than that"""
    import pytest
    assert nbytes <= MAX_NEED, f'a case may need at most 48 GiB, this one {nbytes / GIB:.1f}'
    release()
    free = torch.cuda.mem_get_info(device)[0]
    if free < nbytes:
        pytest.skip(f'needs {nbytes / GIB:.1f} GiB, {free / GIB:.1f} free')


def release():
    gc.collect()
    if torch.cuda.is_available():
        torch.cuda.empty_cache()


def arena_bytes(*payloads):
    """an arena that holds these payloads (bytes each) between their guard zones"""
    return sum(ga._align(int(n)) + ga.GUARD + 256 for n in payloads) + ga.GUARD + 4096


@contextlib.contextmanager
def guarded(device, nbytes):
    """guarded_arena.guarded(device, nbytes, 'nan') that also serves torch.empty(..., memory_format=torch.channels_last): the
    arena's own entry point hands out planar strides whatever the format asked for, so a channels-last output would be stored
    into a planar tensor.  Here it is a (B,H,W,C) payload seen as (B,C,H,W)"""
    with ga.guarded(device, nbytes, 'nan') as arena:
        inner = torch.empty

        def empty(*size, memory_format=None, **kw):
            dev = kw.get('device')
            if memory_format is CL and dev is not None and torch.device(dev).type == arena.device.type:
                shape = tuple(size[0]) if len(size) == 1 and not isinstance(size[0], int) else tuple(size)
                B, C, H, W = shape
                return arena.alloc((B, H, W, C), kw.get('dtype') or torch.get_default_dtype(), 'channels-last').permute(0, 3, 1, 2)
            if memory_format is None:
                return inner(*size, **kw)
            return inner(*size, memory_format=memory_format, **kw)
        torch.empty = empty
        try:
            yield arena
        finally:
            torch.empty = inner


# ------------------------------------------------------------------------------------------------------------------------
# comparisons on the device, in chunks
# ------------------------------------------------------------------------------------------------------------------------
def memory_order(t):
    """the elements of a planar-contiguous or channels-last tensor as a flat view in memory order (no copy)"""
    if t.is_contiguous():
        return t.reshape(-1)
    if t.dim() == 4 and t.is_contiguous(memory_format=CL):
        return t.permute(0, 2, 3, 1).reshape(-1)
    raise ValueError(f'neither planar-contiguous nor channels-last: shape {tuple(t.shape)}, strides {t.stride()}')


def bits(t):
    """memory_order(t) as integers of the element size: a bitwise comparison, NaN == NaN"""
    return memory_order(t).view(_INT[t.element_size()])


def first_mismatch(flat, period, first=0, count=None, chunk_bytes=CHUNK):
    """flat: a 1-D tensor of whole periods of `period` elements.  Periods first + 1 .. first + count - 1 against period `first`,
    element for element, at most chunk_bytes per device operation.  -> None, or the FIRST differing period:
    dict(block=its index, offset=the flat index of its first differing element, differing=how many of its elements differ)"""
    assert flat.dim() == 1 and flat.numel() % period == 0, (tuple(flat.shape), period)
    n = flat.numel() // period
    count = n - first if count is None else count
    assert 0 <= first and first + count <= n
    ref = flat[first * period:(first + 1) * period]
    step = max(1, chunk_bytes // (period * flat.element_size()))
    for b0 in range(first + 1, first + count, step):
        b1 = min(b0 + step, first + count)
        ne = flat[b0 * period:b1 * period].view(b1 - b0, period) != ref
        bad = ne.any(dim=1)
        if bool(bad.any()):
            k = int(torch.nonzero(bad)[0])
            j = int(torch.nonzero(ne[k])[0])
            return dict(block=b0 + k, offset=(b0 + k) * period + j, differing=int(ne[k].sum()))
    return None


def assert_periodic(t, nblocks, what):
    """every one of the nblocks equal parts of t (in memory order) equals part 0 bit for bit"""
    flat = bits(t)
    assert flat.numel() % nblocks == 0
    bad = first_mismatch(flat, flat.numel() // nblocks)
    pc.report(f'{what}: blocks 1 .. {nblocks - 1} vs block 0 (bitwise; differing elements of the first bad block)',
              0 if bad is None else bad['differing'], 0.0)
    assert bad is None, f'{what}: block {bad["block"]} of {nblocks} differs from block 0, first at flat element {bad["offset"]} ' \
                        f'({bad["differing"]} elements of that block differ)'


def count_nan(t, chunk_bytes=CHUNK):
    flat = memory_order(t)
    step = chunk_bytes // t.element_size()
    return sum(int(torch.isnan(flat[a:a + step]).sum()) for a in range(0, flat.numel(), step))


def assert_no_nan(t, what):
    n = count_nan(t)
    assert n == 0, f'{what}: {n} of {t.numel()} elements are NaN (the poison: the kernels left them unwritten)'


def check_guard_zones(arena, what, chunk_bytes=CHUNK):
    """every byte of the arena outside its payloads still holds the poison; one zone (and at most chunk_bytes of it) at a time"""
    if arena.device.type == 'cuda':
        torch.cuda.synchronize(arena.device)
    buf = arena.buf
    pat = torch.tensor(list(int(arena.pattern).to_bytes(4, 'little')), dtype=torch.uint8, device=buf.device)
    want = int(np.array(arena.pattern, dtype=np.uint32).view(np.int32))
    edges = [0] + [x for s, e, _ in arena.blocks for x in (s, e)] + [arena.nbytes]

    def fail(off):
        near = min(arena.blocks, key=lambda b: min(abs(off - b[0]), abs(off - b[1])))
        raise AssertionError(f'{what}: guard byte {off} overwritten; nearest payload {near[2]} = [{near[0]}, {near[1]}): '
                             f'{off - near[1]} bytes past its end / {near[0] - off} bytes before its start')

    def bytewise(a, b):
        if a < b:
            ne = buf[a:b] != pat[torch.arange(a, b, device=buf.device) % 4]
            if bool(ne.any()):
                fail(a + int(torch.nonzero(ne)[0]))
    for i in range(0, len(edges), 2):
        a, b = edges[i], edges[i + 1]
        a4, b4 = min(b, (a + 3) // 4 * 4), max(a, b // 4 * 4)
        if a4 >= b4:
            bytewise(a, b)
            continue
        bytewise(a, a4)
        bytewise(b4, b)
        for c0 in range(a4, b4, chunk_bytes):
            c1 = min(b4, c0 + chunk_bytes)
            ne = buf[c0:c1].view(torch.int32) != want
            if bool(ne.any()):
                w = c0 + 4 * int(torch.nonzero(ne)[0])
                bytewise(w, w + 4)
    return len(edges) // 2


# ------------------------------------------------------------------------------------------------------------------------
# the fused step on a periodic batch
# ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def step_oracle(H, W, bn, training, u16, dtype, backward, raw_grad):
    """the float64 oracle of the block: (raw block as the kernels get it, cotangent block as planar float32 values, dict of
    references).  Computed once per configuration, read-only afterwards"""
    raw = orc.synth_raw(BB, H, W, seed=17, kind='scene')
    if u16:
        codes = np.round(raw * 65535.0).astype(np.uint16)
        raw_in, raw = codes.view(np.int16), (codes.astype(np.float32) / np.float32(65535.0))
    else:
        raw_in = raw
    cot = np.random.default_rng(1017).standard_normal((BB, 3, H, W)).astype(np.float32)
    if dtype is not torch.float32:
        cot = torch.from_numpy(cot).to(dtype).float().numpy()       # the values a cotangent of that type holds
    P64 = orc.IspParams(orc.DRONE_CAMERA_PARAMS, dtype=np.float64)
    out, _, cache = orc.parametrized_forward(raw, P64, bn=rc.bn_arg(bn, training))
    ref = dict(out=out, tol=pc.out_tolerance(cache, bn) + (0.0 if dtype is torch.float32 else hc.ulp16(out, dtype)))
    if bn and training:
        x = cache['pre_bn'].astype(np.float64)
        ref['mean'], ref['var'] = x.mean(axis=(0, 2, 3)), x.var(axis=(0, 2, 3))
    if backward:
        nom, lo, hi = (orc.parametrized_backward(P64, cache, cot, **kw)[:2]
                       for kw in ({}, dict(clip_shift=1e-6), dict(clip_shift=-1e-6)))
        ref['grads'] = {k: (np.asarray(nom[0][k]), max(np.abs(np.asarray(lo[0][k]) - nom[0][k]).max(),
                                                       np.abs(np.asarray(hi[0][k]) - nom[0][k]).max()))
                        for k in nom[0] if k != 'additive_layer'}
        if raw_grad:
            ref['grad_raw'] = nom[1]
            ref['grad_raw_lim'] = rc._limit(nom[1], lo[1], hi[1], nom[1], pc.DEFAULT_GRAD_RTOL)
    for v in (raw_in, cot):
        v.setflags(write=False)
    return raw_in, cot, ref


def step_need(lib, B, H, W, dtype, backward, raw_grad, u16):
    """bytes the step case holds on the device at its peak"""
    px, es = B * H * W, torch.empty((), dtype=dtype).element_size()
    io = 3 * px * es
    n = px * (2 if u16 else 4) + io + lib.r2l_isp_workspace_bytes(B, H, W)
    if backward:
        n += io
    if raw_grad:
        n += 4 * px + lib.r2l_isp_raw_grad_scratch_bytes(B, H, W)
    return n + 3 * GIB       # comparison chunks and their masks, block 0 on the host's way, the allocator's slack


def check_step_case(device, R, H, W, bn, training, dtype=torch.float32, channels_last=False, u16=False, raw_grad=False,
                    backward=True):
    """one fused step (forward, and backward unless backward=False) on BB * R frames of H x W inside the NaN-poisoned arena"""
    from raw2logit_amd import _lib
    B = BB * R
    what = f'large step {B}x{H}x{W} bn={bn} train={training} {str(dtype)[6:]}{" nhwc" if channels_last else ""}' \
           f'{" u16" if u16 else ""}{" d/draw" if raw_grad else ""}'
    lib = _lib.device_library()
    need = step_need(lib, B, H, W, dtype, backward, raw_grad, u16)
    need_or_skip(need, device)
    raw_b, cot_b, ref = step_oracle(H, W, bn, training, u16, dtype, backward, raw_grad)
    raw = torch.tensor(raw_b).to(device).repeat(R, 1, 1)
    assert raw.shape[0] * 3 * H * W >= 2 ** 31 or H * W >= 2 ** 29 - 2 ** 20, what
    cot = None
    if backward:
        c = torch.tensor(cot_b).to(device).to(dtype)
        cot = c.permute(0, 2, 3, 1).contiguous().repeat(R, 1, 1, 1).permute(0, 3, 1, 2) if channels_last else c.repeat(R, 1, 1, 1)
        assert cot.is_contiguous(memory_format=CL) if channels_last else cot.is_contiguous()
        del c
    m = rc.make_plain_module(bn, device, training)
    m.output_dtype = None if dtype is torch.float32 else dtype
    m.output_memory_format = CL if channels_last else None
    if raw_grad:
        raw.requires_grad_(True)
    try:
        with guarded(device, need - 2 * GIB - raw.numel() * raw.element_size() - (cot.numel() * cot.element_size() if backward else 0)) \
                as arena, torch.set_grad_enabled(backward):
            y = m(raw)
            from raw2logit_amd.processing import pipeline_torch as ppt
            assert isinstance(m.stages, ppt._LazyStages), 'the call took the stage-by-stage kernels'
            assert y.dtype == dtype and (y.is_contiguous(memory_format=CL) if channels_last else y.is_contiguous())
            if backward:
                y.backward(cot)
            torch.cuda.synchronize()
            y = y.detach()
            n_zones = check_guard_zones(arena, what)
            assert n_zones >= 3, (what, arena.blocks)     # the output and the workspace at least came out of the arena
            lo, hi = arena.buf.data_ptr(), arena.buf.data_ptr() + arena.nbytes
            assert lo <= y.data_ptr() < hi, 'the output is not an arena payload'
            # 4: nothing left unwritten
            assert_no_nan(y, what + '/out')
            # 1: every block equals block 0
            assert_periodic(y, R, what + '/out')
            graw = raw.grad if raw_grad else None
            if raw_grad:
                assert lo <= graw.data_ptr() < hi, 'grad_raw is not an arena payload'
                assert_no_nan(graw, what + '/grad_raw')
                assert_periodic(graw, R, what + '/grad_raw')
            # 2: block 0 against the float64 oracle
            y0 = y[:BB].float().cpu().numpy().astype(np.float64)
            err = np.abs(y0 - ref['out'])
            worst = np.unravel_index((err / ref['tol']).argmax(), err.shape)
            pc.report(f'{what}/out block 0 vs float64 oracle', err[worst], ref['tol'][worst])
            assert np.all(err <= ref['tol']), (what, 'out', worst, float(err[worst]), float(ref['tol'][worst]))
            if raw_grad:
                e = np.abs(graw[:BB].cpu().numpy() - ref['grad_raw'])
                pc.report(f'{what}/grad_raw block 0 vs float64 oracle', e.max(), float(np.min(ref['grad_raw_lim'])))
                assert np.all(e <= ref['grad_raw_lim']), (what, 'grad_raw', float(e.max()))
            # 3: the sums
            failed = []
            if backward:
                grads = hc.grads_of(m)
                assert len(grads) == 7 and sum(v.size for v in grads.values()) == _lib.R2L_P_NTRAIN
                for k, (og, flip) in ref['grads'].items():
                    want = R * og
                    lim = pc.DEFAULT_GRAD_RTOL * (np.abs(want).max() + 1e-6) + R * flip
                    e = np.abs(grads[k].reshape(og.shape).astype(np.float64) - want).max()
                    pc.report(f'{what}/grad {k} vs {R} x float64 oracle of the block', e, lim)
                    if not (np.isfinite(grads[k]).all() and e <= lim):
                        failed.append((k, float(e), float(lim)))
            if bn and training:
                b, n = m.batch_norm, B * H * W
                want_m = 0.1 * ref['mean']
                want_v = 0.9 + 0.1 * ref['var'] * n / (n - 1)
                for name, got, want in (('running_mean', b.running_mean, want_m), ('running_var', b.running_var, want_v)):
                    got = got.cpu().numpy().astype(np.float64)
                    e = np.abs(got - want)
                    lim = 1e-6 + 1e-5 * np.abs(want)            # (parity_checks.check_param_case: rtol 1e-5, atol 1e-6)
                    i = int((e / lim).argmax())
                    pc.report(f'{what}/{name} vs the oracle (unbiased factor of {n} px)', e[i], lim[i])
                    if not np.all(e <= lim):
                        failed.append((name, float(e[i]), float(lim[i])))
                assert int(b.num_batches_tracked) == 1
            assert not failed, (what, 'sums over the batch (name, error, limit)', failed)
    finally:
        m.__dict__['buffer'] = m.__dict__['stages'] = None
        raw.grad = None
        del m, raw, cot
        y = graw = arena = None
        release()


# ------------------------------------------------------------------------------------------------------------------------
# static chains on a periodic batch
# ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def static_oracle(H, W, chain, options, u16, frames):
    """(raw block as the kernels get it, {frame of the block: float64-accurate output (3,H,W)})"""
    raw = orc.synth_raw(BB, H, W, seed=23, kind='scene')
    if u16:
        codes = np.round(raw * 65535.0).astype(np.uint16)
        raw_in, raw = codes.view(np.int16), (codes.astype(np.float32) / np.float32(65535.0))
    else:
        raw_in = raw
    out = {f: orc.static_batch(raw[f:f + 1], orc.DRONE_CAMERA_PARAMS, *chain, **dict(options))[0] for f in frames}
    raw_in.setflags(write=False)
    return raw_in, out


def static_need(lib, B, H, W, chain, options, dtype, u16):
    from raw2logit_amd import functional as F_
    import ctypes
    o = {**F_.STATIC_OPTION_DEFAULTS, **dict(options)}
    ov = (ctypes.c_double * 5)(*[float(o[k]) for k in ('sharp_radius', 'sharp_amount', 'gaussian_sigma', 'fft_fraction',
                                                      'median_kernel_size')])
    codes = (F_._DEBAYER[chain[0]], F_._SHARPEN.get(chain[1], 0), F_._DENOISE.get(chain[2], 0))
    nws = 0 if dtype is not torch.float32 else lib.r2l_static_workspace_bytes_opts(1 if u16 else 0, B, H, W, *codes, ov)
    px = B * H * W
    return px * (2 if u16 else 4) + 3 * px * torch.empty((), dtype=dtype).element_size() + nws + 3 * GIB, nws


def check_static_case(device, R, H, W, chain, options=(), dtype=torch.float32, u16=False, frames=tuple(range(BB)),
                      workspace_per_px=None, kernel=None):
    """one static chain on BB * R frames inside the NaN-poisoned arena.  frames: the frames of block 0 held to the oracle (the
    rest of the batch by periodicity).  16-bit output: only where the kernels write it themselves (r2l_static_fwd_io)"""
    from raw2logit_amd import _lib
    from raw2logit_amd import functional as F_
    B = BB * R
    what = f'large static {"/".join(chain)}{dict(options) or ""} {B}x{H}x{W}{" u16" if u16 else ""} -> {str(dtype)[6:]}'
    lib = _lib.device_library()
    need, nws = static_need(lib, B, H, W, chain, options, dtype, u16)
    if workspace_per_px is not None:
        assert nws // (B * H * W) == workspace_per_px, (what, nws, workspace_per_px)
    need_or_skip(need, device)
    raw_b, ref = static_oracle(H, W, chain, tuple(options), u16, tuple(frames))
    raw = torch.tensor(raw_b).to(device).repeat(R, 1, 1)
    try:
        if dtype is not torch.float32:
            assert F_.static_io_why(raw, *chain, **dict(options)) is None
        with guarded(device, need - 2 * GIB - raw.numel() * raw.element_size()) as arena:
            y, names = pc.kernels_launched(lib, lambda: F_.static_pipeline(raw, orc.DRONE_CAMERA_PARAMS, *chain, out_dtype=dtype,
                                                                           **dict(options)))
            if kernel is not None:
                assert any(kernel in k for k in names), (what, names)
            n_zones = check_guard_zones(arena, what)
            assert n_zones >= (3 if nws else 2) and arena.buf.data_ptr() <= y.data_ptr() < arena.buf.data_ptr() + arena.nbytes
            assert y.dtype == dtype and y.is_contiguous()
            assert_no_nan(y, what + '/out')
            assert_periodic(y, R, what + '/out')
            for f in frames:
                o = ref[f].astype(np.float64)
                tol = 1e-5 + (0.0 if dtype is torch.float32 else hc.ulp16(o, dtype))
                for b in sorted({f, (R // 2) * BB + f, (R - 1) * BB + f}):      # (the copies are block 0's by periodicity: free)
                    err = np.abs(y[b].float().cpu().numpy().astype(np.float64) - o)
                    worst = np.unravel_index((err / tol).argmax(), err.shape)
                    pc.report(f'{what}/frame {b} vs float64 oracle', err[worst], np.broadcast_to(tol, err.shape)[worst])
                    assert np.all(err <= tol), (what, b, worst, float(err[worst]))
    finally:
        del raw
        y = arena = None
        release()


# ------------------------------------------------------------------------------------------------------------------------
# one frame at the 2^29-pixel limit: content periodic in y with a period of 64 rows
# ------------------------------------------------------------------------------------------------------------------------
PERIOD_ROWS = 64


def tall_frame(H, W, device):
    """(the (1,H,W) frame: a 64-row tile repeated H / 64 times, the 192-row frame with the same top and bottom rows)"""
    assert H % PERIOD_ROWS == 0 and H >= 3 * PERIOD_ROWS
    tile = orc.synth_raw(1, PERIOD_ROWS, W, seed=29, kind='scene')
    return torch.from_numpy(tile).to(device).repeat(1, H // PERIOD_ROWS, 1), np.tile(tile, (1, 3, 1))


def check_tall_output(y, small, tol, what):
    """y (1,3,H,W) on the device, small (1,3,192,W) float64 oracle of the 192-row frame: every 64-row period from row 64 to row
    H - 64 equals the first interior one bit for bit; the top and the bottom 64 rows against the oracle's"""
    _, C, H, W = y.shape
    assert y.is_contiguous()
    assert_no_nan(y, what)
    per = PERIOD_ROWS * W
    worst = None
    for c in range(C):
        bad = first_mismatch(bits(y[0, c]), per, first=1, count=H // PERIOD_ROWS - 2)
        if bad is not None and worst is None:
            worst = (c, bad)
    pc.report(f'{what}: interior 64-row periods vs the first interior one (bitwise; differing elements of the first bad one)',
              0 if worst is None else worst[1]['differing'], 0.0)
    assert worst is None, f'{what}: channel {worst[0]}, period {worst[1]["block"]} (rows from {worst[1]["block"] * PERIOD_ROWS}) ' \
                          f'differs, first at plane element {worst[1]["offset"]}'
    tol = np.broadcast_to(tol, small.shape)
    for name, got, sl in (('top', y[:, :, :PERIOD_ROWS], slice(0, PERIOD_ROWS)),
                          ('first interior period', y[:, :, PERIOD_ROWS:2 * PERIOD_ROWS], slice(PERIOD_ROWS, 2 * PERIOD_ROWS)),
                          ('bottom', y[:, :, H - PERIOD_ROWS:], slice(2 * PERIOD_ROWS, 3 * PERIOD_ROWS))):
        err = np.abs(got.float().cpu().numpy().astype(np.float64) - small[:, :, sl])
        t = tol[:, :, sl]
        w = np.unravel_index((err / t).argmax(), err.shape)
        pc.report(f'{what}: {name} 64 rows vs float64 oracle of the 192-row frame', err[w], t[w])
        assert np.all(err <= t), (what, name, w, float(err[w]), float(t[w]))


def check_tall_static(device, H, W, chain):
    from raw2logit_amd import functional as F_
    need = H * W * 16 + 3 * GIB
    need_or_skip(need, device)
    what = f'large frame static {"/".join(chain)} 1x{H}x{W}'
    raw, small = tall_frame(H, W, device)
    try:
        with guarded(device, arena_bytes(12 * H * W)) as arena:
            y = F_.static_pipeline(raw, orc.DRONE_CAMERA_PARAMS, *chain)
            assert check_guard_zones(arena, what) >= 2
            check_tall_output(y, orc.static_batch(small, orc.DRONE_CAMERA_PARAMS, *chain).astype(np.float64), 1e-5, what)
    finally:
        del raw
        y = arena = None
        release()


def check_tall_step_forward(device, H, W):
    """the step's forward with eval-mode BatchNorm on one H x W frame (no backward follows: torch.no_grad)"""
    from raw2logit_amd import _lib
    lib = _lib.device_library()
    nws = lib.r2l_isp_workspace_bytes(1, H, W)
    need = H * W * 16 + nws + 3 * GIB
    need_or_skip(need, device)
    what = f'large frame step forward bn eval 1x{H}x{W}'
    raw, small = tall_frame(H, W, device)
    m = rc.make_plain_module(True, device, False)
    try:
        with guarded(device, arena_bytes(12 * H * W, nws)) as arena, torch.no_grad():
            y = m(raw)
            torch.cuda.synchronize()
            assert check_guard_zones(arena, what) >= 3
            P64 = orc.IspParams(orc.DRONE_CAMERA_PARAMS, dtype=np.float64)
            o, _, cache = orc.parametrized_forward(small, P64, bn=rc.bn_arg(True, False))
            check_tall_output(y, o, pc.out_tolerance(cache, True), what)
    finally:
        m.__dict__['buffer'] = m.__dict__['stages'] = None
        del m, raw
        y = arena = None
        release()


# ------------------------------------------------------------------------------------------------------------------------
# flat kernels: windows of 64 Ki elements at the start, straddling element 2^31, and at the end
# ------------------------------------------------------------------------------------------------------------------------
def windows(n):
    return [(0, WINDOW), (2 ** 31 - WINDOW // 2, 2 ** 31 + WINDOW // 2), (n - WINDOW, n)]


# ------------------------------------------------------------------------------------------------------------------------
# closed forms of the size queries (pure host functions)
# ------------------------------------------------------------------------------------------------------------------------
def align256(x):
    return (x + 255) // 256 * 256


# (B, H, W): the GPU cases' shapes, frames of 2^29 px, batches of 2^40 px
QUERY_SHAPES = [(2732, 512, 512), (10924, 256, 256), (2052, 1024, 1024), (176, 1024, 1024), (1368, 512, 512),
                (1, 262144, 2048), (1, 32768, 16384), (2048, 262144, 2048), (4096, 16384, 16384), (2 ** 22, 512, 512)]
STEP_SLOTS = dict(STATS=0, MOMENTS=1, BN_SUMS=2, PACKED=3, BN=4, LUMA=5)      # R2L_STEP_* of include/r2l_isp.h


def philox_window(start, count, seed, offset=0):
    """orc.philox_normal restated for the elements start .. start + count - 1 (start and count multiples of 4: whole groups)"""
    assert start % 4 == 0 and count % 4 == 0
    g = np.arange(start // 4, (start + count) // 4, dtype=np.uint64)
    c = np.stack([g & np.uint64(0xFFFFFFFF), g >> np.uint64(32),
                  np.full_like(g, int(offset) & 0xFFFFFFFF), np.full_like(g, (int(offset) >> 32) & 0xFFFFFFFF)], axis=1)
    o = orc.philox4x32_10(c, (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF))
    s = np.float32(2.3283064365386963e-10)
    out = np.empty((len(g), 4), dtype=np.float32)
    for h in (0, 1):
        u1 = (o[:, 2 * h].astype(np.float32) + np.float32(1)) * s
        u2 = o[:, 2 * h + 1].astype(np.float32) * s
        r = np.sqrt(np.float32(-2) * np.log(u1))
        t = np.float32(6.2831853071795865) * u2
        out[:, 2 * h] = r * np.cos(t)
        out[:, 2 * h + 1] = r * np.sin(t)
    return out.reshape(-1)


FLAT_R, FLAT_H, FLAT_W = 683, 512, 512           # (2732,3,512,512): 2 148 532 224 elements
FLAT_N = BB * FLAT_R * 3 * FLAT_H * FLAT_W
PHILOX_ATOL = 2e-6                               # parity_checks.check_augmentation's limit on x + std * deviate


@functools.lru_cache(maxsize=2)
def flat_block(seed, lo=0.0, hi=1.0):
    x = (np.random.default_rng(seed).random((BB, 3, FLAT_H, FLAT_W), dtype=np.float32) * np.float32(hi - lo) + np.float32(lo))
    x.setflags(write=False)
    return x


def flat_input(device, seed, lo=0.0, hi=1.0):
    assert FLAT_N >= 2 ** 31 > FLAT_N - BB * 3 * FLAT_H * FLAT_W
    return torch.tensor(flat_block(seed, lo, hi)).to(device).repeat(FLAT_R, 1, 1, 1)


def check_windows(what, got, want_of, atol, n=None):
    """got: a device tensor of n elements in memory order; want_of(a, b) -> float64 values of elements a .. b - 1"""
    flat = memory_order(got)
    n = flat.numel() if n is None else n
    for a, b in windows(n):
        e = np.abs(flat[a:b].cpu().numpy().astype(np.float64) - want_of(a, b))
        pc.report(f'{what}: elements {a} .. {b - 1} vs the oracle', e.max(), atol)
        assert e.max() <= atol, (what, a, int(e.argmax()) + a, float(e.max()))


def check_flat_philox_noise(device):
    """r2l_add_noise_philox on 2^31 + elements: the deviate of element e is the oracle's, in windows; every element written"""
    from raw2logit_amd import augmentation as A
    need_or_skip(2 * 4 * FLAT_N + 3 * GIB, device)
    what, seed, off, std = f'large add_noise_philox n={FLAT_N}', 2 ** 61 + 7, 5, 0.25
    x = flat_input(device, 41, -1.0, 1.0)
    try:
        with guarded(device, arena_bytes(4 * FLAT_N)) as arena:
            y = A.add_gaussian_noise(x, std, seed, off)
            assert check_guard_zones(arena, what) == 2
            assert_no_nan(y, what)
            xf = memory_order(x)
            check_windows(what, y, lambda a, b: (xf[a:b].cpu().numpy() + np.float32(std) * philox_window(a, b - a, seed, off)
                                                 ).astype(np.float64), PHILOX_ATOL)
    finally:
        del x
        y = xf = arena = None
        release()


def check_flat_corrupt(device, transform, severity=3):
    """r2l_corrupt on (2732,3,512,512).  An elementwise transform is periodic with its input: every block equals block 0, block 0
    against the float64 oracle at corruption_checks.ATOL.  A Philox transform draws per flat element: windows"""
    import corruption_checks as cck
    import corruption_oracle as co
    from raw2logit_amd import corruptions as C
    need_or_skip(2 * 4 * FLAT_N + 3 * GIB, device)
    what = f'large corrupt {transform} s{severity} ({BB * FLAT_R},3,{FLAT_H},{FLAT_W})'
    x = flat_input(device, 43, -0.1, 1.1)
    try:
        nws = C._lib.device_library().r2l_corrupt_workspace_bytes(C.KINDS[transform], BB * FLAT_R, 3, FLAT_H, FLAT_W)
        with guarded(device, arena_bytes(4 * FLAT_N, nws)) as arena:
            y = C.corrupt(x, transform, severity, key=cck.KEY)
            assert check_guard_zones(arena, what) == (3 if nws else 2)
            assert_no_nan(y, what)
            if transform in C.RANDOM:
                assert transform == 'gaussian_noise'
                c, xf = np.float32(C.SEVERITY[transform][severity - 1]), memory_order(x)
                check_windows(what, y, lambda a, b: np.clip(xf[a:b].cpu().numpy() + c * philox_window(a, b - a, cck.KEY), 0, 1
                                                            ).astype(np.float64), PHILOX_ATOL)
            else:
                assert_periodic(y, FLAT_R, what)
                e = np.abs(y[:BB].cpu().numpy().astype(np.float64) - co.apply(flat_block(43, -0.1, 1.1), transform, severity)).max()
                pc.report(f'{what}: block 0 vs float64 oracle', e, cck.ATOL)
                assert e <= cck.ATOL, (what, e)
    finally:
        del x
        y = xf = arena = None
        release()


def check_flat_flip_rot(device, hflip, vflip, k):
    """r2l_augment forward and inverse (its VJP) on (2732,3,512,512): periodic, block 0 equal to the torch ops the reference composes"""
    from raw2logit_amd import augmentation as A
    need_or_skip(3 * 4 * FLAT_N + 3 * GIB, device)
    what = f'large r2l_augment hflip={hflip} vflip={vflip} k={k} ({BB * FLAT_R},3,{FLAT_H},{FLAT_W})'
    x = flat_input(device, 47).requires_grad_(True)

    def ops(t, inverse=False):
        if inverse:
            t = t.rot90(-k, dims=(-1, -2))
            t = t.flip(-2) if vflip else t
            return t.flip(-1) if hflip else t
        t = t.flip(-1) if hflip else t
        t = t.flip(-2) if vflip else t
        return t.rot90(k, dims=(-1, -2))
    try:
        with guarded(device, arena_bytes(4 * FLAT_N, 4 * FLAT_N)) as arena:
            y = A.flip_rot(x, hflip, vflip, k)
            y.backward(x.detach())                 # (the cotangent: the input itself, periodic and known)
            y = y.detach()
            assert check_guard_zones(arena, what) == 3
            for name, t, inv in (('out', y, False), ('vjp', x.grad, True)):
                assert_no_nan(t, f'{what}/{name}')
                assert_periodic(t, FLAT_R, f'{what}/{name}')
                same = torch.equal(t[:BB], ops(x.detach()[:BB], inv))
                pc.report(f'{what}/{name}: block 0 vs torch flip / rot90 (bitwise)', 0 if same else 1, 0.0)
                assert same, (what, name)
    finally:
        x.grad = None
        del x
        y = arena = t = None
        release()


def check_flat_l2(device):
    """r2l_l2_fwd / r2l_l2_bwd on 2^31 + elements: the gradient periodic and, on block 0, the float32 formula bit for bit; the sum
    R x the block's float64 sum within aux_checks.l2_sum_bound (a rounding count, capped by the project's 2e-6)"""
    import aux_checks as ac
    from raw2logit_amd import _lib
    from raw2logit_amd._lib import ptr
    need_or_skip(3 * 4 * FLAT_N + 3 * GIB, device)
    per = FLAT_N // FLAT_R
    xb, yb = ac._l2_inputs(per)
    gup = np.float32(0.7)
    want = (np.float32(-2.0) * (xb - yb)) * gup
    ref_sum = FLAT_R * float(np.square(xb.astype(np.float64) - yb.astype(np.float64)).sum())
    what = f'large l2 n={FLAT_N}'
    x, y = (torch.from_numpy(a).to(device).repeat(FLAT_R) for a in (xb, yb))
    try:
        lib, stream = _lib.library_for(x)
        nws = lib.r2l_aux_workspace_bytes(1, 1, 2, 2)
        with guarded(device, arena_bytes(4 * FLAT_N, nws, 8)) as arena:
            grad = torch.empty_like(y)
            ws = torch.empty(nws, dtype=torch.uint8, device=device)
            out = torch.empty(1, dtype=torch.float64, device=device)
            g_t = torch.full((1,), float(gup), dtype=torch.float32, device=device)
            lib.check(lib.r2l_l2_fwd(ptr(x), ptr(y), ptr(out), ptr(ws), nws, FLAT_N, stream), 'r2l_l2_fwd')
            lib.check(lib.r2l_l2_bwd(ptr(x), ptr(y), ptr(g_t), ptr(grad), FLAT_N, stream), 'r2l_l2_bwd')
            assert check_guard_zones(arena, what) == 4
            assert_no_nan(grad, what + '/grad')
            assert_periodic(grad, FLAT_R, what + '/grad')
            bad = np.nonzero(ac.bits(grad[:per].cpu().numpy()) != ac.bits(want))[0]
            pc.report(f'{what}/grad block 0 vs fl(fl(-2 (x - y)) g) (bitwise)', bad.size, 0.0)
            assert bad.size == 0, (what, int(bad.size), int(bad[0]))
            bound, trips = ac.l2_sum_bound(FLAT_N, ac.L2_FWD_CAP)
            err = abs(float(out.cpu()[0]) - ref_sum) / ref_sum
            pc.report(f'{what}/sum vs {FLAT_R} x float64 sum of the block, relative ({trips} trips)', err, bound)
            assert err <= bound, (what, float(out.cpu()[0]), ref_sum, err, bound)
    finally:
        del x, y
        grad = ws = arena = None
        release()


SSIM_R = 342                                      # (1368,3,512,512): 1 075 838 976 float32 = 4.3e9 bytes per buffer


@functools.lru_cache(maxsize=1)
def ssim_block_refs():
    """aux_checks.ssim_refs of the (4,3,512,512) block, frame by frame on a thread pool (numpy releases the GIL; the planes are
    independent): the mean of the block is the mean of its frames' means, d mean / d img2 a quarter of each frame's"""
    import aux_checks as ac
    from concurrent.futures import ThreadPoolExecutor
    xb, yb = ac.make_inputs('noise', (BB, 3, 512, 512), seed=13)
    with ThreadPoolExecutor(2 * BB) as pool:
        jobs = [(pool.submit(orc.ssim, xb[f:f + 1], yb[f:f + 1]), pool.submit(orc.ssim, xb[f:f + 1], yb[f:f + 1], dtype=np.float32))
                for f in range(BB)]
        r64, r32 = [j[0].result() for j in jobs], [j[1].result() for j in jobs]
    g64 = np.concatenate([np.asarray(g, np.float64) for _, g in r64]) / BB
    g32 = np.concatenate([np.asarray(g, np.float64) for _, g in r32]) / BB
    for a in (g64, g32):
        a.setflags(write=False)
    return float(np.mean([float(v) for v, _ in r64])), g64, float(np.mean([float(v) for v, _ in r32])), g32


def check_ssim_large(device):
    """r2l_ssim_fwd / r2l_ssim_bwd where a float32 byte offset passes 2^32: periodic images, so the gradient is periodic and, on
    block 0, R x it is the block's own d mean / d img2; the mean is the block's.  Limits: aux_checks' (the float32 oracle's own
    distance from the float64 one)"""
    import aux_checks as ac
    from raw2logit_amd import _lib
    from raw2logit_amd._lib import ptr
    shape = (BB * SSIM_R, 3, 512, 512)
    n = int(np.prod(shape))
    assert 4 * n >= 2 ** 32 > 4 * (n - BB * 3 * 512 * 512)
    lib = _lib.device_library()
    nws = lib.r2l_aux_workspace_bytes(*shape)
    need_or_skip(3 * 4 * n + nws + 3 * GIB, device)
    what = f'large ssim {shape}'
    xb, yb = ac.make_inputs('noise', (BB, 3, 512, 512), seed=13)
    v64, g64, v32, g32 = ssim_block_refs()
    x, y = (torch.from_numpy(a).to(device).repeat(SSIM_R, 1, 1, 1) for a in (xb, yb))
    try:
        stream = _lib.library_for(x)[1]
        with guarded(device, arena_bytes(4 * n, nws, 8)) as arena:
            ws = torch.empty(nws, dtype=torch.uint8, device=device)
            out = torch.empty(1, dtype=torch.float64, device=device)
            grad = torch.empty_like(y)
            gup = torch.full((1,), ac.GUP, dtype=torch.float32, device=device)
            lib.check(lib.r2l_ssim_fwd(ptr(x), ptr(y), ptr(out), ptr(ws), nws, 1, *shape, stream), 'r2l_ssim_fwd')
            lib.check(lib.r2l_ssim_bwd(ptr(x), ptr(y), ptr(gup), ptr(grad), ptr(ws), nws, 1, *shape, stream), 'r2l_ssim_bwd')
            assert check_guard_zones(arena, what) == 4
            assert_no_nan(grad, what + '/grad')
            assert_periodic(grad, SSIM_R, what + '/grad')
            # the D maps the forward left: 3 n float32 at the end of the workspace, every one written
            assert_no_nan(ws[nws - 12 * n:].view(torch.float32), what + '/D maps')
            ac.check_mean(what, float(out.cpu()[0]), v64, v32)
            ac.check_grad(what + ' block 0 x R', grad[:BB].cpu().numpy().astype(np.float64) * SSIM_R, g64, g32, ac.GUP)
    finally:
        del x, y
        grad = ws = arena = None
        release()


def check_flat_strong_augmentation(device):
    """the strong set's fused kernel on (2732,3,512,512).  Flip + rotation + sharpness, forward and backward, without noise:
    periodic, block 0 against tests/strong_aug_oracle.py by the criteria of tests/test_gpu_strong_augmentation.py.  Then flip +
    Philox noise, forward: the deviate of flat output element e, in windows"""
    import strong_aug_oracle as so
    from raw2logit_amd import augmentation as A
    from test_strong_augmentation import _check_sharp, _pre_clamp
    need_or_skip(4 * 4 * FLAT_N + FLAT_N + 3 * GIB, device)
    what = f'large strong augmentation ({BB * FLAT_R},3,{FLAT_H},{FLAT_W})'
    hf, vf, angle = 1, 0, 31.7
    xb = torch.tensor(flat_block(53, -0.2, 1.2))
    x = flat_input(device, 53, -0.2, 1.2).requires_grad_(True)
    try:
        with guarded(device, arena_bytes(4 * FLAT_N, FLAT_N, 4 * FLAT_N, 4 * FLAT_N)) as arena:
            y = A.strong_augment(x, hf, vf, angle, sharpness=0.5)
            y.backward(x.detach())
            y = y.detach()
            assert check_guard_zones(arena, what) == 5
            for name, t in (('out', y), ('vjp', x.grad)):
                assert_no_nan(t, f'{what}/{name}')
                assert_periodic(t, FLAT_R, f'{what}/{name}')
            _check_sharp(y[:BB].cpu(), so.apply(xb, hf, vf, angle, sharpness=0.5), _pre_clamp(xb, hf, vf, angle))
            xo = xb.clone().requires_grad_(True)
            go, = torch.autograd.grad(so.apply(xo, hf, vf, angle, sharpness=0.5), xo, xb)
            e, lim = (x.grad[:BB].cpu().double() - go.double()).abs().max().item(), 1e-6 * go.abs().max().item()
            pc.report(f'{what}/vjp block 0 vs autograd through the oracle', e, lim)
            assert e <= lim, (what, e, lim)
        x.grad = None
        y = arena = t = None
        x = x.detach()
        release()
        key, std = 987654321987, 0.0005
        with guarded(device, arena_bytes(4 * FLAT_N)) as arena, torch.no_grad():
            y = A.strong_augment(x, 1, 0, noise_std=std, noise_key=torch.tensor([key], dtype=torch.int64, device=device))
            assert check_guard_zones(arena, what + ' noise') == 2
            assert_no_nan(y, what + '/noise out')
            xflip = memory_order(x).view(-1, FLAT_W)

            def want(a, b):          # rows a / W .. b / W - 1 of the flipped planes, + std x the deviate of the flat index
                rows = xflip[a // FLAT_W:b // FLAT_W].flip(-1).cpu().numpy().reshape(-1)
                return (rows + np.float32(std) * philox_window(a, b - a, key)).astype(np.float64)
            check_windows(what + '/hflip + noise', y, want, PHILOX_ATOL)
    finally:
        x.grad = None
        del x
        y = arena = xflip = None
        release()
