"""The forward's routes on the gfx950 build: one tiny call per route of r2l_fwd_plan and per io slot that serves one (and of the
backward's recomputing BatchNorm-sums pass, which a 16-bit / channels-last cotangent takes at every size) launches exactly what
tests/golden/fwd_routes.txt records for the same call, in a workspace of exactly the queried size."""
import ctypes
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import fwd_routes_record as rec  # noqa: E402
import half_io_checks as hc  # noqa: E402
import parity_checks as pc  # noqa: E402
from raw2logit_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NONE, TRAIN, EVAL = 0, 1, 2
ALL, A, KEEP, HFLIP, VFLIP, ROT90 = 0, 1, 8, 16, 32, 64
FWD, STEP_FWD, STEP_BWD = 0, 1, 2
STATS_ONLY, KEEP_LUMA = 1, 4           # R2L_F_*
IO_SLOTS = {'bf16': (1, 0), 'f16': (2, 0), 'nhwc': (0, 1), 'bf16_nhwc': (1, 1), 'f16_nhwc': (2, 1)}

# name: (entry, 16-bit frames, (B, H, W), BatchNorm mode, phase, io, layout, additive, R2L_F_* flags) -- the key of the record's R line, at the
# smallest shape of the record that reaches the route: W = 8 / 260 / 516 / 1028 for 1 / 2 / 4 / 8 wavefronts per row, W = 10 for the
# ragged tile kernel; the exact one is reached past 2048 columns only, the additive one on 256 x 256
CALLS = {
    'stream_w1': (FWD, 0, (1, 8, 8), NONE, ALL, 0, 0, 0, 0), 'stream_w2': (FWD, 0, (1, 8, 260), NONE, ALL, 0, 0, 0, KEEP_LUMA),
    'stream_w4': (FWD, 0, (1, 8, 516), NONE, ALL, 0, 0, 0, 0), 'stream_w8': (FWD, 0, (1, 8, 1028), NONE, ALL, 0, 0, 0, 0),
    'stream_u16': (STEP_FWD, 1, (2, 8, 8), NONE, KEEP, 0, 0, 0, 0), 'stream_epi': (STEP_FWD, 0, (1, 8, 8), EVAL, VFLIP | ROT90, 0, 0, 0, 0),
    'split_apply': (STEP_FWD, 0, (2, 8, 8), TRAIN, KEEP, 0, 0, 0, 0), 'stats_apply': (STEP_FWD, 1, (1, 8, 516), TRAIN, KEEP, 0, 0, 0, 0),
    'phase_a': (STEP_FWD, 0, (1, 8, 8), TRAIN, A | KEEP, 0, 0, 0, 0), 'stats_only': (FWD, 0, (1, 8, 260), NONE, ALL, 0, 0, 0, STATS_ONLY),
    'tile_ragged': (FWD, 0, (1, 8, 10), NONE, ALL, 0, 0, 0, 0), 'tile_exact': (STEP_FWD, 0, (1, 64, 2112), NONE, KEEP, 0, 0, 0, 0),
    'tile_additive': (STEP_FWD, 0, (1, 256, 256), TRAIN, KEEP, 0, 0, 1, 0), 'bn_reduce': (STEP_BWD, 0, (1, 8, 8), TRAIN, KEEP, 0, 0, 0, 0),
}
for _name, (_io, _layout) in IO_SLOTS.items():
    CALLS['stream_io_' + _name] = (STEP_FWD, 0, (1, 8, 8), NONE, KEEP, _io, _layout, 0, 0)
    CALLS['apply_io_' + _name] = (STEP_FWD, 1, (1, 8, 8), TRAIN, KEEP, _io, _layout, 0, 0)
    CALLS['bnr_io_' + _name] = (STEP_BWD, 0, (1, 8, 8), TRAIN, (A if _io & 1 else ALL) | KEEP, _io, _layout, 0, 0)


@pytest.fixture(scope='module')
def recorded():
    return rec.runs()


def packed_parameters():
    """the drone camera, a bilinear debayer, the reference's sharpening and blur kernels: R2L_P_* order, 150 float32"""
    rb, g = [.25, .5, .25, .5, 1, .5, .25, .5, .25], [0, .25, 0, .25, 1, .25, 0, .25, 0]
    debayer = []
    for k in range(3):
        for c in range(3):
            debayer += (g if k == 1 else rb) if k == c else [0.0] * 9
    b1 = [1, 4, 6, 4, 1]
    p = [0.0625] * 4 + [2.86653646, 1.0, 1.73079425]
    p += [1.50768983, -0.33571374, -0.17197604, -0.23048614, 1.70698738, -0.47650126, -0.03119153, -0.32803956, 1.35923111, 2.2]
    p += debayer + [0, -1, 0, -1, 5, -1, 0, -1, 0] + [a * b / 256.0 for a in b1 for b in b1]
    p += [0.299, 0.587, 0.114, -0.14714119, -0.28886916, 0.43601035, 0.61497538, -0.51496512, -0.10001026]
    p += [1, 0, 1.13988303, 1, -0.394642334, -0.58062185, 1, 2.03206185, 0]
    assert len(p) == 150
    return torch.tensor(p, dtype=torch.float32, device=DEV)


@pytest.mark.parametrize('name', list(CALLS))
def test_route_launches_what_the_record_says(name, recorded):
    entry, u16, (B, H, W), bn_mode, phase, io, layout, additive, flags = CALLS[name]
    want = recorded[CALLS[name]]
    assert want['code'] == 0 and name.startswith(want['tag'].split('_')[0]), want
    raw = hc.frames(B, H, W, 1, DEV, u16=bool(u16))
    lib, stream = _lib.library_for(raw)
    P = packed_parameters()
    offsets = (0, 4, 7, 16, 17, 98, 107, 132, 141)
    table = (ctypes.c_void_p * 9)(*[P.data_ptr() + 4 * o for o in offsets])
    add = torch.zeros((3, 256, 256), device=DEV) if additive else None
    nws = lib.r2l_isp_workspace_bytes(B, H, W)
    assert nws == want['workspace'], (nws, want)
    ws = torch.empty(nws, dtype=torch.uint8, device=DEV)
    dtype = (torch.float32, torch.bfloat16, torch.float16)[io]
    out = torch.zeros((B, 3, H, W), dtype=dtype, device=DEV)
    cot = torch.ones((B, 3, H, W), dtype=dtype, device=DEV)
    rm, rv = torch.full((3,), 0.4, device=DEV), torch.full((3,), 0.04, device=DEV)
    nbt = torch.zeros(1, dtype=torch.int64, device=DEV)
    bn = torch.tensor([0.4, 0.45, 0.35, 4.0, 3.5, 4.5], device=DEV)
    stats = torch.zeros(7, dtype=torch.float64, device=DEV)
    p = _lib.ptr

    def forward(nbytes, ph):
        if entry == FWD:
            return lib.r2l_isp_fwd(p(raw), p(P), p(add), p(bn), p(out), p(stats), p(ws), nbytes, B, H, W, flags, stream)
        return lib.r2l_isp_step_fwd_layout(p(raw), u16, 65535.0, table, p(add), bn_mode, p(rm), p(rv), p(nbt), 1e-5, 0.1, p(out), io,
                                           layout, p(ws), nbytes, B, H, W, 1, ph, None, stream)

    def backward(nbytes):
        return lib.r2l_isp_step_bwd_layout(p(raw), u16, 65535.0, p(add), p(cot), io, layout, p(out), None, None, bn_mode, p(ws),
                                           nbytes, B, H, W, 1, phase, None, stream, None, None, 0, 0)

    if entry == STEP_BWD:       # behind a whole step's forward; the record holds the backward's launches
        assert forward(nws, (phase & ~3) | ALL) == 0, lib.r2l_last_error()
    call = backward if entry == STEP_BWD else (lambda nbytes: forward(nbytes, phase))
    e, names = pc.kernels_launched(lib, lambda: call(nws))
    assert e == 0, lib.r2l_last_error()
    assert names == want['launches'], (names, want['launches'])
    assert bool(torch.isfinite(out.float()).all())
    if entry == STEP_BWD:
        off = lib.r2l_isp_step_offset(2, B, H, W)     # R2L_STEP_BN_SUMS
        assert bool(torch.isfinite(ws[off:off + 48].view(torch.float64)).all())
    assert call(nws - 1) == -2 and b'workspace too small' in lib.r2l_last_error()
