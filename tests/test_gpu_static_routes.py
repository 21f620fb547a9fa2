"""The static chains' routes on the gfx950 build: one call per route of r2l_static_plan (and one 16-bit call per route that serves
one) launches exactly what tests/golden/static_routes.txt records for the same call, in a workspace of exactly the queried size."""
import ctypes
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import half_io_checks as hc  # noqa: E402
import parity_checks as pc  # noqa: E402
import static_routes_record as rec  # noqa: E402
from oracle import isp_oracle as orc  # noqa: E402
from raw2logit_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
MEAN_STD = (0.35, 0.36, 0.35, 0.12, 0.11, 0.12)
FFT = 3

# (io, W, (debayer, sharpening, denoising), median size): float32 frames, B = 1, H = 8, the smallest width of the record that
# reaches the route -- the two tile kernels serve W % 4 != 0 only, hence W = 10
CALLS = {
    'stream': (0, 8, (0, 0, 0), 3.0), 'stream_f16': (2, 8, (0, 0, 0), 3.0), 'stream_two_strips_bf16': (1, 260, (1, 0, 0), 3.0),
    'short': (0, 10, (0, 0, 0), 3.0), 'full': (0, 10, (0, 1, 1), 3.0),
    'chain': (0, 8, (0, 1, 1), 3.0), 'chain_bf16': (1, 8, (0, 1, 1), 3.0), 'chain_two_strips': (0, 260, (0, 0, 1), 3.0),
    'planes_median5': (0, 8, (0, 1, 2), 5.0), 'planes_fft': (0, 8, (1, 0, FFT), 3.0),
    'menon': (0, 8, (2, 0, 0), 3.0), 'menon_luma': (0, 260, (2, 1, 1), 3.0), 'menon_fft': (0, 260, (2, 0, FFT), 3.0),
}


@pytest.fixture(scope='module')
def recorded():
    return rec.runs()


@pytest.mark.parametrize('name', list(CALLS))
def test_route_launches_what_the_record_says(name, recorded):
    io, W, codes, med = CALLS[name]
    B, H = 1, 8
    want = recorded[(0, io, (B, H, W), codes, med)]
    assert want['code'] == 0 and want['route'] == name.split('_')[0]
    raw = hc.frames(B, H, W, 1, DEV)
    lib, stream = _lib.library_for(raw)
    bl, wb, ccm = orc.DRONE_CAMERA_PARAMS
    cam = (ctypes.c_double * 16)(*[float(v) for v in list(bl) + list(wb) + list(ccm)])
    ov = (ctypes.c_double * 5)(1.0, 1.0, 0.5, 0.3, med) if med != 3.0 else None
    ms = (ctypes.c_float * 6)(*MEAN_STD) if want['norm'] else None
    nws = lib.r2l_static_workspace_bytes_opts(0, B, H, W, *codes, ov)
    if codes[2] != FFT:         # (fft_denoising: + rocFFT's work buffer, which the emulation does not have)
        assert nws == want['workspace'], (nws, want)
    else:
        assert nws >= want['workspace'] > 0
    ws = torch.empty(max(nws, 1), dtype=torch.uint8, device=DEV)
    out = torch.empty((B, 3, H, W), dtype=(torch.float32, torch.bfloat16, torch.float16)[io], device=DEV)

    def call(nbytes):
        return lib.r2l_static_fwd_io(_lib.ptr(raw), 0, 1.0, _lib.ptr(out), io, B, H, W, cam, *codes, 2.2, ov, ms,
                                     _lib.ptr(ws) if nbytes else None, nbytes, stream)
    e, names = pc.kernels_launched(lib, lambda: call(nws))
    assert e == 0, lib.r2l_last_error()
    # (fft_denoising: between rocFFT's two transforms the device build masks the spectrum with a kernel of its own, where the
    # emulation low-passes on the host -- the one launch the record cannot hold)
    assert names == dict(want['launches'], **({'r2l_launch_spec_mask_kernel': 1} if codes[2] == FFT else {})), (names, want['launches'])
    assert bool(torch.isfinite(out.float()).all())
    if nws:
        assert call(nws - 1) == -2 and b'workspace too small' in lib.r2l_last_error()


def test_chain_kernel_dynamic_lds_grant():
    """The luma-chain kernel's dynamic LDS follows the frame width (16.1 KiB per 256-column strip), and above 48 KiB the launch
    wrapper has to raise the kernel's limit on the device first (r2l_launch.h: r2l_lds_grant) -- code that neither emulation runs.
    tests/static_chain_grant_child.py makes the four calls that reach its four branches (1x8x260, 1x8x516, 1x8x1028, 1x8x516), each
    against orc.static_batch at 1e-5 with the launch record naming r2l_launch_static_chain_kernel once, the two W = 516 outputs
    bit-identical.  In a process of its own, because what a kernel was granted lasts as long as the process: here, behind the
    tests above, the branches would depend on what ran before."""
    import subprocess
    r = subprocess.run([sys.executable, os.path.join(HERE, 'static_chain_grant_child.py')], capture_output=True, text=True, timeout=300,
                       cwd=os.path.dirname(HERE))
    print(r.stdout)
    assert r.returncode == 0, (r.returncode, (r.stdout + r.stderr)[-3000:])
    assert r.stdout.strip().endswith('ok') and r.stdout.count('dynamic LDS grant') >= 4
