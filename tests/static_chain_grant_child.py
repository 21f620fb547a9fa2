"""Child process of tests/test_gpu_static_routes.py::test_chain_kernel_dynamic_lds_grant: the default chain at 2, 4, 8 and again 4
strips, in this order, in a process that has launched nothing before -- so that the four calls take the four branches of the
luma-chain kernel's dynamic-LDS grant (r2l_launch.h: r2l_lds_grant): no grant needed (32 KiB), the first grant (64 KiB), the grant
raised (129 KiB), the kept grant covers the call.  Exit code 0 and a last line `ok`, or an assertion."""
import ctypes
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import parity_checks as pc  # noqa: E402
from oracle import isp_oracle as orc  # noqa: E402
from raw2logit_amd import _lib  # noqa: E402

DEV = 'cuda'


def main():
    B, H = 1, 8
    cam_params = orc.DRONE_CAMERA_PARAMS
    bl, wb, ccm = cam_params
    cam = (ctypes.c_double * 16)(*[float(v) for v in list(bl) + list(wb) + list(ccm)])
    codes = (0, 1, 1)      # bilinear, sharpening_filter, gaussian_denoising
    outs = []
    for W in (260, 516, 1028, 516):
        u = np.random.default_rng(1000 * H + W).integers(0, 4096, (B, H, W)).astype(np.uint16)
        raw_np = u.astype(np.float32) / np.float32(4095)
        raw = torch.from_numpy(raw_np).to(DEV)
        lib, stream = _lib.library_for(raw)
        assert lib.r2l_static_workspace_bytes_opts(0, B, H, W, *codes, None) == 0
        out = torch.empty((B, 3, H, W), dtype=torch.float32, device=DEV)
        e, names = pc.kernels_launched(lib, lambda: lib.r2l_static_fwd_io(_lib.ptr(raw), 0, 1.0, _lib.ptr(out), 0, B, H, W, cam, *codes,
                                                                          2.2, None, None, None, 0, stream))
        assert e == 0, lib.r2l_last_error()
        assert names == {'r2l_launch_static_chain_kernel': 1}, (W, names)
        ref = orc.static_batch(raw_np, cam_params)
        err = float(np.abs(out.cpu().numpy() - ref).max())
        pc.report(f'static chain, dynamic LDS grant {B}x{H}x{W}', err, 1e-5)
        assert err <= 1e-5, (W, err)
        outs.append(out.cpu())
    assert torch.equal(outs[1], outs[3])
    print('ok')


if __name__ == '__main__':
    main()
