"""Driver of the lock-step run of the corruption kernels (tests/test_lockstep_corruptions.py starts it in a subprocess under
LD_PRELOAD=libasan.so): every kernel of r2l_corruptions.h in its device form -- one fiber per lane, real barriers between the
phases of the blur and mean kernels -- on host memory with malloc redzones, at its smallest shapes, results against the oracle.

    python tests/lockstep_corruptions.py <lock-step library>"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import torch  # noqa: E402

import emul_hook  # noqa: E402


def main():
    emul_hook.enable(sys.argv[1])
    lib = emul_hook.active()
    assert not lib.is_device
    torch.set_num_threads(1)
    import corruption_checks as cc
    import parity_checks as pc
    from raw2logit_amd import corruptions as C
    want = {'contrast': ('corrupt_mean', 'corrupt_contrast'), 'gaussian_blur': ('corrupt_blur',), 'zoom_blur': ('corrupt_zoom',),
            'brightness': ('corrupt_brightness',), 'saturate': ('corrupt_saturate',)}
    for t in cc.DETERMINISTIC:
        # a frame below one tile and below 2 radius + 1, and one with W % 4 != 0 that takes several tiles and workgroups
        _, names = pc.kernels_launched(lib, lambda: cc.check_oracle_parity('cpu', t, ((1, 3, 8, 8), (2, 3, 34, 34)), severities=(5,)))
        for k in want[t]:
            assert any(n.startswith('r2l_launch_' + k) for n in names), (k, sorted(names))
        print('PASS', t, ' '.join(sorted(names)), flush=True)
    _, names = pc.kernels_launched(lib, lambda: (cc.check_identity('cpu'), cc.check_noise_identities('cpu', (1, 3, 10, 18))))
    for k in ('identity', 'gaussian_noise', 'speckle_noise', 'impulse_noise', 'shot_noise'):
        assert any(n.startswith('r2l_launch_corrupt_' + k) for n in names), (k, sorted(names))
    x = torch.rand(1, 3, 10, 18) * 1.2 - 0.1
    for t in C.RANDOM:
        y = C.corrupt(x, t, 5, key=cc.KEY, mean=cc.MEAN, std=cc.STD)
        assert bool(torch.isfinite(y).all())
    print('PASS noises', ' '.join(sorted(names)), flush=True)
    print('corruption lock-step checks passed', flush=True)


if __name__ == '__main__':
    main()
