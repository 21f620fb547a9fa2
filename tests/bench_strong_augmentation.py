"""The strong augmentation kernels (r2l_augment_strong.h) at the training batch: one JSON line per configuration.

Cases: rotation only, rotation + noise + sharpness; forward and backward timed separately with device events after a
warm-up, next to the oracle's torch-eager chain (tests/strong_aug_oracle.py) on the same GPU, whose outputs are compared.
Design bytes: forward 8 B/px (x in, y out; + 1 B/px clamp mask when the sharpness is on and a gradient is wanted),
backward rotation 8 B/px, sharpness adjoint 4 + 1 + 4 B/px more.  Fraction of the 8 TB/s HBM peak."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import strong_aug_oracle as so  # noqa: E402
from raw2logit_amd import augmentation as A  # noqa: E402

PEAK = 8e12
ANGLE, ITERS, WARM = 33.3, 20, 5


def timed(fn):
    for _ in range(WARM):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(ITERS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / ITERS     # us


def oracle_gpu(x, noise, sharp):
    """the oracle's torch-eager chain on the GPU tensor (its grid built on the CPU, as a one-off constant)"""
    H, W = x.shape[-2:]
    grid = so.affine_grid(ANGLE, H, W).to(x.device).expand(x.shape[0], H, W, 2)
    dummy = torch.ones((x.shape[0], 1, H, W), device=x.device)
    out = torch.nn.functional.grid_sample(torch.cat((x, dummy), 1), grid, mode='nearest', padding_mode='zeros',
                                          align_corners=False)
    v = torch.where(out[:, -1:] < 0.5, torch.zeros_like(out[:, :-1]), out[:, :-1])
    if noise is not None:
        v = v + noise
    if sharp:
        k = torch.ones((3, 3), device=x.device)
        k[1, 1] = 5.0
        k = (k / k.sum()).expand(3, 1, 3, 3)
        d = v.clone()
        d[..., 1:-1, 1:-1] = torch.nn.functional.conv2d(v, k, groups=3)
        v = (0.5 * v + 0.5 * d).clamp(0, 1)
    return v


def main():
    dev = 'cuda:0'
    for S in (512, 256):
        B = 64
        x = torch.rand(B, 3, S, S, device=dev)
        g = torch.randn_like(x)
        px = x.numel()
        key = torch.tensor([12345], dtype=torch.int64, device=dev)
        for case in ('rotation', 'rotation+noise+sharpness'):
            full = case != 'rotation'
            kw = dict(angle=ANGLE, noise_std=0.0005 if full else 0.0, noise_key=key if full else None,
                      sharpness=0.5 if full else None)
            xr = x.clone().requires_grad_(True)
            fwd_us = timed(lambda: A.strong_augment(x, **kw))
            y = A.strong_augment(xr, **kw)
            bwd_us = timed(lambda: torch.autograd.grad(y, xr, g, retain_graph=True))
            noise = (A.strong_augment(x, angle=ANGLE, noise_std=0.0005, noise_key=key) -
                     A.strong_augment(x, angle=ANGLE)) if full else None
            xo = x.clone().requires_grad_(True)
            ref_fwd_us = timed(lambda: oracle_gpu(x, noise, full))
            yo = oracle_gpu(xo, noise, full)
            ref_bwd_us = timed(lambda: torch.autograd.grad(yo, xo, g, retain_graph=True))
            diff = (y.detach() - yo.detach()).abs()
            fb, bb = 8.0, (8.0 + (9.0 if full else 0.0))
            print(json.dumps({
                'shape': [B, 3, S, S], 'case': case,
                'fwd_us': round(fwd_us, 1), 'fwd_design_bytes_per_px': fb, 'fwd_frac_of_8TBps': round(px * fb / (fwd_us * 1e-6) / PEAK, 3),
                'bwd_us': round(bwd_us, 1), 'bwd_design_bytes_per_px': bb, 'bwd_frac_of_8TBps': round(px * bb / (bwd_us * 1e-6) / PEAK, 3),
                'eager_fwd_us': round(ref_fwd_us, 1), 'eager_bwd_us': round(ref_bwd_us, 1),
                'max_abs_diff_vs_eager': float(diff.max()), 'px_differing_vs_eager': int((diff > 2e-7).sum())}), flush=True)
            del y, yo, xr, xo


if __name__ == '__main__':
    main()
