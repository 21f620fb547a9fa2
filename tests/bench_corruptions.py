"""The corruption kernels (r2l_corruptions.h) at the evaluation batch: one JSON line per transform, severity and shape, appended
to profiles/corruptions_bench.jsonl.  Record only -- no threshold.

20 timed iterations after 5 warm-ups (device events) on 64x3x256^2 and 64x3x512^2, severities 1 and 5.  Per line: microseconds,
the fraction of the 8 TB/s HBM peak at the design traffic (24 B/px = three channels read and written once; contrast 36 B/px with
its reduction pass), and the time of the same arithmetic as a torch-eager chain on the same GPU where one exists (the pointwise
transforms, and gaussian_blur through conv2d on replicate-padded frames), with the largest difference between the two results."""
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from raw2logit_amd import corruptions as C  # noqa: E402

PEAK = 8e12
ITERS, WARM = 20, 5
KEY = 1234567


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


def _hsv(x):
    r, g, b = x[:, 0], x[:, 1], x[:, 2]
    v = x.amax(1)
    d = v - x.amin(1)
    safe = torch.where(d == 0, torch.ones_like(d), d)
    s = torch.where(d == 0, torch.zeros_like(d), d / v)
    h = torch.where(b == v, 4 + (r - g) / safe, torch.where(g == v, 2 + (b - r) / safe, (g - b) / safe))
    h = torch.where(d == 0, torch.zeros_like(d), torch.remainder(h / 6, 1.0))
    return h, s, v


def _rgb(h, s, v):
    i = torch.floor(h * 6)
    f = h * 6 - i
    p, q, t = v * (1 - s), v * (1 - f * s), v * (1 - (1 - f) * s)
    i = i.long() % 6
    table = ((v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q))
    out = []
    for c in range(3):
        o = table[5][c]
        for k in range(4, -1, -1):
            o = torch.where(i == k, table[k][c], o)
        out.append(o)
    return torch.stack(out, 1)


def eager(x, t, sev):
    """the transform as a chain of torch ops on the device, or None where there is no short one (zoom_blur, impulse / shot noise)"""
    c = C.SEVERITY[t][sev - 1]
    if t == 'contrast':
        def f():
            m = x.mean((-2, -1), keepdim=True)
            return ((x - m) * c + m).clamp(0, 1)
        return f
    if t == 'brightness':
        def f():
            h, s, v = _hsv(x)
            return _rgb(h, s, (v + c).clamp(0, 1)).clamp(0, 1)
        return f
    if t == 'saturate':
        def f():
            h, s, v = _hsv(x)
            return _rgb(h, (s * c[0] + c[1]).clamp(0, 1), v).clamp(0, 1)
        return f
    if t == 'gaussian_noise':
        return lambda: (x + c * torch.randn_like(x)).clamp(0, 1)
    if t == 'speckle_noise':
        return lambda: (x + x * (c * torch.randn_like(x))).clamp(0, 1)
    if t == 'gaussian_blur':
        w = C.gaussian_taps(c)
        k = torch.tensor(w[:0:-1] + w, device=x.device)
        r = len(w) - 1
        kv, kh = k.view(1, 1, -1, 1).expand(3, 1, -1, 1), k.view(1, 1, 1, -1).expand(3, 1, 1, -1)

        def f():
            p = torch.nn.functional.pad(x, (r, r, r, r), mode='replicate')
            return torch.nn.functional.conv2d(torch.nn.functional.conv2d(p, kv, groups=3), kh, groups=3).clamp(0, 1)
        return f
    return None


def main():
    dev = 'cuda:0'
    out = os.path.join(REPO, 'profiles', 'corruptions_bench.jsonl')
    with open(out, 'a') as log:
        for S in (256, 512):
            x = torch.rand(64, 3, S, S, device=dev)
            px = 64 * S * S
            for t in C.KINDS:
                if t == 'identity':
                    continue
                for sev in (1, 5):
                    us = timed(lambda: C.corrupt(x, t, sev, key=KEY))
                    us_norm = timed(lambda: C.corrupt(x, t, sev, key=KEY, mean=[0.35, 0.36, 0.35], std=[0.12, 0.11, 0.12]))
                    bpp = 36.0 if t == 'contrast' else 24.0
                    rec = {'shape': [64, 3, S, S], 'transform': t, 'severity': sev, 'us': round(us, 1),
                           'us_with_normalize': round(us_norm, 1), 'design_bytes_per_px': bpp,
                           'frac_of_8TBps': round(px * bpp / (us * 1e-6) / PEAK, 3)}
                    e = eager(x, t, sev)
                    if e is not None:
                        rec['eager_us'] = round(timed(e), 1)
                        if t not in C.RANDOM:
                            rec['max_abs_diff_vs_eager'] = float((C.corrupt(x, t, sev) - e()).abs().max())
                    line = json.dumps(rec)
                    print(line, flush=True)
                    log.write(line + '\n')
                    log.flush()


if __name__ == '__main__':
    main()
