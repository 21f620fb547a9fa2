"""What the 16-bit output of the static chains buys (StaticProcessing.output_dtype, r2l_static_fwd_io).

One process, three variants ALTERNATED call by call on the same frames, HIP-event time of each call by itself, medians:

  (a) the float32 call                       16 B/px on float32 frames, 14 on 16-bit containers (design bytes)
  (b) the float32 call + .to(bfloat16)       34 / 32 B/px: what a task model under autocast pays today
  (c) the bfloat16 call                      10 /  8 B/px

at 256x1024x1024 and 1024x512x512, for the bilinear short chain, the Malvar2004 short chain and the train.py default chain, on
float32 and uint16 frames.  The comparison that decides whether the feature earns its keep is (c) against (b); (c)/(a) is printed
next to the byte ratios 10/16 and 8/14.  Before it times anything the script checks (c) == (b) bit for bit at the timed size.

    python tests/bench_static_half.py [--out profiles/static_half.json] [--reps 30] [--warmup 12]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raw2logit_amd import _lib, cameras, functional as F_   # noqa: E402

SHAPES = [(256, 1024, 1024), (1024, 512, 512)]
CHAINS = [('bilinear short', ('bilinear', 'none', 'none')), ('malvar2004 short', ('malvar2004', 'none', 'none')),
          ('default chain', ('bilinear', 'sharpening_filter', 'gaussian_denoising'))]
DESIGN_BYTES = {'float32': dict(a=16, b=34, c=10), 'uint16': dict(a=14, b=32, c=8)}      # per pixel


def frames(B, H, W, container):
    u = torch.randint(0, 4096, (B, H, W), device='cuda', dtype=torch.int32, generator=torch.Generator('cuda').manual_seed(0))
    if container == 'uint16':
        return u.to(torch.int16), 12
    return u.to(torch.float32) / 4095.0, 16


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return 1e3 * e0.elapsed_time(e1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=12)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_static_half.py measures on the GPU; there is no other path'
    assert _lib.device_library().is_device
    results = []
    for B, H, W in SHAPES:
        for container in ('float32', 'uint16'):
            raw, bits = frames(B, H, W, container)
            for label, chain in CHAINS:
                variants = {
                    'a': lambda: F_.static_pipeline(raw, cameras.DRONE, *chain, bits=bits),
                    'b': lambda: F_.static_pipeline(raw, cameras.DRONE, *chain, bits=bits).to(torch.bfloat16),
                    'c': lambda: F_.static_pipeline(raw, cameras.DRONE, *chain, bits=bits, out_dtype=torch.bfloat16),
                }
                assert F_.static_io_why(raw, *chain) is None
                same = torch.equal(variants['b'](), variants['c']())
                for _ in range(args.warmup):
                    for k in 'abc':
                        variants[k]()
                torch.cuda.synchronize()
                us = {k: [] for k in 'abc'}
                for _ in range(args.reps):
                    for k in 'abc':                         # alternated: clock and neighbours' load hit all three alike
                        t, out = timed(variants[k])
                        us[k].append(t)
                        del out
                med = {k: statistics.median(v) for k, v in us.items()}
                px = B * H * W
                rec = dict(shape=[B, H, W], frames=container, chain=label, reps=args.reps, warmup=args.warmup,
                           bitwise_c_equals_b=same,
                           median_us={k: round(v, 1) for k, v in med.items()},
                           min_us={k: round(min(v), 1) for k, v in us.items()},
                           design_bytes_per_px=DESIGN_BYTES[container],
                           design_gbps={k: round(DESIGN_BYTES[container][k] * px / med[k] / 1e3, 1) for k in 'abc'},
                           c_over_b=round(med['c'] / med['b'], 4), c_over_a=round(med['c'] / med['a'], 4),
                           byte_ratio_c_over_a=round(DESIGN_BYTES[container]['c'] / DESIGN_BYTES[container]['a'], 4))
                results.append(rec)
                print(f'{B}x{H}x{W} {container:7s} {label:17s} a {med["a"]:8.1f}  b {med["b"]:8.1f}  c {med["c"]:8.1f} us   '
                      f'c/b {rec["c_over_b"]:.3f}   c/a {rec["c_over_a"]:.3f} (bytes {rec["byte_ratio_c_over_a"]:.3f})   '
                      f'c==b {same}', flush=True)
                assert same, 'the bfloat16 call must equal the float32 call + .to(bfloat16) bit for bit'
            del raw
            torch.cuda.empty_cache()
    doc = dict(device=torch.cuda.get_device_name(0), library_digest=_lib.source_digest(),
               method='one process; variants alternated call by call; HIP events around each call; medians', results=results)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(doc, f, indent=1)
    print(json.dumps(dict(worst_c_over_b=max(r['c_over_b'] for r in results), best_c_over_b=min(r['c_over_b'] for r in results))))


if __name__ == '__main__':
    main()
