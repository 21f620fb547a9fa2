"""What the output epilogue of the static chains buys (StaticProcessing armed by ComposeState.arm, static_pipeline(epilogue=...),
r2l_static_fwd_epilogue).

One process, two variants ALTERNATED call by call on the same frames, HIP-event time of each call by itself:

  (a) the plain call, then augmentation.flip_rot      16 + 24 B/px in float32 (design bytes); with a bfloat16 output the float32
                                                      call, flip_rot and torch's cast: 16 + 24 + 18
  (b) the call with the epilogue                      16 B/px in float32, 10 in bfloat16

at 256x1024x1024 and 1024x512x512, for the bilinear short chain, the Malvar2004 short chain and the train.py default chain, with a
float32 and a bfloat16 output, for hflip, vflip and both.  Medians with the distribution-free 95 % interval of the median (order
statistics of the sample).  A form earns its place only where its whole interval lies below that of (a): `fused_below_plain`.
Before it times anything the script checks (b) == (a) bit for bit at the timed size.

    python tests/bench_static_epilogue.py [--out profiles/static_epilogue.json] [--reps 30] [--warmup 8]
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raw2logit_amd import _lib, cameras, functional as F_   # noqa: E402
from raw2logit_amd.augmentation import flip_rot   # noqa: E402

SHAPES = [(256, 1024, 1024), (1024, 512, 512)]
CHAINS = [('bilinear short', ('bilinear', 'none', 'none')), ('malvar2004 short', ('malvar2004', 'none', 'none')),
          ('default chain', ('bilinear', 'sharpening_filter', 'gaussian_denoising'))]
MOVES = [('hflip', (True, False, 0)), ('vflip', (False, True, 0)), ('both', (True, True, 0))]
DESIGN_BYTES = {'float32': dict(a=16 + 24, b=16), 'bfloat16': dict(a=16 + 24 + 18, b=10)}      # per pixel, float32 frames


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return 1e3 * e0.elapsed_time(e1), out


def median_interval(xs):
    """(median, lower, upper): the distribution-free 95 % confidence interval of the median, order statistics k and n - 1 - k with
    k = floor((n - 1.96 sqrt(n)) / 2)"""
    s, n = sorted(xs), len(xs)
    k = max(0, int(math.floor((n - 1.96 * math.sqrt(n)) / 2.0)))
    return statistics.median(s), s[k], s[n - 1 - k]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=8)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_static_epilogue.py measures on the GPU; there is no other path'
    assert _lib.device_library().is_device
    results = []
    for B, H, W in SHAPES:
        raw = torch.randint(0, 4096, (B, H, W), device='cuda', dtype=torch.int32,
                            generator=torch.Generator('cuda').manual_seed(0)).to(torch.float32) / 4095.0
        for label, chain in CHAINS:
            for oname, odt in (('float32', None), ('bfloat16', torch.bfloat16)):
                for mname, move in MOVES:
                    def plain_then_move():
                        y = flip_rot(F_.static_pipeline(raw, cameras.DRONE, *chain), *move)
                        return y if odt is None else y.to(odt)
                    variants = {'a': plain_then_move,
                                'b': lambda: F_.static_pipeline(raw, cameras.DRONE, *chain, out_dtype=odt, epilogue=move)}
                    assert F_.static_epilogue_why(raw, *chain, epilogue=move, out_dtype=odt) is None
                    same = torch.equal(variants['a'](), variants['b']())
                    for _ in range(args.warmup):
                        for k in 'ab':
                            variants[k]()
                    torch.cuda.synchronize()
                    us = {k: [] for k in 'ab'}
                    for _ in range(args.reps):
                        for k in 'ab':                          # alternated: clock and neighbours' load hit both alike
                            t, out = timed(variants[k])
                            us[k].append(t)
                            del out
                    iv = {k: median_interval(v) for k, v in us.items()}
                    px = B * H * W
                    rec = dict(shape=[B, H, W], chain=label, output=oname, move=mname, reps=args.reps, warmup=args.warmup,
                               bitwise_b_equals_a=same,
                               median_us={k: round(iv[k][0], 1) for k in 'ab'},
                               interval_us={k: [round(iv[k][1], 1), round(iv[k][2], 1)] for k in 'ab'},
                               min_us={k: round(min(v), 1) for k, v in us.items()},
                               design_bytes_per_px=DESIGN_BYTES[oname],
                               design_gbps={k: round(DESIGN_BYTES[oname][k] * px / iv[k][0] / 1e3, 1) for k in 'ab'},
                               b_over_a=round(iv['b'][0] / iv['a'][0], 4),
                               byte_ratio_b_over_a=round(DESIGN_BYTES[oname]['b'] / DESIGN_BYTES[oname]['a'], 4),
                               fused_below_plain=iv['b'][2] < iv['a'][1])
                    results.append(rec)
                    print(f'{B}x{H}x{W} {label:17s} {oname:8s} {mname:5s} a {iv["a"][0]:8.1f} [{iv["a"][1]:8.1f}, {iv["a"][2]:8.1f}]  '
                          f'b {iv["b"][0]:8.1f} [{iv["b"][1]:8.1f}, {iv["b"][2]:8.1f}] us   b/a {rec["b_over_a"]:.3f} '
                          f'(bytes {rec["byte_ratio_b_over_a"]:.3f})   below {rec["fused_below_plain"]}   b==a {same}', flush=True)
                    assert same, 'the call with the epilogue must equal the plain call + flip_rot bit for bit'
        del raw
        torch.cuda.empty_cache()
    doc = dict(device=torch.cuda.get_device_name(0), library_digest=_lib.source_digest(),
               method='one process; variants alternated call by call; HIP events around each call; medians with the distribution-free '
                      '95 % interval of the median', results=results)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(doc, f, indent=1)
    print(json.dumps(dict(worst_b_over_a=max(r['b_over_a'] for r in results), best_b_over_a=min(r['b_over_a'] for r in results),
                          forms_not_below=[[r['shape'], r['chain'], r['output'], r['move']] for r in results if not r['fused_below_plain']])))


if __name__ == '__main__':
    main()
