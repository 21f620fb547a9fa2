"""What d/d raw costs (ParametrizedProcessing.fused_raw_grad): one training step -- forward + backward of the processor with
a fixed cotangent -- timed with HIP events, median of --steps steps after --warmup, for
  fused_raw     the fused kernels with d/d raw (fused_raw_grad = True, frames requiring grad)
  fused         the fused kernels without it (frames not requiring grad)
  staged        the stage-by-stage kernels (the default routing of frames requiring grad)
at 64x256x256 and 64x512x512, BatchNorm train and eval.  Prints one JSON line per configuration and, with --out, writes all
of them to a JSON file.

    python tests/bench_raw_grad.py [--steps 30] [--warmup 5] [--shapes 256,512] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import isp_oracle as orc  # noqa: E402
from raw2logit_amd.processing.pipeline_torch import ParametrizedProcessing  # noqa: E402


def time_steps(m, raw, cot, steps, warmup):
    def one():
        raw.grad = None      # (a fresh d/d raw every step, as torch.autograd.grad gives it: no accumulation kernel)
        y = m(raw)
        y.backward(cot)
    for _ in range(warmup):
        one()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        one()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--shapes', default='256,512')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert args.steps >= 20
    dev = 'cuda'
    rows = []
    for H in [int(s) for s in args.shapes.split(',')]:
        B, W = 64, H
        raw0 = torch.from_numpy(orc.synth_raw(B, H, W, seed=1, kind='scene')).to(dev)
        cot = torch.from_numpy(np.random.default_rng(1).standard_normal((B, 3, H, W)).astype(np.float32)).to(dev)
        for bn_mode in ('train', 'eval'):
            for cfg in ('fused_raw', 'fused', 'staged'):
                m = ParametrizedProcessing(orc.DRONE_CAMERA_PARAMS, batch_norm_output=True).to(dev)
                m.train(bn_mode == 'train')
                m.fused_raw_grad = cfg == 'fused_raw'
                raw = raw0.clone().requires_grad_(cfg != 'fused')
                med, lo, hi = time_steps(m, raw, cot, args.steps, args.warmup)
                row = dict(shape=[B, H, W], bn=bn_mode, config=cfg, median_ms=round(med, 4), min_ms=round(lo, 4),
                           max_ms=round(hi, 4), steps=args.steps)
                rows.append(row)
                print(json.dumps(row), flush=True)
                del m, raw
                torch.cuda.empty_cache()
        for bn_mode in ('train', 'eval'):
            t = {r['config']: r['median_ms'] for r in rows if r['shape'][1] == H and r['bn'] == bn_mode}
            print(json.dumps(dict(shape=[B, H, W], bn=bn_mode, fused_raw_over_staged=round(t['fused_raw'] / t['staged'], 4),
                                  raw_grad_extra_ms=round(t['fused_raw'] - t['fused'], 4))), flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
