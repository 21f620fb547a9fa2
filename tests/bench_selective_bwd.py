"""What the selective backward saves (ParametrizedProcessing.selective_backward): one step -- forward + backward of the
processor with a fixed cotangent -- timed with HIP events for the routes RAW-only, GAMMA-only, BLUR-only and RAW+GAMMA, the
attribute off (the full backward) and on, at 64x256x256 and 64x512x512 under BatchNorm train and eval.  Old and new alternate
in one process (rounds of --steps steps each, after a pre-roll of both), the figure is the median over all rounds' steps.
Prints one JSON line per configuration and, with --out, writes all of them to a JSON file.  --limit seconds is a budget the script keeps between
steps (what is measured by then is written); it cannot end a step that hangs inside a HIP call, so on a shared machine run the
script under a limit from outside as well:

    timeout -k 10 300 python tests/bench_selective_bwd.py [--steps 20] [--rounds 5] [--shapes 256,512] [--limit 270] [--out FILE]"""
import argparse
import json
import os
import signal
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import selective_bwd_checks as sc  # noqa: E402
from oracle import isp_oracle as orc  # noqa: E402


class Timeout(Exception):
    pass


def _alarm(*_):
    raise Timeout()


def steps_ms(m, raw, cot, n):
    ts = []
    for _ in range(n):
        raw.grad = None
        for p in m.parameters():
            p.grad = None
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        m(raw).backward(cot)
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--shapes', default='256,512')
    ap.add_argument('--limit', type=int, default=420)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    dev = 'cuda'
    rows = []
    signal.signal(signal.SIGALRM, _alarm)
    signal.alarm(args.limit)
    try:
        for H in [int(s) for s in args.shapes.split(',')]:
            B, W = 64, H
            raw0 = torch.from_numpy(orc.synth_raw(B, H, W, seed=1, kind='scene')).to(dev)
            cot = torch.from_numpy(np.random.default_rng(1).standard_normal((B, 3, H, W)).astype(np.float32)).to(dev)
            for bn_mode in ('eval', 'train'):
                for route in sc.FOUR:
                    raw = raw0.clone().requires_grad_(sc.ROUTES[route][0])
                    ms = {sel: sc.plain_module(True, bn_mode == 'train', dev, route, sel) for sel in (False, True)}
                    for sel in (False, True):      # pre-roll
                        steps_ms(ms[sel], raw, cot, 5)
                    ts = {False: [], True: []}
                    for _ in range(args.rounds):
                        for sel in (False, True):
                            ts[sel] += steps_ms(ms[sel], raw, cot, args.steps)
                    full, sel = statistics.median(ts[False]), statistics.median(ts[True])
                    row = dict(shape=[B, H, W], bn=bn_mode, route=route, full_step_ms=round(full, 4),
                               selective_step_ms=round(sel, 4), selective_over_full=round(sel / full, 4),
                               steps=args.steps * args.rounds)
                    rows.append(row)
                    print(json.dumps(row), flush=True)
                    del ms, raw
    except Timeout:
        print(json.dumps(dict(note=f'time limit of {args.limit} s reached: {len(rows)} configurations measured')), flush=True)
    finally:
        signal.alarm(0)
        if args.out:
            with open(args.out, 'w') as f:
                json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
