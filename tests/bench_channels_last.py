"""What the channels-last output / cotangent saves (ParametrizedProcessing.output_memory_format): one step -- forward + backward of
the processor with a fixed cotangent, train-mode BatchNorm -- timed with HIP events at 64x512x512 and 64x256x256, in float32 and
bfloat16, for three configurations:
    a  planar+conv  what a channels-last caller pays today: the planar kernels, .contiguous(memory_format=channels_last) on the
                    output, and autograd's conversion of the channels-last cotangent back to planar;
    b  nhwc         output_memory_format = torch.channels_last: the kernels store / load the interleaved tensors themselves;
    c  planar       the plain planar step with a planar cotangent and no conversion: the floor.
All configurations live in one process and alternate in RANDOM order (seeded): rounds of --steps steps each after a pre-roll of
all.  A round is ONE timed window -- one pair of events around its --steps steps, a quarter of a second at 64x512x512 with the
default 400 -- and its figure is the window over the steps.  Per configuration: the median of the rounds' figures and the lowest
and highest of them (the spread over the alternations -- the interval to compare).  "faster" means b against a, intervals
apart; b against c is the cost of the interleaved access pattern, whatever its sign.  A second pass reads the library's per-kernel timer for the apply pass, the
BatchNorm sums and kernel B1's plane pass.  Prints one JSON line per (shape, type) and, with --out, writes them to a JSON file
(profiles/channels_last.json).  --limit seconds is a budget the script keeps between steps; run it under a limit from outside too:

    timeout -k 10 400 python tests/bench_channels_last.py [--steps 400] [--rounds 7] [--shapes 512,256] [--limit 360] [--out FILE]

--traffic KIND (planar | nhwc) instead runs a few float32 steps of ONE configuration at 64x512x512 and nothing else: the workload of
a counters-only profiler run (bytes written and fetched per kernel -> profiles/channels_last_pmc.txt)."""
import argparse
import ctypes
import json
import os
import random
import signal
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import raw_grad_checks as rc  # noqa: E402
from oracle import isp_oracle as orc  # noqa: E402
from raw2logit_amd import _lib  # noqa: E402

CONFIGS = ('planar+conv', 'nhwc', 'planar')
KERNELS = ('fwd_apply', 'bnr_planes', 'bwd1_plane')
CL = torch.channels_last


class Timeout(Exception):
    pass


def _alarm(*_):
    raise Timeout()


def make(config, dtype, dev):
    m = rc.make_plain_module(True, dev, True)
    m.fused_raw_grad = False
    m.output_dtype = None if dtype is torch.float32 else dtype
    m.output_memory_format = CL if config == 'nhwc' else None
    return m


def one_step(config, m, raw, cot, cot_cl):
    for p in m.parameters():
        p.grad = None
    if config == 'planar':
        m(raw).backward(cot)
    elif config == 'nhwc':
        m(raw).backward(cot_cl)
    else:
        m(raw).contiguous(memory_format=CL).backward(cot_cl)


def window_ms(config, m, raw, cot, cot_cl, n):
    """ms per step over one timed window of n steps"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        one_step(config, m, raw, cot, cot_cl)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def kernel_us(lib, config, m, raw, cot, cot_cl, n):
    """{kernel: mean us per launch} of the three families from the library's event timer over n steps"""
    torch.cuda.synchronize()
    lib.r2l_timing_enable(1)
    try:
        for _ in range(n):
            one_step(config, m, raw, cot, cot_cl)
        torch.cuda.synchronize()
        buf = ctypes.create_string_buffer(1 << 14)
        lib.r2l_timing_report(buf, len(buf))
    finally:
        lib.r2l_timing_enable(0)
    out = {}
    for line in buf.value.decode().splitlines():
        name, count, ms = line.split()
        for fam in KERNELS:
            if name.startswith('r2l_launch_' + fam):
                out[name[len('r2l_launch_'):-len('_kernel')]] = round(1e3 * float(ms) / int(count), 2)
    return out


def inputs(B, H, W, dtype, dev):
    raw = torch.from_numpy(orc.synth_raw(B, H, W, seed=1, kind='scene')).to(dev)
    cot = torch.from_numpy(np.random.default_rng(1).standard_normal((B, 3, H, W)).astype(np.float32)).to(dev).to(dtype)
    return raw, cot, cot.contiguous(memory_format=CL)


def traffic(kind, steps=3):
    dev = 'cuda'
    raw, cot, cot_cl = inputs(64, 512, 512, torch.float32, dev)
    m = make(kind, torch.float32, dev)
    for _ in range(steps):
        one_step(kind, m, raw, cot, cot_cl)
    torch.cuda.synchronize()
    print(json.dumps(dict(traffic=kind, steps=steps, shape=[64, 512, 512])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=400)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--shapes', default='512,256')
    ap.add_argument('--limit', type=int, default=360)
    ap.add_argument('--out', default=None)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--traffic', choices=('planar', 'nhwc'), default=None)
    args = ap.parse_args()
    if args.traffic:
        return traffic(args.traffic)
    dev = 'cuda'
    rng = random.Random(args.seed)
    rows = []
    signal.signal(signal.SIGALRM, _alarm)
    signal.alarm(args.limit)
    try:
        for H in [int(s) for s in args.shapes.split(',')]:
            for dtype, tag in ((torch.float32, 'float32'), (torch.bfloat16, 'bfloat16')):
                B, W = 64, H
                raw, cot, cot_cl = inputs(B, H, W, dtype, dev)
                ms = {c: make(c, dtype, dev) for c in CONFIGS}
                for c in CONFIGS:
                    window_ms(c, ms[c], raw, cot, cot_cl, 10)       # pre-roll
                meds = {c: [] for c in CONFIGS}
                for _ in range(args.rounds):
                    order = list(CONFIGS)
                    rng.shuffle(order)
                    for c in order:
                        meds[c].append(window_ms(c, ms[c], raw, cot, cot_cl, args.steps))
                lib = _lib.library_for(raw)[0]
                med = {c: statistics.median(meds[c]) for c in CONFIGS}
                row = dict(shape=[B, H, W], dtype=tag, bn='train', steps=args.steps * args.rounds, rounds=args.rounds,
                           step_ms={c: dict(median=round(med[c], 4), rounds=[round(min(meds[c]), 4), round(max(meds[c]), 4)])
                                    for c in CONFIGS},
                           nhwc_over_planar_plus_conversions=round(med['nhwc'] / med['planar+conv'], 4),
                           intervals_apart=bool(max(meds['nhwc']) < min(meds['planar+conv']) or
                                                min(meds['nhwc']) > max(meds['planar+conv'])),
                           nhwc_over_planar=round(med['nhwc'] / med['planar'], 4),
                           kernel_us={c: kernel_us(lib, c, ms[c], raw, cot, cot_cl, 10) for c in ('planar', 'nhwc')},
                           library_digest=_lib.source_digest(), device=torch.cuda.get_device_name(0))
                rows.append(row)
                print(json.dumps(row), flush=True)
                del ms
    except Timeout:
        print(json.dumps(dict(note=f'time limit of {args.limit} s reached: {len(rows)} (shape, type) rows measured')), flush=True)
    finally:
        signal.alarm(0)
        if args.out:
            with open(args.out, 'w') as f:
                json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
