"""What the 16-bit output / cotangent saves (ParametrizedProcessing.output_dtype): one step -- forward + backward of the processor with
a fixed cotangent, train-mode BatchNorm -- timed with HIP events at 64x512x512 and 64x256x256 for three variants:
    f32        the float32 step (output_dtype = None), float32 cotangent;
    bf16       output_dtype = torch.bfloat16, bfloat16 cotangent: the kernels write / read the 16-bit tensors themselves;
    f32+casts  the float32 step plus the two casts a mixed-precision caller pays today: out.to(bfloat16) behind the forward and the
               cotangent widened back to float32 by autograd.
The variants alternate in one process (rounds of --steps steps each, rotating order, after a pre-roll of all), the figure is the
median over all rounds' steps with the minimum beside it.  A second pass reads the library's per-kernel timer for the apply pass,
the BatchNorm sums and kernel B1's plane pass.  Prints one JSON line per shape and, with --out, writes them to a JSON file
(profiles/half_io.json).  --limit seconds is a budget the script keeps between steps; run it under a limit from outside as well:

    timeout -k 10 300 python tests/bench_half_io.py [--steps 20] [--rounds 5] [--shapes 512,256] [--limit 270] [--out FILE]"""
import argparse
import ctypes
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

import raw_grad_checks as rc  # noqa: E402
from oracle import isp_oracle as orc  # noqa: E402
from raw2logit_amd import _lib  # noqa: E402

VARIANTS = ('f32', 'bf16', 'f32+casts')
KERNELS = ('fwd_apply', 'bnr_planes', 'bwd1_plane')


class Timeout(Exception):
    pass


def _alarm(*_):
    raise Timeout()


def one_step(variant, m, raw, cot32, cot16):
    for p in m.parameters():
        p.grad = None
    if variant == 'f32':
        m(raw).backward(cot32)
    elif variant == 'bf16':
        m(raw).backward(cot16)
    else:
        m(raw).to(torch.bfloat16).backward(cot16)


def steps_ms(variant, m, raw, cot32, cot16, n):
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        one_step(variant, m, raw, cot32, cot16)
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return ts


def kernel_us(lib, variant, m, raw, cot32, cot16, n):
    """{kernel family: mean us per launch} from the library's event timer over n steps"""
    torch.cuda.synchronize()
    lib.r2l_timing_enable(1)
    try:
        for _ in range(n):
            one_step(variant, m, raw, cot32, cot16)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--shapes', default='512,256')
    ap.add_argument('--limit', type=int, default=270)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    dev = 'cuda'
    rows = []
    signal.signal(signal.SIGALRM, _alarm)
    signal.alarm(args.limit)
    try:
        for H in [int(s) for s in args.shapes.split(',')]:
            B, W = 64, H
            raw = torch.from_numpy(orc.synth_raw(B, H, W, seed=1, kind='scene')).to(dev)
            cot32 = torch.from_numpy(np.random.default_rng(1).standard_normal((B, 3, H, W)).astype(np.float32)).to(dev)
            cot16 = cot32.to(torch.bfloat16)
            cot32 = cot16.float()
            ms = {}
            for v in VARIANTS:
                ms[v] = rc.make_plain_module(True, dev, True)
                ms[v].fused_raw_grad = False
                ms[v].output_dtype = torch.bfloat16 if v == 'bf16' else None
                steps_ms(v, ms[v], raw, cot32, cot16, 5)       # pre-roll
            ts = {v: [] for v in VARIANTS}
            for r in range(args.rounds):
                for i in range(len(VARIANTS)):
                    v = VARIANTS[(i + r) % len(VARIANTS)]
                    ts[v] += steps_ms(v, ms[v], raw, cot32, cot16, args.steps)
            lib = _lib.library_for(raw)[0]
            row = dict(shape=[B, H, W], bn='train', steps=args.steps * args.rounds,
                       step_ms={v: dict(median=round(statistics.median(ts[v]), 4), min=round(min(ts[v]), 4)) for v in VARIANTS},
                       bf16_over_f32=round(statistics.median(ts['bf16']) / statistics.median(ts['f32']), 4),
                       bf16_over_f32_plus_casts=round(statistics.median(ts['bf16']) / statistics.median(ts['f32+casts']), 4),
                       kernel_us={v: kernel_us(lib, v, ms[v], raw, cot32, cot16, 10) for v in ('f32', 'bf16')},
                       library_digest=_lib.source_digest(), device=torch.cuda.get_device_name(0))
            rows.append(row)
            print(json.dumps(row), flush=True)
            del ms
    except Timeout:
        print(json.dumps(dict(note=f'time limit of {args.limit} s reached: {len(rows)} shapes measured')), flush=True)
    finally:
        signal.alarm(0)
        if args.out:
            with open(args.out, 'w') as f:
                json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
