"""What the statistics-only form of the static kernels saves (functional.static_statistics / r2l_static_stats): the channel sums of
a chain's output, timed with HIP events at 256x1024x1024 and 1024x512x512 on float32 and 16-bit-container frames for the short
bilinear chain, the short Malvar2004 chain and the default chain, in three configurations:
    stats           static_statistics: one statistics-only launch and the one-workgroup finish, no output;
    pipeline        static_pipeline alone: the same loads and arithmetic, and the 12 B/px store -- what `stats` must not exceed;
    pipeline+torch  static_pipeline followed by torch.var_mean over (0, 2, 3): what a caller without `stats` pays.
All configurations live in one process on the same frames and alternate in RANDOM order (seeded): rounds of --steps calls each
after a pre-roll of all.  A round is ONE timed window (one pair of events around its calls); per configuration the median of the
rounds' figures and the lowest and highest of them -- the interval to compare.  --caps 768,1536 adds `stats` on the diagnostic
build with the statistics launches capped at that many workgroups (R2L_GRID_STATIC) instead of the product's 2048.  Prints one JSON
line per cell and, with --out, writes them to a JSON file (profiles/static_stats.json).  Run it under a limit from outside too:

    timeout -k 10 400 python tests/bench_static_stats.py [--steps 30] [--rounds 7] [--limit 360] [--out FILE]"""
import argparse
import json
import os
import random
import signal
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import torch  # noqa: E402

import half_io_checks as hc  # noqa: E402
import parity_checks as pc  # noqa: E402
import static_half_checks as sh  # noqa: E402
from oracle import isp_oracle as orc  # noqa: E402
from raw2logit_amd import _lib  # noqa: E402
from raw2logit_amd import functional as F_  # noqa: E402

CHAINS = (('bilinear_short', sh.SHORT_BILINEAR), ('malvar_short', sh.SHORT_MALVAR), ('default', sh.DEFAULT_CHAIN))
SHAPES = ((256, 1024, 1024), (1024, 512, 512))
CAM = orc.DRONE_CAMERA_PARAMS


class Timeout(Exception):
    pass


def _alarm(*_):
    raise Timeout()


def call(config, raw, chain):
    if config.startswith('stats'):
        return F_.static_statistics(raw, CAM, *chain)
    out = F_.static_pipeline(raw, CAM, *chain)
    return torch.var_mean(out, dim=(0, 2, 3)) if config == 'pipeline+torch' else out


def window_ms(config, raw, chain, n):
    """ms per call over one timed window of n calls"""
    cap = config.split('@')[1] if '@' in config else None
    with (pc.env_overrides('cuda', dict(R2L_GRID_STATIC=cap)) if cap else pc.env_overrides('cpu', {})):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            call(config, raw, chain)
        b.record()
        b.synchronize()
    return a.elapsed_time(b) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--limit', type=int, default=360)
    ap.add_argument('--caps', default='')
    ap.add_argument('--out', default=None)
    ap.add_argument('--seed', type=int, default=0)
    args = ap.parse_args()
    configs = ['stats', 'pipeline', 'pipeline+torch'] + [f'stats@{int(c)}' for c in args.caps.split(',') if c]
    rng = random.Random(args.seed)
    rows = []
    signal.signal(signal.SIGALRM, _alarm)
    signal.alarm(args.limit)
    try:
        for B, H, W in SHAPES:
            for u16 in (False, True):
                # (one image of synthetic scene, repeated: the kernels' time does not depend on the values)
                raw = hc.frames(1, H, W, 1, 'cuda', u16=u16).expand(B, H, W).contiguous()
                for tag, chain in CHAINS:
                    assert F_.static_stats_why(raw, *chain) is None
                    for c in configs:
                        window_ms(c, raw, chain, 3)       # pre-roll
                    ms = {c: [] for c in configs}
                    for _ in range(args.rounds):
                        order = list(configs)
                        rng.shuffle(order)
                        for c in order:
                            ms[c].append(window_ms(c, raw, chain, args.steps))
                    med = {c: statistics.median(ms[c]) for c in configs}
                    px = B * H * W
                    row = dict(shape=[B, H, W], frames='uint16' if u16 else 'float32', chain=tag, calls=args.steps * args.rounds,
                               rounds=args.rounds,
                               call_ms={c: dict(median=round(med[c], 4), rounds=[round(min(ms[c]), 4), round(max(ms[c]), 4)])
                                        for c in configs},
                               stats_over_pipeline=round(med['stats'] / med['pipeline'], 4),
                               stats_at_or_below_pipeline=bool(max(ms['stats']) <= max(ms['pipeline'])),
                               stats_over_pipeline_plus_torch=round(med['stats'] / med['pipeline+torch'], 4),
                               stats_read_GBps=round((2 if u16 else 4) * px / med['stats'] / 1e6, 1),
                               library_digest=_lib.source_digest(), device=torch.cuda.get_device_name(0))
                    rows.append(row)
                    print(json.dumps(row), flush=True)
                del raw
    except Timeout:
        print(json.dumps(dict(note=f'time limit of {args.limit} s reached: {len(rows)} cells measured')), flush=True)
    finally:
        signal.alarm(0)
        if args.out:
            with open(args.out, 'w') as f:
                json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
