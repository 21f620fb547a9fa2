"""The host route of the training step's forward (r2l_fwd_plan / r2l_fwd_launch in r2l_api_impl.h) and of the backward's recomputing
BatchNorm-sums pass (r2l_bwd_plan's bnr fields) against the record of the commit before they existed: every launch's kernel, grid,
bands and argument block over the full product of the entries and their switches, every refusal's code and text, and for each route
the launches and the bytes written -- with a workspace of exactly the queried size, under the sanitizers.  No GPU."""
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import fwd_routes_record as rec  # noqa: E402
import lockstep_driver  # noqa: E402

OVERRIDES = ('FWD_TILED', 'FORCE_SPLIT', 'FWD_APPLY_RECOMPUTE', 'FWD_STATS_SPLIT', 'FWD_STATS_STREAM', 'FS_BAND', 'FL_BAND', 'FST_BAND',
             'FA_BAND', 'GRID_FWD', 'BNR_BAND', 'GRID_BNR', 'BWD_PLANES')
IO_SUFFIXES = ('_bf16', '_f16', '_nhwc', '_bf16_nhwc', '_f16_nhwc')


def test_every_forward_call_plans_launches_and_writes_what_the_parent_did():
    """tests/emul/r2l_fwd_routes_lockstep.cpp (tests/lockstep_driver.py: the lock-step emulation's sources + a main,
    -fsanitize=address,undefined, no Python in the process); its output line by line against tests/golden/fwd_routes.txt.  The
    workspace of every run is a malloc block of exactly r2l_isp_workspace_bytes and `out` one of exactly 3 B H W elements: a kernel
    that writes past either is an ASan report"""
    env = {k: v for k, v in os.environ.items() if not k.startswith('R2L_')}
    r = lockstep_driver.run('fwd_routes', env=env, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert 'Sanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr[-3000:]
    got, want = r.stdout.splitlines(), rec.lines()
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f'line {i + 1}:\n  this tree: {g}\n  recorded:  {w}'
    assert len(got) == len(want)
    # the record is whole.  P without an override: 4 x 2 r2l_isp_fwd[_u16] lines of 8 answers, 2 r2l_isp_fwd_stats_bn[_u16] lines of 2,
    # 8 entries x 2 frame types x 5 BatchNorm modes / phases step_fwd lines and 6 x 2 x 3 step_bwd lines of 12 answers each; every
    # override's pass ends in its count of the same 1188 + 432 answers
    plain = [line for line in want if line.startswith('P - ')]
    assert [sum(1 for line in plain if line.startswith('P - ' + k)) for k in ('fwd ', 'stats_bn ', 'step_fwd ', 'step_bwd ')] == [8, 2, 80, 36]
    for line in plain:
        n = sum(int(t.split('*')[1]) if '*' in t else 1 for t in line.split(': ')[1].split())
        assert n == {'fwd': 8, 'stats_bn': 2}.get(line.split()[2], 12), line
    for name in OVERRIDES:
        m = [re.match(r'^P %s=\d+: (\d+) answers as without, (\d+) differ$' % name, line) for line in want]
        m = [x for x in m if x]
        assert len(m) == 1 and int(m[0].group(1)) + int(m[0].group(2)) == 8 * 8 + 2 * 2 + 80 * 12 + 36 * 12 and int(m[0].group(2)) > 0, name
    kinds = {k: sum(1 for line in want if line.startswith(k)) for k in ('R ', 'S ', 'X ')}
    assert kinds['R '] >= 80 and kinds['S '] == kinds['R '] and kinds['X '] >= 110, kinds
    assert all(re.search(r' -> -2 \[r2l_isp_(step_)?fwd: workspace too small( \(r2l_isp_workspace_bytes\))?\] \[\]$', line)
               for line in want if line[0] == 'S')
    assert all(' -> 0 [] [' in line for line in want if line.startswith('R '))
    # every route, every io slot of the three families, both frame types
    tags = {line.split()[1] for line in want if line.startswith('R ')}
    assert {'stream', 'stream_epi', 'split_apply', 'stats_apply', 'stats_only', 'stream_io', 'apply_io', 'tile_ragged', 'tile_exact',
            'tile_additive', 'bnr_io', 'bnr', 'bnr_epi', 'bn_reduce', 'tiled', 'force_split', 'apply_recompute', 'stats_split',
            'stats_stream', 'bands6_grid1', 'bnr_band6_grid1'} <= tags
    ran = set()
    for line in want:
        if line.startswith('R '):
            ran |= {item.split('*')[0] for item in rec.RUN_RE.match(line).group(16).split(',')}
    for u16 in ('', '_u16'):
        wanted = ['fwd_stream_w%d%s' % (w, u16) for w in (1, 2, 4, 8)]
        wanted += ['fwd_stream_stats_w1' + u16, 'fwd_stream_stats_w2' + u16, 'fwd_stream_epi_w1' + u16, 'fwd_stream_epi_w2' + u16]
        wanted += ['fwd_luma' + u16, 'fwd_stats' + u16, 'fwd_apply' + u16, 'fwd_apply_epi' + u16, 'bnr_planes' + u16, 'bnr_planes_epi' + u16]
        wanted += ['fwd' + u16, 'fwd_ragged' + u16, 'fwd_add_exact' + u16]
        for sfx in IO_SUFFIXES:
            wanted += ['fwd_stream_w1' + u16 + sfx, 'fwd_apply' + u16 + sfx, 'bnr_planes' + u16 + sfx]
        assert set(wanted) <= ran, sorted(set(wanted) - ran)
    assert {'fwd_stream_stats_w4_u16', 'fwd_stream_stats_w8'} <= ran
    assert os.path.getsize(rec.GOLDEN) < 200 * 1000
