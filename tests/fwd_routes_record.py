"""tests/golden/fwd_routes.txt: what every forward call of tests/emul/r2l_fwd_routes_lockstep.cpp planned, launched and wrote on the
PARENT of the commit that introduced r2l_fwd_plan (tests/README.md: how it is regenerated).  Readers of its lines."""
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'fwd_routes.txt')

RUN_RE = re.compile(r'^R (\S+) n(\d) u(\d) (\d+)x(\d+)x(\d+) bn(\d) p(\d+) io(\d) l(\d) a(\d) f(\d+) ws (\d+) -> (-?\d+) \[(.*?)\] \[(.*?)\] \{(.*?)\} ')
OVERRIDE_TAGS = ('bnr', 'bnr_epi', 'bnr_no_luma', 'tiled', 'force_split', 'apply_recompute', 'stats_split', 'stats_stream',
                 'bands6_grid1', 'bnr_band6_grid1')


def lines():
    with open(GOLDEN) as f:
        return f.read().splitlines()


def runs():
    """{(entry, raw_u16, (B, H, W), bn_mode, phase, io, layout, additive, flags): dict(tag, workspace, code, launches)} of the R lines
    without an override of the diagnostic build.  entry: 0 r2l_isp_fwd[_u16] with out and stats, 1 r2l_isp_step_fwd_layout,
    2 r2l_isp_step_bwd_layout behind a whole step's forward (the launches of the backward alone); flags: the R2L_F_* of entry 0;
    launches: {kernel: count}"""
    out = {}
    for line in lines():
        m = RUN_RE.match(line)
        if not m or m.group(1) in OVERRIDE_TAGS:
            continue
        tag, entry, u16, B, H, W, bn, phase, io, layout, add, flags, ws, code, _, rec, _ = m.groups()
        launches = {'r2l_launch_%s_kernel' % k: int(v) for k, v in (item.split('*') for item in rec.split(',') if item)}
        key = (int(entry), int(u16), (int(B), int(H), int(W)), int(bn), int(phase), int(io), int(layout), int(add), int(flags))
        out.setdefault(key, dict(tag=tag, workspace=int(ws), code=int(code), launches=launches))
    return out
