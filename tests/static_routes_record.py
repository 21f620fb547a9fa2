"""tests/golden/static_routes.txt: what every static call of tests/emul/r2l_static_routes_lockstep.cpp answered, launched and wrote
on the PARENT of the commit that introduced r2l_static_plan (tests/README.md: how it is regenerated).  Readers of its lines."""
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'static_routes.txt')

RUN_RE = re.compile(r'^R (\S+) f(\d) io(\d) (\d+)x(\d+)x(\d+) (\d)(\d)(\d) (\S+) n(\d) ws (\d+) -> (-?\d+) \[(.*?)\] \[(.*?)\] ([0-9a-f]{16})$')


def lines():
    with open(GOLDEN) as f:
        return f.read().splitlines()


def runs():
    """{(frames, io, (B, H, W), (debayer, sharpening, denoising), median): dict(norm, workspace, code, launches)} of the R lines
    without an override of the diagnostic build (the first line of a key)"""
    out = {}
    for line in lines():
        m = RUN_RE.match(line)
        if not m or m.group(1) in ('chain_band2', 'stream_bands4', 'grid1', 'tiled'):
            continue
        tag, frames, io, B, H, W, deb, shp, dn, med, norm, ws, code, _, rec, _ = m.groups()
        launches = {k: int(v) for k, v in (item.split('*') for item in rec.split(',') if item)}
        key = (int(frames), int(io), (int(B), int(H), int(W)), (int(deb), int(shp), int(dn)), float(med))
        out.setdefault(key, dict(route=tag, norm=bool(int(norm)), workspace=int(ws), code=int(code), launches=launches))
    return out
