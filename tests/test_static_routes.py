"""The static chains' host route (r2l_static_plan / r2l_static_launch in r2l_api_impl.h) against the record of the commit before
it existed: every answer of the workspace and 16-bit queries, every refusal's code and text, and for each route the launches and
the output bytes -- with a workspace of exactly the queried size, under the sanitizers.  No GPU."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import static_routes_record as rec  # noqa: E402

BUILD = os.path.join(HERE, '_build')
SANITIZE = ['-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-fno-omit-frame-pointer', '-g']


def test_every_static_call_answers_launches_and_writes_what_the_parent_did():
    """tests/emul/r2l_static_routes_lockstep.cpp: the lock-step emulation's sources + a main, -fsanitize=address,undefined, no Python
    in the process; its output line by line against tests/golden/static_routes.txt.  The workspace of every run is a malloc block of
    exactly r2l_static_workspace_bytes_opts: a kernel that writes past what the query reported is an ASan report.  -O0 like the
    lock-step library: the optimiser needs many minutes for these sources under the sanitizers"""
    src = os.path.join(HERE, 'emul', 'r2l_static_routes_lockstep.cpp')
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, 'r2l_static_routes_lockstep')
    csrc = os.path.join(REPO, 'raw2logit_amd', 'csrc')
    deps = [src, os.path.join(HERE, 'emul', 'r2l_lockstep.cpp'), os.path.join(HERE, 'emul', 'r2l_lockstep_rt.h'),
            os.path.join(REPO, 'include', 'r2l_isp.h')] + [os.path.join(csrc, f) for f in os.listdir(csrc)]
    if not (os.path.exists(exe) and all(os.path.getmtime(exe) >= os.path.getmtime(d) for d in deps)):
        tmp = exe + f'.{os.getpid()}.tmp'
        subprocess.run(['g++', '-std=c++17', '-O0', *SANITIZE, '-I' + os.path.join(HERE, 'emul'), src, '-o', tmp], check=True)
        os.replace(tmp, exe)
    env = {k: v for k, v in os.environ.items() if not k.startswith('R2L_')}
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    got, want = r.stdout.splitlines(), rec.lines()
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f'line {i + 1}:\n  this tree: {g}\n  recorded:  {w}'
    assert len(got) == len(want)
    # the record is whole: the full product of the queries with and without R2L_STATIC_TILED (3 frame kinds x 3 x 3 x 4 chains x 3
    # median sizes lines of 5 widths x 2 batches each), every route run, every workspace route with one byte less, the refusals
    kinds = {k: sum(1 for line in want if line.startswith(k)) for k in ('Q0 ', 'Q1 ', 'R ', 'S ', 'X ')}
    assert kinds['Q0 '] == kinds['Q1 '] == 324 and all(line.count(',') == 30 for line in want if line[0] == 'Q')
    assert kinds['R '] >= 200 and kinds['S '] >= 40 and kinds['X '] >= 130, kinds
    assert all(' -> -2 [r2l_static_fwd: workspace too small (r2l_static_workspace_bytes)] [] ' in line for line in want if line[0] == 'S')
    routes = {line.split()[1] for line in want if line.startswith('R ')}
    assert {'menon', 'chain', 'planes', 'full', 'stream', 'short', 'chain_band2', 'stream_bands4', 'tiled'} <= routes
    assert os.path.getsize(rec.GOLDEN) < 200 * 1000
