"""The static chains' host route (r2l_static_plan / r2l_static_launch in r2l_api_impl.h) against the record of the commit before
it existed: every answer of the workspace and 16-bit queries, every refusal's code and text, and for each route the launches and
the output bytes -- with a workspace of exactly the queried size, under the sanitizers.  No GPU."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import lockstep_driver  # noqa: E402
import static_routes_record as rec  # noqa: E402


def test_every_static_call_answers_launches_and_writes_what_the_parent_did():
    """tests/emul/r2l_static_routes_lockstep.cpp (tests/lockstep_driver.py: the lock-step emulation's sources + a main,
    -fsanitize=address,undefined, no Python in the process); its output line by line against tests/golden/static_routes.txt.  The
    workspace of every run is a malloc block of exactly r2l_static_workspace_bytes_opts: a kernel that writes past what the query
    reported is an ASan report"""
    env = {k: v for k, v in os.environ.items() if not k.startswith('R2L_')}
    r = lockstep_driver.run('static_routes', env=env, timeout=900)
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
