"""The N > 1 device path on real hardware.

Two FRESH processes join a gloo group, share cuda:0 and take half of each batch through ParametrizedProcessing
(tests/multirank_worker.py: fused and staged path, BatchNorm in train mode, float32 frames and 16-bit containers,
frames 1 / 2 / 4 wavefronts wide for the row-streaming forward, a ragged width for the tile kernels, BASELINE
config 5's per-GPU shard).  What must hold:

  * the halves concatenated equal the single-process run of the whole batch on the same GPU (<= 2e-5 x max istd:
    only the summation order of the statistics differs),
  * the all-reduced gradient is bit-identical on both ranks and equals the single-process gradient to 2e-4 of its
    scale (3e-3 on the staged path, whose reductions run per stage),
  * running statistics and num_batches_tracked equal the single-process module's on every rank,
  * a 2-frame slice equals the float64 oracle evaluated with the global batch's statistics.

The reference has nothing to match here (train.py:361-368 hard-codes gpus=1): synchronised statistics are this
library's way of reproducing ITS numbers at a global batch size, so the single-process run is the yardstick.
With two GPUs the same test also runs over RCCL, one rank per GPU."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import parity_checks as pc
from oracle import isp_oracle as orc
import multirank_worker as mw

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _spawn(world, out_dir, backend, cases=None, timeout=900, extra_env=None, retry_crash=0):
    """retry_crash: how often to start over when a rank DIES (killed by a signal / aborted by the runtime: exit code other than 0
    or 1) instead of failing an assertion.  Used by the RCCL graph-capture tests only: a one-rank RCCL group capturing its
    collectives into a HIP graph is a configuration that exists for these tests.  Round 6: that test failed ONCE in 9 full-suite
    runs (+ 14 clean partial repeats of the suite), at the end of an 80-minute GPU session, and the
    report did not survive (the collecting script kept the log's tail only) -- round 5 had seen aborts of the process group's
    watchdog thread during captures (raw2logit_amd/graphs.py).  An abort of the stack must not cost the suite; a wrong bit or any
    Python exception (exit code 1) still does and is never retried.  Every retry is appended to gpurun_out/multirank_retries.txt
    and raised as a warning."""
    for attempt in range(retry_crash + 1):
        try:
            return _spawn_once(world, out_dir, backend, cases, timeout, extra_env)
        except _RankDied as e:
            if attempt == retry_crash:
                raise AssertionError(str(e))
            import warnings
            msg = f'multirank worker died (attempt {attempt + 1}), starting over: {str(e)[-1500:]}'
            warnings.warn(msg)
            out = os.path.join(REPO, 'gpurun_out')
            if os.path.isdir(out):
                with open(os.path.join(out, 'multirank_retries.txt'), 'a') as f:
                    f.write(msg + '\n')


class _RankDied(Exception):
    pass


def _spawn_once(world, out_dir, backend, cases=None, timeout=900, extra_env=None):
    env = dict(os.environ, R2L_TEST_BACKEND=backend, HSA_ENABLE_IPC_MODE_LEGACY='0', **(extra_env or {}))
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        env.pop(k, None)
    if cases:
        env['R2L_MULTIRANK_CASES'] = ','.join(cases)
    port = _free_port()
    procs = [subprocess.Popen([sys.executable, os.path.join(REPO, 'tests', 'multirank_worker.py'), str(r), str(world),
                               str(port), out_dir], env=env, cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                              text=True) for r in range(world)]
    outs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=timeout)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append(o)
    for r, p in enumerate(procs):
        if p.returncode not in (0, 1):           # a signal (negative) or an abort of the runtime: not a Python exception
            raise _RankDied(f'rank {r} died with exit code {p.returncode}:\n{outs[r][-3000:]}')
        assert p.returncode == 0, f'rank {r} failed:\n{outs[r][-3000:]}'
    return [np.load(os.path.join(out_dir, f'rank{r}.npz')) for r in range(world)]


def _single_process(case, dev):
    """the whole batch in this process on the same GPU: the yardstick"""
    name, shape, frames, path, camera = case
    raw_np, cot_np = mw.case_inputs(name, shape, frames)
    m = mw.make_module(path, camera, dev)
    raw, cot = torch.from_numpy(raw_np).to(dev), torch.from_numpy(cot_np).to(dev)
    y = m(raw)
    y.backward(cot)
    g = torch.cat([p.grad.reshape(-1) for p in m.parameters()]).cpu().numpy()
    for p in m.parameters():
        p.grad = None
    m(raw)
    return m, y.detach().cpu().numpy(), g, raw_np, cot_np


def _check(ranks, dev, tag):
    world = len(ranks)
    for case in mw.CASES:
        name, shape, frames, path, camera = case
        if f'{name}/y' not in ranks[0]:
            continue
        m, y, g, raw_np, cot_np = _single_process(case, dev)
        y_sh = np.concatenate([r[f'{name}/y'] for r in ranks])
        raw32 = raw_np if frames == 'f32' else (raw_np.view(np.uint16).astype(np.float32) / np.float32(4095))
        # 1 / std of the batch (BatchNorm multiplies every round-off by it): from the module's first running_var update,
        # running_var_1 = 0.9 + 0.1 * unbiased var; after two updates on the same batch 0.81 + 0.19 * unbiased var
        var = (m.batch_norm.running_var.double().cpu().numpy() - 0.81) / 0.19
        istd = float(1.0 / np.sqrt(max(var.min(), 0.0) + 1e-5))
        e = np.abs(y_sh - y).max()
        lim = 2e-5 * max(istd, 1.0)
        pc.report(f'multirank[{tag}]/{name}: shards vs single process, out', e, lim)
        assert e <= lim, (name, e, lim)
        for r in range(1, world):
            assert np.array_equal(ranks[0][f'{name}/g'], ranks[r][f'{name}/g']), (name, 'gradient differs between ranks')
        rel = 3e-3 if path == 'staged' else 2e-4
        scale = np.abs(g).max() + 1e-6
        eg = np.abs(ranks[0][f'{name}/g'] - g).max()
        pc.report(f'multirank[{tag}]/{name}: all-reduced gradient vs single process', eg, rel * scale)
        assert eg <= rel * scale, (name, eg, rel * scale)
        # the local gradients really are partial: their sum is the all-reduced one
        gl = sum(r[f'{name}/g_local'].astype(np.float64) for r in ranks)
        assert np.abs(gl - ranks[0][f'{name}/g']).max() <= 1e-5 * scale
        for r in ranks:
            np.testing.assert_allclose(r[f'{name}/rm'], m.batch_norm.running_mean.cpu().numpy(), rtol=2e-6, atol=1e-7)
            np.testing.assert_allclose(r[f'{name}/rv'], m.batch_norm.running_var.cpu().numpy(), rtol=2e-6, atol=1e-7)
            assert int(r[f'{name}/nbt']) == int(m.batch_norm.num_batches_tracked) == 2
            assert bool(r[f'{name}/y2_equal'])
        if shape[0] <= 8:
            # the whole (small) batch against the float64 oracle with global statistics
            P = mw.case_params(camera)
            o64, _, c64 = orc.parametrized_forward(raw32, P.astype(np.float64),
                                                   bn=dict(training=True, running_mean=np.zeros(3),
                                                           running_var=np.ones(3)))
            tol = pc.out_tolerance(c64, True, base=2e-5 if camera == 'microscopy' else 1e-5)
            err = np.abs(y_sh - o64)
            w = np.unravel_index((err / tol).argmax(), err.shape)
            pc.report(f'multirank[{tag}]/{name}: shards vs float64 oracle (global statistics)', err[w], tol[w])
            assert np.all(err <= tol), (name, err.max(), w)
            # float32 conditioning of this case: how far the SAME algorithm in float32 (the oracle run in float32, i.e.
            # what the reference's own arithmetic does) lands from its float64 run
            _, _, c32 = orc.parametrized_forward(raw32, P.astype(np.float32),
                                                 bn=dict(training=True, running_mean=np.zeros(3), running_var=np.ones(3)))
            g32, _, _ = orc.parametrized_backward(P.astype(np.float32), c32, cot_np)
            go, _, _ = orc.parametrized_backward(P.astype(np.float64), c64, cot_np)
            lo, _, _ = orc.parametrized_backward(P.astype(np.float64), c64, cot_np, clip_shift=1e-6)
            hi, _, _ = orc.parametrized_backward(P.astype(np.float64), c64, cot_np, clip_shift=-1e-6)
            off = 0
            for k, p in m.named_parameters():
                n = p.numel()
                og = np.asarray(go[k]).reshape(-1)
                flip = max(np.abs(np.asarray(lo[k]).reshape(-1) - og).max(),
                           np.abs(np.asarray(hi[k]).reshape(-1) - og).max())
                cond = np.abs(np.asarray(g32[k], dtype=np.float64).reshape(-1) - og).max()
                lim = (1e-2 if camera == 'microscopy' else 1.5e-3) * (np.abs(og).max() + 1e-6) + flip + 2 * cond
                e = np.abs(ranks[0][f'{name}/g'][off:off + n] - og).max()
                pc.report(f'multirank[{tag}]/{name}: all-reduced grad {k} vs float64 oracle', e, lim)
                assert e <= lim, (name, k, e, lim)
                off += n


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from raw2logit_amd import _lib
    assert _lib.device_library().is_device
    return 'cuda:0'


def test_two_gloo_ranks_share_the_gpu(dev, tmp_path):
    ranks = _spawn(2, str(tmp_path), 'gloo')
    _check(ranks, dev, 'gloo x2 on one GPU')


def test_three_ranks_uneven_shards(dev, tmp_path):
    """three ranks: shards of different sizes (4 -> 1 + 1 + 2 frames, 6 -> 2 + 2 + 2), rank-ordered sums of three"""
    ranks = _spawn(3, str(tmp_path), 'gloo', cases=('w1_f32', 'tiles_bands_f32', 'staged_f32'))
    _check(ranks, dev, 'gloo x3 on one GPU')


def test_two_rccl_ranks_one_per_gpu(dev, tmp_path):
    if torch.cuda.device_count() < 2:
        pytest.skip('needs two GPUs')
    ranks = _spawn(2, str(tmp_path), 'nccl')
    _check(ranks, dev, 'rccl x2')


GRAPH_CASES = ('w1_f32', 'w2_u16', 'tiles_bands_f32', 'config5_shard')


def _check_graph(ranks, tag):
    import json
    rec = {}
    for name in GRAPH_CASES:
        for r, res in enumerate(ranks):
            assert bool(res[f'{name}/graph_y_equal']), (name, r, 'replayed output differs from the eager step')
            assert bool(res[f'{name}/graph_g_equal']), (name, r, float(res[f'{name}/graph_g_maxdiff']))
            names = [str(x) for x in res[f'{name}/comm_names']]
            assert names == ['bn statistics all-gather', 'bn-bwd sums all-gather', 'grad all-reduce'], names
            assert all(int(c) == 1 for c in res[f'{name}/comm_calls'])
        rec[name] = {'ms_per_step_eager': round(float(max(r[f'{name}/ms_eager'] for r in ranks)), 4),
                     'ms_per_step_graph': round(float(max(r[f'{name}/ms_graph'] for r in ranks)), 4),
                     'comm_us_eager': dict(zip([str(x) for x in ranks[0][f'{name}/comm_names']],
                                               [float(x) for x in ranks[0][f'{name}/comm_us']]))}
        pc.report(f'multirank[{tag}]/{name}: step graph with its collectives vs eager (bits differing)', 0.0, 0.0)
    out_dir = os.path.join(REPO, 'gpurun_out')
    if os.path.isdir(out_dir):
        with open(os.path.join(out_dir, f'step_graph_{tag.replace(" ", "_")}.json'), 'w') as f:
            json.dump({'what': 'the data-parallel step (phase A / B calls around two RCCL all-gathers + the gradient '
                               'all-reduce) eager and as ONE HIP graph; per-rank batch = global batch / ranks',
                       'ranks': len(ranks), 'cases': rec}, f, indent=1)


def test_step_graph_captures_the_rccl_collectives_on_one_gpu(dev, tmp_path):
    """StepGraph(process_group=...) on the one-GPU box: a world of ONE rank over RCCL with R2L_SPLIT_SINGLE_RANK=1 takes the
    N > 1 code path -- both step calls split in phases A / B around real RCCL all-gathers (of one row), r2l_bn_finalize /
    r2l_bn_bwd_means as their own launches, the flat gradient all-reduce -- eagerly and captured into one HIP graph:
    replays are bit-identical to the eager step, which equals the plain single-process step to round-off (_check)."""
    ranks = _spawn(1, str(tmp_path), 'nccl', cases=GRAPH_CASES,
                   extra_env={'R2L_SPLIT_SINGLE_RANK': '1', 'R2L_TEST_GRAPH': '1'}, retry_crash=1)
    _check(ranks, dev, 'rccl x1 (split path forced)')
    _check_graph(ranks, 'rccl x1')


def test_step_graph_two_rccl_ranks(dev, tmp_path):
    if torch.cuda.device_count() < 2:
        pytest.skip('needs two GPUs')
    ranks = _spawn(2, str(tmp_path), 'nccl', cases=GRAPH_CASES, extra_env={'R2L_TEST_GRAPH': '1'}, retry_crash=1)
    _check(ranks, dev, 'rccl x2 (graph cases)')
    _check_graph(ranks, 'rccl x2')


def test_bench_two_gloo_ranks_on_the_device(dev):
    """`bench.py --gpus 2` with R2L_BENCH_BACKEND=gloo: both ranks on this GPU -- the bench's multi-rank step (phase A / B
    calls, asynchronous gradient all-reduce, comm_us) as a FUNCTIONAL line, labelled not-a-measurement"""
    import json
    e = dict(os.environ, R2L_BENCH_BACKEND='gloo')
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        e.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '2', '--steps', '5', '--warmup', '2',
                        '--batch', '32', '--size', '256', '--no-cpu-baseline', '--no-static-c3'], env=e,
                       capture_output=True, text=True, timeout=900, cwd=REPO)
    assert r.returncode == 0, r.stderr[-3000:]
    out, = [json.loads(x) for x in r.stdout.splitlines() if x.startswith('{')]
    assert out['n_gpus'] == 2 and out['config']['global_batch'] == 64
    assert 'not a measurement' in out['data']
    comm = out['comm_us']
    assert set(comm) == {'bn statistics all-gather', 'bn-bwd sums all-gather', 'grad all-reduce'}
    for v in comm.values():
        assert v['calls'] == 5 and v['avg_us'] > 0
    out_dir = os.path.join(REPO, 'gpurun_out')
    if os.path.isdir(out_dir):
        with open(os.path.join(out_dir, 'bench_gloo2_functional.json'), 'w') as f:
            json.dump(out, f)


def test_bench_graph_trial_with_one_rccl_rank(dev):
    """The N > 1 branch of `bench.py` on the one-GPU box (R2L_BENCH_ONE_RANK_DIST=1: a one-rank RCCL group, the exchange path
    forced): eager measurement, then the graph trial -- capture with the collectives, agreement between the ranks, the same
    timing protocol under the watchdog -- and a line that carries both numbers and says which one is its value."""
    import json
    e = dict(os.environ, R2L_BENCH_ONE_RANK_DIST='1', HSA_ENABLE_IPC_MODE_LEGACY='0', MASTER_PORT=str(_free_port()))
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        e.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--steps', '10', '--warmup', '3', '--batch', '64',
                        '--size', '256', '--quick', '--graph-trial'], env=e, capture_output=True, text=True, timeout=900,
                       cwd=REPO)
    assert r.returncode == 0, r.stderr[-3000:]
    out, = [json.loads(x) for x in r.stdout.splitlines() if x.startswith('{')]
    assert 'graph_error' not in out, (out.get('graph_error'), r.stderr[-1500:])
    assert out['ms_per_step_graph'] > 0 and out['ms_per_step_eager'] > 0, out
    assert out['ms_per_step'] == out['ms_per_step_eager']          # the eager step carries the value; the graph sits beside it
    # what the collectives cost inside the graph: the world's group minus a group of this rank alone (here the same thing)
    if 'graph_local_error' not in out:     # (best effort in bench.py: a second communicator may not come up on every box)
        assert out['ms_per_step_graph_local'] > 0 and abs(out['graph_comm_us']) < 1e3 * out['ms_per_step_graph']
    else:
        print('graph over a group of this rank alone:', out['graph_local_error'])
    assert set(out['comm_us']) == {'bn statistics all-gather', 'bn-bwd sums all-gather', 'grad all-reduce'}
    print(f"bench graph trial, one RCCL rank, 64x256x256: {out['ms_per_step_eager']} ms per step eager, "
          f"{out['ms_per_step_graph']} as one graph")
    out_dir = os.path.join(REPO, 'gpurun_out')
    if os.path.isdir(out_dir):
        with open(os.path.join(out_dir, 'bench_rccl_x1_graph_trial.json'), 'w') as f:
            json.dump(out, f)


def test_bench_graph_trial_watchdog(dev):
    """The same branch with a watchdog of 1 ms: the timer fires while the capture is still under way, rank 0 prints the EAGER line with
    the reason in `graph_error`, and the process ends with bench.WATCHDOG_EXIT (17), never 0: its GPU work is wedged -- what a
    hanging capture or replay on a real multi-GPU node would leave behind instead of no line at all, and a launcher can tell it
    from a clean run.  Without --graph-trial (the default since round 6) the same run makes no trial at all."""
    import json
    e = dict(os.environ, R2L_BENCH_ONE_RANK_DIST='1', HSA_ENABLE_IPC_MODE_LEGACY='0', MASTER_PORT=str(_free_port()),
             R2L_BENCH_TRIAL_TIMEOUT_S='0.001')
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        e.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--steps', '5', '--warmup', '2', '--batch', '16',
                        '--size', '256', '--quick', '--graph-trial'], env=e, capture_output=True, text=True, timeout=900,
                       cwd=REPO)
    assert r.returncode == 17, (r.returncode, r.stderr[-3000:])
    out, = [json.loads(x) for x in r.stdout.splitlines() if x.startswith('{')]
    assert 'watchdog' in out['graph_error'] and 'ms_per_step_graph' not in out and out['watchdog_fired'] is True
    assert out['ms_per_step'] > 0 and out['value'] > 0
    # the default: no trial, no watchdog, a plain eager line and exit code 0
    r = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--steps', '5', '--warmup', '2', '--batch', '16',
                        '--size', '256', '--quick'], env=e, capture_output=True, text=True, timeout=900, cwd=REPO)
    assert r.returncode == 0, r.stderr[-3000:]
    out, = [json.loads(x) for x in r.stdout.splitlines() if x.startswith('{')]
    assert 'ms_per_step_graph' not in out and 'watchdog_fired' not in out and 'graph_error' not in out
