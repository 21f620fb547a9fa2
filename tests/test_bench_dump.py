"""`bench.py --dump-outputs DIR`: after the timed steps the benchmark writes what its last timed step computed -- the output and
every parameter gradient of the parametrized step -- as DIR/<name>.npy, identically from run to run, so that two builds can be
compared output for output.  Here on the host emulation (R2L_BENCH_DEVICE=emulation), against the same step run in this
process; the sampling of large arrays and the size limit on bench.dump_outputs directly."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, S = 2, 32


def _bench(out_dir, steps='3'):
    import conftest
    env = conftest.cpu_only_env(dict(os.environ, R2L_BENCH_DEVICE='emulation'))
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--steps', steps, '--warmup', '1', '--batch', str(B),
                        '--size', str(S), '--no-roofline', '--no-cpu-baseline', '--dump-outputs', str(out_dir)],
                       env=env, capture_output=True, text=True, timeout=600, cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    out, = [json.loads(x) for x in r.stdout.splitlines() if x.startswith('{')]
    assert out['steps'] == int(steps)
    return {f[:-4]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}


def _bench_step_in_process():
    """the step bench.py times (main(): same inputs, same module), run once here"""
    from raw2logit_amd import cameras
    from raw2logit_amd.processing.pipeline_torch import ParametrizedProcessing
    u16 = np.random.default_rng(0).integers(0, 4096, (B, S, S)).astype(np.uint16)
    raw = torch.from_numpy(u16.astype(np.float32) / np.float32(4095))
    cot = torch.randn((B, 3, S, S), generator=torch.Generator('cpu').manual_seed(1))
    model = ParametrizedProcessing(cameras.DRONE, track_stages=False, batch_norm_output=True).train()
    model.raw_bits = 12
    y = model(raw)
    y.backward(cot)
    return dict({'output': y.detach()}, **{'grad.' + n: p.grad for n, p in model.named_parameters()})


def test_dump_outputs_is_the_last_timed_step_and_repeats(emulation, tmp_path):
    a = _bench(tmp_path / 'a')
    b = _bench(tmp_path / 'b', steps='2')
    want = _bench_step_in_process()
    assert sorted(a) == sorted(b) == sorted(want)
    assert sum(v.nbytes for v in a.values()) <= 64 * 10 ** 6
    for name, w in want.items():
        assert a[name].dtype == np.float32 and a[name].shape == tuple(w.shape), name
        np.testing.assert_array_equal(a[name], b[name], err_msg=name)
        np.testing.assert_allclose(a[name], w.numpy(), rtol=1e-6, atol=1e-7, err_msg=name)


def test_dump_outputs_samples_large_arrays(tmp_path, monkeypatch):
    import bench
    n = bench.DUMP_SAMPLE * 3
    arrays = {'big': torch.arange(n, dtype=torch.float64), 'small': torch.full((2, 3), 0.5, dtype=torch.float16)}
    bench.dump_outputs(str(tmp_path / 'a'), arrays)
    bench.dump_outputs(str(tmp_path / 'b'), arrays)
    big, small = np.load(tmp_path / 'a' / 'big.npy'), np.load(tmp_path / 'a' / 'small.npy')
    assert big.dtype == np.float64 and big.ndim == 1 and 0.5 * bench.DUMP_SAMPLE < big.size <= bench.DUMP_SAMPLE
    assert np.all(np.diff(big) > 0) and big[0] >= 0 and big[-1] < n       # distinct elements, in memory order
    np.testing.assert_array_equal(big, np.load(tmp_path / 'b' / 'big.npy'))
    assert small.dtype == np.float32 and small.shape == (2, 3) and np.all(small == 0.5)
    monkeypatch.setattr(bench, 'DUMP_LIMIT_BYTES', 1000)
    with pytest.raises(SystemExit):
        bench.dump_outputs(str(tmp_path / 'c'), {'x': torch.zeros(1000)})
    assert not os.path.exists(tmp_path / 'c' / 'x.npy')
