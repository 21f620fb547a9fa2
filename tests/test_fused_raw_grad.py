"""d/d raw on the fused kernels (ParametrizedProcessing.fused_raw_grad, r2l_isp_step_bwd_raw) on the CPU.

The new passes only exist in the device form (the plane passes), so the checks of tests/raw_grad_checks.py run on the lock-step
emulation under ASan + UBSan in a subprocess, as tests/test_lockstep.py does: fused grad_raw against the reference's golden
grad_raw, against the float64 oracle on border-heavy shapes with short bands, the black-level identity, and bit-identical
outputs / parameter gradients with and without d/d raw.  The routing checks (the opt-in, unsupported frames, the serial
emulation's -3) run in-process on the serial emulation."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import conftest  # noqa: E402
import test_distributed as td  # noqa: E402
from oracle import isp_oracle as orc  # noqa: E402
from raw2logit_amd import _lib  # noqa: E402
from raw2logit_amd.processing import pipeline_torch as ppt  # noqa: E402

REPO = os.path.dirname(HERE)


def _asan_runtime():
    p = subprocess.run(['gcc', '-print-file-name=libasan.so'], capture_output=True, text=True).stdout.strip()
    return p if os.path.isabs(p) and os.path.exists(p) else None


@pytest.fixture(scope='module')
def lockstep_lib():
    if _asan_runtime() is None:
        pytest.skip('no libasan.so next to gcc')
    return conftest.build_lockstep()


def _asan_env(**extra):
    return conftest.cpu_only_env(dict(os.environ, LD_PRELOAD=_asan_runtime(), ASAN_OPTIONS='detect_leaks=0:abort_on_error=0',
                                      UBSAN_OPTIONS='print_stacktrace=1:halt_on_error=1', OMP_NUM_THREADS='1', **extra))


@pytest.mark.parametrize('groups', [('golden',), ('oracle', 'identity'), ('bitwise',)], ids=['golden', 'oracle+identity',
                                                                                          'bitwise'])
def test_fused_raw_grad_on_the_lock_step_emulation(groups, lockstep_lib):
    r = subprocess.run([sys.executable, os.path.join(HERE, 'raw_grad_checks.py'), lockstep_lib, *groups],
                       env=_asan_env(), capture_output=True, text=True, timeout=3000)
    out = r.stdout + r.stderr
    assert 'AddressSanitizer' not in out and 'runtime error' not in out, out[-6000:]
    assert r.returncode == 0, out[-6000:]
    last = [ln for ln in r.stdout.splitlines() if 'raw-grad checks passed' in ln]
    assert last and 'FAILED' not in last[-1], out[-6000:]
    print(last[-1])


def test_default_routing_keeps_the_staged_kernels_for_frames_requiring_grad():
    assert ppt.ParametrizedProcessing.fused_raw_grad is False
    assert ppt.ParametrizedProcessing(orc.DRONE_CAMERA_PARAMS).fused_raw_grad is False


def test_opt_in_sends_unsupported_frames_to_the_staged_kernels(emulation):
    """fused_raw_grad=True, frames the fused d/d raw does not serve (W % 4 != 0, an additive layer): the stage-by-stage kernels
    run, and grad_raw is theirs -- bit-identical to the default routing, and equal to the float64 oracle (W % 4 != 0)"""
    for shape, additive in (((2, 8, 18), False), ((1, 256, 256), True)):
        B, H, W = shape
        raw_np = orc.synth_raw(B, H, W, seed=11, kind='scene')
        cot = np.random.default_rng(11).standard_normal((B, 3, H, W)).astype(np.float32)
        grads = []
        for opt_in in (False, True):
            m = ppt.ParametrizedProcessing(orc.DRONE_CAMERA_PARAMS, batch_norm_output=True).train()
            if additive:
                ppt.append_additive_layer(m)
            m.fused_raw_grad = opt_in
            raw = torch.from_numpy(raw_np).requires_grad_(True)
            y = m(raw)
            assert not isinstance(m.stages, ppt._LazyStages)      # the staged kernels filled the stages during the call
            (y * torch.from_numpy(cot)).sum().backward()
            grads.append(raw.grad.numpy().copy())
        assert np.array_equal(grads[0], grads[1])
        if not additive:
            P64 = orc.IspParams(orc.DRONE_CAMERA_PARAMS, dtype=np.float64)
            _, _, cache = orc.parametrized_forward(raw_np, P64, bn=dict(training=True, running_mean=np.zeros(3),
                                                                        running_var=np.ones(3)))
            ref = orc.parametrized_backward(P64, cache, cot)[1]
            assert np.abs(grads[1] - ref).max() <= 2 * 1.5e-3 * np.abs(ref).max() + 1e-6


def test_serial_emulation_refuses_fused_raw_grad_with_a_reason(emulation):
    """the serial build has no plane passes: r2l_isp_step_bwd_raw returns -3 and says why"""
    m = ppt.ParametrizedProcessing(orc.DRONE_CAMERA_PARAMS, batch_norm_output=True).train()
    m.fused_raw_grad = True
    raw = torch.from_numpy(orc.synth_raw(1, 8, 16, seed=2, kind='scene')).requires_grad_(True)
    y = m(raw)
    assert isinstance(m.stages, ppt._LazyStages)
    with pytest.raises(_lib.R2LError, match=r'\(-3\).*plane passes'):
        y.sum().backward()


def _rank_worker(rank, world, port, lib_path, out_dir):
    import torch.distributed as dist
    sys.path.insert(0, REPO)
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    sys.path.insert(0, HERE)
    import emul_hook
    emul_hook.enable(lib_path)
    torch.set_num_threads(1)
    B, H, W = 4, 12, 264
    raw_np = orc.synth_raw(B, H, W, seed=3, kind='scene')
    cot = torch.from_numpy(np.random.default_rng(7).standard_normal((B, 3, H, W)).astype(np.float32))
    lo, hi = rank * B // world, (rank + 1) * B // world

    def step(frames, c, group):
        m = ppt.ParametrizedProcessing(orc.DRONE_CAMERA_PARAMS, batch_norm_output=True).train()
        m.fused_raw_grad = True
        m.process_group = group
        raw = torch.from_numpy(frames).requires_grad_(True)
        y = m(raw)
        assert isinstance(m.stages, ppt._LazyStages)
        (y * c).sum().backward()
        return raw.grad.numpy()
    g = step(raw_np[lo:hi].copy(), cot[lo:hi], dist.group.WORLD)
    res = dict(g=g)
    if rank == 0:
        res['full'] = step(raw_np, cot, None)     # the whole batch in one process
    np.savez(os.path.join(out_dir, f'rank{rank}.npz'), **res)
    dist.destroy_process_group()


def test_two_gloo_ranks_split_the_fused_raw_grad(lockstep_lib, tmp_path):
    """train-mode BatchNorm over two gloo ranks (phase A / all-gather / phase B on both calls): each rank's grad_raw equals its
    slice of the single-process result on the whole batch"""
    import torch.multiprocessing as mp
    world = 2
    add = conftest.cpu_only_env(dict(LD_PRELOAD=_asan_runtime(), ASAN_OPTIONS='detect_leaks=0',
                                     UBSAN_OPTIONS='print_stacktrace=1:halt_on_error=1', OMP_NUM_THREADS='1'))
    old = {k: os.environ.get(k) for k in add}
    os.environ.update(add)
    try:
        mp.spawn(_rank_worker, args=(world, td._free_port(), lockstep_lib, str(tmp_path)), nprocs=world, join=True)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    r = [np.load(os.path.join(str(tmp_path), f'rank{k}.npz')) for k in range(world)]
    full = r[0]['full']
    got = np.concatenate([r[0]['g'], r[1]['g']])
    assert np.abs(got - full).max() <= 1e-5 * np.abs(full).max()
