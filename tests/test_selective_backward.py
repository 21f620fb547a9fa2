"""The backward of a subset of the gradients (ParametrizedProcessing.selective_backward, r2l_isp_step_bwd_select) on the CPU.

The reduced passes only exist in the device form (plane passes), so the checks of tests/selective_bwd_checks.py run on the
lock-step emulation under ASan + UBSan in a subprocess, as tests/test_fused_raw_grad.py does: the launch record of every route,
the routes against the full backward and the float64 oracle (golden cases, the plane frame shapes, 4-row frames and partial
strips with short bands, 16-bit frames, the output epilogue), the fall-backs and the unchanged default.  The binding, the module
attribute and the serial emulation's routing (always the full backward) run in-process."""
import copy
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import conftest  # noqa: E402
import selective_bwd_checks as sc  # noqa: E402
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


@pytest.mark.parametrize('groups', [('launches',), ('golden',), ('shapes',), ('fallback', 'default')],
                         ids=['launches', 'golden', 'shapes', 'fallback+default'])
def test_selective_backward_on_the_lock_step_emulation(groups, lockstep_lib):
    r = subprocess.run([sys.executable, os.path.join(HERE, 'selective_bwd_checks.py'), lockstep_lib, *groups],
                       env=_asan_env(), capture_output=True, text=True, timeout=3000)
    out = r.stdout + r.stderr
    assert 'AddressSanitizer' not in out and 'runtime error' not in out, out[-6000:]
    assert r.returncode == 0, out[-6000:]
    last = [ln for ln in r.stdout.splitlines() if 'selective-backward checks passed' in ln]
    assert last and 'FAILED' not in last[-1], out[-6000:]
    print(last[-1])


def test_new_symbols_are_declared_and_bound():
    text = open(os.path.join(REPO, 'include', 'r2l_isp.h')).read()
    for name in ('r2l_isp_step_bwd_select', 'r2l_isp_step_bwd_select_passes'):
        assert name in _lib.EXPORTED_SYMBOLS and re.search(r'\b%s\s*\(' % name, text), name
    consts = dict(re.findall(r'\b(R2L_GRAD_[A-Z_]+) = (\d+)', text))
    assert {k: int(v) for k, v in consts.items()} == dict(
        R2L_GRAD_BLACK_LEVEL=1, R2L_GRAD_WHITE_BALANCE=2, R2L_GRAD_CCM=4, R2L_GRAD_GAMMA=8, R2L_GRAD_DEBAYER=16,
        R2L_GRAD_SHARPEN=32, R2L_GRAD_BLUR=64, R2L_GRAD_RAW=128, R2L_GRAD_ALL_PARAMS=127)
    from raw2logit_amd import functional as F_
    assert F_.grad_mask((True,) + (False,) * 7) == 128 and F_.grad_mask((False,) + (True,) * 7) == 127
    assert F_.grad_mask((False, False, False, False, True, False, False, True)) == 8 | 64


def test_attribute_defaults_to_false_and_survives_deepcopy_and_pickle():
    assert ppt.ParametrizedProcessing.selective_backward is False
    p = ppt.ParametrizedProcessing(orc.DRONE_CAMERA_PARAMS)
    assert p.selective_backward is False
    p.selective_backward = True
    q = pickle.loads(pickle.dumps(copy.deepcopy(p)))
    assert q.selective_backward is True and ppt.ParametrizedProcessing(orc.DRONE_CAMERA_PARAMS).selective_backward is False


def test_serial_emulation_always_takes_the_full_backward(emulation):
    """the serial build has no plane passes: every mask reports R2L_SELECT_FULL, and the attribute changes no bit"""
    B, H, W = 2, 12, 264
    for route in ('gamma', 'blur', 'blur_gamma'):
        assert emulation.r2l_isp_step_bwd_select_passes(sc.route_mask(route), 0, 0, B, H, W, sc.KEEP_LUMA) == 0
    raw_np = orc.synth_raw(B, H, W, seed=8, kind='scene')
    cot = np.random.default_rng(8).standard_normal((B, 3, H, W)).astype(np.float32)
    for route in ('gamma', 'blur_gamma'):
        res = [sc.step(sc.plain_module(True, True, 'cpu', route, sel), raw_np, cot, 'cpu', False) for sel in (False, True)]
        sc._same(*res)
        assert sorted(res[1][2]) == sorted(sc.ROUTES[route][1])       # parameters that did not ask: no gradient


def test_epilogue_with_frames_requiring_grad_fails_alike(emulation):
    sc.check_epilogue_with_raw_grad('cpu')


def test_select_entry_point_checks_its_mask(emulation):
    """grad_raw goes with R2L_GRAD_RAW, unknown bits are refused, a mask needs grad_params"""
    import ctypes
    z = ctypes.c_void_p(0)
    one = torch.zeros(64)
    args = lambda gp, graw, mask: (sc._lib.ptr(one), 0, 1.0, z, sc._lib.ptr(one), z, gp, z, 0, sc._lib.ptr(one), 0, 2, 4, 4, 1,  # noqa: E731
                                   0, z, z, graw, z, 0, mask)
    assert emulation.r2l_isp_step_bwd_select(*args(sc._lib.ptr(one), z, 128)) == -1
    assert emulation.r2l_isp_step_bwd_select(*args(sc._lib.ptr(one), sc._lib.ptr(one), 8)) == -1
    assert emulation.r2l_isp_step_bwd_select(*args(sc._lib.ptr(one), z, 256)) == -1
    assert emulation.r2l_isp_step_bwd_select(*args(z, z, 8)) == -1
    assert b'grad_mask' in emulation.r2l_last_error() or b'grad_params' in emulation.r2l_last_error()


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
    os.environ['R2L_BWD_PLANES'] = '1'
    B, H, W = 4, 12, 264
    raw_np = orc.synth_raw(B, H, W, seed=3, kind='scene')
    cot = np.random.default_rng(7).standard_normal((B, 3, H, W)).astype(np.float32)
    lo, hi = rank * B // world, (rank + 1) * B // world
    res = {}
    for route in ('raw', 'gamma'):
        def one(frames, c, group):
            m = sc.plain_module(True, True, 'cpu', route, True)
            m.process_group = group
            _, gr, grads, names = sc.step(m, frames, c, 'cpu', sc.ROUTES[route][0])
            assert any('_sel_' in k for k in names), names
            return gr if route == 'raw' else grads['gamma_correct']
        res[route] = one(raw_np[lo:hi].copy(), cot[lo:hi].copy(), dist.group.WORLD)
        if rank == 0:
            res[route + '_full'] = one(raw_np, cot, None)     # the whole batch in one process
    np.savez(os.path.join(out_dir, f'rank{rank}.npz'), **res)
    dist.destroy_process_group()


def test_two_gloo_ranks_split_the_selective_backward(lockstep_lib, tmp_path):
    """train-mode BatchNorm over two gloo ranks (phase A / all-gather / phase B) with the flag set: the ranks' grad_raw shards
    (RAW-only) and the sum of their gamma gradients (GAMMA-only) equal the single-process run on the whole batch"""
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
    full = r[0]['raw_full']
    got = np.concatenate([r[0]['raw'], r[1]['raw']])
    assert np.abs(got - full).max() <= 1e-5 * np.abs(full).max()
    gfull, gsum = r[0]['gamma_full'], r[0]['gamma'] + r[1]['gamma']
    assert np.abs(gsum - gfull).max() <= 2e-4 * (np.abs(gfull).max() + 1e-6)
