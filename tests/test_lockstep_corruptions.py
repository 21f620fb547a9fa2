"""The corruption kernels (r2l_corruptions.h) in lock step under AddressSanitizer + UBSan on the CPU: tests/test_lockstep.py's
pattern -- the lock-step emulation it builds, a child process that preloads libasan -- over each kernel at its smallest shapes
(tests/lockstep_corruptions.py): a lane that reads or writes past the batch, the workspace's means or the LDS tile ends the run."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import conftest  # noqa: E402
from test_lockstep import _asan_runtime  # noqa: E402


def test_corruption_kernels_in_lock_step_under_address_sanitizer():
    if _asan_runtime() is None:
        pytest.skip('no libasan.so next to gcc')
    lib = conftest.build_lockstep()
    env = conftest.cpu_only_env(dict(os.environ, LD_PRELOAD=_asan_runtime(), ASAN_OPTIONS='detect_leaks=0:abort_on_error=0',
                                     UBSAN_OPTIONS='print_stacktrace=1:halt_on_error=1', OMP_NUM_THREADS='1'))
    r = subprocess.run([sys.executable, os.path.join(HERE, 'lockstep_corruptions.py'), lib], env=env, capture_output=True,
                       text=True, timeout=1200)
    tail = '\n'.join(ln for ln in (r.stdout + r.stderr).splitlines() if not ln.startswith('[parity]'))[-6000:]
    assert 'AddressSanitizer' not in r.stdout + r.stderr and 'runtime error' not in r.stdout + r.stderr, tail
    assert r.returncode == 0 and 'corruption lock-step checks passed' in r.stdout, tail
