"""The public step and static entry points of the C ABI, one descriptor and one entering function each (r2l_step_fwd, r2l_step_bwd,
r2l_static_fwd_impl in r2l_api_impl.h), against the record of the commit before: what every entry refuses, with which code, under
which name and in which order of its checks, and the bits every flavour of a call writes (tests/golden/entry_points.txt, written by
tests/emul/r2l_entries_lockstep.cpp under the sanitizers); then the flavours and the Python path on the serial emulation
(tests/entry_point_checks.py; the gfx950 build: test_gpu_entry_points.py).  No GPU."""
import ctypes
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import entry_point_checks as checks  # noqa: E402
import entry_points_record as rec  # noqa: E402
import lockstep_driver  # noqa: E402
import parity_checks as pc  # noqa: E402

CPU = ctypes.c_void_p(0)


def library(emulation):
    """the emulation library that serves CPU tensors NOW (a test that ran before may have switched it on again: another object)"""
    import emul_hook
    return emul_hook.active() or emulation


def test_every_entry_refuses_and_computes_what_the_parent_did():
    """byte for byte.  (Tried on a scratch copy: with the two first mask checks of r2l_step_bwd swapped the `unknown bits + R2L_GRAD_RAW
    without grad_raw` lines differ; with `r2l_isp_step_bwd_select` spelt otherwise in it every planar float32 mask line does)"""
    env = {k: v for k, v in os.environ.items() if not k.startswith('R2L_')}
    r = lockstep_driver.run('entries', env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert 'Sanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr[-3000:]
    got, want = r.stdout.splitlines(), rec.text().splitlines()
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f'line {i + 1}:\n  this tree: {g}\n  recorded:  {w}'
    assert r.stdout == rec.text()


def test_the_record_is_whole():
    """every entry is on record with the refusals it can meet, and no group of flavours holds two answers"""
    refused = rec.refusals()
    per_entry = {}
    for (entry, what), (code, err) in refused.items():
        per_entry.setdefault(entry, []).append((what, code, err))
    assert sorted(per_entry) == sorted(n[len('r2l_isp_'):] if n.startswith('r2l_isp_') else n[len('r2l_'):]
                                       for n in checks.STEP_FWD + checks.STEP_BWD + checks.STATIC_FWD)
    for entry, cases in per_entry.items():
        assert len(cases) >= 12 and sum(1 for _, code, _ in cases if code != 0) >= 12, entry
        assert all(err for _, code, err in cases if code != 0), entry
    # which name a refusal of the mask carries: r2l_isp_step_bwd_select for planar float32, the entry's own otherwise
    for entry in ('step_bwd_select', 'step_bwd_io', 'step_bwd_layout'):
        assert refused[(entry, 'f32: unknown bits in the mask')] == (-1, 'r2l_isp_step_bwd_select: unknown bits in grad_mask')
    assert refused[('step_bwd_io', 'bf16: unknown bits in the mask')] == (-1, 'r2l_isp_step_bwd_io: unknown bits in grad_mask')
    assert refused[('step_bwd_layout', 'f32 nhwc: a mask without grad_params')] == \
        (-1, 'r2l_isp_step_bwd_layout: a gradient is asked for but grad_params is null')
    assert refused[('step_bwd_raw', 'no grad_raw, a scratch of 1 byte, workspace one byte short')][0] == -2
    groups = rec.flavours()
    assert all(len(set(g.values())) == 1 for g in groups.values())
    # 2 shapes x 2 frame types x 3 BatchNorm modes x (forward with and without KEEP_LUMA, in bf16, backward in float32 and bf16) + the two
    # d/d raw groups of float32 frames; 2 shapes x 3 frame types x (4 chains x 3 + the 5 x 5 median's 2): 30 of them a lone bf16 answer
    assert len(groups) == 2 * 2 * 3 * 5 + 2 * 3 * 2 + 2 * 3 * (4 * 3 + 2)
    assert sum(1 for g in groups.values() if len(g) >= 2) == len(groups) - 30


def test_forward_flavours_agree(emulation):
    checks.check_forward_flavours(library(emulation), CPU, 'cpu')


def test_backward_flavours_agree(emulation):
    checks.check_backward_flavours(library(emulation), CPU, 'cpu')


def test_static_flavours_agree(emulation):
    checks.check_static_flavours(library(emulation), CPU, 'cpu', fft=False)


def test_python_enters_through_one_entry_each(emulation):
    lib = library(emulation)
    assert checks.check_python_step(lib, CPU, 'cpu', pc) >= 24
    checks.check_python_static(lib, CPU, 'cpu', pc, fft=False)
