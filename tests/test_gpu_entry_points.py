"""tests/entry_point_checks.py on the gfx950 build: every flavour of a step and static call bit for bit, and the Python path against the
legacy entry of each call -- entered through r2l_isp_step_fwd_layout, r2l_isp_step_bwd_layout, r2l_static_workspace_bytes_opts and
r2l_static_fwd_io alone.  The CPU half: test_entry_points.py."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import entry_point_checks as checks  # noqa: E402
import parity_checks as pc  # noqa: E402
from raw2logit_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def library():
    return _lib.library_for(torch.empty(1, device=DEV))


def test_forward_flavours_agree():
    checks.check_forward_flavours(*library(), DEV)


def test_backward_flavours_agree():
    checks.check_backward_flavours(*library(), DEV)


def test_static_flavours_agree():
    checks.check_static_flavours(*library(), DEV, fft=True)


def test_python_enters_through_one_entry_each():
    lib, stream = library()
    assert checks.check_python_step(lib, stream, DEV, pc) >= 120
    checks.check_python_static(lib, stream, DEV, pc, fft=True)
