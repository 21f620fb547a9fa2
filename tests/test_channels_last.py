"""Channels-last output and cotangent of the fused step (ParametrizedProcessing.output_memory_format, r2l_isp_step_fwd_layout /
r2l_isp_step_bwd_layout) without a GPU: the C ABI, the attribute, the serial emulation's fall-back, the device-form kernels through
the module on the lock-step emulation, the same kernels under the sanitizers in a stand-alone program, and the registers of the
new gfx950 instantiations."""
import copy
import ctypes
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import channels_last_checks as cc  # noqa: E402
import emul_hook  # noqa: E402
import half_io_checks as hc  # noqa: E402
import kernel_resources  # noqa: E402
import lockstep_driver  # noqa: E402
import parity_checks as pc  # noqa: E402
import raw_grad_checks as rc  # noqa: E402
from oracle import isp_oracle as orc  # noqa: E402
from oracle.golden_cases import PARAM_CASES  # noqa: E402
from raw2logit_amd import _lib  # noqa: E402
from raw2logit_amd import functional as F_  # noqa: E402
from raw2logit_amd.processing import pipeline_torch as ppt  # noqa: E402

NEW_SYMBOLS = ('r2l_isp_layout_supported', 'r2l_isp_step_fwd_layout', 'r2l_isp_step_bwd_layout')
CL = torch.channels_last
KEEP = 8
LOCKSTEP_PLAIN = os.path.join(lockstep_driver.BUILD, 'libr2l_lockstep_plain.so')


@pytest.fixture(scope='module')
def lockstep():
    """CPU tensors served by the lock-step emulation (every kernel in its device form, one fiber per lane) for the duration of a
    test: a build WITHOUT the sanitizers, so that it loads into this process; the sanitized run is the stand-alone program below"""
    if not lockstep_driver.fresh(LOCKSTEP_PLAIN, lockstep_driver.lockstep_deps()):
        os.makedirs(lockstep_driver.BUILD, exist_ok=True)
        tmp = LOCKSTEP_PLAIN + f'.{os.getpid()}.tmp'
        subprocess.run(['g++', '-std=c++17', '-O0', '-DR2L_TEST_HOOKS', '-shared', '-fPIC',
                        os.path.join(HERE, 'emul', 'r2l_lockstep.cpp'), '-o', tmp], check=True)
        os.replace(tmp, LOCKSTEP_PLAIN)
    before = emul_hook.active()
    lib = emul_hook.enable(LOCKSTEP_PLAIN)
    yield lib
    emul_hook.enable(before.path if before is not None else None)


def _step_tables(m):
    return (ctypes.c_void_p * 9)(*[p.data_ptr() for p in (
        m.black_level, m.white_balance, m.colour_correction, m.gamma_correct, m.debayer.weight, m.sharpening_filter.weight,
        m.gaussian_blur.weight, m.M_RGB_2_YUV, m.M_YUV_2_RGB)])


def test_abi_declares_exports_and_binds_the_new_entry_points():
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'r2l_isp.h')).read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r'\b' + name + r'\s*\(', text), name
        assert name in _lib.EXPORTED_SYMBOLS, name
    assert re.search(r'R2L_LAYOUT_NCHW\s*=\s*0\s*,\s*R2L_LAYOUT_NHWC\s*=\s*1', text)
    assert (F_.LAYOUT_NCHW, F_.LAYOUT_NHWC) == (0, 1)
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(cdll, name), name
    cdll.r2l_abi_version.restype = ctypes.c_int
    assert cdll.r2l_abi_version() == 1          # additions only
    # the predicate needs no GPU.  NCHW: r2l_isp_io_supported's answer; NHWC: the conditions of a 16-bit call, float32 included
    q, q_io = cdll.r2l_isp_layout_supported, cdll.r2l_isp_io_supported
    assert q(0, 0, 0, 1, 2, 256, 256, 0) == 1
    for io in (0, 1, 2):
        for args in ((0, 0, 2, 16, 16, KEEP), (0, 0, 2, 16, 16, 0), (0, 1, 2, 256, 256, KEEP), (0, 0, 2, 16, 18, KEEP)):
            assert q(io, 0, *args) == q_io(io, *args)
        assert q(io, 1, 0, 0, 2, 16, 16, KEEP) == 1 and q(io, 1, 1, 0, 64, 512, 2048, KEEP) == 1
        assert q(io, 1, 0, 0, 2, 16, 16, 0) == 0            # no R2L_STEP_KEEP_LUMA
        assert q(io, 1, 0, 1, 2, 256, 256, KEEP) == 0       # an additive layer
        assert q(io, 1, 0, 0, 2, 16, 18, KEEP) == 0 and q(io, 1, 0, 0, 1, 4, 2052, KEEP) == 0      # W % 4, W > 2048
        assert q(io, 1, 0, 0, 2, 16, 16, KEEP | 16) == 0 and q(io, 1, 0, 0, 2, 16, 16, KEEP | (1 << 6)) == 0     # an epilogue
        assert q(io, 2, 0, 0, 2, 16, 16, KEEP) == 0 and q(io, -1, 0, 0, 2, 16, 16, KEEP) == 0       # no such layout
    assert q(3, 1, 0, 0, 2, 16, 16, KEEP) == 0


def test_attribute_default_copies_pickles_and_validation(emulation):
    assert ppt.ParametrizedProcessing.output_memory_format is None
    m = ppt.ParametrizedProcessing(orc.DRONE_CAMERA_PARAMS)
    assert m.output_memory_format is None and 'output_memory_format' not in m.__dict__
    raw = torch.from_numpy(orc.synth_raw(1, 8, 8, seed=0, kind='scene'))
    y = m(raw)
    assert y.is_contiguous() and not y.is_contiguous(memory_format=CL)          # unset: the planar layout
    for mf in (torch.channels_last, torch.contiguous_format):
        m.output_memory_format = mf
        assert copy.deepcopy(m).output_memory_format is mf and pickle.loads(pickle.dumps(m)).output_memory_format is mf
    for bad in (torch.channels_last_3d, torch.preserve_format, 'channels_last', 1):
        m.output_memory_format = bad
        with pytest.raises(_lib.R2LError):
            m(raw)
        with pytest.raises(_lib.R2LError):
            F_.layout_supported(raw, m)
    m.output_memory_format = CL
    m.output_dtype = torch.float64
    with pytest.raises(_lib.R2LError):
        F_.layout_supported(raw, m)


def test_serial_emulation_refuses_with_a_reason(emulation):
    lib = emulation
    B, H, W = 2, 16, 16
    m = ppt.ParametrizedProcessing(orc.DRONE_CAMERA_PARAMS, batch_norm_output=False)
    raw = torch.from_numpy(orc.synth_raw(B, H, W, seed=0, kind='scene'))
    nws = lib.r2l_isp_workspace_bytes(B, H, W)
    ws = torch.empty(nws, dtype=torch.uint8)
    gp = torch.empty(_lib.R2L_P_NTRAIN)
    for io, dt in ((0, torch.float32), (1, torch.bfloat16), (2, torch.float16)):
        assert lib.r2l_isp_layout_supported(io, 1, 0, 0, B, H, W, KEEP) == 0
        out = torch.full((B, 3, H, W), 7.0, dtype=dt).contiguous(memory_format=CL)
        e = lib.r2l_isp_step_fwd_layout(_lib.ptr(raw), 0, 1.0, _step_tables(m), None, 0, None, None, None, 1e-5, 0.1, _lib.ptr(out),
                                        io, 1, _lib.ptr(ws), nws, B, H, W, 1, KEEP, None, None)
        assert e == -3 and b'serial emulation' in lib.r2l_last_error()
        assert bool((out == 7.0).all())         # nothing written
        e = lib.r2l_isp_step_bwd_layout(_lib.ptr(raw), 0, 1.0, None, _lib.ptr(out), io, 1, None, _lib.ptr(gp), None, 0, _lib.ptr(ws),
                                        nws, B, H, W, 1, KEEP, None, None, None, None, 0, 0)
        assert e == -3 and b'serial emulation' in lib.r2l_last_error()
    out = torch.empty((B, 3, H, W))
    e = lib.r2l_isp_step_fwd_layout(_lib.ptr(raw), 0, 1.0, _step_tables(m), None, 0, None, None, None, 1e-5, 0.1, _lib.ptr(out),
                                    0, 2, _lib.ptr(ws), nws, B, H, W, 1, KEEP, None, None)
    assert e == -1 and b'R2L_LAYOUT_' in lib.r2l_last_error()
    assert lib.r2l_isp_layout_supported(0, 0, 0, 0, B, H, W, 0) == 1
    # layout = R2L_LAYOUT_NCHW, io = R2L_IO_F32: exactly the existing calls
    outs = []
    for fn in ('layout', 'plain'):
        out = torch.empty((B, 3, H, W))
        args = [_lib.ptr(raw), 0, 1.0, _step_tables(m), None, 0, None, None, None, 1e-5, 0.1, _lib.ptr(out)]
        tail = [_lib.ptr(ws), nws, B, H, W, 1, KEEP, None, None]
        lib.check(lib.r2l_isp_step_fwd_layout(*args, 0, 0, *tail) if fn == 'layout' else lib.r2l_isp_step_fwd(*args, *tail), fn)
        outs.append(out)
    assert torch.equal(*outs)


@pytest.mark.parametrize('dtype', cc.DTYPES, ids=cc.DTYPE_IDS)
@pytest.mark.parametrize('name', ['drone_bn_train', 'micro_bn_train'])
def test_serial_emulation_module_is_the_default_module_and_a_conversion(emulation, name, dtype):
    """golden cases (2,16,16) and (1,64,64): output == default(raw).contiguous(memory_format=channels_last) (cast first where
    output_dtype is set), parameter gradients == those of the default module driven by the same cotangent values -- bit for bit"""
    case = next(c for c in PARAM_CASES if c['name'] == name)
    B, H, W = case['shape']
    raw = torch.from_numpy(orc.synth_raw(B, H, W, seed=case['seed'], kind=case['kind']))
    P = pc.build_params(case)
    cot, cot32 = cc.cotangent((B, 3, H, W), 7, dtype, 'cpu')
    mcl, mpl = cc.configure(pc.make_module(case, P, 'cpu'), dtype), pc.make_module(case, P, 'cpu')
    assert not F_.layout_supported(raw, mcl)
    ycl, ypl = mcl(raw), mpl(raw)
    assert ycl.dtype == dtype and ycl.is_contiguous(memory_format=CL) and mcl.buffer['processed_rgb'] is ycl
    assert torch.equal(ycl.detach(), ypl.detach().to(dtype).contiguous(memory_format=CL))
    ycl.backward(cot)
    ypl.backward(cot32)
    for k, f in pc.NAME2ATTR.items():
        if k != 'additive_layer':
            assert torch.equal(f(mcl).grad, f(mpl).grad), k
    for a, b in zip(mcl.batch_norm.buffers(), mpl.batch_norm.buffers()):
        assert torch.equal(a, b)


def test_nchw_through_the_new_entry_points_is_the_io_call(lockstep):
    """layout = R2L_LAYOUT_NCHW on the lock-step emulation: r2l_isp_step_fwd_layout / _bwd_layout against r2l_isp_step_fwd_io /
    _bwd_io on the same inputs, bit for bit, float32 and bfloat16"""
    lib = lockstep
    B, H, W = 2, 6, 80
    m = ppt.ParametrizedProcessing(orc.DRONE_CAMERA_PARAMS, batch_norm_output=False)
    raw = hc.frames(B, H, W, 0, 'cpu')
    nws = lib.r2l_isp_workspace_bytes(B, H, W)
    for io, dt in ((0, torch.float32), (1, torch.bfloat16)):
        cot, _ = cc.cotangent((B, 3, H, W), io, dt, 'cpu', layout='planar')
        res = []
        for new in (True, False):
            ws = torch.zeros(nws, dtype=torch.uint8)
            out = torch.zeros((B, 3, H, W), dtype=dt)
            gp = torch.zeros(_lib.R2L_P_NTRAIN)
            head = [_lib.ptr(raw), 0, 1.0, _step_tables(m), None, 0, None, None, None, 1e-5, 0.1, _lib.ptr(out), io]
            tail = [_lib.ptr(ws), nws, B, H, W, 1, KEEP, None, None]
            lib.check(lib.r2l_isp_step_fwd_layout(*head, 0, *tail) if new else lib.r2l_isp_step_fwd_io(*head, *tail), 'fwd')
            bhead = [_lib.ptr(raw), 0, 1.0, None, _lib.ptr(cot), io]
            btail = [_lib.ptr(out), _lib.ptr(gp), None, 0, _lib.ptr(ws), nws, B, H, W, 1, KEEP, None, None, None, None, 0, 0]
            lib.check(lib.r2l_isp_step_bwd_layout(*bhead, 0, *btail) if new else lib.r2l_isp_step_bwd_io(*bhead, *btail), 'bwd')
            res.append((out, gp))
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]), io


LOCKSTEP_SHAPES = [(2, 6, 80), (1, 4, 4), (2, 10, 260), (2, 36, 256)]


@pytest.mark.parametrize('dtype', cc.DTYPES, ids=cc.DTYPE_IDS)
@pytest.mark.parametrize('bn,training', rc.BN_MODES, ids=['bn_none', 'bn_train', 'bn_eval'])
@pytest.mark.parametrize('B,H,W', LOCKSTEP_SHAPES, ids=[f'{b}x{h}x{w}' for b, h, w in LOCKSTEP_SHAPES])
def test_module_on_the_lock_step_emulation_bitwise(lockstep, B, H, W, bn, training, dtype):
    """the device-form kernels through the module, at every shape x element type x BatchNorm mode (none / train / eval): the output
    is the planar output permuted; all 132 parameter gradients, d/d raw (requested in every case: the frames are float32) and
    BatchNorm's buffers are those of the planar step on the plane route fed the same cotangent values"""
    names = cc.check_bitwise(hc.plain(bn, training, 'cpu'), hc.frames(B, H, W, 1, 'cpu'), dtype, 'cpu',
                             f'{B}x{H}x{W} bn={bn} train={training} raw_grad=True', raw_grad=True)
    sfx = cc.suffix(dtype)
    assert names.get('r2l_launch_bwd1_plane_guv' + sfx) == 1 and any('bwd_raw_plane' in k for k in names), names
    if bn and training:
        assert names.get('r2l_launch_fwd_apply' + sfx) == 1 and names.get('r2l_launch_bnr_planes' + sfx) == 1, names
    else:
        assert names.get('r2l_launch_fwd_stream_w' + ('2' if W > 256 else '1') + sfx) == 1, names


def test_device_form_kernels_under_the_sanitizers(tmp_path):
    """tests/emul/r2l_channels_last_lockstep.cpp (tests/lockstep_driver.py: the lock-step emulation's sources + a main,
    -fsanitize=address,undefined, no Python in the process).  (2,6,80) and (1,4,260) -- a last strip of one lane; float32 /
    bfloat16 / float16; BatchNorm none / train / eval; both frame containers; d/d raw: the R2L_LAYOUT_NHWC calls against the
    R2L_LAYOUT_NCHW calls of the same build, bit for bit, `out` and `grad_out` exactly 3 B H W elements long"""
    params = tmp_path / 'params.bin'
    ppt.ParametrizedProcessing(orc.DRONE_CAMERA_PARAMS).packed_parameters().detach().numpy().astype('<f4').tofile(params)
    r = lockstep_driver.run('channels_last', params, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count(': 0 mismatches') == 12, r.stdout


NHWC_RE = re.compile(r'^(r2l_launch_(?:fwd_stream_w\d|fwd_apply|bwd1_plane|bwd1_plane_guv|bnr_planes)(?:_u16)?)((?:_bf16|_f16)?)_nhwc$')
COLUMNS = ('vgpr_count', 'sgpr_count', 'vgpr_spill_count', 'sgpr_spill_count', 'private_segment_fixed_size',
           'group_segment_fixed_size', 'max_flat_workgroup_size')


def _table(lib):
    rows = {}
    for r in kernel_resources.kernel_table(lib):
        name = re.sub(r'_kernel.*$', '', re.sub(r'^_Z\d+', '', r['name']))
        rows[name] = {k: int(v) for k, v in r.items() if k != 'name'}
    return rows


def _recorded(section):
    """the rows of one '## ...' section of profiles/channels_last_resources.txt"""
    rows, on = {}, False
    for line in open(os.path.join(REPO, 'profiles', 'channels_last_resources.txt')):
        if line.startswith('## '):
            on = section in line
            continue
        f = line.split()
        if on and len(f) == 8 and f[0].startswith('r2l_launch_'):
            rows[f[0]] = dict(zip(COLUMNS, map(int, f[1:])))
    return rows


def waves_per_simd(vgprs, workgroup):
    """wavefronts per SIMD the register file allows (gfx950: 512 VGPRs per lane and SIMD, allocated in blocks of 8, at most 8
    wavefronts)"""
    return min(8, 512 // ((vgprs + 7) // 8 * 8))


def test_registers_of_the_new_instantiations():
    """code-object metadata of the gfx950 build (tests/kernel_resources.py).  Every channels-last instantiation: no scratch, no
    spilled vector register, the LDS of its planar sibling of the same element type and frame container, and as many wavefronts
    per SIMD as that sibling's registers allow.  The planar instantiations: the figures of the parent commit, recorded in
    profiles/channels_last_resources.txt"""
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    rows = _table(_lib.LIB_PATH)
    new = {n: NHWC_RE.match(n) for n in rows if NHWC_RE.match(n)}
    assert len(new) == 45, sorted(new)          # (8 + 2 + 3 + 2) x 3 element types
    assert sorted(n for n in rows if n.endswith('_nhwc')) == sorted(new)
    parent = _recorded('parent')
    assert len(parent) == 45, sorted(parent)
    for name, m in sorted(new.items()):
        sib_name = m.group(1) + m.group(2)
        r, sib = rows[name], rows[sib_name]
        print(f'{name:44s} vgpr {r["vgpr_count"]:4d} (planar sibling {sib["vgpr_count"]:4d})  waves/SIMD '
              f'{waves_per_simd(r["vgpr_count"], 0)} ({waves_per_simd(sib["vgpr_count"], 0)})  scratch '
              f'{r["private_segment_fixed_size"]}  vgpr spills {r["vgpr_spill_count"]}  sgpr->lane {r["sgpr_spill_count"]} '
              f'({sib["sgpr_spill_count"]})')
        assert r['private_segment_fixed_size'] == 0 and r['vgpr_spill_count'] == 0, (name, r)
        assert r['group_segment_fixed_size'] == sib['group_segment_fixed_size'], name
        assert r['max_flat_workgroup_size'] == sib['max_flat_workgroup_size'], name
        assert waves_per_simd(r['vgpr_count'], 0) >= waves_per_simd(sib['vgpr_count'], 0), (name, r['vgpr_count'], sib['vgpr_count'])
        assert sib_name in parent and sib == parent[sib_name], ('planar sibling changed', sib_name, sib, parent.get(sib_name))
    assert _recorded('this commit') == {n: {k: rows[n][k] for k in COLUMNS} for n in new}, 'profiles/channels_last_resources.txt is stale'
