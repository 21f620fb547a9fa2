"""16-bit output and cotangent of the fused step (ParametrizedProcessing.output_dtype, r2l_isp_step_fwd_io / r2l_isp_step_bwd_io)
without a GPU: the C ABI, the attribute, the serial emulation's fall-back, the conversion helpers pattern by pattern against torch,
the device-form kernels under the sanitizers in a stand-alone program, and the registers of the new gfx950 instantiations."""
import copy
import ctypes
import os
import pickle
import re
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import kernel_resources  # noqa: E402
import lockstep_driver  # noqa: E402
import parity_checks as pc  # noqa: E402
from oracle import isp_oracle as orc  # noqa: E402
from oracle.golden_cases import PARAM_CASES  # noqa: E402
from raw2logit_amd import _lib  # noqa: E402
from raw2logit_amd import functional as F_  # noqa: E402
from raw2logit_amd.processing import pipeline_torch as ppt  # noqa: E402

NEW_SYMBOLS = ('r2l_isp_io_supported', 'r2l_isp_step_fwd_io', 'r2l_isp_step_bwd_io')
SANITIZE = lockstep_driver.SANITIZE


def test_abi_declares_exports_and_binds_the_new_entry_points():
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'r2l_isp.h')).read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r'\b' + name + r'\s*\(', text), name
        assert name in _lib.EXPORTED_SYMBOLS, name
    assert re.search(r'R2L_IO_F32\s*=\s*0\s*,\s*R2L_IO_BF16\s*=\s*1\s*,\s*R2L_IO_F16\s*=\s*2', text)
    assert (F_.IO_F32, F_.IO_BF16, F_.IO_F16) == (0, 1, 2)
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(cdll, name), name
    cdll.r2l_abi_version.restype = ctypes.c_int
    assert cdll.r2l_abi_version() == 1          # additions only
    # the predicate needs no GPU: float32 always; 16 bits where the row-streaming forward runs, no epilogue, Y' kept
    q = cdll.r2l_isp_io_supported
    KEEP = 8
    assert q(0, 0, 1, 2, 256, 256, 0) == 1
    for io in (1, 2):
        assert q(io, 0, 0, 2, 16, 16, KEEP) == 1 and q(io, 1, 0, 64, 512, 2048, KEEP) == 1
        assert q(io, 0, 0, 2, 16, 16, 0) == 0            # no R2L_STEP_KEEP_LUMA
        assert q(io, 0, 1, 2, 256, 256, KEEP) == 0       # an additive layer
        assert q(io, 0, 0, 2, 16, 18, KEEP) == 0 and q(io, 0, 0, 1, 4, 2052, KEEP) == 0      # W % 4, W > 2048
        assert q(io, 0, 0, 2, 16, 16, KEEP | 16) == 0 and q(io, 0, 0, 2, 16, 16, KEEP | (1 << 6)) == 0     # an epilogue
    assert q(3, 0, 0, 2, 16, 16, KEEP) == 0


def test_attribute_default_copies_pickles_and_validation(emulation):
    assert ppt.ParametrizedProcessing.output_dtype is None
    m = ppt.ParametrizedProcessing(orc.DRONE_CAMERA_PARAMS)
    assert m.output_dtype is None and 'output_dtype' not in m.__dict__
    for dt in (torch.bfloat16, torch.float16, torch.float32):
        m.output_dtype = dt
        assert copy.deepcopy(m).output_dtype is dt and pickle.loads(pickle.dumps(m)).output_dtype is dt
    raw = torch.from_numpy(orc.synth_raw(1, 8, 8, seed=0, kind='scene'))
    for bad in (torch.float64, torch.int16, 'bfloat16'):
        m.output_dtype = bad
        with pytest.raises(_lib.R2LError):
            m(raw)
        with pytest.raises(_lib.R2LError):
            F_.io_supported(raw, m)
    m.output_dtype = torch.bfloat16
    with pytest.raises(TypeError):         # parameters stay float32
        copy.deepcopy(m).half()(raw)


def _step_tables(m):
    return (ctypes.c_void_p * 9)(*[p.data_ptr() for p in (
        m.black_level, m.white_balance, m.colour_correction, m.gamma_correct, m.debayer.weight, m.sharpening_filter.weight,
        m.gaussian_blur.weight, m.M_RGB_2_YUV, m.M_YUV_2_RGB)])


def test_serial_emulation_refuses_with_a_reason(emulation):
    lib = emulation
    B, H, W, KEEP = 2, 16, 16, 8
    m = ppt.ParametrizedProcessing(orc.DRONE_CAMERA_PARAMS, batch_norm_output=False)
    raw = torch.from_numpy(orc.synth_raw(B, H, W, seed=0, kind='scene'))
    nws = lib.r2l_isp_workspace_bytes(B, H, W)
    ws = torch.empty(nws, dtype=torch.uint8)
    gp = torch.empty(_lib.R2L_P_NTRAIN)
    for io, dt in ((1, torch.bfloat16), (2, torch.float16)):
        assert lib.r2l_isp_io_supported(io, 0, 0, B, H, W, KEEP) == 0
        out = torch.empty((B, 3, H, W), dtype=dt)
        e = lib.r2l_isp_step_fwd_io(_lib.ptr(raw), 0, 1.0, _step_tables(m), None, 0, None, None, None, 1e-5, 0.1, _lib.ptr(out), io,
                                    _lib.ptr(ws), nws, B, H, W, 1, KEEP, None, None)
        assert e == -3 and b'serial emulation' in lib.r2l_last_error()
        e = lib.r2l_isp_step_bwd_io(_lib.ptr(raw), 0, 1.0, None, _lib.ptr(out), io, None, _lib.ptr(gp), None, 0, _lib.ptr(ws), nws,
                                    B, H, W, 1, KEEP, None, None, None, None, 0, 0)
        assert e == -3 and b'serial emulation' in lib.r2l_last_error()
    assert lib.r2l_isp_io_supported(0, 0, 0, B, H, W, 0) == 1
    # io = R2L_IO_F32: exactly the existing calls
    outs = []
    for fn in ('io', 'plain'):
        out = torch.empty((B, 3, H, W))
        args = [_lib.ptr(raw), 0, 1.0, _step_tables(m), None, 0, None, None, None, 1e-5, 0.1, _lib.ptr(out)]
        tail = [_lib.ptr(ws), nws, B, H, W, 1, KEEP, None, None]
        lib.check(lib.r2l_isp_step_fwd_io(*args, 0, *tail) if fn == 'io' else lib.r2l_isp_step_fwd(*args, *tail), fn)
        outs.append(out)
    assert torch.equal(*outs)


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'f16'])
@pytest.mark.parametrize('name', ['drone_bn_train', 'micro_bn_train'])
def test_serial_emulation_module_is_the_float32_module_and_a_cast(emulation, name, dtype):
    """golden cases (2,16,16) and (1,64,64): output == module_f32(raw).to(dtype), parameter gradients == those of the float32 module
    driven by the same cotangent widened -- bit for bit"""
    case = next(c for c in PARAM_CASES if c['name'] == name)
    B, H, W = case['shape']
    assert (B, H, W) in ((2, 16, 16), (1, 64, 64))
    raw = torch.from_numpy(orc.synth_raw(B, H, W, seed=case['seed'], kind=case['kind']))
    P = pc.build_params(case)
    cot16 = torch.from_numpy(np.random.default_rng(7).standard_normal((B, 3, H, W)).astype(np.float32)).to(dtype)
    m16, m32 = pc.make_module(case, P, 'cpu'), pc.make_module(case, P, 'cpu')
    m16.output_dtype = dtype
    assert not F_.io_supported(raw, m16)
    y16, y32 = m16(raw), m32(raw)
    assert y16.dtype == dtype and torch.equal(y16.detach(), y32.detach().to(dtype)) and m16.buffer['processed_rgb'] is y16
    assert all(v.dtype == torch.float32 for v in m16.stages.values())
    y16.backward(cot16)
    y32.backward(cot16.float())
    for k, f in pc.NAME2ATTR.items():
        if k != 'additive_layer':
            assert torch.equal(f(m16).grad, f(m32).grad), k
    for a, b in zip(m16.batch_norm.buffers(), m32.batch_norm.buffers()):
        assert torch.equal(a, b)


def _f32(bits):
    return torch.from_numpy(np.asarray(bits, dtype=np.uint32).view(np.int32).copy()).view(torch.float32)


def _bits16(t):
    return t.view(torch.int16).numpy().view(np.uint16)


def _conversion_patterns():
    """float32 bit patterns: every 16-bit value of both types widened, every midpoint between neighbours (ties, both parities),
    one float32 step either side of each midpoint, +-0, float32 and float16 subnormals, the overflow boundaries, Inf, NaN, and
    1 M seeded random patterns"""
    all16 = torch.arange(65536, dtype=torch.int32).to(torch.int16)
    pats = []
    for dt in (torch.bfloat16, torch.float16):
        w = all16.view(dt).float()
        wb = w.view(torch.int32).numpy().view(np.uint32)
        pats.append(wb)
        # neighbours p and p + 1 of one sign and finite: the midpoint in float64, exactly representable in float32
        nxt = (all16.to(torch.int32) + 1).to(torch.int16).view(dt).float()
        ok = torch.isfinite(w) & torch.isfinite(nxt) & ((all16.to(torch.int32) & 0x7fff) != 0x7fff)
        mid = ((w.double() + nxt.double()) / 2)[ok].float()
        mb = mid.view(torch.int32).numpy().view(np.uint32)
        pats += [mb, mb + 1, mb - 1]
    special = np.array([0x00000000, 0x80000000, 0x00000001, 0x807fffff, 0x00800000, 0x33000000, 0x33000001, 0x32ffffff, 0x33800000,
                        0x38800000, 0x387fffff, 0x387fe000, 0x387ff000, 0x477fe000, 0x477fefff, 0x477ff000, 0x477ff001, 0x47800000,
                        0x7f7f0000, 0x7f7f7fff, 0x7f7f8000, 0x7f7fffff, 0xff7f8000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000,
                        0x7f800001, 0x7fffffff, 0xff800001], dtype=np.uint32)
    rnd = np.random.default_rng(2024).integers(0, 1 << 32, size=1 << 20, dtype=np.uint64).astype(np.uint32)
    p = np.concatenate(pats + [special, rnd])
    return p[:len(p) // 4 * 4]


def test_conversion_helpers_bit_for_bit_against_torch(tmp_path):
    """the host forms of r2l_common.h's helpers in a stand-alone program under -fsanitize=address,undefined (serial and lock-step
    defines); expected values: torch's Tensor.to(dtype)"""
    pats = _conversion_patterns()
    x = _f32(pats)
    exp = tmp_path / 'expected.bin'
    rec = np.empty(len(pats), dtype=[('f', '<u4'), ('b', '<u2'), ('h', '<u2')])
    rec['f'], rec['b'], rec['h'] = pats, _bits16(x.to(torch.bfloat16)), _bits16(x.to(torch.float16))
    all16 = torch.arange(65536, dtype=torch.int32).to(torch.int16)
    with open(exp, 'wb') as f:
        f.write(struct.pack('<I', len(pats)))
        f.write(rec.tobytes())
        for dt in (torch.bfloat16, torch.float16):
            f.write(all16.view(dt).float().view(torch.int32).numpy().astype('<i4').tobytes())
    src = os.path.join(HERE, 'emul', 'r2l_half_io_convert.cpp')
    for tag, defs in (('serial', []), ('lockstep', ['-DR2L_CONVERT_LOCKSTEP'])):
        exe = tmp_path / f'convert_{tag}'
        subprocess.run(['g++', '-std=c++17', '-O1', *SANITIZE, *defs, src, '-o', str(exe)], check=True)
        r = subprocess.run([str(exe), str(exp)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        assert f'checked {len(pats)} narrowings' in r.stdout and ' 0 mismatches' in r.stdout, r.stdout


def test_device_form_kernels_under_the_sanitizers(tmp_path):
    """tests/emul/r2l_half_io_lockstep.cpp (tests/lockstep_driver.py: the lock-step emulation's sources + a main,
    -fsanitize=address,undefined, no Python in the process).  (2,4,4), (2,4,260), (1,70,260); BatchNorm none / train / eval; both
    frame types; both 16-bit types; d/d raw: the 16-bit calls against the io = R2L_IO_F32 calls of the same build, bit for bit,
    every buffer exactly as large as the ABI says"""
    params = tmp_path / 'params.bin'
    ppt.ParametrizedProcessing(orc.DRONE_CAMERA_PARAMS).packed_parameters().detach().numpy().astype('<f4').tofile(params)
    r = lockstep_driver.run('half_io', params, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count(': 0 mismatches') == 12, r.stdout


IO_RE = re.compile(r'^(r2l_launch_(?:fwd_stream_w\d|fwd_apply|bwd1_plane|bwd1_plane_guv|bnr_planes)(?:_u16)?)_(bf16|f16)$')


def _table(lib):
    rows = {}
    for r in kernel_resources.kernel_table(lib):
        name = re.sub(r'_kernel.*$', '', re.sub(r'^_Z\d+', '', r['name']))
        rows[name] = {k: int(v) for k, v in r.items() if k != 'name'}
    return rows


def _recorded_parent_table():
    """the float32 siblings' rows of the parent commit, as profiles/half_io_resources.txt records them"""
    rows, on = {}, False
    for line in open(os.path.join(REPO, 'profiles', 'half_io_resources.txt')):
        if line.startswith('## '):
            on = 'parent' in line
            continue
        f = line.split()
        if on and len(f) == 8 and f[0].startswith('r2l_launch_'):
            rows[f[0]] = dict(zip(('vgpr_count', 'sgpr_count', 'vgpr_spill_count', 'sgpr_spill_count', 'private_segment_fixed_size',
                                   'group_segment_fixed_size', 'max_flat_workgroup_size'), map(int, f[1:])))
    return rows


def test_registers_of_the_new_instantiations():
    """code-object metadata of the gfx950 build (tests/kernel_resources.py).  Every 16-bit instantiation: no scratch, no spilled
    vector register (vgpr_spill_count; scalars parked in vector lanes -- sgpr_spill_count, 17 .. 69 in the float32 siblings -- are
    recorded in profiles/half_io_resources.txt, they never reach memory), not more VGPRs than its float32 sibling.  The float32
    siblings: the figures of the parent commit (recorded in the same file)."""
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    rows = _table(_lib.LIB_PATH)
    new = {n: IO_RE.match(n) for n in rows if IO_RE.match(n)}
    assert len(new) == 30, sorted(new)
    parent = _recorded_parent_table()
    over = []
    for name, m in sorted(new.items()):
        r, sib = rows[name], rows[m.group(1)]
        print(f'{name:44s} vgpr {r["vgpr_count"]:4d} (float32 sibling {sib["vgpr_count"]:4d})  scratch {r["private_segment_fixed_size"]}'
              f'  vgpr spills {r["vgpr_spill_count"]}  sgpr->lane {r["sgpr_spill_count"]} ({sib["sgpr_spill_count"]})')
        assert r['private_segment_fixed_size'] == 0 and r['vgpr_spill_count'] == 0, (name, r)
        assert r['group_segment_fixed_size'] == sib['group_segment_fixed_size'], name
        if r['vgpr_count'] > sib['vgpr_count']:
            over.append((name, r['vgpr_count'], sib['vgpr_count']))
        assert m.group(1) in parent and rows[m.group(1)] == parent[m.group(1)], ('float32 sibling changed', m.group(1),
                                                                                  rows[m.group(1)], parent.get(m.group(1)))
    assert not over, over
