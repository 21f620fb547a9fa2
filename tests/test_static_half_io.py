"""16-bit output of the static chains (StaticProcessing.output_dtype, r2l_static_fwd_io / r2l_static_io_supported) without a GPU:
the C ABI, the attribute, the serial emulation's fall-back, the device-form kernels under the sanitizers in a stand-alone program,
and the registers of the new gfx950 instantiations."""
import copy
import ctypes
import os
import pickle
import re
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import half_io_checks as hc  # noqa: E402
import kernel_resources  # noqa: E402
import lockstep_driver  # noqa: E402
import static_half_checks as sh  # noqa: E402
from oracle import isp_oracle as orc  # noqa: E402
from raw2logit_amd import _lib  # noqa: E402
from raw2logit_amd import functional as F_  # noqa: E402
from raw2logit_amd.processing import pipeline_numpy as ppn  # noqa: E402

both = pytest.mark.parametrize('dtype', sh.DTYPES, ids=sh.DTYPE_IDS)


def _declaration(text, name):
    """the parameter list of `name` in the header, comments removed, as a list of C types (names dropped)"""
    m = re.search(r'\b' + name + r'\s*\(([^)]*)\)\s*;', text)
    assert m, name
    out = []
    for p in m.group(1).split(','):
        p = re.sub(r'\s+', ' ', p.strip())
        out.append(re.sub(r'\s*\w+$', '', p) if not p.endswith('*') else p)
    return out


def test_abi_declares_exports_and_binds_the_new_entry_points():
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'r2l_isp.h')).read(), flags=re.S)
    for name in sh.NEW_SYMBOLS:
        assert re.search(r'\b' + name + r'\s*\(', text), name
        assert name in _lib.EXPORTED_SYMBOLS, name
    assert re.search(r'const\s+char\s*\*\s*r2l_static_io_supported\s*\(', text) and re.search(r'\bint\s+r2l_static_fwd_io\s*\(', text)
    # the bound signatures are the declared ones, argument by argument
    ctype = {'int': ctypes.c_int, 'float': ctypes.c_float, 'double': ctypes.c_double, 'size_t': ctypes.c_size_t,
             'const void *': ctypes.c_void_p, 'void *': ctypes.c_void_p, 'const double *': ctypes.POINTER(ctypes.c_double),
             'const float *': ctypes.POINTER(ctypes.c_float)}
    for name, restype in (('r2l_static_io_supported', ctypes.c_char_p), ('r2l_static_fwd_io', ctypes.c_int)):
        declared = [ctype[t] for t in _declaration(text, name)]
        assert _lib._SIGNATURES[name] == (restype, declared), (name, _declaration(text, name))
    assert len(_lib._SIGNATURES['r2l_static_fwd_io'][1]) == 18 and len(_lib._SIGNATURES['r2l_static_io_supported'][1]) == 7
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in sh.NEW_SYMBOLS:
        assert hasattr(cdll, name), name
    cdll.r2l_abi_version.restype = ctypes.c_int
    assert cdll.r2l_abi_version() == 1          # additions only
    # the predicate needs no GPU: (frames, H, W, debayer, sharpening, denoising, options) -> NULL where served, else the reason
    q = cdll.r2l_static_io_supported
    q.restype, q.argtypes = _lib._SIGNATURES['r2l_static_io_supported']
    for frames in (0, 1, 2):
        assert q(frames, 4, 4, 0, 0, 0, None) is None and q(frames, 70, 2048, 1, 0, 0, None) is None      # short chains
    for frames in (0, 1):
        for deb in (0, 1):
            for shp in (0, 1, 2):
                for dn in (0, 1, 2):
                    assert q(frames, 64, 1024, deb, shp, dn, None) is None, (frames, deb, shp, dn)
        assert q(frames, 70, 2048, 0, 1, 1, None) is None
    med5 = (ctypes.c_double * 5)(1.0, 1.0, 0.5, 0.3, 5.0)
    for args, word in (((0, 64, 64, 2, 0, 0, None), b'menon2007'), ((0, 64, 64, 0, 1, 3, None), b'fft_denoising'),
                       ((0, 64, 64, 0, 1, 2, med5), b'5x5 median'), ((0, 64, 262, 0, 0, 0, None), b'W % 4'),
                       ((0, 64, 2052, 0, 0, 0, None), b'W <= 2048'), ((1, 64, 2052, 0, 1, 1, None), b'W <= 2048'),
                       ((0, 64, 1028, 0, 2, 1, None), b'unsharp_masking'), ((2, 64, 64, 0, 1, 1, None), b'float64 frames'),
                       ((3, 64, 64, 0, 0, 0, None), b'R2L_FRAMES'), ((0, 3, 64, 0, 0, 0, None), b'even')):
        why = q(*args)
        assert why and word in why, (args, why)


def test_attribute_default_copies_pickles_state_dict_and_validation(emulation):
    assert ppn.StaticProcessing.output_dtype is None
    m = sh.module(sh.DEFAULT_CHAIN, norm=True)
    assert m.output_dtype is None and 'output_dtype' not in m.__dict__
    keys = sorted(m.state_dict())
    for dt in (torch.bfloat16, torch.float16, torch.float32):
        m.output_dtype = dt
        assert copy.deepcopy(m).output_dtype is dt and pickle.loads(pickle.dumps(m)).output_dtype is dt
        assert sorted(m.state_dict()) == keys                      # a plain attribute: not part of the state ...
        m.load_state_dict(sh.module(sh.DEFAULT_CHAIN, norm=True).state_dict())
        assert m.output_dtype is dt                                # ... and not touched by loading one
    raw = torch.from_numpy(orc.synth_raw(1, 8, 8, seed=0, kind='scene'))
    for bad in (torch.float64, torch.int16, 'bfloat16'):
        m.output_dtype = bad
        with pytest.raises(_lib.R2LError, match='output_dtype must be None, torch.float32, torch.bfloat16 or torch.float16'):
            m(raw)
        with pytest.raises(_lib.R2LError, match='output_dtype must be'):
            F_.static_pipeline(raw, orc.DRONE_CAMERA_PARAMS, out_dtype=bad)
    m.output_dtype = torch.float32
    y = m(raw)
    assert y.dtype == torch.float32 and m.buffer['processed_rgb'] is y


@both
def test_serial_emulation_refuses_with_a_reason(emulation, dtype):
    lib = emulation
    raw = hc.frames(2, 12, 264, 1, 'cpu')
    io = F_.IO_CODES[dtype]
    for chain in (sh.SHORT_BILINEAR, sh.SHORT_MALVAR, sh.DEFAULT_CHAIN):
        why = F_.static_io_why(raw, *chain)
        assert why and 'serial emulation' in why
        out = torch.full((2, 3, 12, 264), 7.0, dtype=dtype)
        assert sh.c_call_io(lib, raw, chain, io, out) == -3 and b'serial emulation' in lib.r2l_last_error()
        assert bool((out == 7.0).all())                            # nothing written
        # out_io = R2L_IO_F32 is today's call
        o32 = torch.empty((2, 3, 12, 264))
        lib.check(sh.c_call_io(lib, raw, chain, 0, o32), 'r2l_static_fwd_io(R2L_IO_F32)')
        assert torch.equal(o32, F_.static_pipeline(raw, orc.DRONE_CAMERA_PARAMS, *chain))
    assert sh.c_call_io(lib, raw, sh.SHORT_BILINEAR, 5, torch.empty((2, 3, 12, 264))) == -1


@both
@pytest.mark.parametrize('norm', [False, True], ids=['plain', 'normalize'])
@pytest.mark.parametrize('B,H,W', [(2, 12, 264), (1, 4, 4)], ids=['2x12x264', '1x4x4'])
@pytest.mark.parametrize('chain', [sh.SHORT_BILINEAR, sh.SHORT_MALVAR, sh.DEFAULT_CHAIN], ids=['bilinear_short', 'malvar_short', 'default'])
def test_serial_emulation_module_is_the_float32_module_and_a_cast(emulation, chain, B, H, W, norm, dtype):
    raw = hc.frames(B, H, W, 2, 'cpu')
    m16, m32 = sh.module(chain, norm), sh.module(chain, norm)
    m16.output_dtype = dtype
    y16, y32 = m16(raw), m32(raw)
    assert y16.dtype == dtype and y32.dtype == torch.float32 and m16.buffer['processed_rgb'] is y16
    assert torch.equal(y16, y32.to(dtype))
    if not norm and (H, W) != (4, 4):
        assert sh.reaches_both_sides_of_the_clip(y32)
    assert torch.equal(y32, F_.static_pipeline(raw, orc.DRONE_CAMERA_PARAMS, *chain, mean_std=(sh.MEAN + sh.STD) if norm else None))


def test_device_form_kernels_under_the_sanitizers():
    """tests/emul/r2l_static_half_lockstep.cpp (tests/lockstep_driver.py: the lock-step emulation's sources + a main,
    -fsanitize=address,undefined, no Python in the process).  1x6x80, 1x10x260 (two strips), 1x4x4; short chain,
    sharpening_filter + gaussian / median; both demosaics; float32 and 16-bit-container frames; bf16 and f16; with and without
    Normalize: each 16-bit output against the float32 instantiation's narrowed by the host helper, bit for bit, every buffer
    exactly as large as the ABI says"""
    r = lockstep_driver.run('static_half', timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    # 3 shapes x 3 chains x 2 demosaics x 2 frame types x 2 output types, 2 behind unsharp_masking, 2 on float64 frames
    assert r.stdout.count(': 0 mismatches') == 76 and r.stdout.count('mismatches') == 76, r.stdout


IO_RE = re.compile(r'^(r2l_launch_static_(?:stream_(?:bilinear|malvar)(?:_u16|_f64)?|chain(?:_malvar)?(?:_unsharp)?(?:_median)?(?:_u16)?))'
                   r'_(bf16|f16)$')
COLUMNS = ('vgpr_count', 'sgpr_count', 'vgpr_spill_count', 'sgpr_spill_count', 'private_segment_fixed_size',
           'group_segment_fixed_size', 'max_flat_workgroup_size')


def _table(lib):
    rows = {}
    for r in kernel_resources.kernel_table(lib):
        name = re.sub(r'_kernel.*$', '', re.sub(r'^_Z\d+', '', r['name']))
        rows[name] = {k: int(v) for k, v in r.items() if k != 'name'}
    return rows


def _recorded():
    """profiles/static_half_resources.txt -> (the float32 siblings' rows of the parent commit, {16-bit kernel: VGPRs it may use
    above its sibling's})"""
    parent, over, section = {}, {}, None
    for line in open(os.path.join(REPO, 'profiles', 'static_half_resources.txt')):
        if line.startswith('## '):
            section = 'parent' if 'parent' in line else ('over' if 'exceptions' in line else None)
            continue
        f = line.split()
        if section == 'parent' and len(f) == 8 and f[0].startswith('r2l_launch_'):
            parent[f[0]] = dict(zip(COLUMNS, map(int, f[1:])))
        if section == 'over' and len(f) >= 3 and f[0].startswith('r2l_launch_'):
            over[f[0]] = (int(f[1]), int(f[2]))       # (VGPRs of the 16-bit kernel, of its float32 sibling)
    return parent, over


def test_registers_of_the_new_instantiations():
    """code-object metadata of the gfx950 build (tests/kernel_resources.py).  Every 16-bit instantiation: no scratch, no spilled
    vector register, the launch shape and static LDS of its float32 sibling, and not more VGPRs than the sibling -- but for the
    exceptions profiles/static_half_resources.txt records with their figures (hipcc's allocation inside the same 256-register
    budget of two wavefronts per SIMD), which must not grow.  The float32 siblings: the figures of the parent commit (recorded
    in the same file), register for register."""
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('the gfx950 build (raw2logit_amd/libr2l_isp.so) is absent')
    rows = _table(_lib.LIB_PATH)
    new = {n: IO_RE.match(n) for n in rows if IO_RE.match(n)}
    assert len(new) == 44, sorted(new)      # 2 x (6 stream + 16 chain)
    parent, allowed = _recorded()
    assert len(parent) == 30 and set(allowed) <= set(new)
    over = []
    for name, m in sorted(new.items()):
        r, sib = rows[name], rows[m.group(1)]
        print(f'{name:56s} vgpr {r["vgpr_count"]:4d} (float32 sibling {sib["vgpr_count"]:4d})  scratch {r["private_segment_fixed_size"]}'
              f'  vgpr spills {r["vgpr_spill_count"]}  sgpr->lane {r["sgpr_spill_count"]} ({sib["sgpr_spill_count"]})')
        assert r['private_segment_fixed_size'] == 0 and r['vgpr_spill_count'] == 0, (name, r)
        assert r['group_segment_fixed_size'] == sib['group_segment_fixed_size'], name
        assert r['max_flat_workgroup_size'] == sib['max_flat_workgroup_size'], name
        if r['vgpr_count'] > sib['vgpr_count'] and not (name in allowed and r['vgpr_count'] <= allowed[name][0] and r['vgpr_count'] <= 256):
            over.append((name, r['vgpr_count'], sib['vgpr_count']))
        assert m.group(1) in parent and sib == parent[m.group(1)], ('float32 sibling changed', m.group(1), sib, parent.get(m.group(1)))
    assert not over, over
