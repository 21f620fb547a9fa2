"""The weak augmentation in the static chains' stores (StaticProcessing.supports_output_epilogue, static_pipeline(epilogue=...),
r2l_static_fwd_epilogue / r2l_static_epilogue_supported) without a GPU: the C ABI and the predicate, the module on the serial
emulation (the epilogue forms refuse there with a reason and the fall-back takes over), arming through ComposeState, the device-form
kernels under the sanitizers in a stand-alone program, and the registers of the new gfx950 instantiations."""
import copy
import ctypes
import os
import pickle
import re
import subprocess
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import half_io_checks as hc  # noqa: E402
import kernel_resources  # noqa: E402
import lockstep_driver  # noqa: E402
import static_epilogue_checks as se  # noqa: E402
import static_half_checks as sh  # noqa: E402
from oracle import isp_oracle as orc  # noqa: E402
from raw2logit_amd import _lib  # noqa: E402
from raw2logit_amd import augmentation as aug  # noqa: E402
from raw2logit_amd import functional as F_  # noqa: E402
from raw2logit_amd.processing import pipeline_numpy as ppn  # noqa: E402

ALL_EPILOGUES = se.EVEN_EPILOGUES + [(False, False, 1), (True, True, 3)]


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
    ctype = {'int': ctypes.c_int, 'float': ctypes.c_float, 'double': ctypes.c_double, 'size_t': ctypes.c_size_t,
             'const void *': ctypes.c_void_p, 'void *': ctypes.c_void_p, 'const double *': ctypes.POINTER(ctypes.c_double),
             'const float *': ctypes.POINTER(ctypes.c_float)}
    assert re.search(r'const\s+char\s*\*\s*r2l_static_epilogue_supported\s*\(', text) and re.search(r'\bint\s+r2l_static_fwd_epilogue\s*\(', text)
    for name, restype in (('r2l_static_epilogue_supported', ctypes.c_char_p), ('r2l_static_fwd_epilogue', ctypes.c_int)):
        assert name in _lib.EXPORTED_SYMBOLS, name
        declared = [ctype[t] for t in _declaration(text, name)]
        assert _lib._SIGNATURES[name] == (restype, declared), (name, _declaration(text, name))
    # r2l_static_fwd_io's arguments plus `int epilogue`
    assert _lib._SIGNATURES['r2l_static_fwd_epilogue'][1] == _lib._SIGNATURES['r2l_static_fwd_io'][1] + [ctypes.c_int]
    assert len(_lib._SIGNATURES['r2l_static_epilogue_supported'][1]) == 9
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in se.NEW_SYMBOLS:
        assert hasattr(cdll, name), name
    cdll.r2l_abi_version.restype = ctypes.c_int
    assert cdll.r2l_abi_version() == 1          # additions only
    # the predicate needs no GPU: (frames, H, W, debayer, sharpening, denoising, options, out_io, epilogue) -> NULL where served
    q = cdll.r2l_static_epilogue_supported
    q.restype, q.argtypes = _lib._SIGNATURES['r2l_static_epilogue_supported']
    codes = lambda chain: (F_._DEBAYER[chain[0]], F_._SHARPEN.get(chain[1], 0), F_._DENOISE.get(chain[2], 0))      # noqa: E731
    for chain in sh.CHAINS:
        for frames in (0, 1):
            for io in (0, 1, 2):
                for e in se.EVEN_EPILOGUES:
                    assert q(frames, 64, 1024, *codes(chain), None, io, F_.epilogue_bits(e)) is None, (chain, frames, io, e)
                assert q(frames, 64, 1024, *codes(chain), None, io, 0) is None      # no epilogue: r2l_static_fwd_io's answer
    med5 = (ctypes.c_double * 5)(1.0, 1.0, 0.5, 0.3, 5.0)
    h, v, hv = F_.epilogue_bits((True, False, 0)), F_.epilogue_bits((False, True, 0)), F_.epilogue_bits((True, True, 0))
    for args, word in (((0, 64, 64, 0, 0, 0, None, 0, F_.epilogue_bits((False, False, 1))), b'k odd'),
                       ((1, 64, 64, 0, 1, 1, None, 1, F_.epilogue_bits((True, True, 3))), b'k odd'),
                       ((2, 64, 64, 0, 0, 0, None, 0, h), b'float64'), ((2, 64, 64, 0, 1, 1, None, 2, v), b'float64'),
                       ((0, 64, 64, 2, 0, 0, None, 0, h), b'menon2007'), ((0, 64, 64, 0, 1, 3, None, 0, v), b'fft_denoising'),
                       ((0, 64, 64, 0, 1, 2, med5, 0, hv), b'5x5 median'), ((0, 64, 262, 0, 0, 0, None, 0, h), b'W % 4'),
                       ((0, 64, 2052, 0, 0, 0, None, 0, v), b'W <= 2048'), ((1, 64, 2052, 0, 1, 1, None, 1, hv), b'W <= 2048'),
                       ((0, 64, 1028, 0, 2, 1, None, 0, h), b'unsharp_masking'), ((0, 64, 64, 0, 0, 0, None, 0, h | 8), b'R2L_STEP_EPI'),
                       ((0, 64, 64, 0, 0, 0, None, 5, h), b'R2L_IO')):
        why = q(*args)
        assert why and word in why, (args, why)
    assert F_.epilogue_bits((True, True, 2)) == 16 | 32 | (2 << 6)          # the step's encoding (R2L_STEP_EPI_*)


def test_class_attribute_copies_pickles_and_state_dict(emulation):
    assert ppn.StaticProcessing.supports_output_epilogue is True
    m = sh.module(sh.DEFAULT_CHAIN, norm=True)
    assert 'supports_output_epilogue' not in m.__dict__ and '_epilogue' not in m.__dict__
    keys = sorted(m.state_dict())
    raw = hc.frames(1, 8, 8, 2, 'cpu')
    y = m(raw)
    for twin in (copy.deepcopy(m), pickle.loads(pickle.dumps(m))):
        assert sorted(twin.state_dict()) == keys and twin.supports_output_epilogue and '_epilogue' not in twin.__dict__
        assert torch.equal(twin(raw), y)
    m.load_state_dict(sh.module(sh.DEFAULT_CHAIN, norm=True).state_dict())
    assert sorted(m.state_dict()) == keys


@pytest.mark.parametrize('chain', [sh.SHORT_BILINEAR, sh.SHORT_MALVAR, sh.DEFAULT_CHAIN], ids=['bilinear_short', 'malvar_short', 'default'])
def test_serial_emulation_refuses_with_a_reason(emulation, chain):
    lib = emulation
    raw = hc.frames(2, 12, 264, 1, 'cpu')
    for e in se.EVEN_EPILOGUES:
        why = F_.static_epilogue_why(raw, *chain, epilogue=e)
        assert why and 'serial emulation' in why
        out = torch.full((2, 3, 12, 264), 7.0)
        assert se.c_call(lib, raw, chain, 0, out, F_.epilogue_bits(e)) == -3 and b'serial emulation' in lib.r2l_last_error()
        assert bool((out == 7.0).all())                            # nothing written
    assert F_.static_epilogue_why(raw, *chain, epilogue=None) is None and F_.static_epilogue_why(raw, *chain, epilogue=(False, False, 0)) is None
    out = torch.full((2, 3, 12, 264), 7.0)
    assert se.c_call(lib, raw, chain, 0, out, 8) == -1 and bool((out == 7.0).all())      # a bit outside R2L_STEP_EPI_*
    # epilogue = 0 is r2l_static_fwd_io
    o0, o1 = torch.empty((2, 3, 12, 264)), torch.empty((2, 3, 12, 264))
    lib.check(se.c_call(lib, raw, chain, 0, o0, 0), 'r2l_static_fwd_epilogue(0)')
    lib.check(se.c_call(lib, raw, chain, 0, o1, 0, plain=True), 'r2l_static_fwd_io')
    assert torch.equal(o0, o1) and torch.equal(o0, F_.static_pipeline(raw, orc.DRONE_CAMERA_PARAMS, *chain))
    with pytest.raises(TypeError):
        F_.static_epilogue_why(raw, *chain, epilogue=(True, False, 0), sigma=1.0)


_PLAIN = {}


def _plain(chain, shape, norm):
    """the plain module's float32 output, computed once per (chain, shape, Normalize) and left unchanged"""
    key = (chain, shape, norm)
    if key not in _PLAIN:
        raw = hc.frames(*shape, 2, 'cpu')
        _PLAIN[key] = (raw, sh.module(chain, norm)(raw))
    return _PLAIN[key]


@pytest.mark.parametrize('dtype', se.OUT_DTYPES, ids=se.OUT_IDS)
@pytest.mark.parametrize('norm', [False, True], ids=['plain', 'normalize'])
@pytest.mark.parametrize('B,H,W', [(2, 12, 264), (1, 4, 4), (1, 8, 8)], ids=['2x12x264', '1x4x4', '1x8x8'])
@pytest.mark.parametrize('chain', [sh.SHORT_BILINEAR, sh.SHORT_MALVAR, sh.DEFAULT_CHAIN], ids=['bilinear_short', 'malvar_short', 'default'])
def test_serial_emulation_module_is_the_plain_module_moved_by_torch(emulation, chain, B, H, W, norm, dtype):
    """against torch.flip / torch.rot90 of the plain module's output on the CPU -- no code of the library's permutation kernel in
    the reference -- bit for bit; k odd on the square frames"""
    raw, plain = _plain(chain, (B, H, W), norm)
    before = plain.clone()
    for e in ALL_EPILOGUES if H == W else se.EVEN_EPILOGUES:
        m = sh.module(chain, norm)
        m.output_dtype = dtype
        y = se.armed_call(m, raw, e)
        want = se.torch_moved(plain, e)
        want = want if dtype is None else want.to(dtype)
        assert y.dtype == want.dtype and y.shape == want.shape and m.buffer['processed_rgb'] is y
        assert torch.equal(y, want), (chain, e)
        # the functional form, and an epilogue that moves nothing
        assert torch.equal(F_.static_pipeline(raw, orc.DRONE_CAMERA_PARAMS, *chain, mean_std=(sh.MEAN + sh.STD) if norm else None,
                                              out_dtype=dtype, epilogue=e), want)
    same = F_.static_pipeline(raw, orc.DRONE_CAMERA_PARAMS, *chain, mean_std=(sh.MEAN + sh.STD) if norm else None, epilogue=(False, False, 4))
    assert torch.equal(same, plain) and torch.equal(plain, before)
    if not norm and (H, W) == (12, 264):
        assert sh.reaches_both_sides_of_the_clip(plain)


def test_arming_through_the_weak_augmentation(emulation):
    """ComposeState.arm(StaticProcessing): the reference's seeded draws, made before the processor call; image and mask agree"""
    raw = hc.frames(2, 16, 16, 9, 'cpu')
    mask = torch.arange(2 * 16 * 16, dtype=torch.float32).reshape(2, 16, 16)
    seen = set()
    for seed in range(6):
        m1, m2 = sh.module(sh.DEFAULT_CHAIN, norm=True), sh.module(sh.DEFAULT_CHAIN, norm=True)
        w1, w2 = copy.deepcopy(aug.get_augmentation('weak')), copy.deepcopy(aug.get_augmentation('weak'))
        aug.set_global_seed(seed)
        ref = w1(m1(raw), retain_state=True)
        used = w1.seed
        ref_mask = w1(mask, mask_transform=True)
        w2.seed = used                                       # the same state the unarmed call left behind
        assert w2.arm(m2, retain_state=True) is True
        seen.add(m2.__dict__['_epilogue'])
        x = m2(raw)
        assert '_epilogue' not in m2.__dict__ and m2.buffer['processed_rgb'] is x
        assert torch.equal(x, ref), seed
        got = w2(x, retain_state=True)
        assert got is x
        assert torch.equal(w2(mask, mask_transform=True), ref_mask) and '_epilogue' not in m2.__dict__
    assert len(seen) > 1
    # a transform list with anything but flips / rot90 arms nothing and leaves the generators where they were
    w3 = aug.ComposeState([aug.RandomHorizontalFlip(), aug.AddGaussianNoise(0.1)])
    m3 = sh.module(sh.DEFAULT_CHAIN)
    aug.set_global_seed(3)
    state = torch.random.get_rng_state()
    assert w3.arm(m3) is False and '_epilogue' not in m3.__dict__ and torch.equal(state, torch.random.get_rng_state())
    # an armed module that raises before its pop leaves the moves for the augmentation call
    w4 = copy.deepcopy(aug.get_augmentation('weak'))
    m4 = sh.module(sh.SHORT_BILINEAR)
    aug.set_global_seed(1)
    assert w4.arm(m4)
    e = m4.__dict__['_epilogue']
    with pytest.raises(AssertionError):
        m4(raw[0])
    assert m4.__dict__['_epilogue'] == e
    plain = sh.module(sh.SHORT_BILINEAR)(raw)
    assert torch.equal(w4(plain), se.torch_moved(plain, e)) and '_epilogue' not in m4.__dict__


EXE = os.path.join(lockstep_driver.BUILD, 'r2l_static_epilogue_lockstep')
SRC = os.path.join(lockstep_driver.EMUL, 'r2l_static_epilogue_lockstep.cpp')


def test_device_form_kernels_under_the_sanitizers():
    """tests/emul/r2l_static_epilogue_lockstep.cpp: the lock-step emulation's sources + a main, -fsanitize=address,undefined, no
    Python in the process, every buffer a malloc block of exactly the size the ABI names.  1x6x80, 1x10x260 (two strips, the second
    a single group) and 1x4x4; short chain and sharpening_filter + gaussian / median; both demosaics; float32 and container frames;
    the three output types; hflip, vflip and both (every other case spelt with k = 2): each output against the plain
    instantiation's, permuted by a host loop over r2l_aug_map; one launch, of an ..._epi kernel; the refusals"""
    if not lockstep_driver.fresh(EXE, [SRC, os.path.join(lockstep_driver.EMUL, 'r2l_driver_util.h')] + lockstep_driver.lockstep_deps()):
        os.makedirs(lockstep_driver.BUILD, exist_ok=True)
        tmp = EXE + f'.{os.getpid()}.tmp'
        subprocess.run(['g++', *lockstep_driver.FLAGS, '-I' + lockstep_driver.EMUL, SRC, '-o', tmp], check=True)
        os.replace(tmp, EXE)
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    # (3 shapes x 3 chains x 2 demosaics x 2 frame types x 3 output types + 2 batches of two + 1 behind unsharp_masking) x 3 moves
    assert r.stdout.count(': 0 mismatches') == 333 and r.stdout.count('mismatches') == 333, r.stdout[-3000:]


EPI_RE = re.compile(r'^(r2l_launch_static_(?:stream_(?:bilinear|malvar)(?:_u16)?|chain(?:_malvar)?(?:_unsharp)?(?:_median)?(?:_u16)?)'
                    r'(?:_bf16|_f16)?)_epi$')
COLUMNS = ('vgpr_count', 'sgpr_count', 'vgpr_spill_count', 'sgpr_spill_count', 'private_segment_fixed_size', 'group_segment_fixed_size',
           'max_flat_workgroup_size')


def _table(lib):
    rows = {}
    for r in kernel_resources.kernel_table(lib):
        name = re.sub(r'_kernel.*$', '', re.sub(r'^_Z\d+', '', r['name']))
        rows[name] = {k: int(v) for k, v in r.items() if k != 'name'}
    return rows


def _waves_per_simd(vgprs):
    """wavefronts per SIMD that a kernel's vector registers allow on gfx950: 512 registers per lane and SIMD, allocated in blocks of 8,
    8 wavefronts at most"""
    return min(8, 512 // ((vgprs + 7) // 8 * 8))


def test_registers_of_the_new_instantiations():
    """code-object metadata of the gfx950 build (tests/kernel_resources.py).  Every epilogue instantiation: no scratch, no spilled
    vector register, the LDS size and workgroup size of its sibling without epilogue, a VGPR count not above the largest that still
    gives the sibling's wavefronts per SIMD, and the figures profiles/static_epilogue_resources.txt records"""
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('the gfx950 build (raw2logit_amd/libr2l_isp.so) is absent')
    rows = _table(_lib.LIB_PATH)
    new = {n: EPI_RE.match(n) for n in rows if EPI_RE.match(n)}
    assert len(new) == 60, sorted(new)      # 3 output types x (4 stream + 16 chain)
    assert not [n for n in rows if n.endswith('_epi') and n.startswith('r2l_launch_static_') and n not in new]
    recorded = {}
    for line in open(os.path.join(REPO, 'profiles', 'static_epilogue_resources.txt')):
        f = line.split()
        if len(f) == 8 and f[0].startswith('r2l_launch_'):
            recorded[f[0]] = [int(v) for v in f[1:]]
    for name, m in sorted(new.items()):
        r, sib = rows[name], rows[m.group(1)]
        waves = _waves_per_simd(sib['vgpr_count'])
        print(f'{name:60s} vgpr {r["vgpr_count"]:4d} (sibling {sib["vgpr_count"]:4d}, {waves} wavefronts per SIMD)  scratch '
              f'{r["private_segment_fixed_size"]}  vgpr spills {r["vgpr_spill_count"]}  sgpr->lane {r["sgpr_spill_count"]} ({sib["sgpr_spill_count"]})')
        assert r['private_segment_fixed_size'] == 0 and r['vgpr_spill_count'] == 0, (name, r)
        assert r['group_segment_fixed_size'] == sib['group_segment_fixed_size'], name
        assert r['max_flat_workgroup_size'] == sib['max_flat_workgroup_size'], name
        assert _waves_per_simd(r['vgpr_count']) >= waves, (name, r['vgpr_count'], sib['vgpr_count'])
        assert recorded.get(name) == [r[c] for c in COLUMNS], (name, recorded.get(name), r)
