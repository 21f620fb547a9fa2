"""Channel mean / std of a static chain without its output (StaticProcessing.statistics, functional.static_statistics /
channel_sums / mean_std_from_sums, r2l_static_stats / r2l_channel_sums) without a GPU: the C ABI, the serial emulation (the flat
kernel runs; the statistics forms of the row-streaming kernels refuse with a reason and the fall-back takes over), the device-form
kernels under the sanitizers in a stand-alone program, and the registers of the new gfx950 instantiations."""
import copy
import ctypes
import math
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
import parity_checks as pc  # noqa: E402
import static_half_checks as sh  # noqa: E402
import static_stats_checks as sc  # noqa: E402
from oracle import isp_oracle as orc  # noqa: E402
from oracle.golden_cases import STATIC_CASES, STATIC_OPT_CASES  # noqa: E402
from raw2logit_amd import _lib  # noqa: E402
from raw2logit_amd import functional as F_  # noqa: E402

CHAIN_IDS = ['bilinear_short', 'malvar_short', 'default', 'malvar_median', 'unsharp_gauss']
CHANNEL_SHAPES = [(3, 1, 1, 1), (2, 3, 35, 67), (1, 4, 35, 66), (2, 3, 70, 260)]


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
             'double *': ctypes.c_void_p, 'const float *': ctypes.c_void_p}
    restypes = {'r2l_static_stats_supported': ctypes.c_char_p, 'r2l_static_stats_workspace_bytes': ctypes.c_size_t,
                'r2l_static_stats': ctypes.c_int, 'r2l_channel_sums_workspace_bytes': ctypes.c_size_t, 'r2l_channel_sums': ctypes.c_int}
    assert set(restypes) == set(sc.NEW_SYMBOLS)
    for name in sc.NEW_SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS, name
        declared = [ctype[t] for t in _declaration(text, name)]
        assert _lib._SIGNATURES[name] == (restypes[name], declared), (name, _declaration(text, name))
    assert [len(_lib._SIGNATURES[n][1]) for n in sc.NEW_SYMBOLS] == [7, 8, 16, 4, 9]
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in sc.NEW_SYMBOLS:
        assert hasattr(cdll, name), name
    cdll.r2l_abi_version.restype = ctypes.c_int
    assert cdll.r2l_abi_version() == 1          # additions only
    # the predicate needs no GPU: the set r2l_static_io_supported serves
    q, w = cdll.r2l_static_stats_supported, cdll.r2l_static_stats_workspace_bytes
    q.restype, q.argtypes = _lib._SIGNATURES['r2l_static_stats_supported']
    w.restype, w.argtypes = _lib._SIGNATURES['r2l_static_stats_workspace_bytes']
    for frames in (0, 1, 2):
        assert q(frames, 4, 4, 0, 0, 0, None) is None and q(frames, 70, 2048, 1, 0, 0, None) is None      # short chains
    for frames in (0, 1):
        for deb in (0, 1):
            for shp in (0, 1, 2):
                for dn in (0, 1, 2):
                    assert q(frames, 64, 1024, deb, shp, dn, None) is None, (frames, deb, shp, dn)
                    # one double[6] per wavefront of at most 2048 workgroups
                    assert 0 < w(frames, 256, 64, 1024, deb, shp, dn, None) <= 48 * 2048 * 8 and w(frames, 256, 64, 1024, deb, shp, dn, None) % 48 == 0
        assert q(frames, 70, 2048, 0, 1, 1, None) is None
    med5 = (ctypes.c_double * 5)(1.0, 1.0, 0.5, 0.3, 5.0)
    for args, word in (((0, 64, 64, 2, 0, 0, None), b'menon2007'), ((0, 64, 64, 0, 1, 3, None), b'fft_denoising'),
                       ((0, 64, 64, 0, 1, 2, med5), b'5x5 median'), ((0, 64, 262, 0, 0, 0, None), b'W % 4'),
                       ((0, 64, 2052, 0, 0, 0, None), b'W <= 2048'), ((1, 64, 2052, 0, 1, 1, None), b'W <= 2048'),
                       ((0, 64, 1028, 0, 2, 1, None), b'unsharp_masking'), ((2, 64, 64, 0, 1, 1, None), b'float64 frames'),
                       ((3, 64, 64, 0, 0, 0, None), b'R2L_FRAMES'), ((0, 3, 64, 0, 0, 0, None), b'even')):
        why = q(*args)
        assert why and word in why, (args, why)
        assert w(args[0], 2, *args[1:]) == 0
    cs = cdll.r2l_channel_sums_workspace_bytes
    cs.restype, cs.argtypes = _lib._SIGNATURES['r2l_channel_sums_workspace_bytes']
    assert cs(3, 1, 1, 1) == 16 and cs(2, 3, 35, 67) == 48 * ((2 * 3 * 35 * 67 // 4 + 511) // 512) and cs(1, 5, 4, 4) == 0
    assert cs(64, 4, 1024, 1024) == 64 * 2048          # at most 2048 shares


@pytest.mark.parametrize('chain', sc.CHAINS, ids=CHAIN_IDS)
def test_serial_emulation_refuses_with_a_reason_and_falls_back(emulation, chain):
    lib = emulation
    raw = hc.frames(2, 12, 264, 1, 'cpu')
    why = F_.static_stats_why(raw, *chain)
    assert why and 'serial emulation' in why
    sums = torch.full((7,), 7.0, dtype=torch.float64)
    ws = torch.empty(4096, dtype=torch.uint8)
    assert sc.c_call(lib, raw, chain, sums, ws, 4096) == -3 and b'serial emulation' in lib.r2l_last_error()
    assert sums.tolist() == [7.0] * 7                              # nothing written
    assert sc.c_call(lib, raw, chain, None, ws, 4096) == -1        # null pointers first
    got, out32 = sc.check_values(chain, raw, f'serial {chain}')    # check 2 through the fall-back
    assert sh.reaches_both_sides_of_the_clip(out32)
    sc.check_repeatable(chain, raw, f'serial {chain}')             # check 5
    m = sh.module(chain, norm=True)
    m.output_dtype = torch.bfloat16                                # neither the Normalize nor the output type plays a part
    mean, std = m.statistics(raw)
    want = F_.mean_std_from_sums(got)
    assert torch.equal(mean, want[0]) and torch.equal(std, want[1]) and m.stages is None and m.buffer is None


@pytest.mark.parametrize('kind', ['f32', 'u16', 'f64'])
@pytest.mark.parametrize('B,H,W', [(1, 4, 4), (2, 10, 264), (2, 70, 260)], ids=['1x4x4', '2x10x264', '2x70x260'])
@pytest.mark.parametrize('chain', sc.CHAINS, ids=CHAIN_IDS)
def test_every_pixel_once_on_constant_frames(emulation, chain, B, H, W, kind):
    sc.check_every_pixel_once(chain, B, H, W, 'cpu', kind, f'serial {chain} {B}x{H}x{W} {kind}')


def test_golden_cases_against_the_reference(emulation, golden):
    """check 3 on every STATIC_CASES / STATIC_OPT_CASES entry"""
    n = 0
    for key, cases in (('static_cases', STATIC_CASES), ('static_opts', STATIC_OPT_CASES)):
        for case in cases:
            n += bool(sc.check_golden(case, golden, key, 'cpu'))
    assert n >= len(STATIC_CASES)


@pytest.mark.parametrize('shape', CHANNEL_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_channel_sums_against_fsum(emulation, shape):
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.rand(shape, generator=g) * 2.0 - 0.5
    sums = sc.check_channel_sums(x, f'channel_sums {shape}')
    assert torch.equal(sums, F_.channel_sums(x))
    # an unaligned view: storage offset 1 (the scalar head and tail around the 16-byte loads)
    flat = torch.empty(x.numel() + 1)
    flat[1:] = x.reshape(-1)
    view = flat[1:].view(shape)
    assert view.storage_offset() == 1 and view.data_ptr() % 16 == 4 and view.is_contiguous()
    sc.check_channel_sums(view, f'channel_sums {shape} offset 1')
    # the result does not depend on the grid: the shares come from the shape
    for grid in (1, 3):
        with pc.env_overrides('cpu', dict(R2L_GRID_FLAT=grid)):
            assert torch.equal(F_.channel_sums(x), sums), grid
    with pytest.raises(TypeError):
        F_.channel_sums(x.double())


def test_channel_sums_refuses_what_it_does_not_take(emulation):
    lib = emulation
    x = torch.zeros(1, 5, 2, 2)
    s = torch.full((11,), 7.0, dtype=torch.float64)
    ws = torch.empty(1 << 16, dtype=torch.uint8)
    assert lib.r2l_channel_sums(_lib.ptr(x), _lib.ptr(s), 1, 5, 2, 2, _lib.ptr(ws), ws.numel(), None) == -1
    assert lib.r2l_channel_sums(None, _lib.ptr(s), 1, 3, 2, 2, _lib.ptr(ws), ws.numel(), None) == -1
    n = lib.r2l_channel_sums_workspace_bytes(1, 3, 2, 2)
    assert lib.r2l_channel_sums(_lib.ptr(x), _lib.ptr(s), 1, 3, 2, 2, _lib.ptr(ws), n - 1, None) == -2
    assert s.tolist() == [7.0] * 11


def test_batches_of_different_sizes_add_up(emulation):
    m = sh.module(sh.DEFAULT_CHAIN)
    batches = [hc.frames(2, 12, 264, 3, 'cpu'), hc.frames(1, 8, 16, 4, 'cpu'), hc.frames(3, 6, 80, 5, 'cpu')]
    mean, std = m.statistics(iter(batches))
    assert mean.dtype == torch.float32 and std.dtype == torch.float32 and tuple(mean.shape) == (3, 1, 1) == tuple(std.shape)
    outs = [F_.static_pipeline(b, orc.DRONE_CAMERA_PARAMS, *sh.DEFAULT_CHAIN) for b in batches]
    parts = [sc.fsums(o) for o in outs]
    n = sum(o.shape[0] * o.shape[2] * o.shape[3] for o in outs)
    s1 = [math.fsum(p[0][c] for p in parts) for c in range(3)]
    s2 = [math.fsum(p[1][c] for p in parts) for c in range(3)]
    merged = torch.tensor(s1 + s2 + [float(n)], dtype=torch.float64)
    want = F_.mean_std_from_sums(merged)
    # the module's float64 sums differ from the fsum ones by the any-order bound (~1e-13 relative): the same float32 but for a
    # value within that of a rounding boundary -- one unit in the last place
    assert (mean - want[0]).abs().max() <= 2.0 ** -24 and (std - want[1]).abs().max() <= 2.0 ** -24
    # ... and torch.mean / torch.std of the float32 output, as get_statistics takes them, within the limits of the golden check
    allv = torch.cat([o.permute(1, 0, 2, 3).reshape(3, -1) for o in outs], dim=1).double()
    assert (mean.reshape(3).double() - allv.mean(dim=1)).abs().max() <= 1e-5 + 2.0 ** -23
    assert (std.reshape(3).double() - allv.std(dim=1)).abs().max() <= 1e-5 * math.sqrt(n / (n - 1)) + 2.0 ** -23
    biased = m.statistics(batches, unbiased=False)[1]
    assert (biased.reshape(3).double() - allv.std(dim=1, unbiased=False)).abs().max() <= 1e-5 + 2.0 ** -23
    one = m.statistics(batches[0])                      # a tensor is a batch
    assert torch.equal(one[0], F_.mean_std_from_sums(F_.static_statistics(batches[0], orc.DRONE_CAMERA_PARAMS, *sh.DEFAULT_CHAIN))[0])
    with pytest.raises(ValueError):
        m.statistics([])


def test_module_copies_and_pickles_as_before(emulation):
    m = sh.module(sh.DEFAULT_CHAIN, norm=True)
    keys = sorted(m.state_dict())
    raw = hc.frames(1, 8, 16, 2, 'cpu')
    m.statistics(raw)
    assert sorted(m.state_dict()) == keys and m.stages is None and m.buffer is None
    for twin in (copy.deepcopy(m), pickle.loads(pickle.dumps(m))):
        assert torch.equal(twin(raw), m(raw)) and torch.equal(twin.statistics(raw)[1], m.statistics(raw)[1])
    # the three-line replacement of get_statistics: the statistics of a chain, then the same chain normalising with them
    mean, std = m.statistics(raw)
    n = type(m)(orc.DRONE_CAMERA_PARAMS, *sh.DEFAULT_CHAIN, mean=mean, std=std)
    y = n(raw)
    assert (y.mean(dim=(0, 2, 3)).abs() < 1e-5).all() and ((y.std(dim=(0, 2, 3)) - 1).abs() < 1e-5).all()


def test_arguments_are_checked_as_static_pipeline_checks_them(emulation):
    raw = hc.frames(1, 8, 16, 2, 'cpu')
    with pytest.raises(NotImplementedError):
        F_.static_statistics(raw, orc.DRONE_CAMERA_PARAMS, 'nearest')
    with pytest.raises(NotImplementedError):
        F_.static_statistics(raw, orc.DRONE_CAMERA_PARAMS, 'bilinear', 'none', 'tv_chambolle')
    with pytest.raises(AssertionError):
        F_.static_statistics(raw[0], orc.DRONE_CAMERA_PARAMS)
    with pytest.raises(TypeError):
        F_.static_statistics(raw, orc.DRONE_CAMERA_PARAMS, sigma=1.0)
    with pytest.raises(TypeError):
        F_.static_stats_why(raw, sigma=1.0)
    with pytest.raises(_lib.R2LError, match='gaussian_sigma'):
        F_.static_statistics(raw, orc.DRONE_CAMERA_PARAMS, 'bilinear', 'none', 'gaussian_denoising', gaussian_sigma=0.7)


EXE = os.path.join(lockstep_driver.BUILD, 'r2l_static_stats_lockstep')
SRC = os.path.join(lockstep_driver.EMUL, 'r2l_static_stats_lockstep.cpp')


def test_device_form_kernels_under_the_sanitizers():
    """tests/emul/r2l_static_stats_lockstep.cpp: the lock-step emulation's sources + a main, -fsanitize=address,undefined, no Python
    in the process, every buffer a malloc block of exactly the size the ABI names.  Checks 1, 2 (long double) and 5 and the launch
    record at 1x6x80, 1x10x260 (two strips) and 1x4x4: short chain and sharpening_filter + gaussian / median, both demosaics,
    float32 and container frames, float64 on the short chain; two capped launches (a workgroup walks several items), two chains
    behind unsharp_masking; r2l_channel_sums on four shapes, three of them unaligned; the refusals."""
    if not lockstep_driver.fresh(EXE, [SRC, os.path.join(lockstep_driver.EMUL, 'r2l_driver_util.h')] + lockstep_driver.lockstep_deps()):
        os.makedirs(lockstep_driver.BUILD, exist_ok=True)
        tmp = EXE + f'.{os.getpid()}.tmp'
        subprocess.run(['g++', *lockstep_driver.FLAGS, '-I' + lockstep_driver.EMUL, SRC, '-o', tmp], check=True)
        os.replace(tmp, EXE)
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    # 3 shapes x (3 chains x 2 demosaics x 2 frame types + 2 float64 short chains) + 2 capped + 2 unsharp + 4 channel_sums
    assert r.stdout.count(': 0 mismatches') == 50 and r.stdout.count('mismatches') == 50, r.stdout


STATS_RE = re.compile(r'^(r2l_launch_static_(?:stream_(?:bilinear|malvar)(?:_u16|_f64)?|chain(?:_malvar)?(?:_unsharp)?(?:_median)?(?:_u16)?))_stats$')


def _table(lib):
    rows = {}
    for r in kernel_resources.kernel_table(lib):
        name = re.sub(r'_kernel.*$', '', re.sub(r'^_Z\d+', '', r['name']))
        rows[name] = {k: int(v) for k, v in r.items() if k != 'name'}
    return rows


def test_registers_of_the_new_instantiations():
    """code-object metadata of the gfx950 build (tests/kernel_resources.py).  Every statistics instantiation: no scratch, no spilled
    vector register, the launch shape and static LDS of its float32 sibling, at most 256 VGPRs (the budget of two wavefronts per
    SIMD), and the figures profiles/static_stats_resources.txt records"""
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('the gfx950 build (raw2logit_amd/libr2l_isp.so) is absent')
    rows = _table(_lib.LIB_PATH)
    new = {n: STATS_RE.match(n) for n in rows if STATS_RE.match(n)}
    assert len(new) == 22, sorted(new)      # 6 stream + 16 chain
    recorded = {}
    for line in open(os.path.join(REPO, 'profiles', 'static_stats_resources.txt')):
        f = line.split()
        if len(f) == 8 and f[0].startswith('r2l_launch_'):
            recorded[f[0]] = [int(v) for v in f[1:]]
    cols = ('vgpr_count', 'sgpr_count', 'vgpr_spill_count', 'sgpr_spill_count', 'private_segment_fixed_size', 'group_segment_fixed_size',
            'max_flat_workgroup_size')
    for name, m in sorted(new.items()):
        r, sib = rows[name], rows[m.group(1)]
        print(f'{name:56s} vgpr {r["vgpr_count"]:4d} (float32 sibling {sib["vgpr_count"]:4d})  scratch {r["private_segment_fixed_size"]}'
              f'  vgpr spills {r["vgpr_spill_count"]}  sgpr->lane {r["sgpr_spill_count"]} ({sib["sgpr_spill_count"]})')
        assert r['private_segment_fixed_size'] == 0 and r['vgpr_spill_count'] == 0, (name, r)
        assert r['group_segment_fixed_size'] == sib['group_segment_fixed_size'], name
        assert r['max_flat_workgroup_size'] == sib['max_flat_workgroup_size'], name
        assert r['vgpr_count'] <= 256, (name, r)
        assert recorded.get(name) == [r[c] for c in cols], (name, recorded.get(name), r)
        assert recorded.get(m.group(1)) == [sib[c] for c in cols], (m.group(1), recorded.get(m.group(1)), sib)
    for name in ('r2l_launch_channel_sums', 'r2l_launch_sums_finish'):
        assert rows[name]['private_segment_fixed_size'] == 0 and rows[name]['vgpr_spill_count'] == 0, (name, rows[name])
