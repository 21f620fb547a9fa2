"""Every public step and static entry point against the others that can express the same call, bit for bit, and the Python path
against the legacy entry it took before it went through r2l_isp_step_fwd_layout / r2l_isp_step_bwd_layout / r2l_static_fwd_io alone.
Shared by test_entry_points.py (the serial emulation: the routes that exist there) and test_gpu_entry_points.py (gfx950).  An
adapter fault does not depend on size: 2x64x96 and 1x16x20."""
import copy
import ctypes
import itertools

import numpy as np
import torch

from oracle import isp_oracle as orc
from raw2logit_amd import _lib
from raw2logit_amd import functional as F
from raw2logit_amd._lib import ptr
from raw2logit_amd.processing.pipeline_torch import ParametrizedProcessing

SHAPES = ((2, 64, 96), (1, 16, 20))
ALL, A, B_, KEEP = 0, 1, 2, 8
F32, BF16, NCHW, NHWC = 0, 1, 0, 1
NONE, TRAIN, EVAL = 0, 1, 2
STATS, MOMENTS, SUMS, BN = 0, 1, 2, 4     # r2l_isp_step_offset (include/r2l_isp.h: R2L_STEP_*)
STEP_FWD = ('r2l_isp_step_fwd', 'r2l_isp_step_fwd_io', 'r2l_isp_step_fwd_layout')
STEP_BWD = ('r2l_isp_step_bwd', 'r2l_isp_step_bwd_raw', 'r2l_isp_step_bwd_select', 'r2l_isp_step_bwd_io', 'r2l_isp_step_bwd_layout')
STATIC_FWD = ('r2l_static_fwd', 'r2l_static_fwd_u16', 'r2l_static_fwd_f64', 'r2l_static_fwd_norm', 'r2l_static_fwd_opts',
              'r2l_static_fwd_io')
STATIC_WS = ('r2l_static_workspace_bytes', 'r2l_static_workspace_bytes_f64', 'r2l_static_workspace_bytes_opts')


def frames(shape, kind, dev, seed=5):
    """kind 0 float32, 1 16-bit containers, 2 float64"""
    raw = orc.synth_raw(*shape, seed=seed, kind='scene')
    if kind == 1:
        return torch.from_numpy((raw * 65535.0).astype(np.uint16).view(np.int16)).to(dev)
    return torch.from_numpy(raw.astype(np.float64 if kind == 2 else np.float32)).to(dev)


def module(dev):
    m = ParametrizedProcessing(orc.DRONE_CAMERA_PARAMS, batch_norm_output=True).to(dev)
    with torch.no_grad():        # (off the defaults, so that no gradient is zero by symmetry)
        m.gamma_correct.fill_(2.0)
        m.batch_norm.running_mean.copy_(torch.tensor([0.4, 0.45, 0.35]))
        m.batch_norm.running_var.copy_(torch.tensor([0.03, 0.05, 0.04]))
    return m


class Step:
    """the tensors of one training step and its direct C calls, entry by entry"""

    def __init__(self, lib, stream, raw, m):
        self.lib, self.stream, self.raw, self.dev = lib, stream, raw, raw.device
        self.u16 = int(raw.dtype in F.U16_DTYPES)
        self.dims = tuple(raw.shape)
        self.params = [p.detach().clone() for p in (m.black_level, m.white_balance, m.colour_correction, m.gamma_correct, m.debayer.weight,
                                                    m.sharpening_filter.weight, m.gaussian_blur.weight, m.M_RGB_2_YUV, m.M_YUV_2_RGB)]
        self.table = (ctypes.c_void_p * 9)(*[p.data_ptr() for p in self.params])
        self.nws = lib.r2l_isp_workspace_bytes(*self.dims)
        self.at = {k: lib.r2l_isp_step_offset(k, *self.dims) for k in (STATS, MOMENTS, SUMS, BN)}
        self.additive, self.epi = None, 0      # the additive layer and the R2L_STEP_EPI_* bits of the backward's calls

    def slot(self, ws, which, nbytes):
        return ws[self.at[which]:self.at[which] + nbytes].clone()

    def forward(self, entry, bn_mode, keep, io=F32, layout=NCHW, split=False):
        """-> (code, dict of everything the call leaves)"""
        lib, (B, H, W) = self.lib, self.dims
        ws = torch.full((self.nws,), 0xA5, dtype=torch.uint8, device=self.dev)
        out = torch.full((B, 3, H, W), -7.0, device=self.dev).to(torch.bfloat16 if io else torch.float32)
        rm, rv = torch.tensor([0.4, 0.45, 0.35], device=self.dev), torch.tensor([0.03, 0.05, 0.04], device=self.dev)
        nbt = torch.tensor(3, dtype=torch.int64, device=self.dev)

        def call(phase, gathered):
            head = (ptr(self.raw), self.u16, 65535.0, self.table, None, bn_mode, ptr(rm), ptr(rv), ptr(nbt), 1e-5, 0.1, ptr(out))
            tail = (ptr(ws), self.nws, B, H, W, 1, phase | keep, ptr(gathered), self.stream)
            if entry == 0:
                return lib.r2l_isp_step_fwd(*head, *tail)
            if entry == 1:
                return lib.r2l_isp_step_fwd_io(*head, io, *tail)
            return lib.r2l_isp_step_fwd_layout(*head, io, layout, *tail)
        code = call(ALL, None) if not split else call(A, None)
        if split and code == 0:
            code = call(B_, self.slot(ws, STATS, 56))
        left = dict(out=out, ws=ws, stats=self.slot(ws, STATS, 56), moments=self.slot(ws, MOMENTS, 56), bn=self.slot(ws, BN, 24), rm=rm,
                    rv=rv, nbt=nbt)
        return code, left

    def backward(self, entry, fwd, cot, bn_mode, mask=0, want_raw=False, io=F32, layout=NCHW, split=False, want_params=True, gadd=None):
        """behind the forward that left `fwd` (on a copy of its workspace) -> (code, grad_params | None, grad_raw | None)"""
        lib, (B, H, W) = self.lib, self.dims
        ws = fwd['ws'].clone()
        gp = torch.full((_lib.R2L_P_NTRAIN,), -7.0, device=self.dev) if want_params else None
        graw = torch.full((B, H, W), -7.0, device=self.dev) if want_raw else None
        nscr = lib.r2l_isp_raw_grad_scratch_bytes(B, H, W) if want_raw else 0
        scr = torch.empty(nscr, dtype=torch.uint8, device=self.dev) if want_raw else None

        def call(phase, gathered):
            mid = (ptr(gp), ptr(gadd), bn_mode, ptr(ws), self.nws, B, H, W, 1, phase | KEEP | self.epi, ptr(gathered), self.stream)
            raw3, rawgrad = (ptr(self.raw), self.u16, 65535.0, ptr(self.additive), ptr(cot)), (ptr(graw), ptr(scr), nscr)
            if entry == 0:
                return lib.r2l_isp_step_bwd(*raw3, ptr(fwd['out']), *mid)
            if entry == 1:
                return lib.r2l_isp_step_bwd_raw(*raw3, ptr(fwd['out']), *mid, *rawgrad)
            if entry == 2:
                return lib.r2l_isp_step_bwd_select(*raw3, ptr(fwd['out']), *mid, *rawgrad, mask)
            if entry == 3:
                return lib.r2l_isp_step_bwd_io(*raw3, io, ptr(fwd['out']), *mid, *rawgrad, mask)
            return lib.r2l_isp_step_bwd_layout(*raw3, io, layout, ptr(fwd['out']), *mid, *rawgrad, mask)
        code = call(ALL, None) if not split else call(A, None)
        if split and code == 0:
            code = call(B_, self.slot(ws, SUMS, 48))
        return code, gp, graw


def same(a, b, what):
    for k in a:
        if k != 'ws':
            assert torch.equal(a[k], b[k]), f'{what}: {k} differs'


def io16_served(lib, u16, shape):
    return bool(lib.r2l_isp_io_supported(BF16, u16, 0, *shape, KEEP))


def check_forward_flavours(lib, stream, dev):
    """step_fwd = step_fwd_io(F32) = step_fwd_layout(F32, NCHW), with and without KEEP_LUMA, whole and as phase A + phase B; step_fwd_io(bf16)
    = step_fwd_layout(bf16, NCHW)"""
    for shape, u16, bn_mode in itertools.product(SHAPES, (0, 1), (NONE, TRAIN, EVAL)):
        st = Step(lib, stream, frames(shape, u16, dev), module(dev))
        for keep in (0, KEEP):
            what = f'{shape} u16={u16} bn_mode={bn_mode} keep={keep}'
            code, first = st.forward(0, bn_mode, keep)
            assert code == 0, (what, lib.r2l_last_error())
            assert torch.isfinite(first['out']).all() and not (first['out'] == -7.0).all(), what
            for entry, split in itertools.product((0, 1, 2), (False, True) if bn_mode == TRAIN else (False,)):
                code, got = st.forward(entry, bn_mode, keep, split=split)
                assert code == 0, (what, entry, split, lib.r2l_last_error())
                same(first, got, f'{what}: {STEP_FWD[entry]}{" A+B" if split else ""}')
        codes, first16 = [], None
        for entry, split in itertools.product((1, 2), (False, True) if bn_mode == TRAIN else (False,)):
            code, got = st.forward(entry, bn_mode, KEEP, io=BF16, split=split)
            codes.append(code)
            if code == 0:
                first16 = first16 or got
                same(first16, got, f'{shape} u16={u16} bn_mode={bn_mode} bf16: {STEP_FWD[entry]}')
        assert set(codes) == ({0} if io16_served(lib, u16, shape) else {-3}), codes


def check_backward_flavours(lib, stream, dev):
    """behind a kept forward: the 132 gradients of step_bwd = _select(0) = _io(F32, 0) = _layout(F32, NCHW, 0); with d/d raw step_bwd_raw =
    _select(255) = _layout(F32, NCHW, 255) (where the plane passes are missing: the same -3); _io(bf16) = _layout(bf16, NCHW); phase A +
    phase B = ALL for each"""
    for shape, u16, bn_mode in itertools.product(SHAPES, (0, 1), (NONE, TRAIN, EVAL)):
        st = Step(lib, stream, frames(shape, u16, dev), module(dev))
        what = f'{shape} u16={u16} bn_mode={bn_mode}'
        cot = torch.from_numpy(np.random.default_rng(7).standard_normal((shape[0], 3) + shape[1:]).astype(np.float32)).to(dev)
        code, fwd = st.forward(2, bn_mode, KEEP)
        assert code == 0, what
        splits = (False, True) if bn_mode == TRAIN else (False,)

        def group(flavours, cot, fwd, expect_raw):
            answers = []
            for (entry, kw), split in itertools.product(flavours, splits):
                code, gp, graw = st.backward(entry, fwd, cot, bn_mode, split=split, **kw)
                answers.append((code, lib.r2l_last_error() if code else b'', gp, graw, f'{what}: {STEP_BWD[entry]} {kw} split={split}'))
            code0, err0, gp0, graw0, _ = answers[0]
            for code, err, gp, graw, name in answers[1:]:
                assert code == code0, (name, code, err)
                if code0 == 0:
                    assert torch.equal(gp, gp0), name
                    assert graw0 is None or torch.equal(graw, graw0), name
            if code0 == 0:
                assert torch.isfinite(gp0).all() and not (gp0 == -7.0).any(), what
                assert graw0 is None or (torch.isfinite(graw0).all() and not (graw0 == -7.0).all()), what
            assert (code0 == 0) == expect_raw, (what, code0, err0)
            return code0

        group([(0, {}), (2, dict(mask=0)), (3, dict(mask=0)), (4, dict(mask=0)), (1, {}), (2, dict(mask=127)), (4, dict(mask=127))], cot, fwd, True)
        if not u16:
            raw_served = io16_served(lib, 0, shape)      # (the same conditions: plane passes, W % 4 == 0, W <= 2048)
            code = group([(1, dict(want_raw=True)), (2, dict(mask=255, want_raw=True)), (3, dict(mask=255, want_raw=True)),
                          (4, dict(mask=255, want_raw=True))], cot, fwd, raw_served)
            assert code in (0, -3)
        if io16_served(lib, u16, shape):
            code, fwd16 = st.forward(2, bn_mode, KEEP, io=BF16)
            assert code == 0, what
            cot16 = cot.to(torch.bfloat16)
            group([(3, dict(io=BF16, mask=0)), (4, dict(io=BF16, mask=0)), (3, dict(io=BF16, mask=127)), (4, dict(io=BF16, mask=127))], cot16,
                  fwd16, True)
            if not u16:
                group([(3, dict(io=BF16, mask=255, want_raw=True)), (4, dict(io=BF16, mask=255, want_raw=True))], cot16, fwd16, True)


# (debayer, sharpening, denoising, options | None): the default chain, the short one, a Malvar2004 chain, two with a workspace
CHAINS = ((0, 1, 1, None), (0, 0, 0, None), (1, 2, 2, None), (0, 1, 3, None), (0, 1, 2, (1.0, 1.0, 0.5, 0.3, 5.0)))
CAMERA = (ctypes.c_double * 16)(*[float(v) for part in orc.DRONE_CAMERA_PARAMS for v in np.asarray(part).reshape(-1)])


def static_call(lib, stream, entry, raw, kind, chain, ws, nws, out, out_io=F32, ms=None, use_opts=True):
    deb, sh, dn, opts = chain
    (B, H, W), ov = raw.shape, ((ctypes.c_double * 5)(*opts) if (opts and use_opts) else None)
    tail = (B, H, W, CAMERA, deb, sh, dn, 2.2)
    if entry < 3:
        den = (65535.0,) if entry == 1 else ()
        return getattr(lib, STATIC_FWD[entry])(ptr(raw), *den, ptr(out), *tail, ptr(ws), nws, stream)
    if entry == 3:
        return lib.r2l_static_fwd_norm(ptr(raw), kind, 65535.0, ptr(out), *tail, ms, ptr(ws), nws, stream)
    if entry == 4:
        return lib.r2l_static_fwd_opts(ptr(raw), kind, 65535.0, ptr(out), *tail, ov, ms, ptr(ws), nws, stream)
    return lib.r2l_static_fwd_io(ptr(raw), kind, 65535.0, ptr(out), out_io, *tail, ov, ms, ptr(ws), nws, stream)


def check_static_flavours(lib, stream, dev, fft):
    """float32: static_fwd = _norm(NULL) = _opts(NULL, NULL) = _io(F32); 16-bit containers: _u16 = _io(frames = 1); float64: _f64 =
    _io(frames = 2); with options and mean_std: _opts = _io(F32); the workspace queries agree.  fft: rocFFT can run here"""
    for shape, chain in itertools.product(SHAPES, CHAINS):
        deb, sh, dn, opts = chain
        if dn == 3 and not fft:
            continue
        ov = (ctypes.c_double * 5)(*opts) if opts else None
        plain, f64 = lib.r2l_static_workspace_bytes(*shape, deb, sh, dn), lib.r2l_static_workspace_bytes_f64(*shape, deb, sh, dn)
        assert plain == lib.r2l_static_workspace_bytes_opts(0, *shape, deb, sh, dn, None)
        assert plain == lib.r2l_static_workspace_bytes_opts(1, *shape, deb, sh, dn, None)
        assert f64 == lib.r2l_static_workspace_bytes_opts(2, *shape, deb, sh, dn, None)
        for kind in (0, 1, 2):
            raw = frames(shape, kind, dev)
            nws = lib.r2l_static_workspace_bytes_opts(kind, *shape, deb, sh, dn, ov)
            ms = (ctypes.c_float * 6)(0.35, 0.36, 0.35, 0.12, 0.11, 0.12)

            def run(entry, **kw):
                ws = torch.empty(nws, dtype=torch.uint8, device=dev) if nws else None
                out = torch.full((shape[0], 3) + shape[1:], -7.0, device=dev)
                code = static_call(lib, stream, entry, raw, kind, chain, ws, nws, out, **kw)
                return code, (lib.r2l_last_error() if code else b''), out
            what = f'{shape} chain {chain} frames {kind}'
            groups = [[(4, dict(ms=ms)), (5, dict(ms=ms))]]
            if opts is None:
                groups += [[(kind, {}), (3, {}), (4, {}), (5, {})], [(3, dict(ms=ms)), (4, dict(ms=ms))]]
            for flavours in groups:
                code0, err0, out0 = run(flavours[0][0], **flavours[0][1])
                for entry, kw in flavours[1:]:
                    code, err, out = run(entry, **kw)
                    assert (code, err) == (code0, err0), (what, STATIC_FWD[entry], code, err, code0, err0)
                    assert torch.equal(out, out0), (what, STATIC_FWD[entry])
                assert code0 == 0 and torch.isfinite(out0).all() and not (out0 == -7.0).any(), (what, code0, err0)


class Recorder:
    """stands in for lib.cdll for the duration of a `with`: every C function called through the library, by name, in order"""

    def __init__(self, lib):
        self.lib, self.real, self.calls = lib, lib.cdll, []

    def __getattr__(self, name):
        fn = getattr(self.real, name)

        def call(*args):
            self.calls.append(name)
            return fn(*args)
        return call

    def __enter__(self):
        self.lib.cdll = self
        return self

    def __exit__(self, *exc):
        self.lib.cdll = self.real

    def entered(self):
        """the step and static calls among them (not the queries of sizes, offsets and predicates other than the static workspace's)"""
        return [n for n in self.calls if n in STEP_FWD + STEP_BWD + STATIC_FWD + STATIC_WS]


def python_cases(lib, dev):
    """(shape, u16, bn_mode, selective, frames require grad, output dtype, channels-last) the fused path serves here"""
    for shape, u16, bn_mode, sel, need_r, odt, nhwc in itertools.product(SHAPES, (0, 1), (NONE, TRAIN, EVAL), (False, True), (False, True),
                                                                         (None, torch.bfloat16), (False, True)):
        if need_r and (u16 or F._raw_grad_why(True, shape[2], False) or not io16_served(lib, 0, shape)):
            continue        # (d/d raw: float32 frames and the plane passes)
        if (odt is not None or nhwc) and not io16_served(lib, u16, shape):
            continue
        yield shape, u16, bn_mode, sel, need_r, odt, nhwc


def check_python_step(lib, stream, dev, pc):
    """every _IspFused call enters the library through r2l_isp_step_fwd_layout and r2l_isp_step_bwd_layout alone, once each, launches the
    kernels the legacy entry of such a call launches, and returns its bits"""
    n = 0
    for case in python_cases(lib, dev):
        python_case(lib, stream, dev, pc, *case)
        n += 1
    # an additive layer (256 x 256 frames; with the parameters' gradients and alone: mask 0, no grad_params) and an output epilogue
    # took r2l_isp_step_bwd, as every call with neither a mask, a 16-bit / channels-last tensor nor d/d raw did
    for frozen in ((0, 4), range(7)):
        python_case(lib, stream, dev, pc, (1, 256, 256), 0, TRAIN, False, False, None, False, additive=True, frozen=frozen)
    python_case(lib, stream, dev, pc, SHAPES[1], 0, NONE, False, False, None, False, epilogue=(1, 0, 0))
    python_case(lib, stream, dev, pc, SHAPES[1], 1, EVAL, True, False, None, False, epilogue=(0, 1, 2))
    return n


def python_case(lib, stream, dev, pc, shape, u16, bn_mode, sel, need_r, odt, nhwc, additive=False, frozen=(0, 4), epilogue=None):
    """frozen: the parameters (in PARAM_LAYOUT's order) that do not require grad"""
    what = f'{shape} u16={u16} bn_mode={bn_mode} selective={sel} raw grad={need_r} {odt} nhwc={nhwc} {additive} {tuple(frozen)} {epilogue}'
    m = module(dev)
    m.selective_backward = sel
    trainable = (m.black_level, m.white_balance, m.colour_correction, m.gamma_correct, m.debayer.weight, m.sharpening_filter.weight,
                 m.gaussian_blur.weight)
    for i in frozen:      # (a frozen part: the selective mask is not the full one)
        trainable[i].requires_grad_(False)
    if additive:
        m.additive_layer = torch.nn.Parameter(0.01 * torch.from_numpy(
            np.random.default_rng(3).standard_normal((1, 3) + shape[1:]).astype(np.float32)).to(dev))
    m2 = copy.deepcopy(m)
    raw = frames(shape, u16, dev)
    if need_r:
        raw.requires_grad_(True)
    io = F.IO_CODES[odt]
    cot = torch.from_numpy(np.random.default_rng(11).standard_normal((shape[0], 3) + shape[1:]).astype(np.float32)).to(dev)
    cot = cot.to(odt or torch.float32).contiguous(memory_format=torch.channels_last if nhwc else torch.contiguous_format)

    def python():
        y = F.isp_fused(raw, m, bn_mode, epilogue=epilogue, out_dtype=odt, out_layout=torch.channels_last if nhwc else None)
        y.backward(cot)
        return y.detach()
    with Recorder(lib) as rec:
        y, launched = pc.kernels_launched(lib, python)
    assert rec.entered() == ['r2l_isp_step_fwd_layout', 'r2l_isp_step_bwd_layout'], (what, rec.entered())

    # the legacy route of the same call: the entry functional.py chose before, with the mask and pointers it passed
    st = Step(lib, stream, raw.detach(), m2)
    st.additive, st.epi = (m2.additive_layer.detach() if additive else None), F.epilogue_bits(epilogue)
    needs = (need_r,) + tuple(i not in frozen for i in range(7))
    need_p = any(needs[1:])
    gadd = torch.full_like(st.additive, -7.0) if additive else None
    mask = F.grad_mask(needs) if sel else 0
    full = (F.GRAD_RAW if need_r else 0) | 127
    if nhwc:
        fe, be, kw = 2, 4, dict(io=io, layout=NHWC, mask=mask or full)
    elif io:
        fe, be, kw = 1, 3, dict(io=io, mask=mask or full)
    elif mask:
        fe, be, kw = 0, 2, dict(mask=mask)
    else:
        fe, be, kw = 0, (1 if need_r else 0), {}

    def legacy():
        lib, (B, H, W) = st.lib, st.dims
        bn = m2.batch_norm
        ws = torch.empty(st.nws, dtype=torch.uint8, device=dev)
        out = torch.empty((B, 3, H, W), dtype=odt or torch.float32, device=dev,
                          memory_format=torch.channels_last if nhwc else torch.contiguous_format)
        rm, rv, nbt = (bn.running_mean, bn.running_var, bn.num_batches_tracked if bn_mode == TRAIN else None) if bn_mode else (None,) * 3
        head = (ptr(raw.detach()), u16, 65535.0 if u16 else 1.0, st.table, ptr(st.additive), bn_mode, ptr(rm), ptr(rv), ptr(nbt), float(bn.eps),
                float(bn.momentum), ptr(out))
        tail = (ptr(ws), st.nws, B, H, W, 1, ALL | KEEP | st.epi, None, stream)
        lib.check((lib.r2l_isp_step_fwd(*head, *tail) if fe == 0 else lib.r2l_isp_step_fwd_io(*head, io, *tail) if fe == 1
                   else lib.r2l_isp_step_fwd_layout(*head, io, NHWC, *tail)), STEP_FWD[fe])
        code, gp, graw = st.backward(be, dict(ws=ws, out=out), cot, bn_mode, want_raw=need_r, want_params=need_p or need_r, gadd=gadd,
                                     **kw)
        lib.check(code, STEP_BWD[be])
        return out, gp, graw
    (out, gp, graw), legacy_launched = pc.kernels_launched(lib, legacy)
    assert launched == legacy_launched, (what, launched, legacy_launched)
    assert y.dtype == out.dtype and y.stride() == out.stride() and torch.equal(y, out), what
    for (name, off, k), p in zip(F.PARAM_LAYOUT, trainable):
        if p.requires_grad:
            assert torch.equal(p.grad.reshape(-1), gp[off:off + k]), (what, name)
        else:
            assert p.grad is None, (what, name)
    assert (raw.grad is None and graw is None) or torch.equal(raw.grad, graw), what
    for b, b2 in zip(m.batch_norm.buffers(), m2.batch_norm.buffers()):
        assert torch.equal(b, b2), what
    if additive:
        assert torch.equal(m.additive_layer.grad, gadd) and not (gadd == -7.0).any(), what


def check_python_static(lib, stream, dev, pc, fft):
    """static_pipeline: one r2l_static_workspace_bytes_opts and one r2l_static_fwd_io per call; the kernels and bits of the entry it took
    before (default: r2l_static_fwd; custom options with mean_std: r2l_static_fwd_opts; float64: r2l_static_fwd_f64)"""
    shape = SHAPES[1]
    ms = (0.35, 0.36, 0.35, 0.12, 0.11, 0.12)
    names = {0: 'bilinear', 1: 'malvar2004'}, {0: 'none', 1: 'sharpening_filter', 2: 'unsharp_masking'}, \
        {0: 'none', 1: 'gaussian_denoising', 2: 'median_denoising', 3: 'fft_denoising'}
    cases = [(0, CHAINS[0], None, 0), (0, CHAINS[4], ms, 4), (2, CHAINS[0], None, 2), (1, CHAINS[2], None, 1)]
    if fft:
        cases.append((0, CHAINS[3], None, 0))
    for kind, chain, mean_std, entry in cases:
        deb, sh, dn, opts = chain
        raw = frames(shape, kind, dev)
        kw = dict(zip(('sharp_radius', 'sharp_amount', 'gaussian_sigma', 'fft_fraction', 'median_kernel_size'), opts)) if opts else {}
        if opts:
            kw['median_kernel_size'] = int(kw['median_kernel_size'])
        with Recorder(lib) as rec:
            y, launched = pc.kernels_launched(lib, lambda: F.static_pipeline(raw, orc.DRONE_CAMERA_PARAMS, names[0][deb], names[1][sh],
                                                                             names[2][dn], mean_std=mean_std, **kw))
        assert rec.entered() == ['r2l_static_workspace_bytes_opts', 'r2l_static_fwd_io'], (chain, kind, rec.entered())
        ov = (ctypes.c_double * 5)(*opts) if opts else None
        nws = lib.r2l_static_workspace_bytes_opts(kind, *shape, deb, sh, dn, ov)
        if not opts:
            assert nws == (lib.r2l_static_workspace_bytes_f64 if kind == 2 else lib.r2l_static_workspace_bytes)(*shape, deb, sh, dn)

        def legacy():
            ws = torch.empty(nws, dtype=torch.uint8, device=dev) if nws else None
            out = torch.empty((shape[0], 3) + shape[1:], device=dev)
            msv = (ctypes.c_float * 6)(*mean_std) if mean_std else None
            lib.check(static_call(lib, stream, entry, raw, kind, chain, ws, nws, out, ms=msv), STATIC_FWD[entry])
            return out
        out, legacy_launched = pc.kernels_launched(lib, legacy)
        assert launched == legacy_launched, (chain, kind, launched, legacy_launched)
        assert torch.equal(y, out), (chain, kind)
