"""BatchNorm off its defaults on every route that finalizes it (shared by tests/test_bn_settings.py on the serial emulation and
tests/test_gpu_bn_settings.py on the gfx950 build).

References, both plain and in float64: the oracle (oracle/isp_oracle.py) with `bn=dict(..., eps=<the case's>)` for the output and the
gradients; a `torch.nn.BatchNorm2d(3, affine=False, eps, momentum, track_running_stats).double()` on the CPU, fed the oracle's output
without BatchNorm and driven through the same train() / eval() / reset_running_stats() calls as the module under test, for the
running statistics, `num_batches_tracked` and every sequence of steps.

Limits, all the project's own: `pc.out_tolerance` at the case's eps for the output, rtol 1e-5 / atol 1e-6 (check_param_case) for the
running statistics after every step, equality for the counter, `pc.frame_shapes_grad_limit` (check_frame_shapes(conditioning=True))
for the gradients on midtone frames of >= 256 pixels with parameters perturbed by 1 %.

POWER: before a case compares the library, the same reference evaluated at the DEFAULT setting (eps 1e-5, momentum 0.1, tracked
buffers; the case's mode) must miss the same limit by at least 50 x -- for every quantity that a knob of the case which differs from
the default acts on: eps on the output and the gradients (least sensitive parameter), momentum on the running statistics after the
case's steps.  A quantity no differing knob acts on (the output under eps = 1e-5, buffers that do not exist or that eval mode leaves
alone) has its own exact check instead (bit-unchanged buffers, no buffers at all, bit-equality with the train-mode run).  The
frame-content cases apply it too, except to the output of the `saturated` frames, which is 0 whatever eps is (check_frame_content)."""
import re

import numpy as np
import torch

import parity_checks as pc
from oracle import isp_oracle as orc
from raw2logit_amd import _lib
from raw2logit_amd import functional as F_
from raw2logit_amd.processing import pipeline_torch as ppt

POWER = 50.0
STATS_RTOL, STATS_ATOL = 1e-5, 1e-6     # check_param_case's bar on the running statistics
DEFAULT = dict(eps=1e-5, momentum=0.1, track=True, train=True)
SETTINGS = {
    1: dict(eps=1e-3, momentum=None, track=True, train=True),
    2: dict(eps=1e-2, momentum=0.5, track=True, train=True),
    3: dict(eps=1e-5, momentum=0.0, track=True, train=True),     # running statistics bit-unchanged, the counter counts
    4: dict(eps=1e-3, momentum=0.1, track=False, train=True),    # no buffers, and the module must not grow any
    5: dict(eps=1e-3, momentum=0.1, track=False, train=False),   # eval mode on batch statistics: the train-mode result bit for bit
    6: dict(eps=1e-3, momentum=0.1, track=True, train=False),    # eval mode on uneven running statistics, buffers bit-unchanged
    # a module that HAS buffers (built tracking, uneven statistics) whose track_running_stats is then set to False: torch normalises
    # with batch statistics in train mode and leaves buffers and counter bit-unchanged; in eval mode it uses the running statistics
    7: dict(eps=1e-3, momentum=0.1, track=False, kept=True, train=True),
    8: dict(eps=1e-3, momentum=0.1, track=False, kept=True, train=False),
}
UNEVEN_MEAN, UNEVEN_VAR = [0.4, 0.45, 0.35], [0.0004, 0.0008, 0.0006]

# route: the smallest shape that reaches it; `train` / `eval`: the entry of test_gpu_fwd_routes.CALLS whose launch names
# tests/golden/fwd_routes.txt records for the route (the names' frame-type and wavefront-count parts follow the case); nw: wavefronts
# per row of the streaming kernels
ROUTES = {
    'stream_w1': dict(shape=(2, 16, 16), train='split_apply', eval='stream_u16', nw=1),
    'stream_w2': dict(shape=(2, 8, 260), train='stats_apply', eval='stream_u16', nw=2),
    'stream_w4': dict(shape=(1, 8, 516), train='stats_apply', eval='stream_u16', nw=4),
    'stream_w8': dict(shape=(1, 8, 1028), train='stats_apply', eval='stream_u16', nw=8),
    'stats_apply_u16': dict(shape=(1, 8, 516), train='stats_apply', eval='stream_u16', nw=4, u16=True),
    'tile_ragged': dict(shape=(2, 32, 10), train='tile_ragged', eval='tile_ragged', nw=1),
    'tile_additive': dict(shape=(2, 256, 256), train='tile_additive', eval='tile_additive', nw=1, additive=True),
    'staged': dict(shape=(2, 16, 16), track_stages=True),
    'raw_grad': dict(shape=(2, 16, 16), raw_grad=True),
}
FULL_ROUTES = ('stream_w1', 'tile_ragged', 'staged')      # the full list of settings and the sequences


def setting_cases():
    """(route, setting, compare gradients): every route gets settings 1 and 4, and 5 and 6 for their gradients (compared at settings 1,
    5 and 6 wherever the frame has >= 256 pixels); the full list (7 and 8 with their gradients too) runs on FULL_ROUTES"""
    cases = []
    for name, route in ROUTES.items():
        _, H, W = route['shape']
        for n in (tuple(SETTINGS) if name in FULL_ROUTES else (1, 4, 5, 6)):
            cases.append((name, n, n in (1, 5, 6, 7, 8) and H * W >= 256))
    return cases


FOLDS = {'r2l_launch_fold_kernel', 'r2l_launch_pack_fold_kernel'}
_RECORD = {}


def recorded_names(call, u16=False, nw=1):
    """the kernels tests/golden/fwd_routes.txt records for entry `call` of test_gpu_fwd_routes.CALLS, without the parameter fold,
    as a call on float32 / 16-bit frames at `nw` wavefronts per row launches them.  The golden file has NO line for most of this
    module's shapes and frame types (`stats_apply` is recorded on 16-bit frames at 4 wavefronts and serves float32 frames at 2, 4 and
    8 here; `stream_u16` serves every eval-mode streaming case): what is asserted is the recorded route's set of kernels under the
    library's naming pattern (`_w<wavefronts>`, `_u16`), not a recorded line.  The staged and `raw_grad` routes are not in the
    record at all: they assert only whether the stand-alone finalize launch ran."""
    if not _RECORD:
        import fwd_routes_record
        import test_gpu_fwd_routes
        _RECORD.update(runs=fwd_routes_record.runs(), calls=test_gpu_fwd_routes.CALLS)
    names = set()
    for n in set(_RECORD['runs'][_RECORD['calls'][call]]['launches']) - FOLDS:
        core = re.sub(r'_w\d', f'_w{nw}', n[len('r2l_launch_'):-len('_kernel')].replace('_u16', ''))
        names.add('r2l_launch_' + core + ('_u16' if u16 else '') + '_kernel')
    return names


def on_device(device):
    return torch.device(device).type == 'cuda'


def launched(raw, fn):
    """fn() -> (its result, {kernel: launches})"""
    return pc.kernels_launched(_lib.library_for(raw)[0], fn)


def assert_route(names, call, route, device, label):
    """the route assertion applies where the device library serves the call (the serial emulation runs the tile forms)"""
    if on_device(device) and call is not None:
        want = recorded_names(call, route.get('u16', False), route.get('nw', 1))
        assert set(names) - FOLDS == want, (label, sorted(names), sorted(want))


def parameters(seed, additive=False, perturbed=True):
    P = orc.IspParams(orc.DRONE_CAMERA_PARAMS, dtype=np.float32)
    if additive:
        P.additive_layer = np.zeros((1, 3, 256, 256), dtype=np.float32)
    if perturbed:
        P.perturb(seed, 0.01)
    return P


def has_buffers(s):
    return bool(s['track'] or s.get('kept'))


def new_bn(s, dtype=torch.float32):
    """nn.BatchNorm2d of the settings; `kept`: built with buffers, track_running_stats set to False afterwards"""
    bn = torch.nn.BatchNorm2d(3, affine=False, eps=s['eps'], momentum=s['momentum'], track_running_stats=has_buffers(s)).to(dtype)
    bn.track_running_stats = bool(s['track'])
    return bn


def set_uneven(bn):
    with torch.no_grad():
        bn.running_mean.copy_(torch.tensor(UNEVEN_MEAN, dtype=bn.running_mean.dtype))
        bn.running_var.copy_(torch.tensor(UNEVEN_VAR, dtype=bn.running_var.dtype))


def make_module(P, s, device, route=None, uneven=False):
    """a ParametrizedProcessing with the parameters P and a FRESH nn.BatchNorm2d of the case's settings as m.batch_norm"""
    route = route or {}
    m = ppt.ParametrizedProcessing(orc.DRONE_CAMERA_PARAMS, track_stages=route.get('track_stages', False), batch_norm_output=True)
    if P.additive_layer is not None:
        ppt.append_additive_layer(m)
    with torch.no_grad():
        for k, v in P.by_name().items():
            pc.NAME2ATTR[k](m).copy_(torch.from_numpy(np.asarray(v)))
    m.batch_norm = new_bn(s)
    if uneven:
        set_uneven(m.batch_norm)
    if route.get('u16'):
        m.raw_bits = 12
    return m.to(device).train(s['train'])


def frames_for(route, raw_np, device):
    """midtone / content frames (12-bit levels / 4095) as the tensor the route takes"""
    if route.get('u16'):
        return torch.from_numpy(np.round(raw_np.astype(np.float64) * 4095).astype(np.int16)).to(device)
    t = torch.from_numpy(raw_np).to(device)
    return t.requires_grad_(True) if route.get('raw_grad') else t


def oracle_bn(s, ref):
    """the oracle's `bn` dict for a step under settings s in front of the float64 nn.BatchNorm2d `ref` (its buffers BEFORE the step)"""
    if s['train'] or ref.running_mean is None:      # (torch: batch statistics in train mode and wherever there are no buffers)
        return dict(training=True, running_mean=np.zeros(3), running_var=np.ones(3), eps=s['eps'])
    return dict(training=False, running_mean=ref.running_mean.numpy().copy(), running_var=ref.running_var.numpy().copy(), eps=s['eps'])


def stats_excess(got, want):
    """largest |got - want| / (atol + rtol |want|): <= 1 passes check_param_case's bar"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float((np.abs(got - want) / (STATS_ATOL + STATS_RTOL * np.abs(want))).max())


def compare_stats(label, bn, ref):
    """running statistics and the counter of the module under test against the float64 nn.BatchNorm2d"""
    if ref.running_mean is None:
        assert bn.running_mean is None and bn.running_var is None and bn.num_batches_tracked is None, label
        assert list(bn.buffers()) == [], label
        return
    for name in ('running_mean', 'running_var'):
        e = stats_excess(getattr(bn, name).detach().cpu().numpy(), getattr(ref, name).numpy())
        pc.report(f'{label}/{name} vs float64 nn.BatchNorm2d, in units of atol 1e-6 + rtol 1e-5', e, 1.0)
        assert e <= 1.0, (label, name, getattr(bn, name), getattr(ref, name))
    assert int(bn.num_batches_tracked) == int(ref.num_batches_tracked), (label, bn.num_batches_tracked, ref.num_batches_tracked)


def stats_power(label, ref, ref_default):
    """the reference driven at the default momentum misses the running-statistics bar by >= POWER x"""
    miss = max(stats_excess(ref_default.running_mean.numpy(), ref.running_mean.numpy()),
               stats_excess(ref_default.running_var.numpy(), ref.running_var.numpy()))
    pc.report(f'{label}/POWER: default momentum misses the running-statistics bar by this factor (>= {POWER:g}; not an error)',
              POWER, max(miss, 1e-300))
    assert miss >= POWER, (label, 'the momentum cannot be seen through the limit', miss)


def compare_output(label, y, raw_np, P64, s, ref, default_differs=True):
    """output against the float64 oracle at the case's eps (`ref`: the float64 BatchNorm BEFORE its step) -> the oracle's cache"""
    o, _, cache = orc.parametrized_forward(raw_np, P64, bn=oracle_bn(s, ref))
    tol = pc.out_tolerance(cache, True)
    if default_differs and s['eps'] != DEFAULT['eps']:
        o0, _, _ = orc.parametrized_forward(raw_np, P64, bn=oracle_bn(dict(s, eps=DEFAULT['eps']), ref))
        miss = float((np.abs(o0 - o) / tol).max())
        pc.report(f'{label}/POWER: default eps misses the output limit by this factor (>= {POWER:g}; not an error)', POWER, miss)
        assert miss >= POWER, (label, 'eps cannot be seen through the output limit', miss)
    err = np.abs(y.detach().float().cpu().numpy() - o)
    worst = np.unravel_index((err / tol).argmax(), err.shape)
    pc.report(f'{label}/out vs float64 oracle', err[worst], tol[worst])
    assert np.all(err <= tol), (label, 'out vs oracle', err.max(), err[worst], tol[worst])
    return o, cache


def module_grads(m):
    return {k: f(m).grad.detach().cpu().numpy() for k, f in pc.NAME2ATTR.items() if k != 'additive_layer' or m.additive_layer is not None}


def compare_grads(label, got_by_name, raw_np, P, s, ref_before, cache, cot):
    """the parameter gradients (by state_dict name) against the float64 oracle at check_frame_shapes(conditioning=True)'s limit"""
    B, H, W = raw_np.shape
    assert H * W >= 256, 'the limit holds on frames of at least 256 pixels'
    P64, P32 = P.astype(np.float64), P.astype(np.float32)
    assert cache['rgb'].min() > 0.05 and cache['rgb'].max() < 0.95, (cache['rgb'].min(), cache['rgb'].max())
    g, _, _ = orc.parametrized_backward(P64, cache, cot)
    glo, _, _ = orc.parametrized_backward(P64, cache, cot, clip_shift=1e-6)
    ghi, _, _ = orc.parametrized_backward(P64, cache, cot, clip_shift=-1e-6)
    _, _, c32 = orc.parametrized_forward(raw_np, P32, bn=oracle_bn(s, ref_before))
    g32, _, _ = orc.parametrized_backward(P32, c32, cot)
    _, _, c0 = orc.parametrized_forward(raw_np, P64, bn=oracle_bn(dict(s, eps=DEFAULT['eps']), ref_before))
    g0, _, _ = orc.parametrized_backward(P64, c0, cot)
    limits = {k: pc.frame_shapes_grad_limit(np.asarray(g[k]), glo[k], ghi[k], cot.size, True, g32[k]) for k in g}
    if s['eps'] != DEFAULT['eps']:      # before the library is compared
        miss = min(np.abs(np.asarray(g0[k]).reshape(np.asarray(g[k]).shape) - np.asarray(g[k])).max() / limits[k] for k in g)
        pc.report(f'{label}/POWER: default eps misses the LEAST sensitive gradient limit by this factor (>= {POWER:g}; not an error)',
                  POWER, miss)
        assert miss >= POWER, (label, 'eps cannot be seen through the gradient limits', miss)
    worst = 0.0
    for k in g:
        r, lim = np.asarray(g[k]), limits[k]
        got = np.asarray(got_by_name[k]).reshape(r.shape)
        e = np.abs(got - r).max()
        pc.report(f'{label}/grad {k} vs float64 oracle', e, lim)
        worst = max(worst, e / lim)
        assert e <= lim, (label, k, e, lim)
    return worst


def check_setting(route_name, n, device, grads=False, seed=0):
    """one step of setting n on a route: the launch names, output, running statistics, counter, and (grads) every gradient"""
    route, s = ROUTES[route_name], SETTINGS[n]
    B, H, W = route['shape']
    label = f'bn/{route_name}/setting{n}'
    raw_np = pc.midtone_frames(B, H, W, seed=20 + seed)
    P = parameters(31 + seed, route.get('additive', False))
    P64 = P.astype(np.float64)
    uneven = has_buffers(s) and (not s['train'] or s['momentum'] == 0.0 or not s['track'])
    m = make_module(P, s, device, route, uneven)
    ref, ref0 = new_bn(s, torch.float64).train(s['train']), new_bn(dict(DEFAULT, track=s['track'], kept=s.get('kept')), torch.float64).train(s['train'])
    if uneven:
        set_uneven(ref), set_uneven(ref0)
    before = new_bn(s, torch.float64)
    before.load_state_dict(ref.state_dict())
    state0 = {k: v.clone() for k, v in m.batch_norm.state_dict().items()}
    raw = frames_for(route, raw_np, device)
    y, names = launched(raw, lambda: m(raw))
    assert y.shape == (B, 3, H, W) and y.dtype == torch.float32
    batch = s['train'] or not has_buffers(s)
    if 'train' in route:
        assert_route(names, route['train' if batch else 'eval'], route, device, label)
    elif on_device(device):     # the staged path: the stand-alone finalize launch in train mode, none in eval mode on running statistics
        assert ('r2l_launch_bn_finalize_kernel' in names) == batch, (label, sorted(names))
    o, cache = compare_output(label, y, raw_np, P64, s, before)
    x = torch.from_numpy(np.asarray(orc.parametrized_forward(raw_np, P64, bn=None)[0], dtype=np.float64))
    ref(x), ref0(x)
    compare_stats(label, m.batch_norm, ref)
    assert sorted(m.batch_norm.state_dict()) == sorted(state0), (label, 'the module grew or lost buffers', sorted(m.batch_norm.state_dict()))
    if s['track'] and s['train'] and s['momentum'] != 0.0:
        stats_power(label, ref, ref0)
    if uneven:      # momentum 0 / eval mode / tracking switched off: the running statistics stay bit-unchanged; only a tracking train step counts
        for k in ('running_mean', 'running_var'):
            assert torch.equal(m.batch_norm.state_dict()[k], state0[k]), (label, k, 'must be bit-unchanged')
        assert int(m.batch_norm.num_batches_tracked) == int(state0['num_batches_tracked']) + int(s['train'] and s['track']), label
    twin = None
    if not has_buffers(s) and not s['train']:       # eval mode without buffers == train mode, bit for bit
        twin = make_module(P, dict(s, train=True), device, route)
        raw2 = frames_for(route, raw_np, device)
        y2 = twin(raw2)
        assert torch.equal(y, y2), (label, 'eval mode on batch statistics differs from train mode')
    if grads:
        cot = np.random.default_rng(40 + seed).standard_normal((B, 3, H, W)).astype(np.float32)
        (y * torch.from_numpy(cot).to(device)).sum().backward()
        compare_grads(label, module_grads(m), raw_np, P, s, before, cache, cot)
        if twin is not None:
            (y2 * torch.from_numpy(cot).to(device)).sum().backward()
            for k, f in pc.NAME2ATTR.items():
                if k != 'additive_layer' or P.additive_layer is not None:
                    assert torch.equal(f(m).grad, f(twin).grad), (label, k, 'eval-mode gradient differs from train mode')
            if route.get('raw_grad'):
                assert torch.equal(raw.grad, raw2.grad), label


def check_sequence(route_name, n, device):
    """four train steps, one eval step on the statistics just accumulated, reset_running_stats(), two more train steps -- different
    frames every step; output, running statistics and counter after every step; the default momentum's miss at the end"""
    route, s = ROUTES[route_name], SETTINGS[n]
    assert s['track'] and s['train']
    B, H, W = route['shape']
    label = f'bn/{route_name}/sequence{n}'
    P = parameters(57, route.get('additive', False))
    P64 = P.astype(np.float64)
    m = make_module(P, s, device, route)
    ref, ref0 = new_bn(s, torch.float64), new_bn(DEFAULT, torch.float64)
    step = 0
    for phase in ('train', 'train', 'train', 'train', 'eval', 'reset', 'train', 'train'):
        if phase == 'reset':
            for b in (m.batch_norm, ref, ref0):
                b.reset_running_stats()
            assert int(m.batch_norm.num_batches_tracked) == 0
            continue
        train = phase == 'train'
        for b in (m, ref, ref0):
            b.train(train)
        raw_np = pc.midtone_frames(B, H, W, seed=60 + step)
        before = new_bn(s, torch.float64)
        before.load_state_dict(ref.state_dict())
        state0 = {k: v.clone() for k, v in m.batch_norm.state_dict().items()}
        y = m(frames_for(route, raw_np, device))
        compare_output(f'{label}/step{step}_{phase}', y, raw_np, P64, dict(s, train=train), before)
        x = torch.from_numpy(np.asarray(orc.parametrized_forward(raw_np, P64, bn=None)[0], dtype=np.float64))
        ref(x), ref0(x)
        compare_stats(f'{label}/step{step}_{phase}', m.batch_norm, ref)
        if not train:
            for k, v in m.batch_norm.state_dict().items():
                assert torch.equal(v, state0[k]), (label, k, 'an eval step changed the buffers')
        step += 1
    assert int(m.batch_norm.num_batches_tracked) == 2
    stats_power(label, ref, ref0)


def check_opt_in_io(which, device):
    """setting 1 with output_dtype=torch.bfloat16 / output_memory_format=torch.channels_last: bit-identical to the float32 planar
    call + torch's cast / contiguous(memory_format=...), running statistics bit-identical; the gradients of the 16-bit / channels-last
    cotangent (the backward's recomputing BatchNorm-sums routes under a non-default eps) against the float64 oracle"""
    route, s = ROUTES['stream_w1'], SETTINGS[1]
    B, H, W = route['shape']
    label = f'bn/io_{which}/setting1'
    raw_np = pc.midtone_frames(B, H, W, seed=23)
    P = parameters(34)
    raw = torch.from_numpy(raw_np).to(device)
    m32, mio = make_module(P, s, device), make_module(P, s, device)
    if which == 'bf16':
        mio.output_dtype = torch.bfloat16
    else:
        mio.output_memory_format = torch.channels_last
    y32 = m32(raw)
    y, fwd_names = launched(raw, lambda: mio(raw))
    want = y32.detach().to(torch.bfloat16) if which == 'bf16' else y32.detach().contiguous(memory_format=torch.channels_last)
    assert y.dtype == want.dtype and y.is_contiguous(memory_format=torch.channels_last if which == 'nhwc' else torch.contiguous_format)
    assert torch.equal(y.detach(), want), (label, 'output')
    for k, v in m32.batch_norm.state_dict().items():
        assert torch.equal(v, mio.batch_norm.state_dict()[k]), (label, k)
    before = new_bn(s, torch.float64)
    _, cache = compare_output(label, y32, raw_np, P.astype(np.float64), s, before)
    cot_t = torch.from_numpy(np.random.default_rng(43).standard_normal((B, 3, H, W)).astype(np.float32)).to(device).to(y.dtype)
    _, bwd_names = launched(raw, lambda: y.backward(cot_t.contiguous(memory_format=torch.channels_last) if which == 'nhwc' else cot_t))
    if on_device(device):
        suffix = '_bf16_kernel' if which == 'bf16' else '_nhwc_kernel'
        assert any(k.startswith('r2l_launch_fwd_apply') and k.endswith(suffix) for k in fwd_names), (label, sorted(fwd_names))
        assert any(k.startswith('r2l_launch_bnr_') and k.endswith(suffix) for k in bwd_names), (label, sorted(bwd_names))
    compare_grads(label, module_grads(mio), raw_np, P, s, before, cache, cot_t.float().cpu().numpy())


# ---- frame content -----------------------------------------------------------------------------------------------------------------
CONTENT_KINDS = ('lowcontrast', 'edge', 'saturated', 'scene', 'dark')
CONTENT_SHAPES = ((2, 16, 24), (2, 70, 134))
CONTENT_SHAPES_GPU = ((2, 8, 260), (1, 8, 516))


def content_frames(kind, B, H, W, seed):
    """12-bit levels / 4095, float32.  lowcontrast: levels 1200..1202 at random; edge: top third 300..319, the rest 3000..3019, the right
    half replaced by 4095 minus itself (a horizontal edge inside the first band, a vertical one mid-row); saturated: all ones (R and B
    clip to exactly 1: variance exactly 0, istd = 1 / sqrt(eps)); scene, dark: orc.synth_raw"""
    rng = np.random.default_rng(seed)
    if kind in ('scene', 'dark'):
        return orc.synth_raw(B, H, W, seed=seed, kind=kind)
    if kind == 'saturated':
        return np.ones((B, H, W), np.float32)
    if kind == 'lowcontrast':
        u = 1200 + rng.integers(0, 3, (B, H, W))
    else:
        assert kind == 'edge'
        u = rng.integers(300, 320, (B, H, W))
        u[:, H // 3:, :] = rng.integers(3000, 3020, (B, H - H // 3, W))
        u[:, :, W // 2:] = 4095 - u[:, :, W // 2:]
    return (u.astype(np.float32) / np.float32(4095)).astype(np.float32)


def check_frame_content(kind, shape, s, device):
    """three train steps on frames that are not smooth: output and running statistics (no gradients) at the usual limits -- the
    statistics are float32 sums about a per-lane pivot taken from the first pixel the lane sees.  POWER under setting 2: the default
    eps must miss the output limit on every kind but `saturated` (there R and B equal their mean exactly, G nearly: the output is 0
    whatever eps is, and the case is about the variance clamp and the statistics, which the running-statistics bar judges); the
    default momentum must miss the running-statistics bar after the three steps on every kind"""
    B, H, W = shape
    label = f'bn/content_{kind}/{B}x{H}x{W}/eps{s["eps"]:g}'
    P = parameters(0, perturbed=False)
    P64 = P.astype(np.float64)
    m = make_module(P, s, device)
    ref, ref0 = new_bn(s, torch.float64), new_bn(DEFAULT, torch.float64)
    for step in range(3):
        raw_np = content_frames(kind, B, H, W, 10 + step)
        before = new_bn(s, torch.float64)
        before.load_state_dict(ref.state_dict())
        with torch.no_grad():
            y = m(torch.from_numpy(raw_np).to(device))
        compare_output(f'{label}/step{step}', y, raw_np, P64, s, before, default_differs=kind != 'saturated')
        x = torch.from_numpy(np.asarray(orc.parametrized_forward(raw_np, P64, bn=None)[0], dtype=np.float64))
        ref(x), ref0(x)
        compare_stats(f'{label}/step{step}', m.batch_norm, ref)
    if s['momentum'] != DEFAULT['momentum']:
        stats_power(label, ref, ref0)


# ---- the C ABI: phase A + r2l_bn_finalize + phase B, r2l_isp_fwd_stats_bn -------------------------------------------------------------
NONE, TRAIN, EVAL = 0, 1, 2
STEP_ALL, STEP_A, STEP_B, KEEP = 0, 1, 2, 8
STEP_STATS, STEP_MOMENTS, STEP_BN_SUMS, STEP_BN = 0, 1, 2, 4


def _abi_case(n, shape, device, seed):
    s = SETTINGS[n]
    assert s['train']
    B, H, W = shape
    raw_np = pc.midtone_frames(B, H, W, seed=20 + seed)
    P = parameters(31 + seed)
    raw = torch.from_numpy(raw_np).to(device)
    lib, stream = _lib.library_for(raw)
    packed = torch.from_numpy(P.pack()).to(device)
    rm = rv = nbt = None
    if s['track']:
        rm, rv = torch.tensor(UNEVEN_MEAN, device=device), torch.tensor(UNEVEN_VAR, device=device)
        nbt = torch.full((1,), 4, dtype=torch.int64, device=device)
    nws = lib.r2l_isp_workspace_bytes(B, H, W)
    ws = torch.zeros(nws, dtype=torch.uint8, device=device)
    out = torch.zeros((B, 3, H, W), device=device)
    mom = -1.0 if s['momentum'] is None else float(s['momentum'])
    return s, raw_np, P, raw, lib, stream, packed, rm, rv, nbt, nws, ws, out, mom


def _abi_reference(label, s, raw_np, P, out, rm, rv, nbt):
    """output, running statistics (from the uneven state, counter at 4) and counter of one train step through the C ABI"""
    P64 = P.astype(np.float64)
    ref, ref0 = new_bn(s, torch.float64), new_bn(dict(DEFAULT, track=s['track']), torch.float64)
    if s['track']:
        for b in (ref, ref0):
            set_uneven(b)
            b.num_batches_tracked.fill_(4)
    _, cache = compare_output(label, out, raw_np, P64, s, ref)
    if s['track']:
        x = torch.from_numpy(np.asarray(orc.parametrized_forward(raw_np, P64, bn=None)[0], dtype=np.float64))
        ref(x), ref0(x)
        for name, got, want in (('running_mean', rm, ref.running_mean), ('running_var', rv, ref.running_var)):
            e = stats_excess(got.cpu().numpy(), want.numpy())
            pc.report(f'{label}/{name} vs float64 nn.BatchNorm2d, in units of atol 1e-6 + rtol 1e-5', e, 1.0)
            assert e <= 1.0, (label, name, got, want)
        assert int(nbt) == 5, (label, nbt)
        if s['momentum'] != 0.0:
            stats_power(label, ref, ref0)
    return cache


def check_abi_phases(n, device, shape=(2, 16, 16), seed=5):
    """the multi-rank step's stand-alone finalize launch on one rank: r2l_isp_step_fwd phase A, r2l_bn_finalize on the statistics it
    left (into buffers of its own), phase B with the same statistics as `gathered` -- phase B's BatchNorm constants, moments and running
    statistics equal r2l_bn_finalize's bit for bit, and output / running statistics / counter meet the usual limits"""
    s, raw_np, P, raw, lib, stream, packed, rm, rv, nbt, nws, ws, out, mom = _abi_case(n, shape, device, seed)
    B, H, W = shape
    label = f'bn/abi_phases/setting{n}'
    p = _lib.ptr
    import ctypes
    offsets = [o for _, o, _ in F_.PARAM_LAYOUT] + [132, 141]
    assert len(offsets) == 9
    table = (ctypes.c_void_p * 9)(*[packed.data_ptr() + 4 * o for o in offsets])

    def fwd(phase, gathered):
        return lib.r2l_isp_step_fwd(p(raw), 0, 1.0, table, None, TRAIN, p(rm), p(rv), p(nbt), s['eps'], mom, p(out), p(ws), nws,
                                    B, H, W, 1, phase | KEEP, p(gathered), stream)
    e, names = pc.kernels_launched(lib, lambda: fwd(STEP_A, None))
    assert e == 0, lib.r2l_last_error()
    assert_route(names, 'phase_a', dict(nw=1), device, label)
    off = lib.r2l_isp_step_offset(STEP_STATS, B, H, W)
    stats = ws[off:off + 56].view(torch.float64).clone()
    assert float(stats[6]) == B * H * W
    rm2, rv2, nbt2 = (t.clone() if t is not None else None for t in (rm, rv, nbt))
    bn2, moments2 = torch.zeros(6, device=device), torch.zeros(7, dtype=torch.float64, device=device)
    assert lib.r2l_bn_finalize(p(stats), 1, p(bn2), p(moments2), p(rm2), p(rv2), p(nbt2), s['eps'], mom, stream) == 0
    e, names = pc.kernels_launched(lib, lambda: fwd(STEP_B, stats))
    assert e == 0, lib.r2l_last_error()
    if on_device(device):
        assert 'r2l_launch_bn_finalize_kernel' in names and 'r2l_launch_fwd_apply_kernel' in names, sorted(names)
    ob, om = lib.r2l_isp_step_offset(STEP_BN, B, H, W), lib.r2l_isp_step_offset(STEP_MOMENTS, B, H, W)
    assert torch.equal(ws[ob:ob + 24].view(torch.float32), bn2), label
    assert torch.equal(ws[om:om + 56].view(torch.float64), moments2), label
    if s['track']:
        assert torch.equal(rm, rm2) and torch.equal(rv, rv2) and torch.equal(nbt, nbt2), label
    cache = _abi_reference(label, s, raw_np, P, out, rm, rv, nbt)
    # the backward of the same step in its two phases: the BatchNorm sums of phase A handed back to phase B as `gathered`
    cot = np.random.default_rng(40 + seed).standard_normal((B, 3, H, W)).astype(np.float32)
    cot_t, gp = torch.from_numpy(cot).to(device), torch.zeros(_lib.R2L_P_NTRAIN, device=device)

    def bwd(phase, gathered):
        return lib.r2l_isp_step_bwd(p(raw), 0, 1.0, None, p(cot_t), p(out), p(gp), None, TRAIN, p(ws), nws, B, H, W, 1, phase | KEEP,
                                    p(gathered), stream)
    assert bwd(STEP_A, None) == 0, lib.r2l_last_error()
    osum = lib.r2l_isp_step_offset(STEP_BN_SUMS, B, H, W)
    sums = ws[osum:osum + 48].view(torch.float64).clone()
    assert bwd(STEP_B, sums) == 0, lib.r2l_last_error()
    got = {k: gp[o:o + cnt].cpu().numpy() for k, o, cnt in F_.PARAM_LAYOUT}
    compare_grads(label, got, raw_np, P, s, new_bn(s, torch.float64), cache, cot)


def check_abi_stats_bn(n, device, shape=(2, 8, 260), seed=6):
    """r2l_isp_fwd_stats_bn (statistics pass + bookkeeping in one launch, the entry's own argument block), then the apply pass of
    r2l_isp_fwd with R2L_F_FOLDED_VALID on the constants it wrote"""
    s, raw_np, P, raw, lib, stream, packed, rm, rv, nbt, nws, ws, out, mom = _abi_case(n, shape, device, seed)
    B, H, W = shape
    label = f'bn/abi_stats_bn/setting{n}'
    p = _lib.ptr
    stats, moments = torch.zeros(7, dtype=torch.float64, device=device), torch.zeros(7, dtype=torch.float64, device=device)
    bn = torch.zeros(6, device=device)
    e, names = pc.kernels_launched(lib, lambda: lib.r2l_isp_fwd_stats_bn(p(raw), p(packed), None, p(stats), p(bn), p(moments), p(rm), p(rv),
                                                                          p(nbt), s['eps'], mom, p(ws), nws, B, H, W, stream))
    assert e == 0, lib.r2l_last_error()
    assert_route(names, 'stats_only', dict(nw=2), device, label)
    assert lib.r2l_isp_fwd(p(raw), p(packed), None, p(bn), p(out), None, p(ws), nws, B, H, W, _lib.R2L_F_FOLDED_VALID, stream) == 0, \
        lib.r2l_last_error()
    assert float(stats[6]) == B * H * W and float(moments[6]) == B * H * W
    # (the constants `bn` / `moments` are judged through what they produce: the output and the running statistics)
    _abi_reference(label, s, raw_np, P, out, rm, rv, nbt)


# ---- r2l_bn_finalize directly ---------------------------------------------------------------------------------------------------
def _ulps32(got, want):
    """|got - float32(want)| in units of float32(want)'s spacing"""
    w32 = np.asarray(want, dtype=np.float64).astype(np.float32)
    return float((np.abs(np.asarray(got, dtype=np.float64) - w32.astype(np.float64)) / np.spacing(np.abs(w32)).astype(np.float64)).max())


def check_finalize_direct(device):
    """synthetic stats[nranks][7] (per channel sum (x - .5), sum (x - .5)^2, then the pixel count) through r2l_bn_finalize against the
    closed form in exact rational arithmetic (fractions.Fraction; the square root and the momentum blend in float64): nranks 1, 2, 3,
    8, uneven pixel counts per rank, n = 1 (the n > 1 ? n - 1 : 1 arm), a channel whose second moment puts the variance below zero,
    momentum 0.1 / 0.0 / 1.0 / cumulative with the counter at 0 and at 4, `moments`, the three buffers and all of them NULL.
    Limits: 2 ulp of the float32-rounded closed form for bn[6] and the running statistics (the device rounds ONE float64 result that
    differs from the closed form's by a few float64 ulps, so it lands on the same float32 or its neighbour), 1e-14 relative for the
    float64 moments (means <= 0.1 in magnitude, variances >= 0.02: the cancellation in s2 / n - m1^2 costs a few ulps of 0.11, i.e.
    < 3e-15 of the variance), the counter exact."""
    from fractions import Fraction as Fr
    rng = np.random.default_rng(7)
    lib, stream = _lib.library_for(torch.zeros(1, device=device))
    p = _lib.ptr
    worst = dict(bn=0.0, running=0.0, moments=0.0)
    cases = []
    for nranks in (1, 2, 3, 8):
        for mom, nbt0 in ((0.1, 0), (0.0, 2), (1.0, 7), (-1.0, 0), (-1.0, 4)):
            cases.append((nranks, mom, nbt0, 'all', False, False))
    cases += [(2, 0.1, 0, 'no_moments', False, False), (3, -1.0, 4, 'no_buffers', False, False), (8, 0.5, 1, 'none', False, False),
              (1, 0.1, 3, 'all', True, False), (1, -1.0, 0, 'all', True, False), (2, 0.1, 0, 'all', False, True),
              (3, -1.0, 4, 'all', False, True)]
    for nranks, mom, nbt0, have, single_pixel, negative in cases:
        eps = float(rng.choice([1e-5, 1e-3, 1e-2]))
        n = np.ones(nranks) if (single_pixel and nranks == 1) else rng.integers(100, 5000, nranks).astype(np.float64)
        m1, v = rng.uniform(-0.1, 0.1, (nranks, 3)), rng.uniform(0.02, 0.1, (nranks, 3))
        if single_pixel:        # one pixel: dyadic numbers, so that s2 / n - m1^2 = 1 / 1024 is exact (nothing to cancel against)
            m1, v = rng.integers(-6, 7, (nranks, 3)) / 64.0, np.full((nranks, 3), 1.0 / 1024)
        tot = np.concatenate([m1 * n[:, None], (v + m1 * m1) * n[:, None], n[:, None]], axis=1)
        if negative:            # channel 1 of the last rank: second moments that put the variance of the whole batch clearly below zero
            N, s1 = tot[:, 6].sum(), tot[:, 1].sum()
            tot[:, 4] = (s1 / N) ** 2 * tot[:, 6] * (1 - 1e-9)
        T = torch.from_numpy(tot.copy()).to(device)
        bn = torch.full((6,), np.nan, device=device)
        moments = torch.full((7,), np.nan, dtype=torch.float64, device=device) if have in ('all', 'no_buffers') else None
        rm0, rv0 = np.array([0.1, -0.2, 0.3], np.float32), np.array([1.0, 2.0, 0.03], np.float32)
        buffers = have in ('all', 'no_moments')
        rm, rv = (torch.from_numpy(rm0.copy()).to(device), torch.from_numpy(rv0.copy()).to(device)) if buffers else (None, None)
        nbt = torch.full((1,), nbt0, dtype=torch.int64, device=device) if buffers else None
        e = lib.r2l_bn_finalize(p(T), nranks, p(bn), p(moments), p(rm), p(rv), p(nbt), eps, mom, stream)
        assert e == 0, lib.r2l_last_error()
        # the closed form
        N = sum(Fr(float(x)) for x in tot[:, 6])
        mean = [sum(Fr(float(x)) for x in tot[:, c]) / N for c in range(3)]
        var = [max(sum(Fr(float(x)) for x in tot[:, 3 + c]) / N - mean[c] ** 2, Fr(0)) for c in range(3)]
        if negative:
            assert sum(Fr(float(x)) for x in tot[:, 4]) / N - mean[1] ** 2 < 0
        want_bn = [float(mu + Fr(1, 2)) for mu in mean] + [1.0 / np.sqrt(float(vv + Fr(eps))) for vv in var]
        label = f'bn/finalize nranks {nranks} momentum {mom:g} counter {nbt0} {have}' + (' n=1' if single_pixel else '') + \
            (' negative variance' if negative else '')
        u = _ulps32(bn.cpu().numpy(), want_bn)
        worst['bn'] = max(worst['bn'], u)
        assert u <= 2, (label, 'bn', bn, want_bn)
        if negative:
            assert float(bn[4]) == np.float32(1.0 / np.sqrt(eps)), (label, bn)
        if moments is not None:
            got = moments.cpu().numpy()
            want = np.array([float(mu + Fr(1, 2)) for mu in mean] + [float(vv) for vv in var] + [float(N)])
            if negative:
                assert got[4] == 0.0, (label, got)
            rel = np.abs(got - want) / np.where(want != 0, np.abs(want), 1.0)
            worst['moments'] = max(worst['moments'], float(rel.max()))
            assert rel.max() <= 1e-14, (label, 'moments', got, want)
        if buffers:
            f = Fr(1, nbt0 + 1) if mom < 0 else Fr(mom)
            unb = [vv * (N / (N - 1 if N > 1 else 1)) for vv in var]
            want_rm = [float((1 - f) * Fr(float(rm0[c])) + f * (mean[c] + Fr(1, 2))) for c in range(3)]
            want_rv = [float((1 - f) * Fr(float(rv0[c])) + f * unb[c]) for c in range(3)]
            u = max(_ulps32(rm.cpu().numpy(), want_rm), _ulps32(rv.cpu().numpy(), want_rv))
            worst['running'] = max(worst['running'], u)
            assert u <= 2, (label, 'running statistics', rm, want_rm, rv, want_rv)
            if mom == 0.0:
                assert np.array_equal(rm.cpu().numpy(), rm0) and np.array_equal(rv.cpu().numpy(), rv0), label
            assert int(nbt) == nbt0 + 1, (label, nbt)
    pc.report('bn/finalize: bn[6] vs the closed form, float32 ulps', worst['bn'], 2.0)
    pc.report('bn/finalize: running statistics vs the closed form, float32 ulps', worst['running'], 2.0)
    pc.report('bn/finalize: moments vs the closed form, relative', worst['moments'], 1e-14)
    # what the call refuses
    T = torch.zeros(7, dtype=torch.float64, device=device)
    bn, rm = torch.zeros(6, device=device), torch.zeros(3, device=device)
    assert lib.r2l_bn_finalize(p(T), 0, p(bn), None, None, None, None, 1e-5, 0.1, stream) == -1
    assert lib.r2l_bn_finalize(p(T), 1, p(bn), None, p(rm), None, None, 1e-5, 0.1, stream) == -1
