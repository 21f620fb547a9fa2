"""The fused ISP step off its usual parameters, buffers and value range (shared by tests/test_value_domain.py on the serial emulation
and tests/test_gpu_value_domain.py on the gfx950 build), in the style of tests/bn_checks.py.

A  legal state the suite holds fixed: the two colour-space matrices (buffers, part of the 150-float block), gamma_correct far from
   2.2, black levels far from the camera's -- every route of bn_checks.ROUTES plus two backward routes (a bfloat16 and a
   channels-last cotangent: the plane passes and the recomputing BatchNorm sums at small shapes) and one selective backward, each with
   BatchNorm off, train and eval (eval on bn_checks' uneven running statistics).
B  finite frames outside [0, 1]: patches at 16.0 and -0.25, isolated pixels, rows of alternating 0 / 16.0.
C  one non-finite element in the cotangent: nothing is swallowed, and nothing spreads past the chain's reach.
D  one non-finite value in a float32 frame: the same containment for the forward, and what the library does inside the window is
   what INTEGRATION.md, "Values outside the ordinary", states (the sentences asserted here are quoted from there).

Reference: the float64 oracle (oracle/isp_oracle.py; parametrized_forward / _backward take any parameters, the matrices included).
Limits, all the project's own and unchanged: A -- pc.out_tolerance on the output, pc.frame_shapes_grad_limit in its conditioning=True
form on the gradients (frames of >= 256 pixels), raw_grad_checks' limit on d/d raw, fuzz_more.fuzz_staged's limits on the tracked
stages; B -- pc.sigma_limit on the output and tests/fuzz_gpu.py's limit for its ill-conditioned kinds on the gradients, bn_checks'
rtol 1e-5 / atol 1e-6 on the running statistics.

Two CONDITIONS per case of part A, asserted before the library is looked at: the oracle's pre-clip rgb stays inside (0.05, 0.95), and
the oracle at the DEFAULT value of the changed quantity (the reference's matrices, gamma 2.2, the camera's black level) misses the
same limit by >= POWER = 50 x (the POWER lines of the parity table).  The gradients of LOW_POWER carry no such claim in their setting
(the default cannot be told from the setting through their limit); the table names them in NO POWER lines."""
import numpy as np
import torch

import bn_checks as bc
import parity_checks as pc
import raw_grad_checks as rc
from oracle import isp_oracle as orc
from raw2logit_amd.processing import pipeline_torch as ppt

POWER = bc.POWER
REACH = 4       # the chain's reach in pixels: blur 2 + sharpen 1 + demosaic 1
BN_MODES = ('off', 'train', 'eval')

# ---- routes ---------------------------------------------------------------------------------------------------------------------------
# bn_checks.ROUTES, and: io -- the output / cotangent type of a step whose backward runs the plane passes (and, in train mode, the
# recomputing BatchNorm sums) at a small shape; select -- frames requiring grad on the fused kernels with only gamma_correct and
# gaussian_blur.weight trainable under selective_backward (the reduced passes)
ROUTES = dict(bc.ROUTES)
ROUTES['bwd_bf16'] = dict(shape=(2, 8, 260), io='bf16')
ROUTES['bwd_nhwc'] = dict(shape=(2, 16, 16), io='nhwc')
ROUTES['select'] = dict(shape=(2, 16, 16), select=('gamma_correct', 'gaussian_blur.weight'))
# (d/d raw on the fused kernels needs the plane passes, which the serial emulation does not have: there the same mask runs without it)
ROUTES['select_no_raw'] = dict(shape=(2, 16, 16), select=('gamma_correct', 'gaussian_blur.weight'), no_raw=True)
FORWARD_ROUTES = tuple(bc.ROUTES)
DEVICE_ONLY, EMULATION_ONLY = ('select',), ('select_no_raw',)

# ---- part A: the settings -----------------------------------------------------------------------------------------------------------------
BT709 = ((0.2126, 0.7152, 0.0722), (-0.1146, -0.3854, 0.5), (0.5, -0.4542, -0.0458))
BLACK_HI, BLACK_NEG = (0.02, 0.11, 0.05, 0.2), (-0.05, -0.01, -0.08, -0.03)
SETTINGS = {        # name -> (what it changes, the other parameters' perturbation)
    'yuv': (dict(yuv=True), 0.01),
    'gamma_1': (dict(gamma=1.0), 0.01), 'gamma_lo': (dict(gamma=0.6), 0.01), 'gamma_hi': (dict(gamma=4.5), 0.01),
    'black_hi': (dict(black=BLACK_HI), 0.01), 'black_neg': (dict(black=BLACK_NEG), 0.01),
    'all': (dict(yuv=True, gamma=0.6, black=BLACK_HI), 0.05),
}
# gradients whose limit the default value of the changed quantity does not miss by POWER x on some route and mode (the oracle alone
# decides this: power_table() below; the smallest factors it gave are in the comments).  They carry NO POWER claim in their setting,
# on any route: the table names them in a 'NO POWER' line.  They are still compared with the oracle at their limit -- a comparison
# that cannot tell the setting from the default there, but still tells a wrong gradient from a right one.
#   additive_layer: sum over the batch of the cotangent behind BatchNorm; without BatchNorm no parameter acts on it (factor 0)
#   gamma_correct under yuv: 13 x;  d/d raw ('raw', whose limit is 3e-3 of its largest element): yuv 21 x, gamma_1 44 x, gamma_hi 22 x
LOW_POWER = {'yuv': ('additive_layer', 'gamma_correct', 'raw'), 'gamma_1': ('additive_layer', 'raw'), 'gamma_lo': ('additive_layer',),
             'gamma_hi': ('additive_layer', 'raw'), 'black_hi': ('additive_layer',), 'black_neg': ('additive_layer',),
             'all': ('additive_layer',)}


def yuv_matrices():
    """M_RGB_2_YUV = BT.709; M_YUV_2_RGB = its float64 inverse times (I + 0.03 R), R standard normal: M2 M1 != I, so that a kernel
    relying on the two being inverses (or on any default coefficient) is wrong.  Both rounded to float32."""
    M1 = np.array(BT709, dtype=np.float64)
    R = np.random.default_rng(709).standard_normal((3, 3))
    return M1.astype(np.float32), (np.linalg.inv(M1) @ (np.eye(3) + 0.03 * R)).astype(np.float32)


def parameters(setting, seed, additive=False):
    """(P of the setting, P0: the same with the changed quantities at their defaults) on top of IspParams(DRONE).perturb(seed, .)"""
    change, scale = SETTINGS[setting] if setting is not None else ({}, 0.01)
    P = orc.IspParams(orc.DRONE_CAMERA_PARAMS, dtype=np.float32)
    if additive:
        P.additive_layer = np.zeros((1, 3, 256, 256), dtype=np.float32)
    P.perturb(seed, scale)
    D = orc.IspParams(orc.DRONE_CAMERA_PARAMS, dtype=np.float32)
    P0 = P.astype(np.float32)
    if change.get('yuv'):
        P.M_RGB_2_YUV, P.M_YUV_2_RGB = yuv_matrices()
        P0.M_RGB_2_YUV, P0.M_YUV_2_RGB = D.M_RGB_2_YUV.copy(), D.M_YUV_2_RGB.copy()
    if 'gamma' in change:
        P.gamma_correct = np.asarray([change['gamma']], dtype=np.float32)
        P0.gamma_correct = D.gamma_correct.copy()
    if 'black' in change:
        P.black_level = np.asarray(change['black'], dtype=np.float32)
        P0.black_level = D.black_level.copy()
    return P, P0


def midtone_frames(B, H, W, seed, black=None, white_balance=None, bits=12, grey=0.2):
    """pc.midtone_frames for any black level, white balance and bit depth (the defaults give pc.midtone_frames bit for bit): levels of
    `bits` bits whose pre-gamma RGB is a smooth grey scene around `grey`.  -> (frames / (2**bits - 1) as float32, the codes)"""
    rng = np.random.default_rng(seed)
    bl, wb, _ = orc.DRONE_CAMERA_PARAMS
    bl = bl if black is None else [float(v) for v in np.asarray(black).reshape(-1)]
    wb = wb if white_balance is None else [float(v) for v in np.asarray(white_balance).reshape(-1)]
    full = (1 << bits) - 1
    y, x = np.mgrid[0:H, 0:W]
    g = grey + 0.03 * np.sin(x / 9.0 + seed) + 0.02 * np.cos(y / 7.0) + rng.uniform(-0.002, 0.002, (B, H, W))
    gain = np.where(y % 2 == 0, np.where(x % 2 == 0, wb[0], wb[1]), np.where(x % 2 == 0, wb[1], wb[2]))
    blk = np.where(y % 2 == 0, np.where(x % 2 == 0, bl[0], bl[1]), np.where(x % 2 == 0, bl[2], bl[3]))
    codes = np.clip(np.round(full * (blk + g / gain)), 0, full)
    return (codes.astype(np.float32) / np.float32(full)).astype(np.float32), codes.astype(np.uint16)


# ---- the module under test and the oracle's BatchNorm -----------------------------------------------------------------------------------
def make_module(P, bn, device, route, raw_bits=12):
    """ParametrizedProcessing with the parameters AND the two matrices of P; BatchNorm off / train / eval on bn_checks' uneven statistics"""
    m = ppt.ParametrizedProcessing(orc.DRONE_CAMERA_PARAMS, track_stages=route.get('track_stages', False), batch_norm_output=bn != 'off')
    if P.additive_layer is not None:
        ppt.append_additive_layer(m)
    with torch.no_grad():
        for k, v in P.by_name().items():
            pc.NAME2ATTR[k](m).copy_(torch.from_numpy(np.asarray(v)))
        m.M_RGB_2_YUV.copy_(torch.from_numpy(P.M_RGB_2_YUV))
        m.M_YUV_2_RGB.copy_(torch.from_numpy(P.M_YUV_2_RGB))
        if bn == 'eval':
            bc.set_uneven(m.batch_norm)
    if route.get('u16'):
        m.raw_bits = raw_bits
    if route.get('io') == 'bf16':
        m.output_dtype = torch.bfloat16
    elif route.get('io') == 'f16':
        m.output_dtype = torch.float16
    if route.get('io') == 'nhwc' or route.get('nhwc'):
        m.output_memory_format = torch.channels_last
    if 'select' in route or route.get('fused_raw'):
        m.fused_raw_grad = True
    if 'select' in route:
        m.selective_backward = True
        for k, f in pc.NAME2ATTR.items():
            if k != 'additive_layer':
                f(m).requires_grad_(k in route['select'])
    return m.to(device).train(bn != 'eval')


def oracle_bn(bn):
    if bn == 'off':
        return None
    if bn == 'train':
        return dict(training=True, running_mean=np.zeros(3), running_var=np.ones(3))
    return dict(training=False, running_mean=np.array(bc.UNEVEN_MEAN), running_var=np.array(bc.UNEVEN_VAR))


def wants_raw_grad(route):
    return bool(route.get('raw_grad') or route.get('track_stages') or ('select' in route and not route.get('no_raw')) or route.get('fused_raw'))


def frames_tensor(route, raw_np, codes, device):
    if route.get('u16'):
        return torch.from_numpy(codes.astype(np.uint16).view(np.int16).copy()).to(device)
    t = torch.from_numpy(raw_np).to(device)
    return t.requires_grad_(True) if wants_raw_grad(route) else t


def cotangent(route, cot_np, device, like):
    """the cotangent as the route's output type and layout"""
    t = torch.from_numpy(cot_np).to(device).to(like.dtype)
    return t.contiguous(memory_format=torch.channels_last) if like.is_contiguous(memory_format=torch.channels_last) and \
        not like.is_contiguous() else t


def assert_forward_route(names, route, bn, device, label):
    """on the device library: the kernels tests/golden/fwd_routes.txt records for the route (bn_checks.assert_route); BatchNorm off
    launches what eval mode launches"""
    if not bc.on_device(device):
        return
    if 'train' in route:
        bc.assert_route(names, route['train' if bn == 'train' else 'eval'], route, device, label)
    elif route.get('track_stages') or route.get('raw_grad'):
        assert ('r2l_launch_bn_finalize_kernel' in names) == (bn == 'train'), (label, sorted(names))
        assert not any(k.startswith('r2l_launch_fwd_') for k in names), (label, 'the fused kernels served a staged case', sorted(names))
    else:
        suffix = {'bf16': '_bf16_kernel', 'nhwc': '_nhwc_kernel', 'f16': '_f16_kernel'}.get(route.get('io'), '_kernel')
        assert any(k.startswith('r2l_launch_fwd_') and (k.endswith(suffix) if route.get('io') else True) for k in names), \
            (label, sorted(names))


def assert_backward_route(names, route, bn, device, label):
    if not bc.on_device(device):
        return
    if route.get('io'):
        suffix = {'bf16': '_bf16_kernel', 'nhwc': '_nhwc_kernel', 'f16': '_f16_kernel'}[route['io']]
        assert any(k.startswith('r2l_launch_bwd1_plane') and k.endswith(suffix) for k in names), (label, sorted(names))
        assert any(k.startswith('r2l_launch_bnr_') and k.endswith(suffix) for k in names) == (bn == 'train'), (label, sorted(names))
    if 'select' in route:
        assert any('_sel_' in k for k in names) and not any('bwd2_sums' in k for k in names), (label, sorted(names))


# ---- the comparisons ------------------------------------------------------------------------------------------------------------------
def _worst(err, tol):
    i = np.unravel_index(int((err / tol).argmax()), err.shape)
    return float(err[i]), float(tol[i]) if np.ndim(tol) else float(tol)


def compare_output(label, y, o, tol):
    err = np.abs(y.detach().float().cpu().numpy().astype(np.float64) - o)
    tol = np.broadcast_to(np.asarray(tol, dtype=np.float64), err.shape)
    e, t = _worst(err, tol)
    pc.report(f'{label}/out vs float64 oracle', e, t)
    assert np.all(err <= tol), (label, 'out vs oracle', err.max(), e, t)


def power_line(label, what, miss):
    pc.report(f'{label}/POWER: the default misses the {what} limit by this factor (>= {POWER:g}; not an error)', POWER, max(miss, 1e-300))


def oracle_gradients(raw_np, P, bn, cot, track=False):
    """the float64 oracle's gradients, those under a clip band shifted by -/+ 1e-6, and the float32 oracle's; -> dict"""
    P64, P32 = P.astype(np.float64), P.astype(np.float32)
    o, stages, cache = orc.parametrized_forward(raw_np, P64, track_stages=track, bn=oracle_bn(bn))
    g, graw, sg = orc.parametrized_backward(P64, cache, cot, stage_grads=track)
    glo, rlo, _ = orc.parametrized_backward(P64, cache, cot, clip_shift=1e-6)
    ghi, rhi, _ = orc.parametrized_backward(P64, cache, cot, clip_shift=-1e-6)
    _, _, c32 = orc.parametrized_forward(raw_np, P32, track_stages=track, bn=oracle_bn(bn))
    g32, _, _ = orc.parametrized_backward(P32, c32, cot)
    return dict(o=o, stages=stages, cache=cache, c32=c32, g=g, graw=graw, sg=sg, glo=glo, ghi=ghi, rlo=rlo, rhi=rhi, g32=g32)


def grad_limits(ref, cot_size, bn):
    """pc.frame_shapes_grad_limit in its conditioning=True form for every gradient of the oracle run `ref`"""
    return {k: pc.frame_shapes_grad_limit(np.asarray(ref['g'][k]), ref['glo'][k], ref['ghi'][k], cot_size, bn != 'off', ref['g32'][k])
            for k in ref['g']}


def gradient_power(ref, ref0, limits):
    """{name: factor by which the default's gradient misses the limit}"""
    return {k: float(np.abs(np.asarray(ref0['g'][k]).reshape(np.asarray(ref['g'][k]).shape) - np.asarray(ref['g'][k])).max() / limits[k])
            for k in ref['g']}


class Worst:
    """every quantity of one kind is asserted against its own limit; the parity table gets ONE line per case and kind, that of the
    quantity closest to its limit, named in the line (3500 lines otherwise)"""

    def __init__(self, label, kind):
        self.label, self.kind, self.n, self.top = label, kind, 0, None

    def add(self, name, err, lim):
        err, lim = float(err), float(lim)
        self.n += 1
        if self.top is None or err / lim > self.top[1] / self.top[2]:
            self.top = (name, err, lim)
        assert err <= lim, (self.label, self.kind, name, err, lim)

    def report(self):
        if self.top is not None:
            pc.report(f'{self.label}/worst of {self.n} {self.kind} vs float64 oracle: {self.top[0]}', self.top[1], self.top[2])


def compare_grads(worst, got, ref, limits, names):
    for k in names:
        r = np.asarray(ref['g'][k])
        worst.add(k, np.abs(np.asarray(got[k], dtype=np.float64).reshape(r.shape) - r).max(), limits[k])


def compare_stats(label, bn, pre_bn):
    """train mode: running statistics and the counter against a float64 nn.BatchNorm2d fed the oracle's output in front of BatchNorm,
    at bn_checks' bar (rtol 1e-5 / atol 1e-6), one line of the table for the two"""
    ref = torch.nn.BatchNorm2d(3, affine=False).double()
    ref(torch.from_numpy(np.asarray(pre_bn, dtype=np.float64)))
    e = max(bc.stats_excess(getattr(bn, k).detach().cpu().numpy(), getattr(ref, k).numpy()) for k in ('running_mean', 'running_var'))
    pc.report(f'{label}/running statistics vs float64 nn.BatchNorm2d, in units of atol 1e-6 + rtol 1e-5', e, 1.0)
    assert e <= 1.0, (label, bn.running_mean, ref.running_mean, bn.running_var, ref.running_var)
    assert int(bn.num_batches_tracked) == int(ref.num_batches_tracked) == 1, (label, bn.num_batches_tracked)


def raw_limit(ref):
    """raw_grad_checks' limit on d/d raw, element by element"""
    return rc._limit(ref['graw'], ref['rlo'], ref['rhi'], ref['graw'], pc.DEFAULT_GRAD_RTOL)


def module_grads(m, names=None):
    return {k: f(m).grad.detach().cpu().numpy() for k, f in pc.NAME2ATTR.items()
            if (k != 'additive_layer' or m.additive_layer is not None) and f(m).grad is not None and (names is None or k in names)}


def trainable(route, P):
    return tuple(route['select']) if 'select' in route else tuple(P.by_name())


# ---- part A -------------------------------------------------------------------------------------------------------------------------
def setting_cases(device_library):
    """(route, setting, BatchNorm mode, raw_bits): every route with every setting and mode; the 16-bit route at raw_bits 12 and 16"""
    cases = []
    for name, route in ROUTES.items():
        if name in (EMULATION_ONLY if device_library else DEVICE_ONLY):
            continue
        for s in SETTINGS:
            for bn in BN_MODES:
                for bits in ((12, 16) if route.get('u16') else (12,)):
                    cases.append((name, s, bn, bits))
    return cases


# the frames' white balance by setting, as a factor on the camera's.  `all` (yuv + gamma_lo + black_hi, 5 % perturbation) puts the red
# channel of a grey scene at 0.013 .. 0.65 and green at 0.10 .. 0.75: a span of 1 : 57, which no grey LEVEL fits into the band's 1 : 19.
# Its scene is therefore tinted red (the red gain the frames are made with is 0.75 x the camera's): rgb inside [0.065, 0.82] on every
# route.  The band stays (0.05, 0.95).
FRAME_TINT = {'all': (0.75, 1.0, 1.0)}


def case_inputs(route_name, setting, bits=12, seed=0):
    route = ROUTES[route_name]
    B, H, W = route['shape']
    P, P0 = parameters(setting, 31 + seed, route.get('additive', False))
    wb = np.asarray(orc.DRONE_CAMERA_PARAMS[1]) * np.asarray(FRAME_TINT.get(setting, (1.0, 1.0, 1.0)))
    raw_np, codes = midtone_frames(B, H, W, 20 + seed, P.black_level, wb, bits if route.get('u16') else 12)
    cot = np.random.default_rng(40 + seed).standard_normal((B, 3, H, W)).astype(np.float32)
    return route, P, P0, raw_np, codes, cot


def check_setting(route_name, setting, bn, device, bits=12, seed=0):
    """one step under a setting of part A on a route: conditions (band, POWER) first, then launch names, output, running statistics,
    every gradient (frames of >= 256 pixels), d/d raw and the tracked stages where the route has them"""
    route, P, P0, raw_np, codes, cot = case_inputs(route_name, setting, bits, seed)
    B, H, W = route['shape']
    label = f'vd/{route_name}{"_bits16" if bits == 16 else ""}/{setting}/bn_{bn}'
    track = bool(route.get('track_stages'))
    io = route.get('io')
    # ---- the reference and the two conditions, before the library is looked at
    if io:          # the cotangent the kernels read is the 16-bit / channels-last one: its values, widened
        cot = torch.from_numpy(cot).to({'bf16': torch.bfloat16, 'f16': torch.float16}.get(io, torch.float32)).float().numpy()
    ref, ref0 = oracle_gradients(raw_np, P, bn, cot, track), oracle_gradients(raw_np, P0, bn, cot, track)
    rgb = ref['cache']['rgb']
    assert rgb.min() > 0.05 and rgb.max() < 0.95, (label, 'the pre-clip rgb leaves (0.05, 0.95)', rgb.min(), rgb.max())
    tol = pc.out_tolerance(ref['cache'], bn != 'off')
    power = {'output': float((np.abs(ref0['o'] - ref['o']) / tol).max())}
    with_grads = H * W >= 256
    names = trainable(route, P)
    if with_grads:
        limits = grad_limits(ref, cot.size, bn)
        power.update({k: v for k, v in gradient_power(ref, ref0, limits).items() if k in names})
        if wants_raw_grad(route):
            power['raw'] = float((np.abs(ref0['graw'] - ref['graw']) / raw_limit(ref)).max())
        for k in power:     # (one line per setting and gradient: the table keeps the smallest factor over routes and modes)
            if k in LOW_POWER[setting]:
                pc.report(f'vd/{setting}/NO POWER claimed for grad {k}: the default misses its limit by this factor only on some '
                          f'route (required elsewhere: {POWER:g}; compared all the same)', POWER, max(power[k], 1e-300))
    least = min((k for k in power if k not in LOW_POWER[setting]), key=lambda k: power[k])
    power_line(label, f'LEAST sensitive of output and {len(power) - 1} gradients ({least})', power[least])
    assert power[least] >= POWER, (label, 'the setting cannot be seen through the limit of', least, power[least])
    # ---- the library
    m = make_module(P, bn, device, route, bits)
    raw = frames_tensor(route, raw_np, codes, device)
    y, fwd_names = bc.launched(raw, lambda: m(raw))
    assert_forward_route(fwd_names, route, bn, device, label)
    assert y.shape == (B, 3, H, W)
    if io:      # the 16-bit / channels-last output is the float32 planar call's, cast / converted by torch: bit for bit
        m32 = make_module(P, bn, device, dict(route, io=None), bits)
        y32 = m32(frames_tensor(route, raw_np, codes, device)).detach()
        want = y32.to(y.dtype).contiguous(memory_format=torch.channels_last) if io == 'nhwc' else y32.to(y.dtype)
        assert y.dtype == want.dtype and torch.equal(y.detach(), want), (label, 'output')
        assert y.is_contiguous(memory_format=torch.channels_last if io == 'nhwc' else torch.contiguous_format), label
        compare_output(label, y32, ref['o'], tol)
    else:
        assert y.dtype == torch.float32
        compare_output(label, y, ref['o'], tol)
    if bn == 'train':
        compare_stats(label, m.batch_norm, ref['cache']['pre_bn'])
    if track:       # fuzz_more.fuzz_staged's limits on the tracked stages
        worst = Worst(label, 'tracked stages')
        for k, st in m.stages.items():
            worst.add(k, np.abs(st.detach().cpu().numpy() - ref['stages'][k]).max(), 2e-5)
        worst.report()
    if not with_grads:
        return
    _, bwd_names = bc.launched(raw, lambda: y.backward(cotangent(route, cot, device, y)))
    assert_backward_route(bwd_names, route, bn, device, label)
    got = module_grads(m)
    assert sorted(got) == sorted(trainable(route, P)), (label, sorted(got))
    worst = Worst(label, 'gradients')
    compare_grads(worst, got, ref, limits, names)
    if wants_raw_grad(route):
        err, lim = np.abs(raw.grad.cpu().numpy() - ref['graw']), raw_limit(ref)
        assert np.all(err <= lim), (label, 'd/d raw', _worst(err, lim))
        worst.add('d/d raw', *_worst(err, lim))
    if track:
        for k, st in m.stages.items():
            worst.add(f'stage gradient {k}', np.abs(st.grad.cpu().numpy() - ref['sg'][k]).max(), 1e-4 * (np.abs(ref['sg'][k]).max() + 1e-6))
    worst.report()


def power_table(routes=None, settings=None):
    """the oracle alone: per setting, the smallest factor over routes and modes by which the default misses each gradient's limit,
    and the band of the pre-clip rgb -- how LOW_POWER and FRAME_TINT were filled in"""
    table = {}
    for name in routes or ROUTES:
        for s in settings or SETTINGS:
            for bn in BN_MODES:
                route, P, P0, raw_np, codes, cot = case_inputs(name, s, 12, 0)
                if raw_np.shape[1] * raw_np.shape[2] < 256:
                    continue
                ref, ref0 = oracle_gradients(raw_np, P, bn, cot), oracle_gradients(raw_np, P0, bn, cot)
                power = gradient_power(ref, ref0, grad_limits(ref, cot.size, bn))
                power['rgb_min'], power['rgb_max'] = -float(ref['cache']['rgb'].min()), float(ref['cache']['rgb'].max())
                power['out'] = float((np.abs(ref0['o'] - ref['o']) / pc.out_tolerance(ref['cache'], bn != 'off')).max())
                power['raw'] = float((np.abs(ref0['graw'] - ref['graw']) / raw_limit(ref)).max())
                for k, v in power.items():
                    table.setdefault(s, {})[k] = min(table.get(s, {}).get(k, np.inf), v)
    return table


# ---- part B: finite frames outside [0, 1] -----------------------------------------------------------------------------------------------
HIGH, LOW, HIGH_PIXEL, LOW_PIXEL = 16.0, -0.25, 65535.0 / 4095.0, -1.0


def outlier_frames(route, raw_np, codes):
    """midtone frames with, written into every image: a 6x6 patch at 16.0 in the frame's corner, a 6x6 patch at -0.25 across rows
    4-9 (a band boundary at band height 6) and across the strip boundary (columns 254-259) where the frame has one, at its right edge
    elsewhere, and isolated pixels at 65535/4095 and at -1; into the last image also two rows of alternating 0 / 16.0.  On the 16-bit
    route the same as codes 65535 and 0 of a container whose raw_bits says 12.  -> (frames as float32, codes)"""
    B, H, W = raw_np.shape
    u16 = bool(route.get('u16'))
    a = codes.astype(np.float64) if u16 else raw_np.astype(np.float64)
    hi, lo, hip, lop = (65535.0, 0.0, 65535.0, 0.0) if u16 else (HIGH, LOW, HIGH_PIXEL, LOW_PIXEL)
    c0 = 254 if W >= 260 else W - 6
    a[:, 0:6, 0:6] = hi
    a[:, 4:10, c0:c0 + 6] = lo
    a[:, min(7, H - 3), W // 2] = hip
    a[:, 1, W - 2] = lop
    a[-1, H - 2:, 0::2] = 0.0
    a[-1, H - 2:, 1::2] = hi
    if u16:
        codes = a.astype(np.uint16)
        return (codes.astype(np.float32) / np.float32(4095)).astype(np.float32), codes
    return a.astype(np.float32), codes


def ill_conditioned_limits(raw_np, P, bn, cot, ref):
    """tests/fuzz_gpu.py's gradient limit for its ill-conditioned kinds: 5e-2 of the scale + 2 flip + 5 conditioning, the flip being
    the largest effect of shifting the clip band by -/+ 1e-6, 3e-6, 1e-5"""
    P64 = P.astype(np.float64)
    shifted = [orc.parametrized_backward(P64, ref['cache'], cot, clip_shift=sgn * sh) for sh in (1e-6, 3e-6, 1e-5) for sgn in (1.0, -1.0)]
    limits = {}
    for k in ref['g']:
        g = np.asarray(ref['g'][k])
        flip = max(np.abs(np.asarray(s[0][k]) - g).max() for s in shifted)
        cond = np.abs(np.asarray(ref['g32'][k], dtype=np.float64).reshape(g.shape) - g).max()
        limits[k] = 5e-2 * (np.abs(g).max() + 1e-6) + 2 * flip + 5 * cond
    rflip = np.max([np.abs(s[1] - ref['graw']) for s in shifted], axis=0)
    return limits, 5e-2 * (np.abs(ref['graw']).max() + 1e-6) + 2 * rflip


def outlier_cases(device_library):
    return [(name, bn) for name in ROUTES if name not in (EMULATION_ONLY if device_library else DEVICE_ONLY) for bn in BN_MODES]


def check_outliers(route_name, bn, device, seed=3):
    """part B on one route and mode: output at every pixel within pc.sigma_limit, gradients within fuzz_gpu's ill-conditioned limit,
    everything finite, train-mode running statistics at bn_checks' bar (the patches make one channel's batch variance large and
    its mean far from the pivot 0.5 of the streaming statistics)"""
    route, P, _, raw_np, codes, cot = case_inputs(route_name, None, 12, seed)
    raw_np, codes = outlier_frames(route, raw_np, codes)
    B, H, W = route['shape']
    label = f'vd/{route_name}/outliers/bn_{bn}'
    io = route.get('io')
    if io:
        cot = torch.from_numpy(cot).to({'bf16': torch.bfloat16, 'f16': torch.float16}.get(io, torch.float32)).float().numpy()
    ref = oracle_gradients(raw_np, P, bn, cot, bool(route.get('track_stages')))
    rgb = ref['cache']['rgb']
    assert rgb.max() > 1.0 and rgb.min() < 1e-5, (label, 'the frames clip at neither end', rgb.min(), rgb.max())
    tol = pc.sigma_limit(pc.out_tolerance(ref['cache'], bn != 'off'), P, ref['cache'], ref['c32'], bn != 'off')
    m = make_module(P, bn, device, route, 12)
    raw = frames_tensor(route, raw_np, codes, device)
    y, fwd_names = bc.launched(raw, lambda: m(raw))
    assert_forward_route(fwd_names, route, bn, device, label)
    assert torch.isfinite(y).all(), (label, 'a non-finite output')
    if io:
        m32 = make_module(P, bn, device, dict(route, io=None), 12)
        y32 = m32(frames_tensor(route, raw_np, codes, device)).detach()
        want = y32.to(y.dtype).contiguous(memory_format=torch.channels_last) if io == 'nhwc' else y32.to(y.dtype)
        assert torch.equal(y.detach(), want), (label, 'output')
        compare_output(label, y32, ref['o'], tol)
    else:
        compare_output(label, y, ref['o'], tol)
    if bn == 'train':
        compare_stats(label, m.batch_norm, ref['cache']['pre_bn'])
    if H * W < 256:
        return
    limits, rlim = ill_conditioned_limits(raw_np, P, bn, cot, ref)
    _, bwd_names = bc.launched(raw, lambda: y.backward(cotangent(route, cot, device, y)))
    assert_backward_route(bwd_names, route, bn, device, label)
    got = module_grads(m)
    for k, v in got.items():
        assert np.isfinite(v).all(), (label, k, 'a non-finite gradient')
    worst = Worst(label, 'gradients')
    compare_grads(worst, got, ref, limits, trainable(route, P))
    if wants_raw_grad(route):
        gr = raw.grad.cpu().numpy()
        assert np.isfinite(gr).all(), (label, 'a non-finite d/d raw')
        err = np.abs(gr - ref['graw'])
        assert np.all(err <= rlim), (label, 'd/d raw', _worst(err, rlim))
        worst.add('d/d raw', *_worst(err, rlim))
    worst.report()


# ---- part C: one non-finite element in the cotangent --------------------------------------------------------------------------------------
NONFINITE = {'+inf': np.inf, '-inf': -np.inf, 'nan': np.nan}
COT_SHAPE = (2, 8, 260)
COT_POSITIONS = {'interior': (1, 1, 4, 100), 'corner': (1, 0, 0, 0), 'strip': (1, 2, 3, 255)}      # (image, channel, row, column)
COT_TYPES = {'f32': {}, 'f16': dict(io='f16'), 'bf16': dict(io='bf16'), 'nhwc': dict(io='nhwc')}


def _window(shape, y, x, reach=REACH):
    """mask (H, W): within `reach` pixels of (y, x)"""
    H, W = shape
    yy, xx = np.mgrid[0:H, 0:W]
    return (np.abs(yy - y) <= reach) & (np.abs(xx - x) <= reach)


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float32).view(np.int32), np.ascontiguousarray(b, dtype=np.float32).view(np.int32))


def _step(P, bn, device, route, raw_np, cot_np):
    """one forward + backward -> (output, {name: gradient}, d/d raw | None, backward launch names)"""
    m = make_module(P, bn, device, route)
    raw = frames_tensor(route, raw_np, None, device)
    y = m(raw)
    _, names = bc.launched(raw, lambda: y.backward(cotangent(route, cot_np, device, y)))
    return y.detach(), module_grads(m), (raw.grad.cpu().numpy() if raw.grad is not None else None), names


def check_cotangent(value, position, cot_type, bn, device, raw_grad):
    """+Inf, -Inf or NaN in one element of the cotangent of image 1 of 2 on midtone frames (no pixel clipped: torch.clip's `where` and
    the oracle's multiplication agree).  Nothing is swallowed: every gradient entry the float64 oracle reports non-finite is
    non-finite -- all 132 of them, in every mode.  Containment (BatchNorm off and eval, `raw_grad`: frames requiring grad on the fused
    kernels): d/d raw of image 0, and of image 1 farther than 4 pixels from the element, equals the run with that element set to 0 bit
    for bit; inside the window every entry the oracle reports non-finite is non-finite."""
    B, H, W = COT_SHAPE
    route = dict(COT_TYPES[cot_type], shape=COT_SHAPE, fused_raw=bool(raw_grad))
    label = f'vd/cotangent/{value}/{position}/{cot_type}/bn_{bn}'
    P, _ = parameters(None, 33)
    raw_np, _ = midtone_frames(B, H, W, 22)
    cot = np.random.default_rng(42).standard_normal((B, 3, H, W)).astype(np.float32)
    dt = {'f16': torch.float16, 'bf16': torch.bfloat16}.get(cot_type, torch.float32)
    cot = torch.from_numpy(cot).to(dt).float().numpy()
    b, c, py, px = COT_POSITIONS[position]
    bad, zero = cot.copy(), cot.copy()
    bad[b, c, py, px], zero[b, c, py, px] = NONFINITE[value], 0.0
    P64 = P.astype(np.float64)
    _, _, cache = orc.parametrized_forward(raw_np, P64, bn=oracle_bn(bn))
    assert cache['rgb'].min() > 0.05 and cache['rgb'].max() < 0.95
    with np.errstate(all='ignore'):
        g, graw, _ = orc.parametrized_backward(P64, cache, bad.astype(np.float64))
    n_bad = sum(int((~np.isfinite(np.asarray(v))).sum()) for v in g.values())
    assert n_bad == 132, (label, 'the oracle reports only', n_bad, 'of 132 gradients non-finite')       # (a condition of the case)
    y, got, gr, names = _step(P, bn, device, route, raw_np, bad)
    assert_backward_route(names, route, bn, device, label)
    assert torch.isfinite(y).all()
    for k in g:
        swallowed = np.isfinite(np.asarray(got[k]).reshape(np.asarray(g[k]).shape)) & ~np.isfinite(np.asarray(g[k]))
        assert not swallowed.any(), (label, k, 'finite where the oracle is not', int(swallowed.sum()), 'entries')
    if not raw_grad:
        return
    inside = _window((H, W), py, px)
    lost = np.isfinite(gr) & ~np.isfinite(graw)
    assert not lost.any(), (label, 'd/d raw finite where the oracle is not', np.argwhere(lost)[:4].tolist())
    if bn == 'train':
        assert not np.isfinite(gr).any(), (label, 'train-mode BatchNorm: the cotangent sums of the channel are non-finite')
        return
    assert np.isfinite(graw[0]).all() and np.isfinite(graw[1][~inside]).all() and not np.isfinite(graw[1][inside]).any()
    _, _, gr0, _ = _step(P, bn, device, route, raw_np, zero)
    assert _bits_equal(gr[0], gr0[0]), (label, 'd/d raw of image 0 changed', int((gr[0] != gr0[0]).sum()))
    assert _bits_equal(gr[1][~inside], gr0[1][~inside]), \
        (label, 'd/d raw of image 1 changed farther than 4 pixels from the element', np.argwhere((gr[1] != gr0[1]) & ~inside)[:4].tolist())


def check_grad_scaler(device, bn='train'):
    """the shape of a torch.cuda.amp.GradScaler step: float16 output, the cotangent scaled until it overflows to Inf -- torch.isfinite
    over the flattened gradients must be False (that is what makes GradScaler skip the step); the same step under a finite scale
    (2^10, divided out again: exact) meets part A's gradient limit"""
    route = dict(shape=(2, 16, 16), io='f16')
    B, H, W = route['shape']
    label = f'vd/grad_scaler/bn_{bn}'
    P, _ = parameters(None, 35)
    raw_np, _ = midtone_frames(B, H, W, 24)
    cot = np.random.default_rng(44).standard_normal((B, 3, H, W)).astype(np.float32)
    over = torch.from_numpy(cot * np.float32(2.0 ** 17)).to(torch.float16)
    assert torch.isinf(over).any() and not torch.isnan(over).any()
    _, got, _, _ = _step(P, bn, device, route, raw_np, over.float().numpy())
    flat = torch.cat([torch.from_numpy(np.asarray(v)).reshape(-1) for v in got.values()])
    assert flat.numel() == 132 and not torch.isfinite(flat).all(), (label, 'an overflowed cotangent left every gradient finite')
    scale = np.float32(2.0 ** 10)
    fine = torch.from_numpy(cot * scale).to(torch.float16)
    assert torch.isfinite(fine).all()
    cot_eff = (fine.float().numpy() / scale).astype(np.float32)
    _, got, _, names = _step(P, bn, device, route, raw_np, fine.float().numpy())
    assert_backward_route(names, route, bn, device, label)
    ref = oracle_gradients(raw_np, P, bn, cot_eff)
    worst = Worst(label, 'gradients')
    compare_grads(worst, {k: np.asarray(v) / scale for k, v in got.items()}, ref, grad_limits(ref, cot.size, bn), tuple(ref['g']))
    worst.report()


# ---- part D: one non-finite value in a float32 frame ---------------------------------------------------------------------------------------
# What INTEGRATION.md, "Values outside the ordinary", states about non-finite frames, sentence by sentence; tests/test_value_domain.py
# asserts that the section holds these sentences verbatim, check_frame_value asserts what they say
DOC_NONFINITE_FRAME = (
    'A NaN or +Inf raw value yields a finite output at every pixel, in every BatchNorm mode, where the reference yields NaN.',
    'Every output pixel within 4 pixels of a NaN raw value is the clip floor\'s, (1e-5)^(1/gamma), before the additive layer and BatchNorm.',
    'Train-mode BatchNorm then takes finite batch statistics and leaves finite running statistics.',
    'With BatchNorm off or in eval mode no output pixel farther than 4 pixels from the value changes, bit for bit.',
)
DOC_OTHER_ROWS = ('Frames below 0 / above 1', 'Non-finite frames', 'Non-finite cotangents', 'M_RGB_2_YUV / M_YUV_2_RGB')
FRAME_VALUES = ('nan', '+inf')


def frame_positions(shape):
    B, H, W = shape
    pos = {'interior': (B - 1, H // 2, W // 2), 'corner': (B - 1, 0, 0)}
    if W >= 260:
        pos['strip'] = (B - 1, 3, 255)
    return pos


def frame_value_cases():
    return [(name, v, p) for name in FORWARD_ROUTES if not ROUTES[name].get('u16') for v in FRAME_VALUES
            for p in frame_positions(ROUTES[name]['shape'])]


def check_frame_value(route_name, value, position, device):
    """NaN / +Inf in one pixel of the last image's float32 frame, inside the guard-zone arena, in the three BatchNorm modes: the four
    sentences of DOC_NONFINITE_FRAME"""
    route = ROUTES[route_name]
    B, H, W = route['shape']
    P, _ = parameters(None, 37, route.get('additive', False))
    clean, _ = midtone_frames(B, H, W, 26)
    b, py, px = frame_positions(route['shape'])[position]
    bad = clean.copy()
    bad[b, py, px] = NONFINITE[value]
    inside = _window((H, W), py, px)
    floor = np.float32(1e-5) ** (np.float32(1.0) / np.float32(P.gamma_correct[0]))
    for bn in BN_MODES:
        label = f'vd/frame/{route_name}/{value}/{position}/bn_{bn}'
        outs = []
        for frames in (clean, bad):
            with pc.poisoned_arena(device, 64 << 20, label) as arena:
                m = make_module(P, bn, device, route)
                raw = arena.place(frames, 'raw')
                if wants_raw_grad(route):
                    raw.requires_grad_(True)
                y, names = bc.launched(raw, lambda: m(raw))
                assert_forward_route(names, route, bn, device, label)
                outs.append(y.detach().cpu().numpy().copy())
                stats = m.batch_norm.state_dict() if bn != 'off' else {}
        y0, y1 = outs
        assert np.isfinite(y1).all(), (label, DOC_NONFINITE_FRAME[0], int((~np.isfinite(y1)).sum()))
        if bn == 'off' and value == 'nan':
            w = y1[b][:, inside] - (P.additive_layer[0][:, inside] if P.additive_layer is not None else 0.0)
            assert np.allclose(w, floor, rtol=1e-5, atol=1e-7 if P.additive_layer is not None else 0.0), \
                (label, DOC_NONFINITE_FRAME[1], float(floor), w.min(), w.max())
        if bn == 'train':
            assert all(bool(torch.isfinite(v.float()).all()) for v in stats.values()), (label, DOC_NONFINITE_FRAME[2], stats)
        else:
            for i in range(B):
                keep = np.ones((H, W), bool) if i != b else ~inside
                assert _bits_equal(y0[i][:, keep], y1[i][:, keep]), \
                    (label, DOC_NONFINITE_FRAME[3], 'image', i, int((y0[i] != y1[i])[:, keep].sum()), 'pixels differ')
