"""The backward of a subset of the gradients (ParametrizedProcessing.selective_backward, r2l_isp_step_bwd_select): the checks, on
any device.

tests/test_selective_backward.py runs them on the lock-step emulation under ASan + UBSan (this file as the driver of a
subprocess, like tests/raw_grad_checks.py); tests/test_gpu_selective_backward.py calls them on the gfx950 build.

    python tests/selective_bwd_checks.py <library> [group ...]        groups: launches golden shapes fallback default

Prints one line per check; exit code 0 only if every check passed."""
import os
import sys
import time
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import parity_checks as pc  # noqa: E402
import raw_grad_checks as rc  # noqa: E402
from oracle import isp_oracle as orc  # noqa: E402
from raw2logit_amd import _lib, functional as F_  # noqa: E402
from raw2logit_amd.processing import pipeline_torch as ppt  # noqa: E402

# include/r2l_isp.h: R2L_GRAD_*, R2L_SELECT_*, R2L_STEP_KEEP_LUMA
GRAD = dict(black_level=1, white_balance=2, colour_correction=4, gamma_correct=8, **{'debayer.weight': 16},
            **{'sharpening_filter.weight': 32, 'gaussian_blur.weight': 64}, raw=128)
SELECT_B1, SELECT_BLUR, SELECT_BLUR_HP, SELECT_HP, SELECT_RAW = 1, 2, 4, 8, 16
KEEP_LUMA = 8
# route -> (frames require grad, trainable parameters)
ROUTES = {'raw': (True, ()), 'gamma': (False, ('gamma_correct',)), 'blur': (False, ('gaussian_blur.weight',)),
          'raw_gamma': (True, ('gamma_correct',)), 'blur_gamma': (False, ('gamma_correct', 'gaussian_blur.weight')),
          'raw_blur': (True, ('gaussian_blur.weight',)),
          'raw_blur_gamma': (True, ('gamma_correct', 'gaussian_blur.weight'))}
FOUR = ('raw', 'gamma', 'blur', 'raw_gamma')
# the kernels of a route behind the BatchNorm sums, from the passes r2l_isp_step_bwd_select_passes reports
PASS_KERNEL = {SELECT_BLUR: 'r2l_launch_bwd1_blur_fin', SELECT_BLUR_HP: 'r2l_launch_bwd1_blur_hp_fin',
               SELECT_HP: 'r2l_launch_bwd2_hp', SELECT_RAW: 'r2l_launch_bwd_raw_plane'}
B1_KERNEL = {'raw': 'r2l_launch_bwd1_sel_raw', 'raw_gamma': 'r2l_launch_bwd1_sel_raw_gamma', 'raw_blur': 'r2l_launch_bwd1_sel_raw',
             'raw_blur_gamma': 'r2l_launch_bwd1_sel_raw_gamma',
             'gamma': 'r2l_launch_bwd1_sel_gamma', 'blur': 'r2l_launch_bwd1_sel_gypp', 'blur_gamma': 'r2l_launch_bwd1_sel_gypp_gamma'}
PLANES = dict(R2L_BWD_PLANES=1)     # diagnostic builds: the plane passes below 4 Mi px


def route_mask(route):
    raw, names = ROUTES[route]
    return (GRAD['raw'] if raw else 0) | sum(GRAD[n] for n in names)


def set_trainable(m, names):
    for k, f in pc.NAME2ATTR.items():
        if k != 'additive_layer' or m.additive_layer is not None:
            f(m).requires_grad_(k in names)
    return m


def step(m, raw_np, cot_np, device, raw_grad, epilogue=None):
    """forward + backward; -> (out, grad_raw | None, {name: grad}, {backward kernel: launches}) -- the launch record of the
    backward alone, without BatchNorm's backward sums (every route runs them)"""
    raw = torch.from_numpy(raw_np).to(device)
    if raw_grad:
        raw.requires_grad_(True)
    if epilogue is not None:
        m.__dict__['_epilogue'] = epilogue
    y = m(raw)
    assert isinstance(m.stages, ppt._LazyStages), 'the call took the stage-by-stage kernels'
    cot = torch.from_numpy(cot_np).to(device)
    lib = _lib.library_for(raw)[0]
    _, names = pc.kernels_launched(lib, lambda: y.backward(cot))
    names = {k[:-len('_kernel')]: v for k, v in names.items() if not k.startswith('r2l_launch_bn')}
    grads = {k: f(m).grad.detach().cpu().numpy().copy() for k, f in pc.NAME2ATTR.items()
             if (k != 'additive_layer' or m.additive_layer is not None) and f(m).grad is not None}
    return y.detach().cpu().numpy(), (raw.grad.cpu().numpy() if raw_grad else None), grads, names


def plain_module(bn, training, device, route, selective, fused_raw=True):
    m = rc.make_plain_module(bn, device, training)
    m.fused_raw_grad = fused_raw
    if selective is not None:
        m.selective_backward = selective
    return set_trainable(m, ROUTES[route][1])


def expected_kernels(route, lib, B, H, W, u16=False, epi=0):
    passes = lib.r2l_isp_step_bwd_select_passes(route_mask(route), int(u16), 0, B, H, W, KEEP_LUMA | epi)
    want = {SELECT_B1}
    raw, names = ROUTES[route]
    if 'gaussian_blur.weight' in names:
        want.add(SELECT_BLUR_HP if raw else SELECT_BLUR)
    elif raw:
        want.add(SELECT_HP)
    if raw:
        want.add(SELECT_RAW)
    assert passes == sum(want), (route, passes, want)
    b1 = B1_KERNEL[route] + ('_epi' if epi else '') + ('_u16' if u16 else '')
    return {b1: 1, **{PASS_KERNEL[p]: 1 for p in want if p != SELECT_B1}}


def check_launches(route, bn, training, device, B, H, W):
    """the selective route launches its reduced passes and nothing else; with the attribute off the full backward runs"""
    raw_np = orc.synth_raw(B, H, W, seed=2, kind='scene')
    cot = np.random.default_rng(2).standard_normal((B, 3, H, W)).astype(np.float32)
    lib = _lib.library_for(torch.from_numpy(raw_np).to(device))[0]
    names = step(plain_module(bn, training, device, route, True), raw_np, cot, device, ROUTES[route][0])[3]
    assert names == expected_kernels(route, lib, B, H, W), (route, names)
    assert not any('bwd2_sums' in k for k in names), names
    if route == 'raw':
        assert not any('blur_hp' in k for k in names), names
    if route == 'gamma':
        assert len(names) == 1 and sum(names.values()) == 1, names
    if route == 'blur':
        assert sorted(names) == ['r2l_launch_bwd1_blur_fin', 'r2l_launch_bwd1_sel_gypp'], names
    off = step(plain_module(bn, training, device, route, False), raw_np, cot, device, ROUTES[route][0])[3]
    assert any('bwd2_sums' in k for k in off) and not any('_sel_' in k or '_fin' in k for k in off), off


def compare_route(route, make, raw_np, cot, device, label, oracle=None):
    """the selective route against the full backward of the same build on the same inputs and cotangent (grad_raw bit for bit
    on the RAW-only route; the gamma / blur gradients within the limit this project uses between two of its backward routes),
    parameters that did not ask get no gradient, and -- oracle = (float64 grads, lo, hi, grad_raw triple | None, rtol) -- against
    the float64 oracle with check_param_case's limits"""
    raw_grad, names = ROUTES[route]
    o1, gr1, g1, k1 = step(make(True), raw_np, cot, device, raw_grad)
    o0, gr0, g0, k0 = step(make(False), raw_np, cot, device, raw_grad)
    assert any('_sel_' in k for k in k1), (route, k1)
    assert not any('_sel_' in k for k in k0), (route, k0)
    assert np.array_equal(o0, o1)
    assert sorted(g1) == sorted(names) == sorted(g0), (route, sorted(g1), sorted(g0))
    if raw_grad:   # (the same map; HP from r2l_bwd2_hp or from the fused blur pass is identical arithmetic, DESIGN section 3.2b')
        assert np.array_equal(gr0, gr1), (label, route, 'grad_raw differs from r2l_isp_step_bwd_raw', float(np.abs(gr0 - gr1).max()))
    for k in names:
        ref, got = g0[k], g1[k]
        err, lim = np.abs(got - ref).max(), 2e-4 * (np.abs(ref).max() + 1e-6)
        pc.report(f'selective {route} vs full backward: {k} ({label})', err, lim)
        assert err <= lim, (label, route, k, float(err), float(lim))
    if oracle is not None:
        o_nom, o_lo, o_hi, graw3, rtol = oracle
        for k in names:
            og = np.asarray(o_nom[k])
            flip = max(np.abs(np.asarray(o_lo[k]) - og).max(), np.abs(np.asarray(o_hi[k]) - og).max())
            e, lim = np.abs(g1[k].reshape(og.shape) - og).max(), rtol * (np.abs(og).max() + 1e-6) + flip
            pc.report(f'selective {route} vs float64 oracle: {k} ({label})', e, lim)
            assert e <= lim, (label, route, k, 'vs oracle', float(e), float(lim))
        if raw_grad:
            nom, lo, hi = graw3
            lim = rc._limit(nom, lo, hi, nom, rtol)
            err = np.abs(gr1 - nom)
            pc.report(f'selective {route} vs float64 oracle: grad_raw ({label})', err.max(), float(np.min(lim)))
            assert np.all(err <= lim), (label, route, 'grad_raw vs oracle', float(err.max()))


def _oracle(raw_np, P64, bn, cot, rtol):
    _, _, cache = orc.parametrized_forward(raw_np, P64, bn=bn)
    nom = orc.parametrized_backward(P64, cache, cot)
    lo = orc.parametrized_backward(P64, cache, cot, clip_shift=1e-6)
    hi = orc.parametrized_backward(P64, cache, cot, clip_shift=-1e-6)
    return nom[0], lo[0], hi[0], (nom[1], lo[1], hi[1]), rtol


def check_golden_case(case, device, routes=FOUR):
    B, H, W = case['shape']
    raw_np = orc.synth_raw(B, H, W, seed=case['seed'], kind=case['kind'])
    cot = np.random.default_rng(1000 + case['seed']).standard_normal((B, 3, H, W)).astype(np.float32)
    P = pc.build_params(case)
    oracle = _oracle(raw_np, P.astype(np.float64), pc.oracle_bn(case), cot, case.get('grad_rtol', pc.DEFAULT_GRAD_RTOL))

    def make(route, selective):
        m = pc.make_module(case, P, device)
        m.fused_raw_grad = True
        m.selective_backward = selective
        return set_trainable(m, ROUTES[route][1])
    with pc.env_overrides(device, PLANES):
        for route in routes:
            compare_route(route, lambda s: make(route, s), raw_np, cot, device, case['name'], oracle)


def check_shape(B, H, W, bn, training, device, routes=FOUR, seed=0, with_oracle=True):
    raw_np = orc.synth_raw(B, H, W, seed=seed, kind='scene')
    cot = np.random.default_rng(77 + seed).standard_normal((B, 3, H, W)).astype(np.float32)
    oracle = _oracle(raw_np, orc.IspParams(orc.DRONE_CAMERA_PARAMS, dtype=np.float64), rc.bn_arg(bn, training), cot,
                     pc.DEFAULT_GRAD_RTOL) if with_oracle else None
    for route in routes:
        compare_route(route, lambda s: plain_module(bn, training, device, route, s), raw_np, cot, device,
                      f'{B}x{H}x{W} bn={bn} train={training}', oracle)


def check_u16_and_epilogue(device, B=2, H=12, W=264):
    """the GAMMA and BLUR routes on 16-bit frames and through the output epilogue"""
    rng = np.random.default_rng(3)
    raw16 = (orc.synth_raw(B, H, W, seed=3, kind='scene') * 65535).astype(np.uint16).view(np.int16)
    cot = rng.standard_normal((B, 3, H, W)).astype(np.float32)
    lib = _lib.library_for(torch.from_numpy(cot).to(device))[0]
    for route in ('gamma', 'blur', 'blur_gamma'):
        for u16, epi in ((True, None), (False, (True, True, 0)), (True, (True, False, 0))):
            raw_np = raw16 if u16 else orc.synth_raw(B, H, W, seed=3, kind='scene')
            res = []
            for sel in (True, False):
                m = plain_module(True, True, device, route, sel)
                res.append(step(m, raw_np, cot, device, False, epilogue=epi))
            (o1, _, g1, k1), (o0, _, g0, k0) = res
            assert k1 == expected_kernels(route, lib, B, H, W, u16, F_.epilogue_bits(epi)), (route, u16, epi, k1)
            assert np.array_equal(o0, o1)
            for k in ROUTES[route][1]:
                err, lim = np.abs(g1[k] - g0[k]).max(), 2e-4 * (np.abs(g0[k]).max() + 1e-6)
                pc.report(f'selective {route} vs full backward: {k} (u16={u16} epilogue={epi})', err, lim)
                assert err <= lim, (route, u16, epi, k, float(err), float(lim))


def _same(a, b):
    (o0, r0, g0, k0), (o1, r1, g1, k1) = a, b
    assert k0 == k1, (k0, k1)
    assert np.array_equal(o0, o1) and sorted(g0) == sorted(g1)
    assert (r0 is None) == (r1 is None) and (r0 is None or np.array_equal(r0, r1))
    for k in g0:
        assert np.array_equal(g0[k], g1[k]), k


def check_fallbacks(device, plane_px=False):
    """masks and frames without a reduced route: the attribute on and off give bit-identical gradients and the same launches.
    plane_px: every case but the tile-kernel one runs with the pixel-count test out of the way (R2L_BWD_PLANES in a
    diagnostic build), so that it is the mask, the width or the additive layer that sends the call to the full backward; the
    route query must say so for the same arguments"""
    cases = [('a mask with white_balance', (2, 12, 264), ('white_balance', 'gamma_correct'), False, False),
             ('W % 4 != 0', (2, 12, 262), ('gamma_correct',), False, False),
             ('W > 2048', (1, 4, 2052), ('gamma_correct', 'gaussian_blur.weight'), False, False),
             ('a batch the tile kernels take', (2, 64, 64), ('gaussian_blur.weight',), False, False),
             ('an additive layer', (1, 256, 256), ('gamma_correct',), False, True)]
    for label, (B, H, W), names, raw_grad, additive in cases:
        raw_np = orc.synth_raw(B, H, W, seed=4, kind='scene')
        cot = np.random.default_rng(4).standard_normal((B, 3, H, W)).astype(np.float32)
        res = []
        for sel in (False, True):
            m = rc.make_plain_module(True, 'cpu', True)
            if additive:
                ppt.append_additive_layer(m)
            m = m.to(device)
            m.selective_backward = sel
            set_trainable(m, names)
            planes = plane_px and label != 'a batch the tile kernels take'
            with pc.env_overrides(device, PLANES if planes else {}):
                res.append(step(m, raw_np, cot, device, raw_grad))
                lib = _lib.library_for(torch.from_numpy(cot).to(device))[0]
                assert lib.r2l_isp_step_bwd_select_passes(sum(GRAD[n] for n in names), 0, int(additive), B, H, W,
                                                          KEEP_LUMA) == 0, label
        _same(*res)
        assert not any('_sel_' in k or '_fin' in k for k in res[1][3]), (label, res[1][3])


def check_epilogue_with_raw_grad(device):
    """an epilogue with frames that require grad: neither call produces d/d raw, with the same error (the library refuses
    such a call in the preconditions it shares with r2l_isp_step_bwd_raw, before any routing)"""
    raw_np = orc.synth_raw(2, 12, 264, seed=4, kind='scene')
    msgs = []
    for sel in (False, True):
        m = plain_module(True, True, device, 'raw', sel)
        raw = torch.from_numpy(raw_np).to(device).requires_grad_(True)
        y = F_.isp_fused(raw, m, F_.BN_TRAIN, None, (True, False, 0))
        try:
            y.sum().backward()
            msgs.append(None)
        except _lib.R2LError as e:
            msgs.append(str(e))
    assert msgs[0] is not None and msgs[0] == msgs[1], msgs


def check_default_unchanged(device, B=2, H=12, W=264):
    """the attribute absent (the class without it, as before it existed) against False: the same launches and the same bits;
    and the default is False"""
    assert ppt.ParametrizedProcessing.selective_backward is False
    raw_np = orc.synth_raw(B, H, W, seed=6, kind='scene')
    cot = np.random.default_rng(6).standard_normal((B, 3, H, W)).astype(np.float32)
    for route in ('raw', 'gamma'):
        res = []
        for absent in (True, False):
            m = plain_module(True, True, device, route, None)
            try:
                if absent:
                    del ppt.ParametrizedProcessing.selective_backward
                    assert not hasattr(m, 'selective_backward')
                with pc.env_overrides(device, PLANES):
                    res.append(step(m, raw_np, cot, device, ROUTES[route][0]))
            finally:
                ppt.ParametrizedProcessing.selective_backward = False
        _same(*res)
        assert any('bwd2_sums' in k for k in res[0][3]), res[0][3]


SHAPES_EXTRA = [(2, 4, 260), (1, 70, 260)]      # 4-row frames with a last strip of one lane; a partially filled last strip


def main():
    import emul_hook
    lib_path = sys.argv[1]
    groups = set(sys.argv[2:]) or {'launches', 'golden', 'shapes', 'fallback', 'default'}
    emul_hook.enable(lib_path)
    assert not emul_hook.active().is_device
    torch.set_num_threads(1)
    results = []

    def run(name, fn):
        t0 = time.time()
        try:
            fn()
            results.append(True)
            print(f'PASS {name}  [{time.time() - t0:.1f} s]', flush=True)
        except Exception:   # noqa: BLE001
            results.append(False)
            print(f'FAIL {name}\n{traceback.format_exc()}', flush=True)

    if 'launches' in groups:
        with rc.env(**PLANES):
            for route in ROUTES:
                run(f'launch record {route}', lambda route=route: check_launches(route, True, True, 'cpu', 2, 12, 264))
            run('16-bit frames and the output epilogue', lambda: check_u16_and_epilogue('cpu'))
    if 'golden' in groups:
        for case in rc.FUSED_CASES:
            run(f'golden {case["name"]}', lambda case=case: check_golden_case(case, 'cpu'))
    if 'shapes' in groups:
        with rc.env(**PLANES):
            for i, (H, W) in enumerate(pc.FRAME_SHAPES_PLANES):
                bn, training = rc.BN_MODES[i % 3]
                run(f'shape 2x{H}x{W} bn={bn} train={training}', lambda: check_shape(2, H, W, bn, training, 'cpu'))
            for (B, H, W) in SHAPES_EXTRA:
                for bn, training in rc.BN_MODES:
                    with rc.env(R2L_BP_BAND=6, R2L_HB_BAND=6, R2L_BR_BAND=6, R2L_HP_BAND=6):
                        run(f'shape {B}x{H}x{W} short bands bn={bn} train={training}',
                            lambda: check_shape(B, H, W, bn, training, 'cpu', routes=tuple(ROUTES)))
    if 'fallback' in groups:
        run('fall-backs', lambda: check_fallbacks('cpu', plane_px=True))
    if 'default' in groups:
        run('default unchanged', lambda: check_default_unchanged('cpu'))
    n_ok = sum(results)
    print(f'selective-backward checks passed: {n_ok} / {len(results)}' + ('' if n_ok == len(results) else '  FAILED'), flush=True)
    sys.exit(0 if n_ok == len(results) else 1)


if __name__ == '__main__':
    main()
