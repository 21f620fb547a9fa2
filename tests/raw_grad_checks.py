"""d/d raw on the fused kernels (ParametrizedProcessing.fused_raw_grad, r2l_isp_step_bwd_raw): the checks, on any device.

tests/test_fused_raw_grad.py runs them on the lock-step emulation under ASan + UBSan (this file as the driver of a subprocess,
like tests/lockstep_checks.py); tests/test_gpu_fused_raw_grad.py calls them on the gfx950 build.

    python tests/raw_grad_checks.py <library> [group ...]        groups: golden oracle identity bitwise

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
from oracle import isp_oracle as orc  # noqa: E402
from oracle.golden_cases import PARAM_CASES  # noqa: E402
from raw2logit_amd.processing import pipeline_torch as ppt  # noqa: E402

# every golden case the fused d/d raw serves: no stage tracking, no additive layer, W % 4 == 0
FUSED_CASES = [c for c in PARAM_CASES if not c['track'] and not c['additive'] and c['shape'][2] % 4 == 0]
BAND_KNOBS = ('R2L_BP_BAND', 'R2L_HB_BAND', 'R2L_B2S_BAND', 'R2L_BR_BAND')


class env:
    """os.environ entries for the duration of a block (the band knobs of builds with R2L_TEST_HOOKS)"""

    def __init__(self, **kw):
        self.kw = {k: str(v) for k, v in kw.items()}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        os.environ.update(self.kw)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def fused_step(m, raw_np, cot_np, device, raw_grad=True):
    """one forward + backward of module m; returns (out, grad_raw | None, {parameter name: grad}) as numpy, and asserts that
    the fused kernels served the call"""
    raw = torch.from_numpy(raw_np).to(device)
    if raw_grad:
        raw.requires_grad_(True)
    y = m(raw)
    assert isinstance(m.stages, ppt._LazyStages), 'the call took the stage-by-stage kernels'
    (y * torch.from_numpy(cot_np).to(device)).sum().backward()
    grads = {k: f(m).grad.detach().cpu().numpy().copy() for k, f in pc.NAME2ATTR.items()
             if k != 'additive_layer' and f(m).grad is not None}
    return y.detach().cpu().numpy(), (raw.grad.cpu().numpy() if raw_grad else None), grads


def _limit(ref, lo, hi, nom, rtol):
    fl = np.maximum(np.abs(lo - nom), np.abs(hi - nom))
    return 2 * rtol * (np.abs(ref).max() + 1e-6) + 2 * fl


def check_golden_case(case, golden, device):
    """fused grad_raw (and the parameter gradients of the same call) against the reference's golden vectors, with the limit
    check_staged_case applies to the staged path's d/d raw"""
    g = golden['param_cases']
    pre = case['name'] + '/'
    rtol = case.get('grad_rtol', pc.DEFAULT_GRAD_RTOL)
    B, H, W = case['shape']
    raw_np = orc.synth_raw(B, H, W, seed=case['seed'], kind=case['kind'])
    cot = np.random.default_rng(1000 + case['seed']).standard_normal((B, 3, H, W)).astype(np.float32)
    P = pc.build_params(case)
    m = pc.make_module(case, P, device)
    m.fused_raw_grad = True
    out, gr, grads = fused_step(m, raw_np, cot, device)
    P64 = P.astype(np.float64)
    _, _, cache = orc.parametrized_forward(raw_np, P64, bn=pc.oracle_bn(case))
    o_nom, gr_nom = orc.parametrized_backward(P64, cache, cot)[:2]
    o_lo, gr_lo = orc.parametrized_backward(P64, cache, cot, clip_shift=1e-6)[:2]
    o_hi, gr_hi = orc.parametrized_backward(P64, cache, cot, clip_shift=-1e-6)[:2]
    ref = g[pre + 'grad_raw']
    lim = _limit(ref, gr_lo, gr_hi, gr_nom, rtol)
    err = np.abs(gr - ref)
    pc.ERROR_LOG.append((f'fused d/d raw golden {case["name"]}', float(err.max()), float(np.min(lim))))
    assert np.all(err <= lim), ('grad_raw', case['name'], float(err.max()), float(np.min(lim)))
    for k in o_nom:
        if k == 'additive_layer':
            continue
        r = g[pre + 'grad/' + k]
        got = grads[k].reshape(np.asarray(r).shape)
        e = np.abs(got - r).max()
        fl = max(np.abs(np.asarray(o_lo[k]) - o_nom[k]).max(), np.abs(np.asarray(o_hi[k]) - o_nom[k]).max())
        assert e <= 2 * rtol * (np.abs(r).max() + 1e-6) + 2 * fl, ('param grad', case['name'], k, e)
    return float(err.max())


def make_plain_module(bn, device, training=True, frozen=False):
    """drone camera, BatchNorm None / train / eval (eval: the running statistics of parity_checks.make_module)"""
    m = ppt.ParametrizedProcessing(camera_parameters=orc.DRONE_CAMERA_PARAMS, batch_norm_output=bn)
    if bn and not training:
        with torch.no_grad():
            m.batch_norm.running_mean.copy_(torch.tensor([0.4, 0.45, 0.35]))
            m.batch_norm.running_var.copy_(torch.tensor([0.03, 0.05, 0.04]))
    m.train(training)
    if frozen:
        for p in m.parameters():
            p.requires_grad_(False)
    m.fused_raw_grad = True
    return m.to(device)


def bn_arg(bn, training):
    return None if not bn else (dict(training=True, running_mean=np.zeros(3), running_var=np.ones(3)) if training else
                                dict(training=False, running_mean=np.array([0.4, 0.45, 0.35]),
                                     running_var=np.array([0.03, 0.05, 0.04])))


def check_oracle_shape(B, H, W, bn, training, device, seed=0, rtol=pc.DEFAULT_GRAD_RTOL):
    """fused grad_raw against the float64 oracle on one frame shape (borders, partial strips, band edges); returns the
    grad_raw and the module's black-level gradient for the identity check"""
    raw_np = orc.synth_raw(B, H, W, seed=seed, kind='scene')
    cot = np.random.default_rng(77 + seed).standard_normal((B, 3, H, W)).astype(np.float32)
    m = make_plain_module(bn, device, training)
    out, gr, grads = fused_step(m, raw_np, cot, device)
    P64 = orc.IspParams(orc.DRONE_CAMERA_PARAMS, dtype=np.float64)
    _, _, cache = orc.parametrized_forward(raw_np, P64, bn=bn_arg(bn, training))
    gr_nom = orc.parametrized_backward(P64, cache, cot)[1]
    gr_lo = orc.parametrized_backward(P64, cache, cot, clip_shift=1e-6)[1]
    gr_hi = orc.parametrized_backward(P64, cache, cot, clip_shift=-1e-6)[1]
    lim = _limit(gr_nom, gr_lo, gr_hi, gr_nom, rtol)
    err = np.abs(gr - gr_nom)
    pc.ERROR_LOG.append((f'fused d/d raw oracle {B}x{H}x{W} bn={bn} train={training}', float(err.max()), float(np.min(lim))))
    assert np.all(err <= lim), ('grad_raw vs oracle', (B, H, W), bn, training, float(err.max()), float(np.min(lim)),
                                np.unravel_index(int(np.argmax(err - lim)), err.shape))
    return gr, grads['black_level']


def check_black_level_identity(gr, gbl):
    """sum of grad_raw over the pixels of Bayer site c = -d/d black_level[c] (V = raw - bl[site]); float64 sums on the host"""
    gr = np.asarray(gr, np.float64)
    gbl = np.asarray(gbl, np.float64).reshape(-1)
    for c in range(4):
        sel = gr[:, c >> 1::2, c & 1::2]
        s, a = sel.sum(), np.abs(sel).sum()
        assert abs(s + gbl[c]) <= 1e-5 * a, ('black-level identity', c, s, -gbl[c], a)


def check_bit_identity(B, H, W, bn, training, device):
    """output and every parameter gradient are bit-identical with and without d/d raw (same backward route: the caller
    makes the plane passes run -- frames >= 4 Mi px, or R2L_BWD_PLANES=1 in a hooks build)"""
    raw_np = orc.synth_raw(B, H, W, seed=5, kind='scene')
    cot = np.random.default_rng(5).standard_normal((B, 3, H, W)).astype(np.float32)
    res = []
    for with_raw in (False, True):
        m = make_plain_module(bn, device, training)
        res.append(fused_step(m, raw_np, cot, device, raw_grad=with_raw))
    (o0, _, g0), (o1, gr, g1) = res
    assert np.array_equal(o0, o1), 'output differs with d/d raw requested'
    assert sorted(g0) == sorted(g1) and len(g0) == 7
    for k in g0:
        assert np.array_equal(g0[k], g1[k]), ('parameter gradient differs with d/d raw requested', k)
    assert np.isfinite(gr).all()


ORACLE_SHAPES = [  # (B, H, W, bands): 4-row frames (every row a border row), partial strips, several strips, short bands
    (2, 4, 4, None), (1, 6, 8, None), (1, 70, 260, 6), (1, 6, 516, None), (1, 70, 8, 12), (2, 4, 260, None)]
BN_MODES = [(False, True), (True, True), (True, False)]   # (batch_norm_output, training): none, train, eval


def main():
    import emul_hook
    lib_path = sys.argv[1]
    groups = set(sys.argv[2:]) or {'golden', 'oracle', 'identity', 'bitwise'}
    emul_hook.enable(lib_path)
    assert not emul_hook.active().is_device
    golden = {'param_cases': np.load(os.path.join(HERE, 'golden', 'param_cases.npz'), allow_pickle=False)}
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

    if 'golden' in groups:
        for case in FUSED_CASES:
            run(f'golden {case["name"]}', lambda case=case: check_golden_case(case, golden, 'cpu'))
    if 'oracle' in groups:
        for (B, H, W, band) in ORACLE_SHAPES:
            for bn, training in BN_MODES:
                knobs = {k: band for k in BAND_KNOBS} if band else {}
                with env(**knobs):
                    run(f'oracle {B}x{H}x{W} bands={band} bn={bn} train={training}',
                        lambda: check_oracle_shape(B, H, W, bn, training, 'cpu'))
    if 'identity' in groups:
        def ident():
            for (B, H, W) in ((2, 4, 8), (1, 70, 260)):
                for bn, training in BN_MODES:
                    gr, gbl = check_oracle_shape(B, H, W, bn, training, 'cpu', seed=3)
                    check_black_level_identity(gr, gbl)
        run('black-level identity', ident)
    if 'bitwise' in groups:
        with env(R2L_BWD_PLANES=1):
            for bn, training in BN_MODES:
                run(f'bit identity 2x12x260 bn={bn} train={training}',
                    lambda: check_bit_identity(2, 12, 260, bn, training, 'cpu'))
    n_ok = sum(results)
    print(f'raw-grad checks passed: {n_ok} / {len(results)}' + ('' if n_ok == len(results) else '  FAILED'), flush=True)
    sys.exit(0 if n_ok == len(results) else 1)


if __name__ == '__main__':
    main()
