"""The common-corruption set (utils/hendrycks_robustness.py: Distortions) through the host emulation of the real kernel source
(CPU tensors): the oracle against the reference's goldens, the kernels against both, the random transforms' identities and
distributions, launch-shape independence, errors.  The checks live in tests/corruption_checks.py (the GPU suite runs them too)."""
import numpy as np
import pytest

import corruption_checks as cc
import corruption_oracle as co
import parity_checks as pc

SHAPES = ((1, 3, 8, 8), (2, 3, 34, 34), (5, 3, 66, 66), (1, 3, 130, 130))      # below a tile, W % 4 != 0, several tiles / blocks
NON_SQUARE = ((2, 3, 24, 40), (1, 3, 66, 130))


def test_oracle_matches_the_reference_goldens():
    """the own float64 restatement against the reference's methods evaluated in float64 (stored as float32: the only slack)"""
    n = 0
    for t, sev, H, x, r32, r64 in cc.golden_cases():
        err = np.abs(co.apply(x, t, sev) - r64.astype(np.float64)).max()
        pc.report(f'corruption oracle {t} s{sev} {H}x{H} vs the reference in float64', err, 1e-6)
        assert err <= 1e-6, (t, sev, H, err)
        assert np.abs(r32.astype(np.float64) - r64).max() <= 1e-6                 # the stored pair itself
        n += 1
    assert n == 5 * (5 + 5 + 1)
    x = cc.golden()['x_18']
    assert (x == 0).any() and (x == 1).any() and (x[0] == x[1])[x[1] == x[2]].any()   # exact 0, exact 1, grey pixels
    assert np.array_equal(co.identity(x), x)
    batch = np.stack([x, x[:, ::-1].copy()])                                      # every image on its own
    for t in cc.DETERMINISTIC:
        assert np.array_equal(co.apply(batch, t, 4)[1], co.apply(batch[1], t, 4)), t


def test_kernels_match_the_reference_goldens(emulation):
    cc.check_goldens('cpu')


@pytest.mark.parametrize('transform', cc.DETERMINISTIC)
def test_kernels_match_the_oracle(emulation, transform):
    cc.check_oracle_parity('cpu', transform, SHAPES + NON_SQUARE)


def test_identity(emulation):
    cc.check_identity('cpu')


def test_host_tables():
    """the factor list is np.arange's (7, 12, 16, 21, 26 entries), out_size rounds half to even, radii 2, 2, 3, 3, 4"""
    from raw2logit_amd import corruptions as C
    assert [len(C.zoom_factors(s)) for s in range(1, 6)] == [7, 12, 16, 21, 26]
    assert [len(C.gaussian_taps(s)) - 1 for s in C.SEVERITY['gaussian_blur']] == [2, 2, 3, 3, 4]
    for s in C.SEVERITY['gaussian_blur']:
        w = C.gaussian_taps(s)
        assert abs(w[0] + 2 * sum(w[1:]) - 1) < 1e-15
    t = np.array(C.zoom_table(5, 50)).reshape(-1, 5)
    assert (t[:, 0] == np.ceil(50 / C.zoom_factors(5))).all() and (t[:, 2] >= 50).all()
    assert t[0].tolist() == [50, 0, 50, 0, 1.0]
    assert all(r[2] == round(r[0] * z) and r[3] == (r[2] - 50) // 2 for r, z in zip(t, C.zoom_factors(5)))


def test_noise_identities(emulation):
    for shape in ((2, 3, 34, 34), (1, 3, 24, 40)):
        cc.check_noise_identities('cpu', shape)


def test_launch_shape_independence(emulation):
    for shape in ((2, 3, 34, 34), (3, 3, 66, 130)):
        cc.check_launch_shape_independence('cpu', shape)


def test_impulse_noise_distribution(emulation):
    cc.check_impulse_distribution('cpu')


def test_shot_noise_distribution(emulation):
    cc.check_shot_distribution('cpu')


def test_poisson_sampler_at_the_ends_of_its_uniforms(emulation):
    cc.check_poisson_sampler_at_the_ends_of_its_uniforms(emulation)


def test_dtypes(emulation):
    cc.check_dtypes('cpu')


def test_errors(emulation):
    cc.check_errors('cpu')
