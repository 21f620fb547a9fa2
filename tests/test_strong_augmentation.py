"""The strong augmentation set (utils/augmentation.py:77-84) against its torchvision 0.10 restatement
(tests/strong_aug_oracle.py), through the host emulation of the real kernel source (CPU tensors)."""
import numpy as np
import pytest
import torch

import strong_aug_oracle as so
from raw2logit_amd import _lib
from raw2logit_amd import augmentation as A

ANGLES = (0.0, 1e-3, -1e-3, 17.3, 45.0, 90.0, -90.0, -89.99)
SHAPES = ((1, 3, 5, 7), (2, 3, 64, 48), (2, 3, 33, 65), (1, 1, 3, 3))
FLIPS = ((0, 0), (1, 0), (0, 1), (1, 1))


def _frames(shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g) * 1.4 - 0.2     # both clamp bounds of the sharpness are crossed


def _near_tie(angle, H, W, tol=1e-4):
    """output pixels whose oracle source coordinate lies within tol px of a rounding tie or of the frame edge"""
    iy, ix = so.source_coordinates(angle, H, W)
    def near(c, n):
        f = c - torch.floor(c)
        return ((f - 0.5).abs() < tol) | ((c + 0.5).abs() < tol) | ((c - (n - 0.5)).abs() < tol)
    return near(iy, H) | near(ix, W)


def _check_rotation(y, o, angle, H, W):
    bad = (y != o).reshape(-1, H, W).any(0)
    if bad.any():
        tie = _near_tie(angle, H, W)
        assert not (bad & ~tie).any(), (angle, H, W, int(bad.sum()))
        assert bad.sum().item() < 1e-3 * H * W
    return int(bad.sum())


def _check_sharp(y, o, pre):
    err = (y - o).abs()
    flip = (err > 2e-7)
    if flip.any():   # a clamp decided the other way: only right at a bound
        assert ((pre[flip] - 0).abs().minimum((pre[flip] - 1).abs()) < 1e-6).all(), float(err.max())


def _pre_clamp(x, hf, vf, angle, noise=None):
    v = so.apply(x, hf, vf, angle, noise=noise)
    return 0.5 * v + 0.5 * so.blurred_degenerate(v)


@pytest.mark.parametrize('shape', SHAPES)
def test_forward_matches_oracle(emulation, shape):
    x = _frames(shape)
    H, W = shape[-2:]
    g = torch.Generator().manual_seed(1)
    drawn = [float(torch.empty(1).uniform_(-90, 90, generator=g)) for _ in range(4)]
    for angle in ANGLES + tuple(drawn):
        for hf, vf in FLIPS:
            _check_rotation(A.strong_augment(x, hf, vf, angle), so.apply(x, hf, vf, angle), angle, H, W)
            y = A.strong_augment(x, hf, vf, angle, sharpness=0.5)
            o = so.apply(x, hf, vf, angle, sharpness=0.5)
            if H > 2 and W > 2:
                _check_sharp(y, o, _pre_clamp(x, hf, vf, angle))
            else:
                assert torch.equal(y, o)


def test_fill_and_masks(emulation):
    """(B, H, W) float 0/1 masks: one image of B channels; fill outside the rotated frame"""
    m = (torch.rand(4, 33, 65) > 0.5).float()
    for angle in (17.3, -45.0, 89.0):
        for fill in (0.0, 0.25):
            y = A.strong_augment(m, True, False, angle, fill=fill)
            _check_rotation(y, so.apply(m, True, False, angle, fill=fill), angle, 33, 65)
            assert set(torch.unique(y).tolist()) <= {0.0, 1.0, fill}


@pytest.mark.parametrize('shape', ((1, 3, 2, 9), (1, 3, 9, 2), (2, 1, 1, 5)))
def test_sharpness_small_frames_unchanged(emulation, shape):
    x = _frames(shape) * 3
    assert torch.equal(A.adjust_sharpness(x, 0.5), x)        # no clamp either
    assert torch.equal(A.adjust_sharpness(x, 0.5), so.adjust_sharpness(x, 0.5))


def test_noise_is_philox_on_rotated_frame(emulation):
    x = _frames((2, 3, 33, 65))
    key = torch.tensor([123456789012345], dtype=torch.int64)
    for angle, hf in ((None, 1), (30.0, 0), (-71.2, 1)):
        y = A.strong_augment(x, hf, 0, angle, noise_std=0.0005, noise_key=key)
        r = A.strong_augment(x, hf, 0, angle) if angle is not None else A.flip_rot(x, hflip=hf)
        n = A.add_gaussian_noise(r, 0.0005, int(key.item()))
        assert torch.equal(y, n)


def test_gradients_match_oracle(emulation):
    for shape in ((2, 3, 33, 65), (1, 3, 5, 7), (2, 3, 64, 48)):
        x = _frames(shape, 3)
        gy = torch.randn(shape, generator=torch.Generator().manual_seed(4))
        for angle in (None, 0.0, 17.3, -45.0, 90.0):
            for hf, vf in ((0, 0), (1, 1), (1, 0)):
                for sharp in (None, 0.5):
                    if angle is None and sharp is None:
                        continue
                    xk = x.clone().requires_grad_(True)
                    A.strong_augment(xk, hf, vf, angle, sharpness=sharp).backward(gy)
                    xo = x.clone().requires_grad_(True)           # float32: torchvision's sampling grid
                    so.apply(xo, hf, vf, angle, sharpness=sharp).backward(gy)
                    scale = xo.grad.abs().max().item()
                    err = (xk.grad.double() - xo.grad.double()).abs().max().item()
                    assert err <= 1e-6 * scale, (shape, angle, hf, vf, sharp, err / scale)


def test_adjoint_identity(emulation):
    """<R x, g> = <x, R^T g> in float64 for the rotation + flips (R^T = the gathered candidates)"""
    for shape in ((1, 1, 33, 65), (1, 1, 64, 48), (1, 1, 5, 7)):
        x = torch.randn(shape).requires_grad_(True)
        g = torch.randn(shape)
        for angle in (13.0, -45.0, 77.7):
            y = A.strong_augment(x, 1, 0, angle)
            gx, = torch.autograd.grad(y, x, g)
            lhs = (y.double() * g.double()).sum().item()
            rhs = (x.double() * gx.double()).sum().item()
            assert abs(lhs - rhs) <= 1e-6 * float(x.detach().abs().max() * g.abs().sum()), (angle, lhs, rhs)


@pytest.mark.parametrize('H,W', ((33, 65), (5, 7), (3, 3), (64, 48), (1, 6)))
def test_candidate_search_is_exhaustive(emulation, H, W):
    """For 361 angles: a forward over index-valued planes gives src(q) for every output pixel; the backward of small-integer
    cotangents must equal their exact scatter-add over those sources -- every q found once, none twice, none missed."""
    idx = torch.arange(H * W, dtype=torch.float32).reshape(1, 1, H, W)
    gy = torch.randint(1, 8, (1, 1, H, W), generator=torch.Generator().manual_seed(H * W)).float()
    for a in np.linspace(-180.0, 180.0, 361):
        for hf, vf in ((0, 0), (1, 1)):
            src = A.strong_augment(idx, hf, vf, float(a), fill=-1.0).reshape(-1).long()
            ref = torch.zeros(H * W, dtype=torch.float64)
            ok = src >= 0
            ref.index_add_(0, src[ok], gy.reshape(-1)[ok].double())
            x = idx.clone().requires_grad_(True)
            gx, = torch.autograd.grad(A.strong_augment(x, hf, vf, float(a)), x, gy)
            assert torch.equal(gx.reshape(-1).double(), ref), (H, W, a, hf, vf)


def test_draw_sequence_matches_reference(emulation):
    """augmentation_strong's decisions with the noise never applied (on a CPU tensor the reference's randn_like consumes
    the CPU generator, so the draws after it could not be compared) equal the oracle's restatement, seed by seed"""
    aug = A.ComposeState([
        A.RandomHorizontalFlip(p=0.5), A.RandomVerticalFlip(p=0.5), A.RandomApply([A.RandomRotation(90)], p=0.5),
        (A.RandomApply([A.AddGaussianNoise(std=0.0005)], p=0.0), False), (A.RandomAdjustSharpness(0.5, p=0.5), False)])
    x = torch.rand(1, 3, 6, 6)
    seen = set()
    for seed in range(200):
        torch.manual_seed(seed)
        aug(x)
        d = aug.last_draws
        after = torch.rand(1).item()
        torch.manual_seed(seed)
        o = so.draws(p_noise=0.0)
        assert (d['hflip'], d['vflip'], d['angle'], d['sharpness']) == (o['hflip'], o['vflip'], o['angle'], o['sharpness'])
        assert d['noise_key'] is None and o['noise'] is None
        assert torch.rand(1).item() == after          # and the same number of draws
        seen.add((d['hflip'], d['vflip'], d['angle'] is not None, d['sharpness'] is not None))
    assert len(seen) == 16


def test_mask_replay(emulation):
    """retain_state=True on the image, then mask_transform=True: the mask gets the same flips and rotation"""
    aug = A.get_augmentation('strong')
    img = torch.rand(2, 3, 40, 56)
    for seed in range(12):
        A.set_global_seed(seed)
        y = aug(img, retain_state=True)
        d = dict(aug.last_draws)
        mask = (img[:, 0] > 0.5).float()
        ym = aug(mask, mask_transform=True)
        assert aug.seed is None
        dm = aug.last_draws
        assert (dm['hflip'], dm['vflip'], dm['angle']) == (d['hflip'], d['vflip'], d['angle'])
        assert dm['noise_key'] is None and dm['sharpness'] is None
        om = so.apply(mask, d['hflip'], d['vflip'], d['angle'])
        if d['angle'] is not None:
            _check_rotation(ym, om, d['angle'], 40, 56)
        else:
            assert torch.equal(ym, om)
        assert y.shape == img.shape


def test_public_interface(emulation):
    aug = A.get_augmentation('strong')
    assert aug is A.augmentation_strong
    assert [type(t).__name__ for t in aug.transforms] == ['RandomHorizontalFlip', 'RandomVerticalFlip', 'RandomApply',
                                                           'RandomApply', 'RandomAdjustSharpness']
    assert len(aug.mask_transforms) == 3
    assert A.RandomRotation(90).degrees == [-90, 90] and A.RandomRotation((10, 20)).degrees == [10, 20]
    for kw in (dict(expand=True), dict(center=(1, 2)), dict(interpolation='bilinear'), dict(fill=[0.0, 0.0, 0.0])):
        with pytest.raises(_lib.R2LError):
            A.RandomRotation(90, **kw)
    with pytest.raises(ValueError):
        A.RandomRotation(-3)

    class P:
        supports_output_epilogue = True
    assert aug.arm(P()) is False                 # applied after the processor, never fused into its epilogue
    x = torch.rand(1, 3, 8, 8)
    A.set_global_seed(5)
    y = aug(x)
    assert y.shape == x.shape
    # nothing drawn: x itself, no launch
    none = A.ComposeState([A.RandomApply([A.RandomRotation(90)], p=0.0), A.RandomAdjustSharpness(0.5, p=0.0)])
    assert none(x) is x
    # generic composition (not the fused plan) still runs transform by transform
    custom = A.ComposeState([A.RandomRotation(30), A.RandomHorizontalFlip(p=1.0)])
    torch.manual_seed(0)
    angle = A.RandomRotation.get_params([-30, 30])
    torch.manual_seed(0)
    assert torch.equal(custom(x), A.flip_rot(A.rotate(x, angle), hflip=True))


def test_errors(emulation):
    x = torch.rand(1, 4, 8, 8)
    with pytest.raises(_lib.R2LError, match='1 or 3 channels'):
        A.adjust_sharpness(x, 0.5)
    with pytest.raises(ValueError):
        A.adjust_sharpness(torch.rand(1, 3, 8, 8), -1.0)
    with pytest.raises(_lib.R2LError, match='noise_key'):
        A.strong_augment(torch.rand(1, 3, 8, 8), angle=3.0, noise_std=0.1, noise_key=torch.tensor([1], dtype=torch.int32))
    with pytest.raises(TypeError):
        A.rotate(torch.rand(1, 3, 8, 8).double(), 3.0)
    lib = emulation
    y = torch.empty(1, 3, 8, 8)
    f = lambda *a: lib.r2l_augment_strong_fwd(*a)      # noqa: E731
    p = _lib.ptr
    assert f(p(y), p(y), None, 3, 2, 8, 8, 0, 0, 1, 0.1, 0.0, 0.0, 0.1, 0.0, 0.0, None, 0, -1.0, None) == -1   # N % C
    assert b'bad dimensions' in lib.r2l_last_error()
    assert f(None, p(y), None, 3, 3, 8, 8, 0, 0, 1, 0.1, 0.0, 0.0, 0.1, 0.0, 0.0, None, 0, -1.0, None) == -1
    assert f(p(y), p(y), None, 3, 3, 8, 8, 0, 0, 1, float('nan'), 0.0, 0.0, 0.1, 0.0, 0.0, None, 0, -1.0, None) == -1
    assert f(p(y), p(y), None, 3, 3, 8, 8, 0, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, None, 0, float('nan'), None) == -1
    assert lib.r2l_augment_strong_bwd(p(y), p(y), None, None, 3, 3, 8, 8, 0, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.5, None) == -1
    assert b'clamp mask' in lib.r2l_last_error()
