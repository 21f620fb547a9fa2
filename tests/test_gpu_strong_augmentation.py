"""The strong augmentation set on the MI355X: parity with tests/strong_aug_oracle.py at training shapes, the draw sequence
with the batch on the GPU (noise included), determinism, and processor gradients through the set end to end."""
import pytest
import torch

import parity_checks as pc
import strong_aug_oracle as so
from raw2logit_amd import augmentation as A

pytestmark = pytest.mark.gpu

from test_strong_augmentation import _check_rotation, _check_sharp, _pre_clamp   # noqa: E402


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from raw2logit_amd import _lib
    assert _lib.device_library().is_device
    return 'cuda:0'


def _always(noise=True):
    """augmentation_strong with every draw applied (p = 1)"""
    return A.ComposeState([
        A.RandomHorizontalFlip(p=1.0), A.RandomVerticalFlip(p=1.0), A.RandomApply([A.RandomRotation(90)], p=1.0),
        (A.RandomApply([A.AddGaussianNoise(std=0.0005)], p=1.0 if noise else 0.0), False),
        (A.RandomAdjustSharpness(0.5, p=1.0), False)])


@pytest.mark.parametrize('shape', ((64, 3, 256, 256), (8, 3, 512, 384)))
def test_parity_at_training_shapes(dev, shape):
    g = torch.Generator().manual_seed(7)
    x = torch.rand(shape, generator=g) * 1.4 - 0.2
    gy = torch.randn(shape, generator=g)
    H, W = shape[-2:]
    for angle, hf, vf in ((31.7, 1, 0), (-90.0, 0, 1), (-12.25, 1, 1)):
        xd = x.to(dev).requires_grad_(True)
        y = A.strong_augment(xd, hf, vf, angle)
        _check_rotation(y.detach().cpu(), so.apply(x, hf, vf, angle), angle, H, W)
        ys = A.strong_augment(xd, hf, vf, angle, sharpness=0.5)
        _check_sharp(ys.detach().cpu(), so.apply(x, hf, vf, angle, sharpness=0.5), _pre_clamp(x, hf, vf, angle))
        gx, = torch.autograd.grad(ys, xd, gy.to(dev))
        xo = x.clone().requires_grad_(True)
        go, = torch.autograd.grad(so.apply(xo, hf, vf, angle, sharpness=0.5), xo, gy)
        assert (gx.cpu().double() - go.double()).abs().max().item() <= 1e-6 * go.abs().max().item()


def test_noise_is_philox_on_rotated_frame(dev):
    x = torch.rand(4, 3, 96, 130, device=dev)
    key = torch.tensor([987654321987], dtype=torch.int64, device=dev)
    y = A.strong_augment(x, 1, 0, 23.0, noise_std=0.0005, noise_key=key)
    assert torch.equal(y, A.add_gaussian_noise(A.strong_augment(x, 1, 0, 23.0), 0.0005, int(key.item())))


def test_draw_sequence_on_gpu(dev):
    """with x on the GPU the reference's randn_like draws from the device generator, so the whole CPU sequence -- the
    sharpness decision after the noise included -- must match"""
    aug = A.get_augmentation('strong')
    x = torch.rand(1, 3, 16, 16, device=dev)
    seen = set()
    for seed in range(200):
        torch.manual_seed(seed)
        aug(x)
        d = aug.last_draws
        after = torch.rand(1).item()
        torch.manual_seed(seed)
        o = so.draws(noise_like=x)
        assert (d['hflip'], d['vflip'], d['angle'], d['sharpness']) == (o['hflip'], o['vflip'], o['angle'], o['sharpness'])
        assert (d['noise_key'] is None) == (o['noise'] is None)
        assert torch.rand(1).item() == after
        seen.add((d['noise_key'] is None, d['sharpness'] is None, d['angle'] is None))
    assert len(seen) == 8


def test_deterministic_across_runs_and_grids(dev):
    aug = _always()
    x = torch.rand(16, 3, 160, 224, device=dev)
    gy = torch.randn(16, 3, 160, 224, device=dev)

    def run():
        torch.manual_seed(11)
        xr = x.clone().requires_grad_(True)
        y = aug(xr)
        y.backward(gy)
        return y.detach().clone(), xr.grad.clone()
    y0, g0 = run()
    y1, g1 = run()
    assert torch.equal(y0, y1) and torch.equal(g0, g1)
    for grid in ('1', '37'):
        with pc.env_overrides(dev, {'R2L_GRID_AUGS': grid}):
            y2, g2 = run()
        assert torch.equal(y0, y2) and torch.equal(g0, g2), grid


def test_end_to_end_processor_gradients(dev):
    """ParametrizedProcessing (train-mode BatchNorm) -> augmentation_strong -> loss, against the same chain with the
    oracle's augmentation (fed the kernel's own noise values): processor gradients within DEFAULT_GRAD_RTOL"""
    from oracle import isp_oracle as orc
    from raw2logit_amd.processing.pipeline_torch import ParametrizedProcessing
    raw = torch.from_numpy(orc.synth_raw(4, 128, 160, seed=5, kind='scene')).to(dev)
    cot = torch.randn(4, 3, 128, 160, generator=torch.Generator().manual_seed(2))
    for noise in (True, False):
        aug = _always(noise)
        m1 = ParametrizedProcessing(orc.DRONE_CAMERA_PARAMS, batch_norm_output=True).to(dev).train()
        m2 = ParametrizedProcessing(orc.DRONE_CAMERA_PARAMS, batch_norm_output=True).to(dev).train()
        m2.load_state_dict(m1.state_dict())
        torch.manual_seed(3)
        out = aug(m1(raw))
        d = aug.last_draws
        (out * cot.to(dev)).sum().backward()

        y = m2(raw)
        n = None
        if d['noise_key'] is not None:
            yd = y.detach()
            geo = dict(hflip=d['hflip'], vflip=d['vflip'], angle=d['angle'])
            n = (A.strong_augment(yd, noise_std=d['noise_std'], noise_key=d['noise_key'], **geo) -
                 A.strong_augment(yd, **geo)).cpu()
        yo = so.apply(y.cpu(), d['hflip'], d['vflip'], d['angle'], noise=n, sharpness=d['sharpness'])
        (yo * cot).sum().backward()
        for (k, p1), (_, p2) in zip(m1.named_parameters(), m2.named_parameters()):
            ref = p2.grad.double()
            err = (p1.grad.double() - ref).abs().max().item()
            assert err <= pc.DEFAULT_GRAD_RTOL * (ref.abs().max().item() + 1e-12), (k, noise, err)


def test_segmentation_pair_same_geometry(dev):
    aug = A.get_augmentation('strong')
    img = torch.rand(4, 3, 96, 128, device=dev)
    mask = (img[:, 0] > 0.5).float()
    for seed in range(8):
        A.set_global_seed(seed)
        aug(img, retain_state=True)
        d = aug.last_draws
        ym = aug(mask, mask_transform=True)
        geo = A.strong_augment(img, d['hflip'], d['vflip'], d['angle'])
        assert torch.equal(ym, (geo[:, 0] > 0.5).float())
