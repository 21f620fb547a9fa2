"""Oracle of the strong augmentation set (utils/augmentation.py:77-84) in torch ops, with autograd.

A restatement of the torchvision 0.10 code the reference runs (requirements.txt: torchvision 0.10.0, torch 1.9), which is
not installed here: RandomHorizontalFlip / RandomVerticalFlip, RandomApply, RandomRotation (F.rotate -> _get_inverse_affine_
matrix, _gen_affine_grid, _apply_grid_transform with NEAREST and a fill), RandomAdjustSharpness (F.adjust_sharpness ->
_blurred_degenerate_image, _blend) and the reference's AddGaussianNoise.  Like the Malvar2004 oracle it restates third-party
code from its published source and is not pinned to a golden file of that code's own output."""
import math

import torch
import torch.nn.functional as F


def rotation_matrix(angle):
    """_get_inverse_affine_matrix([0, 0], -angle, [0, 0], 1.0, [0, 0]) in Python doubles (shear 0, scale 1)"""
    rot = math.radians(-angle)
    sx = sy = 0.0
    a = math.cos(rot - sy) / math.cos(sy)
    b = -math.cos(rot - sy) * math.tan(sx) / math.cos(sy) - math.sin(rot)
    c = math.sin(rot - sy) / math.cos(sy)
    d = -math.sin(rot - sy) * math.tan(sx) / math.cos(sy) + math.cos(rot)
    m = [d, -b, 0.0, -c, a, 0.0]
    m[2] += m[0] * (-0.0 - 0.0) + m[1] * (-0.0 - 0.0)
    m[5] += m[3] * (-0.0 - 0.0) + m[4] * (-0.0 - 0.0)
    return m


def affine_grid(angle, H, W):
    """_gen_affine_grid(theta, w=W, h=H, ow=W, oh=H): (1, H, W, 2) float32"""
    theta = torch.tensor(rotation_matrix(angle), dtype=torch.float32).reshape(1, 2, 3)
    base = torch.empty(1, H, W, 3, dtype=torch.float32)
    base[..., 0].copy_(torch.linspace(-W * 0.5 + 0.5, W * 0.5 + 0.5 - 1, steps=W))
    base[..., 1].copy_(torch.linspace(-H * 0.5 + 0.5, H * 0.5 + 0.5 - 1, steps=H).unsqueeze_(-1))
    base[..., 2].fill_(1)
    rescaled = theta.transpose(1, 2) / torch.tensor([0.5 * W, 0.5 * H], dtype=torch.float32)
    return base.view(1, H * W, 3).bmm(rescaled).view(1, H, W, 2)


def rotate(img, angle, fill=0.0):
    """F.rotate(img, angle, NEAREST, expand=False, center=None, fill=[fill] * C) on a float32 tensor of >= 2 dims"""
    shape = img.shape
    x = img.reshape((1,) * (4 - img.dim()) + tuple(shape)) if img.dim() < 4 else img.reshape(-1, *shape[-3:])
    H, W = shape[-2:]
    grid = affine_grid(angle, H, W).expand(x.shape[0], H, W, 2)
    dummy = torch.ones((x.shape[0], 1, H, W), dtype=x.dtype)
    out = F.grid_sample(torch.cat((x, dummy), dim=1), grid, mode='nearest', padding_mode='zeros', align_corners=False)
    mask = out[:, -1:].expand_as(out[:, :-1]) < 0.5
    out = out[:, :-1].clone()
    out = torch.where(mask, torch.full_like(out, float(fill)), out)
    return out.reshape(shape)


def source_coordinates(angle, H, W):
    """the unrounded source position ((gx + 1) W - 1) / 2 of every output pixel (float64 of the float32 grid): (iy, ix)"""
    g = affine_grid(angle, H, W)[0].double()
    return ((g[..., 1] + 1) * H - 1) / 2, ((g[..., 0] + 1) * W - 1) / 2


def blurred_degenerate(img):
    """_blurred_degenerate_image"""
    kernel = torch.ones((3, 3), dtype=img.dtype)
    kernel[1, 1] = 5.0
    kernel /= kernel.sum()
    C = img.shape[-3]
    x = img.reshape(-1, C, *img.shape[-2:])
    tmp = F.conv2d(x, kernel.expand(C, 1, 3, 3), groups=C)
    result = x.clone()
    result[..., 1:-1, 1:-1] = tmp
    return result.reshape(img.shape)


def adjust_sharpness(img, factor):
    """F.adjust_sharpness for float tensors"""
    img3 = img.unsqueeze(0) if img.dim() < 3 else img
    if img3.shape[-3] not in (1, 3):
        raise TypeError('Input image tensor permitted channel values are [1, 3]')
    if img.shape[-1] <= 2 or img.shape[-2] <= 2:
        return img
    deg = blurred_degenerate(img3).reshape(img.shape)
    return (factor * img + (1.0 - factor) * deg).clamp(0, 1.0)


def apply(x, hflip=False, vflip=False, angle=None, fill=0.0, noise=None, sharpness=None):
    """the strong set's moves on x with given draws; `noise` = the noise tensor (already scaled by std), or None"""
    if hflip:
        x = x.flip(-1)
    if vflip:
        x = x.flip(-2)
    if angle is not None:
        x = rotate(x, angle, fill)
    if noise is not None:
        x = x + noise
    if sharpness is not None:
        x = adjust_sharpness(x, sharpness)
    return x


def draws(noise_like=None, p=0.5, p_noise=0.5, mask_transform=False):
    """the draw sequence of one augmentation_strong call (torchvision 0.10 order) from torch's generators; `noise_like`:
    the tensor the reference's torch.randn_like(x) runs on (its device's generator); p_noise: the noise RandomApply's p.
    -> dict of the decisions ('noise': the scaled noise tensor, or True without `noise_like`)"""
    d = dict(hflip=bool(torch.rand(1) < p), vflip=bool(torch.rand(1) < p), angle=None, noise=None, sharpness=None)
    if not p < torch.rand(1):
        d['angle'] = float(torch.empty(1).uniform_(float(-90), float(90)).item())
    if mask_transform:
        return d
    if not p_noise < torch.rand(1):
        d['noise'] = torch.randn_like(noise_like) * 0.0005 if noise_like is not None else True
    if torch.rand(1).item() < p:
        d['sharpness'] = 0.5
    return d
