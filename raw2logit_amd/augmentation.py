"""Drop-in for the reference's ``utils/augmentation.py`` (weak set) with the pixel moves on the GPU.

``augmentation_weak`` = RandomHorizontalFlip, RandomVerticalFlip, RandomRotate90 (utils/augmentation.py:70-74),
applied to the processor's output batch between ISP and classifier (model.py:79-81) and, for segmentation, to
the masks with the same random state (``retain_state`` / ``mask_transform``, :36-67).  The random draws are made
on the host exactly where torchvision / the reference make them (``torch.rand(1) < p``, ``random.randint``), so a
seeded run takes the same decisions; the three moves of a call are then fused into ONE permutation kernel
(``r2l_augment``) instead of up to three passes, with the inverse permutation as its VJP.

``augmentation_strong`` (:77-84) = the two flips, RandomApply([RandomRotation(90)]), RandomApply([AddGaussianNoise(5e-4)])
and RandomAdjustSharpness(0.5), the last two on the image only.  torchvision 0.10's semantics are restated here (nothing is
imported from torchvision): nearest-neighbour rotation on its float32 sampling grid with a scalar fill, and the 3x3
blur / blend / clamp of adjust_sharpness.  A ComposeState call on that list makes every draw in the reference's order and
then runs ONE fused kernel (``r2l_augment_strong_fwd``: flips folded into the source index, rotation gather, in-kernel
Philox noise, sharpness through LDS); its VJP is at most two launches and gathers instead of scattering, so gradients are
bit-identical from run to run.  The noise key is drawn from the generator of the batch's device, as the reference's
``torch.randn_like(x)`` is, so the CPU generator sees the reference's draw sequence.  Any other transform list still runs
transform by transform."""
import math
import random

import numpy as np
import torch

from . import _lib
from ._lib import ptr
from .functional import _f32c


class _FlipRot(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, hflip, vflip, k):
        x = _f32c(x, 'x')
        H, W = x.shape[-2:]
        N = x.numel() // (H * W)
        lib, stream = _lib.library_for(x)
        out_shape = tuple(x.shape[:-2]) + ((W, H) if (k & 1) else (H, W))
        y = torch.empty(out_shape, dtype=torch.float32, device=x.device)
        lib.check(lib.r2l_augment(ptr(x), ptr(y), N, H, W, int(hflip), int(vflip), int(k), 0, stream), 'r2l_augment')
        ctx.meta = (N, H, W, int(hflip), int(vflip), int(k), tuple(x.shape))
        return y

    @staticmethod
    def backward(ctx, g):
        N, H, W, hflip, vflip, k, shape = ctx.meta
        g = _f32c(g, 'g')
        lib, stream = _lib.library_for(g)
        gx = torch.empty(shape, dtype=torch.float32, device=g.device)
        lib.check(lib.r2l_augment(ptr(g), ptr(gx), N, H, W, hflip, vflip, k, 1, stream), 'r2l_augment(inverse)')
        return gx, None, None, None


def flip_rot(x, hflip=False, vflip=False, k=0):
    """rot90^k(vflip(hflip(x))) over the last two axes, k as in ``x.rot90(k, dims=(-1, -2))``; one kernel."""
    if not (hflip or vflip or (k & 3)):
        return x
    return _FlipRot.apply(x, bool(hflip), bool(vflip), int(k) & 3)


class _Pending:
    """moves decided by the transforms of one ComposeState call, applied together at the end"""

    def __init__(self):
        self.hflip = self.vflip = False
        self.k = 0

    def flush(self, x):
        x = flip_rot(x, self.hflip, self.vflip, self.k)
        self.__init__()
        return x


class RandomHorizontalFlip:
    """torchvision.transforms.RandomHorizontalFlip: one draw per call, the whole batch flips (:71)."""

    def __init__(self, p=0.5):
        self.p = p

    def decide(self, pending):
        if torch.rand(1) < self.p:
            if pending.k:            # a flip after a rotation does not commute: apply what is pending first
                return True
            pending.hflip = not pending.hflip
        return False

    def __call__(self, x):
        return flip_rot(x, hflip=bool(torch.rand(1) < self.p))

    def __repr__(self):
        return f'{self.__class__.__name__}(p={self.p})'


class RandomVerticalFlip(RandomHorizontalFlip):
    """torchvision.transforms.RandomVerticalFlip (:72)."""

    def decide(self, pending):
        if torch.rand(1) < self.p:
            if pending.k:
                return True
            pending.vflip = not pending.vflip
        return False

    def __call__(self, x):
        return flip_rot(x, vflip=bool(torch.rand(1) < self.p))


class RandomRotate90:  # Note: not the same as T.RandomRotation(90)
    """utils/augmentation.py:8-14."""

    def decide(self, pending):
        pending.k = (pending.k + random.randint(0, 3)) & 3
        return False

    def __call__(self, x):
        return flip_rot(x, k=random.randint(0, 3))

    def __repr__(self):
        return self.__class__.__name__


class _PhiloxNoise(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, std, seed, offset):
        x = _f32c(x, 'x')
        lib, stream = _lib.library_for(x)
        y = torch.empty_like(x)
        lib.check(lib.r2l_add_noise_philox(ptr(x), ptr(y), float(std), int(seed), int(offset), x.numel(), stream),
                  'r2l_add_noise_philox')
        return y

    @staticmethod
    def backward(ctx, g):
        return g, None, None, None          # the noise does not depend on x


def add_gaussian_noise(x, std, seed, offset=0):
    """x + std * N(0,1), the deviates generated inside the kernel (Philox4x32-10 keyed by `seed`, Box-Muller): a pure
    function of (seed, offset, element index)"""
    return _PhiloxNoise.apply(x, std, seed, offset)


class AddGaussianNoise:
    """utils/augmentation.py:17-31: x + randn_like(x) * std.  The deviates come from an in-kernel Philox generator
    (no noise tensor, one pass over x); its 63-bit seed is drawn from torch's CPU generator, which
    ``set_global_seed`` seeds -- a seeded run reproduces its noise (same distribution as the reference's
    torch.randn_like, not the same stream)."""

    def __init__(self, std=0.01):
        self.std = std

    def __call__(self, x):
        seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
        return add_gaussian_noise(x, self.std, seed)

    def __repr__(self):
        return self.__class__.__name__ + f'(std={self.std})'


def set_global_seed(seed):
    """utils/augmentation.py:34-37."""
    torch.random.manual_seed(seed)
    np.random.seed(seed % (2**32 - 1))
    random.seed(seed)


class ComposeState:
    """utils/augmentation.py:40-67: a Compose that can replay its random state for the masks."""

    def __init__(self, transforms):
        self.transforms = []
        self.mask_transforms = []
        for t in transforms:
            apply_for_mask = True
            if isinstance(t, tuple):
                t, apply_for_mask = t
            self.transforms.append(t)
            if apply_for_mask:
                self.mask_transforms.append(t)
        self.seed = None

    def _enter(self, retain_state):
        """the reference's seed bookkeeping at the head of a call (:51-57)"""
        if self.seed is not None:   # retain previous state
            set_global_seed(self.seed)
        if retain_state:    # save state for next call
            self.seed = self.seed or torch.seed()
            set_global_seed(self.seed)
        else:
            self.seed = None    # reset / ignore state

    def arm(self, processor, retain_state=False):
        """Make the NEXT ``processor(x)`` call return the augmented batch: the draws of this transform list are made NOW
        (the processor consumes no host randomness, so a seeded run takes the same decisions as the reference, which
        draws after the processor call) and handed to the processor as a one-shot output epilogue -- the fused kernels
        then write the flipped / rotated output themselves instead of a separate 24 B/px pass, and the backward reads
        ``grad_out`` through the same map.  The ``self(x, retain_state=...)`` call that follows in model.py:79-81 returns
        its argument unchanged (once).  In LitModel.forward that is ONE added line in front of ``self.processor(x)``:

            if self.augmentation is not None and apply_augmentation_step:
                self.augmentation.arm(self.processor, retain_state=self.is_segmentation_task)

        Returns False (and arms nothing) for transform lists that hold anything but flips / rot90, or an order of them
        that does not commute into one permutation.  ``processor.buffer['processed_rgb']`` of an armed call holds the
        augmented output."""
        self._armed = None
        # only a processor that pops `_epilogue` itself may be armed (ParametrizedProcessing declares it); RawToRGB,
        # NNProcessing, nn.Identity (train.py:173-202) get the separate permutation kernel in __call__ as before
        if not getattr(processor, 'supports_output_epilogue', False):
            return False
        if not all(hasattr(t, 'decide') for t in self.transforms):
            return False
        state = (torch.random.get_rng_state(), np.random.get_state(), random.getstate(), self.seed)
        self._enter(retain_state)
        pending = _Pending()
        for t in self.transforms:
            if t.decide(pending):           # needs a flush in between: not one permutation -- undo the draws
                torch.random.set_rng_state(state[0])
                np.random.set_state(state[1])
                random.setstate(state[2])
                self.seed = state[3]
                return False
        processor.__dict__['_epilogue'] = (pending.hflip, pending.vflip, pending.k)
        self._armed = processor
        return True

    def __call__(self, x, retain_state=False, mask_transform=False):
        armed = getattr(self, '_armed', None)
        if armed is not None and not mask_transform:
            self._armed = None
            # consumed: the processor's epilogue already applied this call's moves.  Still there (the processor raised
            # before its pop, or was never called): the draws are made, apply them here so that image and mask agree
            left = armed.__dict__.pop('_epilogue', None)
            return x if left is None else flip_rot(x, *left)
        self._enter(retain_state)
        transforms = self.transforms if not mask_transform else self.mask_transforms
        plan = _strong_plan(transforms)
        if plan is not None:                  # the strong set: every draw in the reference's order, then one fused launch
            self.last_draws = _draw_strong(plan, x)
            return strong_augment(x, **self.last_draws)
        pending = _Pending()
        for t in transforms:
            if hasattr(t, 'decide'):          # flip / rot90: drawn now (reference order), moved once at the end
                if t.decide(pending):         # the move does not commute with what is pending: flush, then redo
                    x = pending.flush(x)
                    if isinstance(t, RandomVerticalFlip):
                        pending.vflip = True
                    else:
                        pending.hflip = True
            else:
                x = t(pending.flush(x))
        return pending.flush(x)


# ---- the strong set (utils/augmentation.py:77-84) ----------------------------------------------------------------------
def _rotation_coefficients(angle, H, W):
    """torchvision 0.10 F.rotate(angle, expand=False, center=None) -> theta^T / [W/2, H/2] of _gen_affine_grid, float32:
    the matrix _get_inverse_affine_matrix([0, 0], -angle, [0, 0], 1, [0, 0]) = [cos, sin, 0, -sin, cos, 0] in doubles,
    cast to float32, then divided (float32) by W/2 (grid x) and H/2 (grid y)"""
    rot = math.radians(-angle)
    c, s = np.float32(math.cos(rot)), np.float32(math.sin(rot))
    w2, h2 = np.float32(0.5 * W), np.float32(0.5 * H)
    return float(c / w2), float(s / w2), float(-s / h2), float(c / h2)


class _StrongAug(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, geom, fill, std, key, sharpness):
        x = _f32c(x, 'x')
        H, W = x.shape[-2:]
        N = x.numel() // (H * W)
        C = x.shape[-3] if x.dim() >= 3 else 1
        lib, stream = _lib.library_for(x)
        y = torch.empty_like(x)
        mask = None
        if sharpness >= 0 and ctx.needs_input_grad[0]:
            mask = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
        lib.check(lib.r2l_augment_strong_fwd(ptr(x), ptr(y), ptr(mask), N, C, H, W, *geom, float(fill), float(std),
                                             ptr(key), 0, float(sharpness), stream), 'r2l_augment_strong_fwd')
        ctx.meta = (N, C, H, W, geom, float(sharpness))
        ctx.mask = mask
        return y

    @staticmethod
    def backward(ctx, g):
        N, C, H, W, geom, sharpness = ctx.meta
        g = _f32c(g, 'g')
        lib, stream = _lib.library_for(g)
        gx = torch.empty_like(g)
        work = torch.empty_like(g) if (sharpness >= 0 and H > 2 and W > 2) else None
        lib.check(lib.r2l_augment_strong_bwd(ptr(g), ptr(gx), ptr(ctx.mask), ptr(work), N, C, H, W, *geom, sharpness,
                                             stream), 'r2l_augment_strong_bwd')
        return gx, None, None, None, None, None


def strong_augment(x, hflip=False, vflip=False, angle=None, fill=0.0, noise_std=0.0, noise_key=None, sharpness=None):
    """adjust_sharpness(rotate(vflip(hflip(x)), angle, NEAREST, fill) + noise_std * n(noise_key), sharpness) over the last
    two axes, each step only where given, in one launch (torchvision 0.10 semantics).  ``noise_key``: an int64[1] tensor
    on x's device (the deviates are r2l_add_noise_philox's at the flat output index).  Nothing given returns ``x``;
    flips alone go to the permutation kernel."""
    if angle is None and noise_key is None and sharpness is None:
        return flip_rot(x, hflip, vflip)
    if sharpness is not None and sharpness < 0:
        raise ValueError('sharpness_factor is not non-negative.')
    if noise_key is not None and (noise_key.dtype != torch.int64 or noise_key.numel() != 1 or
                                  noise_key.device != x.device):
        raise _lib.R2LError('noise_key must be an int64 tensor of one element on the device of x')
    H, W = x.shape[-2:]
    geom = (int(bool(hflip)), int(bool(vflip)), int(angle is not None)) + \
        (_rotation_coefficients(float(angle), H, W) if angle is not None else (0.0, 0.0, 0.0, 0.0))
    return _StrongAug.apply(x, geom, float(fill), float(noise_std), noise_key,
                            -1.0 if sharpness is None else float(sharpness))


def rotate(x, angle, fill=0.0):
    """torchvision 0.10 F.rotate(x, angle, InterpolationMode.NEAREST, expand=False, center=None, fill=[fill] * C)"""
    return strong_augment(x, angle=angle, fill=fill)


def adjust_sharpness(x, sharpness_factor):
    """torchvision 0.10 F.adjust_sharpness on float images in [0, 1] (the clamp applies whatever the range)"""
    return strong_augment(x, sharpness=sharpness_factor)


class RandomApply:
    """torchvision.transforms.RandomApply: skipped when p < torch.rand(1), else the transforms in order"""

    def __init__(self, transforms, p=0.5):
        self.transforms = list(transforms)
        self.p = p

    def __call__(self, x):
        if self.p < torch.rand(1):
            return x
        for t in self.transforms:
            x = t(x)
        return x

    def __repr__(self):
        return f'{self.__class__.__name__}(p={self.p}, transforms={self.transforms})'


class RandomRotation:
    """torchvision.transforms.RandomRotation (0.10) for tensors: NEAREST, expand=False, center=None, a scalar fill"""

    def __init__(self, degrees, interpolation='nearest', expand=False, center=None, fill=0, resample=None):
        if isinstance(degrees, (int, float)):
            if degrees < 0:
                raise ValueError('If degrees is a single number, it must be positive.')
            degrees = [-degrees, degrees]
        else:
            if len(degrees) != 2:
                raise ValueError('degrees should be a sequence of length 2.')
            degrees = list(degrees)
        mode = getattr(interpolation, 'value', interpolation)
        if resample is not None or mode != 'nearest':
            raise _lib.R2LError(f'RandomRotation: only NEAREST interpolation is built (got {interpolation!r})')
        if expand:
            raise _lib.R2LError('RandomRotation: expand=True is not built (the output keeps H x W)')
        if center is not None:
            raise _lib.R2LError('RandomRotation: only the frame centre is built (center=None)')
        if not isinstance(fill, (int, float)):
            raise _lib.R2LError('RandomRotation: only a scalar fill is built')
        self.degrees = degrees
        self.interpolation = 'nearest'
        self.expand = False
        self.center = None
        self.fill = fill
        self.resample = None

    @staticmethod
    def get_params(degrees):
        return float(torch.empty(1).uniform_(float(degrees[0]), float(degrees[1])).item())

    def __call__(self, x):
        return rotate(x, self.get_params(self.degrees), fill=float(self.fill))

    def __repr__(self):
        return f'{self.__class__.__name__}(degrees={self.degrees}, interpolation=nearest, expand=False, fill={self.fill})'


class RandomAdjustSharpness:
    """torchvision.transforms.RandomAdjustSharpness: adjust_sharpness when torch.rand(1).item() < p"""

    def __init__(self, sharpness_factor, p=0.5):
        self.sharpness_factor = sharpness_factor
        self.p = p

    def __call__(self, x):
        if torch.rand(1).item() < self.p:
            return adjust_sharpness(x, self.sharpness_factor)
        return x

    def __repr__(self):
        return f'{self.__class__.__name__}(sharpness_factor={self.sharpness_factor},p={self.p})'


_STRONG_ORDER = {'hflip': 0, 'vflip': 0, 'rot': 1, 'noise': 2, 'sharp': 3}


def _strong_plan(transforms):
    """[(kind, RandomApply p or None, transform)] when the list is flips, then a rotation, noise and a sharpness adjustment
    (each at most once, any of them absent, rotation and noise optionally inside a one-transform RandomApply) with a
    rotation or a sharpness adjustment among them; else None (the transform-by-transform path)"""
    plan, seen, last = [], set(), 0
    for t in transforms:
        p, inner = None, t
        if isinstance(t, RandomApply):
            if len(t.transforms) != 1:
                return None
            p, inner = t.p, t.transforms[0]
        if type(inner) is RandomHorizontalFlip and p is None:
            kind = 'hflip'
        elif type(inner) is RandomVerticalFlip and p is None:
            kind = 'vflip'
        elif type(inner) is RandomRotation:
            kind = 'rot'
        elif type(inner) is AddGaussianNoise:
            kind = 'noise'
        elif type(inner) is RandomAdjustSharpness and p is None:
            kind = 'sharp'
        else:
            return None
        if kind in seen or _STRONG_ORDER[kind] < last:
            return None
        seen.add(kind)
        last = _STRONG_ORDER[kind]
        plan.append((kind, p, inner))
    return plan if seen & {'rot', 'sharp'} else None


def _draw_strong(plan, x):
    """the draws of one call, in the reference's order: a RandomApply's torch.rand(1), then its transform's own.  The noise
    key comes from the generator of x's device (the reference's torch.randn_like(x)), the rest from the CPU generator"""
    d = dict(hflip=False, vflip=False, angle=None, fill=0.0, noise_std=0.0, noise_key=None, sharpness=None)
    for kind, p, t in plan:
        if p is not None and p < torch.rand(1):
            continue
        if kind in ('hflip', 'vflip'):
            d[kind] = bool(torch.rand(1) < t.p)
        elif kind == 'rot':
            d['angle'] = t.get_params(t.degrees)
            d['fill'] = float(t.fill)
        elif kind == 'noise':
            d['noise_std'] = float(t.std)
            d['noise_key'] = torch.randint(0, 2 ** 62, (1,), dtype=torch.int64, device=x.device)
        elif torch.rand(1).item() < t.p:
            d['sharpness'] = float(t.sharpness_factor)
    return d


augmentation_weak = ComposeState([
    RandomHorizontalFlip(),
    RandomVerticalFlip(),
    RandomRotate90(),
])


augmentation_strong = ComposeState([
    RandomHorizontalFlip(p=0.5),
    RandomVerticalFlip(p=0.5),
    RandomApply([RandomRotation(90)], p=0.5),
    (RandomApply([AddGaussianNoise(std=0.0005)], p=0.5), False),   # image only
    (RandomAdjustSharpness(0.5, p=0.5), False),                    # image only
])


def get_augmentation(type):
    """utils/augmentation.py:87-93."""
    if type == 'none':
        return None
    if type == 'weak':
        return augmentation_weak
    if type == 'strong':
        return augmentation_strong
