"""Drop-in for the reference's ``utils/hendrycks_robustness.Distortions`` (the common-corruption sweep, "C-testing" in
``figures/ABtesting.py``) with the pixel work on the GPU and on whole batches.

    Compose([RawProcessingPipeline(...), Distortions(severity, transform), Normalize(mean, std)])

becomes ``corrupt(static_pipeline(raw, ...), transform, severity, mean=mean, std=std)``: one call on the (B,3,H,W) float32
batch where it lies, the ``T.Normalize`` folded into the kernel's stores, no copy to the host between ISP and classifier.

Built: ``identity``, ``gaussian_noise``, ``shot_noise``, ``impulse_noise``, ``speckle_noise``, ``gaussian_blur``,
``zoom_blur``, ``contrast``, ``brightness``, ``saturate`` -- CMakeTable's list without ``elastic_transform`` (it rests on
OpenCV's fixed-point warpAffine), which raises like the transforms the reference itself leaves unused.  The deterministic
ones follow the reference's scikit-image 0.18 / scipy arithmetic per pixel; the random ones draw from the same distributions
with an in-kernel Philox4x32-10 generator keyed per call (``AddGaussianNoise``'s rule: same distribution, not numpy's stream).
The severity tables below are the reference's; they reach the kernels as launch arguments.  numpy is used for the host-side
tap and zoom-factor tables only -- there is no CPU path."""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import R2LError, ptr
from .functional import _f32c

KINDS = {'identity': 0, 'gaussian_noise': 1, 'shot_noise': 2, 'impulse_noise': 3, 'speckle_noise': 4, 'gaussian_blur': 5,
         'zoom_blur': 6, 'contrast': 7, 'brightness': 8, 'saturate': 9}
RANDOM = ('gaussian_noise', 'shot_noise', 'impulse_noise', 'speckle_noise')
NOT_BUILT = {
    'elastic_transform': "it rests on OpenCV's fixed-point warpAffine, which cannot be pinned here",
    **{t: "the reference's own sweep leaves it unused" for t in (
        'glass_blur', 'defocus_blur', 'motion_blur', 'fog', 'frost', 'snow', 'spatter', 'jpeg_compression', 'pixelate')}}

# utils/hendrycks_robustness.py, the `c = [...][severity - 1]` line of each method (zoom_blur: the stop of np.arange(1, stop, 0.01))
SEVERITY = {
    'identity': ((),) * 5,
    'gaussian_noise': (0.04, 0.06, .08, .09, .10),
    'shot_noise': (500, 250, 100, 75, 50),
    'impulse_noise': (.01, .02, .03, .05, .07),
    'speckle_noise': (.06, .1, .12, .16, .2),
    'gaussian_blur': (.4, .6, 0.7, .8, 1),
    'zoom_blur': (1.06, 1.11, 1.16, 1.21, 1.26),
    'contrast': (.75, .5, .4, .3, 0.15),
    'brightness': (.05, .1, .15, .2, .3),
    'saturate': ((0.3, 0), (0.1, 0), (1.5, 0), (2, 0.1), (2.5, 0.2)),
}


def gaussian_taps(sigma, truncate=4.0):
    """scipy.ndimage's _gaussian_kernel1d(sigma, 0, int(truncate * sigma + 0.5)) in float64, centre first (it is symmetric)"""
    radius = int(truncate * float(sigma) + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (float(sigma) * float(sigma)) * x ** 2)
    phi = phi / phi.sum()
    return [float(v) for v in phi[radius:]]


def zoom_factors(severity):
    """the reference's np.arange: floating point gives 7, 12, 16, 21, 26 factors"""
    return np.arange(1, SEVERITY['zoom_blur'][severity - 1], 0.01)


def zoom_table(severity, H):
    """per zoom factor z: (ch, top, out_size, trim_top, scale) of clipped_zoom on an H x H frame -- the crop ceil(H / z) from
    (H - ch) // 2, scipy.ndimage.zoom's output size round(ch z) (Python's round: half to even) and coordinate scale
    (ch - 1) / (out_size - 1), the centred trim back to H"""
    rows = []
    for z in zoom_factors(severity):
        ch = int(np.ceil(H / z))
        top = (H - ch) // 2
        out = int(round(ch * z))
        trim = (out - H) // 2
        scale = float(np.float64(ch - 1) / np.float64(out - 1)) if out > 1 else 1.0
        rows += [float(ch), float(top), float(out), float(trim), scale]
    return rows


def parameters(transform, severity, H):
    """the numbers r2l_corrupt takes for `transform` at `severity` on frames of height H"""
    c = SEVERITY[transform][severity - 1]
    if transform == 'gaussian_blur':
        return gaussian_taps(c)
    if transform == 'zoom_blur':
        return zoom_table(severity, H)
    return [float(v) for v in (c if isinstance(c, tuple) else (c,))]


def draw_key():
    """a 62-bit Philox key from torch's CPU generator (which set_global_seed seeds), as AddGaussianNoise draws its own"""
    return int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())


def _check(transform, severity):
    if transform in NOT_BUILT:
        raise R2LError(f'Distortions: {transform!r} is not built ({NOT_BUILT[transform]})')
    if transform not in KINDS:
        raise R2LError(f'Distortions: unknown transform {transform!r} (built: {", ".join(KINDS)})')
    if isinstance(severity, bool) or not isinstance(severity, (int, np.integer)) or not 1 <= severity <= 5:
        raise R2LError(f'Distortions: severity must be an integer from 1 to 5, got {severity!r}')


def corrupt(x, transform, severity, key=None, mean=None, std=None):
    """``Distortions(severity, transform)`` on a (3,H,W) image or a (B,3,H,W) batch of float32 on the device, every image
    treated as the reference treats its one; with ``mean`` and ``std`` (3 numbers each) the result is
    ``T.Normalize(mean, std)`` of it, from the same launch.  ``x`` must be float32 (TypeError otherwise; ``Distortions``
    converts like the reference).  ``key``: the Philox key of the random transforms (an int;
    drawn with ``draw_key()`` when None).  ``identity`` without mean / std returns ``x`` itself."""
    _check(transform, severity)
    if (mean is None) != (std is None):
        raise R2LError('corrupt: mean and std go together')
    if x.dim() not in (3, 4):
        raise R2LError(f'corrupt: expected a (3,H,W) image or a (B,3,H,W) batch, got {tuple(x.shape)}')
    x = _f32c(x, 'x')
    C, H, W = x.shape[-3:]
    N = x.shape[0] if x.dim() == 4 else 1
    if C != 3:
        raise R2LError(f'corrupt: the input should be RGB (3 channels), got {C}')
    if transform == 'zoom_blur' and H != W:
        raise R2LError(f'corrupt: zoom_blur needs square frames (the reference crops both axes by the height), got {H} x {W}')
    if transform in RANDOM and key is None:
        key = draw_key()
    if transform == 'identity' and mean is None:
        return x
    if x.numel() == 0:
        raise R2LError('corrupt: empty batch')
    lib, stream = _lib.library_for(x)
    kind = KINDS[transform]
    p = parameters(transform, int(severity), H)
    params = (ctypes.c_double * len(p))(*p) if p else None
    m3 = s3 = None
    if mean is not None:
        mean, std = [float(v) for v in mean], [float(v) for v in std]
        if len(mean) != 3 or len(std) != 3:
            raise R2LError('corrupt: mean and std have 3 entries each')
        if any(v == 0 for v in std):
            raise R2LError('corrupt: std has a zero entry (T.Normalize refuses it too)')
        m3, s3 = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)
    y = torch.empty_like(x)
    nbytes = lib.r2l_corrupt_workspace_bytes(kind, N, C, H, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device) if nbytes else None
    lib.check(lib.r2l_corrupt(ptr(x), ptr(y), N, C, H, W, kind, params, len(p), int(key or 0), 0, m3, s3, ptr(ws), nbytes,
                              stream), f'r2l_corrupt({transform})')
    return y


class Distortions:
    """utils/hendrycks_robustness.py:141-158: called with a (3,H,W) tensor like the reference's, or with a (B,3,H,W) batch.
    Like the reference it takes a tensor of any dtype and returns float32; unlike it, the tensor is converted BEFORE the
    transform (the reference computes in the input's dtype and converts the result), so a float64 image is corrupted in
    float32.  ``last_key`` holds the Philox key of the last call of a random transform (None otherwise)."""

    def __init__(self, severity=1, transform='identity'):
        _check(transform, severity)
        self.severity = severity
        self.transform = transform
        self.last_key = None

    def __call__(self, img):
        assert torch.is_tensor(img), 'Input data need to be a torch.tensor'
        assert img.dim() in (3, 4), 'Input image should be RGB'
        self.last_key = draw_key() if self.transform in RANDOM else None
        return corrupt(img.float(), self.transform, self.severity, key=self.last_key)

    def __repr__(self):
        return f'{self.__class__.__name__}(severity={self.severity}, transform={self.transform!r})'
