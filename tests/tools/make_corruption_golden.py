"""Writes tests/golden/corruptions.npz: the reference's own ``Distortions`` results for the deterministic transforms.

    python tests/tools/make_corruption_golden.py <path of the reference checkout>

Runs where the reference is checked out (the test suite only reads the file this writes).  The reference module
``utils/hendrycks_robustness.py`` is imported UNMODIFIED; the packages it imports at module level and that this project does
not depend on (skimage, cv2, wand, torchvision, PIL, scipy.ndimage.interpolation) are stubbed through ``sys.modules``, and
``np.float_`` (gone from numpy 2) is put back.  Three of the stubs carry arithmetic the deterministic transforms reach:
``skimage.filters.gaussian``, ``skimage.color.rgb2hsv`` and ``skimage.color.hsv2rgb`` below are OWN RESTATEMENTS of
scikit-image 0.18 on scipy / numpy, written from its documented behaviour and source layout -- unpinned, like the Malvar2004
restatement behind the static goldens: scikit-image itself is not installed where this ran.  Everything else (the severity
tables, clipped_zoom on scipy.ndimage.zoom, contrast, the clips, the torch <-> numpy conversions) is the reference's code.

Stored per case ``<transform>_s<severity>_<H>``: ``ref64_*`` = the method on a float64 copy of the input, as float32, and
``ulp_*`` = the distance in float32 ULPs from that to the reference's own float32 result (int16), which reads back as
``(ref64.view(int32) + ulp).view(float32)`` -- two nearly equal float32 arrays would not fit the size limit.  ``x_<H>``: inputs."""
import importlib.util
import os
import sys
import types

import numpy as np
import scipy.ndimage as ndi
import torch

TRANSFORMS = ('contrast', 'brightness', 'saturate', 'gaussian_blur', 'zoom_blur')
FRAMES = {8: (1, 2, 3, 4, 5), 18: (1, 2, 3, 4, 5), 34: (5,)}      # 8 < 2 radius + 1 at severity 5; 34 % 4 != 0


# ---- own restatements of scikit-image 0.18 (float32 stays float32, as its img_as_float leaves it) -----------------------
def gaussian(image, sigma=1, output=None, mode='nearest', cval=0, multichannel=None, preserve_range=False, truncate=4.0):
    image = np.asarray(image)
    if image.dtype not in (np.float32, np.float64):
        image = image.astype(np.float64)
    sig = [sigma] * (image.ndim - 1) + [0] if multichannel else [sigma] * image.ndim
    out = np.empty_like(image)
    ndi.gaussian_filter(image, sig, output=out, mode=mode, cval=cval, truncate=truncate)
    return out


def rgb2hsv(rgb):
    arr = np.asarray(rgb)
    out = np.empty_like(arr)
    out_v = arr.max(-1)
    delta = np.ptp(arr, -1)
    old = np.seterr(invalid='ignore', divide='ignore')
    out_s = delta / out_v
    out_s[delta == 0.] = 0.
    idx = (arr[..., 0] == out_v)                        # red is max
    out[idx, 0] = (arr[idx, 1] - arr[idx, 2]) / delta[idx]
    idx = (arr[..., 1] == out_v)                        # green is max
    out[idx, 0] = 2. + (arr[idx, 2] - arr[idx, 0]) / delta[idx]
    idx = (arr[..., 2] == out_v)                        # blue is max
    out[idx, 0] = 4. + (arr[idx, 0] - arr[idx, 1]) / delta[idx]
    out_h = (out[..., 0] / 6.) % 1.
    out_h[delta == 0.] = 0.
    np.seterr(**old)
    out[..., 0] = out_h
    out[..., 1] = out_s
    out[..., 2] = out_v
    out[np.isnan(out)] = 0
    return out


def hsv2rgb(hsv):
    arr = np.asarray(hsv)
    hi = np.floor(arr[..., 0] * 6)
    f = arr[..., 0] * 6 - hi
    p = arr[..., 2] * (1 - arr[..., 1])
    q = arr[..., 2] * (1 - f * arr[..., 1])
    t = arr[..., 2] * (1 - (1 - f) * arr[..., 1])
    v = arr[..., 2]
    hi = np.stack([hi, hi, hi], axis=-1).astype(np.uint8) % 6
    return np.choose(hi, np.stack([np.stack((v, t, p), axis=-1), np.stack((q, v, p), axis=-1), np.stack((p, v, t), axis=-1),
                                   np.stack((p, q, v), axis=-1), np.stack((t, p, v), axis=-1), np.stack((v, p, q), axis=-1)]))


def _module(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def import_reference(root):
    if not hasattr(np, 'float_'):
        np.float_ = np.float64
    anything = type('Anything', (), {'__getattr__': lambda self, n: type(self)(), '__call__': lambda self, *a, **k: None})
    _module('skimage', filters=_module('skimage.filters', gaussian=gaussian),
            color=_module('skimage.color', rgb2hsv=rgb2hsv, hsv2rgb=hsv2rgb), util=_module('skimage.util'))
    _module('cv2')
    _module('wand', image=_module('wand.image', Image=type('Image', (), {})), api=_module('wand.api', library=anything()),
            color=_module('wand.color'))
    _module('torchvision', datasets=_module('torchvision.datasets'), transforms=_module('torchvision.transforms'))
    try:
        import PIL.Image  # noqa: F401
    except ImportError:
        _module('PIL', Image=_module('PIL.Image'))
    _module('scipy.ndimage.interpolation', map_coordinates=ndi.map_coordinates)
    spec = importlib.util.spec_from_file_location('hendrycks_robustness', os.path.join(root, 'utils', 'hendrycks_robustness.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def frame(H, seed):
    """uniform in [0, 1] with exact 0, exact 1 and grey pixels (the delta = 0 branch of rgb2hsv) among them"""
    rng = np.random.default_rng(seed)
    x = rng.random((3, H, H)).astype(np.float32)
    x[0, 0, 0] = 0.0
    x[1, 0, 1] = 1.0
    x[:, 1, 2] = 0.0                 # black: V = 0
    x[:, 2, 1] = 1.0                 # white
    x[:, 3, 3] = x[0, 3, 3]          # grey
    x[:, H - 1, H - 1] = x[1, H - 1, H - 1]
    x[2, H - 1, 0] = x[1, H - 1, 0]  # two channels tie for the maximum or the minimum
    x[0, 0, H - 1] = x[2, 0, H - 1]
    return x


def main():
    ref = import_reference(sys.argv[1])
    out = {}
    for H, severities in FRAMES.items():
        x = frame(H, 100 + H)
        out[f'x_{H}'] = x
        for t in TRANSFORMS:
            for sev in severities:
                d = ref.Distortions(severity=sev, transform=t)
                y32 = d(torch.from_numpy(x.copy())).numpy()
                y64 = d(torch.from_numpy(x.astype(np.float64))).numpy()
                assert y32.dtype == np.float32 and y64.dtype == np.float32 and y32.shape == x.shape
                ulp = y32.view(np.int32).astype(np.int64) - y64.view(np.int32).astype(np.int64)
                assert np.abs(ulp).max() < 2 ** 15, (t, sev, H, np.abs(ulp).max())
                out[f'ref64_{t}_s{sev}_{H}'] = y64
                out[f'ulp_{t}_s{sev}_{H}'] = ulp.astype(np.int16)
                print(f'{t} severity {sev} {H}x{H}: float32 vs float64 evaluation max|diff| '
                      f'{np.abs(y32.astype(np.float64) - y64).max():.2e}')
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'golden', 'corruptions.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < 256 * 1024


if __name__ == '__main__':
    main()
