"""Float64 restatement of the deterministic common corruptions (utils/hendrycks_robustness.py: Distortions), written from
their semantics -- numpy, with scipy for the Gaussian filter and the zoom.  It travels with the tests (the reference does
not); tests/test_corruptions.py holds it to the reference's own results in tests/golden/corruptions.npz.

Every function takes (..., 3, H, W) arrays (an image or a batch, channels first as the kernels see them), computes in
float64 whatever comes in, and treats each image on its own."""
import numpy as np
import scipy.ndimage as ndi

CONTRAST = (.75, .5, .4, .3, .15)
BRIGHTNESS = (.05, .1, .15, .2, .3)
SATURATE = ((.3, 0), (.1, 0), (1.5, 0), (2, .1), (2.5, .2))
BLUR_SIGMA = (.4, .6, .7, .8, 1)
ZOOM_STOP = (1.06, 1.11, 1.16, 1.21, 1.26)
DETERMINISTIC = ('identity', 'contrast', 'brightness', 'saturate', 'gaussian_blur', 'zoom_blur')


def _f64(x):
    return np.asarray(x, dtype=np.float64)


def identity(x, severity=1):
    return _f64(x)


def contrast(x, severity):
    x = _f64(x)
    m = x.mean(axis=(-2, -1), keepdims=True)            # per image, per channel
    return np.clip((x - m) * CONTRAST[severity - 1] + m, 0, 1)


def to_hsv(x):
    """hue in [0, 1) by sextant of the largest channel (blue wins ties, then green), saturation (max - min) / max, value max;
    hue and saturation 0 where max == min"""
    r, g, b = x[..., 0, :, :], x[..., 1, :, :], x[..., 2, :, :]
    v = np.maximum(np.maximum(r, g), b)
    d = v - np.minimum(np.minimum(r, g), b)
    safe = np.where(d == 0, 1.0, d)
    with np.errstate(divide='ignore', invalid='ignore'):
        s = np.where(d == 0, 0.0, d / v)
    h = np.where(b == v, 4 + (r - g) / safe, np.where(g == v, 2 + (b - r) / safe, (g - b) / safe))
    h = np.where(d == 0, 0.0, np.mod(h / 6, 1.0))
    return h, s, v


def from_hsv(h, s, v):
    i = np.floor(h * 6)
    f = h * 6 - i
    p, q, t = v * (1 - s), v * (1 - f * s), v * (1 - (1 - f) * s)
    i = i.astype(np.int64) % 6
    table = {0: (v, t, p), 1: (q, v, p), 2: (p, v, t), 3: (p, q, v), 4: (t, p, v), 5: (v, p, q)}
    out = [np.select([i == k for k in range(6)], [table[k][c] for k in range(6)]) for c in range(3)]
    return np.stack(out, axis=-3)


def brightness(x, severity):
    h, s, v = to_hsv(_f64(x))
    return np.clip(from_hsv(h, s, np.clip(v + BRIGHTNESS[severity - 1], 0, 1)), 0, 1)


def saturate(x, severity):
    h, s, v = to_hsv(_f64(x))
    c0, c1 = SATURATE[severity - 1]
    return np.clip(from_hsv(h, np.clip(s * c0 + c1, 0, 1), v), 0, 1)


def gaussian_blur(x, severity):
    x = _f64(x)
    sigma = [0] * (x.ndim - 2) + [BLUR_SIGMA[severity - 1]] * 2         # over H and W only
    return np.clip(ndi.gaussian_filter(x, sigma, mode='nearest', truncate=4.0), 0, 1)


def zoom_blur(x, severity):
    x = _f64(x)
    H, W = x.shape[-2:]
    assert H == W, 'zoom_blur: square frames only (the reference crops both axes by the height)'
    factors = np.arange(1, ZOOM_STOP[severity - 1], 0.01)
    lead = (1,) * (x.ndim - 2)
    acc = np.zeros_like(x)
    for z in factors:
        ch = int(np.ceil(H / z))
        top = (H - ch) // 2
        zoomed = ndi.zoom(x[..., top:top + ch, top:top + ch], lead + (z, z), order=1)
        trim = (zoomed.shape[-1] - H) // 2
        acc += zoomed[..., trim:trim + H, trim:trim + H]
    return np.clip((x + acc) / (len(factors) + 1), 0, 1)


def apply(x, transform, severity):
    return globals()[transform](x, severity)


def normalize(y, mean, std):
    """T.Normalize(mean, std) on (..., 3, H, W)"""
    m = np.asarray(mean, dtype=np.float64).reshape(3, 1, 1)
    s = np.asarray(std, dtype=np.float64).reshape(3, 1, 1)
    return (_f64(y) - m) / s
