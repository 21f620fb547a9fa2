"""Drop-in for the reference's ``processing/pipeline_numpy.py`` (static pipeline) on MI355X.

``processing(img, black_level, white_balance, colour_matrix, debayer=..., sharpening=..., denoising=...)``
and ``RawProcessingPipeline`` keep the reference's signatures and return types
(/root/reference/processing/pipeline_numpy.py:36-141) but run the batched static kernel of libr2l_isp.so
(float64 linear part, numpy semantics: symmetric borders, clip to [0,1], gamma 2.2).

The reference applies this per image inside DataLoader worker processes (train.py:164-171, :318); a GPU
context cannot live in forked workers, so the batched form ``StaticProcessing`` (an nn.Module to use as
the ``processor`` on device batches) is the fast path, and the per-image callables below are the
API-compatible wrappers for the main process (figures/ABtesting.py:135-173, app.py:13-35)."""
import numpy as np
import torch
import torch.nn as nn

from .. import functional as F_


def _device():
    if torch.cuda.is_available():
        return torch.device('cuda')
    return torch.device('cpu')      # only usable under the test emulation; _lib raises otherwise


def processing(img, black_level, white_balance, colour_matrix, debayer="bilinear",
               sharpening="unsharp_masking", sharp_radius=1.0, sharp_amount=1.0,
               denoising="median_filter", median_kernel_size=3, gaussian_sigma=0.5, fft_fraction=0.3,
               weight_chambolle=0.01, weight_bregman=100, sigma_bilateral=0.6, gamma=2.2, bits=16):
    """reference :70-141.  img (H,W) float ndarray -> (H,W,3) float64 ndarray.

    As in the reference, `img` has its black level removed IN PLACE (:152-158), in the array's own dtype:
    a float32 frame (what the reference's datasets hand over, dataset.py:86-87; docstring :57) gets the
    float32 subtraction, a float64 frame the float64 one -- on the device exactly as in the caller's array.
    Option strings that name no algorithm skip their stage (the signature default denoising="median_filter"
    is one).  sharp_radius / sharp_amount / median_kernel_size / gaussian_sigma / fft_fraction (:117-122) are launch
    arguments of the kernels, within what their windows hold (functional.static_pipeline: gaussian_sigma < 0.625,
    sharp_radius < 1.125, median_kernel_size 3 or 5, fft_fraction in [0, 0.5]; anything else raises R2LError with the reason --
    INTEGRATION.md); weight_chambolle / weight_bregman / sigma_bilateral belong to denoisers this library does not build."""
    if not (isinstance(img, np.ndarray) and img.dtype in (np.float32, np.float64)):
        raise TypeError('processing() takes a float32 or float64 ndarray (dataset.py:86-87 delivers float32)')
    raw = torch.from_numpy(np.ascontiguousarray(img))[None].to(_device())
    out = F_.static_pipeline(raw, (black_level, white_balance, colour_matrix), debayer=debayer,
                             sharpening=sharpening, denoising=denoising, gamma=gamma, sharp_radius=sharp_radius,
                             sharp_amount=sharp_amount, median_kernel_size=median_kernel_size,
                             gaussian_sigma=gaussian_sigma, fft_fraction=fft_fraction)
    img[0::2, 0::2] -= black_level[0]      # side effect of remove_blacklv on the caller's array
    img[0::2, 1::2] -= black_level[1]
    img[1::2, 0::2] -= black_level[2]
    img[1::2, 1::2] -= black_level[3]
    return out[0].permute(1, 2, 0).cpu().numpy().astype(np.float64)


class RawProcessingPipeline(object):
    """reference :36-67: callable transform, (H,W) ndarray -> (3,H,W) float32 tensor."""

    def __init__(self, camera_parameters, debayer='bilinear', sharpening='unsharp_masking', denoising='gaussian'):
        self.camera_parameters = camera_parameters

        self.debayer = debayer
        self.sharpening = sharpening
        self.denoising = denoising

    def __call__(self, img):
        black_level, white_balance, colour_matrix = self.camera_parameters
        img = processing(img, black_level, white_balance, colour_matrix,
                         debayer=self.debayer, sharpening=self.sharpening, denoising=self.denoising)
        img = img.transpose(2, 0, 1)

        return torch.Tensor(img)


class StaticProcessing(nn.Module):
    """Batched static pipeline as a ``processor`` module: (B,H,W) raw on the GPU -> (B,3,H,W).

    Equals RawProcessingPipeline applied to every frame followed by the optional T.Normalize(mean, std)
    of train.py:157-171 (fused into the pipeline's kernels: r2l_static_fwd_norm).  No trainable parameters, no gradient.  Frames may be float32 in [0,1] or the
    sensor's 16-bit containers (uint16 / int16 tensors, divided by 2**raw_bits - 1 inside the kernel).

    ``output_dtype`` (opt-in, default None = float32) -- ``torch.bfloat16`` or ``torch.float16``: the module returns
    ``float32_result.to(output_dtype)`` bit for bit (Normalize included), for a task model that runs under torch.autocast /
    precision=16.  Where one row-streaming kernel runs the chain (functional.static_io_why: bilinear / Malvar2004, W % 4 == 0,
    W <= 2048, no fft_denoising, no 5x5 median, float64 frames on the short chain only) it stores the 16-bit values itself -- 6
    instead of 12 bytes per pixel, no cast pass; everywhere else the float32 kernels run and torch casts.  Anything but None or
    those three dtypes raises R2LError.

    ``supports_output_epilogue`` -- this class pops the one-shot `_epilogue` an augmentation armed (ComposeState.arm): the next
    call returns the flipped / rotated batch, ``flip_rot(plain_output, hflip, vflip, k)`` bit for bit.  Where one row-streaming
    kernel runs the chain and k is even (functional.static_epilogue_why) that kernel stores the rows at their flipped positions;
    everywhere else the plain call runs and the permutation kernel follows, right here."""

    raw_bits = 16
    output_dtype = None
    supports_output_epilogue = True

    def __init__(self, camera_parameters, debayer='bilinear', sharpening='sharpening_filter',
                 denoising='gaussian_denoising', gamma=2.2, mean=None, std=None, **options):
        super().__init__()
        unknown = set(options) - set(F_.STATIC_OPTION_DEFAULTS)
        if unknown:
            raise TypeError(f'unknown static options {sorted(unknown)} (have: {sorted(F_.STATIC_OPTION_DEFAULTS)})')
        self.options = dict(options)          # processing()'s numeric arguments (pipeline_numpy.py:70-73), see static_pipeline
        self.camera_parameters = tuple(list(map(float, p)) for p in camera_parameters)
        self.debayer = debayer
        self.sharpening = sharpening
        self.denoising = denoising
        self.gamma = gamma
        self.stages = None
        self.buffer = None
        if mean is not None:
            self.register_buffer('mean_std', torch.cat([torch.as_tensor(mean, dtype=torch.float32).reshape(3),
                                                        torch.as_tensor(std, dtype=torch.float32).reshape(3)]))
        else:
            self.mean_std = None

    @torch.no_grad()
    def forward(self, raw):
        assert raw.ndim == 3, f"needs dims (B, H, W), got {raw.shape}"
        # a one-shot output epilogue armed by the augmentation drop-in (ComposeState.arm); a call that raises before this pop
        # leaves it for ComposeState.__call__ to apply
        epilogue = self.__dict__.pop('_epilogue', None)
        self.stages = {}
        self.buffer = {}
        odt = self.output_dtype
        if odt not in F_.IO_CODES:
            raise F_._lib.R2LError(f'output_dtype must be None, torch.float32, torch.bfloat16 or torch.float16, got {odt!r}')
        # (unset: exactly the call of a module without the attribute)
        io = dict(out_dtype=odt) if F_.IO_CODES[odt] != F_.IO_F32 else {}
        if epilogue is not None and F_.epilogue_bits(epilogue):
            io['epilogue'] = epilogue
        rgb = F_.static_pipeline(raw, self.camera_parameters, self.debayer, self.sharpening,
                                 self.denoising, self.gamma, bits=self.raw_bits, mean_std=self._mean_std_host(),
                                 **getattr(self, 'options', {}), **io)
        self.buffer['processed_rgb'] = rgb
        return rgb

    @torch.no_grad()
    def statistics(self, frames, unbiased=True):
        """(mean, std), float32 of shape (3,1,1): torch.mean / torch.std over (0, 2, 3) of this chain's float32, un-normalised
        output on `frames` -- what get_statistics (pipeline_numpy.py:306-329) returns for a training subset, i.e. the
        ``mean=`` / ``std=`` of a StaticProcessing that normalises.  `frames`: a (B,H,W) tensor, or any iterable of such
        tensors (a loader of raw batches; batch and frame sizes may differ): the seven float64 sums of
        functional.static_statistics are additive and are added on the device in iteration order.  Where one row-streaming
        kernel runs the chain the output is never stored.  The module's own mean / std and output_dtype play no part;
        ``stages`` and ``buffer`` are left alone; ``raw_bits`` and the numeric options count as in forward."""
        total = None
        for raw in ([frames] if torch.is_tensor(frames) else frames):
            s = F_.static_statistics(raw, self.camera_parameters, self.debayer, self.sharpening, self.denoising, self.gamma,
                                     bits=self.raw_bits, **getattr(self, 'options', {}))
            total = s if total is None else total + s
        if total is None:
            raise ValueError('statistics() needs at least one batch of frames')
        return F_.mean_std_from_sums(total, unbiased)

    def _mean_std_host(self):
        """the six floats of the mean_std buffer on the host (the kernels take them as launch arguments), read
        back once per value of the buffer"""
        ms = self.mean_std
        if ms is None:
            return None
        key = (ms.data_ptr(), ms._version)
        cached = self.__dict__.get('_ms_host')
        if cached is None or cached[0] != key:
            cached = (key, [float(v) for v in ms.detach().cpu().tolist()])
            self.__dict__['_ms_host'] = cached
        return cached[1]
