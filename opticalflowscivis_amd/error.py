"""Drop-in for the reference's root error.py: the interpolation metrics (PSNR, SSIM) of a time series and the
time-step selection built on them (error.py:27-150), on the GPU.

Same names, arguments and return values as the reference:
  calculate_psnr(img1, img2), calculate_ssim(img1, img2)   one frame, numpy arrays in [0, 255] (error.py:27-76)
  calculate_metrics(original, interpol, factor)            means over the in-between frames i % factor != 0 (:78-107)
  select_timesteps(original, interpol, factor, threshold)  frames whose PSNR falls below the threshold (:130-150)
Every metric comes from ops.frame_metrics (one batched HIP launch for all frames of a call); data range L = 255.
Sequences [T,H,W] (or [T,H,W,C] with C in {1, 3}) are scored frame by frame with the reference's 11x11 Gaussian SSIM;
[T,D,H,W] sequences of volumes with the same window along three axes (the reference returns None for volumes,
error.py:67-74, so that form is this project's).  Every filtered extent must be >= 11 (valid 11-tap window).
"""
import statistics

import numpy as np
import torch

from . import ops

DATA_RANGE = 255.0


def _to_gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to("cuda")


def _layout(shape):
    """Frame shape -> (axis order putting channels first, window): H x W is one channel, H x W x C with C in {1, 3} the
    reference's cv2 layout, D x H x W a volume."""
    if len(shape) == 2:
        return None, "2d"
    if len(shape) == 3 and shape[2] in (1, 3):
        return (2, 0, 1), "2d"
    if len(shape) == 3:
        return None, "3d"
    raise ValueError('Wrong input image dimensions.')


def _frames(a):
    """[T, *frame] -> ([T, C, *spatial], window)."""
    order, window = _layout(a.shape[1:])
    return (a[:, None] if order is None else np.transpose(a, (0,) + tuple(o + 1 for o in order))), window


def frame_scores(original, interpol):
    """Per-frame (psnr, ssim) numpy fp64 arrays over the first min(len(original), len(interpol)) frames (error.py:85)."""
    original, interpol = np.asarray(original), np.asarray(interpol)
    n = min(original.shape[0], interpol.shape[0])
    a, window = _frames(original[:n])
    b, _ = _frames(interpol[:n])
    if a.shape != b.shape:
        raise ValueError('Input images must have the same dimensions.')
    psnr, ssim = ops.frame_metrics(_to_gpu(a), _to_gpu(b), DATA_RANGE, window)
    return psnr.cpu().numpy(), ssim.cpu().numpy()


def _one(img1, img2, window):
    p, s = ops.frame_metrics(_to_gpu(img1)[None], _to_gpu(img2)[None], DATA_RANGE, window)
    return float(p[0]), float(s[0])


def calculate_psnr(img1, img2):
    """PSNR of two images in [0, 255] (error.py:27-34): 20 log10(255 / sqrt(mse)), inf for identical images.
    H x W, H x W x C and D x H x W arrays; the kernel that sums the squared error also filters, so every spatial extent
    must be >= 11."""
    img1, img2 = np.asarray(img1), np.asarray(img2)
    if img1.shape != img2.shape:
        raise ValueError('Input images must have the same dimensions.')
    a, window = _frames(img1[None])
    b, _ = _frames(img2[None])
    return _one(a[0], b[0], window)[0]


def calculate_ssim(img1, img2):
    """SSIM of two images in [0, 255] (error.py:58-76), with the reference's shape rules: H x W; H x W x 3 (the mean
    over the three channels' maps); H x W x 1; other H x W x C -> None (the reference falls through there); any other
    number of dimensions -> ValueError."""
    img1, img2 = np.asarray(img1), np.asarray(img2)
    if not img1.shape == img2.shape:
        raise ValueError('Input images must have the same dimensions.')
    if img1.ndim == 2:
        return _one(img1[None], img2[None], "2d")[1]
    elif img1.ndim == 3:
        if img1.shape[2] == 3:
            return _one(np.moveaxis(img1, -1, 0), np.moveaxis(img2, -1, 0), "2d")[1]
        elif img1.shape[2] == 1:
            return _one(np.squeeze(img1)[None], np.squeeze(img2)[None], "2d")[1]
        return None
    else:
        raise ValueError('Wrong input image dimensions.')


def calculate_metrics(original_data, interpol_data, factor):
    """(mean PSNR, mean SSIM) over the in-between frames i % factor != 0 of the first min(T_original, T_interpol)
    frames (error.py:78-107); one batched GPU launch per call.  [T,D,H,W] sequences use the volumetric SSIM."""
    psnr, ssim = frame_scores(original_data, interpol_data)
    mid = [i for i in range(len(psnr)) if i % factor != 0]
    return statistics.mean(float(psnr[i]) for i in mid), statistics.mean(float(ssim[i]) for i in mid)


def select_from_psnr(psnr, factor, threshold=None):
    """(indices, threshold): the in-between frames (i % factor != 0) whose PSNR is below `threshold`, by default
    mean - mean / 10 of their PSNRs (error.py:133, 137-145)."""
    mid = [i for i in range(len(psnr)) if i % factor != 0]
    if threshold is None:
        m = statistics.mean(float(psnr[i]) for i in mid)
        threshold = m - m / 10.
    return [i for i in mid if float(psnr[i]) < threshold], float(threshold)


def select_timesteps(original_data, interpol_data, factor, threshold=None):
    """Indices of the time steps to keep: in-between frames whose PSNR against the original falls below `threshold`
    (default: mean - mean / 10 of the in-between PSNRs) -- the selection of error.py:130-150."""
    psnr, _ = frame_scores(original_data, interpol_data)
    return select_from_psnr(psnr, factor, threshold)[0]
