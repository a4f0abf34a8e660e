"""A restatement in numpy of the five OpenCV calls IP-Basic makes (cv2 is not a dependency of this project).

Each function follows OpenCV's documented semantics for a single-channel float32 image:
  * dilate / erode: a 0/1 kernel of any size with cv2's default anchor (kw // 2, kh // 2); the image border takes no part
    (OpenCV's default border value: -FLT_MAX for a dilation, +FLT_MAX for an erosion).
  * morphologyEx(MORPH_CLOSE): dilate, then erode, with the same kernel.
  * medianBlur(src, 5): the 13th of the 25 values of the window, BORDER_REPLICATE.  A selection: exact by definition.
  * GaussianBlur(src, (5, 5), 0): OpenCV's fixed 5-tap kernel [1, 4, 6, 4, 1] / 16 (getGaussianKernel with sigma <= 0),
    BORDER_REFLECT_101, a row pass then a column pass.  ASSUMED summation order (the one OpenCV's scalar
    RowFilter / ColumnFilter loops use): taps left to right (top to bottom), s = k0 * x0, then s = s + k_i * x_i, every
    product and sum rounded to float32, no fused multiply-add.
  * bilateralFilter(src, 5, sigmaColor, sigmaSpace): OpenCV's bilateralFilter_32f scalar loop (cn == 1).  Radius d / 2,
    the taps (i, j) with sqrt(i^2 + j^2) <= radius in row-major order (13 taps for d = 5), space weights
    (float) exp(r^2 * -0.5 / sigmaSpace^2); the colour weights come from a (4096 + 2)-entry table over the frame's global
    max - min, built in double and stored as float, linearly interpolated; BORDER_REFLECT_101.  ASSUMED summation order:
    per pixel, taps in the order above, wsum += w and sum += val * w in float32 starting from 0, then sum / wsum.  A frame
    whose |max - min| < FLT_EPSILON is returned unchanged.  NaN inputs are not handled (the depth maps hold none).

OpenCV itself cannot be run next to this file, so the fidelity of GaussianBlur and bilateralFilter to a real cv2 build
(which may take SIMD paths with fused multiply-adds, or IPP) is an assumption.  Every other call is a selection.
"""
import math

import numpy as np

MORPH_CLOSE = 3
FLT_MAX = np.float32(np.finfo(np.float32).max)
FLT_EPSILON = float(np.finfo(np.float32).eps)
EXP_BINS = 1 << 12  # kExpNumBinsPerChannel
GAUSS5 = (np.float32(0.0625), np.float32(0.25), np.float32(0.375), np.float32(0.25), np.float32(0.0625))


def _f32(src):
    src = np.asarray(src)
    if src.dtype != np.float32 or src.ndim != 2:
        raise ValueError('the stand-in takes 2-D float32 images, got %s %s' % (src.dtype, src.shape))
    return src


def _taps(kernel):
    """(dy, dx) offsets of the non-zero elements of a kernel, row-major, relative to cv2's default anchor."""
    k = np.asarray(kernel)
    kh, kw = k.shape
    return [(i - kh // 2, j - kw // 2) for i in range(kh) for j in range(kw) if k[i, j]]


def _morph(src, kernel, op, border):
    src = _f32(src)
    h, w = src.shape
    taps = _taps(kernel)
    r = max([max(abs(dy), abs(dx)) for dy, dx in taps] + [0])
    pad = np.full((h + 2 * r, w + 2 * r), border, np.float32)
    pad[r:r + h, r:r + w] = src
    out = np.full((h, w), border, np.float32)
    for dy, dx in taps:
        out = op(out, pad[r + dy:r + dy + h, r + dx:r + dx + w])
    return out


def dilate(src, kernel):
    return _morph(src, kernel, np.maximum, -FLT_MAX)


def erode(src, kernel):
    return _morph(src, kernel, np.minimum, FLT_MAX)


def morphologyEx(src, op, kernel):
    if op != MORPH_CLOSE:
        raise NotImplementedError('only MORPH_CLOSE is restated')
    return erode(dilate(src, kernel), kernel)


def medianBlur(src, ksize):
    src = _f32(src)
    if ksize != 5:
        raise NotImplementedError('only ksize 5 is restated')
    h, w = src.shape
    pad = np.pad(src, 2, mode='edge')
    win = np.stack([pad[dy:dy + h, dx:dx + w] for dy in range(5) for dx in range(5)])
    return np.partition(win, 12, axis=0)[12]


def GaussianBlur(src, ksize, sigma):
    src = _f32(src)
    if tuple(ksize) != (5, 5) or sigma != 0:
        raise NotImplementedError('only ksize (5, 5), sigma 0 is restated')
    h, w = src.shape
    pad = np.pad(src, 2, mode='reflect')  # numpy's 'reflect' is BORDER_REFLECT_101 (gfedcb|abcdefgh|gfedcba)
    rows = GAUSS5[0] * pad[:, 0:w]
    for k in range(1, 5):
        rows = rows + GAUSS5[k] * pad[:, k:k + w]
    out = GAUSS5[0] * rows[0:h]
    for k in range(1, 5):
        out = out + GAUSS5[k] * rows[k:k + h]
    return out


def bilateral_space_taps(d, sigma_space):
    """[(dy, dx, float32 weight)] in the order of OpenCV's tap loop."""
    radius = max(d // 2, 1)
    coeff = -0.5 / (sigma_space * sigma_space)
    taps = []
    for i in range(-radius, radius + 1):
        for j in range(-radius, radius + 1):
            r = math.sqrt(float(i * i) + float(j * j))
            if r > radius:
                continue
            taps.append((i, j, np.float32(math.exp(r * r * coeff))))
    return taps


def bilateral_exp_table(vmin, vmax, sigma_color):
    """The colour-weight table of bilateralFilter_32f: (float32 table (4098,), float32 scale_index)."""
    coeff = -0.5 / (sigma_color * sigma_color)
    length = np.float32(float(vmax) - float(vmin))  # (float)(maxValDst - minValDst) * cn
    scale_index = np.float32(np.float32(EXP_BINS) / length)
    table = np.zeros(EXP_BINS + 2, np.float32)
    last = np.float32(1.0)
    for i in range(EXP_BINS + 2):
        if last > 0:
            val = float(np.float32(np.float32(i) / scale_index))  # int / float in float, then widened to double
            table[i] = np.float32(math.exp(val * val * coeff))
            last = table[i]
    return table, scale_index


def bilateralFilter(src, d, sigma_color, sigma_space):
    src = _f32(src)
    if sigma_color <= 0:
        sigma_color = 1.0
    if sigma_space <= 0:
        sigma_space = 1.0
    vmin, vmax = float(src.min()), float(src.max())
    if abs(vmin - vmax) < FLT_EPSILON:
        return src.copy()
    taps = bilateral_space_taps(d, sigma_space)
    radius = max(d // 2, 1)
    table, scale_index = bilateral_exp_table(vmin, vmax, sigma_color)
    h, w = src.shape
    pad = np.pad(src, radius, mode='reflect')
    s = np.zeros((h, w), np.float32)
    wsum = np.zeros((h, w), np.float32)
    for dy, dx, sw in taps:
        val = pad[radius + dy:radius + dy + h, radius + dx:radius + dx + w]
        alpha = np.abs(val - src) * scale_index
        idx = np.floor(alpha).astype(np.int64)
        alpha = alpha - idx.astype(np.float32)
        wgt = sw * (table[idx] + alpha * (table[idx + 1] - table[idx]))
        wsum = wsum + wgt
        s = s + val * wgt
    return s / wsum
