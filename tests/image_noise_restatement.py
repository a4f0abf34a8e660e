"""A restatement in numpy of the image noise of monopsr_amd/csrc/sample_build.hip (mpsr_image_noise), in three parts
that the tests combine:

  apply_stages        the arithmetic alone, in fp64, given which stages fired and their noise;
  philox_draws        the counter-based draws of one (seed, epoch, frame) in the layout of include/monopsr_hip.h, built
                      on jitter_restatement's Philox, uniform53 and normal pair;
  numpy_stream_draws  the same quantities drawn from np.random in the order in which the reference's
                      apply_image_noise (kitti_aug.py:124-170) consumes it, overwritten stages included.

Stages, by bit: 0 swap, 1 Gaussian per element, 2 Gaussian per channel, 3 brightness, 4 uniform per element."""
import numpy as np

import jitter_restatement as jr

SWAP, GAUSSIAN, CHANNEL, BRIGHTNESS, UNIFORM = range(5)
STREAM_IMAGE_FRAME, STREAM_IMAGE_ELEMENT = 2, 3
THRESHOLDS = (0.10, 0.40, 0.40, 0.40, 0.40)
MODES = ('reference', 'composed')
# P(outcome) of the reference's function: the last noise stage that fired, else the swap, else nothing
OUTCOMES = {'uniform': 0.4, 'brightness': 0.6 * 0.4, 'channel': 0.6 * 0.6 * 0.4, 'gaussian': 0.6 ** 3 * 0.4,
            'swap': 0.6 ** 4 * 0.1, 'untouched': 0.6 ** 4 * 0.9}


def outcome(fired):
    """The name in OUTCOMES of a stage bitmask."""
    for bit, name in ((UNIFORM, 'uniform'), (BRIGHTNESS, 'brightness'), (CHANNEL, 'channel'), (GAUSSIAN, 'gaussian'),
                      (SWAP, 'swap')):
        if fired >> bit & 1:
            return name
    return 'untouched'


def _noised(image_u8, noise):
    """np.uint8(np.clip(uint8 + fp64 noise, 0, 255)) -> (the uint8 image, the unclipped fp64 sums)."""
    total = image_u8.astype(np.float64) + noise
    return np.clip(total, 0.0, 255.0).astype(np.uint8), total


def apply_stages(image_u8, fired, gaussian, channel, brightness, uniform_noise, mode, sums=None):
    """image_u8 (h, w, 3) uint8; fired: the bitmask; gaussian, uniform_noise (h, w, 3) fp64; channel (3,) fp64;
    brightness a float (an array is only read where its stage fired, so None serves for the others).
    'reference': the highest noise stage that fired acts on the original; without one, a fired swap sets G := B.
    'composed': every fired stage in order acts on the result of the one before; the swap exchanges G and B.
    `sums`, a list, receives the unclipped fp64 sum of every noise stage that was applied.  -> (h, w, 3) uint8."""
    if mode not in MODES:
        raise ValueError('mode %r' % (mode,))
    image_u8 = np.asarray(image_u8)
    assert image_u8.dtype == np.uint8 and image_u8.ndim == 3 and image_u8.shape[2] == 3
    noise = {GAUSSIAN: gaussian, CHANNEL: None if channel is None else np.asarray(channel, np.float64).reshape(1, 1, 3),
             BRIGHTNESS: None if brightness is None else np.float64(brightness), UNIFORM: uniform_noise}
    stages = [s for s in (GAUSSIAN, CHANNEL, BRIGHTNESS, UNIFORM) if fired >> s & 1]
    out = image_u8.copy()
    if mode == 'reference':
        if stages:
            out, total = _noised(image_u8, noise[stages[-1]])
            if sums is not None:
                sums.append(total)
        elif fired >> SWAP & 1:
            out[:, :, 1] = image_u8[:, :, 2]
        return out
    if fired >> SWAP & 1:
        out = out[:, :, [0, 2, 1]].copy()
    for s in stages:
        out, total = _noised(out, noise[s])
        if sums is not None:
            sums.append(total)
    return out


def _words(c0, c1, split_index, epoch, stream, seed):
    return jr.philox4x32_10((c0, c1, split_index, (int(epoch) << 4) | stream), jr.seed_key(seed))


def frame_draws(seed, epoch, split_index):
    """The per-frame draws (stream 2) -> (fired, params (5,) fp64: amount, channel R, G, B, brightness)."""
    u = []
    for c0 in range(3):
        w = _words(c0, 0, split_index, epoch, STREAM_IMAGE_FRAME, seed)
        u += [float(jr.uniform53(w[0], w[1])), float(jr.uniform53(w[2], w[3]))]
    fired = sum(int(u[s] < THRESHOLDS[s]) << s for s in range(5))
    za, zb = jr.normal_pair(3, 0, split_index, epoch, STREAM_IMAGE_FRAME, seed)
    zc, zd = jr.normal_pair(4, 0, split_index, epoch, STREAM_IMAGE_FRAME, seed)
    params = np.array([10.0 * u[5], float(za) * 8.0, float(zb) * 8.0, float(zc) * 8.0, float(zd) * 15.0], np.float64)
    return fired, params


def fired_of(seed, epochs, split_indices):
    """The stage bitmasks of many coordinates at once (broadcast epochs against split_indices) -> int array."""
    epochs, split_indices = np.broadcast_arrays(np.asarray(epochs, np.uint64), np.asarray(split_indices, np.uint64))
    c3 = (epochs << np.uint64(4)) | np.uint64(STREAM_IMAGE_FRAME)
    u = []
    for c0 in range(3):
        w = jr.philox4x32_10((c0, 0, split_indices, c3), jr.seed_key(seed))
        u += [jr.uniform53(w[0], w[1]), jr.uniform53(w[2], w[3])]
    return sum((u[s] < THRESHOLDS[s]).astype(np.int64) << s for s in range(5))


def philox_draws(seed, epoch, split_index, shape):
    """Everything apply_stages needs for one frame of `shape` (h, w, 3) -> dict(fired, params, gaussian, channel,
    brightness, uniform_noise).  The per-element draws (stream 3): pair q gives elements 2q, 2q + 1 of the frame
    flattened H W C; c1 is the stage's bit."""
    fired, params = frame_draws(seed, epoch, split_index)
    n = int(np.prod(shape))
    q = np.arange((n + 1) // 2)
    za, zb = jr.normal_pair(q, GAUSSIAN, split_index, epoch, STREAM_IMAGE_ELEMENT, seed)
    gaussian = (np.stack([za, zb], 1).reshape(-1)[:n] * 10.0).reshape(shape)
    w = _words(q, UNIFORM, split_index, epoch, STREAM_IMAGE_ELEMENT, seed)
    u = np.stack([jr.uniform53(w[0], w[1]), jr.uniform53(w[2], w[3])], 1).reshape(-1)[:n]
    amount = params[0]
    uniform_noise = (-amount + (2.0 * amount) * u).reshape(shape)
    return dict(fired=fired, params=params, gaussian=gaussian, channel=params[1:4].copy(),
                brightness=float(params[4]), uniform_noise=uniform_noise)


def numpy_stream_draws(shape):
    """The draws of one call of the reference's apply_image_noise from the global np.random, in its order: rand(5); then
    per stage THAT FIRES, whether or not a later one overwrites it, randn(*shape), randn(3), randn(1), and
    uniform(0, 10) followed by uniform(-amount, amount, shape).  -> the dict of philox_draws (None for a stage that did
    not fire)."""
    random_values = np.random.rand(5)
    fired = sum(int(random_values[s] < THRESHOLDS[s]) << s for s in range(5))
    gaussian = channel = brightness = uniform_noise = None
    amount = None
    if fired >> GAUSSIAN & 1:
        gaussian = np.random.randn(*shape) * 10.0
    if fired >> CHANNEL & 1:
        channel = np.random.randn(3) * 8.0
    if fired >> BRIGHTNESS & 1:
        brightness = float((np.random.randn(1) * 15.0)[0])
    if fired >> UNIFORM & 1:
        amount = np.random.uniform(0, 10)
        uniform_noise = np.random.uniform(-amount, amount, shape)
    return dict(fired=fired, amount=amount, gaussian=gaussian, channel=channel, brightness=brightness,
                uniform_noise=uniform_noise)


def restate(image_u8, seed, epoch, split_index, mode, sums=None):
    """apply_stages on philox_draws -> ((h, w, 3) uint8, fired, params)."""
    d = philox_draws(seed, epoch, split_index, image_u8.shape)
    out = apply_stages(image_u8, d['fired'], d['gaussian'], d['channel'], d['brightness'], d['uniform_noise'], mode,
                       sums=sums)
    return out, d['fired'], d['params']


def near_integer(sums, eps=1e-9):
    """Elements whose unclipped fp64 sum, in any applied stage, lies within eps of an integer in [0, 255]: there a
    last-bit difference in log, sqrt, sin or cos can move the truncation by one."""
    mask = None
    for total in sums:
        r = np.rint(total)
        m = (np.abs(total - r) < eps) & (r >= 0) & (r <= 255)
        mask = m if mask is None else mask | m
    return mask
