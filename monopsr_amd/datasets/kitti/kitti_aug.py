"""Augmentation of KITTI training samples on the GPU (csrc/sample_build.hip): the 2-D box jitter of the reference's
datasets/kitti/kitti_aug.py:173-254 (jitter_obj_boxes_2d), one lane per box, and its image noise
(apply_image_noise, kitti_aug.py:124-170), one lane per four elements.

The random numbers are counter-based (Philox4x32-10 keyed by `seed`, counted by epoch, frame, slot or element, and
draw), so a box's jitter and a frame's noise depend on those coordinates alone; numpy's global Mersenne-Twister stream,
which the reference draws from, is not reproduced.

    out = jitter_boxes_2d(boxes_xyxy, image_shapes, seed=0, epoch=0, frame_index=fi, slot=s)
    out['boxes_2d']         # (n, 4) float32 [y1, x1, y2, x2]
    labels = jitter_obj_boxes_2d(obj_labels, 0.7, image_shape, seed=0)
    out = apply_image_noise(frames_u8, frame_index=fi, seed=0, epoch=0, mode='reference')
    out['images']           # (F, h, w, 3) float32 holding 0 .. 255
"""
import copy

import numpy as np
import torch

from monopsr_amd import _lib

IMAGE_NOISE_MODES = {'reference': 1, 'composed': 2}  # MPSR_IMAGE_NOISE_*
IMAGE_NOISE_STAGES = ('swap', 'gaussian', 'channel', 'brightness', 'uniform')  # bit k of `stages`
MAX_TRIALS = 4096  # a slot that used this many trials keeps its box and reports MAX_TRIALS + 1 (unreachable at 0.7)


def _device(device):
    return torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)


def _per_slot(a, n, cols, dtype, dev, name, who='jitter_boxes_2d'):
    """A scalar, one row or n rows -> contiguous (n, cols) tensor of dtype on dev."""
    if torch.is_tensor(a):
        t = a.to(device=dev, dtype=dtype)
    else:
        t = torch.as_tensor(np.asarray(a), dtype=dtype, device=dev)
    shape = (n, cols) if cols else (n,)
    if t.numel() == (cols or 1):
        t = t.reshape((1, cols) if cols else (1,)).expand(shape)
    if t.numel() != n * (cols or 1):
        raise _lib.InvalidArgumentError('%s: %s has %d values for %d rows' % (who, name, t.numel(), n))
    return t.reshape(shape).contiguous()


def jitter_boxes_2d(boxes_xyxy, image_shapes, seed, epoch, frame_index, slot, iou_threshold_min=0.7, cam_p=None,
                    jitter_flags=None, max_trials=MAX_TRIALS, write_unjittered=True, out=None, device=None):
    """mpsr_jitter_boxes_2d.  boxes_xyxy (n, 4) fp64 [x1, y1, x2, y2] (the labels' values); image_shapes (h, w) or
    (n, 2); frame_index and slot the RNG coordinates of each box (a scalar or n values); cam_p None (view angles of a
    pinhole at the origin with unit focal length), [P[0][0], P[0][2]] or (n, 2) of them; jitter_flags None (every box)
    or n flags.  -> dict of CUDA tensors: boxes_xyxy (n, 4) fp64, boxes_2d (n, 4) float32 [y1, x1, y2, x2],
    boxes_2d_norm (n, 4), est_view_angs (n,), trials (n,) int32: 0 = left alone (unflagged, or under 10 px wide or
    high), max_trials + 1 = gave up and kept the box.

    `out` is such a dict to write into; with write_unjittered=False the float32 entries of a box that was left alone
    keep what `out` held."""
    dev = _device(device)
    with torch.cuda.device(dev):
        if torch.is_tensor(boxes_xyxy):
            boxes = boxes_xyxy.to(device=dev, dtype=torch.float64).reshape(-1, 4).contiguous()
        else:
            boxes = torch.as_tensor(np.asarray(boxes_xyxy, np.float64).reshape(-1, 4), device=dev).contiguous()
        n = boxes.shape[0]
        hw = _per_slot(image_shapes, n, 2, torch.int32, dev, 'image_shapes')
        p = _per_slot([1.0, 0.0] if cam_p is None else cam_p, n, 2, torch.float64, dev, 'cam_p')
        fi = _per_slot(frame_index, n, 0, torch.int32, dev, 'frame_index')
        sl = _per_slot(slot, n, 0, torch.int32, dev, 'slot')
        flags = _per_slot(1 if jitter_flags is None else jitter_flags, n, 0, torch.int32, dev, 'jitter_flags')
        if out is None:
            if not write_unjittered:
                raise _lib.InvalidArgumentError('jitter_boxes_2d: write_unjittered=False needs `out`')
            out = dict(boxes_xyxy=torch.empty((n, 4), dtype=torch.float64, device=dev),
                       boxes_2d=torch.empty((n, 4), dtype=torch.float32, device=dev),
                       boxes_2d_norm=torch.empty((n, 4), dtype=torch.float32, device=dev),
                       est_view_angs=torch.empty((n,), dtype=torch.float32, device=dev),
                       trials=torch.empty((n,), dtype=torch.int32, device=dev))
        for k, shape, dt in (('boxes_xyxy', (n, 4), torch.float64), ('boxes_2d', (n, 4), torch.float32),
                             ('boxes_2d_norm', (n, 4), torch.float32), ('est_view_angs', (n,), torch.float32),
                             ('trials', (n,), torch.int32)):
            if tuple(out[k].shape) != shape or out[k].dtype != dt:
                raise _lib.InvalidArgumentError('jitter_boxes_2d: out[%r] must be %s %s' % (k, shape, dt))
        _lib.check(_lib.lib().mpsr_jitter_boxes_2d(
            _lib.ptr(boxes), _lib.ptr(flags), _lib.ptr(hw), _lib.ptr(p), _lib.ptr(fi), _lib.ptr(sl), n,
            int(seed) & 0xFFFFFFFFFFFFFFFF, int(epoch), float(iou_threshold_min), int(max_trials),
            int(bool(write_unjittered)), _lib.ptr(out['boxes_xyxy']), _lib.ptr(out['boxes_2d']),
            _lib.ptr(out['boxes_2d_norm']), _lib.ptr(out['est_view_angs']), _lib.ptr(out['trials']), _lib.stream()))
    return out


def jitter_obj_boxes_2d(obj_labels, iou_threshold_min, image_shape, seed=0, epoch=0, frame_index=0, first_slot=0,
                        device=None):
    """The reference's jitter_obj_boxes_2d(obj_labels, iou_threshold_min, image_shape) plus the RNG coordinates: label k
    is slot first_slot + k of frame frame_index.  -> np.ndarray of deep copies of the labels; a jittered copy holds
    the new x1, y1, x2, y2 as Python floats (fp64, as the reference leaves them)."""
    new_objs = np.empty(len(obj_labels), dtype=object)
    new_objs[:] = [copy.deepcopy(o) for o in obj_labels]
    if len(obj_labels) == 0:
        return new_objs
    boxes = np.asarray([[float(o.x1), float(o.y1), float(o.x2), float(o.y2)] for o in obj_labels], np.float64)
    out = jitter_boxes_2d(boxes, image_shape[0:2], seed, epoch, frame_index,
                          first_slot + np.arange(len(obj_labels)), iou_threshold_min, device=device)
    trials = out['trials'].cpu().numpy()
    if (trials > MAX_TRIALS).any():
        raise RuntimeError('jitter_obj_boxes_2d: %d boxes found no jitter in %d trials at IoU >= %g'
                           % (int((trials > MAX_TRIALS).sum()), MAX_TRIALS, iou_threshold_min))
    new = out['boxes_xyxy'].cpu().numpy()
    for o, b, t in zip(new_objs, new, trials):
        if t > 0:
            o.x1, o.y1, o.x2, o.y2 = (float(v) for v in b)
    return new_objs


def image_noise_mode(mode):
    """'reference' / 'composed' -> MPSR_IMAGE_NOISE_*; anything else is a ValueError naming image_noise."""
    try:
        return IMAGE_NOISE_MODES[mode]
    except (KeyError, TypeError):
        raise ValueError("image_noise = %r: choose 'reference' (what the reference's apply_image_noise does: only "
                         "the last stage that fires is seen, and its swap copies B into G) or 'composed' (what it "
                         "describes: the fired stages act one after the other, and the swap exchanges G and B)"
                         % (mode,)) from None


def apply_image_noise(images, frame_index, seed=0, epoch=0, mode='reference', gather=None, device=None):
    """mpsr_image_noise: the reference's apply_image_noise of a batch of frames, with their gather and their conversion
    to float32, in one launch.  images (F, h, w, 3) or (h, w, 3) uint8, a CUDA tensor or a numpy array (float input is
    refused: the arithmetic is uint8 + fp64 noise); gather None (every frame in order) or nb indices into the frames,
    in any order and with repeats; frame_index the RNG coordinate (the frame's index in the split file) of each
    gathered frame, a scalar or nb values.  mode 'reference' or 'composed' (include/monopsr_hip.h).
    -> dict of CUDA tensors: images (nb, h, w, 3) float32 holding 0 .. 255 ((h, w, 3) for a single image without
    gather), stages (nb,) int32, bit k set where IMAGE_NOISE_STAGES[k] fired, and params (nb, 5) fp64: the uniform
    amount, the channel offsets R, G, B and the brightness offset."""
    mode_id = image_noise_mode(mode)
    if not torch.is_tensor(images):
        images = np.asarray(images)
        if images.dtype != np.uint8:
            raise _lib.InvalidArgumentError('apply_image_noise: images must be uint8, got %s' % images.dtype)
        images = torch.from_numpy(np.ascontiguousarray(images))
    if images.dtype != torch.uint8:
        raise _lib.InvalidArgumentError('apply_image_noise: images must be uint8, got %s' % images.dtype)
    single = images.dim() == 3
    if images.dim() not in (3, 4) or images.shape[-1] != 3:
        raise _lib.InvalidArgumentError('apply_image_noise: images must be (F, h, w, 3) or (h, w, 3), got %s'
                                        % (tuple(images.shape),))
    dev = _device(device)
    with torch.cuda.device(dev):
        frames = images.to(dev).reshape((-1,) + tuple(images.shape[-3:])).contiguous()
        n_frames, h, w = frames.shape[0:3]
        if gather is None:
            idx = torch.arange(n_frames, dtype=torch.int32, device=dev)
        else:
            single = False
            if not torch.is_tensor(gather):
                host = np.asarray(gather, np.int64).reshape(-1)
                if len(host) and (host.min() < 0 or host.max() >= n_frames):
                    raise _lib.InvalidArgumentError('apply_image_noise: gather outside [0, %d)' % n_frames)
                gather = torch.as_tensor(host)
            idx = gather.to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
        nb = idx.numel()
        fi = _per_slot(frame_index, nb, 0, torch.int32, dev, 'frame_index', 'apply_image_noise')
        out = dict(images=torch.empty((nb, h, w, 3), dtype=torch.float32, device=dev),
                   stages=torch.empty((nb,), dtype=torch.int32, device=dev),
                   params=torch.empty((nb, 5), dtype=torch.float64, device=dev))
        _lib.check(_lib.lib().mpsr_image_noise(
            _lib.ptr(frames), n_frames, h, w, _lib.ptr(idx), _lib.ptr(fi), nb, int(seed) & 0xFFFFFFFFFFFFFFFF,
            int(epoch), mode_id, _lib.ptr(out['images']), _lib.ptr(out['stages']), _lib.ptr(out['params']),
            _lib.stream()))
        if single:
            out['images'] = out['images'][0]
    return out
