"""A restatement in numpy of what monopsr_amd/csrc/sample_build.hip computes: Philox4x32-10, the 53-bit uniform, the
Box-Muller pair, the oversampling draw and the 2-D box jitter; and two small oracles written from the description in
DESIGN.md section 7.4, independent of the vectorised code: a scalar jitter loop on Python floats that draws
from np.random as the reference does, and the epoch arithmetic of next_batch as an index state machine.

The restatement is vectorised over slots (trial t of every slot still searching at once); every operation is an
element-wise fp64 +, -, *, /, max, min or a numpy log / sqrt / cos / sin, so a slot's values do not depend on the slots
beside it."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
STREAM_OVERSAMPLE, STREAM_JITTER = 0, 1
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: 4 arrays (or ints) of 32-bit words, key: 2 ints -> 4 uint64 arrays holding 32-bit words."""
    c = [np.asarray(v, np.uint64) & MASK for v in np.broadcast_arrays(*[np.asarray(v, np.uint64) for v in counter])]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]  # 32 x 32 -> 64 bits, no overflow
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1),
             p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c


def seed_key(seed):
    seed = int(seed)
    return seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF


def uniform53(w0, w1):
    return ((w0 >> np.uint64(5)).astype(np.float64) * 67108864.0 + (w1 >> np.uint64(6)).astype(np.float64)) \
        / 9007199254740992.0


def normal_pair(j, s, i, epoch, stream, seed):
    """(z0, z1) of draw j, slot s, frame i."""
    w = philox4x32_10((j, s, i, (int(epoch) << 4) | stream), seed_key(seed))
    u0, u1 = uniform53(w[0], w[1]), uniform53(w[2], w[3])
    r = np.sqrt(-2.0 * np.log(1.0 - u0))
    a = 6.283185307179586 * u1
    return r * np.cos(a), r * np.sin(a)


def oversample_indices(num_objs, num_slots, frame_index, epoch, seed):
    """kitti_dataset.py:301-308 with the counter-based draw: slots < num_objs are the labels in order, the others
    floor(u * num_objs)."""
    s = np.arange(num_slots)
    w = philox4x32_10((0, s, frame_index, (int(epoch) << 4) | STREAM_OVERSAMPLE), seed_key(seed))
    drawn = np.minimum(np.floor(uniform53(w[0], w[1]) * float(num_objs)).astype(np.int64), num_objs - 1)
    return np.where(s < num_objs, s, drawn)


def two_d_iou_pairs(a, b):
    """two_d_iou of box a[k] with box b[k]; (n, 4) x1 y1 x2 y2 fp64 each."""
    w_int = np.minimum(a[:, 2], b[:, 2]) - np.maximum(a[:, 0], b[:, 0])
    h_int = np.minimum(a[:, 3], b[:, 3]) - np.maximum(a[:, 1], b[:, 1])
    non_empty = np.logical_and(w_int > 0, h_int > 0)
    inter = w_int * h_int
    box_area = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    boxes_area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    union = box_area + boxes_area - inter
    iou = np.zeros(len(a))
    iou[non_empty] = inter[non_empty] / union[non_empty]
    return iou


def jitter_boxes(boxes_xyxy, flags, image_hw, frame_index, slot, seed, epoch, iou_threshold_min, max_trials=4096,
                 normals=None, near=1e-9):
    """-> (boxes (n, 4) fp64, trials (n,), near_threshold (n,) bool: some trial's IoU lay within `near` of the
    threshold).  normals(t, active) -> (za, zb, zc, zd) replaces the Philox draws of trial t for the slots `active`."""
    box = np.array(boxes_xyxy, np.float64).reshape(-1, 4)
    n = len(box)
    flags, image_hw = np.asarray(flags).reshape(n), np.asarray(image_hw).reshape(n, 2)
    frame_index, slot = np.asarray(frame_index).reshape(n), np.asarray(slot).reshape(n)
    x1, y1, x2, y2 = box.T
    box_w, box_h = x2 - x1, y2 - y1
    half_w, half_h = box_w / 2, box_h / 2
    cx, cy = (x2 + x1) / 2, (y2 + y1) / 2
    out = box.copy()
    trials = np.zeros(n, np.int64)
    near_thr = np.zeros(n, bool)
    active = np.flatnonzero((flags != 0) & ~((box_w < 10) | (box_h < 10)))
    t = 0
    while len(active) and t < max_trials:
        a = active
        if normals is None:
            za, zb = normal_pair(2 * t, slot[a], frame_index[a], epoch, STREAM_JITTER, seed)
            zc, zd = normal_pair(2 * t + 1, slot[a], frame_index[a], epoch, STREAM_JITTER, seed)
        else:
            za, zb, zc, zd = normals(t, a)
        ncx, ncy = cx[a] + (half_w[a] / 3) * za, cy[a] + (half_h[a] / 3) * zb
        nhw, nhh = half_w[a] + (half_w[a] / 6) * zc, half_h[a] + (half_h[a] / 6) * zd
        new = np.stack([np.maximum(0.0, ncx - nhw), np.maximum(0.0, ncy - nhh),
                        np.minimum((image_hw[a, 1] - 1).astype(np.float64), ncx + nhw),
                        np.minimum((image_hw[a, 0] - 1).astype(np.float64), ncy + nhh)], 1)
        iou = two_d_iou_pairs(new, box[a])
        near_thr[a] |= np.abs(iou - iou_threshold_min) < near
        t += 1
        trials[a] = t
        ok = iou >= iou_threshold_min
        out[a[ok]] = new[ok]
        active = a[~ok]
    trials[active] = max_trials + 1  # the cap: the label's box is kept
    return out, trials, near_thr


def derived_outputs(boxes_xyxy, image_hw, p00_p02):
    """What the kernel derives from the fp64 box: float32 [y1, x1, y2, x2], boxes_2d_norm, est_view_ang."""
    b = np.asarray(boxes_xyxy, np.float64)
    b32 = b[:, [1, 0, 3, 2]].astype(np.float32)
    hw = np.asarray(image_hw).reshape(-1, 2)
    norm = (b32.astype(np.float64) / np.concatenate([hw, hw], 1).astype(np.float64)).astype(np.float32)
    centre = (b32[:, 1] + b32[:, 3]) / np.float32(2)
    p = np.asarray(p00_p02, np.float64).reshape(-1, 2)
    view = np.arctan2((centre.astype(np.float64) - p[:, 1]) / p[:, 0], 1.0).astype(np.float32)
    return b32, norm, view


# ---- oracles written from DESIGN.md section 7.4


def _overlap_ratio(a, b):
    """IoU of two (x1, y1, x2, y2) boxes of Python floats: zero for an empty intersection, and the union summed as
    area(a) + area(b) - intersection, in that order."""
    iw = min(a[2], b[2]) - max(a[0], b[0])
    ih = min(a[3], b[3]) - max(a[1], b[1])
    if not (iw > 0 and ih > 0):
        return 0.0
    both = iw * ih
    return both / ((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - both)


def scalar_jitter(boxes_xyxy, iou_threshold_min, image_hw, normal=None, give_up_after=10 ** 7):
    """The jitter of every box in turn, one box finished before the next begins, on Python floats.  `normal(mean, sd)`
    (default np.random.normal, which returns mean + sd * z) is asked four times per trial, in this order: centre x
    (sd = half width / 3), centre y (half height / 3), half width (sd = half width / 6), half height (half height / 6).
    The trial box is clipped to [0, w - 1] x [0, h - 1]; the first trial whose IoU with the label is not below the
    threshold is kept.  A box narrower or lower than 10 px is returned as it is, with no draw.
    -> ((n, 4) float64 array, list of trials per box)."""
    normal = np.random.normal if normal is None else normal
    rows, last_col = float(image_hw[0] - 1), float(image_hw[1] - 1)
    moved, counts = [], []
    for label in boxes_xyxy:
        left, top, right, bottom = (float(v) for v in label)
        label = (left, top, right, bottom)
        hw, hh = (right - left) / 2, (bottom - top) / 2
        mid_x, mid_y = (right + left) / 2, (bottom + top) / 2
        kept, used = label, 0
        if not (right - left < 10 or bottom - top < 10):
            for used in range(1, give_up_after + 1):
                px, py = float(normal(mid_x, hw / 3)), float(normal(mid_y, hh / 3))
                sx, sy = float(normal(hw, hw / 6)), float(normal(hh, hh / 6))
                trial = (max(0.0, px - sx), max(0.0, py - sy), min(last_col, px + sx), min(rows, py + sy))
                if not _overlap_ratio(trial, label) < iou_threshold_min:
                    kept = trial
                    break
            else:
                raise RuntimeError('no trial accepted')
        moved.append(kept)
        counts.append(used)
    return np.array(moved, np.float64).reshape(-1, 4), counts


class EpochOracle:
    """The epoch arithmetic of next_batch as a cursor over a permuted order: the order is permuted before the very
    first batch and again whenever an epoch ends (both only when asked to shuffle); a batch that reaches or passes the
    end of the order ends the epoch, takes what is left, and continues from the start of the (re-permuted) order; the
    cursor then stands at what it took from there.  A batch larger than the order cannot be served (IndexError)."""

    def __init__(self, total, rng):
        self.total, self.rng = total, rng
        self.order = np.arange(total)
        self.cursor = self.finished = 0

    def _permute(self):
        self.order = self.order[self.rng.permutation(self.total)]

    def take(self, count, reshuffle):
        if reshuffle and self.finished == 0 and self.cursor == 0:
            self._permute()
        first = self.cursor
        if first + count < self.total:
            self.cursor = first + count
            return [int(v) for v in self.order[first:self.cursor]]
        taken = [int(v) for v in self.order[first:]]
        self.finished += 1
        if reshuffle:
            self._permute()
        self.cursor = count - len(taken)
        if self.cursor > self.total:
            raise IndexError('a batch of %d from %d samples' % (count, self.total))
        return taken + [int(v) for v in self.order[:self.cursor]]
